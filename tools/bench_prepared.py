"""What a prepared pair saves: four 1M-point clouds of the bench generator (two pairs of lgr_amd.synthetic.make_pair), prepared once,
then the 12 ordered pairs through lgr_align_prepared and the same 12 through lgr_align_dev.

    python tools/bench_prepared.py [--points N] [--passes R] [--configs lr,cluster,multiscale] [--baseline-only] [--out FILE.json]

Per configuration -- FPFH `lr` (the bench configuration), `cluster`, and multi-scale FPFH -- it reports the preparation time per cloud, the
time per pair of both paths, the bytes a prepared cloud holds, the match-stage time (stage_ms[3]: for multi-scale the pair stage with
its merge and vote) and the pair count at which preparing pays.  Every call returns a host result, so a call's wall time is
device-synchronised; one untimed pass over all pairs warms the workspace up, then --passes timed passes; the per-pass means give the
spread.  --baseline-only times lgr_align_dev alone: that form also runs on a build without the prepared entry points, which is how
the parent commit's numbers in profiles/prepared_bench1m.json were taken."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def params_of(capi, config, vp_src, vp_tgt):
    kw = dict(metric_id=capi.METRIC_UNIFORMITY, score_id=capi.SCORE_MSE, feature_radius=0.25, feature_nr_points=352, normal_nr_points=30,
              bf_block_size=200000, edge_thr_coef=0.95, confidence=0.999, max_iterations=1000000, distance_thr=0.1, vp_src=vp_src, vp_tgt=vp_tgt)
    if config == "lr":
        kw["matching_id"] = capi.MATCH_LR
    elif config == "cluster":
        kw["matching_id"] = capi.MATCH_CLUSTER
    else:   # multi-scale: feature_radius unset; the vote needs the radii
        kw.update(matching_id=capi.MATCH_LR, feature_radius=0.0, iss_radius_src=0.05, iss_radius_tgt=0.05)
    return capi.default_params(**kw)


def summary(per_pass):
    """per_pass[r][i]: seconds of pair i in pass r -> ms: mean over pairs of the per-pair medians, and the spread of the per-pass means"""
    n = len(per_pass[0])
    med = [statistics.median(p[i] for p in per_pass) for i in range(n)]
    means = [1e3 * sum(p) / n for p in per_pass]
    return dict(ms_per_pair=1e3 * sum(med) / n, pass_means_ms=means, spread_ms=max(means) - min(means))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--configs", default="lr,cluster,multiscale")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    clouds, vps = [], []
    for k in range(2):
        pair = synthetic.make_pair(a.points, seed=synthetic.SEED + k)
        clouds += [torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()]
        vps += [pair["vp_src"], pair["vp_tgt"]]
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    out = dict(points=a.points, passes=a.passes, pairs=len(pairs), device=torch.cuda.get_device_name(0), configs={})
    for config in a.configs.split(","):
        prm = {(i, j): params_of(capi, config, vps[i], vps[j]) for i, j in pairs}
        rec = {}

        def run(fn):
            per_pass, match_ms = [], []
            for r in range(a.passes + 1):
                times = []
                for i, j in pairs:
                    t = time.perf_counter()
                    res = fn(i, j)
                    times.append(time.perf_counter() - t)
                    if r:
                        match_ms.append(res.stage_ms[3])
                if r:     # pass 0 is the warm-up
                    per_pass.append(times)
            s = summary(per_pass)
            s["match_stage_ms"] = sum(match_ms) / len(match_ms)
            return s

        rec["unprepared"] = run(lambda i, j: ctx.align(clouds[i], clouds[j], prm[(i, j)]))
        if not a.baseline_only:
            prep_s, prepared = [], [None] * 4
            for r in range(a.passes + 1):
                for i in range(4):
                    if prepared[i] is not None:
                        prepared[i].close()
                    t = time.perf_counter()
                    prepared[i] = ctx.prepare_cloud(clouds[i], prm[(i, (i + 1) % 4)], 0)
                    if r:
                        prep_s.append(time.perf_counter() - t)
            rec["prepare_ms_per_cloud"] = 1e3 * statistics.median(prep_s)
            rec["prepare_ms_min_max"] = [1e3 * min(prep_s), 1e3 * max(prep_s)]
            rec["bytes_per_cloud"] = [int(c.info().bytes) for c in prepared]
            rec["prepared"] = run(lambda i, j: ctx.align_prepared(prepared[i], prepared[j], prm[(i, j)]))
            saved = rec["unprepared"]["ms_per_pair"] - rec["prepared"]["ms_per_pair"]
            # N clouds, every ordered pair: N prepare + N (N - 1) prepared pairs against N (N - 1) unprepared pairs
            rec["saved_ms_per_pair"] = saved
            rec["pairs_per_cloud_to_break_even"] = rec["prepare_ms_per_cloud"] / saved if saved > 0 else None
            for c in prepared:
                c.close()
        out["configs"][config] = rec
        print(config, json.dumps(rec), flush=True)
    if not a.baseline_only:
        sizes = {}
        p = params_of(capi, "lr", vps[0], vps[1])
        for d in ("fpfh", "shot", "rops"):
            with ctx.prepare_cloud(clouds[0], p, 0, capi.feature_params(d, lrf_id=capi.LRF_GRAVITY if d == "rops" else None)) as c:
                sizes[d] = int(c.info().bytes)
        out["bytes_single_scale_by_descriptor"] = sizes
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
