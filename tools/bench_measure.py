"""Cost of the measure test type on the bench pair (bench.py's pair and profile: 1M points per cloud, lr matching, uniformity / MSE):

    python tools/bench_measure.py [--points 1000000] [--n-times 10] [--repeats 3] [--sizes 1,8,10,64] [--skip-loops] [--singles-up-to N] [--out profiles/measure_bench1m.json]

Three things are timed, each as the median wall time of --repeats calls (default 3) after one warm-up call, the device drained before and after:
  * lgr_measure_dev with n_times seeds;
  * the loops a caller can write without it, over the same seeds: per seed lgr_align_ex2_dev, then the search and lgr_ransac_ex_dev once more
    for the final mask, then lgr_evaluate_gt_dev ("loop_align"); and the cheaper composition that searches once per seed -- per seed
    lgr_correspondences_ex_dev + lgr_ransac_ex_dev + lgr_evaluate_gt_dev ("loop_composed");
  * lgr_evaluate_gt_batch_dev at n = 1, 8, 10 and 64 transforms against n lgr_evaluate_gt_dev calls.
The runs of lgr_measure_dev are checked against the loop's (transforms by bits, evaluations field by field) before anything is reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--n-times", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--matching", default="lr", choices=["lr", "one_sided", "cluster"])
    ap.add_argument("--sizes", default="1,8,10,64", help="batch sizes of the lgr_evaluate_gt_batch_dev comparison")
    ap.add_argument("--skip-loops", action="store_true", help="time the evaluation comparison only (a single evaluation of a 1M pair takes seconds)")
    ap.add_argument("--singles-up-to", type=int, default=64, metavar="N", help="time the n single calls for batch sizes up to N only (64 of them take minutes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_bench1m.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    pair = synthetic.make_pair(a.points, seed=synthetic.SEED)
    mid = {"lr": capi.MATCH_LR, "cluster": capi.MATCH_CLUSTER, "one_sided": capi.MATCH_ONE_SIDED}[a.matching]
    prm = capi.default_params(matching_id=mid, metric_id=capi.METRIC_UNIFORMITY, score_id=capi.SCORE_MSE, feature_radius=0.25, feature_nr_points=352,
                              normal_nr_points=30, bf_block_size=200000, edge_thr_coef=0.95, confidence=0.999, max_iterations=1000000, distance_thr=0.1,
                              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"], fix_seed=0)
    src = torch.from_numpy(pair["src"]).cuda()
    tgt = torch.from_numpy(pair["tgt"]).cuda()
    for cloud, vp in ((src, pair["vp_src"]), (tgt, pair["vp_tgt"])):   # the analysis reads the clouds' own normals
        ctx.normals_knn(cloud, 30, vp=vp)
    G = pair["T_gt"].astype(np.float32)
    thr = prm.distance_thr
    seeds = [int(prm.seed) + i for i in range(a.n_times)]

    def timed(f, repeats=None, warm=True):
        repeats = repeats or a.repeats
        if warm:
            f()   # warm-up: workspaces grown, code objects loaded
        ms = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), repeats=repeats)

    def with_seed(seed):
        prm.seed = seed
        return prm

    def loop_align():
        out = []
        for s in seeds:
            res = ctx.align_ex2(src, tgt, with_seed(s))
            corr = ctx.correspondences(src, tgt, prm)
            _, mask = ctx.ransac_ex(src, tgt, corr, prm)
            out.append((res, ctx.evaluate_gt(src, tgt, corr, res.matrix(), G, thr, bool(res.converged), mask)))
        return out

    def loop_composed():
        out = []
        for s in seeds:
            corr = ctx.correspondences(src, tgt, with_seed(s))
            res, mask = ctx.ransac_ex(src, tgt, corr, prm)
            out.append((res, ctx.evaluate_gt(src, tgt, corr, res.matrix(), G, thr, bool(res.converged), mask)))
        return out

    def measure():
        return ctx.measure(src, tgt, with_seed(seeds[0]), G, n_times=a.n_times, seeds=seeds)

    # the same answers first
    t = time.perf_counter()
    m, runs = measure()
    ref = [] if a.skip_loops else loop_composed()
    print(f"first calls (cold): {time.perf_counter() - t:.1f} s", flush=True)
    fields = [n for n, _ in capi.GtEval._fields_ if n != "reserved"]
    for r, (res, e) in zip(runs, ref):
        assert np.array_equal(np.asarray(r.result.transformation, np.float32).view(np.uint32), np.asarray(res.transformation, np.float32).view(np.uint32))
        for f in fields:
            x, y = getattr(r.eval, f), getattr(e, f)
            assert x == y or (x != x and y != y), (f, x, y)
    report = dict(points=a.points, n_times=a.n_times, matching=a.matching, device=torch.cuda.get_device_name(0),
                  n_correspondences=runs[0].result.n_correspondences, n_success=m.n_success,
                  search_ms=round(1e3 * runs[0].result.time_cs, 3),
                  ransac_ms_per_run=round(1e3 * statistics.median(r.result.time_te for r in runs), 3),
                  evaluate_gt={})
    for name, f in (() if a.skip_loops else (("measure", measure), ("loop_composed", loop_composed), ("loop_align", loop_align))):
        report[name] = timed(f)
        print(name, report[name], flush=True)
    corr = ctx.correspondences(src, tgt, with_seed(seeds[0]))
    Ts = [r.result.matrix() for r in runs]
    for n in [int(x) for x in a.sizes.split(",")]:
        tn = [Ts[i % len(Ts)] for i in range(n)]
        masks = torch.zeros((n, corr.shape[0]), dtype=torch.uint8, device=src.device)
        masks[:, ::3] = 1
        batch = timed(lambda: ctx.evaluate_gt_batch(src, tgt, corr, tn, G, thr, [True] * n, masks))
        # (the single calls are warm by now; past ten of them one pass is timed: 64 calls are a long enough sample)
        if n > a.singles_up_to:
            report["evaluate_gt"][str(n)] = dict(batch=batch, singles=None, ratio=None)
        else:
            single = timed(lambda: [ctx.evaluate_gt(src, tgt, corr, tn[i], G, thr, True, masks[i]) for i in range(n)], repeats=a.repeats if n <= 10 else 1,
                           warm=n == 1)
            report["evaluate_gt"][str(n)] = dict(batch=batch, singles=single, ratio=round(single["median_ms"] / batch["median_ms"], 2))
        print("evaluate_gt", n, report["evaluate_gt"][str(n)], flush=True)
    if not a.skip_loops:
        report["measure_vs_loop_align"] = round(report["loop_align"]["median_ms"] / report["measure"]["median_ms"], 2)
        report["measure_vs_loop_composed"] = round(report["loop_composed"]["median_ms"] / report["measure"]["median_ms"], 2)
    text = json.dumps(report, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
