"""What the TEASER alignment costs on one MI355X, beside GROR and RANSAC on the same correspondences:

    python tools/bench_teaser.py [--repeats 11] [--warmup 2] [--points 1000000] [--out profiles/teaser.json]

  * inputs: the correspondences of the bench pair (bench.py's profile on synthetic.make_pair(points), matching lr) and the
    correspondence problem make_correspondence_problem(n_pts = 250000, c = 200000, inlier_frac = 0.4);
  * lgr_teaser_dev at k_select 1024 and 2048 with the reference's commented parameters (noise bound = distance_thr), then lgr_gror_dev
    (K = 800) and lgr_ransac_dev (the bench profile) from the same build, the calls alternating in one process: a host clock around calls
    that end in a device synchronise, and for TEASER the six stage times of lgr_result.stage_ms (device events);
  * every result's rotation error (the angle of R^T R_gt, radians) and translation error against the generator's ground truth.

Median, minimum and maximum over the repeats are written; nothing is asserted.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))

STAGES = ("nodes", "adjacency", "clique", "rotation", "translation", "mask")


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def errors(np, T, T_gt):
    R = T[:3, :3].astype(np.float64).T @ T_gt[:3, :3]
    return dict(r_err=float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))), t_err=float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=1_000_000, help="points per cloud of the bench pair")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teaser.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_teaser needs the MI355X"
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, warmup=a.warmup, inputs=[])

    pair = synthetic.make_pair(a.points, seed=synthetic.SEED)
    p_bench = capi.default_params(matching_id=capi.MATCH_LR, metric_id=capi.METRIC_UNIFORMITY, score_id=capi.SCORE_MSE, feature_radius=0.25,
                                  feature_nr_points=352, normal_nr_points=30, bf_block_size=200000, edge_thr_coef=0.95, confidence=0.999,
                                  max_iterations=1000000, distance_thr=0.1, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    src, tgt = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    inputs = [(f"bench_pair_{a.points}", src, tgt, ctx.correspondences(src, tgt, p_bench).clone(), pair["T_gt"], 0.1)]
    prob = synthetic.make_correspondence_problem(n_pts=250000, c=200000, inlier_frac=0.4)
    inputs.append(("problem_250000_200000_0.4", torch.from_numpy(prob["src"]).cuda(), torch.from_numpy(prob["tgt"]).cuda(),
                   ctx._corr_dev(prob["corr"]), prob["T_gt"], 0.05))

    for name, s, t, corr, T_gt, thr in inputs:
        p = capi.default_params(metric_id=capi.METRIC_UNIFORMITY, score_id=capi.SCORE_MSE, distance_thr=thr, max_iterations=1000000)
        calls = [("teaser_1024", lambda: ctx.teaser(s, t, corr, capi.default_teaser_params(thr, k_select=1024))),
                 ("teaser_2048", lambda: ctx.teaser(s, t, corr, capi.default_teaser_params(thr, k_select=2048))),
                 ("gror_800", lambda: ctx.gror(s, t, corr, thr)),
                 ("ransac", lambda: ctx.ransac(s, t, corr, p))]
        ms = {k: [] for k, _ in calls}
        stage = {k: [[] for _ in STAGES] for k, _ in calls if k.startswith("teaser")}
        last = {}
        for it in range(a.warmup + a.repeats):
            for k, f in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms[k].append(1e3 * (time.perf_counter() - t0))
                    if k in stage:
                        for j in range(len(STAGES)):
                            stage[k][j].append(float(r[0].stage_ms[j]))
                last[k] = r
        row = dict(input=name, correspondences=int(corr.shape[0]), distance_thr=thr, calls={})
        for k, _ in calls:
            res = last[k][0]
            d = dict(ms=spread(ms[k]), converged=int(res.converged), n_inliers=int(res.n_inliers), iterations=int(res.iterations),
                     **errors(np, res.matrix(), T_gt))
            if k in stage:
                info = last[k][1]
                d["stage_ms"] = {STAGES[j]: spread(stage[k][j]) for j in range(len(STAGES))}
                d["info"] = {f: getattr(info, f) for f in ("valid", "n_nodes", "max_core", "n_core", "n_clique", "rotation_iterations",
                                                            "n_rotation_inliers", "n_translation_inliers", "rotation_cost")}
            row["calls"][k] = d
        out["inputs"].append(row)
        print(json.dumps(row))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
