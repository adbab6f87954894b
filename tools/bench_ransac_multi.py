"""What the set of distinct hypotheses costs on one MI355X:

    python tools/bench_ransac_multi.py [--repeats 15] [--warmup 3] [--out profiles/ransac_multi.json]

  * lgr_ransac_multi_dev against lgr_ransac_dev from the same build on the same input, the two calls alternating in one process
    (a host clock around calls that end in a device synchronise), on the single-mode correspondence problem (20000 points, 6000
    correspondences, 40 % inliers, seed 3) and on the two-mode problem scaled to 6000 correspondences;
  * the same pair under closest_plane and combination (unit normals drawn on both clouds): lgr_ransac_multi_ex_dev against
    lgr_ransac_ex_dev, max_set = LGR_HYPOTHESES_MAX (a set that outgrows it is recorded as such, not timed);
  * the fold alone (lgr_fold_hypotheses_dev: the fold kernel, a gather of the set and a 16-byte read-back) on the three generated pose
    lists, as device-event time per item.

Median, minimum and maximum over the repeats are written; nothing is asserted.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_multi.json"))
    ap.add_argument("--metrics", type=int, nargs="+", default=[1, 0, 2, 3], help="metric ids of the problem rows (lgr.h: LGR_METRIC_*)")
    ap.add_argument("--no-fold", action="store_true", help="skip the rows of the fold alone")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_ransac_multi needs the MI355X"
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, warmup=a.warmup, problems=[], fold=[])

    problems = [("single_mode_20000_6000_0.4_seed3", synthetic.make_correspondence_problem(20000, 6000, 0.4, seed=3)),
                ("two_mode_16000_6000_0.30_0.18_seed11", synthetic.make_two_mode_problem(n_pts=16000, c=6000, f1=0.30, f2=0.18, seed=11))]
    names = {capi.METRIC_UNIFORMITY: "uniformity", capi.METRIC_CORRESPONDENCES: "correspondences", capi.METRIC_CLOSEST_PLANE: "closest_plane",
             capi.METRIC_COMBINATION: "combination"}
    for name, prob in problems:
        rng = np.random.default_rng(77)   # unit normals for the plane metrics (the generators leave them empty)
        for side in ("src", "tgt"):
            nrm = rng.normal(size=(prob[side].shape[0], 3))
            prob[side][:, 4:7] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        src, tgt = torch.from_numpy(prob["src"]).cuda(), torch.from_numpy(prob["tgt"]).cuda()
        corr = ctx._corr_dev(prob["corr"])
        for metric in a.metrics:
            planar = metric in (capi.METRIC_CLOSEST_PLANE, capi.METRIC_COMBINATION)
            p = capi.default_params(metric_id=metric, score_id=capi.SCORE_MSE, distance_thr=0.05, max_iterations=100000, ransac_batch=4096)
            t_single, t_multi = [], []
            try:
                for it in range(a.warmup + a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res, _ = ctx.ransac_ex(src, tgt, corr, p) if planar else ctx.ransac(src, tgt, corr, p)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if planar:
                        mres, hyps, best = ctx.ransac_multi_ex(src, tgt, corr, p, max_set=capi.HYPOTHESES_MAX)
                    else:
                        mres, hyps, best = ctx.ransac_multi(src, tgt, corr, p, max_set=256)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if it >= a.warmup:
                        t_single.append(1e3 * (t1 - t0)); t_multi.append(1e3 * (t2 - t1))
            except capi.LgrError as e:
                if f"rc={capi.ERR_UNSUPPORTED}" not in str(e):
                    raise
                row = dict(problem=name, metric=names[metric], outgrew_max_set=capi.HYPOTHESES_MAX)
                out["problems"].append(row)
                print(json.dumps(row))
                continue
            assert mres.iterations == res.iterations
            row = dict(problem=name, metric=names[metric], iterations=res.iterations,
                       members=len(hyps), best_index=best, ransac_ms=spread(t_single), ransac_multi_ms=spread(t_multi),
                       ratio_of_medians=statistics.median(t_multi) / statistics.median(t_single))
            out["problems"].append(row)
            print(json.dumps(row))

    for n, k, seed in (() if a.no_fold else ((3000, 12, 1), (3000, 40, 2), (500, 3, 3))):
        tns, met = synthetic.make_pose_list(n, k, seed)
        dT, dM = torch.from_numpy(tns).cuda(), torch.from_numpy(met).cuda()
        us = []
        members = 0
        for it in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            T, m, idx = ctx.fold_hypotheses(dT, dM, 0.05, capi.HYPOTHESES_MAX)
            e1.record()
            torch.cuda.synchronize()
            members = len(m)
            if it >= a.warmup:
                us.append(1e3 * e0.elapsed_time(e1) / n)
        row = dict(items=n, centres=k, seed=seed, members=members, us_per_item=spread(us))
        out["fold"].append(row)
        print(json.dumps(row))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
