"""weighted_closest_plane measurements on the MI355X -> profiles/weights_bench1m.json.

The bench's 1M pair (synthetic.make_pair(1_000_000, seed=SEED), bench.py's parameters) with k = 30 normals on both clouds, as the loader
hands them over.  Per built weight function: the weight map alone and the map with weights_sum (the difference is the sequential sum);
then the whole registration and its RANSAC stage (lgr_result.stage_ms[5]) under closest_plane and under weighted_closest_plane with each
weight function.  Times: host clocks around work that ends in a device synchronise, after a warm-up run, median of --reps runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-global-registration_amd"), ROOT):
    sys.path.insert(0, p)

WEIGHTS = ("constant", "curvature", "exp_curvature", "curvedness", "nss")


def timed(fn, sync, reps):
    fn(); sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_bench1m.json"))
    args = ap.parse_args()
    import torch
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    pair = synthetic.make_pair(args.points, seed=synthetic.SEED)
    cl = {}
    for side in ("src", "tgt"):
        d = torch.from_numpy(pair[side]).cuda()
        ctx.normals_knn(d, 30, vp=pair["vp_" + side])
        cl[side] = d
    torch.cuda.synchronize()
    src, tgt = cl["src"], cl["tgt"]
    out = dict(points=args.points, reps=args.reps, weights={}, align={})
    for w in WEIGHTS:
        m_map, _ = timed(lambda: ctx.weights(src, w, with_sum=False), ctx.sync, args.reps)
        m_sum, _ = timed(lambda: ctx.weights(src, w, with_sum=True), ctx.sync, args.reps)
        _, s = ctx.weights(src, w)
        out["weights"][w] = dict(map_ms=m_map, map_and_sum_ms=m_sum, sum_ms=m_sum - m_map, weights_sum=s)
    kw = dict(matching_id=capi.MATCH_LR, score_id=capi.SCORE_MSE, feature_radius=0.25, feature_nr_points=352, normal_nr_points=30,
              bf_block_size=200000, edge_thr_coef=0.95, confidence=0.999, max_iterations=1000000, distance_thr=0.1,
              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    cases = [("closest_plane", capi.METRIC_CLOSEST_PLANE, None)] + [
        ("weighted_closest_plane/" + w, capi.METRIC_WEIGHTED_CLOSEST_PLANE, w) for w in WEIGHTS]
    for name, mid, w in cases:
        p = capi.default_params(metric_id=mid, **kw)
        mp = capi.metric_params(w) if w else None
        res_box = {}

        def run():
            res_box["r"] = ctx.align_ex2(src, tgt, p, mparams=mp)
        ms, _ = timed(run, ctx.sync, args.reps)
        ransac = []
        for _ in range(args.reps):
            run(); ctx.sync(); ransac.append(float(res_box["r"].stage_ms[5]))
        r = res_box["r"]
        T = r.matrix()
        Tg = pair["T_gt"]
        R = T[:3, :3].T @ Tg[:3, :3]
        out["align"][name] = dict(end_to_end_ms=ms, ransac_stage_ms=float(np.median(ransac)), converged=int(r.converged),
                                  iterations=int(r.iterations), n_inliers=int(r.n_inliers), metric=float(r.metric),
                                  rot_err_deg=float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))),
                                  trans_err=float(np.linalg.norm(T[:3, 3] - Tg[:3, 3])))
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
