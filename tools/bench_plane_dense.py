"""GPU timing of the dense closest-plane evaluation (lgr_evaluate_plane_dense_dev) on the 1M-point bench pair at its ground truth, beside
lgr_overlap_rmse_dev on the same pair in the same process -- the pass that walks the same grid over the same points and ends in the same
sequential-sum kernel.  Every figure is the median of five individually timed calls after a warm-up, each call
ended by a device synchronise.

    python tools/bench_plane_dense.py [--points 1000000] [--out profiles/plane_dense_bench1m.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_dense_bench1m.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgr_amd import capi, synthetic
    assert torch.cuda.is_available(), "this is a GPU measurement: there is no CPU figure to fall back to"
    ctx = capi.Context(0)

    def timed(f, n=5):
        f(); ctx.sync(); torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t = time.perf_counter()
            r = f()
            ctx.sync(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return sorted(ts)[len(ts) // 2], [round(x, 3) for x in ts], r

    pair = synthetic.make_pair(a.points, seed=synthetic.SEED)   # the bench pair of rank 0
    src, tgt = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    ctx.normals_knn(src, 30, vp=pair["vp_src"])
    ctx.normals_knn(tgt, 30, vp=pair["vp_tgt"])
    G = pair["T_gt"].astype(np.float32)
    out = dict(points=a.points, device=torch.cuda.get_device_name(0), calls_per_figure=5, figure="median of individually timed calls, ms")
    ms, all_ms, thr = timed(lambda: ctx.cloud_density(tgt))
    out["cloud_density_ms"] = dict(median=round(ms, 3), calls=all_ms)
    thr = float(np.float32(thr))
    ms, all_ms, d = timed(lambda: ctx.evaluate_plane_dense(src, tgt, G, capi.SCORE_MSE))
    out["dense_threshold_computed_ms"] = dict(median=round(ms, 3), calls=all_ms)
    out.update(n_inliers=d.n_inliers, rmse=d.rmse, metric=d.metric, threshold=d.threshold)
    ms, all_ms, d2 = timed(lambda: ctx.evaluate_plane_dense(src, tgt, G, capi.SCORE_MSE, threshold=thr))
    out["dense_threshold_supplied_ms"] = dict(median=round(ms, 3), calls=all_ms)
    assert (d2.n_inliers, d2.rmse, d2.metric) == (d.n_inliers, d.rmse, d.metric)
    # with the inlier list and the nearest-target array: the scan, the compaction and two device-to-host copies on top
    ms, all_ms, _ = timed(lambda: ctx.evaluate_plane_dense(src, tgt, G, capi.SCORE_MSE, threshold=thr, with_inliers=True, with_nn=True))
    out["dense_threshold_supplied_with_lists_ms"] = dict(median=round(ms, 3), calls=all_ms)
    ms, all_ms, r = timed(lambda: ctx.overlap_rmse(src, tgt, G, G, thr))
    out["overlap_rmse_ms"] = dict(median=round(ms, 3), calls=all_ms, note="distance_thr = the plane threshold: the same grid cell and radius; includes the copy of its index array to the host")
    out.update(overlap_size=r[1], overlap_rmse=r[0])
    out["dense_supplied_over_overlap"] = round(out["dense_threshold_supplied_ms"]["median"] / out["overlap_rmse_ms"]["median"], 3)
    out["dense_computed_over_overlap"] = round(out["dense_threshold_computed_ms"]["median"] / out["overlap_rmse_ms"]["median"], 3)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
