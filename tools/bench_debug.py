"""GPU timing of the debug layer on the 1M-point bench pair: lgr_temperature_maps_dev at the ground truth,
lgr_compare_overlaps_dev for one transformation at the ground truth, and the same call for a transformation that moves the source ten cloud
extents away.  The near call of the same run is the yardstick for the far one: the search's cost must not grow with the separation.  Every
figure is the median of five individually timed calls after a warm-up, each call ended by a device synchronise.

    python tools/bench_debug.py [--points 1000000] [--out profiles/debug_bench1m.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debug_bench1m.json"))
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
    thr = float(np.float32(2 * ctx.cloud_density(tgt)))
    ext = float((tgt[:, :3].max(0).values - tgt[:, :3].min(0).values).max())
    far = np.eye(4)
    far[:3, 3] = 10 * ext * np.array([0.6, -0.64, 0.48])
    far = (far @ G.astype(np.float64)).astype(np.float32)
    out = dict(points=a.points, device=torch.cuda.get_device_name(0), calls_per_figure=5, figure="median of individually timed calls, ms",
               distance_thr=thr, extent=ext)
    # the far search first, once and alone: should its cost depend on the separation after all, this is where the run stops
    t = time.perf_counter()
    q = ctx.temperature_maps(src[:4096], tgt[:1], far, thr)["moved"]
    ctx.nearest(q, tgt)
    ctx.sync(); torch.cuda.synchronize()
    out["far_nearest_4096_queries_first_call_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    assert out["far_nearest_4096_queries_first_call_ms"] < 5000, out
    ms, all_ms, m = timed(lambda: ctx.temperature_maps(src, tgt, G, thr))
    out["temperature_maps_ms"] = dict(median=round(ms, 3), calls=all_ms, note="includes the copies of ten per-point arrays to the host")
    out.update(n_below_src=m["src"]["n_below"], n_below_tgt=m["tgt"]["n_below"])
    ms, all_ms, o = timed(lambda: ctx.compare_overlaps(src, tgt, [G], thr, with_masks=False))
    out["compare_overlaps_gt_ms"] = dict(median=round(ms, 3), calls=all_ms)
    out.update(overlap_count_gt=int(o["counts"][0]), weighted_count_gt=float(o["weighted"][0]))
    ms, all_ms, o = timed(lambda: ctx.compare_overlaps(src, tgt, [far], thr, with_masks=False))
    out["compare_overlaps_far_ms"] = dict(median=round(ms, 3), calls=all_ms)
    out.update(overlap_count_far=int(o["counts"][0]))
    ms, all_ms, _ = timed(lambda: ctx.nearest(m["moved"], tgt))
    out["nearest_gt_ms"] = dict(median=round(ms, 3), calls=all_ms)
    ms, all_ms, _ = timed(lambda: ctx.knn(m["moved"], tgt, 1))
    out["knn1_gt_ms"] = dict(median=round(ms, 3), calls=all_ms, note="lgr_knn_dev, k = 1: the ring search on the same queries")
    out["far_over_gt"] = round(out["compare_overlaps_far_ms"]["median"] / out["compare_overlaps_gt_ms"]["median"], 3)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
