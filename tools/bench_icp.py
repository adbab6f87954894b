"""GPU timing of the point-to-plane ICP (lgr_icp_plane_dev) on the 1M-point bench pair at the perturbed ground truth of tools/bench_refine.py
(0.5 degrees about z, 0.3 x density along (0.6, 0, 0.8)) -- beside lgr_refine_plane_dev's step on the same clouds in the same run.
Both loops are timed with events on the context's stream around whole calls at two lengths (ICP: 8 and 24 iterations with the stop rule
switched off by eps = 0; refinement: 2 and 10 steps, MSE score); the per-iteration figure is the slope between the two lengths, so the
set-up both share (the grid over the target, the buffers) is not in it; the whole-call times are reported next to it.  One warm-up per
configuration, then five timed calls each, the configurations ALTERNATING; medians.  The distances are supplied (max_dist = 4 x density,
threshold = density), so neither loop computes the density.  

    python tools/bench_icp.py [--points 1000000] [--calls 5] [--out profiles/icp_bench1m.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench1m.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgr_amd import capi, synthetic
    assert torch.cuda.is_available(), "this is a GPU measurement: there is no CPU figure to fall back to"
    ctx = capi.Context(0)
    F = np.float32

    pair = synthetic.make_pair(a.points, seed=synthetic.SEED)   # the bench pair of rank 0
    src, tgt = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    ctx.normals_knn(src, 30, vp=pair["vp_src"])
    ctx.normals_knn(tgt, 30, vp=pair["vp_tgt"])
    thr = float(F(ctx.cloud_density(tgt)))
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    T0 = (dT @ pair["T_gt"]).astype(F)

    def icp(n):
        r = ctx.icp_plane(src, tgt, T0, max_iterations=n, max_dist=4 * thr, rot_eps=0.0, trans_eps=0.0)
        assert r.iterations == n and r.stop == capi.ICP_STOP_MAX_ITERATIONS, (r.iterations, r.stop)
        return r.iterations, r

    def refine(n):
        r = ctx.refine_plane(src, tgt, T0, capi.SCORE_MSE, n, threshold=thr, trace=True)
        return len(r.trace) - 1, r   # candidates evaluated

    configs = [("icp_8", icp, 8), ("icp_24", icp, 24), ("refine_2", refine, 2), ("refine_10", refine, 10)]
    times, counts, last = {k: [] for k, _, _ in configs}, {}, {}
    for k, f, n in configs:   # warm-up: the workspaces grow here
        counts[k], last[k] = f(n)
    ctx.sync()
    for _ in range(a.calls):
        for k, f, n in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c, _ = f(n)
            e1.record()
            e1.synchronize()
            assert c == counts[k]   # the loops are deterministic
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    icp_ms = (med["icp_24"] - med["icp_8"]) / (counts["icp_24"] - counts["icp_8"])
    d_ref = counts["refine_10"] - counts["refine_2"]
    refine_ms = (med["refine_10"] - med["refine_2"]) / d_ref if d_ref > 0 else None
    r = last["icp_24"]
    out = {
        "what": "point-to-plane ICP beside the closest-plane refinement, ms per iteration / step as the slope between two call lengths (tools/bench_icp.py)",
        "device": torch.cuda.get_device_name(0), "points": a.points, "density": thr, "max_dist": 4 * thr, "calls": a.calls,
        "icp_ms_per_iteration": icp_ms, "refine_ms_per_step": refine_ms,
        "call_ms_median": med, "call_ms": times, "evaluated": counts,
        "icp_pairs_first_last": [r.pairs0, r.pairs], "icp_rmse_first_last": [r.rmse0, r.rmse],
        "refine_steps_stop": [last["refine_10"].steps, last["refine_10"].stop],
    }
    print(json.dumps(out))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
