"""GPU timing of trimmed ICP (lgr_icp_trim_dev) beside the neutral lgr_icp_ex_dev in the same process, by the method of
tools/bench_icp_ex.py: the 1M-point bench pair at the ground truth perturbed by 0.5 degrees about z and 0.3 x density along (0.6, 0, 0.8),
max_dist = 4 x density supplied, eps = 0 so that every iteration runs, events on the context's stream around whole calls of 8 and of 24
iterations; the per-iteration figure is the slope between the two lengths, so the set-up all share is not in it.  One warm-up per
configuration, then --calls timed calls each, the configurations ALTERNATING; medians.  Timed: the neutral lgr_icp_ex_dev (one terms
kernel an iteration: the baseline), keep 0.7, Cauchy at 1.4826 x the median, and both together -- each of the three runs the pair kernel,
the select's passes and the trimmed terms kernel in the terms kernel's place.  

    python tools/bench_icp_trim.py [--points 1000000] [--calls 5] [--out profiles/icp_trim_bench1m.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_trim_bench1m.json"))
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
    base = dict(max_dist=4 * thr, rot_eps=0.0, trans_eps=0.0)
    kinds = {
        "ex_neutral": lambda n: ctx.icp_ex(src, tgt, T0, max_iterations=n, **base),
        "trim_keep_0.7": lambda n: ctx.icp_trim(src, tgt, T0, keep=0.7, max_iterations=n, **base),
        "trim_cauchy_median": lambda n: ctx.icp_trim(src, tgt, T0, robust="cauchy", scale_from_median=1.4826, max_iterations=n, **base),
        "trim_keep_0.7_cauchy_median": lambda n: ctx.icp_trim(src, tgt, T0, keep=0.7, robust="cauchy", scale_from_median=1.4826, max_iterations=n, **base),
    }
    lengths = (8, 24)
    configs = [(f"{k}_{n}", f, n) for k, f in kinds.items() for n in lengths]
    times, last = {k: [] for k, _, _ in configs}, {}
    for k, f, n in configs:   # warm-up: the workspaces grow here
        last[k] = f(n)
        assert last[k].iterations == n and last[k].stop == capi.ICP_STOP_MAX_ITERATIONS, (k, last[k].iterations, last[k].stop)
    ctx.sync()
    for _ in range(a.calls):
        for k, f, n in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(n)
            e1.record()
            e1.synchronize()
            assert r.iterations == n   # the loops are deterministic
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    slope = {k: (med[f"{k}_{lengths[1]}"] - med[f"{k}_{lengths[0]}"]) / (lengths[1] - lengths[0]) for k in kinds}
    # the run-to-run spread of the baseline's own slope: every pairing of a short and a long timed call
    spread = [(b - s) / (lengths[1] - lengths[0]) for s in times[f"ex_neutral_{lengths[0]}"] for b in times[f"ex_neutral_{lengths[1]}"]]
    info = {k: last[f"{k}_{lengths[1]}"].info for k in kinds if k != "ex_neutral"}
    out = {
        "what": "trimmed ICP beside the neutral lgr_icp_ex_dev, ms per iteration as the slope between two call lengths (tools/bench_icp_trim.py)",
        "device": torch.cuda.get_device_name(0), "points": a.points, "density": thr, "max_dist": 4 * thr, "calls": a.calls, "lengths": lengths,
        "select_passes": 4 + sum(1 for s in (24, 16, 8, 0) if (a.points - 1) >> s),
        "ms_per_iteration": slope, "ratio_to_ex_neutral": {k: v / slope["ex_neutral"] for k, v in slope.items()},
        "ex_neutral_slope_min_max_over_call_pairings": [min(spread), max(spread)],
        "call_ms_median": med, "call_ms": times,
        "pairs_first_last": {k: [last[f"{k}_{lengths[1]}"].pairs0, last[f"{k}_{lengths[1]}"].pairs] for k in kinds},
        "rmse_first_last": {k: [last[f"{k}_{lengths[1]}"].rmse0, last[f"{k}_{lengths[1]}"].rmse] for k in kinds},
        "info_first_last": {k: [[s.candidates, s.kept, s.cut, s.scale] for s in (v[0], v[-1])] for k, v in info.items()},
    }
    print(json.dumps(out))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
