"""RoPS stage measurements on the MI355X -> profiles/rops_<case>.json (one file per case).

Cases: the bench generator's 1M pair moved by a pure yaw (synthetic.make_pair(yaw_only=True)) with ISS key points -- the gravity-frame
stage and the RoPS stage of the source cloud next to the SHOT stage on the same key points, and the whole registration with rops +
gravity next to SHOT and FPFH -- and a dense 50k x 50k 135-d matcher case.  Times: host clocks around work that ends in a device
synchronise, after a warm-up run of the same shapes, median of --reps runs.  Matcher FLOPs: 3 per element (sub, mul, add) x 135 x
rows_a x rows_b (an exact VALU scan, no MFMA)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-global-registration_amd"), ROOT):
    sys.path.insert(0, p)

F16_PEAK_TFLOPS = 2516.8      # MI355X_MICROARCH.md: BF16/FP16 MFMA ~2.5 PF dense (bench.py's constant)
F32_VECTOR_PEAK_TFLOPS = 157.3  # spec: FP32 vector (packed) peak


def timed(fn, sync, reps):
    fn(); sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), ts


def match_case(ctx, ma, mb, reps, rng):
    import torch
    a = rng.normal(size=(ma, 135)).astype(np.float32)
    b = rng.normal(size=(mb, 135)).astype(np.float32)
    a /= np.abs(a).sum(1, keepdims=True); b /= np.abs(b).sum(1, keepdims=True)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ms, all_ms = timed(lambda: ctx.match2_rops(ta, tb, 200000), ctx.sync, reps)
    flops = 3.0 * 135 * ma * mb
    tf = flops / (ms * 1e-3) / 1e12
    return dict(rows_a=ma, rows_b=mb, match2_ms=ms, match2_ms_all=all_ms, flops=flops, achieved_tflops=tf,
                frac_f16_dense_peak=tf / F16_PEAK_TFLOPS, frac_f32_vector_peak=tf / F32_VECTOR_PEAK_TFLOPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="bench1m,match50k")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_rops.py measures the MI355X; there is no CPU fallback"
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    rng = np.random.default_rng(0)
    os.makedirs(args.out, exist_ok=True)
    cases = args.cases.split(",")
    if "bench1m" in cases:
        pair = synthetic.make_pair(1_000_000, seed=synthetic.SEED, yaw_only=True)
        s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
        kw = dict(matching_id=capi.MATCH_LR, bf_block_size=200000, distance_thr=0.1, keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06,
                  iss_radius_tgt=0.06, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
        p = capi.default_params(**kw)
        runs = {}
        for name in ("rops", "shot", "fpfh"):
            ms, all_ms = timed(lambda: ctx.align(s, t, p, descriptor=name), ctx.sync, args.reps)
            r = ctx.align(s, t, p, descriptor=name)
            G = pair["T_gt"]
            R = r.matrix()[:3, :3].astype(np.float64) @ G[:3, :3].T
            runs[name] = dict(end_to_end_ms=ms, end_to_end_ms_all=all_ms, n_correspondences=r.n_correspondences, n_inliers=r.n_inliers,
                              converged=r.converged, rot_err_deg=float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))),
                              trans_err=float(np.linalg.norm(r.matrix()[:3, 3] - G[:3, 3])),
                              stage_ms=dict(zip(["downsample", "normals", "descriptor", "match", "filter", "align"], list(r.stage_ms)[:6])))
        # the stages alone on the source cloud: ISS key points of the normals-estimated cloud, at the multi-scale radius rule
        ctx.normals_knn(s, 30, vp=pair["vp_src"])
        idx = ctx.iss_keypoints(s, 0.06).long()
        kps = s[idx].contiguous()
        dens = ctx.cloud_density(s)
        radius = float(np.sqrt(352 * dens * dens / np.pi))
        fr = ctx.gravity_lrf(kps, s, radius)
        gravity_ms, _ = timed(lambda: ctx.gravity_lrf(kps, s, radius), ctx.sync, args.reps)
        rops_ms, _ = timed(lambda: ctx.rops(kps, s, radius, fr), ctx.sync, args.reps)
        shot_ms, _ = timed(lambda: ctx.shot(kps, s, radius), ctx.sync, args.reps)
        shot_fr = ctx.shot_lrf(kps, s, radius)
        shot_given_ms, _ = timed(lambda: ctx.shot(kps, s, radius, lrf=shot_fr), ctx.sync, args.reps)
        n_shot = int(torch.isnan(fr[:, 0]).sum().item())
        out = dict(case="bench generator 1M pair, yaw-only motion, ISS key points (0.06), lr, RANSAC", runs=runs,
                   n_keypoints_src=int(kps.shape[0]), stage_radius=radius, gravity_lrf_stage_ms=gravity_ms, rops_stage_ms=rops_ms,
                   shot_stage_ms_with_lrf=shot_ms, shot_stage_ms_given_lrf=shot_given_ms, nan_gravity_frames=n_shot,
                   matcher=match_case(ctx, int(kps.shape[0]), int(kps.shape[0]), args.reps, rng))
        json.dump(out, open(os.path.join(args.out, "rops_bench1m.json"), "w"), indent=1)
        print(json.dumps(out))
    if "match50k" in cases:
        out = dict(case="dense 135-d matcher 50k x 50k, both directions", **match_case(ctx, 50_000, 50_000, args.reps, rng))
        json.dump(out, open(os.path.join(args.out, "rops_match50k.json"), "w"), indent=1)
        print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
