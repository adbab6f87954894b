"""SHOT stage measurements on the MI355X -> profiles/shot_<case>.json (one file per case).

Cases: the acceptance corner scene (tests/test_gpu_reference_acceptance.py, multi-scale, cluster, closest_plane, SHOT end to end), the
bench generator's 1M pair with ISS key points (LRF and SHOT stage of each cloud, both-direction matcher, end to end), and a dense
50k x 50k matcher case.  Times: hipEvent-free host clocks around work that ends in a device synchronise, after a warm-up run of the same
shapes, median of --reps runs.  The matcher FLOPs are counted as the canonical distance needs them: 3 per element (sub, mul, add) x 352
x rows_a x rows_b; the kernel is an exact VALU scan (no MFMA), its rate is reported against the f16 MFMA dense peak as well as the f32
vector peak."""
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
    a = rng.random((ma, 352), dtype=np.float32) ** 4
    b = rng.random((mb, 352), dtype=np.float32) ** 4
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ms, all_ms = timed(lambda: ctx.match2_shot(ta, tb, 200000), ctx.sync, reps)
    flops = 3.0 * 352 * ma * mb
    tf = flops / (ms * 1e-3) / 1e12
    return dict(rows_a=ma, rows_b=mb, match2_ms=ms, match2_ms_all=all_ms, flops=flops, achieved_tflops=tf,
                frac_f16_dense_peak=tf / F16_PEAK_TFLOPS, frac_f32_vector_peak=tf / F32_VECTOR_PEAK_TFLOPS,
                candidates="none: exact dense scan (no filter, no rerank)", fallbacks=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="corner,bench1m,match50k")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_shot.py measures the MI355X; there is no CPU fallback"
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    rng = np.random.default_rng(0)
    os.makedirs(args.out, exist_ok=True)
    cases = args.cases.split(",")
    if "corner" in cases:
        src, tgt, vp_src, vp_tgt = synthetic.make_corner_scene()
        s = ctx.normals_knn(torch.from_numpy(src).cuda(), 30, vp=vp_src)
        t = ctx.normals_knn(torch.from_numpy(tgt).cuda(), 30, vp=vp_tgt)
        # the reference test's parameters (point2plane_distance.cpp:69-80) over the struct defaults: cluster, mse, multi-scale
        p = capi.default_params(matching_id=capi.MATCH_CLUSTER, metric_id=capi.METRIC_CLOSEST_PLANE, score_id=capi.SCORE_MSE,
                                bf_block_size=200000, max_iterations=10000, distance_thr=1.0, iss_radius_src=1.0, iss_radius_tgt=1.0,
                                feature_radius=0.0, normals_available=0, vp_src=vp_src, vp_tgt=vp_tgt)
        res = {}
        ms, all_ms = timed(lambda: res.setdefault("r", ctx.align(s, t, p, descriptor="shot")), ctx.sync, args.reps)
        r = ctx.align(s, t, p, descriptor="shot")
        out = dict(case="corner scene 3 x 100 x 100, multi-scale, cluster, closest_plane, SHOT", end_to_end_ms=ms, end_to_end_ms_all=all_ms,
                   stage_ms=dict(zip(["downsample", "normals", "descriptor", "match", "filter", "align"], list(r.stage_ms)[:6])),
                   n_correspondences=r.n_correspondences, n_inliers=r.n_inliers)
        json.dump(out, open(os.path.join(args.out, "shot_corner.json"), "w"), indent=1)
        print(json.dumps(out))
    if "bench1m" in cases:
        pair = synthetic.make_pair(1_000_000, seed=synthetic.SEED)
        s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
        kw = dict(matching_id=capi.MATCH_LR, bf_block_size=200000, distance_thr=0.1, keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06,
                  iss_radius_tgt=0.06, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
        p = capi.default_params(**kw)
        ms, all_ms = timed(lambda: ctx.align(s, t, p, descriptor="shot"), ctx.sync, args.reps)
        r = ctx.align(s, t, p, descriptor="shot")
        ms_f, _ = timed(lambda: ctx.align(s, t, p), ctx.sync, args.reps)
        # the stage alone on the source cloud: ISS key points on the normals-estimated cloud, SHOT at the multi-scale radius rule
        ctx.normals_knn(s, 30, vp=pair["vp_src"])
        idx = ctx.iss_keypoints(s, 0.06).long()
        kps = s[idx].contiguous()
        dens = ctx.cloud_density(s)
        radius = float(np.sqrt(352 * dens * dens / np.pi))
        lrf_ms, _ = timed(lambda: ctx.shot_lrf(kps, s, radius), ctx.sync, args.reps)
        shot_ms, _ = timed(lambda: ctx.shot(kps, s, radius), ctx.sync, args.reps)
        m = match_case(ctx, int(kps.shape[0]), int(kps.shape[0]), args.reps, rng)
        out = dict(case="bench generator 1M pair, ISS key points (0.06), lr, RANSAC", end_to_end_ms=ms, end_to_end_ms_all=all_ms,
                   end_to_end_fpfh_ms=ms_f, stage_ms=dict(zip(["downsample", "normals", "descriptor", "match", "filter", "align"], list(r.stage_ms)[:6])),
                   n_correspondences=r.n_correspondences, n_keypoints_src=int(kps.shape[0]), stage_radius=radius,
                   lrf_stage_ms=lrf_ms, shot_stage_ms_with_lrf=shot_ms, matcher=m)
        json.dump(out, open(os.path.join(args.out, "shot_bench1m.json"), "w"), indent=1)
        print(json.dumps(out))
    if "match50k" in cases:
        out = dict(case="dense matcher 50k x 50k, both directions", **match_case(ctx, 50_000, 50_000, args.reps, rng))
        json.dump(out, open(os.path.join(args.out, "shot_match50k.json"), "w"), indent=1)
        print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
