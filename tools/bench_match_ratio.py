"""Ratio matcher measurements on the MI355X -> profiles/match_ratio.json.

Cases: lgr_match_ratio_dev at k = 2 on 20 000 x 20 000 x 352 and on 100 000 x 100 000 x 33 beside lgr_match_knn2_dev (both directions:
what lr or cluster over k-nearest lists would sweep) and lgr_match_knn_dev (one direction with its m x k table) at k = 2 on the same rows,
alternating in one run; lgr_align_dev with matching ratio beside lr on the bench generator's 1M pair with ISS key points
(tools/bench_shot.py's configuration) for SHOT and FPFH rows: stage times, correspondences, inliers; the 4000-point pair of the tests
(every point a key point, FPFH at feature_radius 0.25) under one_sided, lr and ratio with ratio_k 2 and 3: correspondences, the share
within 0.1 of the ground truth, and whether RANSAC converges on them.  Every time is the median of --reps
runs after one warm-up run of the same shapes, taken with events on the context's stream (torch's current stream)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-global-registration_amd"), ROOT):
    sys.path.insert(0, p)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_match_knn import rows  # noqa: E402

STAGES = ["downsample", "normals", "descriptor", "match", "filter", "align"]


def timed_alternating(fns, reps):
    """one warm-up of each, then reps rounds that run every function once: {name: (median ms, all ms)}"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts[name].append(float(e0.elapsed_time(e1)))
    return {name: (float(np.median(v)), v) for name, v in ts.items()}


def match_case(ctx, m, dim, block, reps, rng):
    a, b = rows(rng, m, dim), rows(rng, m, dim)
    t = timed_alternating(dict(ratio=lambda: ctx.match_ratio(a, b, block, 2), knn=lambda: ctx.match_knn(a, b, block, 2),
                               knn2=lambda: ctx.match_knn2(a, b, block, 2)), reps)
    idx, _ = ctx.match_ratio(a, b, block, 2)
    ctx.sync()
    return dict(rows=m, row_len=dim, block=block, k=2, ratio_ms=t["ratio"][0], ratio_ms_all=t["ratio"][1], knn_one_direction_ms=t["knn"][0],
                knn_one_direction_ms_all=t["knn"][1], knn2_ms=t["knn2"][0], knn2_ms_all=t["knn2"][1], ratio_to_knn2=t["ratio"][0] / t["knn2"][0],
                ratio_to_knn_one_direction=t["ratio"][0] / t["knn"][0], pairs_per_s=1.0 * m * m / (t["ratio"][0] * 1e-3),
                kept=int((idx >= 0).sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_ratio.json"))
    ap.add_argument("--cases", default="shot20k,fpfh100k,pair4000,align")
    ap.add_argument("--align-points", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_match_ratio.py measures the MI355X; there is no CPU fallback"
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    rng = np.random.default_rng(0)
    cases = args.cases.split(",")
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if "shot20k" in cases:
        out["shot20k"] = match_case(ctx, 20_000, 352, 10000, args.reps, rng)
        print(json.dumps(out["shot20k"]))
    if "fpfh100k" in cases:
        out["fpfh100k"] = match_case(ctx, 100_000, 33, 10000, args.reps, rng)
        print(json.dumps(out["fpfh100k"]))
    if "pair4000" in cases:
        pair = synthetic.make_pair(4000, 12)
        s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
        T = pair["T_gt"].astype(np.float32)
        res = dict(case="make_pair(4000, 12), every point a key point, FPFH, feature_radius 0.25, uniformity metric, RANSAC")
        for name, matching, k in (("one_sided", capi.MATCH_ONE_SIDED, None), ("lr", capi.MATCH_LR, None), ("ratio2", capi.MATCH_RATIO, 2), ("ratio3", capi.MATCH_RATIO, 3)):
            p = capi.default_params(matching_id=matching, feature_radius=0.25, bf_block_size=1500, distance_thr=0.1, iss_radius_src=0.02, iss_radius_tgt=0.03,
                                    vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
            f = capi.feature_params("fpfh", ratio_k=k)
            r = ctx.align(s, t, p, descriptor=f)
            corr = ctx.correspondences(s, t, p, descriptor=f).cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
            moved = pair["src"][corr["index_query"], :3] @ T[:3, :3].T + T[:3, 3]
            res[name] = dict(n_correspondences=len(corr), share_correct_within_0p1=float((np.linalg.norm(moved - pair["tgt"][corr["index_match"], :3], axis=1) < 0.1).mean()),
                             converged=r.converged, n_inliers=r.n_inliers, iterations=r.iterations, max_abs_error_to_ground_truth=float(np.abs(r.matrix() - T).max()))
        out["pair4000"] = res
        print(json.dumps(res))
    if "align" in cases:
        pair = synthetic.make_pair(args.align_points, seed=synthetic.SEED)
        s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
        T = pair["T_gt"].astype(np.float32)
        res = dict(case=f"bench generator {args.align_points} pair, ISS key points (0.06), multi-scale, RANSAC", points=args.align_points)
        for descriptor in ("shot", "fpfh"):
            for matching in ("lr", "ratio"):
                p = capi.default_params(matching_id={"lr": capi.MATCH_LR, "ratio": capi.MATCH_RATIO}[matching], bf_block_size=200000, distance_thr=0.1,
                                        keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06, iss_radius_tgt=0.06, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
                last = {}
                tm = timed_alternating({matching: lambda: last.update(r=ctx.align(s, t, p, descriptor=descriptor))}, args.reps)[matching]
                r = last["r"]
                corr = ctx.correspondences(s, t, p, descriptor=descriptor).cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
                moved = pair["src"][corr["index_query"], :3] @ T[:3, :3].T + T[:3, 3]
                correct = float((np.linalg.norm(moved - pair["tgt"][corr["index_match"], :3], axis=1) < 0.1).mean()) if len(corr) else float("nan")
                res[f"{descriptor}_{matching}"] = dict(ms=tm[0], ms_all=tm[1], stage_ms=dict(zip(STAGES, [float(x) for x in list(r.stage_ms)[:6]])),
                                                       n_correspondences=r.n_correspondences, share_correct_within_0p1=correct, n_inliers=r.n_inliers,
                                                       converged=r.converged, max_abs_error_to_ground_truth=float(np.abs(r.matrix() - T).max()))
        out["align"] = res
        print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
