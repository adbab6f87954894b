"""k-nearest matcher and vote measurements on the MI355X -> profiles/match_knn.json.

Cases: match_knn2 on 20 000 x 20 000 x 352 and on 100 000 x 100 000 x 33 for k = 1, 2, 4, 8, each beside the one-match matcher of the
same rows in the same run (lgr_match2_shot_dev, lgr_match_bf2_dev); the vote on 1M x 8 candidates; lgr_align_dev on the bench
generator's pair with randomness 1 and 3.  Every time is the median of --reps runs after one warm-up run of the same shapes, taken with
events on the context's stream (torch's current stream)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-global-registration_amd"), ROOT):
    sys.path.insert(0, p)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(float(e0.elapsed_time(e1)))
    return float(np.median(ts)), ts


def rows(rng, m, dim):
    import torch
    x = rng.random((m, dim), dtype=np.float32)
    if dim == 352:
        x = x ** 4
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return torch.from_numpy(x).cuda()


def match_case(ctx, m, dim, block, reps, rng):
    a, b = rows(rng, m, dim), rows(rng, m, dim)
    one = {352: ctx.match2_shot, 33: ctx.match_bf2}[dim]
    base, base_all = timed(lambda: one(a, b, block), reps)
    out = dict(rows=m, row_len=dim, block=block, one_match_both_directions_ms=base, one_match_ms_all=base_all, knn2=[])
    for k in (1, 2, 4, 8):
        ms, all_ms = timed(lambda: ctx.match_knn2(a, b, block, k), reps)
        out["knn2"].append(dict(k=k, ms=ms, ms_all=all_ms, ratio_to_one_match=ms / base, pairs_per_s=2.0 * m * m / (ms * 1e-3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_knn.json"))
    ap.add_argument("--cases", default="shot20k,fpfh100k,vote1m,align")
    ap.add_argument("--align-points", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_match_knn.py measures the MI355X; there is no CPU fallback"
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
    if "vote1m" in cases:
        m = 1_000_000
        pts = torch.from_numpy(rng.random((m, 12), dtype=np.float32)).cuda()
        ci = torch.from_numpy(rng.integers(0, m, (m, 8)).astype(np.int32)).cuda()
        cd = torch.from_numpy(rng.random((m, 8), dtype=np.float32)).cuda()
        ms, all_ms = timed(lambda: ctx.vote_matches(ci, cd, pts, 0.01), args.reps)
        out["vote1m"] = dict(queries=m, width=8, ms=ms, ms_all=all_ms)
        print(json.dumps(out["vote1m"]))
    if "align" in cases:
        pair = synthetic.make_pair(args.align_points, seed=synthetic.SEED)
        s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
        res = dict(points=args.align_points)
        for k in (1, 3):
            p = capi.default_params(randomness=k, matching_id=capi.MATCH_CLUSTER, feature_radius=0.25, bf_block_size=200000, max_iterations=1000000,
                                    distance_thr=0.1, iss_radius_src=0.02, iss_radius_tgt=0.02, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
            last = {}
            ms, all_ms = timed(lambda: last.update(r=ctx.align(s, t, p)), args.reps)
            r = last["r"]
            res[f"randomness_{k}"] = dict(ms=ms, ms_all=all_ms, match_stage_ms=float(r.stage_ms[3]), n_correspondences=r.n_correspondences,
                                          n_inliers=r.n_inliers, converged=r.converged)
        out["align"] = res
        print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
