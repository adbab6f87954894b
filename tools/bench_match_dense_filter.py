"""The MFMA-filtered nearest-row matcher of SHOT352 / RoPS135 rows beside the exact scan on the MI355X -> profiles/match_dense_filter.json.

Stand-alone calls: lgr_match2_shot_dev / lgr_match2_rops_dev (both directions, block 10 000) for --sizes on the rows of
tests/test_gpu_match_shot.py's generator (random**4, unit norm) at 352 and 135 floats, under mode 0 (the exact scan) and mode 1
(filtered), the modes alternating in one run.  Per case the counters of lgr_match_dense_last: candidates per query, fallback share.
Real rows (--real): lgr_align on the bench generator's 1M pair with ISS key points (the configuration of tools/bench_shot.py /
tools/bench_rops.py) under both modes: the match stage's time and the counters on real flat-scene descriptors.
Every time is the median of --reps runs after one warm-up run of the same shapes, taken with events on the context's stream."""
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


def counters(ctx, queries):
    c = ctx.match_dense_last()
    return dict(filtered=c[0], canonical_pairs=c[1], candidates_per_query=c[1] / max(1, queries), rows_from_candidates=c[2], rows_on_fallback=c[3],
                fallback_share=c[3] / max(1, queries), train_rows_offered_to_all=c[4], capacity=c[5], reason=c[7])


def rows(rng, m, dim):
    x = rng.random((m, dim), dtype=np.float32) ** 4
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def standalone(ctx, m, dim, reps, rng):
    import torch
    a, b = torch.from_numpy(rows(rng, m, dim)).cuda(), torch.from_numpy(rows(rng, m, dim)).cuda()
    match2 = ctx.match2_shot if dim == 352 else ctx.match2_rops
    case = dict(rows=m, row_len=dim, block=10000)
    for mode in (0, 1):
        ctx.set_dense_filter(mode, 0)
        ms, all_ms = timed(lambda: match2(a, b, 10000), reps)
        case[f"mode{mode}"] = dict(ms=ms, ms_all=all_ms, **counters(ctx, 2 * m))
    ctx.set_dense_filter(-1, 0)
    case["exact_over_filtered"] = case["mode0"]["ms"] / case["mode1"]["ms"]
    print(json.dumps(case), flush=True)
    return case


def real(ctx, name, reps):
    import torch
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(1_000_000, seed=synthetic.SEED)
    s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    p = capi.default_params(matching_id=capi.MATCH_LR, bf_block_size=200000, distance_thr=0.1, keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06,
                            iss_radius_tgt=0.06, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    desc = capi.feature_params("shot") if name == "shot" else capi.feature_params("rops", lrf_id=capi.LRF_GRAVITY)
    case = dict(case="bench generator 1M pair, ISS key points (0.06), lr, RANSAC", descriptor=name)
    for mode in (0, 1):
        ctx.set_dense_filter(mode, 0)
        last = {}
        ms, all_ms = timed(lambda: last.update(r=ctx.align_ex2(s, t, p, descriptor=desc)), reps)
        r = last["r"]
        c = ctx.match_dense_last()
        case[f"mode{mode}"] = dict(end_to_end_ms=ms, ms_all=all_ms, match_stage_ms=float(r.stage_ms[3]), n_correspondences=r.n_correspondences,
                                   n_inliers=r.n_inliers, converged=r.converged, **counters(ctx, c[2] + c[3]))
    ctx.set_dense_filter(-1, 0)
    print(json.dumps(case), flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_dense_filter.json"))
    ap.add_argument("--sizes", default="4096,16384,35913,50000")
    ap.add_argument("--dims", default="352,135")
    ap.add_argument("--real", default="shot,rops")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_match_dense_filter.py measures the MI355X; there is no CPU fallback"
    from lgr_amd import capi
    ctx = capi.Context(0)
    rng = np.random.default_rng(0)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)

    for dim in [int(x) for x in args.dims.split(",") if x]:
        for m in [int(x) for x in args.sizes.split(",") if x]:
            out[f"standalone_{dim}_{m}"] = standalone(ctx, m, dim, args.reps, rng)
            save()
    for name in [x for x in args.real.split(",") if x]:
        out[f"real_{name}"] = real(ctx, name, args.reps)
        save()
    ctx.close()


if __name__ == "__main__":
    main()
