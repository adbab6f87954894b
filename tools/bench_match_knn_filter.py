"""The MFMA-filtered k-nearest matcher beside the exact scan on the MI355X -> profiles/match_knn_filter.json.

Stand-alone calls: lgr_match_knn2_dev (both directions) and lgr_match_ratio_dev (one direction) on uniform random 33-float rows, block
10 000, for --sizes and --ks, under mode 0 (the exact scan, the parent's kernel) and mode 1 (filtered), the modes alternating in one run;
sizes in --filtered-only run under mode 1 alone.  Per case the counters of lgr_match_knn_last: candidates per query, fallback rows.
Pipeline: lgr_align_dev on the bench generator's pair (every point a key point, cluster filter, block 200 000) at randomness 3 and at
matching ratio under mode 1 (--align-exact adds mode 0, which takes tens of seconds per run at 1M points).
Every time is the median of --reps runs after one warm-up run of the same shapes, taken with events on the context's stream.

--row-len 135 | 352 measures the filter of the long rows with the same stand-alone cases (write it to its own --out, e.g.
profiles/match_knn_dense_filter.json); --rows unit takes the rows of tests/test_gpu_match_dense_filter.py (non-negative, ** 4, unit norm)
instead of uniform ones, and the keys of the output carry the row length and the generator.  The pipeline part is for 33-float rows."""
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
    c = ctx.match_knn_last()
    return dict(filtered=c[0], canonical_pairs=c[1], candidates_per_query=c[1] / max(1, queries), rows_from_candidates=c[2], rows_on_fallback=c[3],
                train_rows_offered_to_all=c[4], capacity=c[5], reason=c[7])


def make_rows(rng, m, row_len, kind):
    x = rng.random((m, row_len), dtype=np.float32)
    if kind == "unit":
        x = x ** 4
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return x


def standalone(ctx, m, ks, reps, rng, modes, row_len=33, kind="uniform"):
    import torch
    a = torch.from_numpy(make_rows(rng, m, row_len, kind)).cuda()
    b = torch.from_numpy(make_rows(rng, m, row_len, kind)).cuda()
    out = dict(rows=m, row_len=row_len, generator=kind, block=10000, cases=[])
    for k in ks:
        case = dict(k=k)
        for mode in modes:
            ctx.set_knn_filter(mode, 0)
            ms, all_ms = timed(lambda: ctx.match_knn2(a, b, 10000, k), reps)
            case[f"knn2_mode{mode}"] = dict(ms=ms, ms_all=all_ms, **counters(ctx, 2 * m))
            if k >= 2:
                ms, all_ms = timed(lambda: ctx.match_ratio(a, b, 10000, k), reps)
                case[f"ratio_mode{mode}"] = dict(ms=ms, ms_all=all_ms, **counters(ctx, m))
        if len(modes) == 2:
            case["knn2_exact_over_filtered"] = case["knn2_mode0"]["ms"] / case["knn2_mode1"]["ms"]
            if k >= 2:
                case["ratio_exact_over_filtered"] = case["ratio_mode0"]["ms"] / case["ratio_mode1"]["ms"]
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
    ctx.set_knn_filter(-1, 0)
    return out


def align(ctx, points, seed, reps, modes):
    import torch
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(points, seed=seed)
    s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    kw = dict(feature_radius=0.25, bf_block_size=200000, max_iterations=1000000, distance_thr=0.1, iss_radius_src=0.02, iss_radius_tgt=0.02,
              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    res = dict(points=points, seed=seed)
    for name, p, desc in (("randomness_3", capi.default_params(randomness=3, matching_id=capi.MATCH_CLUSTER, **kw), capi.feature_params("fpfh")),
                          ("ratio", capi.default_params(randomness=1, matching_id=capi.MATCH_RATIO, **kw), capi.feature_params("fpfh", ratio_k=2))):
        for mode in modes:
            ctx.set_knn_filter(mode, 0)
            last = {}
            ms, all_ms = timed(lambda: last.update(r=ctx.align_ex2(s, t, p, descriptor=desc)), reps)
            r = last["r"]
            res[f"{name}_mode{mode}"] = dict(ms=ms, ms_all=all_ms, match_stage_ms=float(r.stage_ms[3]), n_correspondences=r.n_correspondences,
                                             n_inliers=r.n_inliers, converged=r.converged, **counters(ctx, 2 * points if name != "ratio" else points))
            print(name, mode, json.dumps(res[f"{name}_mode{mode}"]), flush=True)
    ctx.set_knn_filter(-1, 0)
    return res


def real_shot(ctx, reps, modes):
    """tools/bench_shot.py's configuration (bench generator 1M pair, ISS key points at 0.06) with the two k-nearest uses of SHOT rows"""
    import torch
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(1_000_000, seed=synthetic.SEED)
    s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    kw = dict(bf_block_size=200000, distance_thr=0.1, keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06, iss_radius_tgt=0.06,
              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    res = dict(case="bench generator 1M pair, ISS key points (0.06), SHOT352, RANSAC")
    for name, p, desc in (("ratio", capi.default_params(randomness=1, matching_id=capi.MATCH_RATIO, **kw), capi.feature_params("shot", ratio_k=2)),
                          ("randomness_3_lr", capi.default_params(randomness=3, matching_id=capi.MATCH_LR, **kw), capi.feature_params("shot"))):
        for mode in modes:
            ctx.set_knn_filter(mode, 0)
            last = {}
            ms, all_ms = timed(lambda: last.update(r=ctx.align_ex2(s, t, p, descriptor=desc)), reps)
            r = last["r"]
            c = ctx.match_knn_last()
            res[f"{name}_mode{mode}"] = dict(end_to_end_ms=ms, ms_all=all_ms, match_stage_ms=float(r.stage_ms[3]), n_correspondences=r.n_correspondences,
                                             n_inliers=r.n_inliers, converged=r.converged, fallback_share=c[3] / max(1, c[2] + c[3]),
                                             **counters(ctx, c[2] + c[3]))
            print(name, mode, json.dumps(res[f"{name}_mode{mode}"]), flush=True)
    ctx.set_knn_filter(-1, 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_knn_filter.json"))
    ap.add_argument("--sizes", default="4096,16384,65536,100000")
    ap.add_argument("--filtered-only", default="1000000")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--align-points", type=int, default=1_000_000)
    ap.add_argument("--align-seeds", default="")
    ap.add_argument("--align-exact", action="store_true")
    ap.add_argument("--row-len", type=int, default=33, choices=(33, 135, 352))
    ap.add_argument("--rows", default="uniform", choices=("uniform", "unit"))
    ap.add_argument("--real-shot", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_match_knn_filter.py measures the MI355X; there is no CPU fallback"
    from lgr_amd import capi, synthetic
    ctx = capi.Context(0)
    rng = np.random.default_rng(0)
    ks = [int(k) for k in args.ks.split(",") if k]
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)

    tag = "" if (args.row_len, args.rows) == (33, "uniform") else f"_{args.row_len}_{args.rows}"
    for m in [int(x) for x in args.sizes.split(",") if x]:
        out[f"standalone_{m}{tag}"] = standalone(ctx, m, ks, args.reps, rng, (0, 1), args.row_len, args.rows)
        save()
    for m in [int(x) for x in args.filtered_only.split(",") if x]:
        out[f"standalone_{m}{tag}"] = standalone(ctx, m, ks, args.reps, rng, (1,), args.row_len, args.rows)
        save()
    for seed in [synthetic.SEED if x == "bench" else int(x) for x in args.align_seeds.split(",") if x]:
        out[f"align_seed{seed}"] = align(ctx, args.align_points, seed, args.reps, (0, 1) if args.align_exact else (1,))
        save()
    if args.real_shot:
        out["real_shot"] = real_shot(ctx, args.reps, (0, 1))
        save()
    ctx.close()


if __name__ == "__main__":
    main()
