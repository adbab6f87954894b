"""Register two PLY scans end to end on one MI355X, the way the reference's `registration alignment` run does
(loadPointClouds -> alignPointClouds -> transformations.csv), through the C ABI:

    python tools/register_ply.py source.ply target.ply [--keypoint iss|any] [--metric uniformity|combination|...]
                                 [--feature-radius R] [--distance-thr D] [--out transformations.csv]
                                 [--ground-truth transformations_gt.csv NAME [--results results.csv] [--metrics-csv metrics.csv]]
                                 [--debug-dir DIR] [--hypotheses N [--hypotheses-plane]] [--refine N]
                                 [--icp N [--icp-max-dist D] [--icp-shrink S [--icp-min-dist M]]
                                  [--icp-variant plane|point|plane2plane] [--icp-robust none|huber|cauchy|tukey --icp-robust-scale K]
                                  [--icp-normal-angle DEG] [--icp-weight WEIGHT_ID] [--icp-plane-eps E]
                                  [--icp-trim KEEP] [--icp-robust-median MULT]]
                                 [--measure N [--measure-seed S0] [--measurements test_measurements.csv]] [--save-features DIR]
                                 [--order canonical|reference] [--alignment ransac|gror|teaser]

Steps: formats.read_ply (include/io.h) -> lgr_preprocess (duplicate filter, 2 x density voxel grid, normals;
src/common.cpp:429-470) -> lgr_align (src/alignment.cpp:72-109) -> formats.save_transformation (src/common.cpp:127-153).
With --ground-truth: formats.get_transformation -> lgr_analysis_metric (the dense metric estimator of start's first statement, every
metric) + lgr_evaluate_gt (AlignmentAnalysis::start, src/analysis.cpp:218-246), printed in the order of AlignmentAnalysis::print (:248-272)
and appended to results.csv as AlignmentAnalysis::save does (:274-328).  With --metrics-csv as well: estimateTestMetric's row
(src/main.cpp:41-116) -- the correspondence metric and the dense closest-plane metric of the found transformation and of the ground truth.
With --debug-dir: the files of generateDebugFiles and compareHypotheses (src/main.cpp:207-284) in DIR, each named <stem>.<ext> with the
reference's `name` argument as the stem -- downsampled_tgt.ply (and downsampled_src.ply with a ground truth: key points beige, correspondences
red, inliers blue, correct correspondences mixed with white), weights.ply under weighted_closest_plane, temperature_{distances_src,
distances_tgt}.csv, temperature_{dists_src,dists_tgt}.ply (ASCII) and temperature_{normal_diffs_src,normal_diffs_tgt}.ply for the found
transformation; with a ground truth the same six as temperature_gt_* and compareOverlaps' two lines.  The histogram PNGs are not written
(plots.py is no part of this project).
With --hypotheses N (ransac, metrics uniformity and correspondences): the loop once more in the reference's SAVE_MULTIPLE_HYPOTHESES mode
(src/sac_prerejective_omp.cpp:11) through lgr_ransac_multi -- the set of up to N distinct hypotheses, one line per member (id, iteration,
loop metric, metric after the refit, inliers, uniformity, chosen); with --debug-dir the members also go through compareOverlaps.
With --hypotheses-plane as well the set is built through lgr_ransac_multi_ex, which takes every metric: closest_plane, combination and
weighted_closest_plane (with --weight); without it --hypotheses refuses those metrics as it always has.
With --refine N: after everything above, the found transformation goes through up to N dense closest-plane steps (lgr_refine_plane: inliers,
refit, evaluation, while the metric rises) under the run's score -- and the run's weights under weighted_closest_plane; the evaluation before
and after is printed, the refined transformation is appended to --out as a second row named <name>_refined, and with --ground-truth it is
analysed like the first (a second results.csv row under that name).
With --icp N: the found transformation goes through up to N iterations of point-to-plane ICP (lgr_icp_plane) with pairing
distance D (--icp-max-dist; default 4 x the target's density), shrunk by S per iteration (--icp-shrink, default 1) down to M (--icp-min-dist;
default with S < 1: half the target's density); the pairs and rmse of the first and the last iteration are printed, the result is appended
to --out as a row named <name>_icp, and with --ground-truth it is analysed like the first.  --icp and --refine may be combined: the ICP runs
first and the refinement starts from its result (rows <name>_icp and <name>_icp_refined).
With any of --icp-variant, --icp-robust, --icp-normal-angle, --icp-weight, --icp-plane-eps the iterations run through lgr_icp_ex (DESIGN.md
section 4, "ICP variants") instead: point-to-plane, point-to-point or plane-to-plane residuals, a Huber / Cauchy / Tukey kernel of scale K (in
units of the variant's residual: a distance, for plane2plane a Mahalanobis distance), pairs rejected when the angle between the moved source
normal and the target normal exceeds DEG (the tool hands the cosine to the ABI), and the source's weight map of --icp-weight (the maps of
lgr_weights; harris and tomasi stay refused) as per-point weights.  Without any of them --icp takes the lgr_icp_plane path as before.
With --icp-trim KEEP or --icp-robust-median MULT the iterations run through lgr_icp_trim ("Trimmed ICP"): each iteration
keeps the fraction KEEP of its pairs with the smallest residuals, and the kernel of --icp-robust takes MULT x the iteration's median residual as
its scale (1.4826: the MAD rule; --icp-robust-scale is then not needed).  The tool then also prints the candidates, the kept pairs, the cut and
the scale of the first and the last iteration.
With --measure N (needs --ground-truth): the reference's `measure` test type (measureTestResults, src/main.cpp:312-382) through lgr_measure --
N alignments that differ in the RANSAC seed only (S0, S0 + 1, ...; S0 defaults to the profile's seed), one correspondence search for all of
them, all judged against the ground truth in one batch; one line per run, then the aggregate row, appended to --measurements when given
(with the header when the file is new).  With --hypotheses N and --ground-truth the members of the set are judged the same way
(lgr_evaluate_gt_batch) and their rotation, translation and overlap error are listed.
With --save-features DIR or --measure N the two clouds are prepared once (lgr_cloud_prepare) and the alignment runs on the prepared clouds
(lgr_align_prepared; lgr_measure itself searches once for all its runs, as before).  --save-features is the reference's save_features: DIR receives the descriptor tables of the levels the clouds share, named as include/matching.h:274-278
names them, plus ids.csv (saveExtractedPointIds for the target cloud) with --ground-truth.
With --alignment teaser the correspondence search runs on its own (lgr_correspondences) and its correspondences go through lgr_teaser with
the reference's commented parameters (src/alignment.cpp:41-69; noise bound = distance_thr); the clique and the two inlier counts are
printed, and --out, --ground-truth, --debug-dir and --refine then work on the found transformation as for the other alignments.  lgr_align
and lgr_measure know no teaser, so --measure, --save-features and --hypotheses refuse it.
With --order reference the loader numbers the points as the reference does (the iteration order of its unordered_set and unordered_map,
lgr_preprocess_order_dev), so every index written afterwards is the reference's; the default, canonical, is the (iz,iy,ix) voxel order.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def _descriptor(capi, a, lrf, as_struct=False):
    """the descriptor argument of the Context calls: the plain name for FPFH, else the feature-parameter struct (which carries ratio_k)"""
    if a.descriptor == "fpfh" and a.matching != "ratio" and not as_struct:
        return a.descriptor
    return capi.feature_params(a.descriptor, lrf_id=lrf, ratio_k=a.ratio_k if a.matching == "ratio" else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source"); ap.add_argument("target")
    ap.add_argument("--keypoint", default="iss", choices=["iss", "any"])           # the reference's default (src/common.cpp:247)
    ap.add_argument("--metric", default="uniformity", choices=["uniformity", "correspondences", "closest_plane", "combination",
                                                                    "weighted_closest_plane"])
    ap.add_argument("--weight", default="constant", choices=["constant", "exp_curvature", "curvedness", "curvature", "nss"],
                    help="point weights of weighted_closest_plane (src/weights.cpp)")
    ap.add_argument("--matching", default="cluster", choices=["lr", "one_sided", "cluster", "ratio"])
    ap.add_argument("--ratio-k", type=int, default=2, metavar="K",
                    help="--matching ratio: the test compares a key point's nearest row with its K-th nearest, 2 .. 8 (threshold 1.1)")
    ap.add_argument("--alignment", default="ransac", choices=["ransac", "gror", "teaser"])
    ap.add_argument("--randomness", type=int, default=1, metavar="K",
                    help="matches kept per key point and level before the proximity vote, 1 .. 8 (include/matching.h:612-625, :327-352)")
    ap.add_argument("--descriptor", default="fpfh", choices=["fpfh", "shot", "rops"])
    ap.add_argument("--lrf", default="default", choices=["default", "gravity"],
                    help="local reference frames (SHOT: default only; RoPS: gravity only; FPFH ignores them)")
    ap.add_argument("--feature-radius", type=float, default=0.0, help="<= 0: multi-scale (the reference's behaviour when unset)")
    ap.add_argument("--distance-thr", type=float, default=0.0, help="<= 0: automatic, 4 x the larger cloud density (src/common.cpp:267)")
    ap.add_argument("--iterations", type=int, default=1000000)
    ap.add_argument("--out", default=None, help="transformations.csv to append to")
    ap.add_argument("--ground-truth", nargs=2, metavar=("CSV", "NAME"), default=None,
                    help="transformation CSV and the row that holds the ground truth: analyse the result against it")
    ap.add_argument("--results", default="results.csv", help="results.csv the analysis row is appended to (with --ground-truth)")
    ap.add_argument("--metrics-csv", default=None, help="metrics.csv estimateTestMetric's row is appended to (needs --ground-truth)")
    ap.add_argument("--debug-dir", default=None, help="write the files of generateDebugFiles / compareHypotheses (src/main.cpp:207-284) there")
    ap.add_argument("--hypotheses", type=int, default=0, metavar="N",
                    help="also keep the set of up to N distinct hypotheses (ransac with uniformity / correspondences) and list its members")
    ap.add_argument("--hypotheses-plane", action="store_true",
                    help="with --hypotheses: build the set through lgr_ransac_multi_ex, which also takes closest_plane, combination and weighted_closest_plane")
    ap.add_argument("--refine", type=int, default=0, metavar="N", help="refine the result by up to N dense closest-plane steps (lgr_refine_plane)")
    ap.add_argument("--icp", type=int, default=0, metavar="N", help="then up to N iterations of point-to-plane ICP (lgr_icp_plane); runs before --refine")
    ap.add_argument("--icp-max-dist", type=float, default=0.0, metavar="D", help="pairing distance of the first iteration (<= 0: 4 x the target's density)")
    ap.add_argument("--icp-shrink", type=float, default=1.0, metavar="S", help="factor on the pairing distance per iteration, in (0, 1]")
    ap.add_argument("--icp-min-dist", type=float, default=0.0, metavar="M",
                    help="floor of the pairing distance (<= 0: half the target's density when --icp-shrink < 1, else the first iteration's distance)")
    ap.add_argument("--icp-variant", default=None, choices=["plane", "point", "plane2plane"], help="the residual of lgr_icp_ex (default with another --icp-* option: plane)")
    ap.add_argument("--icp-robust", default=None, choices=["none", "huber", "cauchy", "tukey"], help="M-estimator on the variant's residual (needs --icp-robust-scale)")
    ap.add_argument("--icp-robust-scale", type=float, default=None, metavar="K", help="scale of --icp-robust, in units of the variant's residual")
    ap.add_argument("--icp-normal-angle", type=float, default=None, metavar="DEG",
                    help="reject a pair whose moved source normal and target normal differ by more than DEG degrees, 0 .. 180")
    ap.add_argument("--icp-weight", default=None, choices=["constant", "exp_curvature", "curvedness", "curvature", "nss"],
                    help="per-point weights of the ICP: the source's weight map of that name (src/weights.cpp)")
    ap.add_argument("--icp-plane-eps", type=float, default=None, metavar="E", help="plane2plane: the covariance along the normal, 1e-6 .. 1 (default 1e-3)")
    ap.add_argument("--icp-trim", type=float, default=None, metavar="KEEP", help="trimmed ICP (lgr_icp_trim): the fraction of each iteration's pairs that is kept, in (0, 1]")
    ap.add_argument("--icp-robust-median", type=float, default=None, metavar="MULT",
                    help="scale of --icp-robust = MULT x the iteration's median residual (1.4826: the MAD rule) instead of --icp-robust-scale")
    ap.add_argument("--measure", type=int, default=0, metavar="N",
                    help="the measure test type: N seeded runs judged against --ground-truth, and their test_measurements.csv row")
    ap.add_argument("--measure-seed", type=int, default=None, metavar="S0", help="seed of the first run (default: the profile's seed); run i uses S0 + i")
    ap.add_argument("--measurements", default=None, metavar="PATH", help="test_measurements.csv the aggregate row is appended to (with --measure)")
    ap.add_argument("--save-features", default=None, metavar="DIR",
                    help="save_features: prepare the two clouds once, align through them and write the levels' descriptor tables (and ids.csv with --ground-truth) to DIR")
    ap.add_argument("--order", default="canonical", choices=["canonical", "reference"],
                    help="point numbering after the loader: (iz,iy,ix) voxel order, or the reference's hash-container order")
    ap.add_argument("--knn-filter", default="auto", choices=["auto", "on", "off"],
                    help="how --randomness > 1 / --matching ratio sweep FPFH, SHOT and RoPS rows (never what they return): the MFMA filter from the crossover size, always, never")
    ap.add_argument("--dense-filter", default="auto", choices=["auto", "on", "off"],
                    help="how SHOT / RoPS rows are matched at --randomness 1 (never what is returned): the MFMA filter from the crossover size, always, never")
    a = ap.parse_args()
    if a.measure and not a.ground_truth:
        ap.error("--measure needs --ground-truth")
    if not 0 <= a.measure <= 64:
        ap.error("--measure takes 1 .. 64 runs")
    if not 1 <= a.randomness <= 8:
        ap.error("--randomness takes 1 .. 8")
    if not 2 <= a.ratio_k <= 8:
        ap.error("--ratio-k takes 2 .. 8")
    if a.matching == "ratio" and a.randomness != 1:
        ap.error("--matching ratio needs --randomness 1")
    if not 0 <= a.refine <= 1024:
        ap.error("--refine takes 0 .. 1024 steps")
    if not 0 <= a.icp <= 1024:
        ap.error("--icp takes 0 .. 1024 iterations")
    if not 0.0 < a.icp_shrink <= 1.0:
        ap.error("--icp-shrink takes a factor in (0, 1]")
    a.icp_ex = any(v is not None for v in (a.icp_variant, a.icp_robust, a.icp_robust_scale, a.icp_normal_angle, a.icp_weight, a.icp_plane_eps))
    if a.icp_ex and not a.icp:
        ap.error("the --icp-* options need --icp N")
    a.icp_trimmed = a.icp_trim is not None or a.icp_robust_median is not None
    if a.icp_trimmed and not a.icp:
        ap.error("the --icp-* options need --icp N")
    if a.icp_trim is not None and not 0.0 < a.icp_trim <= 1.0:
        ap.error("--icp-trim takes a fraction in (0, 1]")
    if a.icp_robust_median is not None:
        if not a.icp_robust_median > 0.0 or a.icp_robust_median == float("inf"):
            ap.error("--icp-robust-median takes a finite multiplier > 0")
        if a.icp_robust in (None, "none") or a.icp_robust_scale is not None:
            ap.error("--icp-robust-median needs --icp-robust huber|cauchy|tukey and replaces --icp-robust-scale")
    elif (a.icp_robust not in (None, "none")) != (a.icp_robust_scale is not None):
        ap.error("--icp-robust huber|cauchy|tukey and --icp-robust-scale go together")
    if a.icp_robust_scale is not None and not a.icp_robust_scale > 0.0:
        ap.error("--icp-robust-scale takes a scale > 0")
    if a.icp_normal_angle is not None and not 0.0 <= a.icp_normal_angle <= 180.0:
        ap.error("--icp-normal-angle takes 0 .. 180 degrees")
    if a.icp_plane_eps is not None and not 1e-6 <= a.icp_plane_eps <= 1.0:
        ap.error("--icp-plane-eps takes 1e-6 .. 1")
    if a.metrics_csv and not a.ground_truth:
        ap.error("--metrics-csv needs --ground-truth")
    if a.hypotheses_plane and not a.hypotheses:
        ap.error("--hypotheses-plane needs --hypotheses")
    if a.hypotheses and (a.alignment != "ransac" or (a.metric not in ("uniformity", "correspondences") and not a.hypotheses_plane)):
        ap.error("--hypotheses needs --alignment ransac and --metric uniformity or correspondences (any other metric: add --hypotheses-plane)")

    if a.alignment == "teaser" and (a.measure or a.save_features):
        ap.error("--alignment teaser runs through lgr_teaser: --measure and --save-features (lgr_measure, lgr_align_prepared) do not take it")

    import numpy as np
    from lgr_amd import capi, formats, profile
    ctx = capi.Context(0)
    ctx.set_knn_filter({"auto": -1, "on": 1, "off": 0}[a.knn_filter])
    ctx.set_dense_filter({"auto": -1, "on": 1, "off": 0}[a.dense_filter])
    t = time.perf_counter()
    # loadPointClouds: duplicates, 2 x density voxel grid, normals
    ld = profile.load_pair(ctx, a.source, a.target, order=capi.ORDER_REFERENCE if a.order == "reference" else capi.ORDER_CANONICAL)
    ctx.sync()
    for side, path in (("src", a.source), ("tgt", a.target)):
        print(f"{os.path.basename(path)}: {len(ld['raw_' + side])} points -> {ld[side].shape[0]} after preprocessing "
              f"(voxel {ld['voxel_' + side]:.4g}, density {ld['density_' + side]:.4g})")
    print(f"loaded in {1e3 * (time.perf_counter() - t):.1f} ms")
    clouds = [ld["src"], ld["tgt"]]
    # getParametersFromConfig with the keys left out: distance_thr = 4 x max density, iss_radius = 2 x density (src/common.cpp:266-271,325-333)
    p = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint=a.keypoint, metric=a.metric, matching=a.matching,
                                alignment="ransac" if a.alignment == "teaser" else a.alignment, feature_radius=a.feature_radius if a.feature_radius > 0 else None,
                                distance_thr=a.distance_thr if a.distance_thr > 0 else None, iterations=a.iterations,
                                normals_available=ld["normals_available"], randomness=a.randomness)
    t = time.perf_counter()
    lrf = {"default": capi.LRF_DEFAULT, "gravity": capi.LRF_GRAVITY}[a.lrf]
    if a.alignment == "teaser":
        res = align_teaser(ctx, capi, a, p, clouds, lrf)
    elif a.save_features or a.measure:
        res = align_prepared(ctx, capi, formats, a, p, clouds, lrf)
    elif a.metric == "weighted_closest_plane":
        res = ctx.align_ex2(clouds[0], clouds[1], p, descriptor=_descriptor(capi, a, lrf, True), mparams=capi.metric_params(a.weight))
    else:
        res = ctx.align(clouds[0], clouds[1], p, descriptor=_descriptor(capi, a, lrf))
    dt = time.perf_counter() - t
    T = res.matrix()
    print(f"aligned in {1e3 * dt:.1f} ms: converged={res.converged} correspondences={res.n_correspondences} inliers={res.n_inliers} "
          f"metric={res.metric:.4f} iterations={res.iterations}")
    print(np.array2string(T, precision=6, suppress_small=True))
    name = os.path.splitext(os.path.basename(a.source))[0] + "_" + os.path.splitext(os.path.basename(a.target))[0]
    if a.out:
        formats.save_transformation(a.out, name, T)
    if a.ground_truth:
        analyse(ctx, capi, formats, a, p, clouds, res, T, name, lrf)
    if a.debug_dir:
        debug_files(ctx, capi, formats, a, p, clouds, T, lrf)
    if a.hypotheses:
        hypotheses(ctx, capi, formats, a, p, clouds, lrf)
    if a.icp:
        T, name = icp(ctx, capi, formats, a, p, clouds, res, T, name, lrf, ld["density_tgt"])
    if a.refine:
        refine(ctx, capi, formats, a, p, clouds, res, T, name, lrf)
    if a.measure:
        measure(ctx, capi, formats, a, p, clouds, name, lrf)


def align_teaser(ctx, capi, a, p, clouds, lrf):
    """alignPointClouds with alignment "teaser" (src/alignment.cpp:92-101): the search, then lgr_teaser on its correspondences"""
    t = time.perf_counter()
    corr = ctx.correspondences(clouds[0], clouds[1], p, descriptor=_descriptor(capi, a, lrf))
    ctx.sync()
    time_cs = time.perf_counter() - t
    res, info, clique, nodes, mask = ctx.teaser(clouds[0], clouds[1], corr, capi.default_teaser_params(p.distance_thr))
    res.time_cs = time_cs
    print(f"teaser: valid={info.valid} nodes={info.n_nodes} max_core={info.max_core} core_nodes={info.n_core} clique={info.n_clique} "
          f"rotation_iterations={info.rotation_iterations} rotation_inliers={info.n_rotation_inliers}/{max(info.n_clique - 1, 0)} "
          f"translation_inliers={info.n_translation_inliers}/{info.n_clique}")
    return res


def align_prepared(ctx, capi, formats, a, p, clouds, lrf):
    """--save-features / --measure: both clouds are prepared once (lgr_cloud_prepare) and the alignment runs on the prepared clouds.
    AlignmentParameters::save_features: the descriptor tables of the levels the two clouds share are written as match_multiscale does for
    source -> target (include/matching.h:273-279): histograms_src.csv / histograms_tgt.csv with a fixed radius,
    histograms<log2_radius>_src.csv / _tgt.csv per level without one.  With --ground-truth also ids.csv for the target cloud
    (saveExtractedPointIds, src/main.cpp:342-344)."""
    f = _descriptor(capi, a, lrf, True)
    t = time.perf_counter()
    with ctx.prepare_cloud(clouds[0], p, 0, f) as src, ctx.prepare_cloud(clouds[1], p, 1, f) as tgt:
        print(f"prepared both clouds in {1e3 * (time.perf_counter() - t):.1f} ms ({src.info().bytes + tgt.info().bytes} bytes held)")
        res = ctx.align_prepared(src, tgt, p, descriptor=f, metric_params=capi.metric_params(a.weight) if a.metric == "weighted_closest_plane" else None)
        if not a.save_features:
            return res
        os.makedirs(a.save_features, exist_ok=True)
        levels = [{li.log2_radius: i for i, li in enumerate(c.levels())} for c in (src, tgt)]
        for log2_radius in sorted(set(levels[0]) & set(levels[1])):
            for c, lv, is_source in ((src, levels[0], True), (tgt, levels[1], False)):
                stem = formats.histograms_name(None if a.feature_radius > 0 else log2_radius, is_source)
                formats.write_histograms(os.path.join(a.save_features, stem + ".csv"), c.level(lv[log2_radius])[2])
                print(f"wrote {stem}.csv")
    if a.ground_truth:
        T_gt = formats.get_transformation(a.ground_truth[0], a.ground_truth[1])
        formats.write_extracted_ids(os.path.join(a.save_features, "ids.csv"), ctx.extracted_point_ids(clouds[0], clouds[1], T_gt, clouds[1]))
        print("wrote ids.csv")
    return res


def measure(ctx, capi, formats, a, p, clouds, name, lrf):
    """measureTestResults: the seeded runs, one line each, and the aggregate row"""
    import numpy as np
    T_gt = formats.get_transformation(a.ground_truth[0], a.ground_truth[1])
    s0 = p.seed if a.measure_seed is None else a.measure_seed
    mp = capi.metric_params(a.weight) if a.metric == "weighted_closest_plane" else None
    t = time.perf_counter()
    m, runs = ctx.measure(clouds[0], clouds[1], p, T_gt, n_times=a.measure, seeds=[s0 + i for i in range(a.measure)],
                          descriptor=_descriptor(capi, a, lrf, True), mparams=mp)
    dt = time.perf_counter() - t
    deg = 180.0 / np.pi
    print(f"\nmeasured {m.n_times} runs in {1e3 * dt:.1f} ms (one correspondence search: {1e3 * runs[0].result.time_cs:.1f} ms):")
    print("\trun\tseed\tconverged\tsuccess\tinliers\tr_err (deg)\tt_err\toverlap_rmse\ttime (s)")
    for i, r in enumerate(runs):
        e = r.eval
        print(f"\t{i}\t{r.seed}\t{r.result.converged}\t{e.converged_and_overlap_ok}\t{r.result.n_inliers}\t{deg * e.r_err:.7f}\t{e.t_err:.7f}\t{e.overlap_rmse:.7f}"
              f"\t{r.result.time_cs + r.result.time_te:.6f}")
    row = formats.measurements_row(name + "_measure", m)
    print(f"success: {m.n_success}/{m.n_times}")
    print(formats.MEASUREMENTS_HEADER)
    print(row)
    if a.measurements:
        new = not os.path.exists(a.measurements)
        with open(a.measurements, "a") as f:
            if new:
                f.write(formats.MEASUREMENTS_HEADER + "\n")
            f.write(row + "\n")
        print(f"appended the measurement row to {a.measurements}" + (" (new file)" if new else ""))


def refine(ctx, capi, formats, a, p, clouds, res, T, name, lrf):
    """the found transformation through lgr_refine_plane; its row in --out and, with a ground truth, its analysis"""
    import numpy as np
    mp = capi.metric_params(a.weight) if a.metric == "weighted_closest_plane" else None
    t = time.perf_counter()
    r = ctx.refine_plane(clouds[0], clouds[1], T, score_id=p.score_id, max_steps=a.refine, metric_params=mp)
    dt = time.perf_counter() - t
    print(f"\nrefined in {1e3 * dt:.1f} ms: {r.steps} steps of at most {a.refine}, stopped by {capi.REFINE_STOP_NAMES[r.stop]} (threshold {r.threshold:.6g})")
    for label, s in (("before", r.first), (" after", r)):
        print(f"  {label}: metric={s.metric:.7f} inliers_rmse={s.rmse:.7f} inliers={s.n_inliers}")
    Tr = r.matrix()
    print(np.array2string(Tr, precision=6, suppress_small=True))
    if a.out:
        formats.save_transformation(a.out, name + "_refined", Tr)
    if a.ground_truth:
        a.metrics_csv = None   # estimateTestMetric's row belongs to the alignment
        analyse(ctx, capi, formats, a, p, clouds, res, Tr, name + "_refined", lrf)


def icp(ctx, capi, formats, a, p, clouds, res, T, name, lrf, density_tgt):
    """the found transformation through lgr_icp_plane (with an --icp-* option: lgr_icp_ex); its row in --out and, with a ground truth, its
    analysis -> (transformation, row name)"""
    import math
    import numpy as np
    min_dist = a.icp_min_dist if a.icp_min_dist > 0 else (0.5 * density_tgt if a.icp_shrink < 1.0 else 0.0)
    base = dict(max_iterations=a.icp, max_dist=a.icp_max_dist, min_dist=min_dist, shrink=a.icp_shrink)
    t = time.perf_counter()
    if a.icp_ex or a.icp_trimmed:
        w = ctx.weights(clouds[0], a.icp_weight, with_sum=False)[0] if a.icp_weight is not None else None
        cos = math.cos(math.radians(a.icp_normal_angle)) if a.icp_normal_angle is not None else -1.0
        ex = dict(variant=a.icp_variant or "plane", robust=a.icp_robust or "none", robust_scale=a.icp_robust_scale or 0.0, min_normal_cos=max(-1.0, min(1.0, cos)),
                  plane_eps=a.icp_plane_eps or 0.0, weights=w)
        if a.icp_trimmed:
            r = ctx.icp_trim(clouds[0], clouds[1], T, keep=a.icp_trim if a.icp_trim is not None else 1.0, scale_from_median=a.icp_robust_median or 0.0, **ex, **base)
        else:
            r = ctx.icp_ex(clouds[0], clouds[1], T, **ex, **base)
        how = f" ({a.icp_variant or 'plane'}, robust {a.icp_robust or 'none'}" + (f" {a.icp_robust_scale:.6g}" if a.icp_robust_scale else "") + \
            (f" {a.icp_robust_median:.6g} x median" if a.icp_robust_median else "") + \
            (f", normals within {a.icp_normal_angle:.6g} deg" if a.icp_normal_angle is not None else "") + (f", weights {a.icp_weight}" if a.icp_weight else "") + \
            (f", keep {a.icp_trim:.6g}" if a.icp_trim is not None else "") + ")"
    else:
        r = ctx.icp_plane(clouds[0], clouds[1], T, **base)
        how = ""
    dt = time.perf_counter() - t
    print(f"\nicp{how} in {1e3 * dt:.1f} ms: {r.iterations} iterations of at most {a.icp}, stopped by {capi.ICP_STOP_NAMES[r.stop]} (max_dist {r.max_dist:.6g})")
    print(f"  first: pairs={r.pairs0} rmse={r.rmse0:.7f}")
    print(f"   last: pairs={r.pairs} rmse={r.rmse:.7f}")
    if a.icp_trimmed:
        for label, s in (("first", r.info[0]), (" last", r.info[-1])) if r.info else ():
            print(f"  {label} trim: candidates={s.candidates} kept={s.kept} cut={s.cut:.7f} scale={s.scale:.7f}")
    Ti = r.matrix()
    print(np.array2string(Ti, precision=6, suppress_small=True))
    if a.out:
        formats.save_transformation(a.out, name + "_icp", Ti)
    if a.ground_truth:
        metrics_csv, a.metrics_csv = a.metrics_csv, None   # estimateTestMetric's row belongs to the alignment
        analyse(ctx, capi, formats, a, p, clouds, res, Ti, name + "_icp", lrf)
        a.metrics_csv = metrics_csv
    return Ti, name + "_icp"


def hypotheses(ctx, capi, formats, a, p, clouds, lrf):
    """the set of distinct hypotheses of the same correspondences (lgr_ransac_multi), and with --debug-dir compareOverlaps over its members"""
    src, tgt = clouds
    desc = _descriptor(capi, a, lrf)
    corr = ctx.correspondences(src, tgt, p, descriptor=desc)
    t = time.perf_counter()
    if a.hypotheses_plane:
        mp = capi.metric_params(a.weight) if a.metric == "weighted_closest_plane" else None
        res, hyps, best = ctx.ransac_multi_ex(src, tgt, corr, p, max_set=a.hypotheses, metric_params=mp)
    else:
        res, hyps, best = ctx.ransac_multi(src, tgt, corr, p, max_set=a.hypotheses)
    print(f"{len(hyps)} distinct hypotheses in {1e3 * (time.perf_counter() - t):.1f} ms (iterations={res.iterations} converged={res.converged}):")
    print("\tid\titeration\tloop_metric\tmetric\tinliers\tuniformity\tchosen")
    for k, h in enumerate(hyps):
        print(f"\t{k}\t{h.iteration}\t{h.loop_metric:.6f}\t{h.metric:.6f}\t{h.n_inliers}\t{h.uniformity:.6f}\t{'*' if k == best else ''}")
    if a.ground_truth and hyps:
        # every member against the ground truth: what the ground truth alone decides is computed once per batch (lgr_evaluate_gt_batch)
        import numpy as np
        T_gt = formats.get_transformation(a.ground_truth[0], a.ground_truth[1])
        evals = []
        for k0 in range(0, len(hyps), capi.GT_BATCH_MAX):
            part = hyps[k0:k0 + capi.GT_BATCH_MAX]
            evals += ctx.evaluate_gt_batch(src, tgt, corr, [h.matrix() for h in part], T_gt, p.distance_thr, [h.converged for h in part])
        print("\tid\tr_err (deg)\tt_err\toverlap_rmse\tsuccess\tchosen")
        for k, e in enumerate(evals):
            print(f"\thypothesis {k} analysis:\t{180.0 / np.pi * e.r_err:.7f}\t{e.t_err:.7f}\t{e.overlap_rmse:.7f}\t{e.converged_and_overlap_ok}\t{'*' if k == best else ''}")
    if a.debug_dir and hyps:
        o = ctx.compare_overlaps(src, tgt, [h.matrix() for h in hyps], p.distance_thr, with_masks=False)
        for k in range(len(hyps)):
            print(f"\thypothesis {k}: {o['counts'][k]} points, {formats._g(o['weighted'][k])}weighted points")


def debug_files(ctx, capi, formats, a, p, clouds, T, lrf):
    """generateDebugFiles, and with a ground truth compareHypotheses, for the alignment just made"""
    import numpy as np
    os.makedirs(a.debug_dir, exist_ok=True)
    src, tgt = clouds
    ns, nt = src.shape[0], tgt.shape[0]
    T_gt = formats.get_transformation(a.ground_truth[0], a.ground_truth[1]) if a.ground_truth else None
    written = []

    def path(stem, ext="ply"):
        written.append(stem + "." + ext)
        return os.path.join(a.debug_dir, stem + "." + ext)

    # one call per transformation: both temperature maps and the moved source (the clouds of the other files)
    maps = {"temperature": ctx.temperature_maps(src, tgt, T, p.distance_thr)}
    if T_gt is not None:
        maps["temperature_gt"] = ctx.temperature_maps(src, tgt, T_gt, p.distance_thr)
    desc = _descriptor(capi, a, lrf)
    corr = ctx.correspondences(src, tgt, p, descriptor=desc).cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
    # metric_estimator->buildInliers(tn, inliers, error, rand) in the estimator's dense form
    if a.metric in ("closest_plane", "weighted_closest_plane"):
        inliers = ctx.evaluate_plane_dense(src, tgt, T, p.score_id, with_inliers=True).inliers
    else:
        mask, _, _, _ = ctx.evaluate(src, tgt, corr, T, metric_id=p.metric_id, score_id=p.score_id)
        inliers = corr[np.asarray(mask.cpu().numpy() if hasattr(mask, "cpu") else mask, bool)]
    kps = []
    for cloud, radius in ((src, p.iss_radius_src), (tgt, p.iss_radius_tgt)):   # detectKeyPoints
        k = ctx.iss_keypoints(cloud, radius).cpu().numpy() if a.keypoint == "iss" else np.arange(cloud.shape[0], dtype=np.int32)
        kps.append(np.sort(k).astype(np.int32))
    correct = corr[:0]
    if T_gt is not None:
        cm, _, _, _ = ctx.correct_correspondences(src, tgt, corr, T_gt)
        correct = corr[cm.astype(bool)]
        formats.write_ply_colored(path("downsampled_src"), maps["temperature_gt"]["moved"].cpu().numpy(),
                                  ctx.color_correspondences(ns, kps[0], corr, correct, inliers, True))
    formats.write_ply_colored(path("downsampled_tgt"), tgt.cpu().numpy(), ctx.color_correspondences(nt, kps[1], corr, correct, inliers, False))
    if a.metric == "weighted_closest_plane":
        w, _ = ctx.weights(src, a.weight, with_sum=False)
        colors, _ = ctx.color_map(w)
        formats.write_ply_colored(path("weights"), maps["temperature"]["moved"].cpu().numpy(), colors)
    for stem, m in maps.items():
        for side, cloud in (("src", m["moved"].cpu().numpy()), ("tgt", tgt.cpu().numpy())):
            s = m[side]
            formats.save_vector(path(f"{stem}_distances_{side}", "csv"), s["temp_distance"][s["temp_distance"] < np.float32(p.distance_thr)])
            formats.write_ply_colored(path(f"{stem}_dists_{side}"), cloud, s["color_distance"], binary=False)
            formats.write_ply_colored(path(f"{stem}_normal_diffs_{side}"), cloud, s["color_normal"], binary=True)
    if T_gt is not None:
        o = ctx.compare_overlaps(src, tgt, [T, T_gt], p.distance_thr, with_masks=False)
        print(f"\tincorrect hypothesis: {o['counts'][0]} points, {formats._g(o['weighted'][0])}weighted points")
        print(f"\t  correct hypothesis: {o['counts'][1]} points, {formats._g(o['weighted'][1])}weighted points")
    print(f"wrote {len(written)} debug files to {a.debug_dir}: " + " ".join(written))


def analyse(ctx, capi, formats, a, p, clouds, res, T, name, lrf):
    """AlignmentAnalysis::start / print / save for the alignment just made"""
    import numpy as np
    from lgr_amd import profile
    T_gt = formats.get_transformation(a.ground_truth[0], a.ground_truth[1])
    score = {v: k for k, v in profile.SCORE.items()}[p.score_id]
    desc = _descriptor(capi, a, lrf)
    # the alignment's own correspondences: lgr_align hands none back, so the search (deterministic) runs once more here
    corr = ctx.correspondences(clouds[0], clouds[1], p, descriptor=desc)
    # metric, rmse, inliers and correct inliers of the final transformation under the run's metric, in the estimator's dense form (start:
    # buildInliersAndEstimateMetric + buildCorrectInliers)
    mkw = dict(weight=a.weight) if a.metric == "weighted_closest_plane" else {}
    m = ctx.analysis_metric(clouds[0], clouds[1], corr, T, T_gt, metric_id=p.metric_id, score_id=p.score_id, **mkw)
    n_inl, rmse, metric = m.n_inliers, m.rmse, m.metric
    t = time.perf_counter()
    e = ctx.evaluate_gt(clouds[0], clouds[1], corr, T, T_gt, p.distance_thr, bool(res.converged))
    dt = time.perf_counter() - t
    deg = 180.0 / np.pi
    print("\n Ground truth transformation:")
    print(np.array2string(T_gt, precision=6, suppress_small=True))
    print(f"converged: {'true' if res.converged else 'false'}")
    print(f"metric: {metric:.7f}")
    print(f"inliers_rmse: {rmse:.7f}")
    print(f"correct inliers: {m.n_correct_inliers}/{n_inl}")
    print(f"correct correspondences: {e.n_correct_correspondences}/{e.n_correspondences}")
    print(f"rotation error (deg): {deg * e.r_err:.7f}")
    print(f"translation error: {e.t_err:.7f}")
    print(f"point cloud error: {e.pcd_err:.7f}")
    print(f"median of normal differences (deg): {deg * e.normal_diff:.7f}")
    print(f"uniformity of correct correspondences' distribution: {e.corr_uniformity:.7f}")
    print(f"overlap error: {e.overlap_rmse:.7f} over {e.overlap_size} points; overlap: {e.overlap:.7f}, overlap area: {e.overlap_area:.7f}")
    print(f"success (converged and overlap error < {p.distance_thr:.6g}): {'true' if e.converged_and_overlap_ok else 'false'}")
    print(f"analysed in {1e3 * dt:.1f} ms")
    row = formats.results_row(
        version="lgr_amd", descriptor=a.descriptor, testname=name, metric=metric, rmse=rmse, correspondences=e.n_correspondences,
        correct_correspondences=e.n_correct_correspondences, inliers=n_inl, correct_inliers=m.n_correct_inliers,
        nr_points=p.feature_nr_points, distance_thr=p.distance_thr, edge_thr=p.edge_thr_coef, iteration=res.iterations,
        matching_type=a.matching, ratio_k=a.ratio_k, randomness=p.randomness, r_err=e.r_err, t_err=e.t_err, pcd_err=e.pcd_err, normal_diff=e.normal_diff,
        corr_uniformity=e.corr_uniformity, lrf_type=a.lrf, metric_type=a.metric, overlap_rmse=e.overlap_rmse, alignment_type=a.alignment,
        keypoint_type=a.keypoint, time_cs=res.time_cs, time_te=res.time_te, score_type=score, iss_radius_src=p.iss_radius_src,
        iss_radius_tgt=p.iss_radius_tgt, normal_nr_points=p.normal_nr_points, reestimate=0,   # (the device path has no frame re-estimation)
        scale=p.scale_factor, cluster_k=p.cluster_k,
        feature_radius=p.feature_radius if p.feature_radius > 0 else "", overlap=e.overlap, overlap_area=e.overlap_area,
        converged=int(res.converged))
    new = not os.path.exists(a.results)
    with open(a.results, "a") as f:
        if new:
            f.write(formats.RESULTS_HEADER + "\n")
        f.write(row + "\n")
    print(f"appended the analysis row to {a.results}" + (" (new file)" if new else ""))
    if a.metrics_csv:
        # estimateTestMetric: CorrespondencesMetricEstimator and the dense ClosestPlaneMetricEstimator, both under the run's score, for the found
        # transformation and for the ground truth; the target's density is computed by the first dense evaluation and handed to the second
        found, thr = [], 0.0
        for tn in (T, T_gt):
            _, n_corr, _, m_corr = ctx.evaluate(clouds[0], clouds[1], corr, tn, metric_id=capi.METRIC_CORRESPONDENCES, score_id=p.score_id)
            d = ctx.evaluate_plane_dense(clouds[0], clouds[1], tn, p.score_id, threshold=thr)
            thr = d.threshold
            found.append((m_corr, d.metric, n_corr, d.n_inliers))
        new = not os.path.exists(a.metrics_csv)
        with open(a.metrics_csv, "a") as f:
            if new:
                f.write(formats.METRICS_HEADER + "\n")
            f.write(formats.metrics_row(name, found[0], found[1]) + "\n")
        print(f"appended the metric row to {a.metrics_csv}" + (" (new file)" if new else ""))


if __name__ == "__main__":
    main()
