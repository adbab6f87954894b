"""GPU: the measure test type (lgr_measure*): seeded repeat runs of one pair judged against the ground truth in one batch.  The yardsticks
are the existing single-run entry points (lgr_align_ex2_dev, lgr_ransac_ex_dev), the CPU statement of the analysis
(analysis_ref_lib.evaluate_gt), the oracle's RANSAC and the numpy restatement of the aggregates (measure_ref_lib) -- never the new code.

The iteration cap and the seeds were chosen on the CPU with the oracle's RANSAC (Philox, uniformity metric) over the correspondences of the
pair below and judged by analysis_ref_lib.evaluate_gt at thr = 0.0617121 (c = 4000, 106 correct).  With max_iterations = 150:
    seed  converged  success  inliers  overlap_rmse  r_err
    119   1          1        89       0.01579       0.02247
    120   1          0        26       0.08527       0.22543     converged, but the overlap error is not below thr
    121   0          0        21       0.13195       0.31834
    122   1          1        75       0.01551       0.02918
    123   0          0         0       nan           nan         the identity: no source point within reach of a target plane
    117   1          1        87       0.02257       0.01654
and seeds 107, 108, 109 all end not converged with 0 inliers (the all-fail case)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref_lib as A  # noqa: E402
import measure_ref_lib as M  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MAX_ITERATIONS = 150
SEEDS = [119, 120, 121, 122, 123, 117]
SEEDS_FAIL = [107, 108, 109]
RESULT_FIELDS = ("iterations", "converged", "n_inliers", "best_iteration", "num_rejections", "estimated_iters", "n_correspondences")
RESULT_FLOATS = ("metric", "best_metric_before_refit")


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_result(got, want):
    """the fields of lgr_result that do not hold a time, by bits"""
    np.testing.assert_array_equal(bits(got.matrix()), bits(want.matrix()))
    for f in RESULT_FIELDS:
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))
    for f in RESULT_FLOATS:
        assert M.same_float(getattr(got, f), getattr(want, f)), (f, getattr(got, f), getattr(want, f))


def same_eval(dev, ref):
    for f in A.FLOAT_FIELDS:
        assert M.same_float(getattr(dev, f), ref[f]), (f, getattr(dev, f), ref[f])
    for f in A.INT_FIELDS:
        assert getattr(dev, f) == ref[f], (f, getattr(dev, f), ref[f])


def same_aggregates(m, runs):
    """the measurement equals measure_ref_lib over the returned runs, their returned times included"""
    want = M.aggregate([dict(success=bool(r.eval.converged_and_overlap_ok), r_err=r.eval.r_err, t_err=r.eval.t_err, overlap_rmse=r.eval.overlap_rmse,
                             time_cs=r.result.time_cs, time_te=r.result.time_te) for r in runs])
    assert (m.n_times, m.n_success) == (want["n_times"], want["n_success"]) and list(m.reserved) == [0] * 5
    for f in M.FIELDS:
        assert M.same_float(getattr(m, f), want[f]), (f, getattr(m, f), want[f])
    return want


@pytest.fixture(scope="module")
def pair(lgr):
    """the pair of test_gpu_evaluate_gt_batch.py: make_pair(4000, seed 12), normals from lgr_normals_knn, thr = twice the target's density"""
    from lgr_amd import synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    out = dict(T_gt=p["T_gt"].astype(F), vp_src=p["vp_src"], vp_tgt=p["vp_tgt"])
    for side in ("src", "tgt"):
        d = cuda(p[side])
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        out[side] = d.cpu().numpy()
        out["d_" + side] = cuda(out[side])
    out["thr"] = float(F(2 * lgr.cloud_density(out["d_tgt"])))
    return out


def params_of(pair, **kw):
    from lgr_amd import capi
    base = dict(matching_id=capi.MATCH_ONE_SIDED, bf_block_size=200000, distance_thr=pair["thr"], vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"],
                max_iterations=MAX_ITERATIONS, fix_seed=0)
    base.update(kw)
    return capi.default_params(**base)


def check_runs(lgr, pair, m, runs, seeds, descriptor="fpfh", mparams=None, with_statement=True, **kw):
    """every run against lgr_align_ex2_dev with its seed, its evaluation against the statement with the final mask of lgr_ransac_ex_dev"""
    src, tgt, G, thr = pair["d_src"], pair["d_tgt"], pair["T_gt"], pair["thr"]
    assert m.n_times == len(runs) == len(seeds)
    corr = lgr.correspondences(src, tgt, params_of(pair, **kw), descriptor=descriptor)
    h_corr = corr.cpu().numpy().view(A.CORR_DTYPE).reshape(-1)
    for r, seed in zip(runs, seeds):
        assert r.seed == seed
        p = params_of(pair, seed=seed, **kw)
        same_result(r.result, lgr.align_ex2(src, tgt, p, descriptor=descriptor, mparams=mparams))
        assert r.result.time_cs == runs[0].result.time_cs and r.result.time_cs > 0 and r.result.time_te > 0   # one shared search
        assert list(r.result.stage_ms)[:5] == list(runs[0].result.stage_ms)[:5]
        if with_statement:
            res, fm = lgr.ransac_ex(src, tgt, corr, p, mparams)
            same_result(r.result, res)
            ref, _ = A.evaluate_gt(pair["src"], pair["tgt"], h_corr, res.matrix(), G, thr, bool(res.converged), fm)
            same_eval(r.eval, ref)
    return h_corr


def test_six_seeds(lgr, oracle, pair):
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair), pair["T_gt"], n_times=6, seeds=SEEDS)
    h_corr = check_runs(lgr, pair, m, runs, SEEDS)
    # the chosen inputs are not degenerate, judged on the yardstick's values (check_runs has tied the runs to them)
    ok = [r for r in runs if r.eval.converged_and_overlap_ok]
    assert len(ok) >= 2 and len(ok) < 6
    assert any(r.result.converged and not r.eval.converged_and_overlap_ok for r in runs)
    assert any(not np.array_equal(bits(r.result.matrix()), bits(ok[0].result.matrix())) for r in ok[1:])
    want = same_aggregates(m, runs)
    assert m.n_success == len(ok) and M.same_float(m.success_rate, F(len(ok)) / F(6))
    assert not np.isnan(want["mae"]) and want["sae"] > 0 and want["stime"] >= 0
    # one seed against the oracle's RANSAC on the CPU
    ocorr = np.zeros(len(h_corr), oracle.CORR_DTYPE)
    ocorr["query"] = h_corr["index_query"]; ocorr["match"] = h_corr["index_match"]; ocorr["distance"] = h_corr["distance"]; ocorr["threshold"] = h_corr["threshold"]
    ores, _ = oracle.ransac(pair["src"], pair["tgt"], ocorr, oracle.default_params(rng_mode=oracle.RNG_PHILOX, seed=SEEDS[0], max_iterations=MAX_ITERATIONS,
                                                                                 distance_thr=pair["thr"]))
    r = runs[0].result
    assert (r.iterations, r.best_iteration, r.num_rejections, r.estimated_iters, r.converged, r.n_inliers) == \
        (ores.iterations, ores.best_iteration, ores.num_rejections, ores.estimated_iters, ores.converged, ores.n_inliers)
    np.testing.assert_array_equal(bits(r.matrix()), bits(ores.matrix()))
    assert M.same_float(r.metric, ores.metric)


def test_default_seeds_count_up_from_params_seed(lgr, pair):
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair, seed=SEEDS[0]), pair["T_gt"], n_times=4)
    assert [r.seed for r in runs] == [SEEDS[0] + i for i in range(4)] == SEEDS[:4]
    m6, runs6 = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair), pair["T_gt"], n_times=4, seeds=SEEDS[:4])
    for a, b in zip(runs, runs6):
        same_result(a.result, b.result)
        same_eval(a.eval, {f: getattr(b.eval, f) for f in A.FLOAT_FIELDS + A.INT_FIELDS})
    same_aggregates(m, runs)
    # fix_seed in the caller's parameters does not reach the runs (src/main.cpp:339)
    _, runs_f = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair, seed=SEEDS[0], fix_seed=1), pair["T_gt"], n_times=2)
    for a, b in zip(runs_f, runs):
        same_result(a.result, b.result)


def test_all_runs_fail(lgr, pair):
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair), pair["T_gt"], n_times=3, seeds=SEEDS_FAIL)
    check_runs(lgr, pair, m, runs, SEEDS_FAIL)
    assert all(not r.eval.converged_and_overlap_ok for r in runs)
    assert m.n_success == 0 and m.success_rate == 0
    for f in ("mae", "sae", "mte", "ste", "mrmse", "srmse"):
        assert np.isnan(getattr(m, f)), f
    assert m.mtime > 0 and not np.isnan(m.stime)
    same_aggregates(m, runs)


def test_gror_runs_once(lgr, pair):
    from lgr_amd import capi
    p = params_of(pair, alignment_id=capi.ALIGN_GROR)
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], p, pair["T_gt"], n_times=5)
    assert m.n_times == 1 and len(runs) == 1   # src/main.cpp:350
    same_result(runs[0].result, lgr.align_ex2(pair["d_src"], pair["d_tgt"], p))
    corr = lgr.correspondences(pair["d_src"], pair["d_tgt"], p)
    res, fm = lgr.gror(pair["d_src"], pair["d_tgt"], corr, pair["thr"])
    ref, _ = A.evaluate_gt(pair["src"], pair["tgt"], corr.cpu().numpy().view(A.CORR_DTYPE).reshape(-1), res.matrix(), pair["T_gt"], pair["thr"],
                           bool(res.converged), fm)
    same_eval(runs[0].eval, ref)
    same_aggregates(m, runs)


def test_shot_descriptor(lgr, pair):
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair), pair["T_gt"], n_times=2, seeds=SEEDS[:2], descriptor="shot")
    check_runs(lgr, pair, m, runs, SEEDS[:2], descriptor="shot")
    same_aggregates(m, runs)


def test_weighted_closest_plane_shares_the_weight_map(lgr, pair):
    """weighted_closest_plane with exp_curvature: the map is computed once and handed to every run; each run equals lgr_align_ex2_dev, which
    computes it itself"""
    from lgr_amd import capi
    mp = capi.metric_params("exp_curvature")
    kw = dict(metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE)
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair, **kw), pair["T_gt"], n_times=2, seeds=SEEDS[:2], mparams=mp)
    check_runs(lgr, pair, m, runs, SEEDS[:2], mparams=mp, **kw)
    same_aggregates(m, runs)
    # ... and with the default (constant) weights, which every run computes for itself
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair, **kw), pair["T_gt"], n_times=2, seeds=SEEDS[:2])
    check_runs(lgr, pair, m, runs, SEEDS[:2], with_statement=False, **kw)


def test_guess_passes_through(lgr, pair):
    ang = np.deg2rad(2.0)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    kw = dict(guess=(dT @ pair["T_gt"]).astype(F), match_search_radius=0.3)
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair, **kw), pair["T_gt"], n_times=2, seeds=SEEDS[:2])
    check_runs(lgr, pair, m, runs, SEEDS[:2], **kw)
    same_aggregates(m, runs)


def test_host_twin(lgr, pair):
    m, runs = lgr.measure(pair["d_src"], pair["d_tgt"], params_of(pair), pair["T_gt"], n_times=3, seeds=SEEDS[:3])
    mh, runs_h = lgr.measure_host(pair["src"], pair["tgt"], params_of(pair), pair["T_gt"], n_times=3, seeds=SEEDS[:3])
    assert mh.n_times == 3 and mh.n_success == m.n_success
    for a, b in zip(runs_h, runs):
        assert a.seed == b.seed
        same_result(a.result, b.result)
        same_eval(a.eval, {f: getattr(b.eval, f) for f in A.FLOAT_FIELDS + A.INT_FIELDS})
    same_aggregates(mh, runs_h)
    for f in ("mae", "sae", "mte", "ste", "mrmse", "srmse"):   # (the times differ between two calls)
        assert M.same_float(getattr(mh, f), getattr(m, f)), f


def test_clouds_without_two_points(lgr, pair):
    m, runs = lgr.measure(pair["d_src"][:1], pair["d_tgt"], params_of(pair), pair["T_gt"], n_times=2, seeds=SEEDS[:2])
    assert m.n_times == 2 and m.n_success == 0
    for r in runs:
        assert not r.result.converged and np.array_equal(r.result.matrix(), np.eye(4, dtype=F)) and r.result.n_correspondences == 0
        ref, _ = A.evaluate_gt(pair["src"][:1], pair["tgt"], np.zeros(0, A.CORR_DTYPE), np.eye(4, dtype=F), pair["T_gt"], pair["thr"], False)
        same_eval(r.eval, ref)
    same_aggregates(m, runs)


def test_refusals(lgr, pair):
    from lgr_amd import capi
    lib = capi.lib()
    s, t = pair["d_src"], pair["d_tgt"]
    T = lgr._T16(pair["T_gt"])
    runs, m, res = (capi.MeasureRun * 65)(), capi.Measurement(), capi.Result()

    def call(p, n, fp=None):
        return lib.lgr_measure_dev(lgr.h, capi._ptr(s), s.shape[0], capi._ptr(t), t.shape[0], C.byref(p), fp, None, T, None, n, runs, C.byref(m))
    for n in (0, 65, -1):
        assert call(params_of(pair), n) == capi.ERR_INVALID_ARG, n
    # what lgr_align_ex2_dev refuses is refused with its code
    cases = [dict(randomness=2, iss_radius_src=0.1, iss_radius_tgt=0.1, guess=np.eye(4), match_search_radius=1.0), dict(n_samples=9), dict(alignment_id=7),
             dict(metric_id=99), dict(cluster_k=65, matching_id=capi.MATCH_CLUSTER)]
    for kw in cases:
        p = params_of(pair, **kw)
        want = lib.lgr_align_ex2_dev(lgr.h, capi._ptr(s), s.shape[0], capi._ptr(t), t.shape[0], C.byref(p), None, None, C.byref(res))
        assert want != 0, kw
        assert call(p, 2) == want, kw
    assert call(params_of(pair, randomness=2, iss_radius_src=0.1, iss_radius_tgt=0.1, guess=np.eye(4), match_search_radius=1.0), 2) == capi.ERR_UNSUPPORTED
    # the evaluation's own bound comes after align's refusals: alone it is an invalid argument, beside one of them align's code stands
    assert call(params_of(pair, distance_thr=0.0), 2) == capi.ERR_INVALID_ARG
    assert call(params_of(pair, distance_thr=0.0, n_samples=9), 2) == capi.ERR_UNSUPPORTED
    assert call(params_of(pair, distance_thr=-1.0, metric_id=99), 2) == capi.ERR_UNSUPPORTED
    mp = capi.metric_params(capi.WEIGHT_HARRIS)
    p = params_of(pair, metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE)
    assert lib.lgr_measure_dev(lgr.h, capi._ptr(s), s.shape[0], capi._ptr(t), t.shape[0], C.byref(p), None, C.byref(mp), T, None, 2, runs, C.byref(m)) == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.LgrError, match="rc=%d" % capi.ERR_INVALID_ARG):
        lgr.measure(s, t, params_of(pair), pair["T_gt"], n_times=0)
