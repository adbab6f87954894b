"""-m gpu: matching_id = LGR_MATCH_RATIO through lgr_correspondences_ex_dev, lgr_align_ex2_dev and lgr_measure_dev.  Every lgr_corr field
is compared bit for bit, in order, with tests/ratio_ref_lib.py's composition of pinned pieces (the descriptor statements, the k-nearest
statement, the ratio test, multiscale_ref_lib.vote, oracle.filter_matches(ONE_SIDED)): single scale for FPFH with ratio_k 2 and 3, for
SHOT and RoPS with ratio_k 2, and one multi-scale case.  lgr_align_ex2_dev is the search followed by lgr_ransac_ex_dev, and
lgr_measure_dev is its runs; whether the alignment converges is not asserted (DESIGN.md section 3.1i records what it did).  Then the
refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiscale_ref_lib as ms  # noqa: E402
import randomness_ref_lib as R  # noqa: E402
import ratio_ref_lib as ratio  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ISS = (0.02, 0.03)
BLOCK = 1500            # three bf blocks over 4000 rows
RESULT_FIELDS = ("iterations", "converged", "n_inliers", "best_iteration", "num_rejections", "estimated_iters", "n_correspondences")
RESULT_FLOATS = ("metric", "best_metric_before_refit")
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def pair():
    from lgr_amd import synthetic
    return synthetic.make_pair(4000, 12)


def _statement(oracle, pair, descriptor):
    if descriptor not in _cache:
        _cache[descriptor] = R.SingleScale(oracle, pair, descriptor)
    return _cache[descriptor]


def _kw(pair, **more):
    from lgr_amd import capi
    kw = dict(randomness=1, matching_id=capi.MATCH_RATIO, feature_radius=0.25, bf_block_size=BLOCK, distance_thr=0.1, iss_radius_src=ISS[0],
              iss_radius_tgt=ISS[1], vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    kw.update(more)
    return kw


def check_corr(corr, want):
    assert len(corr) == len(want)
    np.testing.assert_array_equal(corr["index_query"], want["query"])
    np.testing.assert_array_equal(corr["index_match"], want["match"])
    np.testing.assert_array_equal(bits(corr["distance"]), bits(want["distance"]))
    np.testing.assert_array_equal(bits(corr["threshold"]), bits(want["threshold"]))


def same_result(got, want):
    np.testing.assert_array_equal(bits(got.matrix()), bits(want.matrix()))
    for f in RESULT_FIELDS:
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))
    for f in RESULT_FLOATS:
        assert bits(getattr(got, f)) == bits(getattr(want, f)), (f, getattr(got, f), getattr(want, f))


@pytest.mark.parametrize("descriptor,k", [("fpfh", 2), ("fpfh", 3), ("shot", 2), ("rops", 2)])
def test_single_scale_correspondences(lgr, oracle, pair, descriptor, k):
    from lgr_amd import capi
    want, ij, _ = ratio.single_scale(_statement(oracle, pair, descriptor), oracle, k, BLOCK, ISS[1])
    n = len(pair["src"])
    assert 50 < len(want) < n // 2 and (np.diff(want["query"]) > 0).all()      # the test drops most key points; ascending source index
    got = lgr.correspondences(cuda(pair["src"]), cuda(pair["tgt"]), capi.default_params(**_kw(pair)),
                              descriptor=capi.feature_params(descriptor, ratio_k=k))
    check_corr(got.cpu().numpy().view(capi.CORR_DTYPE).reshape(-1), want)


def test_ratio_k_unset_and_null_feature_params_mean_two(lgr, pair):
    from lgr_amd import capi
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    p = capi.default_params(**_kw(pair))
    two = lgr.correspondences(s, t, p, descriptor=capi.feature_params("fpfh", ratio_k=2)).cpu().numpy()
    for descriptor in ("fpfh", capi.feature_params("fpfh"), capi.feature_params("fpfh", ratio_k=0)):   # 'fpfh': lgr_correspondences_dev, a NULL struct
        np.testing.assert_array_equal(lgr.correspondences(s, t, p, descriptor=descriptor).cpu().numpy(), two)
    three = lgr.correspondences(s, t, p, descriptor=capi.feature_params("fpfh", ratio_k=3)).cpu().numpy()
    assert three.shape != two.shape or (three != two).any()


def test_filter_accepts_ratio_as_one_sided(lgr, oracle, pair):
    from lgr_amd import capi
    st = _statement(oracle, pair, "fpfh")
    want, ij, dij = ratio.single_scale(st, oracle, 2, BLOCK, ISS[1])
    none = np.full(len(pair["tgt"]), -1, np.int32)
    got = lgr.filter(capi.MATCH_RATIO, cuda(pair["src"]), cuda(pair["tgt"]), cuda(ij), cuda(dij), cuda(none), cuda(np.zeros(len(none), F)), 0.1, 40)
    check_corr(got, want)


def test_multiscale_correspondences(lgr, oracle):
    from lgr_amd import capi
    fx = ms.fixture("F1")
    iss = ms.CASES[("F1", "any")]
    st = ms.Statement(oracle, fx["src"], fx["tgt"], descriptor="fpfh", keypoints="any", iss_radius=iss, vp=(fx["vp_src"], fx["vp_tgt"]))
    want, ij, _, n_levels = ratio.multiscale(st, oracle, 2, 2500)
    one = st.tables(2500)[0]
    assert n_levels > 1 and len(want) > 50 and ((ij >= 0) & (ij != one)).sum() > 0    # several levels; the vote sees other candidates
    kw = dict(randomness=1, matching_id=capi.MATCH_RATIO, feature_radius=0.0, bf_block_size=2500, distance_thr=0.1, iss_radius_src=iss[0],
              iss_radius_tgt=iss[1], vp_src=fx["vp_src"], vp_tgt=fx["vp_tgt"])
    got = lgr.correspondences(cuda(fx["src"]), cuda(fx["tgt"]), capi.default_params(**kw), descriptor=capi.feature_params("fpfh", ratio_k=2))
    check_corr(got.cpu().numpy().view(capi.CORR_DTYPE).reshape(-1), want)


def test_align_is_ransac_on_these_correspondences_and_measure_is_its_runs(lgr, pair):
    from lgr_amd import capi
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    f = capi.feature_params("fpfh", ratio_k=2)
    seeds = [119, 120]
    runs_want = []
    for seed in seeds:
        p = capi.default_params(**_kw(pair, max_iterations=2000, fix_seed=0, seed=seed))
        corr = lgr.correspondences(s, t, p, descriptor=f)
        res = lgr.align_ex2(s, t, p, descriptor=f)
        rr, _ = lgr.ransac_ex(s, t, corr, p)
        assert res.n_correspondences == corr.shape[0] > 50
        rr.n_correspondences = res.n_correspondences       # (the loop alone does not fill it in)
        same_result(res, rr)
        runs_want.append(res)
    p = capi.default_params(**_kw(pair, max_iterations=2000))
    m, runs = lgr.measure(s, t, p, pair["T_gt"], n_times=2, seeds=seeds, descriptor=f)
    assert m.n_times == 2 and [r.seed for r in runs] == seeds
    for r, want in zip(runs, runs_want):
        same_result(r.result, want)


def test_refusals(lgr, pair):
    from lgr_amd import capi
    lib = capi.lib()
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    n_pts = s.shape[0]
    out = lgr.empty((n_pts, 4), lgr.torch.int32)
    n = C.c_int(0)
    res = capi.Result()
    runs = (capi.MeasureRun * 2)()
    m = capi.Measurement()
    T16 = lgr._T16(pair["T_gt"])
    cases = [(dict(randomness=2), 2, capi.ERR_UNSUPPORTED), (dict(use_bfmatcher=0), 2, capi.ERR_UNSUPPORTED),
             (dict(guess=np.eye(4), match_search_radius=1.0), 2, capi.ERR_UNSUPPORTED),
             (dict(), 1, capi.ERR_UNSUPPORTED), (dict(), 9, capi.ERR_UNSUPPORTED), (dict(), -2, capi.ERR_UNSUPPORTED),
             (dict(matching_id=7), 2, capi.ERR_INVALID_ARG)]
    for more, k, code in cases:
        p = capi.default_params(**_kw(pair, max_iterations=100, **more))
        for descriptor in ("fpfh", "shot", "rops"):
            if descriptor != "fpfh" and (p.use_bfmatcher == 0 or p.has_guess):
                continue                                    # (refused for the descriptor already)
            f = capi.feature_params(descriptor, ratio_k=k)
            what = (more, k, descriptor)
            assert lib.lgr_correspondences_ex_dev(lgr.h, capi._ptr(s), n_pts, capi._ptr(t), n_pts, C.byref(p), C.byref(f), capi._ptr(out), C.byref(n)) == code, what
            assert lib.lgr_align_ex2_dev(lgr.h, capi._ptr(s), n_pts, capi._ptr(t), n_pts, C.byref(p), C.byref(f), None, C.byref(res)) == code, what
            assert lib.lgr_measure_dev(lgr.h, capi._ptr(s), n_pts, capi._ptr(t), n_pts, C.byref(p), C.byref(f), None, T16, None, 2, runs, C.byref(m)) == code, what
    # ratio_k is read under MATCH_RATIO only: the other matchers take a struct that holds 9 there
    p = capi.default_params(**_kw(pair, matching_id=capi.MATCH_ONE_SIDED))
    assert lgr.correspondences(s, t, p, descriptor=capi.feature_params("fpfh", ratio_k=9)).shape[0] == n_pts
    # the source side is never voted on or matched against: its radius is not read
    p = capi.default_params(**_kw(pair, iss_radius_src=0.0))
    assert lgr.correspondences(s, t, p).shape[0] > 50
