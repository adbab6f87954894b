"""-m gpu: randomness = k > 1 through lgr_correspondences* / lgr_align*: the k nearest rows per key point, the proximity vote, then the
filters as before.  Every lgr_corr field is compared bit for bit with tests/randomness_ref_lib.py's composition of pinned pieces
(oracle features or the SHOT / RoPS statements, the k-nearest statement, multiscale_ref_lib.vote, oracle.filter_matches): single scale
for FPFH (lr, one_sided, cluster), SHOT and RoPS (lr), and one multi-scale case.  In every single-scale case at least 1 % of the source
key points end on a match that is not their nearest row (measured on the CPU composition: 10 % FPFH, 13 % SHOT, 19 % RoPS), so a vote
that is skipped or runs on the wrong side's key points or radius shows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiscale_ref_lib as ms  # noqa: E402
import randomness_ref_lib as R  # noqa: E402

pytestmark = pytest.mark.gpu
ISS = (0.02, 0.03)      # vote radii of source and target: different, so that exchanged sides show
BLOCK = 1500            # three bf blocks over 4000 rows
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def _kw(pair, matching, **more):
    kw = dict(randomness=3, matching_id=matching, feature_radius=0.25, bf_block_size=BLOCK, distance_thr=0.1, iss_radius_src=ISS[0],
              iss_radius_tgt=ISS[1], vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    kw.update(more)
    return kw


def check_corr(corr, want):
    assert len(corr) == len(want)
    np.testing.assert_array_equal(corr["index_query"], want["query"])
    np.testing.assert_array_equal(corr["index_match"], want["match"])
    np.testing.assert_array_equal(bits(corr["distance"]), bits(want["distance"]))
    np.testing.assert_array_equal(bits(corr["threshold"]), bits(want["threshold"]))


@pytest.mark.parametrize("descriptor,matching", [("fpfh", 0), ("fpfh", 1), ("fpfh", 2), ("shot", 0), ("rops", 0)])
def test_single_scale_correspondences(lgr, oracle, pair, descriptor, matching):
    from lgr_amd import capi
    want, moved = _statement(oracle, pair, descriptor).correspondences(matching, 3, BLOCK, ISS)
    assert moved >= 0.01 and len(want) > 50
    got = lgr.correspondences(cuda(pair["src"]), cuda(pair["tgt"]), capi.default_params(**_kw(pair, matching)), descriptor=descriptor)
    check_corr(got.cpu().numpy().view(capi.CORR_DTYPE).reshape(-1), want)


def test_randomness_changes_the_correspondences(lgr, pair):
    from lgr_amd import capi
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    c3 = lgr.correspondences(s, t, capi.default_params(**_kw(pair, 0))).cpu().numpy()
    c1 = lgr.correspondences(s, t, capi.default_params(**_kw(pair, 0, randomness=1))).cpu().numpy()
    assert c1.shape != c3.shape or (c1 != c3).any()


def test_multiscale_correspondences(lgr, oracle):
    from lgr_amd import capi
    fx = ms.fixture("F1")
    iss = ms.CASES[("F1", "any")]
    st = ms.Statement(oracle, fx["src"], fx["tgt"], descriptor="fpfh", keypoints="any", iss_radius=iss, vp=(fx["vp_src"], fx["vp_tgt"]))
    ij, dij, ji, dji = R.multiscale_tables(st, 2, 2500)
    one = st.tables(2500)
    assert (ij != one[0]).mean() >= 0.01                # the second match per level changes the vote's outcome
    want = oracle.filter_matches(0, st.kps[0], st.kps[1], ij, dij, ji, dji, 0.1, 40)
    assert len(want) > 50
    kw = dict(randomness=2, matching_id=0, feature_radius=0.0, bf_block_size=2500, distance_thr=0.1, iss_radius_src=iss[0], iss_radius_tgt=iss[1],
              vp_src=fx["vp_src"], vp_tgt=fx["vp_tgt"])
    got = lgr.correspondences(cuda(fx["src"]), cuda(fx["tgt"]), capi.default_params(**kw))
    check_corr(got.cpu().numpy().view(capi.CORR_DTYPE).reshape(-1), want)


def test_align_is_ransac_on_these_correspondences(lgr, pair):
    from lgr_amd import capi
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    p = capi.default_params(**_kw(pair, 0, max_iterations=20000))
    corr = lgr.correspondences(s, t, p)
    res = lgr.align(s, t, p)
    rr, _ = lgr.ransac(s, t, corr, p)
    assert res.converged == 1 and res.n_correspondences == corr.shape[0]
    assert np.abs(res.matrix() - pair["T_gt"]).max() < 0.05
    assert (res.iterations, res.n_inliers, res.best_iteration, res.converged) == (rr.iterations, rr.n_inliers, rr.best_iteration, rr.converged)
    np.testing.assert_array_equal(bits(res.matrix()), bits(rr.matrix()))


def test_refusals(lgr, pair):
    from lgr_amd import capi
    lib = capi.lib()
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    n_pts = s.shape[0]
    out = lgr.empty((n_pts, 4), lgr.torch.int32)
    n = C.c_int(0)
    res = capi.Result()
    nan = float("nan")
    cases = [(dict(use_bfmatcher=0), capi.ERR_UNSUPPORTED),                                   # matchFLANN
             (dict(guess=np.eye(4), match_search_radius=1.0), capi.ERR_UNSUPPORTED),          # matchLocal
             (dict(randomness=9), capi.ERR_UNSUPPORTED), (dict(randomness=0), capi.ERR_UNSUPPORTED),
             (dict(iss_radius_tgt=0.0), capi.ERR_INVALID_ARG), (dict(iss_radius_src=0.0), capi.ERR_INVALID_ARG),
             (dict(iss_radius_tgt=nan), capi.ERR_INVALID_ARG), (dict(iss_radius_src=-1.0), capi.ERR_INVALID_ARG),
             (dict(iss_radius_tgt=0.0, feature_radius=0.0), capi.ERR_INVALID_ARG)]
    for more, code in cases:
        p = capi.default_params(**_kw(pair, 0, max_iterations=100, **more))
        assert lib.lgr_correspondences_dev(lgr.h, capi._ptr(s), n_pts, capi._ptr(t), n_pts, C.byref(p), capi._ptr(out), C.byref(n)) == code, more
        assert lib.lgr_align_dev(lgr.h, capi._ptr(s), n_pts, capi._ptr(t), n_pts, C.byref(p), C.byref(res)) == code, more
    # one_sided votes on the target key points only: the source radius is not read
    p = capi.default_params(**_kw(pair, 1, iss_radius_src=0.0))
    assert lgr.correspondences(s, t, p).shape[0] > 0
