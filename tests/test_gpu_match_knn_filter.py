"""-m gpu: the MFMA-filtered k-nearest matcher of 33-float rows (lgr_ctx_set_knn_filter) against the CPU statement
tests/cpp/knn_match_ref.cpp, on index and distance bits.  Mode 1 (filtered at any size) with the device self-check unless stated: small
shapes (k > mt, block < k, fewer than k column groups, bf blocks that straddle tiles), tie-heavy rows, rows the operands cannot carry,
many tiles with the counters of lgr_match_knn_last, a row whose candidates overflow the list, the three modes against each other, the
pipeline and prepared clouds under modes 0 and 1, the host twin, the refusals.  Every test restores (-1, 0)."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5   # include/lgr.h
F = np.float32


@contextlib.contextmanager
def knn_filter(lgr, mode, self_check=1):
    lgr.set_knn_filter(mode, self_check)
    try:
        yield
    finally:
        lgr.set_knn_filter(-1, 0)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(rng, m, dim=33):
    return rng.random((m, dim)).astype(F)


def _dev(lgr, q, t, block, k):
    i, d = lgr.match_knn(cuda(q), cuda(t), block, k)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32), err_msg=what)


@pytest.fixture(scope="module")
def many():
    """the input of test_gpu_match_knn.py::test_many_tiles_33 and the statement on its 1500 sampled queries"""
    rng = np.random.default_rng(5000)
    q, t = _rows(rng, 5000), _rows(rng, 7000)
    q[:500] = t[rng.choice(7000, 500)]
    t[3000:3200] = t[100:300]
    sel = np.concatenate([np.arange(0, 600), rng.choice(5000, 900, replace=False)])
    return dict(q=q, t=t, sel=sel, want=ref.match(q[sel], t, 2000, 8))


@pytest.mark.parametrize("mq,mt", [(1, 1), (1, 65), (63, 64), (65, 129), (130, 200), (300, 2100)])
def test_shapes(lgr, mq, mt):
    rng = np.random.default_rng(33000 + mq * 7 + mt)
    q, t = _rows(rng, mq), _rows(rng, mt)
    if mt > 4:
        t[mt // 2] = t[0]; t[mt - 1] = t[0]
    with knn_filter(lgr, 1):
        for k in (1, 2, 5, 8):
            for block in (3, 50, 64, mt + 7):
                _eq(_dev(lgr, q, t, block, k), ref.match(q, t, block, k), f"k={k} block={block}")
    assert lgr.knn_filter() == (-1, 0)


def test_ties_follow_the_two_stage_order(lgr):
    rng = np.random.default_rng(34)
    t = ref.tie_rows(rng, 300, 33)
    q = np.concatenate([t[rng.choice(300, 60)], ref.tie_rows(rng, 40, 33)])
    differs = 0
    with knn_filter(lgr, 1):
        for k, block in ((2, 7), (4, 50), (5, 64), (8, 100), (3, 1000)):
            want = ref.match(q, t, block, k)
            differs += int((want[0] != ref.plain(q, t, k)[0]).any(axis=1).sum())
            _eq(_dev(lgr, q, t, block, k), want, f"k={k} block={block}")
    assert differs > 0


def test_special_rows(lgr):
    rng = np.random.default_rng(35)
    q, t = _rows(rng, 70), _rows(rng, 150)
    t[[30, 31]] = np.nan
    t[32, 32] = np.nan
    t[64, 0] = np.inf
    t[40] = F(3e38)
    q[[3, 66]] = np.nan
    q[4, 16] = np.nan
    q[5, 1] = -np.inf
    t[50] = t[50] * F(1e18)                      # finite distances (about 3e18) that the operands cannot carry inside the bound
    q[7] = q[7] * F(1e18)
    t[51] = F(1e18) * _rows(rng, 1)[0]           # a pair of such rows near each other: q[8]'s nearest row is t[51]
    q[8] = t[51] * F(1.0 + 2.0 ** -20)
    with knn_filter(lgr, 1):
        for k, block in ((1, 1000), (3, 33), (8, 64)):
            want = ref.match(q, t, block, k)
            _eq(_dev(lgr, q, t, block, k), want, f"k={k} block={block}")
            last = lgr.match_knn_last()
            assert last[0] == 1 and last[3] > 0 and last[4] > 0 and last[6] == 0, last
            assert (want[0][[3, 4, 5, 66]] == -1).all() and not np.isin(want[0], [30, 31, 32, 40, 64]).any()
            assert want[0][8, 0] == 51 and np.isfinite(want[1][8, 0])


def test_many_tiles(lgr, many):
    with knn_filter(lgr, 1):
        got = _dev(lgr, many["q"], many["t"], 2000, 8)
        last, worst = lgr.match_knn_last(), lgr.match_knn_last_check()
    _eq((got[0][many["sel"]], got[1][many["sel"]]), many["want"])
    print("match_knn_last", last, "worst |a - d2| / e", worst)
    assert last[0] == 1 and last[1] < 5000 * 7000 and last[2] + last[3] == 5000 and last[6] == 0 and last[5] > 0
    assert 0 <= worst <= 1


def test_capacity_overflow_goes_to_the_fallback(lgr):
    rng = np.random.default_rng(36)
    with knn_filter(lgr, 1):
        _dev(lgr, _rows(rng, 64), _rows(rng, 64), 64, 1)
        cap = lgr.match_knn_last()[5]
        assert 0 < cap < 2000
        t = _rows(rng, 3000 + cap + 1)
        at = rng.choice(len(t), cap + 1, replace=False)
        t[at] = t[at[0]]
        q = _rows(rng, 200)
        q[:50] = t[at[0]]
        for k, block in ((8, 1000), (2, 64)):
            _eq(_dev(lgr, q, t, block, k), ref.match(q, t, block, k), f"k={k} block={block}")
            last = lgr.match_knn_last()
            assert last[0] == 1 and last[3] >= 50 and last[2] + last[3] == 200 and last[6] == 0, last


def test_modes_return_the_same_bytes(lgr, many):
    q, t = cuda(many["q"]), cuda(many["t"])
    out = {}
    for mode in (0, 1, -1):
        with knn_filter(lgr, mode, 0):
            res = [lgr.match_knn(q, t, 2000, 8)]
            flag = lgr.match_knn_last()[0]
            ab_i, ab_d, ba_i, ba_d = lgr.match_knn2(q, t, 2000, 3)
            res += [(ab_i, ab_d), (ba_i, ba_d), lgr.match_knn(q, t, 2000, 3), lgr.match_knn(t, q, 2000, 3)]
            for k in (2, 3):
                res += [lgr.match_ratio(q, t, 2000, k), lgr.ratio_test(*lgr.match_knn(q, t, 2000, k))]
            lgr.sync()
            out[mode] = (flag, [(i.cpu().numpy(), d.cpu().numpy()) for i, d in res])
    assert [out[m][0] for m in (0, 1, -1)] == [0, 1, 0]
    for mode in (0, 1, -1):
        r = out[mode][1]
        _eq((r[0][0][many["sel"]], r[0][1][many["sel"]]), many["want"], f"mode {mode}")
        _eq(r[1], r[3], f"mode {mode}: a -> b"); _eq(r[2], r[4], f"mode {mode}: b -> a")
        _eq(r[5], r[6], f"mode {mode}: ratio k=2"); _eq(r[7], r[8], f"mode {mode}: ratio k=3")
        for got, want in zip(r, out[0][1]):
            _eq(got, want, f"mode {mode} against mode 0")


RESULT_FIELDS = ("iterations", "converged", "n_inliers", "best_iteration", "num_rejections", "estimated_iters", "n_correspondences")
RESULT_FLOATS = ("metric", "best_metric_before_refit")


def _same_result(got, want):
    np.testing.assert_array_equal(got.matrix().astype(F).view(np.uint32), want.matrix().astype(F).view(np.uint32))
    for f in RESULT_FIELDS:
        assert getattr(got, f) == getattr(want, f), f
    for f in RESULT_FLOATS:
        assert np.float32(getattr(got, f)).view(np.uint32) == np.float32(getattr(want, f)).view(np.uint32), f


@pytest.mark.parametrize("case", ["randomness3", "ratio"])
def test_pipeline_and_prepared_clouds(lgr, case):
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(4000, 12)
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    kw = dict(feature_radius=0.25, bf_block_size=1500, distance_thr=0.1, max_iterations=2000, iss_radius_src=0.02, iss_radius_tgt=0.03,
              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    if case == "ratio":
        p, desc = capi.default_params(randomness=1, matching_id=capi.MATCH_RATIO, **kw), capi.feature_params("fpfh", ratio_k=2)
    else:
        p, desc = capi.default_params(randomness=3, matching_id=0, **kw), capi.feature_params("fpfh")
    got = {}
    for mode in (0, 1):
        with knn_filter(lgr, mode):
            corr = lgr.correspondences(s, t, p, descriptor=desc).cpu().numpy()
            flag = lgr.match_knn_last()[0]
            res = lgr.align_ex2(s, t, p, descriptor=desc)
            with lgr.prepare_cloud(s, p, 0, desc) as a, lgr.prepare_cloud(t, p, 1, desc) as b:
                pcorr = lgr.correspondences_prepared(a, b, p, descriptor=desc).cpu().numpy()
                pres = lgr.align_prepared(a, b, p, descriptor=desc)
            got[mode] = (corr, res, pcorr, pres, flag)
    assert got[0][4] == 0 and got[1][4] == 1 and len(got[0][0]) > 50
    for x in (0, 2):
        assert got[0][x].shape == got[1][x].shape and (got[0][x].view(np.uint8) == got[1][x].view(np.uint8)).all()
    _same_result(got[1][1], got[0][1])
    _same_result(got[1][3], got[0][3])
    assert (got[0][0].view(np.uint8) == got[0][2].view(np.uint8)).all()


def test_host_twin(lgr):
    rng = np.random.default_rng(38)
    q, t = _rows(rng, 100), _rows(rng, 700)
    with knn_filter(lgr, 1):
        _eq(lgr.match_knn_host(q, t, 64, 5), ref.match(q, t, 64, 5))
        assert lgr.match_knn_last()[0] == 1


def test_refusals(lgr):
    import ctypes as C
    from lgr_amd import capi
    lib = capi.lib()
    try:
        for mode, check in ((-2, 0), (2, 0), (0, 2), (1, -1), (7, 7)):
            assert lib.lgr_ctx_set_knn_filter(lgr.h, mode, check) == ERR_INVALID_ARG
            assert lgr.knn_filter() == (-1, 0)
        assert lib.lgr_ctx_get_knn_filter(lgr.h, None, None) == ERR_INVALID_ARG
        assert lib.lgr_match_knn_last(lgr.h, None) == ERR_INVALID_ARG and lib.lgr_match_knn_last_check(lgr.h, None) == ERR_INVALID_ARG
        rng = np.random.default_rng(9)
        q, q34 = cuda(_rows(rng, 10)), cuda(_rows(rng, 10, 34))
        out_i, out_d = cuda(np.zeros((10, 8), np.int32)), cuda(np.zeros((10, 8), F))
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        for mode in (0, 1, -1):
            lgr.set_knn_filter(mode, 1)
            for bad_k in (0, 9, -1):
                assert lib.lgr_match_knn_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, bad_k, p(out_i), p(out_d)) == ERR_UNSUPPORTED
                assert lib.lgr_match_knn2_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, bad_k, p(out_i), p(out_d), p(out_i), p(out_d)) == ERR_UNSUPPORTED
            assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, 1, C.c_float(1.25), p(out_i), p(out_d)) == ERR_UNSUPPORTED
            for bad_len in (34, 32, 0, 351):
                assert lib.lgr_match_knn_dev(lgr.h, bad_len, p(q34), 10, p(q34), 10, 10, 2, p(out_i), p(out_d)) == ERR_UNSUPPORTED
            assert lib.lgr_match_knn_dev(lgr.h, 33, p(q), 10, p(q), 10, 0, 2, p(out_i), p(out_d)) == ERR_INVALID_ARG
            i, _ = lgr.match_knn(q, q, 10, 2)            # the context stays usable
            lgr.sync()
            assert (i.cpu().numpy()[:, 0] == np.arange(10)).all()
    finally:
        lgr.set_knn_filter(-1, 0)
