"""-m gpu: the ratio test on the k-nearest lists -- lgr_match_ratio_dev (fused into the sweep's merge) and lgr_ratio_test_dev (on a
caller's table) against the CPU statement tests/ratio_ref_lib.py, index and distance bits; the fused form against lgr_match_knn_dev +
lgr_ratio_test_dev; the host twins.  Row lengths 33, 135 and 352; mq around the 64-row tile and many tiles; mt of 1, k - 1, k, 100 and
1000; bf blocks that cut tiles (7, 100), equal the tile (64) and hold everything; tie-heavy rows; NaN rows on either side; the
refusals.  The reference lists are computed once per (rows, block, k) for 1000 queries; smaller mq are its prefixes (a query's list
does not depend on the other queries)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as knn  # noqa: E402
import ratio_ref_lib as ratio  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
DIMS = [33, 135, 352]
MQS = [1, 63, 64, 65, 1000]
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5   # include/lgr.h


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _eq(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what)


def _rows(rng, mq, mt, dim):
    """half of the queries lie near a train row, from unmistakable to doubtful: the test keeps some and drops some"""
    t = rng.random((mt, dim)).astype(F)
    q = rng.random((mq, dim)).astype(F)
    near = np.arange(0, mq, 2)
    noise = rng.uniform(0.02, 0.4, (len(near), 1)).astype(F)
    q[near] = t[rng.choice(mt, len(near))] + noise * rng.standard_normal((len(near), dim)).astype(F)
    return q, t


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", [2, 3, 8])
def test_shapes(lgr, dim, k):
    rng = np.random.default_rng(dim * 10 + k)
    q, t_all = _rows(rng, 1000, 1000, dim)
    tq = cuda(q)
    kept = 0
    for mt in sorted({1, k - 1, k, 100, 1000}):
        t = t_all[:mt]
        tt = cuda(t)
        for block in (7, 64, 100, mt + 5):
            want = ratio.match(q, t, block, k)
            kept += int((want[0] >= 0).sum())
            if mt < k:
                assert (want[0] == -1).all()
            for mq in MQS:
                what = f"mt={mt} block={block} mq={mq}"
                got = host(lgr.match_ratio(tq[:mq], tt, block, k))
                _eq(got, (want[0][:mq], want[1][:mq]), what)
                two_step = host(lgr.ratio_test(*lgr.match_knn(tq[:mq], tt, block, k)))
                _eq(got, two_step, what)
    assert kept > 1000                                  # the test passes for a good share of the near queries


@pytest.mark.parametrize("dim", DIMS)
def test_other_thresholds(lgr, dim):
    rng = np.random.default_rng(dim + 1)
    q, t = _rows(rng, 130, 200, dim)
    tq, tt = cuda(q), cuda(t)
    sizes = []
    for thr in (1.0, 1.2, 2.5):
        want = ratio.match(q, t, 64, 3, thr)
        _eq(host(lgr.match_ratio(tq, tt, 64, 3, thr)), want, f"thr={thr}")
        _eq(host(lgr.ratio_test(*lgr.match_knn(tq, tt, 64, 3), thr)), want, f"thr={thr}")
        sizes.append(int((want[0] >= 0).sum()))
    assert sizes[0] > sizes[1] > sizes[2]


@pytest.mark.parametrize("dim", DIMS)
def test_ties_drop_the_key_point(lgr, dim):
    """equal first and k-th distances, inside one bf block and with the two entries in different blocks"""
    rng = np.random.default_rng(dim + 2)
    t = knn.tie_rows(rng, 300, dim)
    q = np.concatenate([t[rng.choice(300, 60)], knn.tie_rows(rng, 40, dim)])
    tq, tt = cuda(q), cuda(t)
    tied = 0
    for k, block in ((2, 7), (2, 1000), (3, 7), (3, 64), (4, 50), (8, 100)):
        lists = knn.match(q, t, block, k)
        want = ratio.ratio_test(*lists)
        same = (lists[0][:, k - 1] >= 0) & (lists[1][:, 0] == lists[1][:, k - 1])
        assert (want[0][same] == -1).all()
        tied += int(same.sum())
        _eq(host(lgr.match_ratio(tq, tt, block, k)), want, f"k={k} block={block}")
        _eq(host(lgr.ratio_test(cuda(lists[0]), cuda(lists[1]))), want, f"k={k} block={block}")
    assert tied > 100


@pytest.mark.parametrize("dim", DIMS)
def test_nan_rows_on_either_side(lgr, dim):
    rng = np.random.default_rng(dim + 3)
    q, t = _rows(rng, 70, 150, dim)
    t[[30, 31]] = np.nan
    t[32, dim - 1] = np.nan
    t[64, 0] = np.inf
    t[40] = F(3e38)
    q[[3, 66]] = np.nan
    q[4, dim // 2] = np.nan
    q[5, 1] = -np.inf
    tq, tt = cuda(q), cuda(t)
    for k, block in ((2, 1000), (3, 33), (8, 64)):
        want = ratio.match(q, t, block, k)
        assert (want[0][[3, 4, 5, 66]] == -1).all() and not np.isin(want[0], [30, 31, 32, 40, 64]).any() and (want[0] >= 0).any()
        _eq(host(lgr.match_ratio(tq, tt, block, k)), want, f"k={k} block={block}")
    # a train side of NaN rows but one: every list is shorter than 2
    t2 = np.full((5, dim), np.nan, F)
    t2[2] = q[0]
    got = host(lgr.match_ratio(tq, cuda(t2), 64, 2))
    assert (got[0] == -1).all() and (got[1] == 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_host_twins(lgr, dim):
    rng = np.random.default_rng(dim + 4)
    q, t = _rows(rng, 100, 700, dim)
    want = ratio.match(q, t, 64, 3)
    _eq(lgr.match_ratio_host(q, t, 64, 3), want)
    lists = knn.match(q, t, 64, 3)
    _eq(lgr.ratio_test_host(*lists), want)
    _eq(host(lgr.match_ratio(cuda(q), cuda(t), 64, 3)), want)


def test_empty_sides_write_nothing_or_drop_everything(lgr):
    import torch
    lib = lgr_lib()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    q = torch.rand((5, 33), dtype=torch.float32).cuda()
    out_i = torch.full((5,), 77, dtype=torch.int32).cuda(); out_d = torch.full((5,), 7.0, dtype=torch.float32).cuda()
    thr = C.c_float(1.1)
    assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 0, p(q), 5, 10, 2, thr, p(out_i), p(out_d)) == 0
    assert lib.lgr_match_ratio_dev(lgr.h, 33, None, 0, p(q), 5, 10, 2, thr, None, None) == 0
    assert lib.lgr_ratio_test_dev(lgr.h, p(out_i), p(out_d), 0, 2, thr, p(out_i), p(out_d)) == 0
    assert lib.lgr_ratio_test_dev(lgr.h, None, None, 0, 2, thr, None, None) == 0
    assert lib.lgr_match_ratio(lgr.h, 33, None, 0, None, 0, 10, 2, thr, None, None) == 0
    assert lib.lgr_ratio_test(lgr.h, None, None, 0, 2, thr, None, None) == 0
    lgr.sync()
    assert (out_i.cpu().numpy() == 77).all() and (out_d.cpu().numpy() == 7.0).all()         # mq = 0 wrote nothing
    none = torch.zeros((0, 33), dtype=torch.float32).cuda()
    i, d = host(lgr.match_ratio(q, none, 10, 2))                                            # no train row: nothing passes
    assert (i == -1).all() and (d == 0).all() and i.shape == (5,)


def lgr_lib():
    from lgr_amd import capi
    return capi.lib()


def test_refusals(lgr):
    import torch
    from lgr_amd import capi
    lib = lgr_lib()
    rng = np.random.default_rng(9)
    q = cuda(rng.random((10, 33)).astype(F))
    q34 = cuda(rng.random((10, 34)).astype(F))
    out_i = torch.zeros((10,), dtype=torch.int32).cuda(); out_d = torch.zeros((10,), dtype=torch.float32).cuda()
    ki = torch.zeros((10, 8), dtype=torch.int32).cuda(); kd = torch.zeros((10, 8), dtype=torch.float32).cuda()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    thr = C.c_float(1.1)
    for bad_k in (1, 9, 0, -1):
        assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, bad_k, thr, p(out_i), p(out_d)) == ERR_UNSUPPORTED
        assert lib.lgr_ratio_test_dev(lgr.h, p(ki), p(kd), 10, bad_k, thr, p(out_i), p(out_d)) == ERR_UNSUPPORTED
        assert lib.lgr_match_ratio(lgr.h, 33, p(q), 10, p(q), 10, 10, bad_k, thr, p(out_i), p(out_d)) == ERR_UNSUPPORTED
        assert lib.lgr_ratio_test(lgr.h, p(ki), p(kd), 10, bad_k, thr, p(out_i), p(out_d)) == ERR_UNSUPPORTED
    for bad_len in (34, 32, 0, 351):
        assert lib.lgr_match_ratio_dev(lgr.h, bad_len, p(q34), 10, p(q34), 10, 10, 2, thr, p(out_i), p(out_d)) == ERR_UNSUPPORTED
    for bad_block in (0, -5):
        assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, p(q), 10, bad_block, 2, thr, p(out_i), p(out_d)) == ERR_INVALID_ARG
    for bad_thr in (float("nan"), float("inf"), 0.0, -1.0):
        assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, 2, C.c_float(bad_thr), p(out_i), p(out_d)) == ERR_INVALID_ARG
        assert lib.lgr_ratio_test_dev(lgr.h, p(ki), p(kd), 10, 2, C.c_float(bad_thr), p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_ratio_dev(lgr.h, 33, None, 10, p(q), 10, 10, 2, thr, p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, None, 10, 10, 2, thr, p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, 2, thr, None, p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_ratio_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, 2, thr, p(out_i), None) == ERR_INVALID_ARG
    assert lib.lgr_match_ratio_dev(None, 33, p(q), 10, p(q), 10, 10, 2, thr, p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_ratio(lgr.h, 33, None, 10, None, 10, 10, 2, thr, None, None) == ERR_INVALID_ARG
    for args in ((None, p(kd), p(out_i), p(out_d)), (p(ki), None, p(out_i), p(out_d)), (p(ki), p(kd), None, p(out_d)), (p(ki), p(kd), p(out_i), None)):
        assert lib.lgr_ratio_test_dev(lgr.h, args[0], args[1], 10, 2, thr, args[2], args[3]) == ERR_INVALID_ARG
        assert lib.lgr_ratio_test(lgr.h, args[0], args[1], 10, 2, thr, args[2], args[3]) == ERR_INVALID_ARG
    with pytest.raises(capi.LgrError, match="rc=-5"):
        lgr.match_ratio(q, q, 10, 9)
    i, _ = lgr.match_ratio(torch.cat([q, q + 5]), q, 10, 2)   # the context stays usable
    lgr.sync()
    assert (i.cpu().numpy()[:10] == np.arange(10)).all()
