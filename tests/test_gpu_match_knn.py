"""-m gpu: the exact k-nearest brute-force matcher (lgr_match_knn_dev, lgr_match_knn2_dev, lgr_match_knn) against the CPU statement
tests/cpp/knn_match_ref.cpp: indices and distance bits of every list entry, for row lengths 33, 135 and 352 -- small shapes with
block < k, k > mt, bf blocks that straddle tiles and a single block; tie-heavy rows on which the two-stage order differs from the
plain (distance, index) one; NaN rows and a row whose distances are not below FLT_MAX; sizes of many tiles; k = 1 against the
one-match entry points of the same context; both directions against two one-direction calls; the host twin; the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DIMS = [33, 135, 352]
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5   # include/lgr.h


def _rows(rng, m, dim):
    return rng.random((m, dim)).astype(np.float32)


def _dev(lgr, q, t, block, k):
    import torch
    i, d = lgr.match_knn(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), block, k)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=what)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mq,mt", [(1, 1), (1, 65), (63, 64), (65, 129), (130, 200)])
def test_shapes(lgr, dim, mq, mt):
    rng = np.random.default_rng(dim * 1000 + mq * 7 + mt)
    q, t = _rows(rng, mq, dim), _rows(rng, mt, dim)
    if mt > 4:
        t[mt // 2] = t[0]; t[mt - 1] = t[0]          # equal distances inside and across blocks
    for k in (1, 2, 5, 8):
        for block in (3, 50, 64, mt + 7):
            _eq(_dev(lgr, q, t, block, k), ref.match(q, t, block, k), f"k={k} block={block}")


@pytest.mark.parametrize("dim", DIMS)
def test_ties_follow_the_two_stage_order(lgr, dim):
    rng = np.random.default_rng(dim + 1)
    t = ref.tie_rows(rng, 300, dim)
    q = np.concatenate([t[rng.choice(300, 60)], ref.tie_rows(rng, 40, dim)])
    differs = 0
    for k, block in ((2, 7), (4, 50), (5, 64), (8, 100), (3, 1000)):
        want = ref.match(q, t, block, k)
        differs += int((want[0] != ref.plain(q, t, k)[0]).any(axis=1).sum())
        _eq(_dev(lgr, q, t, block, k), want, f"k={k} block={block}")
    assert differs > 0                                # asserted in the statement: queries whose list is not the plain (d, index) order


@pytest.mark.parametrize("dim", DIMS)
def test_nan_rows_and_distances_not_below_flt_max(lgr, dim):
    rng = np.random.default_rng(dim + 2)
    q, t = _rows(rng, 70, dim), _rows(rng, 150, dim)
    t[[30, 31]] = np.nan
    t[32, dim - 1] = np.nan
    t[64, 0] = np.inf
    t[40] = np.float32(3e38)
    q[[3, 66]] = np.nan
    q[4, dim // 2] = np.nan
    q[5, 1] = -np.inf
    for k, block in ((1, 1000), (3, 33), (8, 64)):
        want = ref.match(q, t, block, k)
        _eq(_dev(lgr, q, t, block, k), want, f"k={k} block={block}")
        assert (want[0][[3, 4, 5, 66]] == -1).all() and not np.isin(want[0], [30, 31, 32, 40, 64]).any()


def test_many_tiles_33(lgr):
    rng = np.random.default_rng(5000)
    q, t = _rows(rng, 5000, 33), _rows(rng, 7000, 33)
    q[:500] = t[rng.choice(7000, 500)]
    t[3000:3200] = t[100:300]
    got = _dev(lgr, q, t, 2000, 8)
    sel = np.concatenate([np.arange(0, 600), rng.choice(5000, 900, replace=False)])
    want = ref.match(q[sel], t, 2000, 8)
    _eq((got[0][sel], got[1][sel]), want)


def test_many_tiles_352(lgr):
    rng = np.random.default_rng(1500)
    q, t = _rows(rng, 1500, 352), _rows(rng, 2000, 352)
    q[:200] = t[rng.choice(2000, 200)]
    _eq(_dev(lgr, q, t, 10000, 4), ref.match(q, t, 10000, 4))


@pytest.mark.parametrize("dim", DIMS)
def test_k1_is_the_one_match_entry_point(lgr, dim):
    import torch
    rng = np.random.default_rng(dim + 3)
    q, t = _rows(rng, 2000, dim), _rows(rng, 3000, dim)
    q[:300] = t[rng.choice(3000, 300)]
    t[2500:2600] = t[:100]
    tq, tt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    one = {33: lgr.match_bf, 135: lgr.match_rops, 352: lgr.match_shot}[dim]
    for block in (10000, 700):
        i1, d1 = one(tq, tt, block)
        ik, dk = lgr.match_knn(tq, tt, block, 1)
        lgr.sync()
        _eq((ik.cpu().numpy()[:, 0], dk.cpu().numpy()[:, 0]), (i1.cpu().numpy(), d1.cpu().numpy()), f"block={block}")


@pytest.mark.parametrize("dim", DIMS)
def test_both_directions_equal_two_single_runs(lgr, dim):
    import torch
    rng = np.random.default_rng(dim + 4)
    a, b = ref.tie_rows(rng, 301, dim), ref.tie_rows(rng, 205, dim)
    b[:50] = a[rng.choice(301, 50)]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for k, block in ((3, 10000), (8, 64), (2, 5)):
        ab_i, ab_d, ba_i, ba_d = [x.cpu().numpy() for x in lgr.match_knn2(ta, tb, block, k)]
        _eq((ab_i, ab_d), _dev(lgr, a, b, block, k))
        _eq((ba_i, ba_d), _dev(lgr, b, a, block, k))
        _eq((ba_i, ba_d), ref.match(b, a, block, k))


@pytest.mark.parametrize("dim", DIMS)
def test_host_entry_point(lgr, dim):
    rng = np.random.default_rng(dim + 5)
    q, t = _rows(rng, 100, dim), _rows(rng, 700, dim)
    _eq(lgr.match_knn_host(q, t, 64, 5), _dev(lgr, q, t, 64, 5))
    _eq(lgr.match_knn_host(q, t, 64, 5), ref.match(q, t, 64, 5))


def test_empty_sides(lgr):
    import torch
    q = torch.zeros((5, 33), dtype=torch.float32).cuda()
    none = torch.zeros((0, 33), dtype=torch.float32).cuda()
    i, d = lgr.match_knn(q, none, 10, 3)
    lgr.sync()
    assert (i.cpu().numpy() == -1).all() and (d.cpu().numpy() == 0).all() and i.shape == (5, 3)
    i, d = lgr.match_knn(none, q, 10, 3)
    assert i.shape == (0, 3)


def test_refusals(lgr):
    import ctypes as C
    import torch
    from lgr_amd import capi
    rng = np.random.default_rng(9)
    q = torch.from_numpy(_rows(rng, 10, 33)).cuda()
    q34 = torch.from_numpy(_rows(rng, 10, 34)).cuda()
    out_i = torch.zeros((10, 8), dtype=torch.int32).cuda(); out_d = torch.zeros((10, 8), dtype=torch.float32).cuda()
    lib = capi.lib()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    for bad_k in (0, 9, -1):
        assert lib.lgr_match_knn_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, bad_k, p(out_i), p(out_d)) == ERR_UNSUPPORTED
        assert lib.lgr_match_knn2_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, bad_k, p(out_i), p(out_d), p(out_i), p(out_d)) == ERR_UNSUPPORTED
    for bad_len in (34, 32, 0, 351):
        assert lib.lgr_match_knn_dev(lgr.h, bad_len, p(q34), 10, p(q34), 10, 10, 2, p(out_i), p(out_d)) == ERR_UNSUPPORTED
    for bad_block in (0, -5):
        assert lib.lgr_match_knn_dev(lgr.h, 33, p(q), 10, p(q), 10, bad_block, 2, p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_knn_dev(lgr.h, 33, None, 10, p(q), 10, 10, 2, p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_knn_dev(lgr.h, 33, p(q), 10, None, 10, 10, 2, p(out_i), p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_knn_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, 2, None, p(out_d)) == ERR_INVALID_ARG
    assert lib.lgr_match_knn2_dev(lgr.h, 33, p(q), 10, p(q), 10, 10, 2, p(out_i), p(out_d), None, None) == ERR_INVALID_ARG
    assert lib.lgr_match_knn(lgr.h, 33, None, 10, None, 10, 10, 2, None, None) == ERR_INVALID_ARG
    with pytest.raises(capi.LgrError, match="rc=-5"):
        lgr.match_knn(q, q, 10, 9)
    i, _ = lgr.match_knn(q, q, 10, 2)            # the context stays usable
    lgr.sync()
    assert (i.cpu().numpy()[:, 0] == np.arange(10)).all()
