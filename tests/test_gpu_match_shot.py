"""-m gpu: the exact 352-d brute-force matcher (lgr_match_shot_dev, lgr_match2_shot_dev, lgr_match_shot) against the CPU reference
tests/cpp/shot_ref.cpp: matched indices and distance bits equal, on sizes 1 .. 50 000, small bf blocks (the block tie rule), exact
duplicates inside and across blocks, NaN rows, rows one float ulp apart, 5 000 identical rows; both directions of one pass against two
single-direction runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shot_ref_lib as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(rng, m):
    x = rng.random((m, 352)).astype(np.float32) ** 4       # SHOT-like: non-negative, sparse-ish, unit norm
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _dev(lgr, q, t, block):
    import torch
    i, d = lgr.match_shot(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), block)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("mq,mt", [(1, 1), (31, 33), (33, 31), (4097, 4097), (1, 5000)])
def test_sizes(lgr, mq, mt):
    rng = np.random.default_rng(mq * 7 + mt)
    q, t = _rows(rng, mq), _rows(rng, mt)
    for block in (10000, 7):
        _eq(_dev(lgr, q, t, block), ref.match(q, t, block))


def test_50k_sampled_queries(lgr):
    rng = np.random.default_rng(50)
    q, t = _rows(rng, 50_000), _rows(rng, 50_000)
    q[:1000] = t[rng.choice(50_000, 1000)]                   # exact hits as well
    got = _dev(lgr, q, t, 200000)
    sel = rng.choice(50_000, 1500, replace=False)
    want = ref.match(q[sel], t, 200000)
    _eq((got[0][sel], got[1][sel]), want)


def test_ties_nan_and_ulp_rows(lgr):
    rng = np.random.default_rng(3)
    t = _rows(rng, 300)
    t[[10, 15, 120, 250]] = t[5]                              # duplicates inside block 0 and across blocks (block 100)
    t[200] = np.nextafter(t[5], np.float32(2))               # one ulp away in every element
    t[201] = t[5]; t[201, 17] = np.nextafter(t[5, 17], np.float32(0))
    t[[30, 31]] = np.nan
    t[32, 100] = np.nan
    q = np.concatenate([t[[5, 10, 200, 201, 30, 32]], _rows(rng, 50)])
    for block in (100, 7, 1, 1000):
        _eq(_dev(lgr, q, t, block), ref.match(q, t, block))
    i, _ = _dev(lgr, q, t, 100)
    assert i[0] == 250 and i[4] == -1 and i[5] == -1


def test_identical_rows(lgr):
    rng = np.random.default_rng(4)
    t = np.repeat(_rows(rng, 1), 5000, axis=0)
    q = np.concatenate([t[:3], _rows(rng, 3)])
    for block in (200000, 333):
        _eq(_dev(lgr, q, t, block), ref.match(q, t, block))


def test_both_directions_equal_two_single_runs(lgr):
    import torch
    rng = np.random.default_rng(5)
    a, b = _rows(rng, 3001), _rows(rng, 2050)
    b[:500] = a[rng.choice(3001, 500)]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for block in (200000, 64):
        ab_i, ab_d, ba_i, ba_d = [x.cpu().numpy() for x in lgr.match2_shot(ta, tb, block)]
        _eq((ab_i, ab_d), _dev(lgr, a, b, block))
        _eq((ba_i, ba_d), _dev(lgr, b, a, block))


def test_host_entry_point(lgr):
    rng = np.random.default_rng(6)
    q, t = _rows(rng, 100), _rows(rng, 700)
    _eq(lgr.match_shot_host(q, t, 64), ref.match(q, t, 64))
