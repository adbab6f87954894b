"""-m gpu: the exact 135-d brute-force matcher (lgr_match_rops_dev, lgr_match2_rops_dev, lgr_match_rops) against the CPU reference
tests/cpp/rops_ref.cpp (OpenCV's normL2Sqr lane order for 8 blocks of 16, then the scalar tail over elements 128..134): matched
indices and distance bits equal, on sizes that are not multiples of 64, small bf blocks (the block tie rule), duplicated rows inside and
across blocks, rows that differ only in the tail, NaN rows; both directions of one pass against two single-direction runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rops_ref_lib as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(rng, m):
    x = rng.normal(size=(m, 135)).astype(np.float32)
    return (x / np.abs(x).sum(1, keepdims=True)).astype(np.float32)   # RoPS-like: signed, unit L1 norm


def _dev(lgr, q, t, block):
    import torch
    i, d = lgr.match_rops(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), block)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_l2sqr_is_not_a_plain_sum():
    rng = np.random.default_rng(0)
    a, b = _rows(rng, 2000), _rows(rng, 2000)
    got = np.array([ref.l2sqr(a[i], b[i]) for i in range(2000)])
    t = (a - b).astype(np.float32)
    seq = np.zeros(2000, np.float32)
    for j in range(135):
        seq = seq + t[:, j] * t[:, j]
    assert np.allclose(got, seq, rtol=1e-5) and (got != seq).any()


@pytest.mark.parametrize("mq,mt", [(1, 1), (31, 33), (65, 127), (4097, 4099), (1, 5000)])
def test_sizes(lgr, mq, mt):
    rng = np.random.default_rng(mq * 7 + mt)
    q, t = _rows(rng, mq), _rows(rng, mt)
    for block in (10000, 7):
        _eq(_dev(lgr, q, t, block), ref.match(q, t, block))


def test_ties_nan_and_tail_rows(lgr):
    rng = np.random.default_rng(3)
    t = _rows(rng, 300)
    t[[10, 15, 120, 250]] = t[5]                              # duplicates inside block 0 and across blocks (block 100)
    t[200] = t[5]; t[200, 130] = np.nextafter(t[5, 130], np.float32(2))   # differs in the tail only
    t[201] = t[5]; t[201, 17] = np.nextafter(t[5, 17], np.float32(0))
    t[[30, 31]] = np.nan
    t[32, 134] = np.nan                                       # NaN in the tail
    q = np.concatenate([t[[5, 10, 200, 201, 30, 32]], _rows(rng, 50)])
    for block in (100, 7, 1, 1000):
        _eq(_dev(lgr, q, t, block), ref.match(q, t, block))
    i, _ = _dev(lgr, q, t, 100)
    assert i[0] == 250 and i[4] == -1 and i[5] == -1


def test_both_directions_equal_two_single_runs(lgr):
    import torch
    rng = np.random.default_rng(5)
    a, b = _rows(rng, 3001), _rows(rng, 2050)
    b[:500] = a[rng.choice(3001, 500)]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for block in (200000, 64):
        ab_i, ab_d, ba_i, ba_d = [x.cpu().numpy() for x in lgr.match2_rops(ta, tb, block)]
        _eq((ab_i, ab_d), _dev(lgr, a, b, block))
        _eq((ba_i, ba_d), _dev(lgr, b, a, block))
        _eq((ab_i, ab_d), ref.match(a, b, block))
        _eq((ba_i, ba_d), ref.match(b, a, block))


def test_host_entry_point(lgr):
    rng = np.random.default_rng(6)
    q, t = _rows(rng, 100), _rows(rng, 700)
    _eq(lgr.match_rops_host(q, t, 64), ref.match(q, t, 64))
