"""The CPU statement of the ratio matcher (tests/ratio_ref_lib.py) on its own: what survives is a subset of the
one-sided matches with their index and distance bits, a larger threshold keeps a subset, equal first and k-th distances drop the key
point (inside a bf block and across one), fewer train rows than k drop every key point, and NaN rows behave as in the k-nearest
statement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as knn  # noqa: E402
import ratio_ref_lib as ratio  # noqa: E402

F = np.float32
DIMS = [33, 135, 352]


def _rows(rng, m, dim):
    return rng.random((m, dim)).astype(F)


def _clustered(rng, mq, mt, dim):
    """queries near a train row (a clear nearest neighbour) among queries with none: the test keeps some and drops some"""
    t = _rows(rng, mt, dim)
    q = _rows(rng, mq, dim)
    near = rng.choice(mq, mq // 2, replace=False)
    noise = rng.uniform(0.02, 0.4, (len(near), 1)).astype(F)          # from unmistakable to doubtful
    q[near] = t[rng.choice(mt, len(near))] + noise * rng.standard_normal((len(near), dim)).astype(F)
    return q, t


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k,block", [(2, 1000), (2, 7), (3, 64), (8, 100)])
def test_survivors_are_one_sided_matches(dim, k, block):
    rng = np.random.default_rng(dim + k)
    q, t = _clustered(rng, 120, 300, dim)
    idx, dist = ratio.match(q, t, block, k)
    one_i, one_d = knn.match(q, t, block, 1)          # what OneSidedMatcher would read
    keep = idx >= 0
    assert 0 < keep.sum() < len(q)
    np.testing.assert_array_equal(idx[keep], one_i[keep, 0])
    np.testing.assert_array_equal(dist[keep].view(np.uint32), one_d[keep, 0].view(np.uint32))
    assert (dist[~keep] == 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_larger_threshold_keeps_a_subset(dim):
    rng = np.random.default_rng(dim + 10)
    q, t = _clustered(rng, 200, 300, dim)
    lists = knn.match(q, t, 64, 3)
    kept = [ratio.ratio_test(*lists, thr)[0] >= 0 for thr in (1.0, 1.1, 1.2, 1.5, 3.0)]
    sizes = [int(x.sum()) for x in kept]
    for a, b in zip(kept, kept[1:]):
        assert not (b & ~a).any()
    assert len(q) >= sizes[0] > sizes[1] > sizes[-1] >= 0


def test_the_product_is_one_float32_multiply_and_the_compare_is_strict():
    d0 = F(1.0)
    edge = F(d0 * F(1.1))                              # the rounded product itself: not above it, so it does not pass
    above = np.nextafter(edge, F(2), dtype=F)
    idx = np.array([[4, 9], [4, 9], [4, -1], [-1, -1]], np.int32)
    dist = np.array([[d0, edge], [d0, above], [d0, 0], [0, 0]], F)
    got = ratio.ratio_test(idx, dist)
    np.testing.assert_array_equal(got[0], [-1, 4, -1, -1])
    np.testing.assert_array_equal(got[1], np.array([0, d0, 0, 0], F))
    # the product is rounded to float32 before the compare: a k-th distance equal to the rounded product never passes, though the
    # exact product of the two floats lies below it for some of these first distances
    d0 = np.linspace(0.5, 1.5, 101).astype(F)
    prod32 = (d0 * F(1.1)).astype(F)
    assert (d0.astype(np.float64) * np.float64(F(1.1)) < prod32.astype(np.float64)).any()
    table_i = np.tile(np.array([[1, 2]], np.int32), (len(d0), 1))
    assert (ratio.ratio_test(table_i, np.stack([d0, prod32], 1))[0] == -1).all()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k,block", [(2, 1000), (2, 7), (3, 7), (4, 50), (3, 1000)])
def test_equal_first_and_kth_distance_drops_the_key_point(dim, k, block):
    """tie_rows: every distinct row 3..6 times, shuffled -- a query that is one of them has >= 3 train rows at distance 0, in one bf
    block (block 1000) or spread over several (block 7: a list's first and k-th entries come from different blocks)"""
    rng = np.random.default_rng(dim + k + block)
    t = knn.tie_rows(rng, 300, dim)
    q = t[rng.choice(300, 80)]
    lists = knn.match(q, t, block, k)
    idx, dist = ratio.ratio_test(*lists)
    tied = lists[1][:, 0] == lists[1][:, k - 1]
    if k <= 3:
        assert tied.mean() > 0.9                       # (the generator's last row may be cut short of its repeats)
    assert tied.any() and (idx[tied] == -1).all() and (dist[tied] == 0).all()
    if block == 7:
        first_block, kth_block = lists[0][:, 0] // block, lists[0][:, k - 1] // block
        assert (first_block != kth_block)[tied].any()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", [2, 3, 8])
def test_fewer_train_rows_than_k_drop_every_key_point(dim, k):
    rng = np.random.default_rng(dim + 20 + k)
    q = _rows(rng, 40, dim)
    for mt in (1, k - 1):
        idx, dist = ratio.match(q, _rows(rng, mt, dim), 5, k)
        assert (idx == -1).all() and (dist == 0).all()
    idx, _ = ratio.match(q, np.concatenate([q[:1] + F(1e-3), _rows(rng, k - 1, dim) + F(5)]), 5, k)   # mt = k: a list can be full
    assert idx[0] == 0


@pytest.mark.parametrize("dim", DIMS)
def test_nan_rows_behave_as_in_the_knn_statement(dim):
    rng = np.random.default_rng(dim + 30)
    q, t = _clustered(rng, 60, 100, dim)
    q[[3, 17]] = np.nan
    q[4, dim // 2] = np.nan
    t[[30, 31]] = np.nan
    t[32, dim - 1] = np.nan
    for k, block in ((2, 1000), (3, 33)):
        lists = knn.match(q, t, block, k)
        assert (lists[0][[3, 4, 17]] == -1).all()                  # a NaN query row has an empty list
        idx, dist = ratio.ratio_test(*lists)
        assert (idx[[3, 4, 17]] == -1).all() and (dist[[3, 4, 17]] == 0).all()
        assert not np.isin(idx, [30, 31, 32]).any()                # a NaN train row is in no list
        clean = np.delete(np.arange(100), [30, 31, 32])
        i2, d2 = ratio.match(q, t[clean], 1000, k)                 # ... and (one bf block) the rest is matched as if it were not there
        if block == 1000:
            np.testing.assert_array_equal(np.where(idx >= 0, idx, -1), np.where(i2 >= 0, clean[np.maximum(i2, 0)], -1))
            np.testing.assert_array_equal(dist.view(np.uint32), d2.view(np.uint32))
    # only NaN rivals: the list is shorter than k, the key point is dropped
    t2 = np.full((3, dim), np.nan, F)
    t2[1] = q[0]
    assert (ratio.match(q, t2, 10, 2)[0] == -1).all()
