"""The CPU statement of the k-nearest brute-force matcher (tests/cpp/knn_match_ref.cpp) against the statements already in the tree --
k = 1 is oracle.match_bf on 33-d rows, shot_ref_lib.match on 352-d rows and rops_ref_lib.match on 135-d rows -- and the closed form
of DESIGN.md section 4 against the literal procedure on tie-heavy rows, where both differ from the plain (distance, index) order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as knn  # noqa: E402


def _rows(rng, m, dim):
    return rng.random((m, dim)).astype(np.float32)


def _with_specials(rng, m, dim):
    x = _rows(rng, m, dim)
    x[3] = x[1]                                  # an exact duplicate
    x[5, dim // 2] = np.nan
    x[7] = np.float32(3e38)                      # every distance to it is not below FLT_MAX
    return x


def _eq1(got, want):
    np.testing.assert_array_equal(got[0][:, 0], want[0])
    np.testing.assert_array_equal(got[1][:, 0].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("block", [10000, 7, 1])
def test_k1_is_the_oracle_matcher_on_33d(oracle, block):
    rng = np.random.default_rng(33)
    q, t = _with_specials(rng, 90, 33), _with_specials(rng, 150, 33)
    t[[20, 40, 100]] = t[2]
    q[0] = t[2]
    _eq1(knn.match(q, t, block, 1), oracle.match_bf(q, t, block))


@pytest.mark.parametrize("block", [10000, 7])
def test_k1_is_the_shot_statement_on_352d(block):
    import shot_ref_lib
    rng = np.random.default_rng(352)
    q, t = _with_specials(rng, 40, 352), _with_specials(rng, 90, 352)
    t[[20, 40, 80]] = t[2]
    q[0] = t[2]
    _eq1(knn.match(q, t, block, 1), shot_ref_lib.match(q, t, block))


@pytest.mark.parametrize("block", [10000, 7])
def test_k1_is_the_rops_statement_on_135d(block):
    import rops_ref_lib
    rng = np.random.default_rng(135)
    q, t = _with_specials(rng, 40, 135), _with_specials(rng, 90, 135)
    t[[20, 40, 80]] = t[2]
    q[0] = t[2]
    _eq1(knn.match(q, t, block, 1), rops_ref_lib.match(q, t, block))


@pytest.mark.parametrize("dim", [33, 135, 352])
def test_closed_form_is_the_procedure_on_ties(dim):
    rng = np.random.default_rng(dim)
    differs = 0
    for case in range(40):
        mt = int(rng.integers(1, 80)); mq = 12
        t = knn.tie_rows(rng, mt, dim, levels=2)
        q = knn.tie_rows(rng, mq, dim, levels=2)
        q[:min(mq, mt) // 2] = t[:min(mq, mt) // 2]
        k = int(rng.integers(1, 9)); block = int(rng.integers(1, mt + 8))
        a, b = knn.match(q, t, block, k), knn.closed(q, t, block, k)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        differs += int((a[0] != knn.plain(q, t, k)[0]).any())
    assert differs >= 10     # the two-stage order is observable on these rows


def test_lists_are_sorted_padded_and_skip_non_finite_rows():
    rng = np.random.default_rng(1)
    q, t = _with_specials(rng, 20, 33), _with_specials(rng, 30, 33)
    idx, dist = knn.match(q, t, 8, 5)
    assert (idx[5] == -1).all() and (dist[5] == 0).all()
    assert idx[7].tolist() == [7, -1, -1, -1, -1] and (dist[7] == 0).all()     # 3e38 rows: distance 0 to each other, else not below FLT_MAX
    ok = np.ones(20, bool); ok[[5, 7]] = False
    assert (idx[ok] >= 0).all() and not np.isin(idx[ok], [5, 7]).any()
    assert (np.diff(dist[ok], axis=1) >= 0).all()
    idx2, _ = knn.match(q[:4], t[:3], 2, 8)      # k above the number of train rows
    assert (idx2[:, 3:] == -1).all() and (np.sort(idx2[:, :3], axis=1) == np.arange(3)).all()
