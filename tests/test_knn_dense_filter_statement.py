"""What the MFMA-filtered k-nearest matcher of 135- and 352-float rows rests on, without a GPU.

The lemma, on the CPU statement tests/cpp/knn_match_ref.cpp at the long row lengths: the list of query i depends only on
S_i = { j : d(i, j) <= D_k(i) } (test_knn_filter_statement.py's construction: rows outside S_i are masked to NaN, every other row keeps
its index and bf block).

The group bound, on a numpy model of the two sweeps: F is any value within E of the exact d2, a group is 16 consecutive train rows
(padding at +inf), U_i = (the k-th smallest group minimum of F + E) (1 + 1e-5), C_i = { j : F - E <= U_i }.  Then C_i contains S_i for
every query that has k finite groups; the others are flagged for the fallback."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as ref  # noqa: E402

CASES = [(2, 7), (4, 50), (5, 64), (8, 100), (3, 1000), (8, 3)]   # test_knn_filter_statement.py's
FLT_MAX = np.finfo(np.float32).max
DIMS = (135, 352)


def _inputs(kind, dim):
    rng = np.random.default_rng(41 if kind == "ties" else 42)
    if kind == "ties":
        t = ref.tie_rows(rng, 300, dim)
        q = np.concatenate([t[rng.choice(300, 20)], ref.tie_rows(rng, 10, dim)])
    else:
        t = rng.random((300, dim)).astype(np.float32)
        q = rng.random((30, dim)).astype(np.float32)
        q[:5] = t[rng.choice(300, 5)]
    t = t.copy()
    t[17] = np.nan
    t[200] = np.float32(3e38)
    return q, t


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("k,block", CASES)
def test_the_list_depends_on_s_only(kind, k, block, dim):
    q, t = _inputs(kind, dim)
    want = ref.match(q, t, block, k)
    full_i, full_d = ref.plain(q, t, len(t))           # every distance below FLT_MAX, ascending; then -1
    masked_rows = 0
    for i in range(len(q)):
        n = int((full_i[i] >= 0).sum())
        keep = np.zeros(len(t), bool)
        if n:
            d_k = full_d[i][min(k, n) - 1]
            assert d_k < FLT_MAX
            keep[full_i[i][:n][full_d[i][:n] <= d_k]] = True
        tm = t.copy()
        tm[~keep] = np.nan
        masked_rows += int((~keep).sum())
        got = ref.match(q[i:i + 1], tm, block, k)
        np.testing.assert_array_equal(got[0][0], want[0][i], err_msg=f"query {i}")
        np.testing.assert_array_equal(got[1][0].view(np.uint32), want[1][i].view(np.uint32), err_msg=f"query {i}")
    assert masked_rows > len(q) * len(t) // 2             # the mask removed most of the train side


GROUP = 16
EPS = {352: 1.4e-4, 135: 6e-5}   # DenseF<NB, TAIL>::EPS


def _model(q, t, k, rng, eps):
    """(covered, flagged, candidates): per query whether C_i contains S_i, whether it has fewer than k finite groups, and |C_i|"""
    mq, mt = len(q), len(t)
    d2 = ((q[:, None, :].astype(np.float64) - t[None, :, :].astype(np.float64)) ** 2).sum(-1)
    x, y = np.linalg.norm(q, axis=1), np.linalg.norm(t, axis=1)
    mtp = -(-mt // GROUP) * GROUP
    y_grp = np.zeros(mtp); y_grp[:mt] = y
    y_grp = np.repeat(y_grp.reshape(-1, GROUP).max(1), GROUP)[:mt]      # the norm bound of a row's group (the kernels': of its 32-row tile)
    s = x[:, None] + y_grp[None, :]
    E = eps * s * s + 2.5e-3 * s + 1e-5
    # the adversary: rows of S_i look as far as the bound allows, every other row as near as it allows
    d_k = np.sort(d2, axis=1)[:, min(k, mt) - 1]
    in_s = d2 <= d_k[:, None]
    Fv = np.where(in_s, d2 + E, d2 - E)
    Fv = np.where(rng.random(d2.shape) < 0.1, d2 + (2 * rng.random(d2.shape) - 1) * E, Fv)   # and some anywhere inside it
    up = np.full((mq, mtp), np.inf); up[:, :mt] = Fv + E
    grp = np.sort(up.reshape(mq, -1, GROUP).min(2), axis=1)
    flagged = np.full(mq, grp.shape[1] < k) if grp.shape[1] < k else ~np.isfinite(grp[:, k - 1])
    U = np.where(flagged, -np.inf, grp[:, min(k, grp.shape[1]) - 1] * (1 + 1e-5))
    cand = Fv - E <= U[:, None]
    covered = (cand | ~in_s).all(1)
    return covered, flagged, cand.sum(1)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", range(1, 9))
def test_the_group_bound_covers_s(k, dim):
    rng = np.random.default_rng(100 * dim + k)
    for mt in (max(1, GROUP * (k - 1) - 3), max(1, GROUP * k - 9), GROUP * k - GROUP + 1, GROUP * k + 40, 700):   # below and above 16 k rows, fewer than k groups
        t = rng.random((mt, dim)).astype(np.float32) ** 4
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        q = rng.random((40, dim)).astype(np.float32) ** 4
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q[:10] = t[rng.choice(mt, 10)]
        q *= 1000.0; t *= 1000.0                                                         # the scale 2^s of unit rows: |X| near 2^10
        covered, flagged, n_cand = _model(q, t, k, rng, EPS[dim])
        n_groups = -(-mt // GROUP)
        assert flagged.all() if n_groups < k else not flagged.any(), (mt, k)
        assert covered[~flagged].all(), (mt, k)
        assert (n_cand[flagged] == 0).all()
        if mt == 700:
            assert n_cand.max() < mt                                                      # the bound does cut
