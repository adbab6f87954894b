"""The statement the MFMA-filtered k-nearest matcher rests on, on the CPU statement tests/cpp/knn_match_ref.cpp:
the list of query i depends only on S_i = { j : d(i, j) <= D_k(i) }, D_k(i) the k-th smallest distance below FLT_MAX (the largest one
when there are fewer than k).  Rows outside S_i are masked to NaN -- a NaN row never matches, and every other row keeps its index and
its bf block -- and the two-stage procedure must return the same lists as on the unmasked train side."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as ref  # noqa: E402

CASES = [(2, 7), (4, 50), (5, 64), (8, 100), (3, 1000), (8, 3)]
FLT_MAX = np.finfo(np.float32).max


def _inputs(kind):
    rng = np.random.default_rng(41 if kind == "ties" else 42)
    if kind == "ties":
        t = ref.tie_rows(rng, 300, 33)
        q = np.concatenate([t[rng.choice(300, 20)], ref.tie_rows(rng, 10, 33)])
    else:
        t = rng.random((300, 33)).astype(np.float32)
        q = rng.random((30, 33)).astype(np.float32)
        q[:5] = t[rng.choice(300, 5)]
    t = t.copy()
    t[17] = np.nan
    t[200] = np.float32(3e38)
    return q, t


@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("k,block", CASES)
def test_the_list_depends_on_s_only(kind, k, block):
    q, t = _inputs(kind)
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
