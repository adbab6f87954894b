"""-m gpu: the vote among a query's candidates (lgr_vote_matches_dev, lgr_vote_matches) against tests/multiscale_ref_lib.vote, the CPU
statement of include/matching.h:327-352: widths 1, 3, 8 and 24, -1 padding, repeated candidates, candidates nearer than r, between
r and 32 r and beyond, count ties decided by the distance and full ties, where the first candidate wins."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiscale_ref_lib as ms  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ERR_INVALID_ARG = -1


def _statement(ci, cd, pts, r):
    cand = [[(int(j), F(d)) for j, d in zip(ri, rd) if j >= 0] for ri, rd in zip(ci, cd)]
    return ms.vote(cand, types.SimpleNamespace(kps=pts, iss_radius=F(r)))


def _dev(lgr, ci, cd, pts, r):
    import torch
    i, d = lgr.vote_matches(torch.from_numpy(ci).cuda(), torch.from_numpy(cd).cuda(), torch.from_numpy(pts).cuda(), r)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _case(rng, mq, width, mt, r):
    """train points in clumps: neighbours nearer than r, within 32 r and far away; rows with padding and repeats"""
    centres = rng.random((max(mt // 8, 1), 3)).astype(F) * F(200 * r)
    scale = np.where(rng.random(mt) < 0.5, 0.5 * r, 10 * r).astype(F)[:, None]
    pts = np.zeros((mt, 12), F)
    pts[:, :3] = centres[rng.integers(0, len(centres), mt)] + rng.standard_normal((mt, 3)).astype(F) * scale
    pts[:, 3:] = rng.random((mt, 9)).astype(F)
    ci = rng.integers(0, mt, (mq, width)).astype(np.int32)
    near = rng.random((mq, width)) < 0.5                         # half of the candidates from the first candidate's clump
    order = np.argsort(np.linalg.norm(pts[None, :, :3] - pts[ci[:, 0], None, :3], axis=2), axis=1)[:, :max(8, width)]
    pick = np.take_along_axis(order, rng.integers(0, order.shape[1], (mq, width)), axis=1)
    ci = np.where(near, pick, ci).astype(np.int32)
    ci[rng.random((mq, width)) < 0.15] = -1
    ci[0] = -1                                                   # a query without candidates
    if width > 1:
        ci[1, 1:] = ci[1, 0]                                     # one candidate repeated
    cd = np.round(rng.random((mq, width)) * 8).astype(F) / F(8)  # few distinct distances: ties
    cd[ci < 0] = 0
    return ci, cd, pts


@pytest.mark.parametrize("width", [1, 3, 8, 24])
def test_against_the_statement(lgr, width):
    rng = np.random.default_rng(width)
    r = 0.05
    ci, cd, pts = _case(rng, 700, width, 400, r)
    want = _statement(ci, cd, pts, r)
    _eq(_dev(lgr, ci, cd, pts, r), want[:2])
    _eq(lgr.vote_matches_host(ci, cd, pts, r), want[:2])
    assert want[0][0] == -1 and want[1][0] == 0
    if width >= 3:
        assert want[2]["count_ties"] > 0


def test_windows_and_ties(lgr):
    r = F(0.1)
    pts = np.zeros((8, 12), F)
    pts[:, 0] = [0, 0.05, 0.5, 3.19, 3.21, 100, 100, 100.05]     # nearer than r, inside 32 r, at its edge, beyond
    pts[6] = pts[5]
    rows = [([0, 1, 2], [3, 2, 1]),          # 0 sees 1 (inside r: weight 1) and 2: the largest count although the largest distance
            ([0, 3, -1], [2, 1, 0]),         # 3.19 < 3.2 counts for the first: it wins with the larger distance
            ([5, 6, 0], [2, 2, 1]),          # 5 and 6 coincide: count 2 then 1; 0 alone: count 1
            ([0, 5, -1], [2, 1, 0]),         # far apart: equal counts, the smaller distance wins
            ([0, 5, -1], [1, 1, 0]),         # a full tie: the first wins
            ([-1, 5, 0], [0, 1, 1]),         # the same behind a gap
            ([2, 2, 2], [3, 2, 1]),          # a repeated candidate: counts 3, 2, 1
            ([0, 4, -1], [2, 1, 0]),         # 3.21 does not count: equal counts, the smaller distance
            ([-1, -1, -1], [0, 0, 0])]
    ci = np.array([x[0] for x in rows], np.int32); cd = np.array([x[1] for x in rows], F)
    want = _statement(ci, cd, pts, r)
    _eq(_dev(lgr, ci, cd, pts, float(r)), want[:2])
    assert want[0].tolist() == [0, 0, 5, 5, 0, 5, 2, 4, -1]
    assert want[1].tolist() == [3, 2, 2, 1, 1, 1, 3, 1, 0]
    assert want[2]["count_ties"] >= 3 and want[2]["decisive_ties"] >= 2


def test_refusals(lgr):
    import ctypes as C
    import torch
    from lgr_amd import capi
    lib = capi.lib()
    ci = torch.tensor([[0, 1], [1, 4]], dtype=torch.int32).cuda(); cd = torch.zeros((2, 2), dtype=torch.float32).cuda()
    pts = torch.zeros((4, 12), dtype=torch.float32).cuda()
    oi = torch.zeros(2, dtype=torch.int32).cuda(); od = torch.zeros(2, dtype=torch.float32).cuda()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    call = lambda w, mt, r: lib.lgr_vote_matches_dev(lgr.h, p(ci), p(cd), 2, w, p(pts), mt, C.c_float(r), p(oi), p(od))  # noqa: E731
    assert call(2, 4, 0.1) == ERR_INVALID_ARG          # candidate 4 of 4 train points
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(1, 4, r) == ERR_INVALID_ARG
    for w in (0, 65, -1):
        assert call(w, 4, 0.1) == ERR_INVALID_ARG
    assert call(1, 4, 0.1) == 0                        # width 1 reads candidates 0 and 0 (row stride 1): valid
    lgr.sync()
