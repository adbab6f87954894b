"""CPU statement of the ratio matcher (RatioMatcher::match_impl is a TODO in the reference), composed from pieces
that are pinned on their own: the k-nearest statement tests/cpp/knn_match_ref.cpp, multiscale_ref_lib.vote and
oracle.filter_matches(ONE_SIDED).  Its only arithmetic of its own is the float32 multiply and the strict compare of ratio_test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as knn  # noqa: E402
import multiscale_ref_lib as ms  # noqa: E402
import randomness_ref_lib as R  # noqa: E402

F = np.float32
THRESHOLD = 1.1      # MATCHING_RATIO_THRESHOLD include/common.h:50
ONE_SIDED = 1        # LGR_MATCH_ONE_SIDED


def ratio_test(idx, dist, threshold=THRESHOLD):
    """[mq, k] lists (list order, then -1 / 0) -> (idx [mq], dist [mq]): a list's first entry iff the list has k entries and
    float32(dist[0] * float32(threshold)) < dist[k - 1]; else -1 / 0"""
    idx = np.asarray(idx, np.int32); dist = np.asarray(dist, F)
    keep = (idx[:, 0] >= 0) & (idx[:, -1] >= 0) & ((dist[:, 0] * F(threshold)).astype(F) < dist[:, -1])
    return np.where(keep, idx[:, 0], -1).astype(np.int32), np.where(keep, dist[:, 0], F(0)).astype(F)


def match(q, t, block, k, threshold=THRESHOLD):
    """a level's candidates: the ratio test on the k-nearest lists of q's rows among t's"""
    return ratio_test(*knn.match(q, t, block, k), threshold)


def _candidates(idx, dist, names_q=None, names_t=None, cand=None):
    """the level's (at most one) candidate per query, appended to its list for the vote"""
    return R._lists(idx[:, None], dist[:, None], names_q, names_t, cand)


def _one_sided(oracle, kps_s, kps_t, ij, dij, distance_thr):
    none = np.full(len(kps_t), -1, np.int32)
    return oracle.filter_matches(ONE_SIDED, kps_s, kps_t, ij, dij, none, np.zeros(len(kps_t), F), distance_thr, 40)


def single_scale(st, oracle, k, block, iss_radius_tgt, distance_thr=0.1, threshold=THRESHOLD):
    """st: a randomness_ref_lib.SingleScale.  (correspondences, ij, dij): source -> target only, one level, the vote (the identity
    here, asserted), OneSidedMatcher's loop"""
    s, t = st.rows
    ci, cd = match(s, t, block, k, threshold)
    ij, dij, _ = ms.vote(_candidates(ci, cd), R._side(st.pair["tgt"], iss_radius_tgt))
    assert (ij == ci).all() and (dij.view(np.uint32) == cd.view(np.uint32)).all()
    return _one_sided(oracle, st.pair["src"], st.pair["tgt"], ij, dij, distance_thr), ij, dij


def multiscale(st, oracle, k, block, distance_thr=0.1, threshold=THRESHOLD):
    """st: a multiscale_ref_lib.Statement (key points 'any').  Common levels ascending, a candidate per level, the vote on the target side"""
    q, t = st.sides
    cand = [[] for _ in range(len(q.kps))]
    n_levels = 0
    for level in range(max(q.min_l2, t.min_l2), min(q.max_l2, t.max_l2) + 1):
        iq, it = level - q.min_l2, level - t.min_l2
        if len(q.lists[iq]) == 0 or len(t.lists[it]) == 0:
            continue
        ci, cd = match(q.rows[iq], t.rows[it], block, k, threshold)
        _candidates(ci, cd, q.lists[iq], t.lists[it], cand)
        n_levels += 1
    ij, dij, _ = ms.vote(cand, t)
    return _one_sided(oracle, st.kps[0], st.kps[1], ij, dij, distance_thr), ij, dij, n_levels
