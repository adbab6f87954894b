"""CPU statement of the correspondence search with randomness = k > 1, composed from pieces that are pinned on their own, the way
tests/multiscale_ref_lib.Statement composes the one-match search: oracle features (or the SHOT / RoPS statements), the k-nearest
statement tests/cpp/knn_match_ref.cpp, multiscale_ref_lib.vote and oracle.filter_matches."""
import math
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as knn  # noqa: E402
import multiscale_ref_lib as ms  # noqa: E402

F = np.float32


def _lists(idx, dist, names_q=None, names_t=None, cand=None):
    """append every query's matches, in list order, to its candidate list; NaN query rows add nothing (their lists are empty)"""
    cand = [[] for _ in range(len(idx))] if cand is None else cand
    for a in range(len(idx)):
        qi = a if names_q is None else int(names_q[a])
        for j, d in zip(idx[a], dist[a]):
            if j >= 0:
                cand[qi].append((int(j) if names_t is None else int(names_t[j]), F(d)))
    return cand


def _side(kps, r):
    return types.SimpleNamespace(kps=kps, iss_radius=F(r))


class SingleScale:
    """feature_radius set, key points = every point: include/matching.h:172,228-248 with one level, then :294-352"""

    def __init__(self, oracle, pair, descriptor, feature_radius=0.25, nr=352, normal_k=30, scale=2.0):
        self.o, self.pair = oracle, pair
        adapter = ms.ADAPTERS[descriptor](oracle)
        level = int(math.floor(F(ms.log2f(feature_radius) / ms.log2f(scale))))
        r, v = ms.radius_voxel(level, nr, scale)
        self.rows = []
        for cloud, vp in ((pair["src"], pair["vp_src"]), (pair["tgt"], pair["vp_tgt"])):
            surf = oracle.normals_knn(oracle.downsample(cloud, float(v)), normal_k, vp=vp, normals_available=False)
            self.rows.append(adapter.rows(cloud, surf, r, vp))

    def tables(self, k, block, iss_radius):
        """(ij, dij, ji, dji, share of the source key points whose voted match is not their nearest row)"""
        s, t = self.rows
        i_st, d_st = knn.match(s, t, block, k)
        i_ts, d_ts = knn.match(t, s, block, k)
        ij, dij, _ = ms.vote(_lists(i_st, d_st), _side(self.pair["tgt"], iss_radius[1]))
        ji, dji, _ = ms.vote(_lists(i_ts, d_ts), _side(self.pair["src"], iss_radius[0]))
        moved = float(((ij != i_st[:, 0]) & (ij >= 0)).mean())
        return ij, dij, ji, dji, moved

    def correspondences(self, matching_id, k, block, iss_radius, distance_thr=0.1, cluster_k=40):
        ij, dij, ji, dji, moved = self.tables(k, block, iss_radius)
        out = self.o.filter_matches(matching_id, self.pair["src"], self.pair["tgt"], ij, dij, ji, dji, distance_thr, cluster_k)
        return out, moved


def multiscale_tables(st, k, block):
    """match_multiscale of a multiscale_ref_lib.Statement with k matches per level and key point: levels ascending, list order"""
    out = []
    for q, t in ((st.sides[0], st.sides[1]), (st.sides[1], st.sides[0])):
        cand = [[] for _ in range(len(q.kps))]
        lo, hi = max(q.min_l2, t.min_l2), min(q.max_l2, t.max_l2)
        for level in range(lo, hi + 1):
            iq, it = level - q.min_l2, level - t.min_l2
            if len(q.lists[iq]) == 0 or len(t.lists[it]) == 0:
                continue
            idx, dist = knn.match(q.rows[iq], t.rows[it], block, k)
            _lists(idx, dist, q.lists[iq], t.lists[it], cand)
        out += list(ms.vote(cand, t)[:2])
    return out
