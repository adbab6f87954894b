"""CPU: the statement of matchLocal with a k-list (tests/cpp/local_match_ref.cpp) against what is already pinned.  At (33, k = 1) it
equals the oracle's matchLocal -- the one tests/test_gpu_match_dispatch.py compares the FPFH entry point against -- on a make_pair(1500)
feature set with a real guess and a finite radius, indices and distance bits; the reference's test_knn_result known answer comes out of
its list rule; the list for k is a prefix of the list for k + 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_match_ref_lib as ref  # noqa: E402
from refine_ref_lib import perturbed  # noqa: E402


@pytest.fixture(scope="module")
def scene(oracle):
    from lgr_amd import synthetic
    pair = synthetic.make_pair(1500, seed=77)
    r = 0.25
    voxel = float(np.sqrt(np.float32(np.pi * r * r / 352.0)))
    feats = []
    for c, vp in ((pair["src"], pair["vp_src"]), (pair["tgt"], pair["vp_tgt"])):
        surf = oracle.normals_knn(oracle.downsample(c, voxel), 30, vp=vp)
        feats.append(oracle.fpfh(c, surf, r))
    fs, ft = feats[0].copy(), feats[1].copy()
    guess = perturbed(pair["T_gt"], 0.1)
    # equal descriptor distances at different spatial distances: three of the train points nearest to query 3's moved position
    moved = guess[:3, :3].astype(np.float64) @ pair["src"][3, :3] + guess[:3, 3]
    order = np.argsort(((pair["tgt"][:, :3] - moved) ** 2).sum(1))
    tied = [int(order[1]), int(order[4]), int(order[9])]   # ascending spatial distance
    ft[tied[0]] = ft[tied[1]]; ft[tied[2]] = ft[tied[1]]
    fs[3] = ft[tied[1]]
    fs[11] = np.nan                                                  # invalid query row
    ft[next(j for j in range(20, 30) if j not in tied)] = np.nan    # invalid train row
    return dict(pair=pair, fs=fs, ft=ft, guess=guess, tied=tied)


@pytest.mark.parametrize("radius", [0.08, 0.3, ref.FLT_MAX])
def test_statement_equals_the_oracle_at_33_k1(oracle, scene, radius):
    pair = scene["pair"]
    for qp, tp, q, t, G in ((pair["src"], pair["tgt"], scene["fs"], scene["ft"], scene["guess"]),
                            (pair["tgt"], pair["src"], scene["ft"], scene["fs"], oracle.inverse4(scene["guess"]))):
        si, sd, n_cand = ref.match(qp, tp, q, t, G, radius, 1, counts=True)
        oi, od = oracle.match_local(qp, tp, q, t, G, radius)
        np.testing.assert_array_equal(si[:, 0], oi)
        np.testing.assert_array_equal(ref.bits(sd[:, 0]), ref.bits(od))
        assert ((oi >= 0) == (n_cand > 0)).all() and (oi >= 0).mean() > 0.2
        if radius < 1:
            assert (oi == -1).sum() > 10   # points outside the overlap have no train point within the radius
    assert ref.match(pair["src"], pair["tgt"], scene["fs"], scene["ft"], scene["guess"], radius, 1)[0][11, 0] == -1


def test_knn_result_known_answer():
    """the reference's test_knn_result: capacity 3, adds (dist, index) = (3,3), (2,2), (4,4), (1,1), (1,5)"""
    idx, dist = ref.knn_list(3, [(3, 3), (2, 2), (4, 4), (1, 1), (1, 5)])
    assert idx == [1, 5, 2] and dist == [1.0, 1.0, 2.0]
    assert ref.knn_list(3, [(2, 9)]) == ([9], [2.0])
    assert ref.knn_list(1, [(2, 9), (2, 4), (1, 7), (1, 3)]) == ([7], [1.0])   # a later equal distance stays behind


def test_list_for_k_is_a_prefix_of_the_list_for_k_plus_1(scene):
    pair = scene["pair"]
    args = (pair["src"], pair["tgt"], scene["fs"], scene["ft"], scene["guess"], 0.3)
    prev = None
    for k in range(1, 9):
        idx, dist, n_cand = ref.match(*args, k, counts=True)
        assert ((idx >= 0).sum(1) == np.minimum(n_cand, k)).all()
        filled = idx >= 0
        assert (np.diff(dist, axis=1)[filled[:, 1:]] >= 0).all() and (dist[~filled] == 0).all()
        if prev is not None:
            np.testing.assert_array_equal(idx[:, :k - 1], prev[0])
            np.testing.assert_array_equal(ref.bits(dist[:, :k - 1]), ref.bits(prev[1]))
        prev = (idx, dist)
    # the three equal rows stand in front of query 3's list, the spatially nearer first
    assert list(prev[0][3][:3]) == scene["tied"] and (prev[1][3][:3] == 0).all()
    one = ref.match(*args, 1)
    assert one[0][3, 0] == scene["tied"][0]
