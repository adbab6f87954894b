"""The CPU statement of the TEASER alignment (tests/cpp/teaser_ref.cpp) against hand-computed answers for its steps
and against the ground truth of a synthetic problem.  The device is compared with this statement bit for bit in test_gpu_teaser.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import teaser_ref_lib as tr  # noqa: E402

SEED = 1   # of the synthetic problem: chosen so that the statement alone meets the three conditions of test_problem


def graph(K, edges):
    A = np.zeros((K, K), np.uint8)
    for u, v in edges:
        A[u, v] = A[v, u] = 1
    return A


def test_clique_k4_with_pendant_path():
    # 0..3 a K4, then the path 3 - 4 - 5: the K4 has core number 3, the path 1
    r = tr.clique(graph(6, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 4), (4, 5)]))
    assert r["core"].tolist() == [3, 3, 3, 3, 1, 1]
    assert (r["max_core"], r["n_core"]) == (3, 4)
    assert r["clique"].tolist() == [0, 1, 2, 3]


def test_clique_prism_tie_rule():
    # two triangles joined by a perfect matching: 3-regular, so V* is the whole graph and no clique.  All degrees tie: 5 leaves (largest
    # position), then 4 (degree 2, like 2 and 3), then 3 (degree 1) -- the triangle of the most reliable nodes stays.  With ties going to
    # the smallest position the answer would be [3, 4, 5].
    r = tr.clique(graph(6, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (0, 3), (1, 4), (2, 5)]))
    assert r["core"].tolist() == [3] * 6 and (r["max_core"], r["n_core"]) == (3, 6)
    assert r["clique"].tolist() == [0, 1, 2]


def test_clique_edgeless():
    r = tr.clique(graph(5, []))
    assert r["core"].tolist() == [0] * 5 and (r["max_core"], r["n_core"]) == (0, 5)
    assert r["clique"].tolist() == [0]   # everything but the most reliable node leaves: n_clique = 1 < 3, no solution


def test_tls_small():
    # the three values near 0 form the consensus: mean ((0 + 0.01) - 0.01) / 3 = 0; cost 0 + 0.2^2 + 0.2^2 + 1 (the outlier, truncated)
    shift, cost, flags = tr.tls([0.0, 0.01, -0.01, 5.0], 0.05)
    assert shift == 0.0
    assert abs(float(cost) - 1.08) < 1e-5
    assert flags.tolist() == [1, 1, 1, 0]


def test_gnc_exact_rotation_stops_after_one_solve():
    rng = np.random.default_rng(3)
    a = rng.integers(-8, 9, (12, 3)).astype(np.float32)
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)   # exact in binary32
    r = tr.gnc(a, a @ Rz.T, 0.05)
    # the residuals are rounding error, 2 max r / e2 - 1 < 0, so mu <= 0: one solve, every weight 1, no cost formed
    assert r["iterations"] == 1 and r["n_inliers"] == 12 and r["cost"] == 0.0
    assert np.array_equal(r["w"], np.ones(12, np.float32))
    assert np.abs(r["R"] - Rz).max() < 1e-5


def problem():
    from lgr_amd import synthetic
    return synthetic.make_correspondence_problem(n_pts=400, c=300, inlier_frac=0.4, seed=SEED)


def test_problem():
    pr = problem()
    beta = 0.05
    r = tr.teaser(pr["src"], pr["tgt"], pr["corr"], beta)
    truth = pr["corr"]["index_query"] == pr["corr"]["index_match"]
    assert r["rc"] == 0 and r["valid"] == 1 and r["n_nodes"] == 300
    assert r["n_clique"] >= 3 and truth[r["clique"]].all()                       # the clique holds ground-truth inliers only
    t_err = np.linalg.norm(r["T"][:3, 3].astype(np.float64) - pr["T_gt"][:3, 3])
    assert t_err < beta
    assert r["mask"][truth].all()                                                # every ground-truth inlier is in the mask
    assert r["n_inliers"] == int(r["mask"].sum())
    assert 1 <= r["rotation_iterations"] <= 100 and r["max_core"] >= r["n_clique"] - 1


def test_small_inputs_and_bad_index():
    pr = problem()
    for c in (0, 1, 2):
        r = tr.teaser(pr["src"], pr["tgt"], pr["corr"][:c], 0.05)
        assert r["rc"] == 0 and r["valid"] == 0 and r["n_nodes"] == c and np.array_equal(r["T"], np.eye(4, dtype=np.float32))
    bad = pr["corr"].copy()
    bad["index_match"][7] = pr["tgt"].shape[0]
    assert tr.teaser(pr["src"], pr["tgt"], bad, 0.05)["rc"] == -1
