"""CPU: the statement of the dense closest-plane evaluation (tests/cpp/plane_dense_ref.cpp, the reference the GPU tests compare
lgr_evaluate_plane_dense* with bit for bit) against an independent float64 numpy evaluation of src/metric.cpp:10-53,55-81,193-215 with
brute-force nearest neighbours.  Input: make_pair(2000, SEED) with the oracle's normals, the transform a small perturbation of the ground
truth, the threshold the oracle's calculatePointCloudDensity(tgt).

The inlier sets must agree except where float32 and float64 may legitimately decide differently: the float64 plane distance lies within
1e-5 x threshold of the threshold, or the two nearest squared distances lie within 1e-6 relative of each other.  Such points are left out of
the comparison; they may be at most 1 % of the source (asserted; SEED was picked so that the statement meets the cap: it leaves out
none).  rmse and metric must match to rtol 1e-5 (a serial f32 sum of n <= 2000 non-negative terms carries a relative error of at most
n x 2^-24 ~ 1.2e-4 in the worst case and ~ sqrt(n) x 2^-24 ~ 3e-6 in practice; the weighted case uses weights whose sum is of the order of
the sum of their magnitudes, so that the bound carries over)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_dense_ref_lib as P  # noqa: E402

F = np.float32
SEED = 12
N = 2000


def perturbed(T_gt, thr):
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    return (dT @ T_gt).astype(F)


@pytest.fixture(scope="module")
def case(oracle):
    from lgr_amd import synthetic
    p = synthetic.make_pair(n_points=N, seed=SEED)
    src = oracle.normals_knn(p["src"], 30, vp=p["vp_src"])
    tgt = oracle.normals_knn(p["tgt"], 30, vp=p["vp_tgt"])
    thr = float(F(oracle.cloud_density(tgt)))
    return dict(src=src, tgt=tgt, thr=thr, T=perturbed(p["T_gt"], thr))


def float64_eval(src, tgt, T, score_id, thr, weights=None):
    """-> dict(inl [ns] bool, ambiguous [ns] bool, dist [ns], value [ns] (the per-point score term, weights applied))"""
    T = np.asarray(T, np.float64)
    thr = float(thr)
    ps = src[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    tp, tn = tgt[:, :3].astype(np.float64), tgt[:, 4:7].astype(np.float64)
    d2 = ((ps[:, None, :] - tp[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(ps))
    first, second = d2[rows, order[:, 0]], d2[rows, order[:, 1]]
    nn = order[:, 0]
    in_range = first < (2 * thr) ** 2
    dist = np.abs(np.einsum("ij,ij->i", tn[nn], tp[nn] - ps))
    inl = in_range & (dist < thr)
    ambiguous = (np.abs(dist - thr) <= 1e-5 * thr) | ((second - first) <= 1e-6 * first)
    if score_id == 0:
        value = np.ones_like(dist)
    elif score_id == 1:
        value = np.abs(dist - thr) / thr
    elif score_id == 2:
        value = (dist - thr) ** 2 / thr ** 2
    else:
        value = np.exp(-dist * dist / (2 * thr * thr))
    if weights is not None:
        value = value * weights.astype(np.float64)
    return dict(inl=inl, ambiguous=ambiguous, dist=dist, value=value)


def check(case, score_id, weights=None):
    src, tgt, T, thr = case["src"], case["tgt"], case["T"], case["thr"]
    ns = len(src)
    st = P.evaluate(src, tgt, T, score_id, thr, weights)
    ref = float64_eval(src, tgt, T, score_id, thr, weights)
    st_inl = np.zeros(ns, bool)
    st_inl[st["inliers"]["index_query"]] = True
    amb = ref["ambiguous"]
    print(f"score {score_id}: statement inliers {st['n_inliers']}, float64 inliers {int(ref['inl'].sum())}, left out {int(amb.sum())} of {ns}")
    assert amb.sum() <= ns // 100                                  # the cap on what may be left out
    assert np.array_equal(st_inl[~amb], ref["inl"][~amb])
    assert ns // 10 <= st["n_inliers"] <= 9 * ns // 10              # not vacuous
    assert st["n_inliers"] == len(st["inliers"]) and (np.diff(st["inliers"]["index_query"]) > 0).all()
    assert (st["inliers"]["threshold"] == F(thr)).all() and np.array_equal(st["inliers"]["index_match"], st["nn"][st["inliers"]["index_query"]])
    # a stored distance: a handful of f32 roundings of numbers as large as the largest coordinate (the moved point, the differences)
    atol = 8 * 2.0 ** -24 * float(np.abs(tgt[:, :3]).max())
    np.testing.assert_allclose(st["inliers"]["distance"], ref["dist"][st_inl], rtol=0, atol=atol)
    member = np.where(amb, st_inl, ref["inl"])                      # left-out points follow the statement in the sums
    rmse = np.sqrt((ref["dist"][member] ** 2).mean())
    denom = float(ns) if weights is None else float(weights.astype(np.float64).sum())
    metric = ref["value"][member].sum() / denom
    print(f"  rmse {st['rmse']!r} vs {rmse!r}, metric {st['metric']!r} vs {metric!r}")
    np.testing.assert_allclose(st["rmse"], rmse, rtol=1e-5)
    np.testing.assert_allclose(st["metric"], metric, rtol=1e-5)
    np.testing.assert_allclose(st["score"], metric * denom, rtol=1e-5)
    return st


@pytest.mark.parametrize("score_id", [0, 1, 2, 3])
def test_statement_against_float64(case, score_id):
    check(case, score_id)


def test_statement_weighted_signed(case):
    """signed weights (uniform in [-0.25, 1)): the score of an inlier is value * w[idx], the metric's denominator the sum of ALL weights"""
    w = np.random.default_rng(3).uniform(-0.25, 1.0, N).astype(F)
    assert (w < 0).sum() > N // 10
    st = check(case, 2, w)
    plain = P.evaluate(case["src"], case["tgt"], case["T"], 2, case["thr"])
    assert st["n_inliers"] == plain["n_inliers"] and P.bits(st["rmse"]) == P.bits(plain["rmse"])   # weights touch the score alone
    assert np.array_equal(st["inliers"].view(np.uint32), plain["inliers"].view(np.uint32))


def test_statement_no_inlier_and_skipped_points(case):
    from lgr_amd import synthetic
    src, tgt, thr = case["src"], case["tgt"], case["thr"]
    far = synthetic.random_se3(np.random.default_rng(5)).astype(F)
    st = P.evaluate(src, tgt, far, 2, thr)
    assert st["n_inliers"] == 0 and st["rmse"] == np.finfo(F).max and st["metric"] == 0 and (st["nn"] == -1).all()
    s_bad = src.copy()
    s_bad[7, :3] = (np.nan, 0, 0)
    st = P.evaluate(s_bad, tgt, case["T"], 2, thr)
    assert st["nn"][7] == -1 and 7 not in st["inliers"]["index_query"]
