"""CPU: the statement of the ground-truth evaluation (tests/cpp/analysis_ref.cpp, the reference of tests/test_gpu_analysis.py) pinned by
itself: hand-worked values on a 4-point source and a 5-point target, a NumPy brute force in float32 with the same operation order on a
3000-point pair (per-point terms, masks, counts), and r_err / t_err bit-equal to the oracle's rot_trans_diff."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref_lib as A  # noqa: E402

F = np.float32
NAN = np.nan


def pts(xyz, normals):
    out = np.zeros((len(xyz), 12), F)
    out[:, :3] = xyz
    out[:, 3] = 1
    out[:, 4:7] = normals
    out[:, 8] = 1
    return out


def translation(x, y, z):
    T = np.eye(4, dtype=F)
    T[:3, 3] = (x, y, z)
    return T


# ---------------------------------------------------------------------------------------------------- hand-worked
# thr = 0.5, so the search radius is 1 (r^2 = 1).  T_gt = identity, T = a shift of 0.375 along x; every number below is a dyadic
# rational, so the float arithmetic is exact up to the few operations named.
THR = 0.5
SRC = pts([(0, 0, 0.5), (2, 0, 0), (4.25, 0, 0), (6, 0, 0)], [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 1)])
TGT = pts([(0, 0, 0), (2, 0, 0), (4, 0, 0), (6, 0, 0.25), (10, 10, 10)], [(0, 0, 1), (0, 0, 1), (1, 0, 0), (NAN, NAN, NAN), (0, 1, 0)])
T_GT = np.eye(4, dtype=F)
T_EST = translation(0.375, 0, 0)
CORR = np.array([(0, 0, 0.0, 0.6), (1, 2, 0.0, 1.0), (2, 2, 0.0, 0.25)], A.CORR_DTYPE)
INLIERS = np.array([1, 1, 0], np.uint8)


def test_hand_point_cloud_error():
    # D = T^-1 T_gt = a shift of -0.375 along x: every point moves by 0.375, term 0.140625; sum of four 0.5625; / 4 = 0.140625; sqrt = 0.375
    assert np.array_equal(A.diff_matrix(T_EST, T_GT), translation(-0.375, 0, 0))
    r = A.overlap_rmse(SRC, TGT, T_EST, T_GT, THR)
    assert np.array_equal(r["term_pcd"], np.full(4, 0.140625, F))
    assert r["pcd_err"] == F(0.375)


def test_hand_overlap_rmse():
    # s0 (0,0,.5): nearest t0 at d2 = .25 < 1; plane z = 0: pi = (0,0,0); |g - pi| = .5, NOT > thr: kept; a = (.375,0,.5): .140625 + .25 = .390625 = .625^2
    # s1 (2,0,0): t1, on its plane: pi = g; a - pi = (.375,0,0): term .140625
    # s2 (4.25,0,0): t2 (normal x): pi = (4,0,0), |g - pi| = .25; a = (4.625,0,0): term .625^2 = .390625
    # s3 (6,0,0): t3 at d2 = .0625, its normal is NaN: skipped
    r = A.overlap_rmse(SRC, TGT, T_EST, T_GT, THR)
    assert r["idx"].tolist() == [0, 1, 2, -1]
    assert np.array_equal(r["term_ov"], np.array([0.390625, 0.140625, 0.390625, 0], F))
    assert r["overlap_size"] == 3
    assert r["overlap_rmse"] == np.sqrt(F(0.921875) / F(3))   # .390625 + .140625 + .390625 = .921875 exactly


def test_hand_normal_difference():
    # s0: t0 at distance .5, not < thr.  s1: t1 at 0, normals (0,1,0) . (0,0,1) = 0: acos = pi / 2.  s2: t2 at .25, normals equal: acos(1) = 0.
    # s3: t3 at .25, target normal_x NaN.  Two values {0, pi / 2}: rank 2 / 2 = 1 of the ascending list = pi / 2.
    nd, n, v = A.normal_difference(SRC, TGT, T_GT, THR)
    assert n == 2
    assert np.array_equal(v, np.array([-1, np.arccos(F(0)), 0, -1], F))
    assert nd == F(np.pi / 2)
    # nothing counts when the source is far away: pi
    nd, n, _ = A.normal_difference(SRC, TGT, translation(0, 0, 50), THR)
    assert n == 0 and nd == F(np.pi)


def test_hand_merge_overlaps():
    # source against target: s0 -> t0, dp = |(0,0,1) . (0,0,-.5)| = .5, not < thr: out; s1 -> t1, dp 0: in; s2 -> t2, dp .25: in;
    #   s3 -> t3, NaN normal: dp := d2 = .0625: in.
    # target against source: t0 -> s0, dp .5: out; t1 -> s1, 0: in; t2 -> s2, .25: in; t3 -> s3 (normal z), dp .25: in; t4: no neighbour.
    m = A.merge_overlaps(SRC, TGT, T_GT, THR)
    assert m["mask_src"].tolist() == [0, 1, 1, 1] and m["mask_tgt"].tolist() == [0, 1, 1, 1, 0]
    assert (m["n_overlap_src"], m["n_overlap_tgt"]) == (3, 3)
    assert m["overlap"] == F(6) / F(9)
    # overlap cloud (2,0,0) (4.25,0,0) (6,0,0) (2,0,0) (4,0,0) (6,0,.25), k = 2: densities 0, .25, .25, 0, .25, .25: sum of squares .25.
    # source: s0, s1 are each other's second neighbours at sqrt(4.25); s2, s3 at 1.75: sum = ((a a + a a) + 3.0625) + 3.0625
    a = np.sqrt(F(4.25))
    assert m["overlap_area"] == F(0.25) / (((a * a + a * a) + F(3.0625)) + F(3.0625))


def test_hand_correspondences_and_verdict():
    # (s0, t0): distance .5 < .6: correct.  (s1, t2): distance 2, not < 1.  (s2, t2): distance .25, not < .25 (strict).
    m, n, n_inl, n_ci = A.correct_correspondences(SRC, TGT, CORR, T_GT, INLIERS)
    assert m.tolist() == [1, 0, 0] and (n, n_inl, n_ci) == (1, 2, 1)
    e, m2 = A.evaluate_gt(SRC, TGT, CORR, T_EST, T_GT, THR, True, INLIERS)
    assert m2.tolist() == [1, 0, 0]
    assert (e["r_err"], e["t_err"], e["pcd_err"]) == (F(0), F(0.375), F(0.375))
    assert (e["overlap_size"], e["n_normal_overlap"], e["n_overlap"], e["n_correct_correspondences"], e["n_correct_inliers"]) == (3, 2, 6, 1, 1)
    assert e["corr_uniformity"] == F(0)   # one correspondence: every projection has one full bin, entropy 0
    assert e["overlap_rmse"] > THR and e["converged_and_overlap_ok"] == 0   # sqrt(.307) = .554
    # within thr: the verdict is `converged && overlap_rmse < thr`; a NaN error (no overlap) compares false
    e2, _ = A.evaluate_gt(SRC, TGT, CORR, translation(0.125, 0, 0), T_GT, THR, True)
    assert e2["overlap_rmse"] < THR and e2["converged_and_overlap_ok"] == 1
    assert A.evaluate_gt(SRC, TGT, CORR, translation(0.125, 0, 0), T_GT, THR, False)[0]["converged_and_overlap_ok"] == 0
    e3, _ = A.evaluate_gt(SRC, TGT, CORR, T_GT, translation(0, 0, 50), THR, True)
    assert e3["overlap_size"] == 0 and np.isnan(e3["overlap_rmse"]) and e3["converged_and_overlap_ok"] == 0


# ---------------------------------------------------------------------------------------------------- NumPy brute force
def se3(M, p):
    M = M.astype(F)
    return np.stack([M[r, 0] * p[:, 0] + (M[r, 1] * p[:, 1] + (M[r, 2] * p[:, 2] + M[r, 3])) for r in range(3)], 1)


def so3(M, n):
    M = M.astype(F)
    return np.stack([M[r, 0] * n[:, 0] + (M[r, 1] * n[:, 1] + M[r, 2] * n[:, 2]) for r in range(3)], 1)


def sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def nearest(q, p, r2=None):
    """index of the nearest row of p per row of q under (d2, index), -1 where none (within r2), and its d2"""
    d2 = sq3(q[:, None, :] - p[None, :, :])
    if r2 is not None:
        d2 = np.where(d2 < r2, d2, F(np.inf))
    j = np.argmin(d2, 1)   # the first occurrence of the minimum: the lowest index
    best = d2[np.arange(len(q)), j]
    return np.where(np.isfinite(best), j, -1), best


@pytest.fixture(scope="module")
def pair(oracle):
    from lgr_amd import synthetic
    p = synthetic.make_pair(n_points=3000, seed=7)
    src = oracle.normals_knn(p["src"], 30, vp=p["vp_src"])
    tgt = oracle.normals_knn(p["tgt"], 30, vp=p["vp_tgt"])
    thr = 2 * float(oracle.cloud_density(tgt))
    rng = np.random.default_rng(3)
    ang = np.deg2rad(0.5)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    dT = np.eye(4)
    dT[:3, :3] = R
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    T = (dT @ p["T_gt"]).astype(F)
    # correspondences: half of them true nearest neighbours under the ground truth, half random
    g = se3(p["T_gt"].astype(F), src[:, :3])
    j, _ = nearest(g[:600], tgt[:, :3])
    corr = np.zeros(600, A.CORR_DTYPE)
    corr["index_query"] = np.arange(600)
    corr["index_match"] = np.where(np.arange(600) % 2 == 0, j, rng.integers(0, len(tgt), 600))
    corr["threshold"] = thr
    return dict(src=np.ascontiguousarray(src, F), tgt=np.ascontiguousarray(tgt, F), T=T, T_gt=p["T_gt"].astype(F), thr=F(thr), corr=corr,
                inl=(rng.random(600) < 0.5).astype(np.uint8))


def test_bruteforce_overlap_terms(pair):
    src, tgt, T, G, thr = pair["src"], pair["tgt"], pair["T"], pair["T_gt"], pair["thr"]
    r = A.overlap_rmse(src, tgt, T, G, thr)
    P = src[:, :3]
    g, a, b = se3(G, P), se3(T, P), se3(A.diff_matrix(T, G), P)
    assert np.array_equal(A.bits(r["term_pcd"]), A.bits(sq3(P - b)))
    radius = F(2) * thr
    j, _ = nearest(g, tgt[:, :3], radius * radius)
    q, n = tgt[j, :3], tgt[j, 4:7]
    s = dot3(g - q, n)
    pi = g - s[:, None] * n
    keep = (j >= 0) & np.isfinite(n).all(1) & ~(np.sqrt(sq3(g - pi)) > thr)
    d = np.sqrt(sq3(a - pi))
    assert keep.sum() >= len(src) // 10
    assert np.array_equal(r["idx"], np.where(keep, j, -1))
    assert np.array_equal(A.bits(r["term_ov"]), A.bits(np.where(keep, d * d, F(0))))
    assert r["overlap_size"] == keep.sum()
    seq = F(0)
    for t in r["term_ov"]:
        seq = F(seq + t)
    assert r["overlap_rmse"] == np.sqrt(seq / F(keep.sum()))


def test_bruteforce_normal_difference(pair):
    src, tgt, G, thr = pair["src"], pair["tgt"], pair["T_gt"], pair["thr"]
    nd, n, v = A.normal_difference(src, tgt, G, thr)
    al = A.align(src, G)
    assert np.array_equal(A.bits(al[:, :3]), A.bits(se3(G, src[:, :3]))) and np.array_equal(A.bits(al[:, 4:7]), A.bits(so3(G, src[:, 4:7])))
    j, d2 = nearest(al[:, :3], tgt[:, :3])
    ok = (np.sqrt(d2) < thr) & np.isfinite(al[:, 4]) & np.isfinite(tgt[j, 4])
    cs = np.clip(dot3(al[:, 4:7], tgt[j, 4:7]), F(-1), F(1))
    assert ok.sum() >= len(src) // 10 and n == ok.sum()
    assert np.array_equal(v >= 0, ok)
    # numpy's arccos is not the statement's acosf: the angles agree to a few ulp, the counted set and the rank are exact
    assert np.allclose(v[ok], np.abs(np.arccos(cs[ok])), rtol=0, atol=4e-7)
    assert nd == np.sort(v[ok])[n // 2]


def test_bruteforce_merge_overlaps(pair, oracle):
    src, tgt, G, thr = pair["src"], pair["tgt"], pair["T_gt"], pair["thr"]
    m = A.merge_overlaps(src, tgt, G, thr)
    al = A.align(src, G)
    radius = F(2) * thr

    def one(cmp, ref):
        j, d2 = nearest(cmp[:, :3], ref[:, :3], radius * radius)
        dp = np.abs(dot3(ref[j, 4:7], ref[j, :3] - cmp[:, :3]))
        dp = np.where(np.isfinite(dp), dp, d2)
        return ((j >= 0) & (dp < thr)).astype(np.uint8)
    ms, mt = one(al, tgt), one(tgt, al)
    assert np.array_equal(m["mask_src"], ms) and np.array_equal(m["mask_tgt"], mt)
    assert (m["n_overlap_src"], m["n_overlap_tgt"]) == (ms.sum(), mt.sum()) and ms.sum() >= len(src) // 10
    assert m["overlap"] == F(ms.sum() + mt.sum()) / F(len(src) + len(tgt))
    # the densities are the oracle's calculateSmoothedDensities (k = 2); the sums are sequential
    ov = np.concatenate([al[ms.astype(bool)], tgt[mt.astype(bool)]])

    def ssq(d):
        s = F(0)
        for x in d.astype(F):
            s = F(s + F(x * x))
        return s
    assert m["overlap_area"] == ssq(oracle.smoothed_densities(ov, 2)) / ssq(oracle.smoothed_densities(src, 2))


def test_bruteforce_correspondences(pair):
    src, tgt, G, corr = pair["src"], pair["tgt"], pair["T_gt"], pair["corr"]
    m, n, n_inl, n_ci = A.correct_correspondences(src, tgt, corr, G, pair["inl"])
    e = np.sqrt(sq3(se3(G, src[corr["index_query"], :3]) - tgt[corr["index_match"], :3]))
    ok = e < corr["threshold"]
    assert np.array_equal(m, ok.astype(np.uint8)) and n == ok.sum() and n >= 20
    assert n_inl == pair["inl"].sum() and n_ci == (ok & (pair["inl"] > 0)).sum()
    ev, m2 = A.evaluate_gt(src, tgt, corr, pair["T"], G, pair["thr"], True, pair["inl"])
    assert np.array_equal(m2, m) and ev["n_correct_correspondences"] == n and ev["n_correct_inliers"] == n_ci
    assert 0 < ev["corr_uniformity"] <= 1
    assert ev["converged_and_overlap_ok"] == 1   # T is 0.5 degrees and 0.3 thr from the ground truth


def test_rot_trans_diff_equals_oracle(pair, oracle):
    rng = np.random.default_rng(11)
    from lgr_amd import synthetic
    cases = [(pair["T"], pair["T_gt"]), (pair["T_gt"], pair["T_gt"]), (T_EST, T_GT)]
    cases += [(synthetic.random_se3(rng).astype(F), synthetic.random_se3(rng).astype(F)) for _ in range(20)]
    for T1, T2 in cases:
        a, t = A.rot_trans_diff(T1, T2)
        oa, ot = oracle.rot_trans_diff(T1, T2)
        assert A.bits(a) == A.bits(F(oa)) and A.bits(t) == A.bits(F(ot))
