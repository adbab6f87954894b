"""CPU: the statement of the ICP variants (tests/icp_ex_ref_lib.py: tests/cpp/icp_ex_ref.cpp + csrc/lgr_icp_math.h) -- the two shared pieces
against known answers, the neutral configuration against the point-to-plane statement bit for bit, point-to-point on a noise-free copy,
and what each option does on the half-overlapping pair where the plain step drifts.

Measured on the CPU before anything was asserted (make_pair(4000, 12), the oracle's normals, density 0.03086):

Noise-free copy (the target moved back by 3 degrees / 0.1, coordinates and normals rounded to f32 once; start: identity; max_dist 0.3):
  point-to-point  CONVERGED after 19 iterations, 4000 pairs, max |T - T_gt| entry 4.9e-7, rmse 5.5e-7
  point-to-plane  7 iterations, 4.8e-7;  plane-to-plane  5 iterations, 4.3e-7
  The floor is the f32 rounding of the inputs: coordinates up to 5.04 carry an ulp of 4.8e-7, and the transform itself is f32.  Asserted:
  max |T - T_gt| <= 4 ulp of the largest coordinate (1.9e-6), four times what was seen.

Half overlap, from the ground truth, shrink 1, max_dist = density, 60 iterations allowed (rotation error in degrees, translation error):
  point-to-plane, plain (= lgr_icp_plane)      60 it  0.9277  0.01630   drifts, as DESIGN.md section 3.1o records
  point-to-plane + Huber  k = 0.25 density     18 it  0.4501  0.00734   CONVERGED
  point-to-plane + Cauchy k = 0.25 density     16 it  0.2162  0.00267   CONVERGED
  point-to-plane + Tukey  k = 0.5 density      60 it  0.2061  0.00460
  point-to-plane + gate cos 0.97               60 it  0.1838  0.00246
  point-to-plane + Tukey 0.5 density + gate    60 it  0.1933  0.00458
  point-to-point, plain                        47 it  0.2094  0.00645   CONVERGED
  point-to-point + Huber k = 0.5 density       18 it  0.1384  0.00307   CONVERGED
  plane-to-plane, plain (eps 1e-3)              6 it  0.0760  0.00201   CONVERGED
  plane-to-plane + gate cos 0.97                7 it  0.0783  0.00211   CONVERGED
  plane-to-plane + Tukey k = 0.15              60 it  0.0709  0.00175
  (also run, not asserted: Huber at k = density changes nothing -- no residual reaches it; Huber 0.5 density 0.6998 / 0.01217; Cauchy 0.5
  density 0.3240 / 0.00524; Tukey 0.25 density 0.6099 / 0.01290; gate 0.9: 0.2349 / 0.00289, gate 0.99: 0.2151 / 0.00448; plane-to-plane
  with eps 1e-2: 0.0875 / 0.00105 without converging.)
Every configuration listed ends closer to the ground truth than the plain run.  The smallest measured gap is Huber's: 0.478 degrees and
0.0090.  Asserted for every listed configuration: at least 0.2 degrees and 0.004 closer than the plain run of the same session -- under
half the smallest gap, so that a change of the last digits of a run does not fail it while a configuration that drifts like the plain
one does."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ex_ref_lib as X  # noqa: E402
import icp_ref_lib as I  # noqa: E402
import refine_ref_lib as R  # noqa: E402

F = np.float32
U = 2.0 ** -53


def test_inv_sym3_known_answers():
    rng = np.random.default_rng(4)
    for _ in range(50):   # well conditioned: against numpy, loosely
        A = rng.normal(size=(3, 3))
        S = A @ A.T + 3.0 * np.eye(3)
        M, want = X.inv_sym3(S), np.linalg.inv(S)
        assert np.abs(M - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(M, M.T)
    # Sigma = 2 I - (1 - eps)(n n^T + m m^T) with unit n.  Exactly: m = n gives Sigma n = 2 eps n, so Sigma^-1 n = n / (2 eps), and
    # Sigma^-1 t = t / 2 for t perpendicular to n; m perpendicular to n gives Sigma n = (1 + eps) n, so Sigma^-1 n = n / (1 + eps).
    # To rounding: the condition number is 1 / eps in the first case (at most 2 in the second) and the adjugate takes a handful of
    # operations per entry: 16 units in the last place times the condition number.
    for eps in (1e-6, 1e-3, 0.1, 1.0):
        for _ in range(5):
            n = rng.normal(size=3); n /= np.linalg.norm(n)
            t = np.cross(n, rng.normal(size=3)); t /= np.linalg.norm(t)
            s = 1.0 - eps
            M = X.inv_sym3(2.0 * np.eye(3) - s * 2.0 * np.outer(n, n))
            e1, e2 = np.abs(M @ n - n / (2 * eps)).max() * 2 * eps, np.abs(M @ t - t / 2).max() * 2
            M = X.inv_sym3(2.0 * np.eye(3) - s * (np.outer(n, n) + np.outer(t, t)))
            e3 = np.abs(M @ n - n / (1 + eps)).max() * (1 + eps)
            print(eps, e1, e2, e3)
            assert e1 <= 16 * U / eps and e2 <= 16 * U / eps and e3 <= 16 * U
    assert np.array_equal(X.inv_sym3(np.diag([2.0, 4.0, 8.0])), np.diag([0.5, 0.25, 0.125]))
    for S in (np.zeros((3, 3)), np.diag([1.0, 1.0, 0.0]), np.diag([1.0, 1.0, -1.0]), np.full((3, 3), np.nan), np.diag([np.inf, 1.0, 1.0]), np.ones((3, 3))):
        assert X.inv_sym3(S) is None   # a determinant that is not finite or not > 0


def test_robust_weight_known_answers():
    k = 0.75   # (2 k)^2 / k^2 and (k / 2)^2 / k^2 are exact
    want = {X.NONE: (1.0, 1.0, 1.0, 1.0), X.HUBER: (1.0, 1.0, 1.0, 0.5), X.CAUCHY: (1.0, 0.8, 0.5, 0.2), X.TUKEY: (1.0, 0.5625, 0.0, 0.0)}
    for kind, w in want.items():
        got = tuple(X.robust_weight(kind, rho, k) for rho in (0.0, k / 2, k, 2 * k))
        assert got == w, (kind, got)
    assert X.robust_weight(X.HUBER, np.nextafter(k, 1.0), k) < 1.0 and X.robust_weight(X.TUKEY, np.nextafter(k, 0.0), k) > 0.0
    for kind in (X.HUBER, X.CAUCHY, X.TUKEY):   # a NaN residual: a weight that is not > 0
        assert not X.robust_weight(kind, np.nan, k) > 0.0
    assert X.robust_weight(X.HUBER, np.inf, k) == 0.0 and X.robust_weight(X.CAUCHY, np.inf, k) == 0.0


def test_neutral_configuration_is_the_plane_statement(oracle):
    p = R.make_pair(oracle)
    d = p["thr"]
    T_near = I.perturb(p["T_gt"], 0.5, 0.04)
    src, tgt = p["src"].copy(), p["tgt"].copy()
    src[5::97, 0] = np.nan
    tgt[3::11, 5] = np.nan    # normals
    tgt[7::13, :3] = np.nan   # points
    runs = ((p["src"], p["tgt"], dict(max_dist=2 * d, max_iterations=6)), (p["src"][:65], p["tgt"], dict(max_dist=4 * d, min_dist=0.5 * d, shrink=0.9, max_iterations=6)),
            (src, tgt, dict(max_dist=4 * d, min_dist=0.5 * d, shrink=0.9, max_iterations=9)), (p["src"][:5], p["tgt"], dict(max_dist=4 * d, max_iterations=3)),
            (p["src"][:0], p["tgt"], dict(max_dist=0.5, max_iterations=3)), (p["src"], p["tgt"], dict(max_iterations=0)))
    for s, t, kw in runs:
        a, b = I.icp(s, t, T_near, **kw), X.icp(s, t, T_near, **kw)
        assert X.bits(a) == X.bits(b), kw
    assert I.icp(*runs[0][:2], T_near, **runs[0][2])["pairs0"] > 1000


def test_point_to_point_on_a_noise_free_copy(oracle):
    """the figures of this module's docstring"""
    tgt = R.make_pair(oracle)["tgt"].copy()
    T = I.perturb(np.eye(4), 3.0, 0.1).astype(np.float64)
    Ti = np.linalg.inv(T)
    src = tgt.copy()
    src[:, :3] = (tgt[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    src[:, 4:7] = (tgt[:, 4:7].astype(np.float64) @ Ti[:3, :3].T).astype(F)
    big = float(max(np.abs(src[:, :3]).max(), np.abs(tgt[:, :3]).max()))
    ulp = float(np.spacing(F(big)))
    for v in X.VARIANTS:
        r = X.icp(src, tgt, np.eye(4, dtype=F), variant=v, max_iterations=60, max_dist=0.3)
        err = float(np.abs(r["T"].astype(np.float64) - T).max())
        print(f"variant {v}: {r['iterations']} iterations, stop {r['stop']}, pairs {r['pairs0']} -> {r['pairs']}, max |T - T_gt| {err:.3g}, rmse {r['rmse']:.3g} "
              f"(largest coordinate {big:.3f}, ulp {ulp:.3g})")
        if v == X.POINT_TO_POINT:
            assert r["stop"] == I.STOP_CONVERGED and r["pairs"] == len(src) and err <= 4 * ulp


def test_half_overlap_from_the_ground_truth(oracle):
    """the figures of this module's docstring: every listed configuration ends at least 0.2 degrees and 0.004 closer than the plain step"""
    p = R.make_pair(oracle)
    d = p["thr"]
    base = dict(max_iterations=60, max_dist=d, shrink=1.0)

    def run(name, **kw):
        r = X.icp(p["src"], p["tgt"], p["T_gt"], **dict(base, **kw))
        e = R.errors(r["T"], p["T_gt"])
        print(f"{name:44s} {r['iterations']:3d} iterations, stop {r['stop']}: {e[0]:.4f} deg {e[1]:.5f}, pairs {r['pairs0']} -> {r['pairs']}, "
              f"rmse {r['rmse0']:.5f} -> {r['rmse']:.5f}")
        return e
    plain = run("point-to-plane, plain")
    ref = I.icp(p["src"], p["tgt"], p["T_gt"], **base)
    assert R.errors(ref["T"], p["T_gt"]) == plain and plain[0] > 0.8   # lgr_icp_plane's drift (0.93 degrees)
    configs = (("point-to-plane + Huber 0.25 density", dict(robust=X.HUBER, robust_scale=0.25 * d)),
               ("point-to-plane + Cauchy 0.25 density", dict(robust=X.CAUCHY, robust_scale=0.25 * d)),
               ("point-to-plane + Tukey 0.5 density", dict(robust=X.TUKEY, robust_scale=0.5 * d)),
               ("point-to-plane + gate 0.97", dict(min_normal_cos=0.97)),
               ("point-to-plane + Tukey 0.5 density + gate 0.97", dict(robust=X.TUKEY, robust_scale=0.5 * d, min_normal_cos=0.97)),
               ("point-to-point, plain", dict(variant=X.POINT_TO_POINT)),
               ("point-to-point + Huber 0.5 density", dict(variant=X.POINT_TO_POINT, robust=X.HUBER, robust_scale=0.5 * d)),
               ("plane-to-plane, plain", dict(variant=X.PLANE_TO_PLANE)),
               ("plane-to-plane + gate 0.97", dict(variant=X.PLANE_TO_PLANE, min_normal_cos=0.97)),
               ("plane-to-plane + Tukey 0.15", dict(variant=X.PLANE_TO_PLANE, robust=X.TUKEY, robust_scale=0.15)))
    for name, kw in configs:
        e = run(name, **kw)
        assert e[0] <= plain[0] - 0.2 and e[1] <= plain[1] - 0.004, name
