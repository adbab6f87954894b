"""CPU: the statement of the point-to-plane ICP (tests/icp_ref_lib.py: tests/cpp/icp_ref.cpp + csrc/lgr_icp_math.h) -- its tree sum, its
solve and its rotation against numpy, its stop reasons, and what it reaches on make_pair(4000, 12) with the oracle's normals from the
ground truth perturbed by 5 degrees / 0.3 and by 0.5 degrees / 4 cm (rotation about (1, 2, 3) / |.|, shift along (0.6, 0, 0.8):
icp_ref_lib.perturb).

The pair overlaps by half and is a height field, so its in-plane motions are weakly held; what the statement reaches depends on the
pairing distances (measured on the CPU before anything was asserted, density = the target's, 0.03086):
  5 deg / 0.3 (errors 5.000 deg, 0.3414 at the start), max_dist 8 x density, shrink 0.85, min_dist 0.5 x density: CONVERGED after 37
      iterations at 0.270 deg, 0.0057 (6 x density and shrink 0.9 reach the same pose; 2, 3, 4 and 10 x density do not converge from there).
      lgr_refine_plane's statement from the same start (MSE, threshold = density, 40 steps): 24.81 deg, 0.2478 -- it does not get there.
  0.5 deg / 4 cm (0.4999 deg, 0.0435), max_dist 0 = 4 x density, shrink 0.9, min_dist 0.5 x density: CONVERGED after 37 iterations at
      0.270 deg, 0.0057.  The refinement's statement from the same start: 13 steps, 0.161 deg, 0.0056.
  10 deg / 0.3 converges (0.271 deg, 0.0057) with max_dist 10 x density, shrink 0.9 and with none of the smaller distances tried: not asserted.
Without a shrinking distance (shrink 1) the statement drifts on this pair even from the ground truth (0.93 deg at max_dist = density after
60 iterations): pairs across the overlap's edge pull along the weakly held motions."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref_lib as I  # noqa: E402
import refine_ref_lib as R  # noqa: E402

F = np.float32
MSE = 2


def test_tree_sum_against_fsum():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 64, 65, 4096, 5000):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
        want, got = math.fsum(x), I.tree_sum(x)
        print(n, got, want)
        assert abs(got - want) <= 13 * 2.0 ** -53 * float(np.abs(x).sum())   # one rounding per level, at most 13 levels, each within 2^-53 of sum |x|
    x = rng.uniform(0.5, 1.5, 5000)   # the bound of the statement's users: positive terms, relative to the sum itself
    assert abs(I.tree_sum(x) - math.fsum(x)) <= 1e-12 * math.fsum(x)
    # the tree is the declared one: pairs first, the padding on the right
    x = np.array([1e16, 1.0, -1e16, 1.0, 1.0])
    assert I.tree_sum(x) == ((1e16 + 1.0) + (-1e16 + 1.0)) + ((1.0 + 0.0) + (0.0 + 0.0))
    assert math.copysign(1.0, I.tree_sum(np.array([-0.0]))) == -1.0 and math.copysign(1.0, I.tree_sum(np.array([-0.0, -0.0, -0.0]))) == 1.0


def test_solve_against_numpy():
    rng = np.random.default_rng(2)
    for _ in range(20):
        M = rng.normal(size=(6, 6))
        A = M @ M.T + 6.0 * np.eye(6)   # condition number of a few tens at most
        b = rng.normal(size=6)
        xi, want = I.solve(A, b), np.linalg.solve(A, -b)
        assert np.abs(xi - want).max() <= 1e-9 * np.abs(want).max()
    A[2] = 0; A[:, 2] = 0   # a direction nothing holds
    assert I.solve(A, b) is None
    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 5e-13])   # the pivot rule: not > 1e-12 x the largest diagonal entry
    assert I.solve(A, b) is None and I.solve(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 2e-12]), b) is not None
    assert I.solve(np.full((6, 6), np.nan), b) is None


def test_rotation():
    assert np.array_equal(I.rotation([0.0, 0.0, 0.0]), np.eye(3))
    rng = np.random.default_rng(3)
    for scale in (1e-6, 1e-2, 0.3, 2.0):
        w = rng.normal(size=3) * scale
        Rm = I.rotation(w)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rm) - 1) <= 1e-15
        ang = 2 * np.arctan(np.linalg.norm(w) / 2)   # the angle of (1, w / 2): |w| to second order
        assert abs(np.arccos(np.clip((np.trace(Rm) - 1) / 2, -1, 1)) - ang) <= 1e-7 and np.abs(Rm @ w - w).max() <= 1e-15 * scale * 10


def plane_lattice():
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2).astype(F)
    t = np.zeros((len(g), 12), F)
    t[:, :2] = g; t[:, 3] = 1; t[:, 6] = 1; t[:, 8] = 1
    s = t.copy()
    s[:, :2] += F(0.25); s[:, 2] = F(0.125)
    return s, t


def test_stop_reasons(oracle):
    s, t = plane_lattice()
    r = I.icp(s, t, np.eye(4, dtype=F), max_iterations=5, max_dist=1.0)
    assert (r["iterations"], r["stop"], r["pairs"], len(r["trace"])) == (0, I.STOP_DEGENERATE, 400, 1)
    assert np.array_equal(r["T"], np.eye(4, dtype=F)) and abs(float(r["rmse"]) - 0.125) < 1e-7
    p = R.make_pair(oracle)
    r = I.icp(p["src"], p["tgt"], p["T_far"], max_iterations=5, max_dist=2 * p["thr"])   # out of reach
    assert (r["iterations"], r["stop"], r["pairs"], len(r["trace"])) == (0, I.STOP_NO_PAIRS, 0, 1) and r["rmse"] == I.FLT_MAX
    assert np.array_equal(I.u32(r["T"]), I.u32(p["T_far"]))
    r = I.icp(p["src"][:5], p["tgt"], p["T_gt"], max_iterations=5, max_dist=4 * p["thr"])   # fewer than six pairs can exist
    assert r["stop"] == I.STOP_NO_PAIRS and r["iterations"] == 0
    r = I.icp(p["src"], p["tgt"], p["T_far"], max_iterations=0)
    assert (r["iterations"], r["stop"], r["trace"], r["pairs"]) == (0, I.STOP_MAX_ITERATIONS, [], 0) and np.array_equal(I.u32(r["T"]), I.u32(p["T_far"]))
    r = I.icp(p["src"][:0], p["tgt"], p["T_far"], max_iterations=5, max_dist=0.5)
    assert (r["iterations"], r["stop"], r["trace"]) == (0, I.STOP_NO_PAIRS, []) and r["max_dist"] == F(0.5)


def test_distance_schedule(oracle):
    p = R.make_pair(oracle)
    d = F(p["thr"])
    r = I.icp(p["src"], p["tgt"], I.perturb(p["T_gt"], 0.5, 0.04), max_iterations=12, max_dist=4 * d, min_dist=2 * d, shrink=0.8)
    want, cur = [], F(4 * d)
    for _ in range(12):
        want.append(cur)
        cur = max(F(2 * d), F(cur * F(0.8)))
    n = len(r["trace"])   # (the run may converge before the twelfth iteration)
    assert n >= 6 and [int(I.u32(s["dist"])) for s in r["trace"]] == [int(I.u32(v)) for v in want[:n]] and want[n - 1] == F(2 * d)
    r = I.icp(p["src"], p["tgt"], I.perturb(p["T_gt"], 0.5, 0.04), max_iterations=3, max_dist=4 * d, shrink=0.5)   # min_dist 0: max_dist
    assert all(s["dist"] == F(4 * d) for s in r["trace"])


def test_converges_from_both_perturbations(oracle):
    """the figures of this module's docstring"""
    p = R.make_pair(oracle)
    d = p["thr"]
    runs = (("5 deg / 0.3", 5.0, 0.3, dict(max_dist=8 * d, min_dist=0.5 * d, shrink=0.85)), ("0.5 deg / 4 cm", 0.5, 0.04, dict(max_dist=0, min_dist=0.5 * d, shrink=0.9)))
    for name, deg, shift, kw in runs:
        T0 = I.perturb(p["T_gt"], deg, shift)
        r = I.reference(("near", 60) if deg < 1 else ("far", 60), p["src"], p["tgt"], T0, max_iterations=60, density=d, **kw)
        r0, t0 = R.errors(T0, p["T_gt"])
        r1, t1 = R.errors(r["T"], p["T_gt"])
        ref = R.refine(oracle, p["src"], p["tgt"], T0, MSE, d, 40)
        r2, t2 = R.errors(ref["T"], p["T_gt"])
        print(f"{name}: start {r0:.4f} deg {t0:.4f}; icp {r['iterations']} iterations, stop {r['stop']}: {r1:.4f} deg {t1:.4f}, pairs {r['pairs0']} -> {r['pairs']}, "
              f"rmse {r['rmse0']:.4f} -> {r['rmse']:.4f}; refine {ref['steps']} steps, stop {ref['stop']}: {r2:.4f} deg {t2:.4f}")
        assert r["stop"] == I.STOP_CONVERGED and r["iterations"] < 60
        assert r1 < r0 and t1 < t0
        assert r["trace"][-1]["rot"] < 1e-6 and r["trace"][-1]["trans"] < 1e-6 and len(r["trace"]) == r["iterations"]
