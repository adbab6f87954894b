"""CPU: the statement of trimmed ICP (tests/icp_trim_ref_lib.py: tests/cpp/icp_trim_ref.cpp + csrc/lgr_icp_math.h) -- the shared scalar
pieces against known answers, the neutral configuration against the statement of the variants bit for bit, and what trimming and the
median-scaled kernels do on the half-overlapping pair where the plain step drifts.

Measured on the CPU with this statement before anything was asserted (make_pair(4000, 12), the oracle's normals, density 0.03086).  Half
overlap, from the ground truth, shrink 1, max_dist = density, 60 iterations allowed (rotation error in degrees, translation error; the
cut and the scale are those of the last iteration):
  point-to-plane, plain (= lgr_icp_plane)      60 it  0.9277  0.01630   drifts, 2069 pairs in iteration 0
  point-to-plane, keep 0.9                     26 it  0.2182  0.00558   CONVERGED, 1862 pairs, cut 0.00914
  point-to-plane, keep 0.7                     23 it  0.4246  0.00862   CONVERGED, 1448 pairs, cut 0.00575
  point-to-plane, keep 0.5                     19 it  0.1057  0.00260   CONVERGED, 1034 pairs, cut 0.00362
  point-to-plane + Cauchy k = 1.4826 median    16 it  0.1376  0.00144   CONVERGED, scale 0.00552 (the largest key 0.0299)
  point-to-plane + Huber  k = 1.4826 median    13 it  0.2856  0.00432   CONVERGED, scale 0.00544
  point-to-point, plain                        47 it  0.2094  0.00645   CONVERGED
  point-to-point, keep 0.7                     18 it  0.1163  0.00283   CONVERGED
  plane-to-plane, plain (eps 1e-3)              6 it  0.0760  0.00201   CONVERGED
  plane-to-plane, keep 0.7                      7 it  0.0605  0.00124   CONVERGED
Every point-to-plane configuration ends closer to the ground truth than the plain run.  The smallest measured gap is keep 0.7's: 0.503
degrees and 0.00768.  Asserted for every point-to-plane configuration: at least 0.2 degrees and 0.0035 closer than the plain run of the
same session -- under half the smallest gap (0.2515 / 0.00384), the rule of tests/test_icp_ex_ref.py.  Point-to-point and plane-to-plane
gain little (0.09 / 0.016 degrees): asserted only that keep 0.7 is not worse than the untrimmed run of the same variant.  From 5 degrees /
0.3 away without a shrinking distance the outcome is erratic; nothing is asserted there.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ex_ref_lib as X  # noqa: E402
import icp_ref_lib as I  # noqa: E402
import icp_trim_ref_lib as TR  # noqa: E402
import refine_ref_lib as R  # noqa: E402

F = np.float32
MAD = 1.4826


def test_scalar_pieces_known_answers():
    # K = floor((double) keep * (double) P): 0.9f is 0.89999997615..., so 0.9f x 2070 is just under 1863
    assert TR.trim_k(0.9, 2069) == 1862 and TR.trim_k(0.9, 2070) == 1862 and TR.trim_k(0.9, 10) == 8
    assert TR.trim_k(0.5, 2069) == 1034 and TR.trim_k(0.7, 10) == 6   # 0.7f is 0.69999998...
    assert [TR.trim_k(k, 1) for k in (1e-3, 0.5, 0.9, 1.0)] == [0, 0, 0, 1]
    assert [TR.trim_k(k, 2) for k in (1e-3, 0.5, 0.9, 1.0)] == [0, 1, 1, 2]
    assert TR.trim_k(1.0, 0) == 0 and TR.trim_k(0.5, 0) == 0
    for P in (1, 2, 3, 2069, 4000, 2 ** 31 - 1):
        assert TR.trim_k(1.0, P) == P
    # the median rank: the lower of two middles
    assert [TR.median_rank(P) for P in (1, 2, 3, 4, 5, 2069, 2070)] == [0, 0, 1, 1, 2, 1034, 1034]
    # k of the iteration: the f32 multiplier times the f32 key, one f64 product; the caller's scale where the multiplier is 0
    assert TR.scale(MAD, 0.25) == float(F(MAD)) * 0.25 and TR.scale(2.0, 3.0, 9.0) == 6.0 and TR.scale(0.0, 3.0, 9.0) == 9.0
    assert TR.scale(MAD, 0.0) == 0.0
    # a scale of 0 (an all-zero key set's median), a NaN or an infinite one: every weight is 1
    for kind in X.ROBUSTS:
        for k in (0.0, -1.0, np.nan, np.inf):
            assert [TR.weight(kind, rho, k) for rho in (0.0, 0.5, 7.0)] == [1.0, 1.0, 1.0]
        for rho in (0.0, 0.375, 0.75, 1.5):   # a usable k: the variants' weight
            assert TR.weight(kind, rho, 0.75) == X.robust_weight(kind, rho, 0.75)
    # the key: (float) rho as bits; candidates are the finite keys without a sign
    assert TR.key(0.0) == (True, 0) and TR.key(1.0) == (True, 0x3F800000) and TR.key(float(np.finfo(F).max)) == (True, 0x7F7FFFFF)
    assert TR.key(1e-46) == (True, 0) and TR.key(1.0 + 2.0 ** -30) == (True, 0x3F800000)   # rounded to f32
    for rho in (np.nan, np.inf, -1.0, -0.0, 1e39):
        assert not TR.key(rho)[0]


def test_neutral_configuration_is_the_variants_statement(oracle):
    """the runs of test_icp_ex_ref.py::test_neutral_configuration_is_the_plane_statement, and the same under other options: keep 1 and
    scale_from_median 0 give the bits of the icp_ex statement, info = (pairs, pairs, 0, the caller's scale)"""
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
        a, b, c = I.icp(s, t, T_near, **kw), X.icp(s, t, T_near, **kw), TR.icp(s, t, T_near, **kw)
        assert X.bits(a) == X.bits(b) == X.bits(c), kw
        assert c["info"] == [dict(candidates=st["pairs"], kept=st["pairs"], cut=F(0), scale=F(0)) for st in c["trace"]]
    s, t, kw = runs[2]
    opt = dict(variant=X.PLANE_TO_PLANE, robust=X.TUKEY, robust_scale=0.15, min_normal_cos=0.9)
    b, c = X.icp(s, t, T_near, **opt, **kw), TR.icp(s, t, T_near, **opt, **kw)
    assert X.bits(b) == X.bits(c) and c["info"] == [dict(candidates=st["pairs"], kept=st["pairs"], cut=F(0), scale=F(0.15)) for st in c["trace"]]


def test_trim_and_median_on_a_run(oracle):
    """one run of each kind: info follows the rules (K from P, cut and scale from the order), trimming drops pairs, and a source that is a
    copy of the target has an all-zero key set -- median 0, every weight 1, the bits of the run without a kernel"""
    p = R.make_pair(oracle)
    d = p["thr"]
    T_near = I.perturb(p["T_gt"], 0.5, 0.04)
    kw = dict(max_dist=4 * d, min_dist=0.5 * d, shrink=0.9, max_iterations=6)
    full = TR.icp(p["src"], p["tgt"], T_near, **kw)
    r = TR.icp(p["src"], p["tgt"], T_near, keep=0.9, **kw)
    assert r["iterations"] == 6 and X.bits(r)[0] != X.bits(full)[0]
    assert r["info"][0]["candidates"] == full["info"][0]["candidates"] == full["pairs0"]   # iteration 0 sees the same pairs
    for st, inf in zip(r["trace"], r["info"]):
        assert inf["kept"] == TR.trim_k(0.9, inf["candidates"]) == st["pairs"] and inf["cut"] > 0 and inf["scale"] == 0
    m = TR.icp(p["src"], p["tgt"], T_near, scale_from_median=MAD, robust=X.CAUCHY, **kw)
    assert m["iterations"] == 6 and X.bits(m)[0] != X.bits(full)[0]
    for st, inf in zip(m["trace"], m["info"]):
        assert inf["kept"] == inf["candidates"] == st["pairs"] and 0 < inf["scale"] < inf["cut"]   # keep 1: the cut is the largest key
    # a copy of the target from the identity: every residual is exactly 0
    t = p["tgt"][np.isfinite(p["tgt"]).all(1)]
    E = np.eye(4, dtype=F)
    for v in X.VARIANTS:
        a = TR.icp(t, t, E, variant=v, keep=0.999, max_dist=d, max_iterations=3)   # (not neutral: the trimmed loop, no kernel)
        b = TR.icp(t, t, E, variant=v, keep=0.999, scale_from_median=MAD, robust=X.TUKEY, max_dist=d, max_iterations=3)
        assert X.bits(a) == X.bits(b) and a["pairs0"] == TR.trim_k(0.999, len(t))
        assert [(i["cut"], i["scale"]) for i in b["info"][:1]] == [(F(0), F(0))]


def test_half_overlap_from_the_ground_truth(oracle):
    """the figures of this module's docstring"""
    p = R.make_pair(oracle)
    d = p["thr"]
    base = dict(max_iterations=60, max_dist=d, shrink=1.0)

    def run(name, **kw):
        r = TR.icp(p["src"], p["tgt"], p["T_gt"], **dict(base, **kw))
        e = R.errors(r["T"], p["T_gt"])
        print(f"{name:44s} {r['iterations']:3d} iterations, stop {r['stop']}: {e[0]:.4f} deg {e[1]:.5f}, pairs {r['pairs0']} -> {r['pairs']}, "
              f"rmse {r['rmse0']:.5f} -> {r['rmse']:.5f}, cut {r['info'][-1]['cut']:.5f} scale {r['info'][-1]['scale']:.5f}")
        return e
    plain = run("point-to-plane, plain")
    assert plain[0] > 0.8   # lgr_icp_plane's drift (0.93 degrees)
    for name, kw in (("point-to-plane, keep 0.9", dict(keep=0.9)), ("point-to-plane, keep 0.7", dict(keep=0.7)), ("point-to-plane, keep 0.5", dict(keep=0.5)),
                     ("point-to-plane + Cauchy 1.4826 median", dict(robust=X.CAUCHY, scale_from_median=MAD)),
                     ("point-to-plane + Huber 1.4826 median", dict(robust=X.HUBER, scale_from_median=MAD))):
        e = run(name, **kw)
        assert e[0] <= plain[0] - 0.2 and e[1] <= plain[1] - 0.0035, name
    for v, name in ((X.POINT_TO_POINT, "point-to-point"), (X.PLANE_TO_PLANE, "plane-to-plane")):
        whole, trimmed = run(name + ", plain", variant=v), run(name + ", keep 0.7", variant=v, keep=0.7)
        assert trimmed[0] <= whole[0] and trimmed[1] <= whole[1], name
