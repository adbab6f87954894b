"""GPU: the ICP variants (lgr_icp_ex_dev / lgr_icp_ex_host) against the CPU statement tests/icp_ex_ref_lib.py (tests/cpp/icp_ex_ref.cpp +
csrc/lgr_icp_math.h): the result and the full trace bit for bit -- every float compared as uint32, counts and stop codes exactly -- as
tests/test_gpu_icp.py does for lgr_icp_plane*.  make_pair(4000, 12) with the oracle's normals from the ground truth perturbed by 0.5
degrees / 4 cm; the large source is that cloud tiled over a 1000-point target; the exact edges of the rules on a corner of three lattice
planes whose coordinates, offsets and normals are powers of two, so that every residual there is exactly 0.125.

The scales, the cosine and the weights of the grid were chosen on the CPU so that every option bites (the statement's bits differ from the
same run without it, with at least ns / 4 pairs in iteration 0): k = density (point-to-plane), 2 x density (point-to-point), 0.15
(plane-to-plane, Mahalanobis), cos 0.97, weights uniform in [0.25, 1) with every 50th zero.  The test checks that again before it
compares anything."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ex_ref_lib as X  # noqa: E402
import icp_ref_lib as I  # noqa: E402
import refine_ref_lib as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
G = I.GROUP
COS = 0.97


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared pair is read-only)


def u32(v):
    return np.asarray(v, F).view(np.uint32)


def dev_bits(r):
    """a device result and its trace in the form of icp_ex_ref_lib.bits"""
    assert list(r.reserved) == [0] * 5
    head = (u32(np.array(r.transformation, F)).tolist(), r.iterations, r.stop, int(u32(r.max_dist)), r.pairs, int(u32(r.rmse)), r.pairs0, int(u32(r.rmse0)))
    steps = []
    for s in r.trace or []:
        assert list(s.reserved) == [0] * 3
        steps.append((u32(np.array(s.transformation, F)).tolist(), int(u32(s.dist)), s.pairs, int(u32(s.rmse)), int(u32(s.rot)), int(u32(s.trans))))
    return head, steps


def check(dev, ref):
    want, got = X.bits(ref), dev_bits(dev)
    assert got[0] == want[0], (dev.iterations, dev.stop, dev.pairs, ref["iterations"], ref["stop"], ref["pairs"])
    assert len(got[1]) == len(want[1])
    for k, (a, b) in enumerate(zip(got[1], want[1])):
        assert a == b, k


@pytest.fixture(scope="module")
def pair(oracle):
    p = dict(R.make_pair(oracle))
    w = np.random.default_rng(7).uniform(0.25, 1.0, len(p["src"])).astype(F)
    w[::50] = 0
    d = p["thr"]
    p.update(d_src=cuda(p["src"]), d_tgt=cuda(p["tgt"]), T_near=I.perturb(p["T_gt"], 0.5, 0.04), w=w, d_w=cuda(w),
             K={X.POINT_TO_PLANE: d, X.POINT_TO_POINT: 2 * d, X.PLANE_TO_PLANE: 0.15}, kw=dict(max_dist=4 * d, min_dist=0.5 * d, shrink=0.9))
    return p


def options(pair, variant, robust, gate):
    return dict(variant=variant, robust=robust, robust_scale=pair["K"][variant] if robust else 0.0, min_normal_cos=COS if gate else -1.0)


def configs(pair):
    """the three configurations of the size tests: (name, options, weighted)"""
    return (("huber + gate + weights", options(pair, X.POINT_TO_PLANE, X.HUBER, True), True),
            ("plane-to-plane + tukey", options(pair, X.PLANE_TO_PLANE, X.TUKEY, False), False),
            ("point-to-point + cauchy", options(pair, X.POINT_TO_POINT, X.CAUCHY, False), False))


def test_neutral_identity(lgr, pair):
    """POINT_TO_PLANE / NONE / gate off / no weights: the bytes of lgr_icp_plane* on the same inputs"""
    for ns, kw in ((4000, dict(pair["kw"], max_iterations=G + 1)), (257, dict(max_dist=2 * pair["thr"], max_iterations=4))):
        s = pair["src"][:ns]
        a = lgr.icp_plane(cuda(s), pair["d_tgt"], pair["T_near"], trace=True, **kw)
        b = lgr.icp_ex(cuda(s), pair["d_tgt"], pair["T_near"], trace=True, **kw)
        c = lgr.icp_ex_host(s, pair["tgt"], pair["T_near"], trace=True, **kw)
        assert a.iterations >= 2 and a.pairs0 >= ns // 4
        assert dev_bits(a) == dev_bits(b) == dev_bits(c)
        check(b, I.icp(s, pair["tgt"], pair["T_near"], **kw))


@pytest.mark.parametrize("variant", X.VARIANTS)
def test_configuration_grid(lgr, pair, variant):
    """every robust kernel x gate off / on x weights none / given of one variant, 4000 points, 6 iterations from T_near; first that each
    option bites on the statement alone"""
    kw, cache = dict(pair["kw"], max_iterations=6), {}

    def ref(r, g, w):
        if (r, g, w) not in cache:
            cache[(r, g, w)] = X.icp(pair["src"], pair["tgt"], pair["T_near"], weights=pair["w"] if w else None, **options(pair, variant, r, g), **kw)
        return cache[(r, g, w)]
    for r, g, w in itertools.product(X.ROBUSTS, (False, True), (False, True)):
        want = ref(r, g, w)
        assert want["pairs0"] >= len(pair["src"]) // 4 and want["iterations"] == 6, (r, g, w)
        for without in ([(X.NONE, g, w)] if r else []) + ([(r, False, w)] if g else []) + ([(r, g, False)] if w else []):
            assert X.bits(want) != X.bits(ref(*without)), ((r, g, w), without)   # the option bites
        dev = lgr.icp_ex(pair["d_src"], pair["d_tgt"], pair["T_near"], weights=pair["d_w"] if w else None, trace=True, **options(pair, variant, r, g), **kw)
        check(dev, want)


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257])
def test_tree_and_wave_boundaries(lgr, pair, ns):
    """a single lane, the wave and workgroup boundaries, through the device and the host entry"""
    s, w, kw = pair["src"][:ns], pair["w"][:ns], dict(pair["kw"], max_iterations=6)
    for name, opt, weighted in configs(pair)[:2]:
        want = X.icp(s, pair["tgt"], pair["T_near"], weights=w if weighted else None, **opt, **kw)
        assert want["pairs0"] >= ns // 4, name
        check(lgr.icp_ex(cuda(s), pair["d_tgt"], pair["T_near"], weights=cuda(w) if weighted else None, trace=True, **opt, **kw), want)
        check(lgr.icp_ex_host(s, pair["tgt"], pair["T_near"], weights=w if weighted else None, trace=True, **opt, **kw), want)


def test_three_tree_levels(lgr, pair):
    """65 537 points: 257 workgroups, 2 partials of the second level, a third launch; over a 1000-point target"""
    s = np.concatenate([pair["src"]] * 17)[:65537]
    w = np.concatenate([pair["w"]] * 17)[:65537]
    t = pair["tgt"][:1000]
    kw = dict(max_dist=8 * pair["thr"], max_iterations=3)
    d_s, d_t, d_w = cuda(s), cuda(t), cuda(w)
    for name, opt, weighted in configs(pair):
        want = X.icp(s, t, pair["T_near"], weights=w if weighted else None, **opt, **kw)
        assert want["iterations"] == 3 and want["pairs0"] > 65537 // 8, name
        check(lgr.icp_ex(d_s, d_t, pair["T_near"], weights=d_w if weighted else None, trace=True, **opt, **kw), want)


def corner():
    """three lattice planes z = 0, x = 0, y = 0 (coordinates 1 .. 8, axis normals) and the same points moved by (1/8, 1/8, 1/8) with the
    same normals: every pair's e is (1/8, 1/8, 1/8), its point-to-plane residual exactly 1/8, its m . n exactly 1"""
    g = np.stack(np.meshgrid(np.arange(1, 9), np.arange(1, 9), indexing="ij"), -1).reshape(-1, 2).astype(F)
    planes = []
    for axis in range(3):
        t = np.zeros((len(g), 12), F)
        t[:, [a for a in range(3) if a != axis]] = g
        t[:, 3] = 1; t[:, 4 + axis] = 1; t[:, 8] = 1
        planes.append(t)
    t = np.concatenate(planes)
    s = t.copy()
    s[:, :3] += F(0.125)
    return s, t


def test_edges_of_the_rules(lgr):
    s, t = corner()
    n, E, kw = len(s), np.eye(4, dtype=F), dict(max_iterations=3, max_dist=1.0)

    def both(src=s, tgt=t, weights=None, **opt):
        want = X.icp(src, tgt, E, weights=weights, **opt, **kw)
        check(lgr.icp_ex(cuda(src), cuda(tgt), E, weights=cuda(weights) if weights is not None else None, trace=True, **opt, **kw), want)
        check(lgr.icp_ex_host(src, tgt, E, weights=weights, trace=True, **opt, **kw), want)
        return want
    plain = both()
    assert plain["pairs0"] == n and plain["rmse0"] == F(0.125) and plain["iterations"] >= 1
    # Huber with rho == k exactly: weight 1, the plain run's bits; with the x = 0 plane's points twice as far (rho = 1/4 there, weight
    # 1/2; 1/8 and weight 1 on the other two planes) it is another run
    assert X.bits(both(robust=X.HUBER, robust_scale=0.125)) == X.bits(plain)
    far = s.copy()
    far[:64, 0] += F(0.125)
    assert X.bits(both(src=far, robust=X.HUBER, robust_scale=0.125)) != X.bits(both(src=far))
    # Tukey with every residual >= k: nothing pairs (point-to-point's rho is sqrt(3) / 8 there)
    for v in (X.POINT_TO_PLANE, X.POINT_TO_POINT):
        r = both(variant=v, robust=X.TUKEY, robust_scale=0.125)
        assert (r["stop"], r["pairs"], r["iterations"], len(r["trace"])) == (I.STOP_NO_PAIRS, 0, 0, 1) and r["rmse"] == I.FLT_MAX
    assert both(robust=X.TUKEY, robust_scale=float(np.nextafter(F(0.125), F(1))))["pairs0"] == n
    # a gate cosine met exactly is kept: m . n == 1 with the normals as they are, == 0.5 with the source's halved
    assert both(min_normal_cos=1.0)["pairs0"] == n
    half = s.copy()
    half[:, 4:7] *= F(0.5)
    assert both(src=half, min_normal_cos=0.5)["pairs0"] == n
    r = both(src=half, min_normal_cos=float(np.nextafter(F(0.5), F(1))))
    assert (r["stop"], r["pairs"]) == (I.STOP_NO_PAIRS, 0)
    # weights: 0, a negative, NaN and inf make no pair
    w = np.full(n, 0.5, F)
    w[[3, 70, 71, 140]] = [0.0, -1.0, np.nan, np.inf]
    for v in X.VARIANTS:
        assert both(variant=v, weights=w)["pairs0"] == n - 4
    # NaN source normals: no pair where they are read (the gate, plane-to-plane), the same bits where they are not
    bad = s.copy()
    bad[5::7, 5] = np.nan
    n_bad = len(bad[5::7])
    assert both(src=bad, min_normal_cos=0.5)["pairs0"] == n - n_bad
    assert both(src=bad, variant=X.POINT_TO_POINT, min_normal_cos=0.5)["pairs0"] == n - n_bad
    assert both(src=bad, variant=X.PLANE_TO_PLANE)["pairs0"] == n - n_bad
    assert X.bits(both(src=bad)) == X.bits(plain)
    # NaN target normals under point-to-point without the gate: not read
    tb = t.copy()
    tb[2::5, 4] = np.nan
    assert X.bits(both(tgt=tb, variant=X.POINT_TO_POINT)) == X.bits(both(variant=X.POINT_TO_POINT))
    assert both(tgt=tb, variant=X.POINT_TO_POINT, min_normal_cos=0.5)["pairs0"] == n - len(tb[2::5])
    # a single plane: point-to-plane has no pivot for the in-plane motions, with or without the new factors.  Plane-to-plane is NOT
    # degenerate there, whatever plane_eps: Sigma^-1 weighs the in-plane part of e by 1 / 2 against 1 / (2 eps) along the normal, a ratio
    # of eps >= 1e-6, far above the pivot rule's 1e-12 -- the lattice itself holds the in-plane motions, and the run lands on it exactly
    # (measured on the CPU: CONVERGED after 2 iterations at the shift (-1/4, -1/4, -1/8), rmse 0).
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2).astype(F)
    pt = np.zeros((len(g), 12), F)
    pt[:, :2] = g; pt[:, 3] = 1; pt[:, 4:7] = [0, 0, 1]; pt[:, 8] = 1
    ps = pt.copy()
    ps[:, :2] += F(0.25); ps[:, 2] = F(0.125)
    for opt in (dict(), dict(robust=X.CAUCHY, robust_scale=0.25, min_normal_cos=0.5, weights=np.full(len(ps), 0.5, F))):
        r = both(src=ps, tgt=pt, **opt)
        assert (r["iterations"], r["stop"], len(r["trace"])) == (0, I.STOP_DEGENERATE, 1) and r["pairs"] == 400
    for eps in (0.0, 1e-6):
        r = both(src=ps, tgt=pt, variant=X.PLANE_TO_PLANE, plane_eps=eps)
        assert (r["iterations"], r["stop"], r["pairs"]) == (2, I.STOP_CONVERGED, 400) and r["rmse"] == 0
        assert np.array_equal(r["T"][:3, 3], np.array([-0.25, -0.25, -0.125], F))


def test_duplicate_targets_three_rows(lgr, pair):
    """the tie of tests/test_gpu_icp.py::test_non_finite_and_duplicates under the three-row body: every third target point duplicated behind
    the cloud with another normal, which plane-to-plane reads -- the lower index must answer"""
    src, tgt = pair["src"].copy(), pair["tgt"].copy()
    rows = np.arange(5, len(src), 97)
    src[rows[0::3], 0] = np.nan
    src[rows[1::3], 1] = np.inf
    src[rows[2::3], 2] = -np.inf
    tgt[3::11, 5] = np.nan    # normals
    tgt[7::13, :3] = np.nan   # points
    dup = tgt[::3].copy()
    dup[:, 4:7] = dup[:, [5, 6, 4]]
    tgt = np.concatenate([tgt, dup])
    kw = dict(pair["kw"], max_iterations=6, variant=X.PLANE_TO_PLANE)
    ref = X.icp(src, tgt, pair["T_near"], **kw)
    assert ref["iterations"] == 6 and 1000 < ref["pairs0"] < 4000 - len(rows)
    check(lgr.icp_ex(cuda(src), cuda(tgt), pair["T_near"], trace=True, **kw), ref)
    swapped = np.concatenate([dup, tgt[:len(pair["tgt"])]])   # the copies first: another winner, other bits -- the tie is really there
    assert X.bits(X.icp(src, swapped, pair["T_near"], **kw))[0] != X.bits(ref)[0]


def test_group_edges(lgr, pair):
    """MAX_ITERATIONS one short of a group, exactly at its end, one into the next, and a single iteration"""
    opt = options(pair, X.POINT_TO_POINT, X.CAUCHY, False)
    for m in (1, G - 1, G, G + 1):
        ref = X.icp(pair["src"], pair["tgt"], pair["T_near"], max_iterations=m, **opt, **pair["kw"])
        assert (ref["iterations"], ref["stop"]) == (m, I.STOP_MAX_ITERATIONS)
        check(lgr.icp_ex(pair["d_src"], pair["d_tgt"], pair["T_near"], max_iterations=m, trace=True, **opt, **pair["kw"]), ref)


def test_convergence_inside_a_group(lgr, pair):
    """plane-to-plane from the ground truth at max_dist = density (tests/test_icp_ex_ref.py): CONVERGED after 6 iterations"""
    kw = dict(variant=X.PLANE_TO_PLANE, max_iterations=60, max_dist=pair["thr"])
    ref = X.icp(pair["src"], pair["tgt"], pair["T_gt"], **kw)
    assert ref["stop"] == I.STOP_CONVERGED and ref["iterations"] % G not in (0, 1)
    dev = lgr.icp_ex(pair["d_src"], pair["d_tgt"], pair["T_gt"], trace=True, **kw)
    check(dev, ref)
    assert len(dev.trace) == dev.iterations
    assert dev_bits(lgr.icp_ex(pair["d_src"], pair["d_tgt"], pair["T_gt"], **kw))[0] == X.bits(ref)[0]   # no trace; the call after a stop inside a group


def test_refusals_and_context_reuse(lgr, pair):
    from lgr_amd import capi
    d_src, d_tgt, T0 = pair["d_src"], pair["d_tgt"], pair["T_near"]
    nan, inf = float("nan"), float("inf")
    bad = [dict(variant=-1), dict(variant=3), dict(robust=-1), dict(robust=4), dict(robust=1, robust_scale=0.0), dict(robust=2, robust_scale=-1.0),
           dict(robust=3, robust_scale=nan), dict(robust=1, robust_scale=inf), dict(min_normal_cos=nan), dict(min_normal_cos=-1.5), dict(min_normal_cos=1.5),
           dict(plane_eps=nan), dict(plane_eps=-1.0), dict(plane_eps=1e-7), dict(plane_eps=2.0), dict(variant=2, plane_eps=inf),
           dict(max_iterations=-1), dict(max_iterations=capi.ICP_MAX_ITERATIONS + 1), dict(max_dist=nan), dict(min_dist=inf), dict(max_dist=0.1, min_dist=0.2),
           dict(shrink=0.0), dict(shrink=1.5), dict(rot_eps=-1.0), dict(trans_eps=nan)]
    for kw in bad:
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.icp_ex(d_src, d_tgt, T0, **kw)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.icp_ex_host(pair["src"], pair["tgt"], T0, **kw)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.icp_ex(d_src, d_tgt[:1], T0)
    out, n = capi.IcpResult(), C.c_int(0)
    p = capi.icp_ex_params(variant="point", robust="huber", robust_scale=0.05, max_iterations=2, max_dist=0.1)
    for fn, a, b in ((capi.lib().lgr_icp_ex_dev, d_src, d_tgt), (capi.lib().lgr_icp_ex_host, pair["src"], pair["tgt"])):
        args = lambda **k: [k.get("src", capi._ptr(a)), k.get("ns", len(pair["src"])), k.get("tgt", capi._ptr(b)), len(pair["tgt"]), k.get("T", lgr._T16(T0)),  # noqa: E731
                            k.get("p", C.byref(p)), k.get("out", C.byref(out)), k.get("trace"), k.get("n")]
        for k in (dict(src=None), dict(tgt=None), dict(T=None), dict(p=None), dict(out=None), dict(ns=-1), dict(trace=(capi.IcpStep * 2)())):
            assert fn(lgr.h, *args(**k)) == -1, list(k)
        for w in range(3):   # the reserved words at both levels
            p.reserved[w] = 1
            assert fn(lgr.h, *args()) == -1
            p.reserved[w] = 0
        for w in range(2):
            p.base.reserved[w] = 1
            assert fn(lgr.h, *args()) == -1
            p.base.reserved[w] = 0
        p.robust_scale = 0.0   # not read under ROBUST_NONE, refused under a kernel
        assert fn(lgr.h, *args()) == -1
        p.robust = capi.ICP_ROBUST_NONE
        assert fn(lgr.h, *args()) == 0 and out.iterations == 2
        p.robust, p.robust_scale = capi.ICP_ROBUST_HUBER, 0.05
        assert fn(lgr.h, *args()) == 0 and out.iterations == 2   # a good call afterwards works
    off4 = C.c_void_p(d_src.data_ptr() + 4)   # rows not 16-byte aligned
    assert capi.lib().lgr_icp_ex_dev(lgr.h, off4, len(pair["src"]) - 1, capi._ptr(d_tgt), len(pair["tgt"]), lgr._T16(T0), C.byref(p), C.byref(out), None, None) == -1
    # the idle calls return what lgr_icp_plane* returns
    for s, m in ((d_src, 0), (d_src[:0], 5)):
        for md in (0.0, 0.25):
            a = lgr.icp_plane(s, d_tgt, T0, max_iterations=m, max_dist=md, trace=True)
            b = lgr.icp_ex(s, d_tgt, T0, variant="plane2plane", robust="tukey", robust_scale=1.0, min_normal_cos=0.5, max_iterations=m, max_dist=md, trace=True)
            assert dev_bits(a) == dev_bits(b) and a.trace == []
    # lgr_icp_plane, lgr_icp_ex, lgr_icp_plane on one context: the first call's bytes
    kw = dict(pair["kw"], max_iterations=G + 1)
    a = lgr.icp_plane(d_src, d_tgt, T0, trace=True, **kw)
    lgr.icp_ex(d_src, d_tgt, T0, weights=pair["d_w"], trace=True, **options(pair, X.PLANE_TO_PLANE, X.TUKEY, True), **kw)
    b = lgr.icp_plane(d_src, d_tgt, T0, trace=True, **kw)
    assert dev_bits(a) == dev_bits(b)
