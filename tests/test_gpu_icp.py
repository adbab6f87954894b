"""GPU: the point-to-plane ICP (lgr_icp_plane_dev) against the CPU statement tests/icp_ref_lib.py (tests/cpp/icp_ref.cpp +
csrc/lgr_icp_math.h): the result and the full trace bit for bit -- every float compared as uint32, counts and stop codes exactly.
make_pair(4000, 12) with the oracle's normals from the ground truth perturbed by 0.5 degrees / 4 cm (tests/test_icp_ref.py runs the
statement there to convergence); the large source is that cloud tiled over a 1000-point target."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref_lib as I  # noqa: E402
import refine_ref_lib as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
G = I.GROUP


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared pair is read-only)


def u32(v):
    return np.asarray(v, F).view(np.uint32)


def step_bits(s):
    if isinstance(s, dict):
        return (u32(s["T"].T.reshape(16)).tolist(), int(u32(s["dist"])), s["pairs"], int(u32(s["rmse"])), int(u32(s["rot"])), int(u32(s["trans"])))
    assert list(s.reserved) == [0] * 3
    return (u32(np.array(s.transformation, F)).tolist(), int(u32(s.dist)), s.pairs, int(u32(s.rmse)), int(u32(s.rot)), int(u32(s.trans)))


def result_bits(r):
    if isinstance(r, dict):
        return (u32(r["T"].T.reshape(16)).tolist(), r["iterations"], r["stop"], int(u32(r["max_dist"])), r["pairs"], int(u32(r["rmse"])), r["pairs0"],
                int(u32(r["rmse0"])))
    assert list(r.reserved) == [0] * 5
    return (u32(np.array(r.transformation, F)).tolist(), r.iterations, r.stop, int(u32(r.max_dist)), r.pairs, int(u32(r.rmse)), r.pairs0, int(u32(r.rmse0)))


def check(dev, ref, trace=True):
    assert result_bits(dev) == result_bits(ref), (dev.iterations, dev.stop, ref["iterations"], ref["stop"])
    if trace:
        assert len(dev.trace) == len(ref["trace"])
        for k, (a, b) in enumerate(zip(dev.trace, ref["trace"])):
            assert step_bits(a) == step_bits(b), k
    else:
        assert dev.trace is None


@pytest.fixture(scope="module")
def pair(oracle):
    p = dict(R.make_pair(oracle))
    p.update(d_src=cuda(p["src"]), d_tgt=cuda(p["tgt"]), T_near=I.perturb(p["T_gt"], 0.5, 0.04), T_5=I.perturb(p["T_gt"], 5.0, 0.3))
    return p


def kw_of(pair, shrink):
    d = pair["thr"]
    return dict(max_dist=4 * d, min_dist=0.5 * d, shrink=0.9) if shrink else dict(max_dist=2 * d)


@pytest.mark.parametrize("shrink", [False, True])
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257, 4000])
def test_source_sizes(lgr, pair, ns, shrink):
    """a single lane, the wave and workgroup boundaries, two tree levels (4000 points: 16 workgroups)"""
    s, kw = pair["src"][:ns], dict(kw_of(pair, shrink), max_iterations=6)
    ref = I.icp(s, pair["tgt"], pair["T_near"], **kw)
    assert ref["iterations"] >= (2 if ns >= 255 else 0) and ref["pairs0"] >= ns // 4
    check(lgr.icp_plane(cuda(s), pair["d_tgt"], pair["T_near"], trace=True, **kw), ref)
    check(lgr.icp_plane_host(s, pair["tgt"], pair["T_near"], trace=True, **kw), ref)


def test_source_normals_are_not_read(lgr, pair):
    """every source normal NaN: the plain entries launch the point-to-plane terms with the gate off, which reads the target's normals
    only -- a source normal that was read would drop its pair.  257 points: two workgroups, as test_source_sizes[257]"""
    s = pair["src"][:257].copy()
    s[:, 4:7] = np.nan
    kw = dict(max_dist=2 * pair["thr"], max_iterations=4)
    ref = I.icp(s, pair["tgt"], pair["T_near"], **kw)
    assert ref["iterations"] >= 2 and ref["pairs0"] >= 257 // 4
    check(lgr.icp_plane(cuda(s), pair["d_tgt"], pair["T_near"], trace=True, **kw), ref)
    check(lgr.icp_plane_host(s, pair["tgt"], pair["T_near"], trace=True, **kw), ref)


@pytest.mark.parametrize("shrink", [False, True])
def test_three_tree_levels(lgr, pair, shrink):
    """65 537 points: 257 workgroups, 2 partials of the second level, a third launch; over a 1000-point target"""
    s = np.concatenate([pair["src"]] * 17)[:65537]
    t = pair["tgt"][:1000]
    d = 2 * pair["thr"]
    kw = dict(max_dist=8 * d, min_dist=2 * d, shrink=0.8, max_iterations=3) if shrink else dict(max_dist=4 * d, max_iterations=3)
    ref = I.icp(s, t, pair["T_near"], **kw)
    assert ref["iterations"] == 3 and ref["pairs0"] > 65537 // 8
    check(lgr.icp_plane(cuda(s), cuda(t), pair["T_near"], trace=True, **kw), ref)


def test_default_distance_and_convergence(lgr, pair):
    """max_dist 0: 4 x the target's density, computed on the device; the run of tests/test_icp_ref.py, which stops CONVERGED inside a group"""
    kw = dict(max_dist=0, min_dist=0.5 * pair["thr"], shrink=0.9, max_iterations=60)
    ref = I.reference(("near", 60), pair["src"], pair["tgt"], pair["T_near"], density=pair["thr"], **kw)
    assert ref["stop"] == I.STOP_CONVERGED and ref["iterations"] % G not in (0, 1) and int(u32(ref["max_dist"])) == int(u32(F(4) * F(pair["thr"])))
    dev = lgr.icp_plane(pair["d_src"], pair["d_tgt"], pair["T_near"], trace=True, **kw)
    check(dev, ref)
    assert len(dev.trace) == dev.iterations
    check(lgr.icp_plane(pair["d_src"], pair["d_tgt"], pair["T_near"], **kw), ref, trace=False)   # no trace; the call after a stop inside a group


def test_group_edges(lgr, pair):
    """MAX_ITERATIONS one short of a group, exactly at its end, one into the next; then a run cut from the converging one"""
    kw = kw_of(pair, True)
    for m in (1, G - 1, G, G + 1, 2 * G):
        ref = I.icp(pair["src"], pair["tgt"], pair["T_near"], max_iterations=m, **kw)
        assert (ref["iterations"], ref["stop"]) == (m, I.STOP_MAX_ITERATIONS)
        check(lgr.icp_plane(pair["d_src"], pair["d_tgt"], pair["T_near"], max_iterations=m, trace=True, **kw), ref)


def test_no_pairs_and_degenerate(lgr, pair):
    far = pair["T_far"]
    ref = I.icp(pair["src"], pair["tgt"], far, max_iterations=5, max_dist=2 * pair["thr"])
    assert (ref["iterations"], ref["stop"], ref["pairs"], len(ref["trace"])) == (0, I.STOP_NO_PAIRS, 0, 1) and ref["rmse"] == I.FLT_MAX
    dev = lgr.icp_plane(pair["d_src"], pair["d_tgt"], far, max_iterations=5, max_dist=2 * pair["thr"], trace=True)
    check(dev, ref)
    assert np.array_equal(u32(dev.matrix()), u32(far))
    # a single plane: the lattice z = 0 with normals (0, 0, 1); the in-plane motions have no pivot
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2).astype(F)
    t = np.zeros((len(g), 12), F)
    t[:, :2] = g; t[:, 3] = 1; t[:, 6] = 1; t[:, 8] = 1
    s = t.copy()
    s[:, :2] += F(0.25); s[:, 2] = F(0.125)
    ref = I.icp(s, t, np.eye(4, dtype=F), max_iterations=5, max_dist=1.0)
    assert (ref["iterations"], ref["stop"], len(ref["trace"])) == (0, I.STOP_DEGENERATE, 1) and ref["pairs"] > 300
    check(lgr.icp_plane(cuda(s), cuda(t), np.eye(4, dtype=F), max_iterations=5, max_dist=1.0, trace=True), ref)


def test_idle_calls(lgr, pair):
    for s, d_s, m, stop in ((pair["src"], pair["d_src"], 0, I.STOP_MAX_ITERATIONS), (pair["src"][:0], pair["d_src"][:0], 5, I.STOP_NO_PAIRS)):
        for md in (0.0, 0.25):
            ref = I.icp(s, pair["tgt"], pair["T_5"], max_iterations=m, max_dist=md)
            assert (ref["iterations"], ref["stop"], ref["trace"]) == (0, stop, []) and ref["max_dist"] == F(md)
            check(lgr.icp_plane(d_s, pair["d_tgt"], pair["T_5"], max_iterations=m, max_dist=md, trace=True), ref)
            check(lgr.icp_plane_host(s, pair["tgt"], pair["T_5"], max_iterations=m, max_dist=md), ref, trace=False)


def test_non_finite_and_duplicates(lgr, pair):
    """NaN / inf source points, NaN target normals and points, and every third target point duplicated behind the cloud: the lower index
    must answer (the copy carries another normal, so a wrong winner changes the sums)"""
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
    kw = dict(kw_of(pair, True), max_iterations=6)
    ref = I.icp(src, tgt, pair["T_near"], **kw)
    assert ref["iterations"] == 6 and 1000 < ref["pairs0"] < 4000 - len(rows)
    check(lgr.icp_plane(cuda(src), cuda(tgt), pair["T_near"], trace=True, **kw), ref)
    swapped = np.concatenate([dup, tgt[:len(pair["tgt"])]])   # the copies first: another winner, other bits -- the tie is really there
    assert result_bits(I.icp(src, swapped, pair["T_near"], **kw)) != result_bits(ref)


def test_large_perturbation(lgr, pair):
    """5 degrees / 0.3: the first two groups of the run tests/test_icp_ref.py takes to convergence"""
    kw = dict(max_dist=8 * pair["thr"], min_dist=0.5 * pair["thr"], shrink=0.85, max_iterations=2 * G)
    ref = I.icp(pair["src"], pair["tgt"], pair["T_5"], **kw)
    check(lgr.icp_plane(pair["d_src"], pair["d_tgt"], pair["T_5"], trace=True, **kw), ref)


def test_context_reuse(lgr, pair):
    kw = dict(kw_of(pair, True), max_iterations=G + 1)
    a = lgr.icp_plane(pair["d_src"], pair["d_tgt"], pair["T_near"], trace=True, **kw)
    lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T_near"], 2, 3)
    b = lgr.icp_plane(pair["d_src"], pair["d_tgt"], pair["T_near"], trace=True, **kw)
    assert result_bits(a) == result_bits(b) and [step_bits(s) for s in a.trace] == [step_bits(s) for s in b.trace]


def test_refusals(lgr, pair):
    from lgr_amd import capi
    d_src, d_tgt, T0 = pair["d_src"], pair["d_tgt"], pair["T_near"]
    nan, inf = float("nan"), float("inf")
    bad = [dict(max_iterations=-1), dict(max_iterations=capi.ICP_MAX_ITERATIONS + 1), dict(max_dist=nan), dict(max_dist=inf), dict(max_dist=2e18),
           dict(min_dist=nan), dict(min_dist=inf), dict(min_dist=2e18), dict(max_dist=0.1, min_dist=0.2), dict(shrink=0.0), dict(shrink=-0.5),
           dict(shrink=1.5), dict(shrink=nan), dict(rot_eps=-1.0), dict(rot_eps=nan), dict(trans_eps=-1.0), dict(trans_eps=nan)]
    for kw in bad:
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.icp_plane(d_src, d_tgt, T0, **kw)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.icp_plane_host(pair["src"], pair["tgt"], T0, **kw)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.icp_plane(d_src, d_tgt[:1], T0)
    out, n = capi.IcpResult(), C.c_int(0)
    p = capi.icp_params(max_iterations=2, max_dist=0.1)
    args = lambda **k: [k.get("src", capi._ptr(d_src)), k.get("ns", len(pair["src"])), k.get("tgt", capi._ptr(d_tgt)), len(pair["tgt"]), k.get("T", lgr._T16(T0)),  # noqa: E731
                        k.get("p", C.byref(p)), k.get("out", C.byref(out)), k.get("trace"), k.get("n")]
    off4 = C.c_void_p(d_src.data_ptr() + 4)   # rows not 16-byte aligned
    for k in (dict(src=None), dict(tgt=None), dict(T=None), dict(p=None), dict(out=None), dict(ns=-1), dict(trace=(capi.IcpStep * 2)()), dict(src=off4)):
        assert capi.lib().lgr_icp_plane_dev(lgr.h, *args(**k)) == -1, list(k)
    for w in (0, 1):
        p.reserved[w] = 1
        assert capi.lib().lgr_icp_plane_dev(lgr.h, *args()) == -1
        p.reserved[w] = 0
    assert capi.lib().lgr_icp_plane_dev(lgr.h, *args()) == 0 and out.iterations == 2
