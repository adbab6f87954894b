"""GPU: trimmed ICP and the median-scaled robust kernels (lgr_icp_trim_dev / lgr_icp_trim_host) against the CPU statement
tests/icp_trim_ref_lib.py (tests/cpp/icp_trim_ref.cpp + csrc/lgr_icp_math.h): the result, the full trace and the info records bit for bit --
every float compared as uint32, counts and stop codes exactly -- as tests/test_gpu_icp_ex.py does for lgr_icp_ex*.  make_pair(4000, 12)
with the oracle's normals from the ground truth perturbed by 0.5 degrees / 4 cm, 6 to 9 iterations a run.  The statement finds its ranks
by sorting; the device by radix select inside the iteration loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ex_ref_lib as X  # noqa: E402
import icp_ref_lib as I  # noqa: E402
import icp_trim_ref_lib as TR  # noqa: E402
import refine_ref_lib as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
G = I.GROUP
MAD = 1.4826


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def u32(v):
    return np.asarray(v, F).view(np.uint32)


def dev_bits(r):
    """a device result, its trace and its info in the form of icp_trim_ref_lib.bits"""
    assert list(r.reserved) == [0] * 5
    head = (u32(np.array(r.transformation, F)).tolist(), r.iterations, r.stop, int(u32(r.max_dist)), r.pairs, int(u32(r.rmse)), r.pairs0, int(u32(r.rmse0)))
    steps = []
    for s in r.trace or []:
        assert list(s.reserved) == [0] * 3
        steps.append((u32(np.array(s.transformation, F)).tolist(), int(u32(s.dist)), s.pairs, int(u32(s.rmse)), int(u32(s.rot)), int(u32(s.trans))))
    return head, steps, [(s.candidates, s.kept, int(u32(s.cut)), int(u32(s.scale))) for s in r.info]


def check(dev, ref):
    want, got = TR.bits(ref), dev_bits(dev)
    print(f"  {ref['iterations']} iterations, stop {ref['stop']}, pairs {ref['pairs0']} -> {ref['pairs']}, info[0] {ref['info'][:1]}")
    assert got[0] == want[0], (dev.iterations, dev.stop, dev.pairs, ref["iterations"], ref["stop"], ref["pairs"])
    assert len(got[1]) == len(want[1]) == len(got[2]) == len(want[2])
    for k, (a, b) in enumerate(zip(got[1], want[1])):
        assert a == b, k
    assert got[2] == want[2]


@pytest.fixture(scope="module")
def pair(oracle):
    p = dict(R.make_pair(oracle))
    w = np.random.default_rng(7).uniform(0.25, 1.0, len(p["src"])).astype(F)
    w[::50] = 0
    d = p["thr"]
    p.update(d_src=cuda(p["src"]), d_tgt=cuda(p["tgt"]), T_near=I.perturb(p["T_gt"], 0.5, 0.04), w=w, d_w=cuda(w),
             kw=dict(max_dist=4 * d, min_dist=0.5 * d, shrink=0.9, max_iterations=6))
    return p


def both(lgr, pair, src=None, tgt=None, weights=None, host=True, **opt):
    """the statement, the device and (host=True) the host twin on one configuration -> the statement's result"""
    s = pair["src"] if src is None else src
    t = pair["tgt"] if tgt is None else tgt
    kw = dict(pair["kw"], **opt)
    want = TR.icp(s, t, pair["T_near"], weights=weights, **kw)
    d_s = pair["d_src"] if src is None else cuda(s)
    d_t = pair["d_tgt"] if tgt is None else cuda(t)
    check(lgr.icp_trim(d_s, d_t, pair["T_near"], weights=cuda(weights) if weights is not None else None, trace=True, **kw), want)
    if host:
        check(lgr.icp_trim_host(s, t, pair["T_near"], weights=weights, trace=True, **kw), want)
    return want


CONFIGS = {
    "keep 0.9": dict(keep=0.9),
    "keep 0.5": dict(keep=0.5),
    "cauchy x median": dict(robust=X.CAUCHY, scale_from_median=MAD),
    "huber x median": dict(robust=X.HUBER, scale_from_median=MAD),
    "tukey x median": dict(robust=X.TUKEY, scale_from_median=MAD),
    "point-to-plane keep 0.7": dict(variant=X.POINT_TO_PLANE, keep=0.7),
    "point-to-point keep 0.7": dict(variant=X.POINT_TO_POINT, keep=0.7),
    "plane-to-plane keep 0.7": dict(variant=X.PLANE_TO_PLANE, keep=0.7),
    "keep + median + gate + weights": dict(keep=0.8, robust=X.HUBER, scale_from_median=2.0, min_normal_cos=0.97, weighted=True),
    "plane-to-plane, tukey x median, keep 0.6, 9 iterations": dict(variant=X.PLANE_TO_PLANE, robust=X.TUKEY, scale_from_median=3.0, keep=0.6, max_iterations=G + 1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configurations(lgr, pair, name):
    opt = dict(CONFIGS[name])
    w = pair["w"] if opt.pop("weighted", False) else None
    want = both(lgr, pair, weights=w, host=name.startswith("keep +"), **opt)
    full = TR.icp(pair["src"], pair["tgt"], pair["T_near"], weights=w, **dict(pair["kw"], **dict(opt, keep=1.0, scale_from_median=0.0, robust=X.NONE)))
    assert want["iterations"] == opt.get("max_iterations", 6) and want["pairs0"] >= 500
    assert X.bits(want)[0] != X.bits(full)[0]   # the option bites
    for inf in want["info"]:
        assert inf["kept"] == TR.trim_k(opt.get("keep", 1.0), inf["candidates"]) and (inf["scale"] > 0) == ("robust" in opt)


def test_nan_input(lgr, pair):
    """the NaN-polluted clouds of tests/test_gpu_icp_ex.py::test_duplicate_targets_three_rows, without the duplicates"""
    src, tgt = pair["src"].copy(), pair["tgt"].copy()
    rows = np.arange(5, len(src), 97)
    src[rows[0::3], 0] = np.nan
    src[rows[1::3], 1] = np.inf
    src[rows[2::3], 2] = -np.inf
    src[7::101, 5] = np.nan   # source normals: read by plane-to-plane
    tgt[3::11, 5] = np.nan    # normals
    tgt[7::13, :3] = np.nan   # points
    for opt in (dict(keep=0.7), dict(variant=X.PLANE_TO_PLANE, keep=0.8, robust=X.CAUCHY, scale_from_median=MAD)):
        want = both(lgr, pair, src=src, tgt=tgt, max_iterations=9, **opt)
        assert 500 < want["info"][0]["candidates"] < 4000 - len(rows)


def test_small_sources(lgr, pair):
    for opt in (dict(keep=0.7), dict(robust=X.HUBER, scale_from_median=MAD, keep=0.9)):
        for ns in (65, 64, 257):
            want = both(lgr, pair, src=pair["src"][:ns], **opt)
            assert want["info"][0]["candidates"] >= ns // 4
    want = both(lgr, pair, src=pair["src"][:5], keep=0.9)
    assert (want["stop"], want["iterations"], len(want["info"])) == (I.STOP_NO_PAIRS, 0, 1)
    want = both(lgr, pair, src=pair["src"][:65], keep=1e-3)
    assert (want["stop"], want["iterations"]) == (I.STOP_NO_PAIRS, 0) and want["info"][0]["kept"] < 6 and want["info"][0]["candidates"] >= 16
    want = both(lgr, pair, src=pair["src"][:1], keep=0.5, robust=X.TUKEY, scale_from_median=1.0)
    assert want["stop"] == I.STOP_NO_PAIRS


def test_exact_ties(lgr, pair):
    """a source that is its first 1500 points twice: every key appears twice, and with an odd K the cut falls inside a pair of equals --
    the lower index is kept, as the statement's sort by (key, i) says.  Rows 1500 .. 2999 carry another weight than their twins, so
    keeping the wrong one of the two changes W of that pair and with it the sums."""
    a = pair["src"][:1500]
    s = np.concatenate([a, a])
    w = np.concatenate([np.full(1500, 1.0, F), np.full(1500, 0.5, F)])
    odd = None
    for keep in (0.5, 0.51, 0.52, 0.53, 0.54, 0.55, 0.56, 0.57):
        r = TR.icp(s, pair["tgt"], pair["T_near"], keep=keep, weights=w, **pair["kw"])
        assert all(i["candidates"] % 2 == 0 for i in r["info"])
        if r["info"][0]["kept"] % 2 == 1:
            odd = keep
            break
    assert odd is not None
    want = both(lgr, pair, src=s, weights=w, keep=odd)
    assert want["iterations"] == 6 and want["info"][0]["kept"] % 2 == 1


def test_neutral_call_is_lgr_icp_ex(lgr, pair):
    d_src, d_tgt, T0 = pair["d_src"], pair["d_tgt"], pair["T_near"]
    for opt in (dict(), dict(variant=X.PLANE_TO_PLANE, robust=X.TUKEY, robust_scale=0.15, min_normal_cos=0.9)):
        kw = dict(pair["kw"], max_iterations=G + 1, **opt)
        a = lgr.icp_ex(d_src, d_tgt, T0, trace=True, **kw)
        for b in (lgr.icp_trim(d_src, d_tgt, T0, trace=True, **kw), lgr.icp_trim_host(pair["src"], pair["tgt"], T0, trace=True, **kw)):
            assert dev_bits(b)[:2] == dev_bits_ex(a)[:2]
            scale = int(u32(opt.get("robust_scale", 0.0)))
            assert dev_bits(b)[2] == [(s.pairs, s.pairs, 0, scale) for s in a.trace] and len(b.info) == len(a.trace)
        c = lgr.icp_trim(d_src, d_tgt, T0, **kw)   # without a trace: info all the same
        assert c.trace is None and dev_bits(c)[2] == dev_bits(b)[2]
        check(b, TR.icp(pair["src"], pair["tgt"], T0, **kw))


def dev_bits_ex(r):
    r.info = []
    return dev_bits(r)


def test_refusals_and_idle_calls(lgr, pair):
    from lgr_amd import capi
    d_src, d_tgt, T0 = pair["d_src"], pair["d_tgt"], pair["T_near"]
    nan, inf = float("nan"), float("inf")
    bad = [dict(keep=nan), dict(keep=0.0), dict(keep=-0.5), dict(keep=1.5), dict(keep=inf), dict(robust=2, robust_scale=1.0, scale_from_median=nan),
           dict(robust=2, robust_scale=1.0, scale_from_median=-1.0), dict(robust=2, robust_scale=1.0, scale_from_median=inf), dict(scale_from_median=1.0),
           dict(keep=0.5, robust=1, robust_scale=0.0), dict(keep=0.5, robust=1, robust_scale=nan),
           # whatever lgr_icp_ex* refuses, under a configuration that is not neutral
           dict(keep=0.5, variant=3), dict(keep=0.5, robust=4), dict(keep=0.5, min_normal_cos=1.5), dict(keep=0.5, plane_eps=2.0), dict(keep=0.5, max_iterations=-1),
           dict(keep=0.5, max_dist=nan), dict(keep=0.5, shrink=0.0), dict(robust=1, scale_from_median=1.0, rot_eps=-1.0), dict(variant=-1), dict(max_dist=0.1, min_dist=0.2)]
    for kw in bad:
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.icp_trim(d_src, d_tgt, T0, **kw)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.icp_trim_host(pair["src"], pair["tgt"], T0, **kw)
    # with scale_from_median > 0 the caller's scale is neither read nor validated
    for rs in (0.0, -1.0, nan):
        a = lgr.icp_trim(d_src, d_tgt, T0, robust="cauchy", robust_scale=rs, scale_from_median=MAD, max_iterations=2, max_dist=0.1)
        assert a.iterations == 2 and a.info[0].scale > 0
    out, n = capi.IcpResult(), C.c_int(-7)
    p = capi.icp_trim_params(keep=0.5, max_iterations=3, max_dist=0.1)
    info = (capi.IcpTrimStep * 3)()
    L = capi.lib()
    for fn, efn, a, b in ((L.lgr_icp_trim_dev, L.lgr_icp_ex_dev, d_src, d_tgt), (L.lgr_icp_trim_host, L.lgr_icp_ex_host, pair["src"], pair["tgt"])):
        args = lambda **k: [k.get("src", capi._ptr(a)), k.get("ns", len(pair["src"])), k.get("tgt", capi._ptr(b)), len(pair["tgt"]), k.get("T", lgr._T16(T0)),  # noqa: E731
                            k.get("p", C.byref(p)), k.get("out", C.byref(out)), k.get("trace"), k.get("info"), k.get("n")]
        for k in (dict(src=None), dict(tgt=None), dict(T=None), dict(p=None), dict(out=None), dict(ns=-1), dict(trace=(capi.IcpStep * 3)()), dict(info=info)):
            assert fn(lgr.h, *args(**k)) == -1, list(k)
        for w in range(2):   # the reserved words at every level
            p.reserved[w] = 1
            assert fn(lgr.h, *args()) == -1
            p.reserved[w] = 0
        p.ex.reserved[1] = 1
        assert fn(lgr.h, *args()) == -1
        p.ex.reserved[1] = 0
        p.ex.base.reserved[0] = 1
        assert fn(lgr.h, *args()) == -1
        p.ex.base.reserved[0] = 0
        assert fn(lgr.h, *args(info=info, n=C.byref(n))) == 0 and out.iterations == 3 and n.value == 3 and info[2].kept == TR.trim_k(0.5, info[2].candidates)
        # the idle calls: what lgr_icp_ex* returns, and no info
        for ns, m in ((len(pair["src"]), 0), (0, 5)):
            p.ex.base.max_iterations = m
            C.memset(info, 0xCD, C.sizeof(info))
            n.value = -7
            assert fn(lgr.h, *args(ns=ns, info=info, n=C.byref(n))) == 0 and n.value == 0
            assert bytes(info) == bytes([0xCD]) * C.sizeof(info)
            ex, pe = capi.IcpResult(), capi.icp_ex_params(max_iterations=m, max_dist=0.1)
            assert efn(lgr.h, capi._ptr(a), ns, capi._ptr(b), len(pair["tgt"]), lgr._T16(T0), C.byref(pe), C.byref(ex), None, None) == 0
            assert bytes(ex) == bytes(out)
        p.ex.base.max_iterations = 3
    # lgr_icp_ex, lgr_icp_trim, lgr_icp_ex on one context: the first call's bytes
    kw = dict(pair["kw"], max_iterations=G + 1)
    a = lgr.icp_ex(d_src, d_tgt, T0, trace=True, **kw)
    lgr.icp_trim(d_src, d_tgt, T0, keep=0.6, robust="tukey", scale_from_median=2.0, trace=True, **kw)
    b = lgr.icp_ex(d_src, d_tgt, T0, trace=True, **kw)
    assert dev_bits_ex(a) == dev_bits_ex(b)
