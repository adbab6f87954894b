"""Loader of tests/cpp/icp_trim_ref.cpp (the CPU statement of trimmed ICP, include/lgr.h lgr_icp_trim*, DESIGN.md section 4, "Trimmed
ICP"), compiled once per session like the statement of the variants (g++ -O2 -ffp-contract=off -fopenmp); the shared scalar pieces are
csrc/lgr_icp_math.h, the text the device compiles too.  numpy in, numpy out: the dict of icp_ex_ref_lib.icp plus `info`, one
dict(candidates, kept, cut, scale) per evaluated iteration."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ex_ref_lib as X  # noqa: E402
import icp_ref_lib as I  # noqa: E402

SRC = os.path.join(I.ROOT, "tests", "cpp", "icp_trim_ref.cpp")
F = np.float32
_lib = None


class TrimStep(C.Structure):
    """lgr_icp_trim_step (include/lgr.h)"""
    _fields_ = [("candidates", C.c_int32), ("kept", C.c_int32), ("cut", C.c_float), ("scale", C.c_float)]


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="icp_trim_ref_"), "libicp_trim_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-I", I.CSRC, "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.icptrimref_k.restype = C.c_longlong
        _lib.icptrimref_k.argtypes = [C.c_float, C.c_longlong]
        _lib.icptrimref_median_rank.restype = C.c_longlong
        _lib.icptrimref_median_rank.argtypes = [C.c_longlong]
        _lib.icptrimref_scale.restype = C.c_double
        _lib.icptrimref_scale.argtypes = [C.c_float, C.c_float, C.c_float]
        _lib.icptrimref_weight.restype = C.c_double
        _lib.icptrimref_weight.argtypes = [C.c_int, C.c_double, C.c_double]
        _lib.icptrimref_key.argtypes = [C.c_double, C.POINTER(C.c_uint32)]
    return _lib


def trim_k(keep, P):
    return lib().icptrimref_k(float(F(keep)), int(P))


def median_rank(P):
    return lib().icptrimref_median_rank(int(P))


def scale(scale_from_median, key_median, robust_scale=0.0):
    return lib().icptrimref_scale(float(F(scale_from_median)), float(F(key_median)), float(F(robust_scale)))


def weight(kind, rho, k):
    return lib().icptrimref_weight(int(kind), float(rho), float(k))


def key(rho):
    """(candidate?, the key's bits)"""
    b = C.c_uint32(0)
    ok = lib().icptrimref_key(float(rho), C.byref(b))
    return bool(ok), b.value


def icp(src, tgt, T0, keep=1.0, scale_from_median=0.0, variant=X.POINT_TO_PLANE, robust=X.NONE, robust_scale=0.0, min_normal_cos=-1.0, plane_eps=0.0, weights=None,
        max_iterations=30, max_dist=0.0, min_dist=0.0, shrink=1.0, rot_eps=1e-6, trans_eps=1e-6, density=None):
    """the statement -> the dict of icp_ex_ref_lib.icp plus info.  The keywords are resolved as there."""
    src = np.ascontiguousarray(src, F); tgt = np.ascontiguousarray(tgt, F)
    ns = len(src)
    idle = ns == 0 or max_iterations == 0
    md = F(max_dist)
    if not md > 0:
        md = F(0) if idle else F(4) * F(density)
    mn = F(min_dist) if F(min_dist) > 0 else md
    assert idle or (md > 0 and mn <= md)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, F)
        assert w.shape == (ns,)
    eps = F(plane_eps) if F(plane_eps) != 0 else F(1e-3)
    T16 = np.ascontiguousarray(np.asarray(T0, F).T.reshape(16))
    out = I.Result()
    trace = (I.Step * max(max_iterations, 1))()
    info = (TrimStep * max(max_iterations, 1))()
    n = lib().icptrimref_run(X._p(src), ns, X._p(tgt), len(tgt), X._p(T16), int(max_iterations), C.c_float(md), C.c_float(mn), C.c_float(shrink), C.c_float(rot_eps),
                             C.c_float(trans_eps), int(variant), int(robust), C.c_float(robust_scale), C.c_float(min_normal_cos), C.c_float(eps), X._p(w),
                             C.c_float(keep), C.c_float(scale_from_median), C.byref(out), trace, info)
    mat = lambda s: np.array(s.T, F).reshape(4, 4).T.copy()   # noqa: E731
    return dict(T=mat(out), iterations=out.iterations, stop=out.stop, max_dist=F(out.max_dist), pairs=out.pairs, rmse=F(out.rmse), pairs0=out.pairs0,
                rmse0=F(out.rmse0), trace=[dict(T=mat(s), dist=F(s.dist), pairs=s.pairs, rmse=F(s.rmse), rot=F(s.rot), trans=F(s.trans)) for s in trace[:n]],
                info=[dict(candidates=s.candidates, kept=s.kept, cut=F(s.cut), scale=F(s.scale)) for s in info[:n]])


def bits(r):
    """icp_ex_ref_lib.bits plus the info entries, every float as its uint32"""
    u = lambda v: int(np.asarray(v, F).view(np.uint32))   # noqa: E731
    return X.bits(r) + ([(s["candidates"], s["kept"], u(s["cut"]), u(s["scale"])) for s in r["info"]],)
