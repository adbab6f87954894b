"""Loader of tests/cpp/icp_ex_ref.cpp (the CPU statement of the ICP variants, include/lgr.h lgr_icp_ex*, DESIGN.md section 4, "ICP
variants"), compiled once per session with g++ -O2 -ffp-contract=off -fopenmp into a temporary directory; the step's arithmetic, the 3 x 3
inverse and the robust weights are csrc/lgr_icp_math.h, the text the device compiles too.  numpy in, numpy out; the result has the shape
of icp_ref_lib.icp's."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref_lib as I  # noqa: E402

SRC = os.path.join(I.ROOT, "tests", "cpp", "icp_ex_ref.cpp")
POINT_TO_PLANE, POINT_TO_POINT, PLANE_TO_PLANE = 0, 1, 2
NONE, HUBER, CAUCHY, TUKEY = 0, 1, 2, 3
VARIANTS, ROBUSTS = (POINT_TO_PLANE, POINT_TO_POINT, PLANE_TO_PLANE), (NONE, HUBER, CAUCHY, TUKEY)
F = np.float32
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="icp_ex_ref_"), "libicp_ex_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-I", I.CSRC, "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.icpexref_robust_weight.restype = C.c_double
        _lib.icpexref_robust_weight.argtypes = [C.c_int, C.c_double, C.c_double]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def inv_sym3(S):
    """the inverse of the symmetric 3 x 3 S through icp_inv_sym3 -> [3, 3] or None (a refused determinant)"""
    S = np.asarray(S, np.float64)
    s6 = np.ascontiguousarray([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
    m = np.zeros(6)
    if not lib().icpexref_inv_sym3(_p(s6), _p(m)):
        return None
    return np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])


def robust_weight(kind, rho, k):
    return lib().icpexref_robust_weight(int(kind), float(rho), float(k))


def icp(src, tgt, T0, variant=POINT_TO_PLANE, robust=NONE, robust_scale=0.0, min_normal_cos=-1.0, plane_eps=0.0, weights=None, max_iterations=30, max_dist=0.0,
        min_dist=0.0, shrink=1.0, rot_eps=1e-6, trans_eps=1e-6, density=None):
    """the statement -> the dict of icp_ref_lib.icp.  The base keywords are resolved as there (max_dist <= 0: 4 x density)."""
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
    n = lib().icpexref_run(_p(src), ns, _p(tgt), len(tgt), _p(T16), int(max_iterations), C.c_float(md), C.c_float(mn), C.c_float(shrink), C.c_float(rot_eps),
                           C.c_float(trans_eps), int(variant), int(robust), C.c_float(robust_scale), C.c_float(min_normal_cos), C.c_float(eps), _p(w),
                           C.byref(out), trace)
    mat = lambda s: np.array(s.T, F).reshape(4, 4).T.copy()   # noqa: E731
    return dict(T=mat(out), iterations=out.iterations, stop=out.stop, max_dist=F(out.max_dist), pairs=out.pairs, rmse=F(out.rmse), pairs0=out.pairs0,
                rmse0=F(out.rmse0), trace=[dict(T=mat(s), dist=F(s.dist), pairs=s.pairs, rmse=F(s.rmse), rot=F(s.rot), trans=F(s.trans)) for s in trace[:n]])


def bits(r):
    """a statement result and its trace as comparable integers (every float as its uint32)"""
    u = lambda v: np.asarray(v, F).view(np.uint32)   # noqa: E731
    head = (u(r["T"].T.reshape(16)).tolist(), r["iterations"], r["stop"], int(u(r["max_dist"])), r["pairs"], int(u(r["rmse"])), r["pairs0"], int(u(r["rmse0"])))
    return head, [(u(s["T"].T.reshape(16)).tolist(), int(u(s["dist"])), s["pairs"], int(u(s["rmse"])), int(u(s["rot"])), int(u(s["trans"]))) for s in r["trace"]]


_runs = {}


def reference(key, *args, **kw):
    """icp(*args, **kw) computed once per key and shared among the tests"""
    if key not in _runs:
        _runs[key] = icp(*args, **kw)
    return _runs[key]
