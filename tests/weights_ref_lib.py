"""Loader of tests/cpp/weights_ref.cpp (the CPU statement of weighted_closest_plane's point weights and weighted plane metric), compiled
once per session with g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "weights_ref.cpp")
WEIGHTS = {"constant": 0, "exp_curvature": 1, "curvedness": 2, "harris": 3, "tomasi": 4, "curvature": 5, "nss": 6}
BUILT = ("constant", "exp_curvature", "curvedness", "curvature", "nss")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="weights_ref_"), "libweights_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.wref_quantile.restype = C.c_float
        _lib.wref_quantile.argtypes = [C.c_double, C.c_void_p, C.c_int]
        _lib.wref_nss_bin.restype = C.c_int
        _lib.wref_nss_bin.argtypes = [C.c_float, C.c_float, C.c_float]
        _lib.wref_plane_metric.restype = C.c_float
        _lib.wref_plane_metric.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_float]
        _lib.wref_count_libm.restype = C.c_longlong
        _lib.wref_count_libm.argtypes = [C.c_int, C.c_uint, C.c_uint]
        _lib.wref_libm.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def knn(pts, k=30):
    pts = _f32(pts)
    idx = np.zeros((pts.shape[0], k), np.int32)
    lib().wref_knn(_p(pts), pts.shape[0], k, _p(idx))
    return idx


def principal_curvatures(pts, k=30, idx=None):
    pts = _f32(pts)
    idx = knn(pts, k) if idx is None else np.ascontiguousarray(idx, np.int32)
    pc1 = np.zeros(pts.shape[0], np.float32); pc2 = np.zeros(pts.shape[0], np.float32)
    lib().wref_pcs(_p(pts), pts.shape[0], k, _p(idx), _p(pc1), _p(pc2))
    return pc1, pc2


def weights(pts, weight, k=30, idx=None):
    """(weights [n], weights_sum) of the named weight function"""
    pts = _f32(pts)
    wid = WEIGHTS[weight]
    if wid in (1, 2) and idx is None:
        idx = knn(pts, k)
    w = np.zeros(pts.shape[0], np.float32)
    s = C.c_float(0)
    rc = lib().wref_weights(_p(pts), pts.shape[0], wid, k, _p(None if idx is None else np.ascontiguousarray(idx, np.int32)), _p(w), C.byref(s))
    assert rc == 0, weight
    return w, s.value


def quantile(values, q=0.8):
    v = _f32(values)
    return lib().wref_quantile(q, _p(v), v.shape[0])


def nss_bin(nx, ny, nz):
    return lib().wref_nss_bin(nx, ny, nz)


def plane_metric(src, tgt, T, score_id, thr, pairs, w, weights_sum):
    """weighted metric of a transform (4x4) over its plane pairs [np, 2] (source index, target index)"""
    src = _f32(src); tgt = _f32(tgt); w = _f32(w)
    T16 = _f32(np.asarray(T, np.float32).T.reshape(16))
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return lib().wref_plane_metric(_p(src), _p(tgt), _p(T16), int(score_id), float(np.float32(thr)), _p(pairs), pairs.shape[0], _p(w),
                                   float(np.float32(weights_sum)))


def count_libm_mismatch(fn, lo_bits, hi_bits):
    return lib().wref_count_libm(int(fn), int(lo_bits), int(hi_bits))


def host_libm(fn, a):
    a = _f32(a)
    out = np.zeros_like(a)
    lib().wref_libm(int(fn), _p(a), a.shape[0], _p(out))
    return out
