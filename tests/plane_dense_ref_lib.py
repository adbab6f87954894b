"""Loader of tests/cpp/plane_dense_ref.cpp (the CPU statement of the dense closest-plane evaluation, include/lgr.h
lgr_evaluate_plane_dense*), compiled once per session with g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in,
numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plane_dense_ref.cpp")
CORR_DTYPE = np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4"), ("threshold", "<f4")])
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="plane_dense_ref_"), "libplane_dense_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.pdref_evaluate.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def T16(T):
    """4x4 -> 16 floats column-major"""
    return _f32(np.asarray(T, np.float32).T.reshape(16))


def bits(x):
    """the bit pattern(s) of float32 value(s)"""
    return np.asarray(x, np.float32).view(np.uint32)


def evaluate(src, tgt, T, score_id, thr, weights=None):
    """-> dict(n_inliers, rmse, metric, score (np.float32), threshold, inliers [n_inliers] CORR_DTYPE, nn [ns] int32)"""
    src = _f32(src); tgt = _f32(tgt)
    ns = src.shape[0]
    w = None if weights is None else _f32(weights)
    rmse, metric, score = C.c_float(0), C.c_float(0), C.c_float(0)
    inl = np.zeros(max(ns, 1), CORR_DTYPE)
    nn = np.zeros(max(ns, 1), np.int32)
    n = lib().pdref_evaluate(_p(src), ns, _p(tgt), tgt.shape[0], _p(T16(T)), int(score_id), _p(w), C.c_float(thr), C.byref(rmse), C.byref(metric),
                             C.byref(score), _p(inl), _p(nn))
    return dict(n_inliers=n, rmse=np.float32(rmse.value), metric=np.float32(metric.value), score=np.float32(score.value), threshold=np.float32(thr),
                inliers=inl[:n].copy(), nn=nn[:ns].copy())
