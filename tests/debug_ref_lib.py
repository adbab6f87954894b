"""Loader of tests/cpp/debug_ref.cpp (the CPU statement of the temperature maps, the hypothesis overlap comparison, the far-safe nearest
neighbour and the colour passes, include/lgr.h lgr_temperature_map* ... lgr_color_correspondences*), compiled once per session with
g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "debug_ref.cpp")
CORR_DTYPE = np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4"), ("threshold", "<f4")])
COLOR_BEIGE, COLOR_RED, COLOR_PARAKEET, COLOR_BLUE, COLOR_WHITE = 0xf8c471, 0xff0000, 0x03c04a, 0x0000ff, 0xffffff
TEMP_FIELDS = ("temp_distance", "temp_normal", "color_distance", "color_normal", "nn")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="debug_ref_"), "libdebug_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        for f in (_lib.dref_color_map, _lib.dref_color_weights, _lib.dref_color_correspondences, _lib.dref_move, _lib.dref_nearest,
                  _lib.dref_temperature_map, _lib.dref_temperature_maps, _lib.dref_compare_overlaps):
            f.restype = None
        _lib.dref_get_color.restype = C.c_int
        _lib.dref_get_color.argtypes = [C.c_float, C.c_float, C.c_float]
        _lib.dref_mix_color.restype = C.c_int
        _lib.dref_mix_color.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.dref_quantile.restype = C.c_float
        _lib.dref_quantile.argtypes = [C.c_double, C.c_void_p, C.c_int]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def T16(T):
    """4x4 -> 16 floats column-major"""
    return _f32(np.asarray(T, np.float32).T.reshape(16))


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def get_color(v, vmin, vmax):
    return lib().dref_get_color(float(np.float32(v)), float(np.float32(vmin)), float(np.float32(vmax)))


def mix_color(color, mix=COLOR_WHITE, times=1):
    return lib().dref_mix_color(int(color), int(mix), int(times))


def quantile(q, values):
    v = _f32(values)
    return np.float32(lib().dref_quantile(float(q), _p(v), len(v)))


def color_map(values, vmin, vmax):
    v = _f32(values)
    out = np.zeros(len(v), np.int32)
    lib().dref_color_map(_p(v), len(v), C.c_float(vmin), C.c_float(vmax), _p(out))
    return out


def color_weights(w):
    """-> (colours, (q01, q99))"""
    w = _f32(w)
    out = np.zeros(len(w), np.int32)
    r = np.zeros(2, np.float32)
    lib().dref_color_weights(_p(w), len(w), _p(out), _p(r))
    return out, r


def _corr(c):
    return np.zeros(0, CORR_DTYPE) if c is None else np.ascontiguousarray(np.asarray(c).view(CORR_DTYPE).reshape(-1))


def color_correspondences(n, kp, corr, correct, inliers, is_source):
    kpa = None if kp is None else np.ascontiguousarray(kp, np.int32)
    corr, correct, inliers = _corr(corr), _corr(correct), _corr(inliers)
    out = np.zeros(n, np.int32)
    lib().dref_color_correspondences(n, _p(kpa), 0 if kpa is None else len(kpa), int(kp is not None), _p(corr), len(corr), _p(correct), len(correct),
                                     _p(inliers), len(inliers), int(bool(is_source)), _p(out))
    return out


def move(src, T):
    src = _f32(src)
    out = np.zeros_like(src)
    lib().dref_move(_p(src), src.shape[0], _p(T16(T)), _p(out))
    return out


def nearest(q, pts):
    """-> (idx int32 [nq], d2 float32 [nq])"""
    q = _f32(q); pts = _f32(pts)
    idx = np.zeros(max(q.shape[0], 1), np.int32); d2 = np.zeros(max(q.shape[0], 1), np.float32)
    lib().dref_nearest(_p(q), q.shape[0], _p(pts), pts.shape[0], _p(idx), _p(d2))
    return idx[:q.shape[0]], d2[:q.shape[0]]


def _temp_arrays(n):
    m = max(n, 1)
    return [np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)]


def temperature_map(cmp, ref, dmax):
    """-> dict(temp_distance, temp_normal, color_distance, color_normal, nn, n_below)"""
    cmp = _f32(cmp); ref = _f32(ref)
    n = cmp.shape[0]
    a = _temp_arrays(n)
    nb = C.c_int(0)
    lib().dref_temperature_map(_p(cmp), n, _p(ref), ref.shape[0], C.c_float(dmax), *[_p(x) for x in a], C.byref(nb))
    out = {k: v[:n] for k, v in zip(TEMP_FIELDS, a)}
    out["n_below"] = nb.value
    return out


def temperature_maps(src, tgt, T, thr):
    """-> dict(src=<as temperature_map>, tgt=<...>, moved [ns, 12])"""
    src = _f32(src); tgt = _f32(tgt)
    ns, nt = src.shape[0], tgt.shape[0]
    a, b = _temp_arrays(ns), _temp_arrays(nt)
    moved = np.zeros((max(ns, 1), 12), np.float32)
    nb = (C.c_int * 2)()
    lib().dref_temperature_maps(_p(src), ns, _p(tgt), nt, _p(T16(T)), C.c_float(thr), *[_p(x) for x in a], *[_p(x) for x in b], _p(moved), nb)
    s = {k: v[:ns] for k, v in zip(TEMP_FIELDS, a)}
    t = {k: v[:nt] for k, v in zip(TEMP_FIELDS, b)}
    s["n_below"], t["n_below"] = nb[0], nb[1]
    return dict(src=s, tgt=t, moved=moved[:ns])


def compare_overlaps(src, tgt, Ts, thr):
    """-> dict(counts [n], weighted [n], counts2 [n, 2], mask_src [n, ns], mask_tgt [n, nt])"""
    src = _f32(src); tgt = _f32(tgt)
    ns, nt, n = src.shape[0], tgt.shape[0], len(Ts)
    tns = _f32(np.concatenate([T16(T) for T in Ts])) if n else np.zeros(0, np.float32)
    counts = np.zeros(max(n, 1), np.int32); w = np.zeros(max(n, 1), np.float32); c2 = np.zeros((max(n, 1), 2), np.int32)
    msb = np.zeros(max(n * ns, 1), np.uint8); mtb = np.zeros(max(n * nt, 1), np.uint8)
    lib().dref_compare_overlaps(_p(src), ns, _p(tgt), nt, _p(tns), n, C.c_float(thr), _p(counts), _p(w), _p(c2), _p(msb), _p(mtb))
    return dict(counts=counts[:n], weighted=w[:n], counts2=c2[:n], mask_src=msb[:n * ns].reshape(n, ns), mask_tgt=mtb[:n * nt].reshape(n, nt))
