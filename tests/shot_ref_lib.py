"""Loader of tests/cpp/shot_ref.cpp (the CPU statement of the SHOT stage and the 352-d matcher), compiled once per session with
g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shot_ref.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="shot_ref_"), "libshot_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.shot_ref_l2sqr.restype = C.c_float
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def shot(kps, surf, radius, lrf=None):
    """(rows [m, 352], frames [m, 9]) of the reference; lrf: given frames or None."""
    kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
    m = kps.shape[0]
    out = np.zeros((m, 352), np.float32); fr = np.zeros((m, 9), np.float32)
    lrf = None if lrf is None else np.ascontiguousarray(lrf, np.float32)
    lib().shot_ref(_p(kps), m, _p(surf), surf.shape[0], C.c_float(radius), _p(lrf), _p(fr), _p(out))
    return out, fr


def frame_margins(kps, surf, radius):
    """[m, 5] float64: eigenvalues of the frame's covariance (ascending) and the x / z sign votes before the tie-break (NaN: no frame)."""
    kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
    out = np.zeros((kps.shape[0], 5), np.float64)
    lib().shot_ref_frame_margins(_p(kps), kps.shape[0], _p(surf), surf.shape[0], C.c_float(radius), _p(out))
    return out


def match(q, t, block):
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
    lib().shot_ref_match(_p(q), q.shape[0], _p(t), t.shape[0], int(block), _p(idx), _p(dist))
    return idx, dist


def l2sqr(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return np.float32(lib().shot_ref_l2sqr(_p(a), _p(b)))


def acos(x, which="shot"):
    x = np.ascontiguousarray(x, np.float64); out = np.empty_like(x)
    getattr(lib(), "shot_ref_acos" if which == "shot" else "libm_acos")(_p(x), C.c_longlong(x.size), _p(out))
    return out


def atan2(y, x, which="shot"):
    y = np.ascontiguousarray(y, np.float64); x = np.ascontiguousarray(x, np.float64); out = np.empty_like(x)
    getattr(lib(), "shot_ref_atan2" if which == "shot" else "libm_atan2")(_p(y), _p(x), C.c_longlong(x.size), _p(out))
    return out
