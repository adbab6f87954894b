"""Loader of tests/cpp/rops_ref.cpp (the CPU statement of the gravity frames, the RoPS135 rows and the 135-d matcher), compiled once
per session with g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out.  The SHOT frames of the
key points that fail the gravity test come from tests/shot_ref_lib.py."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shot_ref_lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rops_ref.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="rops_ref_"), "librops_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.rops_ref_l2sqr.restype = C.c_float
        _lib.rops_ref_count_logf.restype = C.c_longlong
        _lib.rops_ref_count_logf.argtypes = [C.c_uint, C.c_uint]
        _lib.rops_ref_cast_u32.restype = C.c_uint
        _lib.rops_ref_cast_u32.argtypes = [C.c_float]
        _lib.rops_ref_bin.restype = C.c_uint
        _lib.rops_ref_bin.argtypes = [C.c_float]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def gravity_only(kps):
    """(frames [m, 9] with NaN rows where the angle test fails, fail mask [m] bool)"""
    kps = np.ascontiguousarray(kps, np.float32)
    m = kps.shape[0]
    fr = np.zeros((m, 9), np.float32); fail = np.zeros(m, np.int32)
    lib().rops_ref_gravity(_p(kps), m, _p(fr), _p(fail))
    return fr, fail.astype(bool)


def gravity_lrf(kps, surf, radius):
    """gravity frames [m, 9]; the failing key points get the SHOT frame on (surf, radius)"""
    fr, fail = gravity_only(kps)
    if fail.any():
        _, sf = shot_ref_lib.shot(np.ascontiguousarray(kps[fail], np.float32), surf, radius)
        fr[fail] = sf
    return fr


def rops(kps, surf, radius, lrf):
    kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
    lrf = np.ascontiguousarray(lrf, np.float32)
    out = np.zeros((kps.shape[0], 135), np.float32)
    lib().rops_ref(_p(kps), kps.shape[0], _p(surf), surf.shape[0], C.c_float(radius), _p(lrf), _p(out))
    return out


def row(pts):
    """one row from an explicit transformed support [n, 3]"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    out = np.zeros(135, np.float32)
    lib().rops_ref_row(_p(pts), pts.shape[0], _p(out))
    return out


def count_logf_mismatch(lo_bits, hi_bits):
    return int(lib().rops_ref_count_logf(lo_bits, hi_bits))


def cast_u32(x):
    return int(lib().rops_ref_cast_u32(float(x)))


def bin_rule(x):
    return int(lib().rops_ref_bin(float(x)))


def match(q, t, block):
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
    lib().rops_ref_match(_p(q), q.shape[0], _p(t), t.shape[0], int(block), _p(idx), _p(dist))
    return idx, dist


def l2sqr(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return np.float32(lib().rops_ref_l2sqr(_p(a), _p(b)))
