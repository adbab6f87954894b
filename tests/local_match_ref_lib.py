"""Loader of tests/cpp/local_match_ref.cpp (the CPU statement of matchLocal with a k-list and of the FLANN-contract distance), compiled
once per session with g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "local_match_ref.cpp")
FLT_MAX = 3.4028234663852886e38
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="local_ref_"), "liblocal_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def match(qpts, tpts, q, t, guess, radius, k=1, counts=False):
    """the statement: (idx int32 [mq, k], dist float32 [mq, k]) and, with counts, every query's number of candidates"""
    qpts = np.ascontiguousarray(qpts, np.float32); tpts = np.ascontiguousarray(tpts, np.float32)
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    assert q.shape[1] == t.shape[1] and qpts.shape == (q.shape[0], 12) and tpts.shape == (t.shape[0], 12)
    g = np.ascontiguousarray(np.asarray(guess, np.float32).T).reshape(16)   # column-major
    idx = np.zeros((q.shape[0], k), np.int32); dist = np.zeros((q.shape[0], k), np.float32)
    n_cand = np.zeros(q.shape[0], np.int32)
    lib().local_ref_match(int(q.shape[1]), _p(qpts), q.shape[0], _p(tpts), t.shape[0], _p(q), _p(t), _p(g), C.c_float(radius), int(k),
                          _p(idx), _p(dist), _p(n_cand))
    return (idx, dist, n_cand) if counts else (idx, dist)


def flann_dist(q, t, idx):
    """sqrt of the sequential sum of squares between query i and train row idx[i] (0 where idx[i] < 0)"""
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    idx = np.ascontiguousarray(idx, np.int32)
    dist = np.zeros(q.shape[0], np.float32)
    lib().local_ref_flann_dist(int(q.shape[1]), _p(q), q.shape[0], _p(t), _p(idx), _p(dist))
    return dist


def knn_list(capacity, adds):
    """adds: [(dist, index), ...] through the list rule -> (indices, distances)"""
    d = np.array([a[0] for a in adds], np.float32); i = np.array([a[1] for a in adds], np.int32)
    oi = np.zeros(capacity, np.int32); od = np.zeros(capacity, np.float32)
    n = lib().local_ref_list(int(capacity), len(adds), _p(d), _p(i), _p(oi), _p(od))
    return oi[:n].tolist(), od[:n].tolist()


def pts12(xyz):
    """[m, 3] -> the library's point rows [m, 12] (x y z first, the rest 0)"""
    xyz = np.asarray(xyz, np.float32)
    out = np.zeros((xyz.shape[0], 12), np.float32)
    out[:, :3] = xyz
    return out
