"""Loader of tests/cpp/knn_match_ref.cpp (the CPU statement of the k-nearest brute-force matcher), compiled once per session with
g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out: (idx int32 [mq, k], dist float32 [mq, k])."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "knn_match_ref.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="knn_ref_"), "libknn_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        _lib.knn_ref_l2sqr.restype = C.c_float
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(fn, q, t, k, *block):
    q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
    assert q.shape[1] == t.shape[1]
    idx = np.zeros((q.shape[0], k), np.int32); dist = np.zeros((q.shape[0], k), np.float32)
    fn(q.shape[1], _p(q), q.shape[0], _p(t), t.shape[0], *[int(b) for b in block], int(k), _p(idx), _p(dist))
    return idx, dist


def match(q, t, block, k):
    """the procedure: per bf block the K-list, then the insertion of updateMultivaluedCorrespondence"""
    return _run(lib().knn_ref_match, q, t, k, block)


def closed(q, t, block, k):
    """the closed form: the first k of the blocks' lists in (d ascending, block descending, index descending)"""
    return _run(lib().knn_ref_closed, q, t, k, block)


def plain(q, t, k):
    """the first k of all rows in (d ascending, index ascending)"""
    return _run(lib().knn_ref_plain, q, t, k)


def tie_rows(rng, m, dim, lo=3, hi=6, levels=3):
    """integer-valued rows, each distinct row repeated lo..hi times, shuffled: equal distances within and across bf blocks"""
    rows = []
    while len(rows) < m:
        r = rng.integers(0, levels, dim).astype(np.float32)
        rows += [r] * int(rng.integers(lo, hi + 1))
    rows = np.stack(rows[:m])
    return np.ascontiguousarray(rows[rng.permutation(m)])
