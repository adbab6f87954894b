"""Loader of tests/cpp/teaser_ref.cpp (the CPU statement of the TEASER alignment), compiled once per session with
g++ -O2 -ffp-contract=off into a temporary directory.  numpy in, numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "teaser_ref.cpp")
NODES_MAX = 2048
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="teaser_ref_"), "libteaser_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clique(A):
    """steps 3 and 4 on a 0/1 matrix -> dict(core [K], max_core, n_core, clique [n_clique] ascending positions)"""
    A = np.ascontiguousarray(A, np.uint8)
    K = A.shape[0]
    assert A.shape == (K, K) and np.array_equal(A, A.T) and not A.diagonal().any()
    core = np.zeros(K, np.int32); q = np.zeros(K, np.int32)
    mc = C.c_int(0); nc = C.c_int(0)
    n = lib().teaser_ref_clique(_p(A), K, _p(core), C.byref(mc), C.byref(nc), _p(q))
    return dict(core=core, max_core=mc.value, n_core=nc.value, clique=q[:n].copy())


def gnc(a, b, beta, max_iterations=100, gnc_factor=1.4, cost_threshold=0.005):
    """step 5 on TIM lists a, b [n, 3] -> dict(R [3, 3], w [n], iterations, cost, n_inliers)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    n = a.shape[0]
    R = np.zeros(9, np.float32); w = np.zeros(n, np.float32)
    it = C.c_int(0); cost = C.c_float(0); nin = C.c_int(0)
    lib().teaser_ref_gnc(_p(a), _p(b), n, C.c_float(beta), int(max_iterations), C.c_float(gnc_factor), C.c_float(cost_threshold), _p(R), _p(w),
                         C.byref(it), C.byref(cost), C.byref(nin))
    return dict(R=R.reshape(3, 3), w=w, iterations=it.value, cost=cost.value, n_inliers=nin.value)


def tls(x, beta):
    """step 6 on one axis -> (shift, cost, consensus flags of the chosen centre)"""
    x = np.ascontiguousarray(x, np.float32)
    shift = C.c_float(0); cost = C.c_float(0)
    flags = np.zeros(x.shape[0], np.uint8)
    lib().teaser_ref_tls(_p(x), x.shape[0], C.c_float(beta), C.byref(shift), C.byref(cost), _p(flags))
    return np.float32(shift.value), np.float32(cost.value), flags


def degrees(src, tgt, corr, beta):
    src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32); corr = np.ascontiguousarray(corr)
    deg = np.zeros(max(corr.shape[0], 1), np.int32)
    assert lib().teaser_ref_degrees(_p(src), src.shape[0], _p(tgt), tgt.shape[0], _p(corr), corr.shape[0], C.c_float(beta), _p(deg)) == 0
    return deg[: corr.shape[0]]


INFO_INT = ("valid", "n_nodes", "max_core", "n_core", "n_clique", "rotation_iterations", "n_rotation_inliers", "n_translation_inliers")


def teaser(src, tgt, corr, beta, k_select=0, max_iterations=100, gnc_factor=1.4, cost_threshold=0.005):
    """the whole call -> dict(rc, T [4, 4], the lgr_teaser_info fields, n_inliers, clique, nodes, mask); rc -1: an index outside its cloud"""
    src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32); corr = np.ascontiguousarray(corr)
    c = corr.shape[0]
    T = np.zeros(16, np.float32); ii = np.zeros(9, np.int32); ff = np.zeros(4, np.float32)
    lists = np.zeros(2 * NODES_MAX, np.int32); mask = np.zeros(max(c, 1), np.uint8)
    rc = lib().teaser_ref(_p(src), src.shape[0], _p(tgt), tgt.shape[0], _p(corr), c, C.c_float(beta), int(k_select), int(max_iterations),
                          C.c_float(gnc_factor), C.c_float(cost_threshold), _p(T), _p(ii), _p(ff), _p(lists), _p(mask))
    out = dict(rc=rc, T=T.reshape(4, 4).T.copy(), n_inliers=int(ii[8]), rotation_cost=np.float32(ff[0]), translation_cost=ff[1:4].copy(),
               clique=lists[: ii[4]].copy(), nodes=lists[NODES_MAX: NODES_MAX + ii[1]].copy(), lists=lists, mask=mask[:c].copy())
    out.update({k: int(ii[j]) for j, k in enumerate(INFO_INT)})
    return out
