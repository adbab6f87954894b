"""Loader of tests/cpp/hash_order_ref.cpp (this compiler's std::hash and std::unordered_map / unordered_set beside the restatement in
csrc/lgr_stdhash.h), compiled once per session with g++ -O2 into a temporary directory.  numpy in, numpy out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "hash_order_ref.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="hash_order_ref_"), "libhash_order_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pair(fn, a, n):
    s = np.zeros(n, np.uint64); h = np.zeros(n, np.uint64)
    fn(_p(a), C.c_longlong(n), _p(s), _p(h))
    return s, h


def hash_float(bits):
    """(std::hash<float>, header) of the floats with these bit patterns"""
    bits = np.ascontiguousarray(bits, np.uint32)
    return _pair(lib().hor_hash_float, bits, bits.size)


def hash_voxel(xyz):
    """(folded HashEigen over std::hash<int>, header) of int32 [n, 3]"""
    xyz = np.ascontiguousarray(xyz, np.int32)
    return _pair(lib().hor_hash_voxel, xyz, xyz.shape[0])


def hash_point(bits3):
    """(folded PointHash over std::hash<float>, header) of the coordinate bit patterns uint32 [n, 3]"""
    bits3 = np.ascontiguousarray(bits3, np.uint32)
    return _pair(lib().hor_hash_point, bits3, bits3.shape[0])


def rehash_counts(limit):
    """element counts <= limit at which an insertion rehashes a container that was not reserved (from the policy object)"""
    out = np.zeros(128, np.int64)
    c = lib().hor_rehash_counts(C.c_longlong(limit), _p(out), 128)
    assert 0 < c <= 128
    return out[:c].tolist()


def sizes(limit=5088, cross=42043):
    """the element counts of the tests: 0, 1, 2, every scheduled rehash count c <= limit with c - 1 and c + 1, one past `cross`"""
    ns = {0, 1, 2, cross + 700}
    for c in rehash_counts(limit):
        ns.update({max(c - 1, 0), c, c + 1})
    return sorted(ns)


def distinct_keys(n, spread, seed):
    """exactly n distinct voxel keys in a random first-insertion order, coordinates in [0, spread) (n <= spread ** 3)"""
    rng = np.random.default_rng(seed)
    assert n <= spread ** 3
    if spread ** 3 <= 4 * max(n, 1):
        ids = rng.permutation(spread ** 3)[:n]
    else:
        ids = np.unique(rng.integers(0, spread ** 3, 2 * n + 16))
        ids = rng.permutation(ids)[:n]
        assert len(ids) == n
    return np.stack([ids % spread, (ids // spread) % spread, ids // (spread * spread)], axis=1).astype(np.int32)


def map_order(xyz, reserve=0):
    """(hashes, container order, rule order) of the elements of the key sequence xyz (repeats allowed)"""
    xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
    nd = xyz.shape[0]
    h = np.zeros(max(nd, 1), np.uint64); oc = np.zeros(max(nd, 1), np.int32); orr = np.zeros(max(nd, 1), np.int32)
    n = lib().hor_map_order(_p(xyz), nd, C.c_longlong(reserve), _p(h), _p(oc), _p(orr))
    return h[:n], oc[:n], orr[:n]


def set_order(xyz):
    """the same for float32 [n, 3] points through unordered_set after reserve(n)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nd = xyz.shape[0]
    h = np.zeros(max(nd, 1), np.uint64); oc = np.zeros(max(nd, 1), np.int32); orr = np.zeros(max(nd, 1), np.int32)
    n = lib().hor_set_order(_p(xyz), nd, _p(h), _p(oc), _p(orr))
    return h[:n], oc[:n], orr[:n]


def replay(hashes, reserve=0):
    """iteration order of a real container whose element i has hash code hashes[i]"""
    hashes = np.ascontiguousarray(hashes, np.uint64)
    out = np.zeros(max(hashes.size, 1), np.int32)
    lib().hor_replay(_p(hashes), hashes.size, C.c_longlong(reserve), _p(out))
    return out[: hashes.size]


def rule(hashes, reserve=0):
    hashes = np.ascontiguousarray(hashes, np.uint64)
    out = np.zeros(max(hashes.size, 1), np.int32)
    lib().hor_rule(_p(hashes), hashes.size, C.c_longlong(reserve), _p(out))
    return out[: hashes.size]
