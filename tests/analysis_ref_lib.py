"""Loader of tests/cpp/analysis_ref.cpp (the CPU statement of the ground-truth evaluation of an alignment, include/lgr.h
lgr_evaluate_gt*), compiled once per session with g++ -O2 -ffp-contract=off -fopenmp into a temporary directory.  numpy in, numpy out.
The correspondence uniformity comes from the oracle: orc_evaluate over the correct correspondences, each with an infinite threshold, so
that the inlier set of that evaluation is exactly the set (0 for an empty set)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "analysis_ref.cpp")
CORR_DTYPE = np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4"), ("threshold", "<f4")])
_lib = None


class Eval(C.Structure):
    _fields_ = [("r_err", C.c_float), ("t_err", C.c_float), ("pcd_err", C.c_float), ("overlap_rmse", C.c_float), ("overlap_size", C.c_int32),
                ("normal_diff", C.c_float), ("n_normal_overlap", C.c_int32), ("n_overlap_src", C.c_int32), ("n_overlap_tgt", C.c_int32),
                ("n_overlap", C.c_int32), ("overlap", C.c_float), ("overlap_area", C.c_float), ("n_correspondences", C.c_int32),
                ("n_correct_correspondences", C.c_int32), ("n_inliers", C.c_int32), ("n_correct_inliers", C.c_int32), ("converged", C.c_int32),
                ("converged_and_overlap_ok", C.c_int32)]


FLOAT_FIELDS = ("r_err", "t_err", "pcd_err", "overlap_rmse", "normal_diff", "overlap", "overlap_area", "corr_uniformity")
INT_FIELDS = ("overlap_size", "n_normal_overlap", "n_overlap_src", "n_overlap_tgt", "n_overlap", "n_correspondences",
              "n_correct_correspondences", "n_inliers", "n_correct_inliers", "converged", "converged_and_overlap_ok")


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="analysis_ref_"), "libanalysis_ref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", out, SRC])
        _lib = C.CDLL(out)
        for f in (_lib.aref_rot_trans_diff, _lib.aref_diff_matrix, _lib.aref_overlap_rmse, _lib.aref_align, _lib.aref_normal_difference,
                  _lib.aref_merge_overlaps, _lib.aref_correct_correspondences, _lib.aref_evaluate):
            f.restype = None
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


def rot_trans_diff(T1, T2):
    a, t = C.c_float(0), C.c_float(0)
    lib().aref_rot_trans_diff(_p(T16(T1)), _p(T16(T2)), C.byref(a), C.byref(t))
    return np.float32(a.value), np.float32(t.value)


def diff_matrix(T, T_gt):
    D = np.zeros(16, np.float32)
    lib().aref_diff_matrix(_p(T16(T)), _p(T16(T_gt)), _p(D))
    return D.reshape(4, 4).T.copy()


def overlap_rmse(src, tgt, T, T_gt, thr):
    """-> dict(pcd_err, overlap_rmse, overlap_size, term_pcd [ns], term_ov [ns], idx [ns])"""
    src = _f32(src); tgt = _f32(tgt)
    ns = src.shape[0]
    pe, orm, n = C.c_float(0), C.c_float(0), C.c_int(0)
    tp = np.zeros(ns, np.float32); to = np.zeros(ns, np.float32); idx = np.zeros(ns, np.int32)
    lib().aref_overlap_rmse(_p(src), ns, _p(tgt), tgt.shape[0], _p(T16(T)), _p(T16(T_gt)), C.c_float(thr), C.byref(pe), C.byref(orm), C.byref(n),
                            _p(tp), _p(to), _p(idx))
    return dict(pcd_err=np.float32(pe.value), overlap_rmse=np.float32(orm.value), overlap_size=n.value, term_pcd=tp, term_ov=to, idx=idx)


def align(src, T_gt):
    src = _f32(src)
    out = np.zeros_like(src)
    lib().aref_align(_p(src), src.shape[0], _p(T16(T_gt)), _p(out))
    return out


def normal_difference(src, tgt, T_gt, thr):
    """-> (normal_diff, n_normal_overlap, values [ns], -1 where the point does not count)"""
    src = _f32(src); tgt = _f32(tgt)
    nd, n = C.c_float(0), C.c_int(0)
    v = np.zeros(src.shape[0], np.float32)
    lib().aref_normal_difference(_p(src), src.shape[0], _p(tgt), tgt.shape[0], _p(T16(T_gt)), C.c_float(thr), C.byref(nd), C.byref(n), _p(v))
    return np.float32(nd.value), n.value, v


def merge_overlaps(src, tgt, T_gt, thr):
    """-> dict(mask_src, mask_tgt, n_overlap_src, n_overlap_tgt, overlap, overlap_area)"""
    src = _f32(src); tgt = _f32(tgt)
    ms = np.zeros(max(src.shape[0], 1), np.uint8); mt = np.zeros(max(tgt.shape[0], 1), np.uint8)
    n2 = (C.c_int * 2)()
    ov, oa = C.c_float(0), C.c_float(0)
    lib().aref_merge_overlaps(_p(src), src.shape[0], _p(tgt), tgt.shape[0], _p(T16(T_gt)), C.c_float(thr), _p(ms), _p(mt), n2, C.byref(ov), C.byref(oa))
    return dict(mask_src=ms[:src.shape[0]], mask_tgt=mt[:tgt.shape[0]], n_overlap_src=n2[0], n_overlap_tgt=n2[1], overlap=np.float32(ov.value),
                overlap_area=np.float32(oa.value))


def _corr(corr):
    return np.ascontiguousarray(np.asarray(corr).view(CORR_DTYPE).reshape(-1))


def correct_correspondences(src, tgt, corr, T_gt, inlier_mask=None):
    """-> (correct mask [c], n_correct, n_inliers, n_correct_inliers)"""
    src = _f32(src); tgt = _f32(tgt); corr = _corr(corr)
    c = corr.shape[0]
    m = np.zeros(max(c, 1), np.uint8)
    o3 = (C.c_int * 3)()
    im = None if inlier_mask is None else np.ascontiguousarray(inlier_mask, np.uint8)
    lib().aref_correct_correspondences(_p(src), _p(tgt), _p(corr), c, _p(T16(T_gt)), _p(im), _p(m), o3)
    return m[:c], o3[0], o3[1], o3[2]


def uniformity(src, tgt, corr, correct, T_gt):
    """calculateCorrespondenceUniformity over the correct correspondences, through the oracle (orc_evaluate, uniformity metric)"""
    if os.path.join(ROOT, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as o
    o.build()
    cc = _corr(corr)[np.asarray(correct, bool)].copy()
    if cc.shape[0] == 0:
        return np.float32(0.0)
    cc["threshold"] = np.inf
    _, n_inl, _, metric = o.evaluate(_f32(src), _f32(tgt), cc.view(o.CORR_DTYPE), np.asarray(T_gt, np.float32), metric_id=o.METRIC_UNIFORMITY,
                                     score_id=o.SCORE_MSE)
    assert n_inl == cc.shape[0], (n_inl, cc.shape[0])   # every correct correspondence is an inlier of that evaluation
    return np.float32(metric)


def evaluate_gt(src, tgt, corr, T, T_gt, thr, converged=True, inlier_mask=None):
    """-> (dict of every field of lgr_gt_eval, correct mask [c])"""
    src = _f32(src); tgt = _f32(tgt); corr = _corr(corr)
    c = corr.shape[0]
    e = Eval()
    m = np.zeros(max(c, 1), np.uint8)
    im = None if inlier_mask is None else np.ascontiguousarray(inlier_mask, np.uint8)
    lib().aref_evaluate(_p(src), src.shape[0], _p(tgt), tgt.shape[0], _p(corr), c, _p(T16(T)), _p(T16(T_gt)), C.c_float(thr), int(bool(converged)),
                        _p(im), C.byref(e), _p(m))
    out = {name: (np.float32(getattr(e, name)) if name in FLOAT_FIELDS else int(getattr(e, name))) for name, _ in Eval._fields_}
    out["corr_uniformity"] = uniformity(src, tgt, corr, m[:c], T_gt) if src.shape[0] and tgt.shape[0] else np.float32(0.0)
    return out, m[:c]
