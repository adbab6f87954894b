"""The CPU statement of the iterated closest-plane refinement (include/lgr.h lgr_refine_plane*), composed from
plane_dense_ref_lib.evaluate (the dense closest-plane evaluation) and the oracle's refit (estimateOptimalRigidTransformation) taken over the
inlier pairs as correspondences with an all-ones mask.  No arithmetic of its own: the loop, one float compare and the stop reasons."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_dense_ref_lib as P  # noqa: E402

STOP_MAX_STEPS, STOP_NO_GAIN, STOP_NO_PAIRS = 0, 1, 2
GROUP = 4   # LGR_REFINE_GROUP
F = np.float32


def _step(T, e):
    return dict(T=np.asarray(T, F).copy(), metric=e["metric"], rmse=e["rmse"], score=e["score"], n_inliers=int(e["n_inliers"]))


def refine(oracle, src, tgt, T0, score_id, thr, max_steps, weights=None):
    """-> dict(T, metric, rmse, score, n_inliers: the last accepted step's; threshold, steps, stop; first, rejected (None when there is
    none); trace: every evaluated transform in order -- T0, each candidate, the rejected one last).  thr must be > 0 (the entry points
    compute the target's density once when asked to; the statement takes the value)."""
    src = np.ascontiguousarray(src, F); tgt = np.ascontiguousarray(tgt, F)
    ev = lambda T: P.evaluate(src, tgt, T, score_id, thr, weights)   # noqa: E731
    T = np.asarray(T0, F).copy()
    if len(src) == 0:
        e = dict(metric=F(0), rmse=np.finfo(F).max, score=F(0), n_inliers=0)
        first = _step(T, e)
        return dict(first, threshold=F(thr), steps=0, stop=STOP_NO_PAIRS, first=first, rejected=None, trace=[first])
    E = ev(T)
    first = _step(T, E)
    trace, rejected, steps, stop = [first], None, 0, STOP_MAX_STEPS
    while steps < max_steps:
        if E["n_inliers"] < 3:
            stop = STOP_NO_PAIRS
            break
        inl = np.ascontiguousarray(E["inliers"])   # {source i, nearest target of i, dist, thr} in ascending i
        Tn = oracle.refit(src, tgt, inl, np.ones(len(inl), np.uint8)).astype(F)
        En = ev(Tn)
        trace.append(_step(Tn, En))
        if not (F(En["metric"]) > F(E["metric"])):   # a NaN or zero metric never wins
            stop, rejected = STOP_NO_GAIN, trace[-1]
            break
        T, E, steps = Tn, En, steps + 1
    return dict(_step(T, E), threshold=F(thr), steps=steps, stop=stop, first=first, rejected=rejected, trace=trace)


def perturbed(T_gt, thr):
    """the perturbation of tests/test_gpu_plane_dense.py: 0.5 degrees about z and 0.3 thr along (0.6, 0, 0.8), applied after the ground truth"""
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    return (dT @ T_gt).astype(F)


def errors(T, T_gt):
    """(rotation error in degrees, translation error) of T against T_gt, in float64"""
    D = np.linalg.inv(np.asarray(T_gt, np.float64)) @ np.asarray(T, np.float64)
    c = np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)
    return float(np.rad2deg(np.arccos(c))), float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - np.asarray(T_gt, np.float64)[:3, 3]))


_pair = {}


def make_pair(oracle, n=4000, seed=12):
    """make_pair(n, seed) with the oracle's normals (k = 30, towards the viewpoints), thr = the oracle's density of the target, T0 the
    perturbed ground truth, T_far a random pose; built once per session and shared (nobody writes into it)"""
    if (n, seed) not in _pair:
        from lgr_amd import synthetic
        p = synthetic.make_pair(n_points=n, seed=seed)
        out = dict(T_gt=p["T_gt"].astype(F))
        for side in ("src", "tgt"):
            out[side] = np.ascontiguousarray(oracle.normals_knn(p[side], 30, vp=p["vp_" + side]), F)
        thr = float(F(oracle.cloud_density(out["tgt"])))
        out.update(thr=thr, T0=perturbed(p["T_gt"], thr), T_far=synthetic.random_se3(np.random.default_rng(5)).astype(F))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _pair[(n, seed)] = out
    return _pair[(n, seed)]


_runs = {}


def reference(oracle, key, *args, **kw):
    """refine(oracle, *args, **kw) computed once per key and shared among the tests"""
    if key not in _runs:
        _runs[key] = refine(oracle, *args, **kw)
    return _runs[key]
