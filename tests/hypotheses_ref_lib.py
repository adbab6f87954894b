"""The statement of the hypothesis-set mode (SampleConsensusPrerejectiveOMP::align with SAVE_MULTIPLE_HYPOTHESES,
src/sac_prerejective_omp.cpp:11), composed from existing oracle calls only:

  items    the guess (oracle.evaluate's metric, no inlier gate), then every iteration of oracle.ransac's loop whose sample tuple
           (philox_draws / select_n) survives prerejection with >= 10 inliers, with oracle.replay's transform and metric
  set      the left fold of orc_update_hypotheses over the items, one stream in iteration order
  final    per member: oracle.evaluate -> converged, oracle.refit, oracle.evaluate of the refit
  choice   oracle.choose_best_hypothesis over the refit transforms

The fold carries each item's position with it: orc_update_hypotheses copies all 16 floats of a transform and reads only R|t, so the
position travels in the fourth row (element 3) and is taken out again afterwards.
"""
import ctypes as C
import functools

import numpy as np

F = np.float32
MIN_NR_INLIERS, MIN_NR_FINAL_INLIERS, MIN_INLIER_RATE = 10, 20, 0.15
CAP = 2048


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def to_orc_corr(oracle, corr):
    out = np.zeros(corr.shape[0], oracle.CORR_DTYPE)
    out["query"] = corr["index_query"]; out["match"] = corr["index_match"]
    out["distance"] = corr["distance"]; out["threshold"] = corr["threshold"]
    return out


def fold(oracle, tns16, metrics, distance_thr, cap=CAP, keep=None):
    """orc_update_hypotheses folded over the items (keep: a boolean mask of the items that take part).
    -> dict(T [m, 16], metric [m], index [m], peak, changes) or None when the set outgrows cap."""
    tns16 = np.ascontiguousarray(tns16, F).reshape(-1, 16)
    metrics = np.ascontiguousarray(metrics, F)
    lib = oracle.lib()
    buf = np.zeros((cap, 16), F)
    mb = np.zeros(cap, F)
    n = peak = changes = 0
    for i in range(len(metrics)):
        if keep is not None and not keep[i]:
            continue
        t = tns16[i].copy()
        assert i + 1 < 2 ** 24
        t[3] = F(i + 1)
        before = (n, buf[:n, 3].copy())
        m = lib.orc_update_hypotheses(buf.ctypes.data_as(C.c_void_p), mb.ctypes.data_as(C.c_void_p), n, cap, t.ctypes.data_as(C.c_void_p),
                                      C.c_float(float(metrics[i])), C.c_float(float(distance_thr)))
        if m < 0:
            return None
        n = m
        peak = max(peak, n)
        if before[0] != n or not np.array_equal(before[1], buf[:n, 3]):
            changes += 1
    index = buf[:n, 3].astype(np.int64) - 1
    T = tns16[index].copy() if n else np.zeros((0, 16), F)
    assert np.array_equal(bits(np.delete(T, 3, axis=1)), bits(np.delete(buf[:n], 3, axis=1)))
    return dict(T=T, metric=mb[:n].copy(), index=index.astype(np.int32), peak=peak, changes=changes)


def keep_mask(metrics, m_star):
    """!(m < 0.1 * M*) in double, as updateHypotheses compares"""
    return np.array([not (float(m) < 0.1 * float(m_star)) for m in np.asarray(metrics, F)], bool)


def items_of_loop(oracle, prob, p_o):
    """-> (oracle.ransac's result, item iterations, item transforms [n, 16], item metrics)"""
    src, tgt = prob["src"], prob["tgt"]
    ocorr = to_orc_corr(oracle, prob["corr"])
    c = len(ocorr)
    ores, _ = oracle.ransac(src, tgt, ocorr, p_o)
    its, Ts, ms = [], [], []
    if p_o.has_guess:
        G = np.array(p_o.guess, F).reshape(4, 4).T
        _, _, _, gm = oracle.evaluate(src, tgt, ocorr, G, p_o.metric_id, p_o.score_id)
        its.append(-1); Ts.append(np.array(p_o.guess, F)); ms.append(F(gm))
    n = ores.iterations
    if n:
        tuples = np.array([oracle.select_n(oracle.philox_draws(p_o.seed, i, p_o.n_samples), c) for i in range(n)], np.int32)
        ok, T, ninl, met = oracle.replay(src, tgt, ocorr, p_o, tuples)
        for i in np.nonzero((ok != 0) & (ninl >= MIN_NR_INLIERS))[0]:
            its.append(int(i)); Ts.append(T[i]); ms.append(met[i])
    return ores, np.array(its, np.int32), np.array(Ts, F).reshape(-1, 16), np.array(ms, F)


def statement(oracle, prob, p_o, cap=CAP, filtered=False):
    """the set, final block and choice; None in place of the set when it outgrows cap"""
    src, tgt = prob["src"], prob["tgt"]
    ocorr = to_orc_corr(oracle, prob["corr"])
    c = len(ocorr)
    ores, its, Ts, ms = items_of_loop(oracle, prob, p_o)
    keep = keep_mask(ms, ores.best_metric_before_refit) if filtered else None
    s = fold(oracle, Ts, ms, p_o.distance_thr, cap, keep)
    out = dict(ores=ores, n_items=len(ms), n_items_kept=int(keep_mask(ms, ores.best_metric_before_refit).sum()), set=s, item_iterations=its)
    if s is None:
        return out
    min_tol = F(0.3) if p_o.metric_id == oracle.METRIC_UNIFORMITY else F(0.0)
    members = []
    for k in range(len(s["metric"])):
        Tl = s["T"][k].reshape(4, 4).T
        mask, ninl, _, met = oracle.evaluate(src, tgt, ocorr, Tl, p_o.metric_id, p_o.score_id)
        enough = ninl > MIN_NR_FINAL_INLIERS or float(ninl) > MIN_INLIER_RATE * float(c)
        Tn = oracle.refit(src, tgt, ocorr, mask) if ninl > 0 else np.full((4, 4), np.nan, F)
        _, ninl2, _, met2 = oracle.evaluate(src, tgt, ocorr, Tn, p_o.metric_id, p_o.score_id)
        members.append(dict(loop_T=Tl.copy(), T=Tn, iteration=int(its[s["index"][k]]), loop_metric=F(s["metric"][k]), metric=F(met2),
                            n_inliers=int(ninl2), converged=int(bool(enough and F(met) > min_tol))))
    bi, Tb, uni = oracle.choose_best_hypothesis(src, tgt, ocorr, [m["T"] for m in members])
    for m, u in zip(members, uni):
        m["uniformity"] = F(u)
    out.update(members=members, best_index=int(bi), T=Tb, converged=int(any(m["converged"] for m in members)))
    return out


# ---- the inputs (lgr_amd.synthetic holds the generators)
TWO_MODE_ROWS = [   # metric_id, f1, f2, max_iterations, batch
    (1, 0.30, 0.18, 6000, 1000),
    (1, 0.50, 0.20, 8000, 256),
    (0, 0.30, 0.18, 6000, 1000),
    (0, 0.50, 0.20, 8000, 256),
    # batch 64: a second-pass round is 16 * 64 = 1024 iterations, so the 3584 iterations of the loop take three full rounds and one of 512
    (1, 0.50, 0.20, 8000, 64),
    (0, 0.50, 0.20, 8000, 64),
]
POSE_LISTS = [(3000, 12, 1), (3000, 40, 2), (500, 3, 3)]   # n, K, seed
DISTANCE_THR = 0.05


@functools.lru_cache(maxsize=None)
def two_mode(f1, f2):
    from lgr_amd import synthetic
    return synthetic.make_two_mode_problem(n_pts=4000, c=1500, f1=f1, f2=f2, seed=11)


@functools.lru_cache(maxsize=None)
def pose_list(n, k, seed):
    from lgr_amd import synthetic
    return synthetic.make_pose_list(n, k, seed)


def params_pair(oracle, capi, **kw):
    p_o = oracle.default_params(rng_mode=oracle.RNG_PHILOX, **{k: v for k, v in kw.items() if k != "ransac_batch"})
    if "ransac_batch" in kw:
        p_o.batch_size = kw["ransac_batch"]
    return p_o, (capi.default_params(**kw) if capi is not None else None)


def row_params(oracle, capi, row, **extra):
    metric, _, _, iters, batch = row
    return params_pair(oracle, capi, metric_id=metric, score_id=2, distance_thr=DISTANCE_THR, max_iterations=iters, ransac_batch=batch, **extra)


_STATEMENTS = {}


def row_statement(oracle, row, guess=None, filtered=False):
    """computed once per (row, guess, filtered) and shared; callers must not change it"""
    key = (row, None if guess is None else bits(guess).tobytes(), filtered)
    if key not in _STATEMENTS:
        p_o, _ = row_params(oracle, None, row, **({} if guess is None else {"guess": guess}))
        _STATEMENTS[key] = statement(oracle, two_mode(row[1], row[2]), p_o, filtered=filtered)
    return _STATEMENTS[key]
