"""The statement of the hypothesis-set mode under the plane metrics (closest_plane 2, combination 3, weighted_closest_plane 4), composed
from existing pieces only: hypotheses_ref_lib (fold, keep_mask, to_orc_corr), plane_gate_lib (hypotheses, plane_values, params_pair,
caller_weights, seq_sum_f32), weights_ref_lib.plane_metric and the oracle.

  items    the guess (evaluated on the plane subset of counter 0xFFFFFFFD, no inlier gate, iteration -1), then every iteration of the loop
           that survives prerejection with >= 10 inliers.  closest_plane / weighted: plane inliers on the subset of counter = iteration,
           metric = the plane metric.  combination: correspondence inliers, metric = the f32 product of the correspondences metric under
           the constant score and the plane metric.  `iterations` is oracle.ransac's with the same metric -- under the weighted metric the
           closest_plane run's, as plane_gate_lib.weighted_reference argues.
  set      hypotheses_ref_lib.fold over the items in iteration order
  final    per member, as plane_gate_lib.weighted_reference does it: evaluation under counter 0xFFFFFFFE, refit (over the plane pairs in
           ascending source index; combination: over the correspondence inliers), evaluation of the refit under 0xFFFFFFFF
  choice   oracle.choose_best_hypothesis over the refit transforms
"""
import functools

import numpy as np

import hypotheses_ref_lib as H
import plane_gate_lib as P

F = np.float32
C_GUESS, C_FINAL, C_REFIT = 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF


def with_normals(prob):
    """unit normals on both clouds, drawn as plane_gate_lib.make_scene draws them (default_rng(77), the source first)"""
    rng = np.random.default_rng(77)
    out = dict(prob)
    for side in ("src", "tgt"):
        pts = np.ascontiguousarray(prob[side], F).copy()
        nrm = rng.normal(size=(pts.shape[0], 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pts[:, 4:7] = nrm.astype(F)
        out[side] = pts
    return out


@functools.lru_cache(maxsize=None)
def scene_a(n_pts, f1, f2, seed=11):
    from lgr_amd import synthetic
    return with_normals(synthetic.make_two_mode_problem(n_pts=n_pts, c=1500, f1=f1, f2=f2, seed=seed))


@functools.lru_cache(maxsize=None)
def scene_b():
    return P.make_scene(8000, 0.4)


# scene A: metric_id, f1, f2, max_iterations, batch (hypotheses_ref_lib.row_params reads a row like its own TWO_MODE_ROWS)
ROWS_A = [
    (2, 0.30, 0.18, 6000, 1000),
    (2, 0.50, 0.20, 8000, 256),
    (3, 0.30, 0.18, 6000, 1000),
    (3, 0.50, 0.20, 8000, 256),
]


def _T16(T):
    return np.ascontiguousarray(np.asarray(T, F).T.reshape(16))


def _plane_metric(scene, T, score_id, e, weights):
    """the plane metric of one evaluation e (oracle.evaluate_plane's dict, with pairs when weighted)"""
    if weights is None:
        return F(e["metric"])
    import weights_ref_lib as W
    return F(W.plane_metric(scene["src"], scene["tgt"], T, score_id, e["thr"], e["pairs"], weights[0], weights[1]))


def _eval_many(oracle, scene, Ts, counter, score_id, weights, ocorr, combination):
    """the evaluation of every 4x4 transform in Ts under a plane metric with one counter -> list of dict(metric, n_inl, pairs, mask)"""
    src, tgt = scene["src"], scene["tgt"]
    if not len(Ts):
        return []
    r = oracle.evaluate_plane_many(src, tgt, np.stack([_T16(T) for T in Ts]), np.full(len(Ts), counter, np.uint32), score_id=score_id,
                                   seed=P.SEED, with_pairs=True)
    out = []
    for k, T in enumerate(Ts):
        e = dict(n_inl=int(r["n_inl"][k]), metric=r["metric"][k], thr=r["thr"], pairs=r["pairs"][k])
        cp = _plane_metric(scene, T, score_id, e, weights)
        if combination:
            mask, ninl, _, cs = oracle.evaluate(src, tgt, ocorr, T, oracle.METRIC_CORRESPONDENCES, oracle.SCORE_CONSTANT)
            out.append(dict(metric=F(F(cs) * cp), n_inl=int(ninl), mask=mask, pairs=None))
        else:
            out.append(dict(metric=cp, n_inl=e["n_inl"], mask=None, pairs=e["pairs"], thr=e["thr"]))
    return out


def items(oracle, scene, p_o, weights=None):
    """-> (oracle.ransac's result, item iterations, item transforms [n, 16], item metrics).  p_o.metric_id is 2 or 3; `weights` = (w, w_sum)
    turns 2 into the weighted metric (the loop's counts, hence `iterations`, are closest_plane's)."""
    src, tgt = scene["src"], scene["tgt"]
    ocorr = H.to_orc_corr(oracle, scene["corr"])
    combination = p_o.metric_id == 3
    assert p_o.metric_id in (2, 3) and p_o.n_samples == 3 and not (combination and weights is not None)
    ores, _ = oracle.ransac(src, tgt, ocorr, p_o)
    its, Ts, ms = [], [], []
    if p_o.has_guess:
        G = np.array(p_o.guess, F).reshape(4, 4).T
        g = _eval_many(oracle, scene, [G], C_GUESS, p_o.score_id, weights, ocorr, combination)[0]
        its.append(-1); Ts.append(np.array(p_o.guess, F)); ms.append(g["metric"])
    n = ores.iterations
    if n:
        hyp = P.hypotheses(oracle, scene, n, p_o.edge_thr_coef)
        pv = P.plane_values(oracle, scene, hyp, p_o.score_id, weights)
        if combination:
            cand = hyp["ok"] & (hyp["corr_inl"] >= H.MIN_NR_INLIERS)
            met = (hyp["corr_metric"] * pv["metric"]).astype(F)      # metric_cs * metric_cp in f32
        else:
            cand = hyp["ok"] & (pv["cnt"] >= H.MIN_NR_INLIERS)
            met = pv["metric"]
        for i in np.flatnonzero(cand):
            its.append(int(i)); Ts.append(hyp["Ts"][i]); ms.append(met[i])
    return ores, np.array(its, np.int32), np.array(Ts, F).reshape(-1, 16), np.array(ms, F)


def m_star_of(ms):
    """the loop's final best metric: the first strict maximum of the item metrics from 0 (a guess included)"""
    best = F(0)
    for m in ms:
        if best < m:
            best = m
    return best


def final_blocks(oracle, scene, p_o, loop_Ts, weights=None):
    """:270-291 on every 4x4 transform of loop_Ts -> list of dict(T, metric, n_inliers, converged)"""
    src, tgt = scene["src"], scene["tgt"]
    ocorr = H.to_orc_corr(oracle, scene["corr"])
    c = len(ocorr)
    combination = p_o.metric_id == 3
    ev = _eval_many(oracle, scene, loop_Ts, C_FINAL, p_o.score_id, weights, ocorr, combination)
    Tns = []
    for e in ev:
        if e["n_inl"] == 0:
            Tns.append(np.full((4, 4), np.nan, F))
        elif combination:
            Tns.append(oracle.refit(src, tgt, ocorr, e["mask"]))
        else:
            pl = np.zeros(len(e["pairs"]), oracle.CORR_DTYPE)
            pl["query"], pl["match"], pl["threshold"] = e["pairs"][:, 0], e["pairs"][:, 1], e["thr"]
            Tns.append(oracle.refit(src, tgt, pl, np.ones(len(pl), np.uint8)))
    ev2 = _eval_many(oracle, scene, Tns, C_REFIT, p_o.score_id, weights, ocorr, combination)
    out = []
    for e, Tn, e2 in zip(ev, Tns, ev2):
        enough = e["n_inl"] > H.MIN_NR_FINAL_INLIERS or float(e["n_inl"]) > H.MIN_INLIER_RATE * float(c)
        out.append(dict(T=Tn, metric=F(e2["metric"]), n_inliers=int(e2["n_inl"]), converged=int(bool(enough and F(e["metric"]) > F(0)))))
    return out


def statement(oracle, scene, p_o, weights=None, cap=H.CAP, filtered=False, members="all"):
    """the set, final block and choice; None in place of the set when it outgrows cap.  members = "all", or "set": the set alone (the final
    blocks of chosen members: final_blocks)"""
    src, tgt = scene["src"], scene["tgt"]
    ocorr = H.to_orc_corr(oracle, scene["corr"])
    ores, its, Ts, ms = items(oracle, scene, p_o, weights)
    m_star = m_star_of(ms)
    if weights is None:
        assert H.bits(m_star) == H.bits(ores.best_metric_before_refit), (m_star, ores.best_metric_before_refit)
    kept = H.keep_mask(ms, m_star)
    s = H.fold(oracle, Ts, ms, p_o.distance_thr, cap, kept if filtered else None)
    out = dict(ores=ores, n_items=len(ms), n_items_kept=int(kept.sum()), set=s, item_iterations=its, m_star=m_star)
    if s is None:
        return out
    loop_Ts = [s["T"][k].reshape(4, 4).T.copy() for k in range(len(s["metric"]))]
    out["loop"] = [dict(loop_T=Tl, iteration=int(its[s["index"][k]]), loop_metric=F(s["metric"][k])) for k, Tl in enumerate(loop_Ts)]
    if members == "set":
        return out
    fb = final_blocks(oracle, scene, p_o, loop_Ts, weights)
    mem = [dict(l, **f) for l, f in zip(out["loop"], fb)]
    bi, Tb, uni = oracle.choose_best_hypothesis(src, tgt, ocorr, [m["T"] for m in mem])
    for m, u in zip(mem, uni):
        m["uniformity"] = F(u)
    out.update(members=mem, best_index=int(bi), T=Tb, converged=int(any(m["converged"] for m in mem)))
    return out


# ---- the inputs' parameters and shared statements
def row_params(oracle, capi, row, **extra):
    return H.row_params(oracle, capi, row, **extra)


def scene_b_params(oracle, capi, metric, **kw):
    return P.params_pair(oracle, capi, metric, **kw)


_STATEMENTS = {}


def row_statement(oracle, row, n_pts=4000, guess=None, filtered=False):
    """scene A, computed once per (row, size, guess, filtered) and shared; callers must not change it"""
    key = ("A", row, n_pts, None if guess is None else H.bits(guess).tobytes(), filtered)
    if key not in _STATEMENTS:
        p_o, _ = row_params(oracle, None, row, **({} if guess is None else {"guess": guess}))
        _STATEMENTS[key] = statement(oracle, scene_a(n_pts, row[1], row[2]), p_o, filtered=filtered)
    return _STATEMENTS[key]


def scene_b_statement(oracle, metric, filtered=False):
    key = ("B", metric, filtered)
    if key not in _STATEMENTS:
        p_o, _ = scene_b_params(oracle, None, metric)
        _STATEMENTS[key] = statement(oracle, scene_b(), p_o, filtered=filtered)
    return _STATEMENTS[key]


def weighted_row_statement(oracle, row, n_pts=4000, seed=11):
    """scene A under weighted_closest_plane with plane_gate_lib.caller_weights as the caller's map (row: a metric-2 row)"""
    key = ("W", row, n_pts, seed)
    if key not in _STATEMENTS:
        sc = scene_a(n_pts, row[1], row[2], seed)
        w = P.caller_weights(sc["src"].shape[0])
        p_o, _ = row_params(oracle, None, row)
        _STATEMENTS[key] = statement(oracle, sc, p_o, weights=(w, P.seq_sum_f32(w)))
    return _STATEMENTS[key]


def has_both_modes(oracle, members, prob):
    """each planted pose has a member similar to it in updateHypotheses' own sense (no tolerance of ours)"""
    t_thr = F(20 * F(H.DISTANCE_THR))
    return all(any(r < np.pi / 9 and t < t_thr for r, t in (oracle.rot_trans_diff(m["T"], Tp.astype(F)) for m in members))
               for Tp in (prob["T1"], prob["T2"]))
