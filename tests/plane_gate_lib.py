"""Scenes for the gate of plane_kernel (csrc/lgr_plane.hip) and a CPU statement of which hypotheses it MUST abandon.

The gate abandons a hypothesis part-way through its sparse subset once it can be neither the best nor a record.  It is checked after every
CHECK = GATE_ITERS * PB = 1024 subset points while points are left, so it can fire only from n_sp = 1025 on (102 500 source points).
Which prefix of the subset has been evaluated at a check depends on thread timing, so the device's count of abandoned hypotheses is not
reproducible -- but a prefix holds no more score and no more inliers than the whole subset, and the kernel's bound grows with both.  A
hypothesis whose WHOLE-subset score and count already satisfy the kernel's condition at the check after d points is therefore abandoned
at that check at the latest, whatever the prefix: `certain` counts those, from the oracle alone (oracle.replay for the transforms and
survivors, oracle.evaluate_plane_many with counter = iteration for the whole-subset values).  The device's count must be at least it.

What is restated from the loop (csrc/lgr_ransac_schedule.cuh, lgr_ransac.hip), exactly where the count depends on it:
  * the first round is one batch and runs with the loop's initial state: best metric = the guess's (0 without one), record = 0 under
    closest_plane / weighted_closest_plane (nothing can be abandoned: count + left < 0 never holds) and INT_MAX under combination (the
    metric alone gates, so only a guess makes the first round gate);
  * the second round starts at the end of the first batch and spans min(MAX_ROUND_BATCHES, ceil((min(bound, max_iterations) - done) /
    batch)) batches with the state the first batch left: best metric (strict >, candidates only), record count, bound from the record;
    a third round would run with a tighter state still (best metric and record only grow), so it is simply not counted here;
  * closest_plane scores EVERY survivor of the prerejection on its subset, combination only the candidates (correspondence inliers >=
    MIN_NR_INLIERS); a candidate under closest_plane is a survivor with >= MIN_NR_INLIERS plane inliers.
The kernel's bound with the whole-subset score S in place of the prefix's:
    m_max = (float) ((S + left [* w_gate]) / (0.01 * (double) (float) ns [w_sum])) * fac * 1.00001f,  abandoned when
    m_max < best_prev && count + left < record_prev
S is the exact 2^-32 fixed-point sum on the device; the oracle reports it rounded to float (or, weighted, only the metric it gives), so an
upper bound of it is used: one float step above the reported value (see score_upper) -- a larger S only makes the statement more cautious.
"""
import numpy as np

CHECK = 1024                 # GATE_ITERS * PB
MIN_NR_INLIERS = 10
MAX_ROUND_BATCHES = 16
INT_MAX = 0x7FFFFFFF
SEED = 566
GUESS_COUNTER = 0xFFFFFFFD   # the plane subset of the guess's evaluation; 0xFFFFFFFE / 0xFFFFFFFF: the final block's two
N_MAIN = 250000              # n_sp = 2500: checks after 1024 and 2048 points
LOOP = dict(score_id=2, edge_thr_coef=0.6, max_iterations=4000, ransac_batch=500)
CHUNK_EDGES = {102400: 1024, 102500: 1025, 204800: 2048, 204900: 2049, 409700: 4097}   # source points -> n_sp


def n_sp_of(ns):
    return int(0.01 * float(np.float32(ns)))


def make_scene(n_pts, inlier_frac=0.2):
    """the recipe of every gated case: a correspondence problem on n_pts points with 6000 correspondences, unit normals on both clouds"""
    from lgr_amd import synthetic
    p = synthetic.make_correspondence_problem(n_pts=n_pts, c=6000, inlier_frac=inlier_frac, seed=3)
    rng = np.random.default_rng(77)
    out = dict(T_gt=p["T_gt"].astype(np.float32), corr=p["corr"])
    for side in ("src", "tgt"):                       # (the source's normals are drawn first)
        nrm = rng.normal(size=(n_pts, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pts = np.ascontiguousarray(p[side], np.float32).copy()
        pts[:, 4:7] = nrm.astype(np.float32)
        out[side] = pts
    return out


def to_orc_corr(oracle, corr):
    out = np.zeros(corr.shape[0], oracle.CORR_DTYPE)
    out["query"] = corr["index_query"]; out["match"] = corr["index_match"]
    out["distance"] = corr["distance"]; out["threshold"] = corr["threshold"]
    return out


def params_pair(oracle, capi, metric, **kw):
    """(oracle params, device params) of the loop; kw overrides LOOP (score_id, max_iterations, guess, ...)"""
    args = dict(LOOP, metric_id=metric)
    args.update(kw)
    o = {k: v for k, v in args.items() if k != "ransac_batch"}
    p_o = oracle.default_params(rng_mode=oracle.RNG_PHILOX, batch_size=args["ransac_batch"], **o)
    return p_o, (capi.default_params(**args) if capi is not None else None)


def caller_weights(ns):
    """the caller's map of the weighted case: uniform in [0, 1) with 1 % of the points at 20 -- the gate's bound on one point's score
    (the largest weight) is 40 times the mean weight"""
    w = np.random.default_rng(5).random(ns).astype(np.float32)
    w[np.random.default_rng(6).permutation(ns)[: ns // 100]] = 20.0
    return w


def seq_sum_f32(w):
    """sequential f32 sum in index order (the metric's denominator): a float32 cumulative sum is that chain of adds"""
    return np.float32(np.cumsum(np.ascontiguousarray(w, np.float32), dtype=np.float32)[-1])


# ---------------------------------------------------------------------------------------------------------------- per-iteration values
def hypotheses(oracle, scene, n_iter, edge_thr_coef):
    """iterations [0, n_iter) of the Philox schedule: prerejection flags, transforms (16 floats, column-major), correspondence inlier
    counts and the correspondence metric under the constant score (what `combination` multiplies the plane metric with)"""
    c = scene["corr"].shape[0]
    triples = np.array([oracle.select_n(oracle.philox_draws(SEED, i, 3), c) for i in range(n_iter)], np.int32)
    p = oracle.default_params(rng_mode=oracle.RNG_PHILOX, metric_id=oracle.METRIC_CORRESPONDENCES, score_id=oracle.SCORE_CONSTANT,
                              edge_thr_coef=edge_thr_coef)
    ok, Ts, ninl, met = oracle.replay(scene["src"], scene["tgt"], to_orc_corr(oracle, scene["corr"]), p, triples)
    return dict(ok=ok.astype(bool), Ts=Ts, corr_inl=ninl, corr_metric=met)


def plane_values(oracle, scene, hyp, score_id, weights=None):
    """whole-subset plane values of every survivor (counter = iteration), scattered to iteration order: count, score, metric, and with
    `weights` = (w, w_sum) the weighted metric (weights_ref_lib.plane_metric over the oracle's pairs) in place of the plain one"""
    it = np.flatnonzero(hyp["ok"])
    r = oracle.evaluate_plane_many(scene["src"], scene["tgt"], hyp["Ts"][it], it.astype(np.uint32), score_id=score_id, seed=SEED,
                                   with_pairs=weights is not None)
    n = hyp["ok"].shape[0]
    out = dict(cnt=np.zeros(n, np.int32), score=np.zeros(n, np.float32), metric=np.zeros(n, np.float32), thr=r["thr"])
    out["cnt"][it] = r["n_inl"]; out["score"][it] = r["score"]; out["metric"][it] = r["metric"]
    if weights is not None:
        import weights_ref_lib as W
        w, w_sum = weights
        for k, i in enumerate(it):
            T = hyp["Ts"][i].reshape(4, 4).T
            out["metric"][i] = W.plane_metric(scene["src"], scene["tgt"], T, score_id, r["thr"], r["pairs"][k], w, w_sum)
    return out


def score_upper(pv, ns, weights=None):
    """an upper bound (double) of the exact fixed-point score sum S of every hypothesis.  Plain: the oracle's score is S rounded to
    float, so S <= the next float above it.  Weighted: the metric is fl32(fl32(S) / (0.01 * w_sum)) with the quotient in double, so
    fl32(S) <= next float above the metric x 0.01 x w_sum (x 1 + 1e-12 for the double operations), and S is within 2^-24 of fl32(S)."""
    if weights is None:
        return np.nextafter(pv["score"], np.float32(np.inf)).astype(np.float64)
    m_up = np.nextafter(pv["metric"], np.float32(np.inf)).astype(np.float64)
    return m_up * (0.01 * float(weights[1])) * (1 + 1e-12) * (1 + 2.0 ** -23)


def m_max(S, left, fac, ns, weights=None, w_gate=0.0):
    """the kernel's bound after a check, its float / double sequence"""
    if weights is None:
        m = np.float32((S + float(left)) / (0.01 * float(np.float32(ns))))
    else:
        m = np.float32((S + float(left) * float(np.float32(w_gate))) / (0.01 * float(np.float32(weights[1]))))
    return np.float32(np.float32(m * np.float32(fac)) * np.float32(1.00001))


def certain(oracle, scene, metric, score_id=LOOP["score_id"], guess=None, weights=None, max_iterations=LOOP["max_iterations"],
            batch=LOOP["ransac_batch"], edge_thr_coef=LOOP["edge_thr_coef"], hyp=None):
    """The statement above for one run of the loop.  metric: 2 closest_plane, 3 combination; weights = (w, w_sum): the weighted metric.
    Returns dict(certain, certain_first (already at the first check), evaluated (hypotheses scored on a subset in rounds one and two),
    two_rounds (the loop ends with the second round: `evaluated` is then all of them), rounds = [(first, end, best_prev, record_prev)],
    hyp, pv, candidates (bool per iteration: the loop's candidate rule))."""
    src, tgt = scene["src"], scene["tgt"]
    ns, c = src.shape[0], scene["corr"].shape[0]
    n_sp = n_sp_of(ns)
    ocorr = to_orc_corr(oracle, scene["corr"])
    max_it = min(oracle.comb_or_max(c, 3), max_iterations)
    combination = metric == 3
    if hyp is None:
        hyp = hypotheses(oracle, scene, max_it, edge_thr_coef)
    pv = plane_values(oracle, scene, hyp, score_id, weights)
    w_gate = 0.0 if weights is None else max(float(weights[0].max()), 0.0)
    if combination:
        cand = hyp["ok"] & (hyp["corr_inl"] >= MIN_NR_INLIERS)
        loop_metric = (hyp["corr_metric"] * pv["metric"]).astype(np.float32)     # metric_cs * metric_cp in f32
        record_of, scored, fac = hyp["corr_inl"], cand, hyp["corr_metric"]
    else:
        cand = hyp["ok"] & (pv["cnt"] >= MIN_NR_INLIERS)
        loop_metric = pv["metric"]
        record_of, scored, fac = pv["cnt"], hyp["ok"], np.ones(max_it, np.float32)
    best = np.float32(0)
    if guess is not None:
        g = oracle.evaluate_plane(src, tgt, guess, score_id=score_id, seed=SEED, counter=GUESS_COUNTER, with_pairs=weights is not None)
        best = np.float32(g["metric"])
        if weights is not None:
            import weights_ref_lib as W
            best = np.float32(W.plane_metric(src, tgt, guess, score_id, g["thr"], g["pairs"], weights[0], weights[1]))
        if combination:
            _, _, _, cs = oracle.evaluate(src, tgt, ocorr, guess, oracle.METRIC_CORRESPONDENCES, oracle.SCORE_CONSTANT)
            best = np.float32(np.float32(cs) * best)
    # round one: the first batch under the initial state; then the state it leaves
    nb1 = min(batch, max_it)
    rounds = [(0, nb1, best, INT_MAX if combination else 0)]
    largest, bound, rec = 0, max_it, -1
    for i in np.flatnonzero(cand[:nb1]):
        if rec < 0 or record_of[i] > record_of[rec]:
            rec = i
        if best < loop_metric[i]:
            best = loop_metric[i]
    if rec >= 0 and record_of[rec] > largest:
        largest = int(record_of[rec])
        bound = min(bound, oracle.estimate_max_iterations(src, tgt, ocorr, hyp["Ts"][rec].reshape(4, 4).T, 0.999, 3))
    done = nb1
    two_rounds = True
    if done < bound and done < max_it:
        want = min(bound, max_it) - done
        nb2 = min(min(MAX_ROUND_BATCHES, -(-want // batch)) * batch, max_it - done)
        rounds.append((done, done + nb2, best, INT_MAX if combination else largest))
        two_rounds = done + nb2 >= min(bound, max_it)
    S_up = score_upper(pv, ns, weights)
    n_certain = n_first = evaluated = 0
    for first, end, best_prev, record_prev in rounds:
        idx = first + np.flatnonzero(scored[first:end])
        evaluated += len(idx)
        if not (best_prev > 0 or record_prev < INT_MAX):
            continue
        for i in idx:
            for d in range(CHECK, n_sp, CHECK):                      # checks run only while points are left
                left = n_sp - d
                if m_max(S_up[i], left, fac[i], ns, weights, w_gate) < best_prev and int(pv["cnt"][i]) + left < record_prev:
                    n_certain += 1
                    n_first += d == CHECK
                    break
    return dict(certain=n_certain, certain_first=n_first, evaluated=evaluated, two_rounds=two_rounds, rounds=rounds, hyp=hyp, pv=pv,
                candidates=cand, loop_metric=loop_metric)


# ---------------------------------------------------------------------------------------------------------------- the cases
# Every whole-loop case of tests/test_gpu_plane_gate.py, and the condition tests/test_plane_gate_ref.py holds each to on the CPU: a GATED
# case must have at least MIN_CERTAIN certainly-abandoned hypotheses (n_sp = 2500: at least MIN_CERTAIN_FIRST of them already at the first
# check); an UNGATED one (no check runs, or no record exists yet) must have none, and the device must then report exactly 0.
#   * combination scores only the candidates on a subset (38 of the 746 survivors at inlier_frac 0.2, 11 of them certain): its scenes use
#     inlier_frac 0.4 (271 candidates).
#   * the caller's map (1 % of the weights at 20, the rest below 1): one point may score w_gate = 20, so the bound keeps left * 20 /
#     (0.01 * w_sum) in hand -- above 5 for the 452 points left at the last check of n_sp = 2500, where no metric exceeds ~1.1: nothing can be
#     abandoned there.  That case therefore runs at 204 900 points (n_sp = 2049): the second check has ONE point left.
MIN_CERTAIN, MIN_CERTAIN_FIRST = 20, 5
CASES = {
    "closest_plane":            dict(ns=N_MAIN, frac=0.2, metric=2, score=2),
    "combination":              dict(ns=N_MAIN, frac=0.4, metric=3, score=2),
    "combination_score0":       dict(ns=N_MAIN, frac=0.4, metric=3, score=0),
    "closest_plane_guess":      dict(ns=N_MAIN, frac=0.2, metric=2, score=2, guess=True),
    "combination_guess":        dict(ns=N_MAIN, frac=0.4, metric=3, score=2, guess=True),
    "closest_plane_guess_one_batch": dict(ns=N_MAIN, frac=0.2, metric=2, score=2, guess=True, max_iterations=LOOP["ransac_batch"], gated=False),
    "edge_102400":              dict(ns=102400, frac=0.2, metric=2, score=2, gated=False),
    "edge_102500":              dict(ns=102500, frac=0.2, metric=2, score=2),
    "edge_204800":              dict(ns=204800, frac=0.2, metric=2, score=2),
    "edge_204900":              dict(ns=204900, frac=0.2, metric=2, score=2),
    "edge_409700":              dict(ns=409700, frac=0.2, metric=2, score=2),
    "weighted_uniform":         dict(ns=N_MAIN, frac=0.2, metric=2, score=0, weights="uniform"),
    "weighted_map":             dict(ns=204900, frac=0.2, metric=2, score=0, weights="map"),
}
_scenes = {}


def case_scene(oracle, name):
    """(scene, per-iteration hypotheses) of a case, made once per (size, inlier fraction)"""
    k = CASES[name]
    key = (k["ns"], k["frac"])
    if key not in _scenes:
        if len(_scenes) >= 2:                      # (the cases come grouped by scene: keep two at most)
            _scenes.pop(next(iter(_scenes)))
        sc = make_scene(*key)
        _scenes[key] = (sc, hypotheses(oracle, sc, LOOP["max_iterations"], LOOP["edge_thr_coef"]))
    return _scenes[key]


def case_weights(name, ns):
    kind = CASES[name].get("weights")
    if kind is None:
        return None
    w = np.full(ns, 0.5, np.float32) if kind == "uniform" else caller_weights(ns)
    return w, seq_sum_f32(w)


def case_certain(oracle, name):
    k = CASES[name]
    sc, hyp = case_scene(oracle, name)
    return certain(oracle, sc, k["metric"], score_id=k["score"], guess=sc["T_gt"] if k.get("guess") else None,
                   weights=case_weights(name, k["ns"]), max_iterations=k.get("max_iterations", LOOP["max_iterations"]), hyp=hyp)


def case_params(oracle, capi, name, metric=None):
    """(oracle params, device params) of a case; metric overrides the case's (the weighted cases: 4 on the device)"""
    k = CASES[name]
    sc, _ = case_scene(oracle, name)
    kw = dict(score_id=k["score"], max_iterations=k.get("max_iterations", LOOP["max_iterations"]))
    if k.get("guess"):
        kw["guess"] = sc["T_gt"]
    p_o, _ = params_pair(oracle, None, k["metric"], **kw)
    _, p_g = params_pair(oracle, capi, k["metric"] if metric is None else metric, **kw)
    return p_o, p_g


def check_case_condition(name, cert):
    k = CASES[name]
    if not k.get("gated", True):
        assert cert["certain"] == 0, (name, cert["certain"])
        return
    assert cert["certain"] >= MIN_CERTAIN, (name, cert["certain"])
    if n_sp_of(k["ns"]) == 2500:
        assert cert["certain_first"] >= MIN_CERTAIN_FIRST, (name, cert["certain_first"])


def weighted_reference(oracle, scene, cert, weights, score_id, n_iterations):
    """The result of the loop under weighted_closest_plane, from parts (the oracle has no weighted loop).  In orc_ransac's loop the
    metric decides only final_metric / final_T / best_iter (and what the final block derives from final_T); iterations, num_rejections
    and the bound follow the prerejection and the plane inlier COUNTS, which no weight touches -- those are the closest_plane run's
    (n_iterations = its `iterations`).  Here: the first strict maximum of the weighted metric over the loop's candidates in iteration
    order, then the final block on that hypothesis (evaluation under counter 0xFFFFFFFE, refit over its plane pairs, evaluation of the
    refit under 0xFFFFFFFF)."""
    import weights_ref_lib as W
    src, tgt, c = scene["src"], scene["tgt"], scene["corr"].shape[0]
    w, w_sum = weights
    best, best_it = np.float32(0), -1
    for i in np.flatnonzero(cert["candidates"][:n_iterations]):
        if best < cert["loop_metric"][i]:
            best, best_it = cert["loop_metric"][i], int(i)
    T = cert["hyp"]["Ts"][best_it].reshape(4, 4).T
    e = oracle.evaluate_plane(src, tgt, T, score_id=score_id, seed=SEED, counter=0xFFFFFFFE, with_pairs=True)
    e_metric = W.plane_metric(src, tgt, T, score_id, e["thr"], e["pairs"], w, w_sum)
    converged = (e["n_inl"] > 20 or float(e["n_inl"]) > 0.15 * float(c)) and e_metric > 0   # (MIN_NR_FINAL_INLIERS, MIN_INLIER_RATE)
    pl = np.zeros(len(e["pairs"]), oracle.CORR_DTYPE)
    pl["query"], pl["match"], pl["threshold"] = e["pairs"][:, 0], e["pairs"][:, 1], e["thr"]
    Tn = oracle.refit(src, tgt, pl, np.ones(len(pl), np.uint8))
    e2 = oracle.evaluate_plane(src, tgt, Tn, score_id=score_id, seed=SEED, counter=0xFFFFFFFF, with_pairs=True)
    return dict(best_iteration=best_it, best_metric_before_refit=best, converged=int(converged), matrix=Tn, n_inliers=e2["n_inl"],
                metric=np.float32(W.plane_metric(src, tgt, Tn, score_id, e2["thr"], e2["pairs"], w, w_sum)))


# ---------------------------------------------------------------------------------------------------------------- subset wrap-around
def subset(oracle, ns, counter, seed=SEED):
    """the sparse subset of hypothesis `counter` on ns source points, restated: (raw draws r % ns, the set after linear probing, whether
    a probe stepped from ns - 1 to 0)"""
    draws, taken, wrapped = [], set(), False
    for j in range(n_sp_of(ns)):
        w = oracle.philox_full(seed, [counter, j >> 2, 0x5A17, 0])
        idx = (w[j & 3] >> 1) % ns
        draws.append(idx)
        while idx in taken:
            wrapped |= idx == ns - 1
            idx = (idx + 1) % ns
        taken.add(idx)
    return draws, taken, wrapped


def find_wrap(oracle, ns, seed=SEED, start=0, limit=1 << 20):
    """the first counter >= start whose subset probes across the end of the cloud (how the counters of the wrap-around test were found:
    find_wrap(oracle, 400) -> 157030, find_wrap(oracle, 800) -> 6732)"""
    for counter in range(start, start + limit):
        if subset(oracle, ns, counter, seed)[2]:
            return counter
    return None


def wrap_cloud(ns):
    """a small cloud to evaluate against itself under the identity: every subset point is its own nearest neighbour at distance 0, so
    the pairs list is the whole subset"""
    rng = np.random.default_rng(ns)
    xyz = rng.uniform(-1, 1, (ns, 3))
    nrm = rng.normal(size=(ns, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    from lgr_amd import synthetic
    pts = synthetic.make_points(xyz)
    pts[:, 4:7] = nrm.astype(np.float32)
    return pts
