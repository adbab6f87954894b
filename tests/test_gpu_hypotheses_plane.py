"""GPU parity of the hypothesis-set mode under the plane metrics (lgr_ransac_multi_ex_dev / lgr_ransac_multi_ex) against the statement
composed from the oracle (tests/hypotheses_plane_ref_lib.py).  Bars: bit-exact -- set members, their order, metrics, iterations, every
field of every member after the final block, the choice, and the loop's fields against lgr_ransac_ex_dev on the same input."""
import ctypes as C

import numpy as np
import pytest

import hypotheses_plane_ref_lib as HP
import hypotheses_ref_lib as H
import plane_gate_lib as P

pytestmark = pytest.mark.gpu
bits = H.bits


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_members(hyps, want):
    assert len(hyps) == len(want["members"])
    for h, w in zip(hyps, want["members"]):
        assert h.iteration == w["iteration"]
        np.testing.assert_array_equal(bits(h.loop_matrix()), bits(w["loop_T"]))
        np.testing.assert_array_equal(bits(h.matrix()), bits(w["T"]))
        assert bits(h.loop_metric) == bits(w["loop_metric"]) and bits(h.metric) == bits(w["metric"])
        assert h.n_inliers == w["n_inliers"] and h.converged == w["converged"]
        assert bits(h.uniformity) == bits(w["uniformity"])


def check_choice(res, bi, want):
    assert bi == want["best_index"] and res.converged == want["converged"]
    np.testing.assert_array_equal(bits(res.matrix()), bits(want["T"]))
    if bi >= 0:
        w = want["members"][bi]
        assert res.n_inliers == w["n_inliers"] and bits(res.metric) == bits(w["metric"])
    else:
        assert res.n_inliers == 0 and res.metric == 0.0


def check_loop_fields(res, single):
    for f in ("iterations", "num_rejections", "estimated_iters", "best_iteration", "n_correspondences"):
        assert getattr(res, f) == getattr(single, f), f
    assert bits(res.best_metric_before_refit) == bits(single.best_metric_before_refit)


def raw(res, hyps, bi):
    skip = type(res).time_cs.offset   # the timings behind it differ from call to call
    return bytes(C.string_at(C.addressof(res), skip)) + b"".join(bytes(C.string_at(C.addressof(h), C.sizeof(h))) for h in hyps) + bytes([bi & 0xff])


def run_a(lgr, row, n_pts=4000, max_set=64, mparams=None, metric=None, seed=11, **extra):
    from lgr_amd import capi
    import oracle
    prob = HP.scene_a(n_pts, row[1], row[2], seed)
    _, p_g = HP.row_params(oracle, capi, row if metric is None else (metric,) + tuple(row[1:]), **extra)
    src, tgt = cuda(prob["src"]), cuda(prob["tgt"])
    return lgr.ransac_multi_ex(src, tgt, prob["corr"], p_g, max_set, mparams), (src, tgt, prob, p_g)


def check_whole(lgr, oracle, got, ctx, want, mparams=None):
    (res, hyps, bi), (src, tgt, prob, p_g) = got, ctx
    check_members(hyps, want)
    check_choice(res, bi, want)
    single, _ = lgr.ransac_ex(src, tgt, prob["corr"], p_g, mparams)
    check_loop_fields(res, single)
    assert res.iterations == want["ores"].iterations


# ---- 1. scene A at 4000 points: n_sp = 40, less than one wave
@pytest.mark.parametrize("row", HP.ROWS_A)
def test_scene_a_4000(lgr, oracle, row):
    want = HP.row_statement(oracle, row)
    got, ctx = run_a(lgr, row)
    check_whole(lgr, oracle, got, ctx, want)
    assert len(got[1]) >= 2
    assert HP.has_both_modes(oracle, [dict(T=h.matrix()) for h in got[1]], ctx[2])


# ---- 2. scene A at 30000 points: n_sp = 300, more than one 256-thread pass over the subset and a pair ordering of several waves
@pytest.mark.parametrize("row", [HP.ROWS_A[0], HP.ROWS_A[2]])
def test_scene_a_30000(lgr, oracle, row):
    want = HP.row_statement(oracle, row, 30000)
    got, ctx = run_a(lgr, row, 30000)
    check_whole(lgr, oracle, got, ctx, want)
    assert len(got[1]) >= 2


# ---- 3. scene B: the volumetric set of closest_plane, the single member of combination
def run_b(lgr, metric, max_set):
    from lgr_amd import capi
    import oracle
    sc = HP.scene_b()
    _, p_g = HP.scene_b_params(oracle, capi, metric)
    src, tgt = cuda(sc["src"]), cuda(sc["tgt"])
    return lgr.ransac_multi_ex(src, tgt, sc["corr"], p_g, max_set), (src, tgt, sc, p_g)


def test_scene_b_closest_plane_set_of_hundreds(lgr, oracle):
    want = HP.scene_b_statement(oracle, 2)
    (res, hyps, bi), (src, tgt, sc, p_g) = run_b(lgr, 2, 1024)
    assert len(hyps) == len(want["members"]) > 64
    for h, w in zip(hyps, want["members"]):       # the set: all members
        assert h.iteration == w["iteration"] and bits(h.loop_metric) == bits(w["loop_metric"])
        np.testing.assert_array_equal(bits(h.loop_matrix()), bits(w["loop_T"]))
    k_best = int(np.argmax([w["loop_metric"] for w in want["members"]]))
    picks = sorted({0, len(hyps) - 1, k_best, want["best_index"]} - {-1})
    check_members([hyps[k] for k in picks], dict(members=[want["members"][k] for k in picks]))   # the final block
    check_choice(res, bi, want)
    single, _ = lgr.ransac_ex(src, tgt, sc["corr"], p_g)
    check_loop_fields(res, single)


def test_scene_b_combination_is_the_single_result(lgr, oracle):
    want = HP.scene_b_statement(oracle, 3)
    (res, hyps, bi), (src, tgt, sc, p_g) = run_b(lgr, 3, 64)
    check_members(hyps, want)
    check_choice(res, bi, want)
    assert len(hyps) == 1
    single, _ = lgr.ransac_ex(src, tgt, sc["corr"], p_g)
    check_loop_fields(res, single)
    h = hyps[0]
    np.testing.assert_array_equal(bits(h.matrix()), bits(single.matrix()))
    assert bits(h.metric) == bits(single.metric) and h.n_inliers == single.n_inliers and h.converged == single.converged


# ---- 4. weighted_closest_plane with the caller's weights
def test_weighted_with_caller_weights(lgr, oracle):
    from lgr_amd import capi
    row = HP.ROWS_A[0]
    want = HP.weighted_row_statement(oracle, row)
    assert len(want["members"]) >= 2 and want["set"]["peak"] <= 64     # conditions on the scene (change its seed, not these)
    w = cuda(P.caller_weights(4000))
    mp = capi.metric_params(weights=w)
    got, ctx = run_a(lgr, row, metric=4, mparams=mp)
    check_whole(lgr, oracle, got, ctx, want, mp)


# ---- 5. the guess is the first item
@pytest.mark.parametrize("row", [HP.ROWS_A[0], HP.ROWS_A[2]])
def test_guess_is_the_first_item(lgr, oracle, row):
    G = HP.scene_a(4000, row[1], row[2])["T2"].astype(np.float32)
    want = HP.row_statement(oracle, row, guess=G)
    assert want["item_iterations"][0] == -1
    got, ctx = run_a(lgr, row, guess=G)
    check_whole(lgr, oracle, got, ctx, want)


# ---- 6. refusals and edges
def test_max_set_below_the_peak_is_refused(lgr, oracle):
    from lgr_amd import capi
    assert HP.row_statement(oracle, HP.ROWS_A[0])["set"]["peak"] > 8
    with pytest.raises(capi.LgrError, match=f"rc={capi.ERR_UNSUPPORTED}"):
        run_a(lgr, HP.ROWS_A[0], max_set=8)


def test_harris_weights_are_refused(lgr):
    from lgr_amd import capi
    with pytest.raises(capi.LgrError, match=f"rc={capi.ERR_UNSUPPORTED}"):
        run_a(lgr, HP.ROWS_A[0], metric=4, mparams=capi.metric_params(weight="harris"))


def test_gror_is_refused(lgr):
    from lgr_amd import capi
    prob = HP.scene_a(4000, 0.30, 0.18)
    p = capi.default_params(metric_id=2, score_id=2, distance_thr=H.DISTANCE_THR, max_iterations=1000, ransac_batch=1000, alignment_id=1)
    with pytest.raises(capi.LgrError, match=f"rc={capi.ERR_UNSUPPORTED}"):
        lgr.ransac_multi_ex(cuda(prob["src"]), cuda(prob["tgt"]), prob["corr"], p, 64)


@pytest.mark.parametrize("metric", [2, 3])
def test_two_correspondences_give_an_empty_set(lgr, metric):
    from lgr_amd import capi
    prob = HP.scene_a(4000, 0.30, 0.18)
    p = capi.default_params(metric_id=metric, score_id=2, distance_thr=H.DISTANCE_THR, max_iterations=1000, ransac_batch=1000)
    res, hyps, bi = lgr.ransac_multi_ex(cuda(prob["src"]), cuda(prob["tgt"]), prob["corr"][:2], p, 64)
    assert hyps == [] and bi == -1 and res.iterations == 0 and res.converged == 0
    np.testing.assert_array_equal(res.matrix(), np.eye(4, dtype=np.float32))


def test_uniformity_returns_the_bytes_of_ransac_multi(lgr, oracle):
    from lgr_amd import capi
    row = H.TWO_MODE_ROWS[0]
    prob = H.two_mode(row[1], row[2])
    _, p_g = H.row_params(oracle, capi, row)
    src, tgt = cuda(prob["src"]), cuda(prob["tgt"])
    a = lgr.ransac_multi(src, tgt, prob["corr"], p_g, 64)
    b = lgr.ransac_multi_ex(src, tgt, prob["corr"], p_g, 64)
    assert raw(*a) == raw(*b) and len(a[1]) >= 2


# ---- 7. repeatability, entry points
@pytest.mark.parametrize("row", [HP.ROWS_A[1], HP.ROWS_A[3]])
def test_two_calls_and_the_host_entry_give_identical_bytes(lgr, oracle, row):
    from lgr_amd import capi
    a, (_, _, prob, p_g) = run_a(lgr, row)
    b, _ = run_a(lgr, row)
    assert raw(*a) == raw(*b) and len(a[1]) >= 2
    h = lgr.ransac_multi_ex_host(prob["src"], prob["tgt"], prob["corr"], p_g, 64)
    assert raw(*a) == raw(*h)
