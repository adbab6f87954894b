"""GPU parity of the hypothesis-set mode (lgr_fold_hypotheses_dev, lgr_ransac_multi_dev) against the statement composed from the oracle
(tests/hypotheses_ref_lib.py).  Bars: bit-exact -- set members, their order, metrics, source indices, every field of every member after
the final block, the choice."""
import numpy as np
import pytest

import hypotheses_ref_lib as H

pytestmark = pytest.mark.gpu
bits = H.bits


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_fold(lgr, tns, met, max_set=H.CAP):
    return lgr.fold_hypotheses(cuda(tns), cuda(met), H.DISTANCE_THR, max_set)


def check_fold(lgr, oracle, tns, met, max_set=H.CAP):
    want = H.fold(oracle, tns, met, H.DISTANCE_THR)
    T, m, idx = gpu_fold(lgr, tns, met, max_set)
    np.testing.assert_array_equal(idx, want["index"])
    np.testing.assert_array_equal(bits(m), bits(want["metric"]))
    np.testing.assert_array_equal(bits(T), bits(want["T"]))
    return want


# ---- 1. the fold alone
@pytest.mark.parametrize("n,k,seed", H.POSE_LISTS)
def test_fold_of_the_pose_lists(lgr, oracle, n, k, seed):
    tns, met = H.pose_list(n, k, seed)
    want = check_fold(lgr, oracle, tns, met)
    assert len(want["metric"]) >= 30


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_fold_of_a_prefix(lgr, oracle, n):
    tns, met = H.pose_list(*H.POSE_LISTS[0])
    check_fold(lgr, oracle, tns[:n], met[:n])


def test_fold_of_a_prefix_host_arrays(lgr, oracle):
    tns, met = H.pose_list(*H.POSE_LISTS[0])
    want = H.fold(oracle, tns[:257], met[:257], H.DISTANCE_THR)
    T, m, idx = lgr.fold_hypotheses_host(tns[:257], met[:257], H.DISTANCE_THR, 512)
    np.testing.assert_array_equal(idx, want["index"])
    np.testing.assert_array_equal(bits(m), bits(want["metric"]))
    np.testing.assert_array_equal(bits(T), bits(want["T"]))


def test_fold_of_identical_poses_keeps_the_last(lgr, oracle):
    tns, _ = H.pose_list(*H.POSE_LISTS[2])
    tns = np.repeat(tns[:1], 200, axis=0)
    met = np.full(200, 0.5, np.float32)
    want = check_fold(lgr, oracle, tns, met)
    assert want["index"].tolist() == [199]   # a similar member with an EQUAL metric is erased


@pytest.mark.parametrize("rising", [False, True])
def test_fold_of_monotonic_metrics_from_one_centre(lgr, oracle, rising):
    tns, _ = H.pose_list(300, 1, 5)
    met = np.linspace(0.05, 0.95, 300).astype(np.float32)
    assert (np.diff(met) > 0).all()
    want = check_fold(lgr, oracle, tns, met if rising else met[::-1].copy())
    assert len(want["metric"]) >= 2


def test_fold_refuses_a_set_that_outgrows_max_set(lgr, oracle):
    from lgr_amd import capi
    tns, met = H.pose_list(*H.POSE_LISTS[1])
    assert H.fold(oracle, tns, met, H.DISTANCE_THR)["peak"] == 325
    with pytest.raises(capi.LgrError, match=f"rc={capi.ERR_UNSUPPORTED}"):
        gpu_fold(lgr, tns, met, 64)
    check_fold(lgr, oracle, tns, met, 325)   # the peak itself fits


# ---- 2. the whole mode
def run_multi(lgr, row, max_set=64, **extra):
    from lgr_amd import capi
    prob = H.two_mode(row[1], row[2])
    import oracle
    _, p_g = H.row_params(oracle, capi, row, **extra)
    src, tgt = cuda(prob["src"]), cuda(prob["tgt"])
    return lgr.ransac_multi(src, tgt, prob["corr"], p_g, max_set), (src, tgt, prob, p_g)


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


@pytest.mark.parametrize("row", H.TWO_MODE_ROWS)
def test_whole_mode_on_the_two_mode_problems(lgr, oracle, row):
    want = H.row_statement(oracle, row)
    (res, hyps, bi), (src, tgt, prob, p_g) = run_multi(lgr, row)
    check_members(hyps, want)
    check_choice(res, bi, want)
    single, _ = lgr.ransac(src, tgt, prob["corr"], p_g)
    check_loop_fields(res, single)
    assert res.iterations == want["ores"].iterations
    if row[4] == 64:   # these rows are here for a second pass of several rounds (16 batches each)
        assert res.iterations > 2 * 16 * row[4]
    assert len(hyps) >= 2
    t_thr = np.float32(20 * np.float32(H.DISTANCE_THR))
    for Tp in (prob["T1"], prob["T2"]):   # updateHypotheses' own similarity test, no tolerance of ours
        assert any(r < np.pi / 9 and t < t_thr for r, t in (oracle.rot_trans_diff(h.matrix(), Tp.astype(np.float32)) for h in hyps))


# ---- 3. the guess is the first item
def test_whole_mode_with_a_guess(lgr, oracle):
    row = H.TWO_MODE_ROWS[0]
    G = H.two_mode(row[1], row[2])["T2"].astype(np.float32)
    want = H.row_statement(oracle, row, guess=G)
    assert want["item_iterations"][0] == -1
    (res, hyps, bi), (src, tgt, prob, p_g) = run_multi(lgr, row, guess=G)
    check_members(hyps, want)
    check_choice(res, bi, want)
    single, _ = lgr.ransac(src, tgt, prob["corr"], p_g)
    check_loop_fields(res, single)


# ---- 4. one mode: the set has one member and the mode returns the single-hypothesis result
def test_single_mode_problem_equals_ransac(lgr, oracle):
    from lgr_amd import capi, synthetic
    prob = synthetic.make_correspondence_problem(n_pts=4000, c=1500, inlier_frac=0.4, seed=3)
    p_o, p_g = H.params_pair(oracle, capi, metric_id=1, score_id=2, distance_thr=H.DISTANCE_THR, max_iterations=6000, ransac_batch=1000)
    want = H.statement(oracle, prob, p_o)
    src, tgt = cuda(prob["src"]), cuda(prob["tgt"])
    res, hyps, bi = lgr.ransac_multi(src, tgt, prob["corr"], p_g, 64)
    check_members(hyps, want)
    check_choice(res, bi, want)
    if len(want["members"]) == 1 and want["members"][0]["uniformity"] > 0:
        single, _ = lgr.ransac(src, tgt, prob["corr"], p_g)
        assert bi == 0 and res.n_inliers == single.n_inliers and bits(res.metric) == bits(single.metric)
        np.testing.assert_array_equal(bits(res.matrix()), bits(single.matrix()))
        assert res.converged == single.converged


# ---- 5.-7. refusals and the empty case
def test_max_set_of_one_is_refused_on_two_modes(lgr):
    from lgr_amd import capi
    with pytest.raises(capi.LgrError, match=f"rc={capi.ERR_UNSUPPORTED}"):
        run_multi(lgr, H.TWO_MODE_ROWS[0], max_set=1)


@pytest.mark.parametrize("kw", [dict(metric_id=2), dict(metric_id=3), dict(metric_id=4), dict(alignment_id=1)])
def test_unsupported_modes_are_refused(lgr, kw):
    from lgr_amd import capi
    prob = H.two_mode(0.30, 0.18)
    p = capi.default_params(score_id=2, distance_thr=H.DISTANCE_THR, max_iterations=1000, ransac_batch=1000, **kw)
    with pytest.raises(capi.LgrError, match=f"rc={capi.ERR_UNSUPPORTED}"):
        lgr.ransac_multi(cuda(prob["src"]), cuda(prob["tgt"]), prob["corr"], p, 64)


def test_two_correspondences_give_an_empty_set(lgr):
    from lgr_amd import capi
    prob = H.two_mode(0.30, 0.18)
    p = capi.default_params(metric_id=1, score_id=2, distance_thr=H.DISTANCE_THR, max_iterations=1000, ransac_batch=1000)
    res, hyps, bi = lgr.ransac_multi(cuda(prob["src"]), cuda(prob["tgt"]), prob["corr"][:2], p, 64)
    assert hyps == [] and bi == -1 and res.iterations == 0 and res.converged == 0
    np.testing.assert_array_equal(res.matrix(), np.eye(4, dtype=np.float32))


# ---- 8.-9. repeatability, schedules
def raw(res, hyps, bi):
    import ctypes as C
    skip = type(res).time_cs.offset   # the timings behind it differ from call to call
    return bytes(C.string_at(C.addressof(res), skip)) + b"".join(bytes(C.string_at(C.addressof(h), C.sizeof(h))) for h in hyps) + bytes([bi & 0xff])


def test_two_calls_on_one_context_give_identical_bytes(lgr):
    a, _ = run_multi(lgr, H.TWO_MODE_ROWS[3])
    b, _ = run_multi(lgr, H.TWO_MODE_ROWS[3])
    assert raw(*a) == raw(*b) and len(a[1]) >= 2


def test_resident_schedule_option_returns_the_chain_bytes(lgr):
    a, _ = run_multi(lgr, H.TWO_MODE_ROWS[1])
    lgr.set_options(ransac_schedule=2)
    try:
        b, _ = run_multi(lgr, H.TWO_MODE_ROWS[1])
    finally:
        lgr.set_options()
    assert raw(*a) == raw(*b) and len(a[1]) >= 2


def test_host_arrays_entry_point(lgr, oracle):
    from lgr_amd import capi
    row = H.TWO_MODE_ROWS[2]
    prob = H.two_mode(row[1], row[2])
    _, p_g = H.row_params(oracle, capi, row)
    res, hyps, bi = lgr.ransac_multi_host(prob["src"], prob["tgt"], prob["corr"], p_g, 64)
    want = H.row_statement(oracle, row)
    check_members(hyps, want)
    check_choice(res, bi, want)
