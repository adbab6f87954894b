"""GPU: the iterated closest-plane refinement (lgr_refine_plane*) against the CPU statement tests/refine_ref_lib.py -- plane_dense_ref_lib's
evaluation + the oracle's refit in a loop: the 16 floats of every evaluated transform, metric, rmse and score bit for bit (compared as
uint32), the counts, the step count and the stop reason equal.  make_pair(4000, 12) with the oracle's normals at the perturbation of
tests/test_gpu_plane_dense.py; under the MSE score the statement takes S = 19 steps there and then meets a candidate that loses
(tests/test_refine_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref_lib as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
MSE = 2
G = R.GROUP
MAX = 40


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared pair is read-only)


def u32(v):
    return np.asarray(v, F).view(np.uint32)


def step_bits(s):
    """a capi.RefineStep / RefineResult or a statement's step -> (16 transform words, metric, rmse, score words, count)"""
    if isinstance(s, dict):
        return (u32(s["T"].T.reshape(16)).tolist(), int(u32(s["metric"])), int(u32(s["rmse"])), int(u32(s["score"])), s["n_inliers"])
    return (u32(np.array(s.transformation, F)).tolist(), int(u32(s.metric)), int(u32(s.rmse)), int(u32(s.score)), s.n_inliers)


ZERO_STEP = ([0] * 16, 0, 0, 0, 0)


def check(dev, ref, trace=True):
    assert (dev.steps, dev.stop) == (ref["steps"], ref["stop"]), (dev.steps, dev.stop, ref["steps"], ref["stop"])
    assert step_bits(dev) == step_bits(ref)
    assert step_bits(dev.first) == step_bits(ref["first"])
    assert step_bits(dev.rejected) == (ZERO_STEP if ref["rejected"] is None else step_bits(ref["rejected"]))
    assert int(u32(dev.threshold)) == int(u32(ref["threshold"]))
    assert dev.reserved0 == 0 and list(dev.reserved) == [0] * 4
    if trace:
        assert len(dev.trace) == len(ref["trace"])
        for k, (a, b) in enumerate(zip(dev.trace, ref["trace"])):
            assert step_bits(a) == step_bits(b), k
    else:
        assert dev.trace is None


def cut(full, m):
    """the statement at max_steps = m from a longer run of it (the loop does not look at max_steps before it stops: tests/test_refine_ref.py)"""
    S = full["steps"]
    if m > S:
        return full
    tr = full["trace"][: m + 1]
    return dict(tr[m], threshold=full["threshold"], steps=m, stop=R.STOP_MAX_STEPS, first=full["first"], rejected=None, trace=tr)


@pytest.fixture(scope="module")
def pair(oracle):
    p = dict(R.make_pair(oracle))
    p.update(d_src=cuda(p["src"]), d_tgt=cuda(p["tgt"]))
    return p


def full_run(oracle, pair, score_id=MSE):
    return R.reference(oracle, ("near", score_id, MAX), pair["src"], pair["tgt"], pair["T0"], score_id, pair["thr"], MAX)


@pytest.mark.parametrize("score_id", [0, 1, 2, 3])
def test_near_ground_truth(lgr, oracle, pair, score_id):
    ref = full_run(oracle, pair, score_id)
    assert ref["stop"] == R.STOP_NO_GAIN and ref["steps"] >= 2 * G + 1   # not vacuous (the constant score stops on a TIE of the metric)
    d_src, d_tgt, T0, thr = pair["d_src"], pair["d_tgt"], pair["T0"], pair["thr"]
    dev = lgr.refine_plane(d_src, d_tgt, T0, score_id, MAX, trace=True)                      # threshold computed
    check(dev, ref)
    check(lgr.refine_plane(d_src, d_tgt, T0, score_id, MAX, threshold=dev.threshold, trace=True), ref)   # passed in
    check(lgr.refine_plane(d_src, d_tgt, T0, score_id, MAX, threshold=thr), ref, trace=False)           # no trace
    check(lgr.refine_plane_host(pair["src"], pair["tgt"], T0, score_id, MAX, trace=True), ref)           # the host twin
    check(lgr.refine_plane_host(pair["src"], pair["tgt"], T0, score_id, MAX, threshold=thr), ref, trace=False)


def test_stop_paths(lgr, oracle, pair):
    full = full_run(oracle, pair)
    S = full["steps"]
    for m in (0, 1, S - 1, S, S + 1):
        ref = cut(full, m)
        assert ref["stop"] == (R.STOP_NO_GAIN if m == S + 1 else R.STOP_MAX_STEPS)
        dev = lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T0"], MSE, m, threshold=pair["thr"], trace=True)
        check(dev, ref)
        assert len(dev.trace) == min(m, S) + 1 + (m == S + 1)
    assert step_bits(dev.rejected) == step_bits(full["trace"][-1]) != ZERO_STEP   # S + 1: the loser is reported


def test_group_edges(lgr, oracle, pair):
    full = full_run(oracle, pair)
    for m in (G - 1, G, G + 1, 2 * G, 2 * G + 1):
        check(lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T0"], MSE, m, threshold=pair["thr"], trace=True), cut(full, m))
    # a stop INSIDE a group: at 0.4 x the density the statement accepts 24 steps, so the loser is the FIRST step of the seventh group and the
    # three steps enqueued behind it must leave the state and the trace alone (chosen on the CPU; 0.25, 0.5 and 1 x end a group); under the
    # constant score (test_near_ground_truth) the loser is the third step of its group
    thr = float(F(0.4 * pair["thr"]))
    ref = R.reference(oracle, ("near", MSE, MAX, "0.4"), pair["src"], pair["tgt"], pair["T0"], MSE, thr, MAX)
    assert ref["stop"] == R.STOP_NO_GAIN and (ref["steps"] + 1) % G == 1, ref["steps"]
    dev = lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T0"], MSE, MAX, threshold=thr, trace=True)
    check(dev, ref)
    # ... and the call after it starts from a clean state
    check(lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T0"], MSE, G + 1, threshold=pair["thr"], trace=True), cut(full, G + 1))


def test_far_pose(lgr, oracle, pair):
    ref = R.refine(oracle, pair["src"], pair["tgt"], pair["T_far"], MSE, pair["thr"], 5)
    dev = lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T_far"], MSE, 5, trace=True)
    check(dev, ref)
    assert dev.stop == R.STOP_NO_PAIRS and dev.steps == 0 and dev.n_inliers == 0 and dev.metric == 0 and dev.rmse == FLT_MAX
    assert np.array_equal(u32(dev.matrix()), u32(pair["T_far"])) and len(dev.trace) == 1
    # an empty source: nothing to do, T0 comes back
    e = lgr.refine_plane(pair["d_src"][:0], pair["d_tgt"], pair["T_far"], MSE, 5, trace=True)
    check(e, R.refine(oracle, pair["src"][:0], pair["tgt"], pair["T_far"], MSE, pair["thr"], 5) | dict(threshold=F(0)))
    e = lgr.refine_plane_host(pair["src"][:0], pair["tgt"], pair["T_far"], MSE, 5, threshold=pair["thr"])
    assert (e.steps, e.stop, e.rmse) == (0, R.STOP_NO_PAIRS, FLT_MAX) and np.array_equal(u32(e.matrix()), u32(pair["T_far"]))


def test_ties_survive_the_loop(lgr, oracle):
    """the lattice of tests/test_gpu_plane_dense.py: the target is the source's integer lattice shifted by half a cell along x and row 0 of
    T0 is (1, 0, 0, 0), so at T0 every source point with x >= 1 has two nearest targets at equal squared distance with different normals
    and the lower index must win -- in the first evaluation and, through the pairs it hands the refit, in every transform after it"""
    n, thr = 12, 0.4
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(F)
    nrm = np.where((g[:, :1] % 2) == 0, np.array([[0, 0, 1]], F), np.array([[1, 0, 0]], F))   # alternate with x
    src = np.zeros((len(g), 12), F)
    src[:, :3] = g; src[:, 3] = 1; src[:, 4:7] = nrm; src[:, 8] = 1
    tgt = src.copy()
    tgt[:, 0] += 0.5
    a = 0.04
    T = np.eye(4, dtype=F)
    T[1:3, 1:3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[1:3, 3] = (0.0625, 0.03125)
    for score_id in (0, MSE):
        ref = R.refine(oracle, src, tgt, T, score_id, thr, 6)
        assert ref["first"]["n_inliers"] > 3 and len(ref["trace"]) >= 2
        check(lgr.refine_plane(cuda(src), cuda(tgt), T, score_id, 6, threshold=thr, trace=True), ref)


@pytest.mark.parametrize("ns", [2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_source_sizes(lgr, oracle, pair, ns):
    s = pair["src"][:ns]
    ref = R.refine(oracle, s, pair["tgt"], pair["T0"], MSE, pair["thr"], 6)
    check(lgr.refine_plane(cuda(s), pair["d_tgt"], pair["T0"], MSE, 6, threshold=pair["thr"], trace=True), ref)
    check(lgr.refine_plane_host(s, pair["tgt"], pair["T0"], MSE, 6, threshold=pair["thr"], trace=True), ref)


@pytest.mark.parametrize("ns", [4095, 4096, 4097, 8193])
def test_source_sizes_across_sum_tiles(lgr, oracle, pair, ns):
    """refine_sum_kernel takes its terms in tiles of 4096 (GT_SUM_TILE, staged one ahead): a tile short of one term, exactly one, one
    term into the second, one term into the third.  The source is the fixture's repeated and cut to ns; two steps."""
    s = np.concatenate([pair["src"]] * 3)[:ns]
    ref = R.refine(oracle, s, pair["tgt"], pair["T0"], MSE, pair["thr"], 2)
    assert ref["first"]["n_inliers"] > ns // 10 and len(ref["trace"]) >= 2
    check(lgr.refine_plane(cuda(s), pair["d_tgt"], pair["T0"], MSE, 2, threshold=pair["thr"], trace=True), ref)


def test_non_finite_points_and_normals(lgr, oracle, pair):
    src, tgt, T0, thr = (pair[k] for k in ("src", "tgt", "T0", "thr"))
    s_bad = src.copy()
    rows = np.arange(5, len(src), 97)
    s_bad[rows[0::3], 0] = np.nan
    s_bad[rows[1::3], 1] = np.inf
    s_bad[rows[2::3], 2] = -np.inf
    ref = R.refine(oracle, s_bad, tgt, T0, MSE, thr, 6)
    assert ref["steps"] >= 2
    check(lgr.refine_plane(cuda(s_bad), pair["d_tgt"], T0, MSE, 6, threshold=thr, trace=True), ref)
    t_bad = tgt.copy()
    t_bad[3::11, 5] = np.nan    # normals
    t_bad[7::13, :3] = np.nan   # points
    ref = R.refine(oracle, src, t_bad, T0, MSE, thr, 6)
    assert ref["steps"] >= 2 and np.isfinite(ref["metric"])
    check(lgr.refine_plane(pair["d_src"], cuda(t_bad), T0, MSE, 6, threshold=thr, trace=True), ref)


def test_weights(lgr, oracle, pair):
    from lgr_amd import capi
    src, tgt, T0, thr = (pair[k] for k in ("src", "tgt", "T0", "thr"))
    plain = cut(full_run(oracle, pair), 6)
    w, _ = lgr.weights(pair["d_src"], "exp_curvature")
    ref = R.refine(oracle, src, tgt, T0, MSE, thr, 6, weights=w.cpu().numpy())
    assert int(u32(ref["metric"])) != int(u32(plain["metric"]))
    check(lgr.refine_plane(pair["d_src"], pair["d_tgt"], T0, MSE, 6, threshold=thr, metric_params=capi.metric_params("exp_curvature"), trace=True), ref)
    rng = np.random.default_rng(3)
    wc = rng.uniform(-0.25, 1.0, len(src)).astype(F)
    wc[::7] = 0
    ref = R.refine(oracle, src, tgt, T0, 3, thr, 6, weights=wc)
    d_wc = cuda(wc)
    check(lgr.refine_plane(pair["d_src"], pair["d_tgt"], T0, 3, 6, threshold=thr, metric_params=capi.metric_params(weights=d_wc), trace=True), ref)
    check(lgr.refine_plane_host(src, tgt, T0, 3, 6, threshold=thr, metric_params=capi.metric_params(weights=wc), trace=True), ref)


def test_same_loop_composed_on_the_device(lgr, pair):
    """no CPU in this one: the loop driven from Python through lgr_evaluate_plane_dense_dev + lgr_refit_svd_dev gives the same bits"""
    d_src, d_tgt, thr = pair["d_src"], pair["d_tgt"], pair["thr"]
    m = 2 * G + 1
    dev = lgr.refine_plane(d_src, d_tgt, pair["T0"], MSE, m, threshold=thr, trace=True)
    assert dev.steps == m and len(dev.trace) == m + 1
    T = pair["T0"]
    for k in range(m + 1):
        e = lgr.evaluate_plane_dense(d_src, d_tgt, T, MSE, threshold=thr, with_inliers=True)
        got = dev.trace[k]
        assert u32(got.matrix()).tolist() == u32(T).tolist(), k
        assert (int(u32(got.metric)), int(u32(got.rmse)), int(u32(got.score)), got.n_inliers) == (int(u32(e.metric)), int(u32(e.rmse)), int(u32(e.score)), e.n_inliers), k
        if k < m:
            T = lgr.refit(d_src, d_tgt, e.inliers)


def test_context_reuse(lgr, pair):
    from lgr_amd import capi, synthetic
    p = synthetic.make_pair(4000, seed=5)
    src, tgt = cuda(p["src"]), cuda(p["tgt"])
    prm = capi.default_params(matching_id=0, bf_block_size=200000, max_iterations=5000, distance_thr=0.1, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"])
    a = lgr.align(src, tgt, prm)
    r1 = lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T0"], MSE, G + 1, trace=True)
    b = lgr.align(src, tgt, prm)
    r2 = lgr.refine_plane(pair["d_src"], pair["d_tgt"], pair["T0"], MSE, G + 1, trace=True)
    assert u32(a.matrix()).tolist() == u32(b.matrix()).tolist() and (a.n_inliers, a.iterations, a.converged) == (b.n_inliers, b.iterations, b.converged)
    assert [step_bits(s) for s in r1.trace] == [step_bits(s) for s in r2.trace] and (r1.steps, r1.stop) == (r2.steps, r2.stop)


def test_refusals(lgr, pair):
    from lgr_amd import capi
    d_src, d_tgt, T0 = pair["d_src"], pair["d_tgt"], pair["T0"]
    bad = [dict(max_steps=-1), dict(max_steps=capi.REFINE_MAX_STEPS + 1), dict(score_id=-1), dict(score_id=4), dict(threshold=float("nan")), dict(threshold=2e18)]
    for kw in bad:
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.refine_plane(d_src, d_tgt, T0, **kw)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.refine_plane_host(pair["src"], pair["tgt"], T0, **kw)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.refine_plane(d_src, d_tgt[:1], T0)
    import ctypes as C
    out, n = capi.RefineResult(), C.c_int(0)
    p = capi.refine_params()
    args = lambda **k: [k.get("src", capi._ptr(d_src)), k.get("ns", len(pair["src"])), k.get("tgt", capi._ptr(d_tgt)), len(pair["tgt"]), k.get("T", lgr._T16(T0)),  # noqa: E731
                        k.get("p", C.byref(p)), None, k.get("out", C.byref(out)), k.get("trace"), k.get("n")]
    for k in (dict(src=None), dict(tgt=None), dict(T=None), dict(p=None), dict(out=None), dict(ns=-1), dict(trace=(capi.RefineStep * 12)())):
        assert capi.lib().lgr_refine_plane_dev(lgr.h, *args(**k)) == -1, list(k)
    p.reserved[4] = 1
    assert capi.lib().lgr_refine_plane_dev(lgr.h, *args()) == -1
    p.reserved[4] = 0
    assert capi.lib().lgr_refine_plane_dev(lgr.h, *args()) == 0
    for name in ("harris", "tomasi"):
        with pytest.raises(capi.LgrError, match="rc=-5"):
            lgr.refine_plane(d_src, d_tgt, T0, metric_params=capi.metric_params(name))
