"""GPU: the gate of plane_kernel (csrc/lgr_plane.hip) -- the early abandoning of a hypothesis part-way through its sparse subset -- and the
subset's linear probing across the end of the cloud, against the gate-free oracle.

The gate is checked after every 1024 subset points while points are left, so it needs n_sp >= 1025: source clouds of 102 500 points and
more, which no other plane-metric test reaches.  Every whole-loop case runs twice in one context; both runs must give the oracle's result
in every field the whole-loop tests compare (bit for bit), and the number of abandoned hypotheses the context reports
(Context.ransac_plane_gate) must reach the number tests/plane_gate_lib.py proves certain on the CPU -- which tests/test_plane_gate_ref.py
holds to at least 20 per gated case -- or be exactly 0 where no check can run or no record exists yet.  WHICH hypotheses are abandoned,
and the partial count / metric such a hypothesis leaves in the round's arrays, depend on thread timing; no caller sees them (they lose
every reduction of rs_replay by the gate's own condition) and nothing here asserts them."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_gate_lib as G  # noqa: E402

pytestmark = pytest.mark.gpu
INT_FIELDS = ("iterations", "best_iteration", "num_rejections", "estimated_iters", "converged", "n_inliers")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_result(a, ma, b, mb):
    """every field the whole-loop tests compare, bit for bit (a, b: device or oracle results)"""
    for f in INT_FIELDS:
        assert getattr(a, f) == getattr(b, f), (f, getattr(a, f), getattr(b, f))
    np.testing.assert_array_equal(ma, mb)
    np.testing.assert_array_equal(bits(a.matrix()), bits(b.matrix()))
    assert bits(a.metric) == bits(b.metric), (a.metric, b.metric)
    assert bits(a.best_metric_before_refit) == bits(b.best_metric_before_refit), (a.best_metric_before_refit, b.best_metric_before_refit)


@pytest.fixture(scope="module")
def device_clouds():
    """the clouds of the current scene on the device (the cases come grouped by scene)"""
    held = {}

    def get(scene):
        if held.get("scene") is not scene:
            held.clear()
            held.update(scene=scene, src=cuda(scene["src"]), tgt=cuda(scene["tgt"]))
        return held["src"], held["tgt"]
    return get


def run_case(lgr, oracle, device_clouds, name, device_metric=None, weights=None):
    """the oracle's run of the case, the CPU statement of the certain count, and the device's run TWICE; returns what the cases compare"""
    from lgr_amd import capi
    t0 = time.time()
    scene, _ = G.case_scene(oracle, name)
    cert = G.case_certain(oracle, name)
    G.check_case_condition(name, cert)
    p_o, p_g = G.case_params(oracle, capi, name, metric=device_metric)
    ores, omask = oracle.ransac(scene["src"], scene["tgt"], G.to_orc_corr(oracle, scene["corr"]), p_o)
    t1 = time.time()
    s, t = device_clouds(scene)
    runs = []
    for _ in range(2):
        if weights is None:
            res, mask = lgr.ransac(s, t, scene["corr"], p_g)
        else:
            res, mask = lgr.ransac_ex(s, t, scene["corr"], p_g, capi.metric_params(weights=weights))
        runs.append((res, mask, lgr.ransac_plane_gate()))
    print(f"{name}: certain {cert['certain']} (first check {cert['certain_first']}), scored on a subset {cert['evaluated']}; device (scored, abandoned) "
          f"{runs[0][2]} {runs[1][2]}; oracle side {t1 - t0:.2f} s, device side {time.time() - t1:.2f} s")
    same_result(runs[0][0], runs[0][1], runs[1][0], runs[1][1])                   # run independent
    for _, _, (scored, abandoned) in runs:
        assert scored == cert["evaluated"], (scored, cert["evaluated"])
        if G.CASES[name].get("gated", True):
            assert cert["certain"] <= abandoned <= scored, (abandoned, cert["certain"])
        else:
            assert abandoned == 0
    return scene, cert, ores, omask, runs


@pytest.mark.parametrize("name", ["closest_plane", "closest_plane_guess", "closest_plane_guess_one_batch", "combination", "combination_score0", "combination_guess"])
def test_gated_loop_is_the_oracle(lgr, oracle, device_clouds, name):
    """metrics 2 and 3 at 250 000 points (n_sp = 2500: checks after 1024 and 2048 points), the best hypothesis found in the round the gate is live
    in.  With a good guess (the ground truth) the oracle, which applies no gate, still sets iterations and estimated_iters: under
    combination the guess's metric alone gates from the first round on, under closest_plane nothing is abandoned before the loop's own
    first record (`largest` starts at 0) -- the one-batch run ends before there is one, so its count is exactly 0."""
    scene, cert, ores, omask, runs = run_case(lgr, oracle, device_clouds, name)
    for res, mask, _ in runs:
        same_result(res, mask, ores, omask)
    assert ores.converged == 1 and np.abs(ores.matrix() - scene["T_gt"]).max() < 1e-3
    if G.CASES[name].get("guess"):
        assert ores.best_iteration == -1                                        # nothing beats the guess
    elif name != "combination_score0":
        assert ores.best_iteration >= G.LOOP["ransac_batch"]                   # found while the gate's state was live


@pytest.mark.parametrize("name", ["edge_102400", "edge_102500", "edge_204800", "edge_204900", "edge_409700"])
def test_chunk_edges(lgr, oracle, device_clouds, name):
    """n_sp = 1024 (no check runs: exactly 0 abandoned), 1025 (one check, one point left), 2048 and 2049 (the second check at and just
    past a chunk's end), 4097 (four checks)"""
    scene, cert, ores, omask, runs = run_case(lgr, oracle, device_clouds, name)
    for res, mask, _ in runs:
        same_result(res, mask, ores, omask)
    assert ores.converged == 1 and ores.n_inliers > 0.9 * G.n_sp_of(G.CASES[name]["ns"])


def test_weighted_gate_uniform_weights(lgr, oracle, device_clouds):
    """weighted_closest_plane with every weight 0.5 under the constant score: score and weight sum scale alike (a power of two: exactly), so
    every field is closest_plane's -- the oracle's -- through the W = true gate with w_gate = 0.5"""
    name = "weighted_uniform"
    w = G.case_weights(name, G.CASES[name]["ns"])[0]
    scene, cert, ores, omask, runs = run_case(lgr, oracle, device_clouds, name, device_metric=4, weights=cuda(w))
    for res, mask, _ in runs:
        same_result(res, mask, ores, omask)


def test_weighted_gate_callers_map(lgr, oracle, device_clouds):
    """a caller's map whose largest weight (20) is far above the mean (0.7): the reference from parts (plane_gate_lib.weighted_reference),
    the abandoned count against the certain count under the weighted bound"""
    name = "weighted_map"
    weights = G.case_weights(name, G.CASES[name]["ns"])
    scene, cert, ores, omask, runs = run_case(lgr, oracle, device_clouds, name, device_metric=4, weights=cuda(weights[0]))
    ref = G.weighted_reference(oracle, scene, cert, weights, G.CASES[name]["score"], ores.iterations)
    assert ref["best_iteration"] >= G.LOOP["ransac_batch"] and ref["converged"] == 1
    for res, mask, _ in runs:
        for f in ("iterations", "num_rejections", "estimated_iters"):          # the closest_plane run's: no weight enters them
            assert getattr(res, f) == getattr(ores, f), f
        assert res.best_iteration == ref["best_iteration"] and res.converged == ref["converged"] and res.n_inliers == ref["n_inliers"]
        assert bits(res.best_metric_before_refit) == bits(ref["best_metric_before_refit"])
        np.testing.assert_array_equal(bits(res.matrix()), bits(ref["matrix"]))
        assert bits(res.metric) == bits(ref["metric"])
        assert not mask.any()                                                   # (the plane metrics' inliers are plane pairs: no correspondence is flagged)
    assert np.abs(ref["matrix"] - scene["T_gt"]).max() < 1e-3


@pytest.mark.parametrize("ns,counter,want", [(400, 157030, [0, 25, 356, 399]), (800, 6732, None)])
def test_subset_wraps_around(lgr, oracle, ns, counter, want):
    """linear probing from index ns - 1 to 0: target = source under the identity, so the pairs list is the whole subset"""
    draws, taken, wrapped = G.subset(oracle, ns, counter)
    assert wrapped and {0, ns - 1} <= taken
    if want is not None:
        assert draws == [25, 399, 356, 399] and sorted(taken) == want
    src = G.wrap_cloud(ns)
    eye = np.eye(4, dtype=np.float32)
    ref = oracle.evaluate_plane(src, src, eye, counter=counter, with_pairs=True)
    got = lgr.evaluate_plane(cuda(src), cuda(src), eye, counter=counter, with_pairs=True)
    assert got["n_inl"] == ref["n_inl"] == G.n_sp_of(ns)
    assert np.array_equal(got["pairs"], ref["pairs"])
    assert got["pairs"][:, 0].tolist() == sorted(taken) == got["pairs"][:, 1].tolist()
    assert bits(got["metric"]) == bits(ref["metric"]) and bits(got["rmse"]) == bits(ref["rmse"]) and bits(got["thr"]) == bits(ref["thr"])


@pytest.mark.parametrize("ns", [99, 100])
def test_tiny_subsets(lgr, oracle, ns):
    """n_sp = 0 (nothing is evaluated: count 0, metric 0, rmse FLT_MAX) and n_sp = 1"""
    src = G.wrap_cloud(ns)
    eye = np.eye(4, dtype=np.float32)
    for counter in (0, 3):
        ref = oracle.evaluate_plane(src, src, eye, counter=counter, with_pairs=True)
        got = lgr.evaluate_plane(cuda(src), cuda(src), eye, counter=counter, with_pairs=True)
        assert got["n_inl"] == ref["n_inl"] == G.n_sp_of(ns)
        assert np.array_equal(got["pairs"], ref["pairs"]) and len(got["pairs"]) == G.n_sp_of(ns)
        assert bits(got["metric"]) == bits(ref["metric"]) and bits(got["rmse"]) == bits(ref["rmse"]) and bits(got["thr"]) == bits(ref["thr"])
        if ns == 99:
            assert got["metric"] == 0.0 and bits(got["rmse"]) == bits(np.finfo(np.float32).max)
