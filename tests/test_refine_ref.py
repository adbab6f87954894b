"""CPU: the statement of the iterated closest-plane refinement (tests/refine_ref_lib.py: plane_dense_ref_lib.evaluate + the oracle's refit)
behaves as the device tests need it to, on make_pair(4000, 12) with the oracle's normals and the perturbation of
tests/test_gpu_plane_dense.py::perturbed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref_lib as R  # noqa: E402

F = np.float32
MSE = 2


def same_step(a, b):
    return (np.array_equal(a["T"].view(np.uint32), b["T"].view(np.uint32)) and a["n_inliers"] == b["n_inliers"]
            and all(F(a[k]).view(np.uint32) == F(b[k]).view(np.uint32) for k in ("metric", "rmse", "score")))


def test_metric_rises_and_pose_improves(oracle):
    """MSE score, max_steps 40, thr = the target's density (0.0802...): 19 accepted steps, then a candidate whose metric is lower (NO_GAIN);
    metric 0.2529 -> 0.3901, inliers 1982 -> 2131 of 4000.  Against the ground truth the rotation error falls from 0.4999 to 0.1514
    degrees and the translation error from 0.04010 to 0.01005."""
    p = R.make_pair(oracle)
    r = R.reference(oracle, ("near", MSE, 40), p["src"], p["tgt"], p["T0"], MSE, p["thr"], 40)
    m = [float(s["metric"]) for s in r["trace"]]
    print("steps", r["steps"], "stop", r["stop"], "metrics", m)
    assert r["stop"] == R.STOP_NO_GAIN and r["rejected"] is r["trace"][-1] and len(r["trace"]) == r["steps"] + 2
    assert all(b > a for a, b in zip(m[:-2], m[1:-1])) and not (m[-1] > m[-2])   # strictly up over the accepted steps, then the loser
    assert r["steps"] >= 2 * R.GROUP + 1   # the device's group tests need that many
    assert same_step(r["trace"][r["steps"]], r) and same_step(r["trace"][0], r["first"])
    r0, t0 = R.errors(p["T0"], p["T_gt"])
    r1, t1 = R.errors(r["T"], p["T_gt"])
    print("rotation error (deg)", r0, "->", r1, "translation error", t0, "->", t1)
    assert r1 < r0 and t1 < t0
    assert r["n_inliers"] > r["first"]["n_inliers"] >= len(p["src"]) // 10


def test_max_steps_cuts_the_same_run(oracle):
    p = R.make_pair(oracle)
    full = R.reference(oracle, ("near", MSE, 40), p["src"], p["tgt"], p["T0"], MSE, p["thr"], 40)
    r = R.refine(oracle, p["src"], p["tgt"], p["T0"], MSE, p["thr"], 0)
    assert r["steps"] == 0 and r["stop"] == R.STOP_MAX_STEPS and r["rejected"] is None and len(r["trace"]) == 1
    assert np.array_equal(r["T"].view(np.uint32), p["T0"].view(np.uint32)) and same_step(r, full["first"])
    r = R.refine(oracle, p["src"], p["tgt"], p["T0"], MSE, p["thr"], 3)
    assert r["steps"] == 3 and r["stop"] == R.STOP_MAX_STEPS and r["rejected"] is None
    assert len(r["trace"]) == 4 and all(same_step(a, b) for a, b in zip(r["trace"], full["trace"]))


def test_far_pose_has_no_pairs(oracle):
    p = R.make_pair(oracle)
    r = R.refine(oracle, p["src"], p["tgt"], p["T_far"], MSE, p["thr"], 5)
    assert r["steps"] == 0 and r["stop"] == R.STOP_NO_PAIRS and r["n_inliers"] < 3 and r["rejected"] is None and len(r["trace"]) == 1
    assert np.array_equal(r["T"].view(np.uint32), p["T_far"].view(np.uint32))
    assert r["n_inliers"] == 0 and r["metric"] == 0 and r["rmse"] == np.finfo(F).max
    # max_steps is looked at first: without a step to take the reason is MAX_STEPS
    assert R.refine(oracle, p["src"], p["tgt"], p["T_far"], MSE, p["thr"], 0)["stop"] == R.STOP_MAX_STEPS
    e = R.refine(oracle, p["src"][:0], p["tgt"], p["T_far"], MSE, p["thr"], 5)
    assert e["steps"] == 0 and e["stop"] == R.STOP_NO_PAIRS and np.array_equal(e["T"], p["T_far"])
