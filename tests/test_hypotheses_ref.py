"""The statement of the hypothesis-set mode on the CPU (tests/hypotheses_ref_lib.py): what the device's second pass relies on, and that
the inputs of the GPU tests are not trivial.

The device never scores a hypothesis that cannot beat the best so far, so it builds the set from a second pass that keeps only the items
with !(metric < 0.1 * M*), M* = the loop's final best metric.  Here: on every input of tests/test_gpu_hypotheses.py the fold of those
items equals the fold of all items -- transforms, metrics, positions and order -- and the sets are large enough to mean something."""
import numpy as np
import pytest

import hypotheses_ref_lib as H


def same_set(a, b):
    assert np.array_equal(a["index"], b["index"])
    assert np.array_equal(H.bits(a["T"]), H.bits(b["T"]))
    assert np.array_equal(H.bits(a["metric"]), H.bits(b["metric"]))


@pytest.mark.parametrize("n,k,seed", H.POSE_LISTS)
def test_filtered_fold_equals_full_fold_on_the_pose_lists(oracle, n, k, seed):
    tns, met = H.pose_list(n, k, seed)
    full = H.fold(oracle, tns, met, H.DISTANCE_THR)
    m_star = met.max()   # the fold's best is the prefix maximum of the item metrics
    part = H.fold(oracle, tns, met, H.DISTANCE_THR, keep=H.keep_mask(met, m_star))
    same_set(full, part)
    print(f"list n={n} K={k} seed={seed}: set {len(full['metric'])} peak {full['peak']} changes {full['changes']}")
    assert len(full["metric"]) >= 30          # a condition on the input: the GPU test of the fold is not trivial
    assert full["changes"] > len(full["metric"])   # ... members were erased or pruned on the way
    assert np.isclose(full["metric"].max(), m_star, rtol=0, atol=0)


def test_pose_list_2_outgrows_a_set_of_64(oracle):
    tns, met = H.pose_list(*H.POSE_LISTS[1])
    assert H.fold(oracle, tns, met, H.DISTANCE_THR)["peak"] > 64
    assert H.fold(oracle, tns, met, H.DISTANCE_THR, cap=64) is None


@pytest.mark.parametrize("row", H.TWO_MODE_ROWS)
def test_filtered_fold_equals_full_fold_on_the_two_mode_problems(oracle, row):
    full = H.row_statement(oracle, row)
    part = H.row_statement(oracle, row, filtered=True)
    same_set(full["set"], part["set"])
    ores = full["ores"]
    prob = H.two_mode(row[1], row[2])
    print(f"row {row}: iterations {ores.iterations} items {full['n_items']} kept {full['n_items_kept']} set {len(full['members'])} "
          f"metrics {[float(m['loop_metric']) for m in full['members']]}")
    assert ores.iterations <= row[3] and full["n_items"] >= full["n_items_kept"] >= 2
    # M* is the loop's final best metric and equals the largest item metric
    _, its, Ts, ms = H.items_of_loop(oracle, prob, H.row_params(oracle, None, row)[0])
    assert np.float32(ores.best_metric_before_refit) == ms.max()
    assert len(full["members"]) >= 2          # a condition on the input: two modes, two members
    # each planted pose has a member that is similar to it in updateHypotheses' own sense
    for Tp in (prob["T1"], prob["T2"]):
        assert any(r < np.pi / 9 and t < np.float32(20 * np.float32(H.DISTANCE_THR))
                   for r, t in (oracle.rot_trans_diff(m["T"], Tp.astype(np.float32)) for m in full["members"]))
    assert full["best_index"] >= 0
