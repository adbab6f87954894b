"""The statement of the hypothesis-set mode under the plane metrics on the CPU (tests/hypotheses_plane_ref_lib.py): what the device's
second pass relies on, and that the inputs of tests/test_gpu_hypotheses_plane.py are not trivial.

The device builds the set from a second pass that keeps only the items with !(metric < 0.1 * M*), M* = the loop's final best metric.
Here: on scene A (both sizes, both metrics) and scene B the fold of those items equals the fold of all items; on scene B the final block
of the member with the largest loop metric is oracle.ransac's result in all bits; and the conditions that keep the GPU tests honest hold:
both planted poses are in the set, at least two members and a peak of at most 64 on scene A, and at least one item below 0.1 * M* on
every combination row."""
import numpy as np
import pytest

import hypotheses_plane_ref_lib as HP
import hypotheses_ref_lib as H


def same_set(a, b):
    assert np.array_equal(a["index"], b["index"])
    assert np.array_equal(H.bits(a["T"]), H.bits(b["T"]))
    assert np.array_equal(H.bits(a["metric"]), H.bits(b["metric"]))


@pytest.mark.parametrize("n_pts", [4000, 30000])
@pytest.mark.parametrize("row", HP.ROWS_A)
def test_filtered_fold_equals_full_fold_on_scene_a(oracle, row, n_pts):
    full = HP.row_statement(oracle, row, n_pts)
    part = HP.row_statement(oracle, row, n_pts, filtered=True)
    same_set(full["set"], part["set"])
    below = full["n_items"] - full["n_items_kept"]
    print(f"scene A n_pts {n_pts} row {row}: iterations {full['ores'].iterations} items {full['n_items']} below {below} "
          f"members {len(full['members'])} peak {full['set']['peak']}")
    assert full["ores"].iterations <= row[3]
    assert len(full["members"]) >= 2 and full["set"]["peak"] <= 64
    if row[0] == 3:
        assert below >= 1          # the filter of the second pass has something to drop
    assert HP.has_both_modes(oracle, full["members"], HP.scene_a(n_pts, row[1], row[2]))
    assert full["best_index"] >= 0


@pytest.mark.parametrize("metric", [2, 3])
def test_scene_b_fold_and_the_best_member_is_the_single_result(oracle, metric):
    full = HP.scene_b_statement(oracle, metric)
    part = HP.scene_b_statement(oracle, metric, filtered=True)
    same_set(full["set"], part["set"])
    print(f"scene B metric {metric}: items {full['n_items']} members {len(full['members'])} peak {full['set']['peak']}")
    ores = full["ores"]
    k = int(np.argmax([m["loop_metric"] for m in full["members"]]))
    m = full["members"][k]
    assert m["iteration"] == ores.best_iteration and H.bits(m["loop_metric"]) == H.bits(ores.best_metric_before_refit)
    np.testing.assert_array_equal(H.bits(m["T"]), H.bits(ores.matrix()))
    assert m["converged"] == ores.converged and m["n_inliers"] == ores.n_inliers and H.bits(m["metric"]) == H.bits(ores.metric)
    if metric == 2:
        assert len(full["members"]) > 64       # the volumetric set: what max_set = 1024 in the GPU test is for
    else:
        assert len(full["members"]) == 1
