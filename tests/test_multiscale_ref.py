"""CPU: the multi-scale statement of tests/multiscale_ref_lib.py with the fpfh adapter equals oracle.correspondences(feature_radius = 0)
bit for bit -- query, match, distance and threshold bits -- for lr / one_sided / cluster, key points any and ISS, and a block size
larger than every level and one smaller than a level (the matcher's cross-block tie rule).  Each fixture asserts the level case it
was built for from the statement's record, so the statement is trustworthy where the oracle has no descriptor (SHOT, RoPS:
tests/test_gpu_multiscale_descriptors.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multiscale_ref_lib import CASES  # noqa: E402

BLOCKS = (200000, 1000)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fixtures():
    import multiscale_ref_lib as M
    return {name: M.fixture(name) for name in ("F1", "F2", "F3", "F4", "F5")}


@pytest.fixture(scope="module")
def statements(oracle, fixtures):
    import multiscale_ref_lib as M
    cache = {}

    def get(fx, kp):
        if (fx, kp) not in cache:
            p = fixtures[fx]
            cache[(fx, kp)] = M.Statement(oracle, p["src"], p["tgt"], "fpfh", kp, iss_radius=CASES[(fx, kp)], vp=(p["vp_src"], p["vp_tgt"]))
        return cache[(fx, kp)]
    return get


@pytest.mark.parametrize("fx,kp", list(CASES))
def test_fpfh_statement_equals_oracle(oracle, fixtures, statements, fx, kp):
    p = fixtures[fx]
    st = statements(fx, kp)
    rs, rt = CASES[(fx, kp)]
    for block in BLOCKS:
        for mid in (oracle.MATCH_LR, oracle.MATCH_ONE_SIDED, oracle.MATCH_CLUSTER):
            kw = dict(feature_radius=0.0, matching_id=mid, bf_block_size=block, distance_thr=0.1, keypoint_id=int(kp == "iss"),
                      iss_radius_src=rs, iss_radius_tgt=rt, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"])
            want, _ = oracle.correspondences(p["src"], p["tgt"], oracle.default_params(**kw))
            got = st.correspondences(mid, block)
            assert len(got) == len(want), (block, mid)
            np.testing.assert_array_equal(got["query"], want["query"])
            np.testing.assert_array_equal(got["match"], want["match"])
            np.testing.assert_array_equal(bits(got["distance"]), bits(want["distance"]))
            np.testing.assert_array_equal(bits(got["threshold"]), bits(want["threshold"]))
            if fx == "F3":
                assert len(got) == 0
            elif fx == "F5":   # the lattice's equal rows leave few mutual matches; one_sided keeps every query
                assert len(got) > 0 and (mid != oracle.MATCH_ONE_SIDED or len(got) == len(p["src"]))
            else:
                assert len(got) > 10 if kp == "any" else len(got) > 5


def test_f1_several_levels(statements):
    for kp in ("any", "iss"):
        for rec in statements("F1", kp).records():
            assert rec["max_l2"] - rec["min_l2"] >= 1               # at least two levels per side
    rec = statements("F1", "any").records()
    for r in rec:   # the dense and the thinned half really sit on different levels: two levels hold >= 10 % of the largest each
        c = np.array(r["raw"]["count"])
        assert (10 * c >= c.max()).sum() >= 2
        assert r["radius"] == [2.0 ** (r["min_l2"] + i) for i in range(len(r["sizes"]))]
        assert r["sizes"] == sorted(r["sizes"])                    # a key point takes part in every level from its own up


def test_f2_pruned_at_both_ends(statements, fixtures):
    for r in statements("F2", "any").records():
        c = np.array(r["raw"]["count"])
        mx = c.max()
        # the lowest raw level (the dense blob) has fewer than 10 % of the largest level: pruned, its key points clamped up
        assert 10 * c[0] < mx and r["min_l2"] > r["raw"]["min_l2"] and r["n_clamped_up"] >= 100
        # the highest raw level (the lifted outliers) has fewer than 0.1 %: pruned, clamped down
        assert 1000 * c[-1] < mx and r["max_l2"] < r["raw"]["max_l2"] and r["n_clamped_down"] >= 3
        # the pruning stops at the first level that passes its rule
        lo, hi = r["min_l2"] - r["raw"]["min_l2"], r["max_l2"] - r["raw"]["min_l2"]
        assert 10 * c[lo] >= mx and 1000 * c[hi] >= mx


def test_f3_no_common_level(statements):
    for kp in ("any", "iss"):
        s, t = statements("F3", kp).records()
        assert max(s["min_l2"], t["min_l2"]) > min(s["max_l2"], t["max_l2"])
        for block in BLOCKS:
            ij, _, ji, _ = statements("F3", kp).tables(block)
            assert (ij == -1).all() and (ji == -1).all()
            for mid in (0, 1, 2):
                assert len(statements("F3", kp).correspondences(mid, block)) == 0


def test_f4_duplicates_meet_the_block_tie_rule_and_count_ties(statements, fixtures):
    st = statements("F4", "any")
    p = fixtures["F4"]
    orig, copy = p["dup_tgt"][:, 0], p["dup_tgt"][:, 1]
    t = st.sides[1]
    # equal positions give equal rows on every level both copies take part in
    for s, lst in enumerate(t.lists):
        pos = np.full(len(p["tgt"]), -1)
        pos[lst] = np.arange(len(lst))
        both = (pos[orig] >= 0) & (pos[copy] >= 0)
        assert both.sum() > 100
        np.testing.assert_array_equal(bits(t.rows[s][pos[orig[both]]]), bits(t.rows[s][pos[copy[both]]]))
    # one block: the lower index wins a tie inside the block; 1000-row blocks put the copies in a later block, which wins
    ij_one = st.tables(200000)[0]
    ij_blk = st.tables(1000)[0]
    assert np.isin(ij_one, orig).sum() > 50 and not np.isin(ij_one, copy).any()
    assert np.isin(ij_blk, copy).sum() > 50
    # the vote: candidates with equal counts, decided by the distance
    for block in BLOCKS:
        assert min(x["count_ties"] for x in st.vote_stats[block]) > 100


def test_f5_lattice_meets_the_vote_distance_tie(statements):
    """equal counts at bit-equal distances against different train key points: only the strict '<' keeps the first level's candidate"""
    st = statements("F5", "any")
    s, t = st.records()
    assert s["max_l2"] > s["min_l2"] and s == t
    for block in BLOCKS:
        st.tables(block)
        assert min(x["decisive_ties"] for x in st.vote_stats[block]) > 100


def test_level_arithmetic_rounds_through_float():
    """sqrtf((float) nr * d * d / M_PI) rounds to float before sqrtf and log2f: at these squared distances, one float below a level
    boundary, the float chain lands on the upper level and the same formula in double on the lower one.  (Which of the float steps
    round where is pinned by the bit-exact comparison with the oracle above.)"""
    import multiscale_ref_lib as M
    d2 = np.array([957495826, 974273042], np.uint32).view(np.float32)
    np.testing.assert_array_equal(M.level_of(d2, 352, 2.0), [-3, -2])
    in_double = np.floor(np.log2(np.sqrt(352 * d2.astype(np.float64) / np.pi))).astype(int)
    np.testing.assert_array_equal(in_double, [-4, -3])
    r, v = M.radius_voxel(-3, 352, 2.0)
    assert r == np.float32(0.125) and v == np.float32(np.sqrt(np.float32(np.pi * 0.125 * 0.125 / 352)))
