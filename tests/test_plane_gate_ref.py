"""CPU: the oracle's many-transforms plane entry is the single call bit for bit, and every gated case of tests/test_gpu_plane_gate.py really
has hypotheses the gate of plane_kernel MUST abandon (tests/plane_gate_lib.py states which) -- so that a device count of abandoned
hypotheses that stays above the library's figure means the gate ran, on a scene where it had something to do."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_gate_lib as G  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("score", [0, 2])
def test_many_is_the_single_call(oracle, score):
    """n transforms and n counters on one set-up of the target grid: counts, scores, metrics and pairs of n single calls"""
    from lgr_amd import synthetic
    sc = G.make_scene(20000, inlier_frac=0.4)
    hyp = G.hypotheses(oracle, sc, 300, G.LOOP["edge_thr_coef"])
    it = np.flatnonzero(hyp["ok"])[:8]
    rng = np.random.default_rng(score)
    Ts = [hyp["Ts"][i].reshape(4, 4).T for i in it] + [sc["T_gt"], np.eye(4, dtype=np.float32), synthetic.random_se3(rng).astype(np.float32)]
    counters = np.array(list(it) + [0xFFFFFFFD, 0, 7], np.uint32)
    many = oracle.evaluate_plane_many(sc["src"], sc["tgt"], np.stack([T.T.reshape(16) for T in Ts]), counters, score_id=score, seed=G.SEED, with_pairs=True)
    plain = oracle.evaluate_plane_many(sc["src"], sc["tgt"], np.stack([T.T.reshape(16) for T in Ts]), counters, score_id=score, seed=G.SEED)
    seen = 0
    for k, (T, counter) in enumerate(zip(Ts, counters)):
        one = oracle.evaluate_plane(sc["src"], sc["tgt"], T, score_id=score, seed=G.SEED, counter=int(counter), with_pairs=True)
        assert many["n_inl"][k] == one["n_inl"] == plain["n_inl"][k]
        assert bits(many["score"][k]) == bits(one["score"]) == bits(plain["score"][k])
        assert bits(many["metric"][k]) == bits(one["metric"]) == bits(plain["metric"][k])
        assert np.array_equal(many["pairs"][k], one["pairs"])
        assert bits(many["thr"]) == bits(one["thr"])
        seen += one["n_inl"]
    assert seen > 200 and many["n_inl"][len(it)] > 100        # (the planted transform has inliers; the random one need not)
    empty = oracle.evaluate_plane_many(sc["src"], sc["tgt"], np.zeros((0, 16), np.float32), np.zeros(0, np.uint32))
    assert len(empty["n_inl"]) == 0


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_has_certainly_abandoned_hypotheses(oracle, name):
    cert = G.case_certain(oracle, name)
    print(name, {k: cert[k] for k in ("certain", "certain_first", "evaluated", "two_rounds", "rounds")})
    G.check_case_condition(name, cert)
    assert cert["two_rounds"]                                  # `evaluated` is then what the device must report as scored on a subset
    if name == "closest_plane":                                # the recipe as it was tried: 746 survivors, 108 of them in the first batch
        assert cert["hyp"]["ok"].sum() == cert["evaluated"] == 746 and cert["hyp"]["ok"][:500].sum() == 108


def test_chunk_edge_sizes():
    for ns, n_sp in G.CHUNK_EDGES.items():
        assert G.n_sp_of(ns) == n_sp
    assert G.n_sp_of(G.N_MAIN) == 2500 and G.n_sp_of(99) == 0 and G.n_sp_of(100) == 1


def test_wrap_around_counters(oracle):
    """the two subsets of the device test that probe from the last index to 0, restated from the Philox words"""
    draws, taken, wrapped = G.subset(oracle, 400, 157030)
    assert draws == [25, 399, 356, 399] and taken == {0, 25, 356, 399} and wrapped
    draws, taken, wrapped = G.subset(oracle, 800, 6732)
    assert wrapped and {0, 799} <= taken and len(taken) == 8
    assert G.find_wrap(oracle, 800, start=6000, limit=1000) == 6732
    src = G.wrap_cloud(400)
    ref = oracle.evaluate_plane(src, src, np.eye(4, dtype=np.float32), counter=157030, with_pairs=True)
    assert ref["pairs"][:, 0].tolist() == [0, 25, 356, 399] == ref["pairs"][:, 1].tolist()
