"""-m gpu: the multi-scale correspondence search (feature_radius unset: ms_initialize, ms_match_tables, ms_vote and descriptor_dev
in csrc/lgr_align.hip) with SHOT352 and RoPS135 (gravity frames) against the CPU statement of tests/multiscale_ref_lib.py, whose
fpfh form equals the oracle bit for bit (tests/test_multiscale_ref.py).

- F1 (two densities), F2 (levels pruned at both ends), F3 (no common level), F4 (duplicates: the block tie rule, equal vote counts)
  x key points any and ISS, and F5 (exact lattices: equal vote counts at bit-equal distances against different key points) x lr /
  one_sided / cluster x a block larger than every level and one smaller than a level: correspondences bit for bit, and
  lgr_align_ex_dev equals oracle.ransac (Philox) on the statement's correspondences.
- The reference's own default on its corner scene (SHOT, multi-scale, cluster, closest plane): correspondences equal the statement.
- The fixtures hold SHOT rows that are NaN on the finer levels only and RoPS key points whose re-estimated normal fails the gravity
  test on some level (SHOT frame fallback).
- With feature_radius unset too, SHOT and RoPS refuse FLANN, a guess and LGR_ARITH_PCL."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multiscale_ref_lib import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS = (200000, 1000)
FIXTURES = ("F1", "F2", "F3", "F4", "F5")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fixtures():
    import torch
    import multiscale_ref_lib as M
    out = {name: M.fixture(name) for name in FIXTURES}
    for p in out.values():
        p["s"], p["t"] = torch.from_numpy(p["src"]).cuda(), torch.from_numpy(p["tgt"]).cuda()
    return out


@pytest.fixture(scope="module")
def statements(oracle, fixtures):
    import multiscale_ref_lib as M
    cache = {}

    def get(desc, fx, kp):
        if (desc, fx, kp) not in cache:
            p = fixtures[fx]
            cache[(desc, fx, kp)] = M.Statement(oracle, p["src"], p["tgt"], desc, kp, iss_radius=CASES[(fx, kp)], vp=(p["vp_src"], p["vp_tgt"]))
        return cache[(desc, fx, kp)]
    return get


def _params(capi, p, mid, block, kp, radii, **extra):
    return dict(feature_radius=0.0, matching_id=mid, bf_block_size=block, distance_thr=0.1, keypoint_id=int(kp == "iss"),
                iss_radius_src=radii[0], iss_radius_tgt=radii[1], max_iterations=5000, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"], **extra)


def check_corr(got, want):
    assert len(got) == len(want)
    np.testing.assert_array_equal(got["index_query"], want["query"])
    np.testing.assert_array_equal(got["index_match"], want["match"])
    np.testing.assert_array_equal(bits(got["distance"]), bits(want["distance"]))
    np.testing.assert_array_equal(bits(got["threshold"]), bits(want["threshold"]))


def _desc(capi, desc):
    return capi.feature_params("rops", lrf_id=capi.LRF_GRAVITY) if desc == "rops" else desc


@pytest.mark.parametrize("fx,kp", list(CASES))
@pytest.mark.parametrize("desc", ["shot", "rops"])
def test_multiscale_equals_statement(lgr, oracle, fixtures, statements, desc, fx, kp):
    from lgr_amd import capi
    p = fixtures[fx]
    st = statements(desc, fx, kp)
    for block in BLOCKS:
        for mid in (capi.MATCH_LR, capi.MATCH_ONE_SIDED, capi.MATCH_CLUSTER):
            kw = _params(capi, p, mid, block, kp, CASES[(fx, kp)])
            want = st.correspondences(mid, block)
            got = lgr.correspondences(p["s"], p["t"], capi.default_params(**kw), descriptor=_desc(capi, desc))
            got = got.cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
            check_corr(got, want)
            res = lgr.align(p["s"], p["t"], capi.default_params(**kw), descriptor=_desc(capi, desc))
            assert res.n_correspondences == len(want)
            if fx == "F3":
                assert len(want) == 0      # no common level: nothing to match
                continue
            assert len(want) > 5
            ores, _ = oracle.ransac(p["src"], p["tgt"], want, oracle.default_params(rng_mode=oracle.RNG_PHILOX, **kw))
            assert (res.iterations, res.n_inliers, res.best_iteration, res.converged) == \
                (ores.iterations, ores.n_inliers, ores.best_iteration, ores.converged), (block, mid)
            np.testing.assert_array_equal(bits(res.matrix()), bits(ores.matrix()))


def test_fixtures_hold_the_edge_rows(statements):
    """SHOT rows that are NaN on a finer level only (edge points of the sparse half), and RoPS key points whose re-estimated normal
    fails the gravity test on some level, so the SHOT frame stands in"""
    nan_fine_only = 0
    for kp in ("any", "iss"):
        for side in statements("shot", "F1", kp).sides:
            bad = [np.zeros(len(side.kps), bool) for _ in side.lists]
            for s, (lst, rows) in enumerate(zip(side.lists, side.rows)):
                bad[s][lst[~np.isfinite(rows).all(1)]] = True
            for s in range(len(side.lists) - 1):
                later_ok = np.zeros(len(side.kps), bool)
                for u in range(s + 1, len(side.lists)):
                    later_ok[side.lists[u][np.isfinite(side.rows[u]).all(1)]] = True
                nan_fine_only += int((bad[s] & later_ok).sum())
    assert nan_fine_only > 0
    for fx in ("F1", "F2", "F3"):
        st = statements("rops", fx, "any")
        if st.sides is not None:
            fails = [int(f.sum()) for _, f in st.adapter.frames]
            assert sum(fails) > 0 and min(len(f) - int(f.sum()) for _, f in st.adapter.frames) > 0


@pytest.mark.parametrize("desc", ["shot", "rops"])
def test_fixtures_reach_the_vote_tie_rules(statements, desc):
    """F4: equal counts, decided by the distance; F5: equal counts at bit-equal distances against different train key points, where
    only ms_vote's strict '<' keeps the first level's candidate"""
    for fx, key in (("F4", "count_ties"), ("F5", "decisive_ties")):
        st = statements(desc, fx, "any")
        for block in BLOCKS:
            st.tables(block)
            assert min(x[key] for x in st.vote_stats[block]) > 50, (fx, block, st.vote_stats[block])


def test_reference_default_on_the_corner_scene(lgr, oracle):
    """the reference's own default (SHOT, multi-scale, cluster, closest plane) on its corner scene: the correspondences of the
    bounds test in tests/test_gpu_align_shot.py equal the statement"""
    import torch
    import multiscale_ref_lib as M
    from lgr_amd import capi
    from test_gpu_reference_acceptance import corner_scene, reference_params
    src, tgt, vp_src, vp_tgt = corner_scene()
    p = reference_params(capi, vp_src, vp_tgt)
    st = M.Statement(oracle, src, tgt, "shot", "any", iss_radius=(p.iss_radius_src, p.iss_radius_tgt), vp=(vp_src, vp_tgt))
    want = st.correspondences(p.matching_id, p.bf_block_size, p.distance_thr, p.cluster_k)
    got = lgr.correspondences(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), p, descriptor="shot")
    check_corr(got.cpu().numpy().view(capi.CORR_DTYPE).reshape(-1), want)
    assert len(want) > 100


def test_multiscale_unsupported_combinations(lgr):
    from lgr_amd import capi
    lib = capi.lib()
    import torch
    from lgr_amd import synthetic
    pair = synthetic.make_pair(4000, seed=21)
    s, t = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    res = capi.Result()
    out = lgr.empty((4000, 4), lgr.torch.int32)
    n = C.c_int(0)
    base = dict(feature_radius=0.0, bf_block_size=200000, max_iterations=100, distance_thr=0.1)
    for f in (capi.feature_params("shot"), capi.feature_params("rops", lrf_id=capi.LRF_GRAVITY)):
        for p in (capi.default_params(use_bfmatcher=0, **base), capi.default_params(guess=np.eye(4), match_search_radius=1.0, **base)):
            assert p.feature_radius == 0.0
            assert lib.lgr_align_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), C.byref(res)) == capi.ERR_UNSUPPORTED
            assert lib.lgr_correspondences_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), capi._ptr(out),
                                                  C.byref(n)) == capi.ERR_UNSUPPORTED
        lgr.set_options(arithmetic=capi.ARITH_PCL)
        try:
            p = capi.default_params(**base)
            assert lib.lgr_align_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), C.byref(res)) == capi.ERR_UNSUPPORTED
            assert lib.lgr_correspondences_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), capi._ptr(out),
                                                  C.byref(n)) == capi.ERR_UNSUPPORTED
        finally:
            lgr.set_options()
