"""-m gpu: prepared clouds (lgr_cloud: csrc/lgr_cloud.hip and the prepared entry points of csrc/lgr_align.hip).

- lgr_correspondences_prepared_dev returns the bytes of lgr_correspondences_ex_dev and lgr_align_prepared the lgr_result of
  lgr_align_ex2_dev (time fields apart; stage_ms[0..2] are 0), single scale and multi-scale, every matcher and filter.
- One prepared cloud serves any number of pairs on both sides and is bit-equal afterwards.
- The getters equal the CPU statement of tests/multiscale_ref_lib.py (multi-scale) and the public per-stage calls (single scale).
- The reference's tests/keypoint_extraction.cpp property: the rows at the ISS key points equal the rows of the same points when
  every point is a key point.
- The contract: fingerprint mismatches and NULLs are LGR_ERR_INVALID_ARG, the pinned unsupported combinations keep their code,
  clouds without two points give nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multiscale_ref_lib import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS = (200000, 1000)     # the two block sizes of test_gpu_multiscale_descriptors.py
RESULT_FIELDS = ("iterations", "converged", "n_inliers", "metric", "best_metric_before_refit", "best_iteration", "num_rejections",
                 "estimated_iters", "n_correspondences")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(corr):
    return corr.cpu().numpy().copy()


def same_result(got, want):
    np.testing.assert_array_equal(bits(np.array(got.transformation)), bits(np.array(want.transformation)))
    for f in RESULT_FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a == b or (a != a and b != b), (f, a, b)
    assert list(got.stage_ms)[:3] == [0.0, 0.0, 0.0]


def _desc(capi, desc, **kw):
    if isinstance(desc, str):
        return capi.feature_params(desc, lrf_id=capi.LRF_GRAVITY if desc == "rops" else None, **kw)
    return desc


def check_pair(lgr, s, t, params, desc, mparams=None, align=True, min_corr=None):
    """prepared == unprepared for one pair; returns the number of correspondences"""
    want = raw(lgr.correspondences(s, t, params, descriptor=desc))
    with lgr.prepare_cloud(s, params, 0, desc) as a, lgr.prepare_cloud(t, params, 1, desc) as b:
        got = raw(lgr.correspondences_prepared(a, b, params, descriptor=desc))
        assert got.shape == want.shape and (got == want).all()
        if min_corr is not None:
            assert len(want) > min_corr     # a case without correspondences is a wrong fixture, not a pass
        if align:
            same_result(lgr.align_prepared(a, b, params, descriptor=desc, metric_params=mparams),
                        lgr.align_ex2(s, t, params, descriptor=desc, mparams=mparams))
    return len(want)


@pytest.fixture(scope="module")
def pair():
    from lgr_amd import synthetic
    p = synthetic.make_pair(4000, 12)
    p["s"], p["t"] = cuda(p["src"]), cuda(p["tgt"])
    return p


def _kw(pair, **more):
    kw = dict(matching_id=0, feature_radius=0.25, bf_block_size=1500, distance_thr=0.1, max_iterations=5000, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    kw.update(more)
    return kw


def _single_cases(capi, pair):
    iss = dict(keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.03, iss_radius_tgt=0.03)
    return {
        "fpfh-lr": ("fpfh", dict(matching_id=capi.MATCH_LR), None),
        "fpfh-one_sided": ("fpfh", dict(matching_id=capi.MATCH_ONE_SIDED), None),
        "fpfh-cluster": ("fpfh", dict(matching_id=capi.MATCH_CLUSTER), None),
        "fpfh-flann": ("fpfh", dict(use_bfmatcher=0), None),
        "fpfh-guess": ("fpfh", dict(guess=pair["T_gt"], match_search_radius=0.5), None),
        "iss-shot-cluster": ("shot", dict(matching_id=capi.MATCH_CLUSTER, **iss), None),
        "rops-gravity": ("rops", dict(), None),
        "randomness2": ("fpfh", dict(randomness=2, iss_radius_src=0.02, iss_radius_tgt=0.03), None),
        "ratio": (capi.feature_params("fpfh", ratio_k=2), dict(matching_id=capi.MATCH_RATIO), None),
        "gror": ("fpfh", dict(alignment_id=capi.ALIGN_GROR), None),
        "closest_plane": ("fpfh", dict(metric_id=capi.METRIC_CLOSEST_PLANE), capi.metric_params()),
        "weighted_closest_plane": ("fpfh", dict(metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE), capi.metric_params("curvature")),
    }


SINGLE = ["fpfh-lr", "fpfh-one_sided", "fpfh-cluster", "fpfh-flann", "fpfh-guess", "iss-shot-cluster", "rops-gravity", "randomness2", "ratio", "gror",
          "closest_plane", "weighted_closest_plane"]


@pytest.mark.parametrize("case", SINGLE)
def test_single_scale_parity(lgr, pair, case):
    from lgr_amd import capi
    desc, more, mparams = _single_cases(capi, pair)[case]
    check_pair(lgr, pair["s"], pair["t"], capi.default_params(**_kw(pair, **more)), _desc(capi, desc), mparams, min_corr=5)


def test_pcl_arithmetic_parity(lgr, pair):
    from lgr_amd import capi
    lgr.set_options(arithmetic=capi.ARITH_PCL)
    try:
        p = capi.default_params(**_kw(pair))
        check_pair(lgr, pair["s"], pair["t"], p, "fpfh", min_corr=5)
        with lgr.prepare_cloud(pair["s"], p, 0) as a, lgr.prepare_cloud(pair["t"], p, 1) as b:
            lgr.set_options()     # the clouds were prepared under another arithmetic than the pair call's context has now
            out, n = lgr.empty((4000, 4), lgr.torch.int32), C.c_int(0)
            assert capi.lib().lgr_correspondences_prepared_dev(lgr.h, a.h, b.h, C.byref(p), None, capi._ptr(out), C.byref(n)) == capi.ERR_INVALID_ARG
    finally:
        lgr.set_options()


# ---- multi-scale
@pytest.fixture(scope="module")
def fixtures():
    import multiscale_ref_lib as M
    out = {name: M.fixture(name) for name in ("F1", "F2", "F3", "F4", "F5")}
    for p in out.values():
        p["s"], p["t"] = cuda(p["src"]), cuda(p["tgt"])
    return out


def _ms_kw(p, mid, block, kp, radii, **extra):
    return dict(feature_radius=0.0, matching_id=mid, bf_block_size=block, distance_thr=0.1, keypoint_id=int(kp == "iss"),
                iss_radius_src=radii[0], iss_radius_tgt=radii[1], max_iterations=2000, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"], **extra)


@pytest.mark.parametrize("fx,kp", list(CASES))
@pytest.mark.parametrize("desc", ["fpfh", "shot", "rops"])
def test_multiscale_parity(lgr, fixtures, desc, fx, kp):
    """the clouds are prepared once per (filter tables) and serve both block sizes; lgr_align_prepared on the large block"""
    from lgr_amd import capi
    p = fixtures[fx]
    d = _desc(capi, desc)
    for mid in (capi.MATCH_LR, capi.MATCH_ONE_SIDED, capi.MATCH_CLUSTER):
        prm = capi.default_params(**_ms_kw(p, mid, BLOCKS[0], kp, CASES[(fx, kp)]))
        with lgr.prepare_cloud(p["s"], prm, 0, d) as a, lgr.prepare_cloud(p["t"], prm, 1, d) as b:
            for block in BLOCKS:
                prm = capi.default_params(**_ms_kw(p, mid, block, kp, CASES[(fx, kp)]))
                want = raw(lgr.correspondences(p["s"], p["t"], prm, descriptor=d))
                got = raw(lgr.correspondences_prepared(a, b, prm, descriptor=d))
                assert got.shape == want.shape and (got == want).all(), (mid, block)
                if fx == "F3":
                    assert len(want) == 0      # no common level
                elif (desc, fx) != ("fpfh", "F5"):     # (FPFH on the exact lattices leaves at most 5 correspondences: parity only)
                    assert len(want) > 5, len(want)
            if mid == capi.MATCH_LR:
                same_result(lgr.align_prepared(a, b, prm, descriptor=d), lgr.align_ex2(p["s"], p["t"], prm, descriptor=d))


def test_multiscale_randomness_and_ratio(lgr, fixtures):
    from lgr_amd import capi
    p = fixtures["F1"]
    radii = CASES[("F1", "any")]
    check_pair(lgr, p["s"], p["t"], capi.default_params(**_ms_kw(p, capi.MATCH_LR, 2500, "any", radii, randomness=2)), "fpfh", min_corr=5)
    check_pair(lgr, p["s"], p["t"], capi.default_params(**_ms_kw(p, capi.MATCH_RATIO, 2500, "any", radii)), capi.feature_params("fpfh", ratio_k=2),
               min_corr=5)


# ---- reuse
def _snapshot(cloud):
    return [cloud.keypoints().tobytes()] + [x.tobytes() for i in range(cloud.info().levels) for x in cloud.level(i)[1:]] + [cloud.info().bytes]


@pytest.mark.parametrize("radius", [0.25, 0.0])
def test_reuse(lgr, pair, radius):
    """A, B: the two clouds of one pair, C: the source of another seed.  Neither side has a view point, so every cloud serves on both sides."""
    from lgr_amd import capi, synthetic
    clouds = [pair["s"], pair["t"], cuda(synthetic.make_pair(4000, 13)["src"])]
    p = capi.default_params(matching_id=capi.MATCH_CLUSTER, feature_radius=radius, bf_block_size=1500, distance_thr=0.1, max_iterations=2000,
                            iss_radius_src=0.05, iss_radius_tgt=0.05)
    prepared = [lgr.prepare_cloud(c, p, side) for c, side in zip(clouds, (0, 1, 0))]
    try:
        before = [_snapshot(c) for c in prepared]
        for i, j in [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (0, 0)]:
            want = raw(lgr.correspondences(clouds[i], clouds[j], p))
            got = raw(lgr.correspondences_prepared(prepared[i], prepared[j], p))
            assert got.shape == want.shape and (got == want).all(), (i, j)
            assert len(want) > 5 or i != j
            same_result(lgr.align_prepared(prepared[i], prepared[j], p), lgr.align_ex2(clouds[i], clouds[j], p))
        assert [_snapshot(c) for c in prepared] == before
    finally:
        for c in prepared:
            c.close()


# ---- getters
@pytest.mark.parametrize("fx", ["F1", "F2", "F4"])
@pytest.mark.parametrize("kp", ["any", "iss"])
@pytest.mark.parametrize("desc", ["fpfh", "shot", "rops"])
def test_getters_equal_the_statement(lgr, oracle, fixtures, desc, kp, fx):
    import multiscale_ref_lib as M
    from lgr_amd import capi
    p = fixtures[fx]
    st = M.Statement(oracle, p["src"], p["tgt"], desc, kp, iss_radius=CASES[(fx, kp)], vp=(p["vp_src"], p["vp_tgt"]))
    prm = capi.default_params(**_ms_kw(p, capi.MATCH_LR, BLOCKS[0], kp, CASES[(fx, kp)]))
    for s, cloud in enumerate((p["s"], p["t"])):
        side = st.sides[s]
        with lgr.prepare_cloud(cloud, prm, s, _desc(capi, desc)) as c:
            info = c.info()
            assert (info.n, info.keypoints, info.row_len, info.multiscale) == (cloud.shape[0], len(side.kps), M.ADAPTERS[desc].dim, 1)
            assert (info.first_log2_radius, info.levels) == (side.min_l2, side.max_l2 - side.min_l2 + 1)
            want_kidx = st.kidx[s] if st.kidx[s] is not None else np.arange(cloud.shape[0])
            np.testing.assert_array_equal(c.keypoints(), want_kidx)
            for i, li in enumerate(c.levels()):
                li2, lst, rows = c.level(i)
                assert (li.log2_radius, li.rows, li.surface) == (side.min_l2 + i, len(side.lists[i]), len(side.surf[i])) == (li2.log2_radius, li2.rows, li2.surface)
                assert (bits(li.radius), bits(li.voxel)) == (bits(side.radius[i]), bits(side.voxel[i]))
                np.testing.assert_array_equal(lst, side.lists[i])
                np.testing.assert_array_equal(bits(rows), bits(side.rows[i]))     # NaN rows: equal by their bits


@pytest.mark.parametrize("desc", ["fpfh", "shot", "rops"])
def test_single_scale_getters_equal_the_public_stages(lgr, pair, desc):
    from lgr_amd import capi
    radius = np.float32(0.25)
    voxel = np.sqrt(np.float32(np.pi * float(radius) * float(radius) / 352.0))
    prm = capi.default_params(**_kw(pair))
    for s, (cloud, vp) in enumerate(((pair["s"], pair["vp_src"]), (pair["t"], pair["vp_tgt"]))):
        surf = lgr.downsample(cloud, float(voxel)).contiguous()
        lgr.normals_knn(surf, 30, vp=vp)
        if desc == "fpfh":
            want = lgr.fpfh(cloud, surf, float(radius))
        elif desc == "shot":
            want = lgr.shot(cloud, surf, float(radius))
        else:   # include/matching.h:243-246: the key points' normals re-estimated on the surface
            kn = cloud.clone()
            v = (C.c_float * 3)(*[float(x) for x in vp])
            lgr.check(capi.lib().lgr_normals_knn_dev(lgr.h, capi._ptr(kn), kn.shape[0], capi._ptr(surf), surf.shape[0], 30, v, 1))
            want = lgr.rops(kn, surf, float(radius), lgr.gravity_lrf(kn, surf, float(radius)))
        with lgr.prepare_cloud(cloud, prm, s, _desc(capi, desc)) as c:
            info = c.info()
            assert (info.levels, info.multiscale, info.keypoints, info.first_log2_radius) == (1, 0, cloud.shape[0], -2)
            li, lst, rows = c.level(0)
            assert (li.rows, li.surface, float(li.radius)) == (cloud.shape[0], surf.shape[0], 0.25) and bits(li.voxel) == bits(voxel)
            np.testing.assert_array_equal(lst, np.arange(cloud.shape[0]))
            np.testing.assert_array_equal(c.keypoints(), np.arange(cloud.shape[0]))
            np.testing.assert_array_equal(bits(rows), bits(want.cpu().numpy()))


# ---- the reference's tests/keypoint_extraction.cpp
@pytest.mark.parametrize("desc", ["shot", "fpfh"])
def test_keypoint_extraction_property(lgr, pair, desc):
    """SHOT as in the reference's test, and FPFH.  (RoPS re-estimates the key points' normals per level from the key-point copy.)"""
    from lgr_amd import capi
    base = _kw(pair, iss_radius_src=0.05)
    with lgr.prepare_cloud(pair["s"], capi.default_params(keypoint_id=capi.KEYPOINT_ISS, **base), 0, desc) as iss, \
            lgr.prepare_cloud(pair["s"], capi.default_params(keypoint_id=capi.KEYPOINT_ANY, **base), 0, desc) as every:
        kidx = iss.keypoints()
        assert 20 <= len(kidx) < 2000
        np.testing.assert_array_equal(bits(iss.level(0)[2]), bits(every.level(0)[2][kidx]))


# ---- contract
def test_contract(lgr, pair):
    from lgr_amd import capi
    lib = capi.lib()
    out, n, res = lgr.empty((4000, 4), lgr.torch.int32), C.c_int(0), capi.Result()
    iss = dict(keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.05, iss_radius_tgt=0.05)
    p = capi.default_params(**_kw(pair, **iss))
    f = capi.feature_params("fpfh")

    def corr(a, b, prm, fp=f):
        return lib.lgr_correspondences_prepared_dev(lgr.h, a.h if a else None, b.h if b else None, C.byref(prm) if prm else None,
                                                    C.byref(fp) if fp else None, capi._ptr(out), C.byref(n))

    def align(a, b, prm, fp=f):
        return lib.lgr_align_prepared(lgr.h, a.h if a else None, b.h if b else None, C.byref(prm) if prm else None, C.byref(fp) if fp else None, None,
                                      C.byref(res))

    with lgr.prepare_cloud(pair["s"], p, 0) as a, lgr.prepare_cloud(pair["t"], p, 1) as b:
        assert corr(a, b, p) == 0 and align(a, b, p) == 0
        assert corr(a, b, p, None) == 0                                # a NULL struct is FPFH
        other_vp = np.asarray(pair["vp_src"], np.float32) + np.float32(1)
        for more in (dict(normal_nr_points=20), dict(vp_src=other_vp), dict(iss_radius_src=0.06), dict(iss_radius_tgt=0.06), dict(feature_nr_points=300),
                     dict(scale_factor=3.0), dict(normals_available=1), dict(keypoint_id=capi.KEYPOINT_ANY), dict(matching_id=capi.MATCH_CLUSTER),
                     dict(feature_radius=0.0)):
            q = capi.default_params(**_kw(pair, **dict(iss, **more)))
            assert corr(a, b, q) == capi.ERR_INVALID_ARG, more
            assert align(a, b, q) == capi.ERR_INVALID_ARG, more
        assert corr(a, b, p, capi.feature_params("shot")) == capi.ERR_INVALID_ARG      # another descriptor
        assert corr(b, a, p) == capi.ERR_INVALID_ARG                                    # the sides' view points differ
        # what the fingerprint leaves out may change from pair to pair
        assert corr(a, b, capi.default_params(**_kw(pair, **dict(iss, bf_block_size=700, distance_thr=0.2, matching_id=capi.MATCH_ONE_SIDED)))) == 0
        for args in ((None, b, p), (a, None, p), (a, b, None)):
            assert corr(*args) == capi.ERR_INVALID_ARG and align(*args) == capi.ERR_INVALID_ARG
        assert lib.lgr_correspondences_prepared_dev(lgr.h, a.h, b.h, C.byref(p), C.byref(f), capi._ptr(out), None) == capi.ERR_INVALID_ARG
        assert lib.lgr_align_prepared(lgr.h, a.h, b.h, C.byref(p), C.byref(f), None, None) == capi.ERR_INVALID_ARG
        assert lib.lgr_correspondences_prepared_dev(None, a.h, b.h, C.byref(p), C.byref(f), capi._ptr(out), C.byref(n)) == capi.ERR_INVALID_ARG
        assert align(a, b, capi.default_params(**_kw(pair, **dict(iss, n_samples=9)))) == capi.ERR_UNSUPPORTED
    h = C.c_void_p()
    assert lib.lgr_cloud_prepare_dev(lgr.h, capi._ptr(pair["s"]), 4000, 2, C.byref(p), C.byref(f), C.byref(h)) == capi.ERR_INVALID_ARG
    assert lib.lgr_cloud_prepare_dev(lgr.h, None, 4000, 0, C.byref(p), C.byref(f), C.byref(h)) == capi.ERR_INVALID_ARG
    assert lib.lgr_cloud_prepare_dev(lgr.h, capi._ptr(pair["s"]), 4000, 0, None, C.byref(f), C.byref(h)) == capi.ERR_INVALID_ARG
    assert lib.lgr_cloud_prepare_dev(lgr.h, capi._ptr(pair["s"]), 4000, 0, C.byref(p), C.byref(f), None) == capi.ERR_INVALID_ARG
    assert not h.value


def test_unsupported_combinations_keep_their_code(lgr, pair):
    """the pinned cases of test_gpu_align_shot.py / test_gpu_align_rops.py, from lgr_cloud_prepare_dev"""
    from lgr_amd import capi
    lib = capi.lib()
    base = dict(bf_block_size=200000, max_iterations=100, distance_thr=0.1)
    g = capi.LRF_GRAVITY
    cases = [(capi.default_params(**base), capi.feature_params("rops", lrf_id=capi.LRF_DEFAULT), capi.ERR_UNSUPPORTED),
             (capi.default_params(**base), capi.feature_params("rops", lrf_id=capi.LRF_GT), capi.ERR_UNSUPPORTED),
             (capi.default_params(use_bfmatcher=0, **base), capi.feature_params("rops", lrf_id=g), capi.ERR_UNSUPPORTED),
             (capi.default_params(guess=np.eye(4), match_search_radius=1.0, **base), capi.feature_params("rops", lrf_id=g), capi.ERR_UNSUPPORTED),
             (capi.default_params(**base), capi.feature_params("rops", lrf_id=3), capi.ERR_INVALID_ARG),
             (capi.default_params(use_bfmatcher=0, **base), capi.feature_params("shot"), capi.ERR_UNSUPPORTED),
             (capi.default_params(guess=np.eye(4), match_search_radius=1.0, **base), capi.feature_params("shot"), capi.ERR_UNSUPPORTED),
             (capi.default_params(**base), capi.feature_params("shot", lrf_id=g), capi.ERR_UNSUPPORTED),
             (capi.default_params(randomness=9, **base), capi.feature_params("fpfh"), capi.ERR_UNSUPPORTED),
             (capi.default_params(keypoint_id=7, **base), capi.feature_params("fpfh"), capi.ERR_UNSUPPORTED)]
    out, n, h = lgr.empty((4000, 4), lgr.torch.int32), C.c_int(0), C.c_void_p()
    for p, f, code in cases:
        assert lib.lgr_correspondences_ex_dev(lgr.h, capi._ptr(pair["s"]), 4000, capi._ptr(pair["t"]), 4000, C.byref(p), C.byref(f), capi._ptr(out), C.byref(n)) == code
        assert lib.lgr_cloud_prepare_dev(lgr.h, capi._ptr(pair["s"]), 4000, 0, C.byref(p), C.byref(f), C.byref(h)) == code
        assert not h.value
    # ... and from the pair call, on clouds that were prepared for something the pair's parameters are not
    p = capi.default_params(**_kw(pair))
    with lgr.prepare_cloud(pair["s"], p, 0) as a, lgr.prepare_cloud(pair["t"], p, 1) as b:
        for q, f, code in cases:
            assert lib.lgr_correspondences_prepared_dev(lgr.h, a.h, b.h, C.byref(q), C.byref(f), capi._ptr(out), C.byref(n)) == code
    lgr.set_options(arithmetic=capi.ARITH_PCL)
    try:
        for d in ("shot", "rops"):
            f = _desc(capi, d)
            assert lib.lgr_cloud_prepare_dev(lgr.h, capi._ptr(pair["s"]), 4000, 0, C.byref(p), C.byref(f), C.byref(h)) == capi.ERR_UNSUPPORTED
    finally:
        lgr.set_options()


def test_clouds_without_two_points(lgr, pair):
    from lgr_amd import capi
    p = capi.default_params(**_kw(pair))
    with lgr.prepare_cloud(pair["s"][:1].contiguous(), p, 0) as one, lgr.prepare_cloud(pair["s"][:0].contiguous(), p, 0) as none, \
            lgr.prepare_cloud(pair["t"], p, 1) as b:
        assert (one.info().n, one.info().keypoints, one.info().levels) == (1, 0, 0) and none.info().n == 0
        assert len(one.keypoints()) == 0
        for a in (one, none):
            assert len(lgr.correspondences_prepared(a, b, p)) == 0
            res = lgr.align_prepared(a, b, p)
            assert res.converged == 0 and res.n_correspondences == 0
            np.testing.assert_array_equal(res.matrix(), np.eye(4, dtype=np.float32))
