"""-m gpu: SHOT through the whole correspondence search and alignment (lgr_align_ex*, lgr_correspondences_ex*).

- The reference's end-to-end test tests/point2plane_distance.cpp WITHOUT the substitution of test_gpu_reference_acceptance.py: the corner
  scene with the struct-default descriptor SHOT, multi-scale matching, the cluster filter, the closest-plane metric, fix_seed; the three
  bounds of :94-96 evaluated in float64 independently of the library.
- Single scale, lr and cluster: device SHOT rows -> the CPU reference matcher -> oracle.filter_matches -> oracle.ransac equals
  lgr_align_ex_dev's correspondences and result bit for bit.
- Two runs are identical; GROR runs behind SHOT; single-scale SHOT with ISS key points runs; the combinations that are not built
  return LGR_ERR_UNSUPPORTED; lgr_align_ex(NULL) and lgr_correspondences_ex_dev(NULL) are lgr_align / lgr_correspondences_dev."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_reference_acceptance import acceptance, corner_scene, reference_params  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(lgr):
    import torch
    src, tgt, vp_src, vp_tgt = corner_scene()
    src_n = lgr.normals_knn(torch.from_numpy(src).cuda(), 30, vp=vp_src)
    tgt_n = lgr.normals_knn(torch.from_numpy(tgt).cuda(), 30, vp=vp_tgt)
    lgr.sync()
    return dict(src=src_n, tgt=tgt_n, src_h=src_n.cpu().numpy(), tgt_h=tgt_n.cpu().numpy(), vp_src=vp_src, vp_tgt=vp_tgt)


def test_reference_acceptance_point2plane_shot(lgr, scene):
    from lgr_amd import capi
    p = reference_params(capi, scene["vp_src"], scene["vp_tgt"])
    res = lgr.align(scene["src"], scene["tgt"], p, descriptor="shot")
    T = res.matrix()
    thr = lgr.cloud_density(scene["tgt"])
    ratio, error, overlap = acceptance(scene["src_h"], scene["tgt_h"], T, thr)
    print(f"SHOT corner scene: {res.n_correspondences} correspondences, inlier ratio {ratio}, error {error}, overlap {overlap}, "
          f"stage ms {list(res.stage_ms)[:7]}")
    assert res.converged == 1
    assert abs(ratio - 1.0) <= 1e-5, ratio
    assert error < 2.0 / 3.0, error
    assert overlap < 0.72, overlap
    res2 = lgr.align(scene["src"], scene["tgt"], p, descriptor="shot")   # determinism
    skip = capi.Result.time_cs.offset                       # the wall times and stage timers are measurements
    assert bytes(res2)[:skip] == bytes(res)[:skip]


def _pair(n=20000, seed=21):
    import torch
    from lgr_amd import synthetic
    pair = synthetic.make_pair(n, seed=seed)
    return pair, torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()


def test_single_scale_filters_and_gror(lgr):
    from lgr_amd import capi
    pair, s, t = _pair()
    for mid in (capi.MATCH_LR, capi.MATCH_CLUSTER, capi.MATCH_ONE_SIDED):
        p = capi.default_params(matching_id=mid, bf_block_size=200000, max_iterations=5000, distance_thr=0.1,
                                vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
        c1 = lgr.correspondences(s, t, p, descriptor="shot").cpu().numpy()
        c2 = lgr.correspondences(s, t, p, descriptor="shot").cpu().numpy()
        assert len(c1) > 0 and (c1 == c2).all()
        c_f = lgr.correspondences(s, t, p).cpu().numpy()
        assert c1.shape != c_f.shape or (c1 != c_f).any()    # a different descriptor gives different correspondences
    p = capi.default_params(alignment_id=capi.ALIGN_GROR, bf_block_size=200000, distance_thr=0.1,
                            vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    r = lgr.align(s, t, p, descriptor="shot")
    assert r.converged == 1 and r.n_correspondences > 0
    p = capi.default_params(keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06, iss_radius_tgt=0.06, bf_block_size=200000,
                            max_iterations=5000, distance_thr=0.1, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    r = lgr.align(s, t, p, descriptor="shot")
    assert r.n_correspondences >= 0 and r.stage_ms[2] > 0


@pytest.mark.parametrize("matching", ["lr", "cluster"])
def test_single_scale_parity_with_the_reference_pieces(lgr, oracle, matching):
    """Device SHOT rows -> tests/cpp/shot_ref.cpp's matcher -> oracle.filter_matches -> oracle.ransac equals lgr_align_ex_dev's
    correspondences and result bit for bit (single scale, keypoint any).  The surface of the descriptor stage is the device's own
    down-sampling and normals (each pinned against the oracle elsewhere); what this pins is the SHOT glue of the correspondence search:
    row stride, descriptor stage, matcher routing."""
    import torch
    from lgr_amd import capi
    import shot_ref_lib as ref
    mid = capi.MATCH_LR if matching == "lr" else capi.MATCH_CLUSTER
    pair, s, t = _pair(10000, seed=5)
    kw = dict(matching_id=mid, feature_radius=0.25, bf_block_size=4096, max_iterations=20000, distance_thr=0.1,
              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    p = capi.default_params(**kw)
    # include/matching.h:172,230-231 with feature_radius 0.25, scale_factor 2: search radius 2^-2, voxel sqrtf(pi r^2 / 352)
    radius = np.float32(0.25)
    voxel = np.sqrt(np.float32(np.pi * float(radius) * float(radius) / 352.0))
    rows = []
    for cloud, vp in ((s, pair["vp_src"]), (t, pair["vp_tgt"])):
        surf = lgr.downsample(cloud, float(voxel)).contiguous()
        lgr.normals_knn(surf, 30, vp=vp)
        rows.append(lgr.shot(cloud, surf, float(radius)).cpu().numpy())
    ij, dij = ref.match(rows[0], rows[1], 4096)
    ji, dji = ref.match(rows[1], rows[0], 4096)
    want = oracle.filter_matches(mid, pair["src"], pair["tgt"], ij, dij, ji, dji, 0.1, 40)
    got = lgr.correspondences(s, t, p, descriptor="shot").cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
    assert len(got) == len(want) > 20
    np.testing.assert_array_equal(got["index_query"], want["query"])
    np.testing.assert_array_equal(got["index_match"], want["match"])
    np.testing.assert_array_equal(got["distance"].view(np.uint32), want["distance"].view(np.uint32))
    np.testing.assert_array_equal(got["threshold"].view(np.uint32), want["threshold"].view(np.uint32))
    ores, _ = oracle.ransac(pair["src"], pair["tgt"], want, oracle.default_params(rng_mode=oracle.RNG_PHILOX, **kw))
    res = lgr.align(s, t, p, descriptor="shot")
    assert res.n_correspondences == len(want)
    assert (res.iterations, res.n_inliers, res.best_iteration, res.converged) == (ores.iterations, ores.n_inliers, ores.best_iteration, ores.converged)
    np.testing.assert_array_equal(res.matrix().view(np.uint32), ores.matrix().view(np.uint32))


def test_unsupported_combinations(lgr):
    from lgr_amd import capi
    lib = capi.lib()
    pair, s, t = _pair(4000)
    res = capi.Result()
    out = lgr.empty((4000, 4), lgr.torch.int32)
    n = C.c_int(0)
    base = dict(bf_block_size=200000, max_iterations=100, distance_thr=0.1)
    cases = [(capi.default_params(use_bfmatcher=0, **base), capi.feature_params("shot")),
             (capi.default_params(guess=np.eye(4), match_search_radius=1.0, **base), capi.feature_params("shot")),
             (capi.default_params(**base), capi.feature_params("shot", lrf_id=1)),
             (capi.default_params(**base), capi.feature_params(7))]
    for p, f in cases:
        assert lib.lgr_align_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), C.byref(res)) == capi.ERR_UNSUPPORTED
        assert lib.lgr_correspondences_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), capi._ptr(out),
                                              C.byref(n)) == capi.ERR_UNSUPPORTED
    lgr.set_options(arithmetic=1)
    try:
        p, f = capi.default_params(**base), capi.feature_params("shot")
        assert lib.lgr_align_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), C.byref(res)) == capi.ERR_UNSUPPORTED
    finally:
        lgr.set_options()


def test_ex_null_is_the_fpfh_path(lgr):
    from lgr_amd import capi
    lib = capi.lib()
    pair, s, t = _pair(8000, seed=5)
    p = capi.default_params(matching_id=0, bf_block_size=200000, max_iterations=20000, distance_thr=0.1,
                            vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    src, tgt = pair["src"], pair["tgt"]
    a, b = capi.Result(), capi.Result()
    assert lib.lgr_align(lgr.h, capi._ptr(src), len(src), capi._ptr(tgt), len(tgt), C.byref(p), C.byref(a)) == 0
    assert lib.lgr_align_ex(lgr.h, capi._ptr(src), len(src), capi._ptr(tgt), len(tgt), C.byref(p), None, C.byref(b)) == 0
    skip = capi.Result.time_cs.offset   # the wall times and stage timers are measurements, everything before them must be equal
    assert bytes(a)[:skip] == bytes(b)[:skip]
    f = capi.feature_params("fpfh")
    c1 = lgr.correspondences(s, t, p).cpu().numpy()
    c2 = lgr.correspondences(s, t, p, descriptor=f).cpu().numpy()
    assert (c1 == c2).all()
    # FPFH never reads the frames (include/common.h:366,407): a gravity frame id changes nothing there
    c3 = lgr.correspondences(s, t, p, descriptor=capi.feature_params("fpfh", lrf_id=1)).cpu().numpy()
    assert (c1 == c3).all()
