"""-m gpu: RoPS on gravity frames through the whole correspondence search and alignment (lgr_align_ex*, lgr_correspondences_ex*).

- Single scale, lr / one_sided / cluster: device RoPS rows (gravity frames) -> tests/cpp/rops_ref.cpp's matcher -> oracle.filter_matches
  -> oracle.ransac equals lgr_align_ex_dev's correspondences and result bit for bit.
- Multi-scale and ISS key points run, GROR runs behind RoPS, two runs are identical.
- A generator pair moved by a pure yaw registers with rops + gravity (rotation and translation errors against stated bounds).
- Every combination that is not built returns its status code."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _pair(n=20000, seed=21, **kw):
    import torch
    from lgr_amd import synthetic
    pair = synthetic.make_pair(n, seed=seed, **kw)
    return pair, torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()


@pytest.mark.parametrize("matching", ["lr", "one_sided", "cluster"])
def test_single_scale_parity_with_the_reference_pieces(lgr, oracle, matching):
    import torch
    from lgr_amd import capi
    import rops_ref_lib as ref
    mid = {"lr": capi.MATCH_LR, "one_sided": capi.MATCH_ONE_SIDED, "cluster": capi.MATCH_CLUSTER}[matching]
    pair, s, t = _pair(10000, seed=5)
    kw = dict(matching_id=mid, feature_radius=0.25, bf_block_size=4096, max_iterations=20000, distance_thr=0.1,
              vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    p = capi.default_params(**kw)
    radius = np.float32(0.25)
    voxel = np.sqrt(np.float32(np.pi * float(radius) * float(radius) / 352.0))
    rows = []
    for cloud, vp in ((s, pair["vp_src"]), (t, pair["vp_tgt"])):
        surf = lgr.downsample(cloud, float(voxel)).contiguous()
        lgr.normals_knn(surf, 30, vp=vp)
        # include/matching.h:243-246: the key points' normals re-estimated on the surface (normals_available = true)
        kn = cloud.clone()
        v = (C.c_float * 3)(*[float(x) for x in vp])
        lgr.check(capi.lib().lgr_normals_knn_dev(lgr.h, capi._ptr(kn), kn.shape[0], capi._ptr(surf), surf.shape[0], 30, v, 1))
        fr = lgr.gravity_lrf(kn, surf, float(radius))
        rows.append(lgr.rops(kn, surf, float(radius), fr).cpu().numpy())
    ij, dij = ref.match(rows[0], rows[1], 4096)
    ji, dji = ref.match(rows[1], rows[0], 4096)
    want = oracle.filter_matches(mid, pair["src"], pair["tgt"], ij, dij, ji, dji, 0.1, 40)
    f = capi.feature_params("rops", lrf_id=capi.LRF_GRAVITY)
    got = lgr.correspondences(s, t, p, descriptor=f).cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
    assert len(got) == len(want) > 20
    np.testing.assert_array_equal(got["index_query"], want["query"])
    np.testing.assert_array_equal(got["index_match"], want["match"])
    np.testing.assert_array_equal(got["distance"].view(np.uint32), want["distance"].view(np.uint32))
    np.testing.assert_array_equal(got["threshold"].view(np.uint32), want["threshold"].view(np.uint32))
    ores, _ = oracle.ransac(pair["src"], pair["tgt"], want, oracle.default_params(rng_mode=oracle.RNG_PHILOX, **kw))
    res = lgr.align(s, t, p, descriptor="rops")
    assert res.n_correspondences == len(want)
    assert (res.iterations, res.n_inliers, res.best_iteration, res.converged) == (ores.iterations, ores.n_inliers, ores.best_iteration, ores.converged)
    np.testing.assert_array_equal(res.matrix().view(np.uint32), ores.matrix().view(np.uint32))


def test_multiscale_iss_gror_and_determinism(lgr):
    from lgr_amd import capi
    pair, s, t = _pair()
    base = dict(bf_block_size=200000, max_iterations=5000, distance_thr=0.1, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    p = capi.default_params(matching_id=capi.MATCH_CLUSTER, **base)           # feature_radius unset: multi-scale
    c1 = lgr.correspondences(s, t, p, descriptor="rops").cpu().numpy()
    c2 = lgr.correspondences(s, t, p, descriptor="rops").cpu().numpy()
    assert len(c1) > 0 and (c1 == c2).all()
    c_s = lgr.correspondences(s, t, p, descriptor="shot").cpu().numpy()
    assert c1.shape != c_s.shape or (c1 != c_s).any()
    r = lgr.align(s, t, capi.default_params(alignment_id=capi.ALIGN_GROR, **dict(base, max_iterations=100)), descriptor="rops")
    assert r.n_correspondences > 0
    p = capi.default_params(keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06, iss_radius_tgt=0.06, **base)
    r = lgr.align(s, t, p, descriptor="rops")
    r2 = lgr.align(s, t, p, descriptor="rops")
    assert r.n_correspondences >= 0 and r.stage_ms[2] > 0
    skip = capi.Result.time_cs.offset
    assert bytes(r)[:skip] == bytes(r2)[:skip]
    p = capi.default_params(keypoint_id=capi.KEYPOINT_ISS, iss_radius_src=0.06, iss_radius_tgt=0.06, feature_radius=0.25, **base)
    assert lgr.align(s, t, p, descriptor="rops").n_correspondences > 0


def _errors(T, G):
    R = T[:3, :3].astype(np.float64) @ G[:3, :3].T
    rot = float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))
    return rot, float(np.linalg.norm(T[:3, 3] - G[:3, 3]))


def test_yaw_only_pair_registers(lgr):
    from lgr_amd import capi
    pair, s, t = _pair(100_000, seed=8, yaw_only=True)
    G = pair["T_gt"]
    assert abs(G[2, 2] - 1) < 1e-12
    p = capi.default_params(matching_id=capi.MATCH_LR, feature_radius=0.25, bf_block_size=200000, max_iterations=100000,
                            distance_thr=0.05, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    res = lgr.align(s, t, p, descriptor=capi.feature_params("rops", lrf_id=capi.LRF_GRAVITY))
    rot, tr = _errors(res.matrix(), G)
    print(f"yaw-only pair, rops + gravity: {res.n_correspondences} correspondences, {res.n_inliers} inliers, "
          f"rotation error {rot:.4f} deg, translation error {tr:.4f} m, stage ms {list(res.stage_ms)[:7]}")
    assert res.converged == 1
    assert rot < 1.0 and tr < 0.05


def test_unsupported_combinations(lgr):
    from lgr_amd import capi
    lib = capi.lib()
    pair, s, t = _pair(4000)
    res = capi.Result()
    out = lgr.empty((4000, 4), lgr.torch.int32)
    n = C.c_int(0)
    base = dict(bf_block_size=200000, max_iterations=100, distance_thr=0.1)
    g = capi.LRF_GRAVITY
    cases = [(capi.default_params(**base), capi.feature_params("rops", lrf_id=capi.LRF_DEFAULT), capi.ERR_UNSUPPORTED),
             (capi.default_params(**base), capi.feature_params("rops", lrf_id=capi.LRF_GT), capi.ERR_UNSUPPORTED),
             (capi.default_params(use_bfmatcher=0, **base), capi.feature_params("rops", lrf_id=g), capi.ERR_UNSUPPORTED),
             (capi.default_params(guess=np.eye(4), match_search_radius=1.0, **base), capi.feature_params("rops", lrf_id=g), capi.ERR_UNSUPPORTED),
             (capi.default_params(**base), capi.feature_params("rops", lrf_id=3), -1),
             (capi.default_params(**base), capi.feature_params("rops", lrf_id=-1), -1)]
    for p, f, code in cases:
        rc = lib.lgr_align_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), C.byref(res))
        rc2 = lib.lgr_correspondences_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), capi._ptr(out), C.byref(n))
        assert rc == code and rc2 == code   # -1: LGR_ERR_INVALID_ARG
    lgr.set_options(arithmetic=1)
    try:
        p, f = capi.default_params(**base), capi.feature_params("rops", lrf_id=g)
        assert lib.lgr_align_ex_dev(lgr.h, capi._ptr(s), 4000, capi._ptr(t), 4000, C.byref(p), C.byref(f), C.byref(res)) == capi.ERR_UNSUPPORTED
    finally:
        lgr.set_options()
