"""GPU: the dense closest-plane evaluation (lgr_evaluate_plane_dense*, lgr_analysis_metric*) against the CPU statement
tests/cpp/plane_dense_ref.cpp: every float bit for bit (compared as uint32), every inlier list, nearest-target array and count equal.
Cases: a transform near the ground truth (four scores, threshold computed and passed in, outputs present and absent, host twin), one far
from it, a lattice whose queries all have two equidistant nearest targets with different normals, source sizes around the wave and
workgroup edges, non-finite points and normals, point weights, agreement with the sparse evaluation, the analysis figures of all five
metrics, and the reference's own acceptance conditions (tests/point2plane_distance.cpp:88-96) on the corner scene."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_dense_ref_lib as P  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
SEED = 12   # make_pair(4000, 12) at perturbed(): the statement on the oracle's normals counts 1982 inliers of 4000 (chosen on the CPU)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(v):
    return int(np.asarray(v, F).view(np.uint32))


def check(dev, ref, with_inliers=True, with_nn=True):
    """dev: capi.PlaneDenseEval, ref: plane_dense_ref_lib.evaluate"""
    assert dev.n_inliers == ref["n_inliers"], (dev.n_inliers, ref["n_inliers"])
    for f in ("rmse", "metric", "threshold", "score"):
        assert bits(getattr(dev, f)) == bits(ref[f]), (f, getattr(dev, f), ref[f])
    assert list(dev.reserved) == [0, 0, 0]
    if with_inliers:
        assert dev.inliers.shape == ref["inliers"].shape and np.array_equal(dev.inliers.view(np.uint32), ref["inliers"].view(np.uint32))
    if with_nn:
        assert np.array_equal(dev.nn, ref["nn"])


def perturbed(T_gt, thr):
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    return (dT @ T_gt).astype(F)


@pytest.fixture(scope="module")
def pair(lgr):
    """make_pair(4000, SEED), normals from lgr_normals_knn, thr = the target's density (what the entry computes itself), T a small
    perturbation of the ground truth, correspondences from lgr_correspondences (one-sided matching at distance_thr = 2 thr)"""
    from lgr_amd import capi, synthetic
    p = synthetic.make_pair(n_points=4000, seed=SEED)
    out = dict(T_gt=p["T_gt"].astype(F))
    for side in ("src", "tgt"):
        d = cuda(p[side])
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        out[side] = d.cpu().numpy()
    thr = float(F(lgr.cloud_density(cuda(out["tgt"]))))
    params = capi.default_params(matching_id=capi.MATCH_ONE_SIDED, bf_block_size=200000, distance_thr=2 * thr, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"])
    corr = lgr.correspondences(cuda(out["src"]), cuda(out["tgt"]), params).cpu().numpy().view(P.CORR_DTYPE).reshape(-1)
    out.update(thr=thr, corr=corr, T=perturbed(p["T_gt"], thr), T_far=synthetic.random_se3(np.random.default_rng(5)).astype(F))
    return out


@pytest.mark.parametrize("score_id", [0, 1, 2, 3])
def test_near_ground_truth(lgr, pair, score_id):
    src, tgt, T, thr = (pair[k] for k in ("src", "tgt", "T", "thr"))
    ns = len(src)
    ref = P.evaluate(src, tgt, T, score_id, thr)
    assert ns // 10 <= ref["n_inliers"] <= 9 * ns // 10   # not vacuous
    d_src, d_tgt = cuda(src), cuda(tgt)
    dev = lgr.evaluate_plane_dense(d_src, d_tgt, T, score_id, with_inliers=True, with_nn=True)        # threshold computed
    check(dev, ref)
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, score_id, threshold=dev.threshold, with_inliers=True, with_nn=True), ref)   # passed in
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, score_id), ref, False, False)                      # neither output
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, score_id, with_inliers=True), ref, True, False)
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, score_id, threshold=thr, with_nn=True), ref, False, True)
    check(lgr.evaluate_plane_dense_host(src, tgt, T, score_id, with_inliers=True, with_nn=True), ref)  # the host twin
    check(lgr.evaluate_plane_dense_host(src, tgt, T, score_id, threshold=thr), ref, False, False)
    # another threshold is another result, against the statement at that threshold
    thr2 = float(F(0.5 * thr))
    ref2 = P.evaluate(src, tgt, T, score_id, thr2)
    assert 0 < ref2["n_inliers"] < ref["n_inliers"]
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, score_id, threshold=thr2, with_inliers=True, with_nn=True), ref2)


def test_far_from_ground_truth(lgr, pair):
    src, tgt, thr = (pair[k] for k in ("src", "tgt", "thr"))
    ref = P.evaluate(src, tgt, pair["T_far"], 2, thr)
    dev = lgr.evaluate_plane_dense(cuda(src), cuda(tgt), pair["T_far"], 2, with_inliers=True, with_nn=True)
    check(dev, ref)
    assert dev.n_inliers == 0 and dev.rmse == FLT_MAX and dev.metric == 0 and len(dev.inliers) == 0 and (dev.nn == -1).all()


def lattice(n=12):
    """source on the integer lattice n^3 (index = (x n + y) n + z), the target the same lattice shifted by exactly 0.5 along x.  The normals
    alternate with x between (0,0,1) and (1,0,0)."""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(F)
    nrm = np.where((g[:, :1] % 2) == 0, np.array([[0, 0, 1]], F), np.array([[1, 0, 0]], F))
    src = np.zeros((len(g), 12), F)
    src[:, :3] = g; src[:, 3] = 1; src[:, 4:7] = nrm; src[:, 8] = 1
    tgt = src.copy()
    tgt[:, 0] += 0.5
    return src, tgt


@pytest.mark.parametrize("score_id", [0, 2])
def test_ties_lower_index_wins(lgr, score_id):
    """The transform turns the lattice by 0.04 rad about the x axis and shifts it in y and z: a moved point keeps its x EXACTLY (row 0 of T
    is (1, 0, 0, 0)), so a source point with x >= 1 has two nearest targets at equal squared distance, x - 0.5 (the lower index) and
    x + 0.5, whose normals differ.  Along (1,0,0) the plane distance is 0.5, along (0,0,1) it is the z displacement, which the turn
    spreads over [0, 0.45].  With thr = 0.4 (radius 0.8) the two candidates' distances lie on either side of the threshold wherever the
    z displacement is below 0.4: which of the two wins decides whether the point is an inlier."""
    n, thr = 12, 0.4
    src, tgt = lattice(n)
    a = 0.04
    T = np.eye(4, dtype=F)
    T[1:3, 1:3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[1:3, 3] = (0.0625, 0.03125)
    assert T[0].tolist() == [1, 0, 0, 0]
    ref = P.evaluate(src, tgt, T, score_id, thr)
    dev = lgr.evaluate_plane_dense(cuda(src), cuda(tgt), T, score_id, threshold=thr, with_inliers=True, with_nn=True)
    check(dev, ref)
    idx = np.arange(len(src))
    x = idx // (n * n)
    lower = np.where(x >= 1, idx - n * n, idx)   # the target at x - 0.5 (x = 0: the only one, at + 0.5)
    assert (dev.nn >= 0).all() and np.array_equal(dev.nn, lower)
    # the winner's normal: (0,0,1) when its lattice x is even.  Were the higher index to win, the other parity would hold the inliers
    win_z = (dev.nn // (n * n)) % 2 == 0
    inl = np.zeros(len(src), bool)
    inl[dev.inliers["index_query"]] = True
    assert 0 < inl.sum() < win_z.sum() and not inl[~win_z].any()   # x-normal winners are 0.5 away: never inliers; z-normal ones straddle thr
    assert (x[inl] >= 1).sum() > 0


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_source_sizes_across_launch_geometry(lgr, pair, ns):
    src, tgt, T, thr = (pair[k] for k in ("src", "tgt", "T", "thr"))
    s = src[:ns]
    ref = P.evaluate(s, tgt, T, 2, thr)
    check(lgr.evaluate_plane_dense(cuda(s), cuda(tgt), T, 2, with_inliers=True, with_nn=True), ref)
    check(lgr.evaluate_plane_dense_host(s, tgt, T, 2, threshold=thr, with_inliers=True, with_nn=True), ref)


@pytest.mark.parametrize("ns", [4095, 4096, 4097, 8193])
def test_source_sizes_across_sum_tiles(lgr, pair, ns):
    """the sequential sums take their terms in tiles of 4096 (GT_SUM_TILE, staged one ahead): a tile short of one term, exactly one, one
    term into the second, one term into the third.  The source is the fixture's repeated and cut to ns."""
    src, tgt, T, thr = (pair[k] for k in ("src", "tgt", "T", "thr"))
    s = np.concatenate([src] * 3)[:ns]
    ref = P.evaluate(s, tgt, T, 2, thr)
    assert ref["n_inliers"] > ns // 10
    check(lgr.evaluate_plane_dense(cuda(s), cuda(tgt), T, 2, with_inliers=True, with_nn=True), ref)
    check(lgr.evaluate_plane_dense_host(s, tgt, T, 2, threshold=thr, with_inliers=True, with_nn=True), ref)


def test_non_finite_points_and_normals(lgr, pair):
    src, tgt, T, thr = (pair[k] for k in ("src", "tgt", "T", "thr"))
    full = P.evaluate(src, tgt, T, 1, thr)
    # NaN / Inf source rows scattered through the cloud: skipped (nn = -1), everything else unchanged
    s_bad = src.copy()
    rows = np.arange(5, len(src), 97)
    s_bad[rows[0::3], 0] = np.nan
    s_bad[rows[1::3], 1] = np.inf
    s_bad[rows[2::3], 2] = -np.inf
    ref = P.evaluate(s_bad, tgt, T, 1, thr)
    dev = lgr.evaluate_plane_dense(cuda(s_bad), cuda(tgt), T, 1, threshold=thr, with_inliers=True, with_nn=True)
    check(dev, ref)
    assert (dev.nn[rows] == -1).all() and not np.isin(rows, dev.inliers["index_query"]).any() and 0 < dev.n_inliers < full["n_inliers"]
    # NaN target rows never answer: the points that had them as nearest get another target or none
    t_bad = tgt.copy()
    hit = np.unique(full["nn"][full["nn"] >= 0])[::5]
    t_bad[hit, :3] = np.nan
    ref = P.evaluate(src, t_bad, T, 1, thr)
    dev = lgr.evaluate_plane_dense(cuda(src), cuda(t_bad), T, 1, threshold=thr, with_inliers=True, with_nn=True)
    check(dev, ref)
    assert not np.isin(dev.nn, hit).any() and len(hit) > 50
    # a NaN normal on the nearest target: the point keeps its nearest target (nn) but is no inlier
    t_nn = tgt.copy()
    hit = np.unique(full["inliers"]["index_match"])[::4]
    t_nn[hit, 5] = np.nan
    ref = P.evaluate(src, t_nn, T, 1, thr)
    dev = lgr.evaluate_plane_dense(cuda(src), cuda(t_nn), T, 1, threshold=thr, with_inliers=True, with_nn=True)
    check(dev, ref)
    assert np.array_equal(dev.nn, full["nn"]) and not np.isin(dev.inliers["index_match"], hit).any() and 0 < dev.n_inliers < full["n_inliers"]
    assert np.isfinite(dev.rmse) and np.isfinite(dev.metric)


def test_weights(lgr, pair):
    from lgr_amd import capi
    src, tgt, T, thr = (pair[k] for k in ("src", "tgt", "T", "thr"))
    d_src, d_tgt = cuda(src), cuda(tgt)
    plain = P.evaluate(src, tgt, T, 2, thr)
    # a built map: weight = "curvature" (lgr_weights_dev gives the same map and its sum)
    w, w_sum = lgr.weights(d_src, "curvature")
    w_h = w.cpu().numpy()
    ref = P.evaluate(src, tgt, T, 2, thr, w_h)
    dev = lgr.evaluate_plane_dense(d_src, d_tgt, T, 2, weight="curvature", with_inliers=True, with_nn=True)
    check(dev, ref)
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, 2, weights=w, weights_sum=w_sum, threshold=thr), ref, False, False)   # the same map handed over
    assert bits(dev.metric) == bits(F(np.float64(dev.score) / np.float64(F(w_sum))))   # the denominator is weights_sum, the division in double
    assert dev.n_inliers == plain["n_inliers"] and bits(dev.rmse) == bits(plain["rmse"]) and bits(dev.metric) != bits(plain["metric"])
    # a caller's map with negative and zero entries
    rng = np.random.default_rng(3)
    wc = rng.uniform(-0.25, 1.0, len(src)).astype(F)
    wc[::7] = 0
    assert (wc < 0).sum() > 100
    ref = P.evaluate(src, tgt, T, 3, thr, wc)
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, 3, weights=cuda(wc), with_inliers=True, with_nn=True), ref)
    check(lgr.evaluate_plane_dense_host(src, tgt, T, 3, weights=wc, threshold=thr, with_inliers=True), ref, True, False)
    s = F(0)
    for v in wc:
        s = F(s + v)
    assert bits(ref["metric"]) == bits(F(np.float64(ref["score"]) / np.float64(s)))
    # constant weights: the sum of ns ones is ns, the figures are closest_plane's
    check(lgr.evaluate_plane_dense(d_src, d_tgt, T, 2, weight="constant", with_inliers=True, with_nn=True), plain)
    for name in ("harris", "tomasi"):
        with pytest.raises(capi.LgrError, match="rc=-5"):
            lgr.evaluate_plane_dense(d_src, d_tgt, T, 2, weight=name)


def test_invalid_arguments(lgr, pair):
    from lgr_amd import capi
    src, tgt, T = (pair[k] for k in ("src", "tgt", "T"))
    for s, t in ((src[:0], tgt), (src, tgt[:1]), (src, tgt[:0])):
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.evaluate_plane_dense(cuda(s), cuda(t), T, 0)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.evaluate_plane_dense(cuda(src), cuda(tgt), T, 4)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.evaluate_plane_dense(cuda(src), cuda(tgt), T, 0, threshold=float("nan"))


def test_agrees_with_the_sparse_evaluation(lgr, pair):
    """every pair (source index, nearest target) the sparse evaluation of the same transform reports is the dense evaluation's nearest
    target of that point, and the point is a dense inlier"""
    src, tgt, T = (pair[k] for k in ("src", "tgt", "T"))
    d_src, d_tgt = cuda(src), cuda(tgt)
    dev = lgr.evaluate_plane_dense(d_src, d_tgt, T, 2, with_inliers=True, with_nn=True)
    seen = 0
    for counter in (0, 1, 7):
        sp = lgr.evaluate_plane(d_src, d_tgt, T, 2, counter=counter, with_pairs=True)
        assert bits(sp["thr"]) == bits(dev.threshold) and len(sp["pairs"]) == sp["n_inl"]
        assert np.array_equal(dev.nn[sp["pairs"][:, 0]], sp["pairs"][:, 1])
        assert np.isin(sp["pairs"][:, 0], dev.inliers["index_query"]).all()
        seen += len(sp["pairs"])
    assert seen >= 30   # 1 % subsets of 4000 points, more than half of them inliers


@pytest.mark.parametrize("metric", ["correspondences", "uniformity", "closest_plane", "combination", "weighted_closest_plane"])
def test_analysis_metric(lgr, pair, metric):
    from lgr_amd import capi
    src, tgt, corr, T, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T", "T_gt", "thr"))
    d_src, d_tgt = cuda(src), cuda(tgt)
    mid = {"correspondences": capi.METRIC_CORRESPONDENCES, "uniformity": capi.METRIC_UNIFORMITY, "closest_plane": capi.METRIC_CLOSEST_PLANE,
           "combination": capi.METRIC_COMBINATION, "weighted_closest_plane": capi.METRIC_WEIGHTED_CLOSEST_PLANE}[metric]
    sid = capi.SCORE_MSE
    kw = dict(weight="curvature") if metric == "weighted_closest_plane" else {}
    m = lgr.analysis_metric(d_src, d_tgt, corr, T, G, metric_id=mid, score_id=sid, **kw)
    assert list(m.reserved) == [0, 0, 0, 0]
    if metric in ("closest_plane", "weighted_closest_plane"):
        w_h = lgr.weights(d_src, "curvature")[0].cpu().numpy() if kw else None
        ref = P.evaluate(src, tgt, T, sid, thr, w_h)
        assert m.n_inliers == ref["n_inliers"] > 0 and bits(m.rmse) == bits(ref["rmse"]) and bits(m.metric) == bits(ref["metric"])
        d = lgr.evaluate_plane_dense(d_src, d_tgt, T, sid, with_inliers=True, **kw)
        _, n_correct, _, _ = lgr.correct_correspondences(d_src, d_tgt, d.inliers, G)
        # buildCorrectInliers in float64 over the statement's list, away from the threshold (the f32 figure itself is lgr_correct_correspondences')
        ps = src[ref["inliers"]["index_query"], :3].astype(np.float64) @ G[:3, :3].astype(np.float64).T + G[:3, 3].astype(np.float64)
        e = np.linalg.norm(ps - tgt[ref["inliers"]["index_match"], :3].astype(np.float64), axis=1)
        sure = np.abs(e - thr) > 16 * 2.0 ** -24 * float(np.abs(tgt[:, :3]).max())   # a dozen f32 roundings at the size of a coordinate
        assert m.n_correct_inliers == n_correct and (e < thr)[sure].sum() <= n_correct <= (e < thr)[sure].sum() + (~sure).sum()
        assert 0 < n_correct <= m.n_inliers
    else:
        e_mid = capi.METRIC_CORRESPONDENCES if metric == "combination" else mid
        e_sid = capi.SCORE_CONSTANT if metric == "combination" else sid
        mask, n_inl, rmse, me = lgr.evaluate(d_src, d_tgt, corr, T, metric_id=e_mid, score_id=e_sid)
        _, _, n_correct_inl, n3_inl = lgr.correct_correspondences(d_src, d_tgt, corr, G, mask)
        assert m.n_inliers == n_inl == n3_inl and bits(m.rmse) == bits(rmse) and m.n_correct_inliers == n_correct_inl
        if metric == "combination":
            cp = P.evaluate(src, tgt, T, sid, thr)
            assert bits(m.metric) == bits(F(F(me) * cp["metric"])) and me > 0 and cp["metric"] > 0
        else:
            assert bits(m.metric) == bits(me)
    # without a ground truth: the same figures, no correct inliers; the host twin gives the device entry's figures
    m0 = lgr.analysis_metric(d_src, d_tgt, corr, T, None, metric_id=mid, score_id=sid, **kw)
    assert (m0.n_inliers, bits(m0.rmse), bits(m0.metric), m0.n_correct_inliers) == (m.n_inliers, bits(m.rmse), bits(m.metric), 0)
    mh = lgr.analysis_metric_host(src, tgt, corr, T, G, metric_id=mid, score_id=sid, **kw)
    assert (mh.n_inliers, bits(mh.rmse), bits(mh.metric), mh.n_correct_inliers) == (m.n_inliers, bits(m.rmse), bits(m.metric), m.n_correct_inliers)


# tests/point2plane_distance.cpp:29-58 of the reference: its ground-truth transform and corner scene, rebuilt here
CORNER_GT = np.array([[0.0803703, -0.996763, -0.00201846, 1.2143], [0.996758, 0.080377, -0.00349969, -6.13404],
                      [0.00365057, -0.00173067, 0.999992, -1.17221], [0, 0, 0, 1]], F)


def corner_scene(n=100, shift=5):
    from lgr_amd.synthetic import make_points
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    i, j = ij[:, 0], ij[:, 1]
    z = np.zeros_like(i)
    s = np.stack([np.stack([2 * i, 2 * j, z], 1), np.stack([shift + 2 * i, z, shift + 2 * j], 1), np.stack([z, 2 * shift + 2 * i, 2 * shift + 2 * j], 1)], 1).reshape(-1, 3)
    t = np.stack([np.stack([2 * i + 1, 2 * j, z], 1), np.stack([shift + 2 * i, z, shift + 2 * j + 1], 1), np.stack([z, 2 * shift + 2 * i + 1, 2 * shift + 2 * j], 1)], 1).reshape(-1, 3)
    gi = np.linalg.inv(CORNER_GT).astype(np.float64)
    src = make_points((s @ gi[:3, :3].T + gi[:3, 3]).astype(F))
    tgt = make_points(t.astype(F))
    vp_tgt = np.full(3, 2.0 * n, F)
    vp_src = (CORNER_GT[:3, :3].T.astype(np.float64) @ (vp_tgt - CORNER_GT[:3, 3]).astype(np.float64)).astype(F)
    return src, tgt, vp_src, vp_tgt


def test_reference_acceptance_through_the_dense_entry(lgr):
    """tests/point2plane_distance.cpp:88-96 on the device's own figures: after lgr_align on the 100 x 100 x 3 corner scene with the
    reference's parameters (FPFH standing in for the struct default SHOT, the one substitution tests/test_gpu_reference_acceptance.py
    documents), the dense closest-plane evaluation of the found transform has n_inliers / ns within 1e-5 of 1 and rmse < 2/3 -- and equals
    the statement bit for bit."""
    from lgr_amd import capi
    src, tgt, vp_src, vp_tgt = corner_scene()
    d_src, d_tgt = cuda(src), cuda(tgt)
    lgr.normals_knn(d_src, 30, vp=vp_src)
    lgr.normals_knn(d_tgt, 30, vp=vp_tgt)
    lgr.sync()
    prm = capi.default_params(matching_id=capi.MATCH_CLUSTER, metric_id=capi.METRIC_CLOSEST_PLANE, score_id=capi.SCORE_MSE, bf_block_size=200000,
                              max_iterations=10000, distance_thr=1.0, iss_radius_src=1.0, iss_radius_tgt=1.0, feature_radius=0.0, normals_available=0,
                              vp_src=vp_src, vp_tgt=vp_tgt)
    res = lgr.align(d_src, d_tgt, prm)
    assert res.converged == 1
    dev = lgr.evaluate_plane_dense(d_src, d_tgt, res.matrix(), capi.SCORE_MSE, with_inliers=True, with_nn=True)
    ns = len(src)
    print(f"corner scene: {dev.n_inliers} inliers of {ns}, rmse {dev.rmse!r}, metric {dev.metric!r}, threshold {dev.threshold!r}")
    assert abs(dev.n_inliers / ns - 1.0) <= 1e-5      # assertClose("inlier ratio", 1.f, ...)   :94
    assert dev.rmse < 2.0 / 3.0                       # assertLess("metric error", error, 2/3)  :95
    check(dev, P.evaluate(d_src.cpu().numpy(), d_tgt.cpu().numpy(), res.matrix(), capi.SCORE_MSE, dev.threshold))


def test_register_ply_plane_metric_rows(lgr, tmp_path):
    """tools/register_ply.py --metric closest_plane --ground-truth ... --metrics-csv ...: the results.csv row holds lgr_analysis_metric's
    rmse, inliers and correct inliers for the same steps made here (loader, alignment, correspondences: all deterministic), and the
    metrics.csv row is estimateTestMetric's, with its header on the new file"""
    import subprocess
    from lgr_amd import capi, formats, profile, synthetic
    # 100 000 raw points leave about 11 000 per cloud after the loader's voxel grid: the smallest size (tried on the CPU oracle: 4 000, 20 000 and
    # 60 000 do not) at which the closest-plane RANSAC, whose subsets are 1 % of the source, finds the ground truth within 20 000 iterations
    p = synthetic.make_pair(n_points=100000, seed=SEED)
    sp, tp, gt, res_csv, met_csv = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv", "results.csv", "metrics.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--metric", "closest_plane", "--ground-truth", gt, "a_b", "--results", res_csv, "--metrics-csv", met_csv]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "n/a" not in out.stdout
    # the same steps here
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", metric="closest_plane", iterations=20000,
                                  normals_available=ld["normals_available"])
    res = lgr.align(ld["src"], ld["tgt"], prm)
    corr = lgr.correspondences(ld["src"], ld["tgt"], prm)
    T, T_gt = res.matrix(), formats.get_transformation(gt, "a_b")
    m = lgr.analysis_metric(ld["src"], ld["tgt"], corr, T, T_gt, metric_id=prm.metric_id, score_id=prm.score_id)
    assert m.n_inliers > 0 and m.n_correct_inliers > 0
    lines = open(res_csv).read().splitlines()
    assert len(lines) == 2 and lines[0] == formats.RESULTS_HEADER
    got = dict(zip(formats.csv_row(lines[0]), formats.csv_row(lines[1])))
    assert got["metric_type"] == "closest_plane" and got["metric"] == formats._g(m.metric) and got["rmse"] == formats._g(m.rmse)
    assert got["inliers"] == str(m.n_inliers) and got["correct_inliers"] == str(m.n_correct_inliers)
    assert f"inliers_rmse: {m.rmse:.7f}" in out.stdout and f"correct inliers: {m.n_correct_inliers}/{m.n_inliers}" in out.stdout
    lines = open(met_csv).read().splitlines()
    assert len(lines) == 2 and lines[0] == formats.METRICS_HEADER
    cols, row = formats.csv_row(lines[0]), formats.csv_row(lines[1])
    assert len(row) == len(cols) == 9 and row[0] == "a_b"
    got = dict(zip(cols, row))
    for suffix, tn in (("", T), ("_gt", T_gt)):
        _, n_corr, _, m_corr = lgr.evaluate(ld["src"], ld["tgt"], corr, tn, metric_id=capi.METRIC_CORRESPONDENCES, score_id=prm.score_id)
        d = lgr.evaluate_plane_dense(ld["src"], ld["tgt"], tn, prm.score_id)
        assert float(got["metric_corr" + suffix]) >= 0 and int(got["inliers_icp" + suffix]) >= 0   # the fields parse
        assert (got["metric_corr" + suffix], got["metric_icp" + suffix]) == (formats._g(m_corr), formats._g(d.metric))
        assert (got["inliers_corr" + suffix], got["inliers_icp" + suffix]) == (str(n_corr), str(d.n_inliers))
    assert got["metric_icp"] == formats._g(m.metric) and got["inliers_icp"] == str(m.n_inliers)   # the run's metric IS the dense closest-plane one
