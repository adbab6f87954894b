"""GPU: the ground-truth evaluation of an alignment (lgr_evaluate_gt*, lgr_overlap_rmse_dev, lgr_merge_overlaps_dev,
lgr_normal_difference_dev) against the CPU statement tests/cpp/analysis_ref.cpp: every float bit for bit (compared as uint32; two NaNs
count as equal), every mask, index list and count equal.  Cases: an estimate near the ground truth, one far from it, a lattice whose
queries all have two equidistant nearest targets, degenerate inputs, source sizes around the wave and workgroup edges, the host twin
and the inlier mask."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref_lib as A  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_float(x, y):
    x, y = F(x), F(y)
    return (np.isnan(x) and np.isnan(y)) or x.view(np.uint32) == y.view(np.uint32)


def check_eval(dev, ref, ref_mask):
    """dev: capi.GtEval, ref / ref_mask: analysis_ref_lib.evaluate_gt"""
    for f in A.FLOAT_FIELDS:
        assert same_float(getattr(dev, f), ref[f]), (f, getattr(dev, f), ref[f])
    for f in A.INT_FIELDS:
        assert getattr(dev, f) == ref[f], (f, getattr(dev, f), ref[f])
    assert np.array_equal(dev.correct_mask, ref_mask)


def check_blocks(lgr, src, tgt, T, G, thr):
    """the three building blocks against the statement, per-point outputs included"""
    d_src, d_tgt = cuda(src), cuda(tgt)
    r = A.overlap_rmse(src, tgt, T, G, thr)
    rm, n, pe, idx = lgr.overlap_rmse(d_src, d_tgt, T, G, thr)
    assert same_float(rm, r["overlap_rmse"]) and n == r["overlap_size"] and same_float(pe, r["pcd_err"])
    assert np.array_equal(idx, r["idx"])
    m = A.merge_overlaps(src, tgt, G, thr)
    dm = lgr.merge_overlaps(d_src, d_tgt, G, thr)
    assert np.array_equal(dm["mask_src"], m["mask_src"]) and np.array_equal(dm["mask_tgt"], m["mask_tgt"])
    assert (dm["n_overlap_src"], dm["n_overlap_tgt"]) == (m["n_overlap_src"], m["n_overlap_tgt"])
    assert same_float(dm["overlap"], m["overlap"]) and same_float(dm["overlap_area"], m["overlap_area"])
    nd, nn, _ = A.normal_difference(src, tgt, G, thr)
    dnd, dnn = lgr.normal_difference(d_src, d_tgt, G, thr)
    assert same_float(dnd, nd) and dnn == nn
    return r, m, (nd, nn)


def perturbed(T_gt, thr):
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    return (dT @ T_gt).astype(F)


@pytest.fixture(scope="module")
def pair(lgr):
    """make_pair(4000, seed 12), normals from lgr_normals_knn, thr = twice the target's density, correspondences from lgr_correspondences
    (one-sided matching: 4000 of them, about a hundred correct; seed and matching chosen on the CPU so that the conditions of
    test_near_ground_truth hold)"""
    from lgr_amd import capi, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    out = dict(T_gt=p["T_gt"].astype(F))
    for side in ("src", "tgt"):
        d = cuda(p[side])
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        out[side] = d.cpu().numpy()
    thr = 2 * lgr.cloud_density(cuda(out["tgt"]))
    params = capi.default_params(matching_id=capi.MATCH_ONE_SIDED, bf_block_size=200000, distance_thr=thr, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"])
    corr = lgr.correspondences(cuda(out["src"]), cuda(out["tgt"]), params).cpu().numpy().view(A.CORR_DTYPE).reshape(-1)
    out.update(thr=float(F(thr)), corr=corr, T=perturbed(p["T_gt"], thr))
    rng = np.random.default_rng(5)
    out["T_far"] = synthetic.random_se3(rng).astype(F)
    out["inl"] = (rng.random(len(corr)) < 0.5).astype(np.uint8)
    return out


def test_near_ground_truth(lgr, pair):
    src, tgt, corr, T, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T", "T_gt", "thr"))
    ref, mask = A.evaluate_gt(src, tgt, corr, T, G, thr, True)
    ns = len(src)
    assert ref["overlap_size"] >= ns // 10 and ref["n_normal_overlap"] >= ns // 10 and ref["n_correct_correspondences"] >= 20   # not vacuous
    dev = lgr.evaluate_gt(cuda(src), cuda(tgt), corr, T, G, thr, True)
    check_eval(dev, ref, mask)
    assert dev.converged_and_overlap_ok == 1
    r, m, _ = check_blocks(lgr, src, tgt, T, G, thr)
    assert r["overlap_size"] == ref["overlap_size"] and m["n_overlap_src"] == ref["n_overlap_src"]


def test_far_from_ground_truth(lgr, pair):
    src, tgt, corr, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T_gt", "thr"))
    T = pair["T_far"]
    ref, mask = A.evaluate_gt(src, tgt, corr, T, G, thr, True)
    dev = lgr.evaluate_gt(cuda(src), cuda(tgt), corr, T, G, thr, True)
    check_eval(dev, ref, mask)
    assert dev.converged_and_overlap_ok == 0 and dev.overlap_rmse > thr
    check_blocks(lgr, src, tgt, T, G, thr)


def lattice(n=12):
    """source on the integer lattice n^3 (index = (x n + y) n + z), the target the same lattice shifted by exactly 0.5 along x: a source
    point with x >= 1 has two nearest targets at squared distance 0.25, x - 0.5 (the lower index) and x + 0.5.  The normals alternate with
    x between (0,0,1) and (1,0,0), so that the chosen neighbour decides plane distances, overlap terms and normal differences."""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(F)
    nrm = np.where((g[:, :1] % 2) == 0, np.array([[0, 0, 1]], F), np.array([[1, 0, 0]], F))
    src = np.zeros((len(g), 12), F)
    src[:, :3] = g; src[:, 3] = 1; src[:, 4:7] = nrm; src[:, 8] = 1
    tgt = src.copy()
    tgt[:, 0] += 0.5
    return src, tgt


@pytest.mark.parametrize("thr", [0.45, 0.75])
def test_ties_lower_index_wins(lgr, thr):
    # thr 0.45: radius 0.9 holds the two tied targets only; a target with normal (1,0,0) is 0.5 away along its normal: skipped / outside the
    #   overlap, one with (0,0,1) is in its plane: the tie decides masks and skipped points; no normal difference counts (0.5 is not < thr).
    # thr 0.75: everything counts; the tie decides every term and every normal difference.
    n = 12
    src, tgt = lattice(n)
    G = np.eye(4, dtype=F)
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0.125, 0.0625, 0.03125)
    corr = np.zeros(len(src), A.CORR_DTYPE)
    corr["index_query"] = np.arange(len(src)); corr["index_match"] = np.arange(len(src)); corr["threshold"] = np.where(np.arange(len(src)) % 3 == 0, 0.5, 0.75)
    r, m, (nd, nn) = check_blocks(lgr, src, tgt, T, G, thr)
    x = np.arange(len(src)) // (n * n)
    lower = np.where(x >= 1, np.arange(len(src)) - n * n, np.arange(len(src)))   # the target at x - 0.5 (x = 0: the only one, at + 0.5)
    _, _, _, idx = lgr.overlap_rmse(cuda(src), cuda(tgt), T, G, thr)
    assert np.array_equal(idx[idx >= 0], lower[idx >= 0])
    if thr == 0.75:
        assert (idx >= 0).all() and nn == len(src)
    else:
        assert 0 < (idx >= 0).sum() < len(src) and nn == 0 and same_float(nd, np.pi)
        assert 0 < m["n_overlap_src"] < len(src)
    ref, mask = A.evaluate_gt(src, tgt, corr, T, G, thr, True)
    check_eval(lgr.evaluate_gt(cuda(src), cuda(tgt), corr, T, G, thr, True), ref, mask)
    assert 0 < mask.sum() < len(mask)   # distance 0.5: not < 0.5, < 0.75


def test_degenerate_inputs(lgr, pair):
    src, tgt, corr, T, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T", "T_gt", "thr"))

    def run(s, t, c, Tg=G, inl=None):
        ref, mask = A.evaluate_gt(s, t, c, T, Tg, thr, True, inl)
        dev = lgr.evaluate_gt(cuda(s), cuda(t), c, T, Tg, thr, True, inl)
        check_eval(dev, ref, mask)
        return dev
    # target normals all NaN: no overlap term, mergeOverlaps falls back to the squared distance
    t_nan = tgt.copy()
    t_nan[:, 4:7] = np.nan
    d = run(src, t_nan, corr)
    assert d.overlap_size == 0 and np.isnan(d.overlap_rmse) and d.n_overlap_src > 0 and d.n_normal_overlap == 0 and d.converged_and_overlap_ok == 0
    # the source 100 thr away from the target under the ground truth: no neighbour in radius
    far = np.eye(4)
    far[2, 3] = 100 * thr
    far = (far @ G.astype(np.float64)).astype(F)
    d = run(src, tgt, corr, Tg=far)
    assert same_float(d.normal_diff, np.pi) and d.n_overlap == 0 and d.overlap == 0 and np.isnan(d.overlap_area) and np.isnan(d.overlap_rmse)
    # one source point; no correspondences
    d = run(src[:1], tgt, corr[:0])
    assert d.n_correspondences == 0 and np.isnan(d.overlap_area)
    d = run(src, tgt, corr[:0])
    assert d.n_correct_correspondences == 0 and d.corr_uniformity == 0 and d.overlap_size > 0
    # a non-finite source point in the middle of the cloud (and a correspondence through it)
    s_bad = src.copy()
    s_bad[len(src) // 2, :3] = (np.nan, np.inf, 0)
    c_bad = corr.copy()
    c_bad["index_query"][0] = len(src) // 2
    d = run(s_bad, tgt, c_bad)
    assert d.overlap_size > 0 and np.isnan(d.pcd_err) and d.correct_mask[0] == 0
    check_blocks(lgr, s_bad, tgt, T, G, thr)
    # a normal with a finite x and a NaN y.  In the source the rotation spreads the NaN to the rotated x, and the point fails "normal_x is
    # finite"; in the target the point passes the three listed conditions and the angle itself is NaN: it does not count either (the
    # reference's `diff >= 0.f` filter).  Every other point still counts.
    full = run(src, tgt, corr)
    for s_ny, t_ny in ((src.copy(), tgt), (src, tgt.copy())):
        (s_ny if t_ny is tgt else t_ny)[::3, 5] = np.nan
        d = run(s_ny, t_ny, corr)
        assert 0 < d.n_normal_overlap < full.n_normal_overlap
        nd, nn, vals = A.normal_difference(s_ny, t_ny, G, thr)
        dnd, dnn = lgr.normal_difference(cuda(s_ny), cuda(t_ny), G, thr)
        assert same_float(dnd, nd) and dnn == nn == d.n_normal_overlap and (vals >= 0).sum() == nn and not np.isnan(nd)
    # an empty cloud is a defined result, not an error
    for s, t in ((src[:0], tgt), (src, tgt[:0])):
        d = run(s, t, corr[:0])
        assert d.overlap_size == 0 and np.isnan(d.overlap_rmse) and same_float(d.normal_diff, np.pi) and d.n_overlap == 0


def test_invalid_arguments(lgr, pair):
    from lgr_amd import capi
    src, tgt, corr, T, G = (pair[k] for k in ("src", "tgt", "corr", "T", "T_gt"))
    for thr in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.evaluate_gt(cuda(src), cuda(tgt), corr, T, G, thr)
    bad = corr.copy()
    bad["index_match"][3] = len(tgt)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.evaluate_gt(cuda(src), cuda(tgt), bad, T, G, pair["thr"])


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 257, 4097])
def test_sizes_across_launch_geometry(lgr, pair, ns):
    src, tgt, corr, T, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T", "T_gt", "thr"))
    extra = src[:97].copy()
    extra[:, :3] += F(0.25 * thr)
    s = np.concatenate([src, extra])[:ns]
    c = corr[corr["index_query"] < ns]
    ref, mask = A.evaluate_gt(s, tgt, c, T, G, thr, True)
    check_eval(lgr.evaluate_gt(cuda(s), cuda(tgt), c, T, G, thr, True), ref, mask)


def test_host_twin_and_inlier_mask(lgr, pair):
    src, tgt, corr, T, G, thr, inl = (pair[k] for k in ("src", "tgt", "corr", "T", "T_gt", "thr", "inl"))
    ref, mask = A.evaluate_gt(src, tgt, corr, T, G, thr, True, inl)
    dev = lgr.evaluate_gt(cuda(src), cuda(tgt), corr, T, G, thr, True, inl)
    host = lgr.evaluate_gt_host(src, tgt, corr, T, G, thr, True, inl)
    check_eval(dev, ref, mask)
    check_eval(host, ref, mask)
    assert dev.n_inliers == int(inl.sum()) and dev.n_correct_inliers == int((inl & dev.correct_mask).sum()) and dev.n_correct_inliers > 0
    # the final mask of a RANSAC run as the inlier mask
    from lgr_amd import capi
    res, fm = lgr.ransac(cuda(src), cuda(tgt), corr, capi.default_params(distance_thr=thr, max_iterations=20000))
    ref, mask = A.evaluate_gt(src, tgt, corr, res.matrix(), G, thr, bool(res.converged), fm)
    dev = lgr.evaluate_gt(cuda(src), cuda(tgt), corr, res.matrix(), G, thr, bool(res.converged), fm)
    check_eval(dev, ref, mask)
    assert dev.n_correct_inliers == int((fm & mask).sum())


def test_register_ply_ground_truth(lgr, pair, tmp_path):
    """tools/register_ply.py --ground-truth: the printed analysis and the appended results.csv row hold the numbers lgr_evaluate_gt gives
    for the same steps made here (loader, alignment, correspondences: all deterministic)"""
    import subprocess
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp, gt, res_csv = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv", "results.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--ground-truth", gt, "a_b", "--results", res_csv]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    # the same steps here
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", iterations=20000,
                                  normals_available=ld["normals_available"])
    res = lgr.align(ld["src"], ld["tgt"], prm)
    corr = lgr.correspondences(ld["src"], ld["tgt"], prm)
    inl, n_inl, rmse, metric = lgr.evaluate(ld["src"], ld["tgt"], corr, res.matrix(), metric_id=prm.metric_id, score_id=prm.score_id)
    T_gt = formats.get_transformation(gt, "a_b")
    e = lgr.evaluate_gt(ld["src"], ld["tgt"], corr, res.matrix(), T_gt, prm.distance_thr, bool(res.converged), inl)
    ref, mask = A.evaluate_gt(ld["src"].cpu().numpy(), ld["tgt"].cpu().numpy(), corr.cpu().numpy().view(A.CORR_DTYPE).reshape(-1), res.matrix(), T_gt,
                              prm.distance_thr, bool(res.converged), inl)
    check_eval(e, ref, mask)
    lines = open(res_csv).read().splitlines()
    assert len(lines) == 2 and lines[0] == formats.RESULTS_HEADER
    cols, row = formats.csv_row(lines[0]), formats.csv_row(lines[1])
    assert len(row) == len(cols)
    got = dict(zip(cols, row))
    for name in ("r_err", "t_err", "pcd_err", "normal_diff", "corr_uniformity", "overlap_rmse", "overlap", "overlap_area"):
        assert got[name] == formats._g(getattr(e, name)), name
    assert got["correct_correspondences"] == str(e.n_correct_correspondences) and got["correct_inliers"] == str(e.n_correct_inliers)
    assert got["correspondences"] == str(len(corr)) and got["inliers"] == str(n_inl) and got["testname"] == "a_b" and got["converged"] == str(int(res.converged))
    assert f"correct correspondences: {e.n_correct_correspondences}/{len(corr)}" in out.stdout
    assert f"point cloud error: {e.pcd_err:.7f}" in out.stdout and f"translation error: {e.t_err:.7f}" in out.stdout
    assert f"overlap error: {e.overlap_rmse:.7f} over {e.overlap_size} points" in out.stdout
