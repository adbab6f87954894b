"""GPU: n transforms judged against one ground truth (lgr_evaluate_gt_batch*).  The yardstick is the CPU statement
analysis_ref_lib.evaluate_gt, asked once per distinct (transform, converged, inlier mask) and kept for every case that needs it; every
member of a batch equals it on every field by bit pattern (two NaNs count as equal), and the correct mask equals the statement's.  Batch
sizes straddle the chunk of 8 and reach the maximum of 64; source sizes cross a workgroup and the 4096-term tile of the sum jobs."""
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


def perturbed(T_gt, thr):
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    return (dT @ T_gt).astype(F)


@pytest.fixture(scope="module")
def pair(lgr):
    """the scene of test_gpu_analysis.py: make_pair(4000, seed 12), normals from lgr_normals_knn, thr = twice the target's density, one-sided
    correspondences; the five poses the batches cycle through and the four inlier masks"""
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
    rng = np.random.default_rng(5)
    T_far = synthetic.random_se3(rng).astype(F)
    res, _ = lgr.ransac(cuda(out["src"]), cuda(out["tgt"]), corr, capi.default_params(distance_thr=thr, max_iterations=20000))
    c = len(corr)
    out.update(thr=float(F(thr)), corr=corr, T=perturbed(p["T_gt"], thr),
               poses=[out["T_gt"], perturbed(p["T_gt"], thr), np.eye(4, dtype=F), T_far, res.matrix()],
               masks=[(rng.random(c) < 0.5).astype(np.uint8), np.zeros(c, np.uint8), (rng.random(c) < 0.1).astype(np.uint8), np.ones(c, np.uint8)],
               memo={})
    return out


def member(pair, s, with_masks):
    """what member s of a batch is made of: (pose index, converged, mask index or None); ten distinct members with masks, ten without"""
    k = s % 10
    return k % 5, k < 5 or k == 7, (k % 4 if with_masks else None)


def reference(pair, key):
    """the statement's answer for one member, computed once"""
    if key not in pair["memo"]:
        pose, conv, mi = key
        pair["memo"][key] = A.evaluate_gt(pair["src"], pair["tgt"], pair["corr"], pair["poses"][pose], pair["T_gt"], pair["thr"], conv,
                                          None if mi is None else pair["masks"][mi])
    return pair["memo"][key]


def batch_inputs(pair, n, with_masks):
    keys = [member(pair, s, with_masks) for s in range(n)]
    Ts = [pair["poses"][k[0]] for k in keys]
    conv = [k[1] for k in keys]
    masks = np.stack([pair["masks"][k[2]] for k in keys]) if with_masks else None
    return keys, Ts, conv, masks


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("n", [1, 2, 8, 9, 64])
def test_batch_equals_the_statement(lgr, pair, n, with_masks):
    src, tgt, corr, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T_gt", "thr"))
    keys, Ts, conv, masks = batch_inputs(pair, n, with_masks)
    ns = len(src)
    # not vacuous, on the statement's values: the members near the ground truth overlap and have correct correspondences, the far pose is far
    for pose in (0, 1):
        ref, _ = reference(pair, member(pair, pose, with_masks))
        assert ref["overlap_size"] >= ns // 10 and ref["n_correct_correspondences"] >= 20
    if n > 3:
        assert reference(pair, member(pair, 3, with_masks))[0]["overlap_rmse"] > thr
    if n >= 8:
        assert len(set(conv)) == 2
    out = lgr.evaluate_gt_batch(cuda(src), cuda(tgt), corr, Ts, G, thr, conv, masks)
    assert len(out) == n
    for s in range(n):
        ref, mask = reference(pair, keys[s])
        check_eval(out[s], ref, mask)
    if with_masks and n >= 4:
        assert out[1].n_inliers == 0 and out[3].n_inliers == len(corr) and out[3].n_correct_inliers == out[3].n_correct_correspondences > 0
        assert 0 < out[0].n_correct_inliers < out[0].n_inliers < len(corr)


def test_batch_equals_the_single_entry(lgr, pair):
    """... and the existing single-transform entry point, member by member (9 members: a full chunk and one more)"""
    src, tgt, corr, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T_gt", "thr"))
    keys, Ts, conv, masks = batch_inputs(pair, 9, True)
    d_src, d_tgt = cuda(src), cuda(tgt)
    out = lgr.evaluate_gt_batch(d_src, d_tgt, corr, Ts, G, thr, conv, masks)
    for s in (0, 3, 7, 8):
        one = lgr.evaluate_gt(d_src, d_tgt, corr, Ts[s], G, thr, conv[s], masks[s])
        check_eval(out[s], {f: getattr(one, f) for f in A.FLOAT_FIELDS + A.INT_FIELDS}, one.correct_mask)


def sized_source(pair, ns):
    """the source of test_sizes_across_launch_geometry"""
    extra = pair["src"][:97].copy()
    extra[:, :3] += F(0.25 * pair["thr"])
    return np.concatenate([pair["src"], extra])[:ns]


@pytest.mark.parametrize("ns,variant", [(1, "plain"), (257, "plain"), (4097, "plain"), (257, "corr_twice"), (257, "no_corr")])
def test_sizes_across_launch_geometry(lgr, pair, ns, variant):
    """three members; ns = 257 crosses a workgroup, 4097 the 4096-term tile of a sum job; c > ns (the correspondences listed twice) makes the
    correspondence half of the kernels the longer one; c = 0 leaves only the point half"""
    tgt, G, thr = (pair[k] for k in ("tgt", "T_gt", "thr"))
    s = sized_source(pair, ns)
    c = pair["corr"][pair["corr"]["index_query"] < ns]
    if variant == "corr_twice":
        c = np.concatenate([c, c])
        assert len(c) > ns
    elif variant == "no_corr":
        c = c[:0]
    rng = np.random.default_rng(ns)
    Ts = [pair["poses"][1], pair["poses"][3], pair["poses"][0]]
    conv = [True, True, False]
    masks = (rng.random((3, len(c))) < 0.5).astype(np.uint8)
    out = lgr.evaluate_gt_batch(cuda(s), cuda(tgt), c, Ts, G, thr, conv, masks)
    for k in range(3):
        ref, mask = A.evaluate_gt(s, tgt, c, Ts[k], G, thr, conv[k], masks[k])
        check_eval(out[k], ref, mask)


def test_ground_truth_far_away(lgr, pair):
    """a ground truth ten extents away from the target: no source point finds a target point"""
    src, tgt, corr, thr = (pair[k] for k in ("src", "tgt", "corr", "thr"))
    extent = float((tgt[:, :3].max(0) - tgt[:, :3].min(0)).max())
    far = np.eye(4)
    far[2, 3] = 10 * extent
    far = (far @ pair["T_gt"].astype(np.float64)).astype(F)
    Ts = [pair["poses"][0], pair["poses"][1], far]
    out = lgr.evaluate_gt_batch(cuda(src), cuda(tgt), corr, Ts, far, thr, [True, True, True])
    for k in range(3):
        ref, mask = A.evaluate_gt(src, tgt, corr, Ts[k], far, thr, True)
        check_eval(out[k], ref, mask)
        assert out[k].overlap_size == 0 and np.isnan(out[k].overlap_rmse) and out[k].converged_and_overlap_ok == 0 and out[k].converged == 1


def lattice(n=12):
    """the tie scene of test_gpu_analysis.py: a source point with x >= 1 has two nearest targets at squared distance 0.25"""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(F)
    nrm = np.where((g[:, :1] % 2) == 0, np.array([[0, 0, 1]], F), np.array([[1, 0, 0]], F))
    src = np.zeros((len(g), 12), F)
    src[:, :3] = g; src[:, 3] = 1; src[:, 4:7] = nrm; src[:, 8] = 1
    tgt = src.copy()
    tgt[:, 0] += 0.5
    return src, tgt


@pytest.mark.parametrize("thr", [0.45, 0.75])
def test_ties_lower_index_wins(lgr, thr):
    src, tgt = lattice(12)
    G = np.eye(4, dtype=F)
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0.125, 0.0625, 0.03125)
    T2 = np.eye(4, dtype=F)
    T2[:3, 3] = (-0.25, 0.5, 0.0)
    corr = np.zeros(len(src), A.CORR_DTYPE)
    corr["index_query"] = np.arange(len(src)); corr["index_match"] = np.arange(len(src)); corr["threshold"] = np.where(np.arange(len(src)) % 3 == 0, 0.5, 0.75)
    out = lgr.evaluate_gt_batch(cuda(src), cuda(tgt), corr, [T, T2], G, thr, [True, True])
    for k, Tk in enumerate((T, T2)):
        ref, mask = A.evaluate_gt(src, tgt, corr, Tk, G, thr, True)
        check_eval(out[k], ref, mask)
    assert 0 < out[0].overlap_size <= len(src) and not same_float(out[0].overlap_rmse, out[1].overlap_rmse)


def test_host_twin(lgr, pair):
    src, tgt, corr, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T_gt", "thr"))
    keys, Ts, conv, masks = batch_inputs(pair, 9, True)
    dev = lgr.evaluate_gt_batch(cuda(src), cuda(tgt), corr, Ts, G, thr, conv, masks)
    host = lgr.evaluate_gt_batch_host(src, tgt, corr, Ts, G, thr, conv, masks)
    assert len(host) == len(dev) == 9
    for s in range(9):
        ref, mask = reference(pair, keys[s])
        check_eval(host[s], ref, mask)
        check_eval(dev[s], ref, mask)
    keys, Ts, conv, _ = batch_inputs(pair, 2, False)
    host = lgr.evaluate_gt_batch_host(src, tgt, corr, Ts, G, thr, conv)
    for s in range(2):
        check_eval(host[s], *reference(pair, keys[s]))


def test_argument_handling(lgr, pair):
    from lgr_amd import capi
    src, tgt, corr, G, thr = (pair[k] for k in ("src", "tgt", "corr", "T_gt", "thr"))
    d_src, d_tgt = cuda(src), cuda(tgt)
    assert lgr.evaluate_gt_batch(d_src, d_tgt, corr, [], G, thr) == []   # n = 0: nothing to do, nothing written
    assert lgr.evaluate_gt_batch_host(src, tgt, corr, [], G, thr) == []
    with pytest.raises(capi.LgrError, match="rc=%d" % capi.ERR_UNSUPPORTED):
        lgr.evaluate_gt_batch(d_src, d_tgt, corr, [G] * (capi.GT_BATCH_MAX + 1), G, thr)
    with pytest.raises(capi.LgrError, match="rc=%d" % capi.ERR_UNSUPPORTED):
        lgr.evaluate_gt_batch_host(src, tgt, corr, [G] * (capi.GT_BATCH_MAX + 1), G, thr)
    for bad_thr in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.LgrError, match="rc=%d" % capi.ERR_INVALID_ARG):
            lgr.evaluate_gt_batch(d_src, d_tgt, corr, [G, G], G, bad_thr)
    bad = corr.copy()
    bad["index_match"][3] = len(tgt)
    with pytest.raises(capi.LgrError, match="rc=%d" % capi.ERR_INVALID_ARG):
        lgr.evaluate_gt_batch(d_src, d_tgt, bad, [G], G, thr)
