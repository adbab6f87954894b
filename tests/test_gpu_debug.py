"""GPU: temperature maps, hypothesis overlap comparison, the far-safe nearest neighbour and the colour passes (lgr_temperature_map*,
lgr_temperature_maps*, lgr_compare_overlaps*, lgr_nearest_dev, lgr_color_*) against the CPU statement tests/cpp/debug_ref.cpp: every float bit
for bit (compared as uint32), every colour, index, mask and count equal.  The pair, threshold and transformations are those of
test_gpu_analysis.py's fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_ref_lib as D  # noqa: E402
from test_gpu_analysis import lattice, perturbed  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_side(dev, ref, what=""):
    for k in D.TEMP_FIELDS:
        assert same_bits(dev[k], ref[k]), (what, k, int((dev[k].view(np.uint32) != ref[k].view(np.uint32)).sum()))
    assert dev["n_below"] == ref["n_below"], (what, dev["n_below"], ref["n_below"])


def check_maps(dev, ref):
    check_side(dev["src"], ref["src"], "src")
    check_side(dev["tgt"], ref["tgt"], "tgt")
    moved = dev["moved"] if isinstance(dev["moved"], np.ndarray) else dev["moved"].cpu().numpy()
    assert same_bits(moved, ref["moved"])


def check_overlaps(dev, ref):
    assert np.array_equal(dev["counts"], ref["counts"]), (dev["counts"], ref["counts"])
    assert np.array_equal(dev["counts2"], ref["counts2"])
    assert same_bits(dev["weighted"], ref["weighted"]), (dev["weighted"], ref["weighted"])
    assert np.array_equal(dev["mask_src"], ref["mask_src"]) and np.array_equal(dev["mask_tgt"], ref["mask_tgt"])


@pytest.fixture(scope="module")
def pair(lgr):
    """make_pair(4000, seed 12), normals from lgr_normals_knn, thr = twice the target's density (test_gpu_analysis.py's fixture)"""
    from lgr_amd import synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    out = dict(T_gt=p["T_gt"].astype(F))
    for side in ("src", "tgt"):
        d = cuda(p[side])
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        out[side] = d.cpu().numpy()
    thr = float(F(2 * lgr.cloud_density(cuda(out["tgt"]))))
    out.update(thr=thr, T=perturbed(p["T_gt"], thr))
    rng = np.random.default_rng(5)
    out["T_far"] = synthetic.random_se3(rng).astype(F)
    ext = float((out["tgt"][:, :3].max(0) - out["tgt"][:, :3].min(0)).max())
    shift = np.eye(4)
    shift[:3, 3] = 10 * ext * np.array([0.6, -0.64, 0.48])
    out["T_shift"] = (shift @ p["T_gt"].astype(np.float64)).astype(F)
    return out


@pytest.mark.parametrize("which", ["T_gt", "T"])
def test_temperature_maps_near(lgr, pair, which):
    src, tgt, thr, T = pair["src"], pair["tgt"], pair["thr"], pair[which]
    ref = D.temperature_maps(src, tgt, T, thr)
    assert ref["src"]["n_below"] >= len(src) // 10 and ref["tgt"]["n_below"] >= len(src) // 10   # not vacuous, by the statement alone
    dev = lgr.temperature_maps(cuda(src), cuda(tgt), T, thr)
    check_maps(dev, ref)
    assert (dev["src"]["temp_distance"] < F(thr)).sum() == dev["src"]["n_below"]
    # the reference's mergeOverlaps applies the identical rule (src/common.cpp:558-591): the masks pinned by test_gpu_analysis.py
    m = lgr.merge_overlaps(cuda(src), cuda(tgt), T, thr)
    assert np.array_equal(dev["src"]["temp_distance"] < F(thr), m["mask_src"].astype(bool))
    assert np.array_equal(dev["tgt"]["temp_distance"] < F(thr), m["mask_tgt"].astype(bool))
    # one direction alone
    one = lgr.temperature_map(dev["moved"], cuda(tgt), thr)
    check_side(one, ref["src"])


def test_compare_overlaps_near_and_far(lgr, pair):
    src, tgt, thr = pair["src"], pair["tgt"], pair["thr"]
    Ts = [pair["T"], pair["T_gt"], pair["T_far"], pair["T_shift"]]
    ref = D.compare_overlaps(src, tgt, Ts, thr)
    assert ref["counts"][1] >= len(src) // 10 and ref["weighted"][1] > 0
    dev = lgr.compare_overlaps(cuda(src), cuda(tgt), Ts, thr)
    check_overlaps(dev, ref)
    assert dev["counts"][3] == 0 and dev["weighted"][3] == 0     # ten extents away: nothing lies within thr of its nearest neighbour's plane
    # the unbounded search finds at least what the search within 2 thr finds
    for k in (0, 1):
        m = lgr.merge_overlaps(cuda(src), cuda(tgt), Ts[k], thr)
        assert not (m["mask_src"].astype(bool) & ~dev["mask_src"][k].astype(bool)).any()
        assert not (m["mask_tgt"].astype(bool) & ~dev["mask_tgt"][k].astype(bool)).any()
    nomask = lgr.compare_overlaps(cuda(src), cuda(tgt), Ts, thr, with_masks=False)
    assert np.array_equal(nomask["counts"], ref["counts"]) and same_bits(nomask["weighted"], ref["weighted"])


@pytest.mark.parametrize("which", ["T_far", "T_shift", "T_gt"])
def test_nearest_against_statement(lgr, pair, which):
    src, tgt = pair["src"], pair["tgt"]
    q = D.move(src, pair[which])
    for a, b in ((q, tgt), (tgt, q)):
        idx, d2 = lgr.nearest(cuda(a), cuda(b))
        ri, rd = D.nearest(a, b)
        assert np.array_equal(idx.cpu().numpy(), ri) and same_bits(d2.cpu().numpy(), rd)


def test_nearest_equals_knn_inside_the_box(lgr, pair):
    src, tgt = pair["src"], pair["tgt"]
    q = D.move(src, pair["T"])
    lo, hi = tgt[:, :3].min(0), tgt[:, :3].max(0)
    inside = ((q[:, :3] >= lo) & (q[:, :3] <= hi)).all(1)
    assert inside.sum() >= len(q) // 4
    qi = q[inside]
    idx, d2 = lgr.nearest(cuda(qi), cuda(tgt))
    ki, kd = lgr.knn(cuda(qi), cuda(tgt), 1)
    assert np.array_equal(idx.cpu().numpy(), ki.cpu().numpy()[:, 0]) and same_bits(d2.cpu().numpy(), kd.cpu().numpy()[:, 0])
    # the cloud against itself: every point is its own nearest neighbour at distance 0
    idx, d2 = lgr.nearest(cuda(tgt), cuda(tgt))
    assert np.array_equal(idx.cpu().numpy(), np.arange(len(tgt))) and not d2.cpu().numpy().any()


def test_ties_lower_index_wins(lgr):
    n = 12
    src, tgt = lattice(n)
    x = np.arange(len(src)) // (n * n)
    lower = np.where(x >= 1, np.arange(len(src)) - n * n, np.arange(len(src)))   # the target at x - 0.5 (x = 0: the only one, at + 0.5)
    idx, d2 = lgr.nearest(cuda(src), cuda(tgt))
    assert np.array_equal(idx.cpu().numpy(), lower) and (d2.cpu().numpy() == 0.25).all()
    ri, _ = D.nearest(src, tgt)
    assert np.array_equal(ri, lower)
    eye = np.eye(4, dtype=F)
    for thr in (0.45, 0.75):
        ref = D.temperature_maps(src, tgt, eye, thr)
        dev = lgr.temperature_maps(cuda(src), cuda(tgt), eye, thr)
        check_maps(dev, ref)
        assert np.array_equal(dev["src"]["nn"], lower)
        check_overlaps(lgr.compare_overlaps(cuda(src), cuda(tgt), [eye], thr), D.compare_overlaps(src, tgt, [eye], thr))
    assert 0 < dev["src"]["n_below"]


def test_degenerate_inputs(lgr, pair):
    src, tgt, thr, T = pair["src"], pair["tgt"], pair["thr"], pair["T"]

    def run(s, t, Ts=(T,)):
        ref = D.temperature_maps(s, t, Ts[0], thr)
        dev = lgr.temperature_maps(cuda(s), cuda(t), Ts[0], thr)
        check_maps(dev, ref)
        ro = D.compare_overlaps(s, t, list(Ts), thr)
        do = lgr.compare_overlaps(cuda(s), cuda(t), list(Ts), thr)
        check_overlaps(do, ro)
        return dev, do
    # NaN normals on some reference points: the squared-distance branch
    t_nan = tgt.copy()
    t_nan[::3, 4:7] = np.nan
    dev, _ = run(src, t_nan)
    nn = dev["src"]["nn"]
    hit = (nn >= 0) & (nn % 3 == 0)
    assert hit.any() and (dev["src"]["temp_normal"][hit] == F(np.pi / 2)).all()
    # NaN points on both sides: they neither ask nor answer
    s_bad, t_bad = src.copy(), tgt.copy()
    s_bad[len(src) // 2, :3] = (np.nan, np.inf, 0)
    t_bad[7, 1] = np.nan
    dev, do = run(s_bad, t_bad)
    assert dev["src"]["nn"][len(src) // 2] == -1 and 7 not in dev["src"]["nn"] and do["mask_src"][0][len(src) // 2] == 0 and do["mask_tgt"][0][7] == 0
    # clouds of one point
    run(src[:1], tgt)
    run(src, tgt[:1])
    run(src[:1], tgt[:1])
    # an overlap of 0 points and of exactly 1 point: weighted_count 0
    _, do = run(src, tgt, (pair["T_shift"],))
    assert do["counts"][0] == 0 and do["weighted"][0] == 0
    s1, t1 = src[:1].copy(), src[:1].copy()
    s1[0, 4:7] = (0, 1, 0)
    t1[0, 4:7] = (1, 0, 0); t1[0, 0] += 1.0
    ro = D.compare_overlaps(s1, t1, [np.eye(4, dtype=F)], 0.5)
    do = lgr.compare_overlaps(cuda(s1), cuda(t1), [np.eye(4, dtype=F)], 0.5)
    check_overlaps(do, ro)
    assert do["counts"][0] == 1 and do["weighted"][0] == 0
    # empty clouds: counts 0, nothing written
    for s, t in ((src[:0], tgt), (src, tgt[:0])):
        dev = lgr.temperature_maps(cuda(s), cuda(t), T, thr)
        assert dev["src"]["n_below"] == 0 and dev["tgt"]["n_below"] == 0 and len(dev["src"]["nn"]) == 0
        do = lgr.compare_overlaps(cuda(s), cuda(t), [T, T], thr)
        assert not do["counts"].any() and not do["weighted"].any()
        idx, d2 = lgr.nearest(cuda(tgt[:5]), cuda(t[:0]))
        assert (idx.cpu().numpy() == -1).all() and np.isinf(d2.cpu().numpy()).all()
    assert len(lgr.compare_overlaps(cuda(src), cuda(tgt), [], thr)["counts"]) == 0


def test_invalid_arguments(lgr, pair):
    from lgr_amd import capi
    src, tgt, T = pair["src"], pair["tgt"], pair["T"]
    for thr in (0.0, -1.0, float("nan"), 1e19):
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.temperature_maps(cuda(src), cuda(tgt), T, thr)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            lgr.compare_overlaps(cuda(src), cuda(tgt), [T], thr)
    corr = np.zeros(1, D.CORR_DTYPE)
    corr["index_query"] = 5
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.color_correspondences(5, None, corr, None, None, True)


@pytest.mark.parametrize("ns", [63, 64, 65, 255, 256, 257])
def test_sizes_across_launch_geometry(lgr, pair, ns):
    src, tgt, thr, T = pair["src"][:ns], pair["tgt"], pair["thr"], pair["T"]
    check_maps(lgr.temperature_maps(cuda(src), cuda(tgt), T, thr), D.temperature_maps(src, tgt, T, thr))
    Ts = [T, pair["T_far"]]
    check_overlaps(lgr.compare_overlaps(cuda(src), cuda(tgt), Ts, thr), D.compare_overlaps(src, tgt, Ts, thr))
    # and as the reference side of the search
    idx, d2 = lgr.nearest(cuda(tgt), cuda(src))
    ri, rd = D.nearest(tgt, src)
    assert np.array_equal(idx.cpu().numpy(), ri) and same_bits(d2.cpu().numpy(), rd)


def test_host_twins(lgr, pair):
    src, tgt, thr, T = pair["src"], pair["tgt"], pair["thr"], pair["T"]
    ref = D.temperature_maps(src, tgt, T, thr)
    check_maps(lgr.temperature_maps_host(src, tgt, T, thr), ref)
    check_side(lgr.temperature_map_host(ref["moved"], tgt, thr), ref["src"])
    Ts = [T, pair["T_far"]]
    dev = lgr.compare_overlaps(cuda(src), cuda(tgt), Ts, thr)
    host = lgr.compare_overlaps_host(src, tgt, Ts, thr)
    check_overlaps(host, dev)
    check_overlaps(host, D.compare_overlaps(src, tgt, Ts, thr))
    host = lgr.compare_overlaps_host(src, tgt, Ts, thr, with_masks=False)
    assert np.array_equal(host["counts"], dev["counts"])


def test_colour_passes(lgr, pair):
    rng = np.random.default_rng(3)
    # getColor over a range, its edges and outside it
    vmin, vmax = F(0.25), F(1.75)
    v = np.concatenate([rng.uniform(-0.5, 2.5, 1000).astype(F), [vmin, vmax, F(vmin + (vmax - vmin) / F(3)), F(np.nan), F(np.inf), F(-np.inf)]]).astype(F)
    ref = D.color_map(v, vmin, vmax)
    assert np.array_equal(lgr.color_map(cuda(v), vmin, vmax), ref) and np.array_equal(lgr.color_map_host(v, vmin, vmax), ref)
    assert np.array_equal(lgr.color_map(cuda(v[:3]), 1.0, 1.0), D.color_map(v[:3], 1.0, 1.0))   # vmin == vmax
    # saveColorizedWeights: the quantile range
    for n in (1, 2, 100, 1001):
        w = rng.standard_normal(n).astype(F)
        rc, rr = D.color_weights(w)
        for col, r in (lgr.color_map(cuda(w)), lgr.color_map_host(w)):
            assert same_bits(np.array(r, F), rr) and np.array_equal(col, rc), n
    # savePointCloudWithCorrespondences: point 0 is touched by three correct correspondences
    src = pair["src"]
    n = len(src)
    c = 600
    corr = np.zeros(c, D.CORR_DTYPE)
    corr["index_query"] = rng.integers(1, n, c); corr["index_match"] = rng.integers(0, n, c)
    corr["index_query"][:3] = 0
    correct = np.concatenate([corr[:3], corr[3:][rng.random(c - 3) < 0.3]])
    inl = corr[rng.random(c) < 0.4]
    kp = np.unique(rng.integers(0, n, 500)).astype(np.int32)
    for is_source in (True, False):
        for k in (kp, None):
            ref = D.color_correspondences(n, k, corr, correct, inl, is_source)
            assert np.array_equal(lgr.color_correspondences(n, k, corr, correct, inl, is_source), ref)
            assert np.array_equal(lgr.color_correspondences_host(n, k, corr, correct, inl, is_source), ref)
    ref = D.color_correspondences(n, kp, corr, correct, inl, True)
    assert ref[0] in (D.mix_color(D.COLOR_RED, times=3), D.mix_color(D.COLOR_BLUE, times=3))
    assert np.array_equal(lgr.color_correspondences(4, np.zeros(0, np.int32), None, None, None, True), [D.COLOR_PARAKEET] * 4)
    assert np.array_equal(lgr.color_correspondences(4, None, None, None, None, True), [D.COLOR_BEIGE] * 4)
