"""CPU: the statement tests/cpp/debug_ref.cpp (temperature maps, overlap comparison, far-safe nearest neighbour, colour passes) against an
independent numpy formulation on a few hundred points, and getColor / mixPointColor / quantile at their edges."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_ref_lib as D  # noqa: E402

F = np.float32


def cloud(n, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 12), F)
    c[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    c[:, 2] = 0.2 * np.sin(3 * c[:, 0]) + 0.02 * rng.standard_normal(n)
    nrm = rng.standard_normal((n, 3)) * 0.2 + np.array([0, 0, 1.0])
    c[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    c[:, 3] = 1
    c[:, 8] = rng.uniform(0, 0.1, n)
    return c


def small_T(seed=3, t=0.02, ang=0.05):
    rng = np.random.default_rng(seed)
    ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    T[:3, 3] = t * rng.standard_normal(3)
    return T.astype(F)


# ---- the numpy formulation (vectorised, float32 throughout, the declared operation order) ----
def np_move(src, T):
    M = np.asarray(T, F)
    out = src.copy()
    p, n = src[:, :3], src[:, 4:7]
    for r in range(3):
        out[:, r] = M[r, 0] * p[:, 0] + (M[r, 1] * p[:, 1] + (M[r, 2] * p[:, 2] + M[r, 3]))
        out[:, 4 + r] = M[r, 0] * n[:, 0] + (M[r, 1] * n[:, 1] + M[r, 2] * n[:, 2])
    out[:, 3] = 1; out[:, 7] = 0
    return out


def np_d2(a, b):
    d = a[:, None, :3] - b[None, :, :3]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def np_nearest(q, pts, r2=None):
    """index of the minimum under (d2, index) (argmin takes the first of equal values), -1 where nothing qualifies"""
    d2 = np_d2(q, pts)
    ok = np.isfinite(pts[:, :3]).all(1)[None, :] & np.isfinite(q[:, :3]).all(1)[:, None]
    if r2 is not None:
        ok &= d2 < r2
    d2m = np.where(ok, d2, np.inf)
    j = np.argmin(d2m, axis=1)
    none = ~ok.any(1)
    # all-inf rows that still have a valid candidate (overflowed distances): the first valid one
    first_ok = np.argmax(ok, axis=1)
    j = np.where(np.isinf(d2m[np.arange(len(q)), j]) & ~none, first_ok, j)
    return np.where(none, -1, j).astype(np.int32), d2[np.arange(len(q)), j]


def np_plane_distance(p, q, d2):
    dp = np.abs((q[:, 4] * (q[:, 0] - p[:, 0]) + q[:, 5] * (q[:, 1] - p[:, 1])) + q[:, 6] * (q[:, 2] - p[:, 2]))
    return np.where(np.isfinite(dp), dp, d2).astype(F)


def np_get_color(v, vmin, vmax):
    v, vmin, vmax = F(v), F(vmin), F(vmax)
    dv = F(vmax - vmin)
    if vmax < v:
        v = vmax
    if not (vmin < v):
        v = vmin
    r = g = b = F(1)
    with np.errstate(all="ignore"):
        x = F(F(F(3) * F(v - vmin)) / dv)
        if v < F(vmin + F(dv / F(3))):
            b = F(F(1) - x)
        elif v < F(vmin + F(F(F(2) * dv) / F(3))):
            b = F(0); g = F(F(2) - x)
        else:
            b = F(0); g = F(0); r = F(F(3) - x)
    c8 = lambda c: 0 if np.isnan(c) else int(np.trunc(F(F(255) * c))) & 255   # noqa: E731
    return (c8(r) << 16) + (c8(g) << 8) + c8(b)


def np_temperature_map(cmp, ref, dmax):
    dmax = F(dmax)
    radius = F(2) * dmax
    j, d2 = np_nearest(cmp, ref, radius * radius)
    q = ref[np.maximum(j, 0)]
    dp = np.where(j >= 0, np_plane_distance(cmp, q, d2), dmax)
    below = dp < dmax
    td = np.where(below, dp, dmax).astype(F)
    cs = (q[:, 4] * cmp[:, 4] + q[:, 5] * cmp[:, 5]) + q[:, 6] * cmp[:, 6]
    with np.errstate(invalid="ignore"):
        nd = np.abs(np.arccos(np.clip(cs.astype(np.float64), -1, 1)))
    tmax = F(np.pi / 2)
    nd = np.where(np.isfinite(nd), np.minimum(nd, tmax), tmax)
    tn = np.where(below, nd, tmax).astype(F)
    return td, tn, j, int(below.sum())


def np_smoothed_densities(pts):
    d2 = np_d2(pts, pts)
    order = np.lexsort((np.broadcast_to(np.arange(len(pts)), d2.shape), d2), axis=1)   # ascending (d2, index) per row
    second = order[:, 1]
    dk = np.sqrt(d2[np.arange(len(pts)), second])
    return np.minimum(dk, dk[second])


def np_compare_overlaps(src, tgt, T, thr):
    al = np_move(src, T)
    masks = []
    for cmp, ref in ((al, tgt), (tgt, al)):
        j, d2 = np_nearest(cmp, ref)
        dp = np_plane_distance(cmp, ref[np.maximum(j, 0)], d2)
        masks.append((j >= 0) & (dp < F(thr)))
    ov = np.concatenate([al[masks[0]], tgt[masks[1]]])
    w = F(0)
    if len(ov) >= 2:
        dens = np_smoothed_densities(ov).astype(F)
        w = np.add.accumulate(dens * dens, dtype=F)[-1]
    return masks[0], masks[1], w


# ---- tests ----
@pytest.fixture(scope="module")
def pair():
    src, tgt = cloud(300, 1), cloud(340, 2)
    tgt[::7, 4:7] = np.nan           # invalid normals: the squared-distance branch
    src[5, :3] = np.nan              # a point that neither asks nor answers
    tgt[11, 0] = np.inf
    return src, tgt, small_T(), 0.08


def test_move_and_nearest(pair):
    src, tgt, T, _ = pair
    al = D.move(src, T)
    assert np.array_equal(D.bits(al), D.bits(np_move(src, T)))
    far = np.eye(4, dtype=F); far[:3, 3] = (40, -25, 10)
    for q in (al, D.move(src, far)):
        idx, d2 = D.nearest(q, tgt)
        j, e2 = np_nearest(q, tgt)
        assert np.array_equal(idx, j) and idx[5] == -1 and np.isinf(d2[5])
        assert np.array_equal(D.bits(d2[idx >= 0]), D.bits(e2[idx >= 0]))
        assert 11 not in idx


def test_temperature_map_against_numpy(pair):
    src, tgt, T, thr = pair
    r = D.temperature_maps(src, tgt, T, thr)
    al = np_move(src, T)
    for side, cmp, ref in (("src", al, tgt), ("tgt", tgt, al)):
        td, tn, j, nb = np_temperature_map(cmp, ref, thr)
        s = r[side]
        assert np.array_equal(s["nn"], j) and s["n_below"] == nb and nb >= len(cmp) // 10
        assert np.array_equal(D.bits(s["temp_distance"]), D.bits(td))
        assert np.allclose(s["temp_normal"], tn, rtol=0, atol=5e-7)   # acos: the host libm against float64 rounded once
        assert (s["temp_distance"] < F(thr)).sum() == nb
        assert np.array_equal(s["color_distance"], [np_get_color(v, 0, thr) for v in s["temp_distance"]])
        assert np.array_equal(s["color_normal"], [np_get_color(v, 0, F(np.pi / 2)) for v in s["temp_normal"]])
        assert (s["temp_normal"][s["temp_distance"] >= F(thr)] == F(np.pi / 2)).all()
    assert (r["src"]["nn"] >= 0).sum() > r["src"]["n_below"] > 0    # some neighbours are not below the threshold
    # the squared-distance branch was taken
    nn = r["src"]["nn"]
    assert np.isnan(tgt[nn[nn >= 0], 4]).any()
    one = D.temperature_map(al, tgt, thr)
    for k in D.TEMP_FIELDS:
        assert np.array_equal(one[k].view(np.uint32), r["src"][k].view(np.uint32))


def test_compare_overlaps_against_numpy(pair):
    src, tgt, T, thr = pair
    far = np.eye(4, dtype=F); far[:3, 3] = (40, -25, 10)
    Ts = [T, np.eye(4, dtype=F), far]
    r = D.compare_overlaps(src, tgt, Ts, thr)
    for k, Tk in enumerate(Ts):
        ms, mt, w = np_compare_overlaps(src, tgt, Tk, thr)
        assert np.array_equal(r["mask_src"][k].astype(bool), ms) and np.array_equal(r["mask_tgt"][k].astype(bool), mt)
        assert r["counts"][k] == ms.sum() + mt.sum() and tuple(r["counts2"][k]) == (ms.sum(), mt.sum())
        assert D.bits(r["weighted"][k]) == D.bits(w), (k, r["weighted"][k], w)
    assert r["counts"][0] >= 60 and r["counts"][2] == 0 and r["weighted"][2] == 0
    # an overlap of exactly one point is declared 0
    one = D.compare_overlaps(src[:1], tgt[:1] * 0 + src[:1], [np.eye(4, dtype=F)], thr)
    assert one["counts"][0] == 2
    s1, t1 = src[:1].copy(), src[:1].copy()
    t1[0, 4:7] = (1, 0, 0); t1[0, 0] += 1.0     # the target a unit away along its own normal, the source's normal across: only one side passes
    s1[0, 4:7] = (0, 1, 0)
    one = D.compare_overlaps(s1, t1, [np.eye(4, dtype=F)], 0.5)
    assert one["counts"][0] == 1 and one["weighted"][0] == 0


def test_get_color_edges():
    vmin, vmax = F(0.25), F(1.75)
    dv = F(vmax - vmin)
    t1, t2 = F(vmin + F(dv / F(3))), F(vmin + F(F(F(2) * dv) / F(3)))
    vals = [vmin, vmax, t1, np.nextafter(t1, F(-9)), np.nextafter(t1, F(9)), t2, np.nextafter(t2, F(-9)), np.nextafter(t2, F(9)), F(-5), F(7), F(np.nan),
            F(np.inf), F(-np.inf), F(1.0)]
    for v in vals:
        assert D.get_color(v, vmin, vmax) == np_get_color(v, vmin, vmax), v
    assert D.get_color(vmin, vmin, vmax) == 0xffffff and D.get_color(vmax, vmin, vmax) == 0x000000
    assert D.get_color(-5, vmin, vmax) == 0xffffff and D.get_color(7, vmin, vmax) == 0 and D.get_color(np.nan, vmin, vmax) == 0xffffff
    assert D.get_color(np.nextafter(t1, F(-9)), vmin, vmax) >> 16 == 0xff and D.get_color(t2, vmin, vmax) & 0xffff == 0
    rng = np.random.default_rng(0)
    v = rng.uniform(-0.5, 2.5, 500).astype(F)
    assert np.array_equal(D.color_map(v, vmin, vmax), [np_get_color(x, vmin, vmax) for x in v])
    assert D.get_color(1.0, 1.0, 1.0) == np_get_color(1.0, 1.0, 1.0) == 0      # vmin == vmax: NaN channel, declared 0


def test_mix_color_zero_to_three_times():
    exp = {0: D.COLOR_RED, 1: 0xfe7f7f, 2: 0xfebebe, 3: 0xfedede}
    for k, e in exp.items():
        assert D.mix_color(D.COLOR_RED, D.COLOR_WHITE, k) == e
    assert D.mix_color(0, D.COLOR_WHITE, 8) == D.mix_color(0, D.COLOR_WHITE, 50) == 0xfdfdfd    # the fixed point is reached after 8 steps
    assert D.mix_color(0xffffff, D.COLOR_WHITE, 8) == D.mix_color(0xffffff, D.COLOR_WHITE, 9) == 0xfefefe
    for c in range(256):
        assert D.mix_color(c, D.COLOR_WHITE, 8) == D.mix_color(c, D.COLOR_WHITE, 9)
    # the colour pass: a point touched by three correct correspondences, one by none
    corr = np.zeros(5, D.CORR_DTYPE)
    corr["index_query"] = [0, 0, 0, 1, 2]; corr["index_match"] = [3, 2, 1, 0, 0]
    col = D.color_correspondences(4, np.array([3], np.int32), corr, corr[:3], corr[3:4], True)
    assert list(col) == [D.mix_color(D.COLOR_RED, times=3), D.COLOR_BLUE, D.COLOR_RED, D.COLOR_BEIGE]
    col = D.color_correspondences(4, None, corr, corr[:3], corr[3:4], False)
    assert list(col) == [D.COLOR_BLUE, D.mix_color(D.COLOR_RED), D.mix_color(D.COLOR_RED), D.mix_color(D.COLOR_RED)]
    assert list(D.color_correspondences(3, np.array([1], np.int32), None, None, None, True)) == [D.COLOR_PARAKEET, D.COLOR_BEIGE, D.COLOR_PARAKEET]


@pytest.mark.parametrize("n", [1, 2, 100])
def test_quantile(n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(F)
    s = np.sort(v)
    for q in (0.01, 0.99, 0.8):
        i = int(np.floor(q * (n - 1))); j = min(i + 1, n - 1)
        exp = s[i] if (n == 1 or i == j) else F(float(s[i]) * (n * q - i) + float(s[j]) * (j - n * q))
        assert D.bits(D.quantile(q, v)) == D.bits(exp), (q, n)
    col, r = D.color_weights(v)
    assert D.bits(r[0]) == D.bits(D.quantile(0.01, v)) and D.bits(r[1]) == D.bits(D.quantile(0.99, v))
    assert np.array_equal(col, [np_get_color(x, r[0], r[1]) for x in v])
    assert np.isnan(D.quantile(0.5, np.zeros(0, F))) and np.isnan(D.quantile(1.5, v))
