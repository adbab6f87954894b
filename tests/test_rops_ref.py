"""CPU: the RoPS reference of the tests (tests/cpp/rops_ref.cpp) and the arithmetic it shares with the kernels (csrc/lgr_rops_math.h).

- rows worked out by hand: two support points in general position fill two opposite corner cells of every distribution matrix, so
  every (rotation, projection) gives (+-4, 0, 0, 16, ln 2) before the L1 normalization; empty, single-point and NaN-frame supports
  give the zero row; regular rows have L1 norm 1;
- the restated logf equals the host's logf on every float of (0, 1]; the bin-index rule equals g++'s static_cast<unsigned>;
- gravity frames agree with a float64 evaluation, and the 0.04 rad switch is exercised on both sides."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rops_ref_lib as ref  # noqa: E402

ANGLES = np.radians([22.5, 45.0, 67.5])


def _rot(axis, th):
    c, s = np.cos(th), np.sin(th)
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def test_two_points_by_hand():
    rng = np.random.default_rng(11)
    for _ in range(20):
        a = rng.uniform(-1, 1, 3)
        pts = np.stack([np.zeros(3), a]).astype(np.float32)
        want = []
        for axis in range(3):
            for th in ANGLES:
                d = _rot(axis, th) @ pts[1].astype(np.float64)   # the second point minus the first, rotated
                for cu, cv in ((0, 1), (0, 2), (1, 2)):
                    s = 1.0 if (d[cu] > 0) == (d[cv] > 0) else -1.0
                    want += [4 * s, 0.0, 0.0, 16.0, np.log(2.0)]
        want = np.array(want)
        want /= np.abs(want).sum()
        got = ref.row(pts)
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
        assert abs(np.abs(got.astype(np.float64)).sum() - 1) < 1e-5


def test_degenerate_supports_give_the_zero_row():
    assert (ref.row(np.zeros((0, 3))) == 0).all()                       # empty support
    assert (ref.row(np.zeros((1, 3))) == 0).all()                       # the key point alone
    assert (ref.row(np.full((7, 3), 0.25)) == 0).all()                  # every point in one place
    # a NaN frame: every transformed coordinate NaN -> box untouched, every ratio NaN -> cell (0, 0) -> m = 1 -> zero moments
    surf = np.zeros((20, 12), np.float32)
    surf[:, :3] = np.random.default_rng(2).uniform(-0.1, 0.1, (20, 3))
    kps = surf[:3].copy()
    r = ref.rops(kps, surf, 1.0, np.full((3, 9), np.nan, np.float32))
    assert not np.isnan(r).any() and (r == 0).all()
    # a key point with no surface in reach, and a NaN key point
    far = kps.copy(); far[0, :3] = 50.0; far[1, :3] = np.nan
    r = ref.rops(far, surf, 1.0, np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (3, 1)))
    assert (r[:2] == 0).all()


def test_regular_rows_have_unit_l1_norm():
    rng = np.random.default_rng(3)
    surf = np.zeros((3000, 12), np.float32)
    surf[:, :3] = rng.uniform(-1, 1, (3000, 3))
    kps = surf[:200]
    fr = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (200, 1))
    r = ref.rops(kps, surf, 0.3, fr)
    l1 = np.abs(r.astype(np.float64)).sum(1)
    assert np.abs(l1 - 1).max() < 1e-5


def test_logf_restatement_equals_host_logf_on_all_of_0_1():
    bad = ref.count_logf_mismatch(0x00000001, 0x3F800000)
    print(f"rops_logf vs host logf on every float of (0, 1]: {bad} differences")
    assert bad == 0


def test_bin_rule_equals_gxx_static_cast():
    f32 = np.float32
    probes = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, 4.9999995, 5.0, np.nextafter(f32(5), f32(6)), 5.9999995, 6.0, 7.5,
              -0.5, -1.0, -1.5, 2.0 ** 32, 2.0 ** 32 + 2 ** 9, 3 * 2.0 ** 33, 2.0 ** 62, np.nextafter(f32(2 ** 63), f32(0)), 2.0 ** 63,
              -(2.0 ** 63), 1e30, -1e30, 1e-45]
    for x in probes:
        assert ref.bin_rule(f32(x)) == ref.cast_u32(f32(x)), x
    assert ref.cast_u32(f32(np.nan)) == 0 and ref.cast_u32(f32(np.inf)) == 0 and ref.cast_u32(f32(-np.inf)) == 0
    assert ref.cast_u32(np.nextafter(f32(5), f32(6))) == 5


def test_gravity_frames_float64_and_threshold():
    rng = np.random.default_rng(4)
    m = 2000
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    kps = np.zeros((m, 12), np.float32)
    kps[:, 4:7] = n
    fr, fail = ref.gravity_only(kps)
    ang = np.arccos(np.abs(np.clip(kps[:, 6].astype(np.float64), -1, 1)))
    ok = ~fail
    assert ok.sum() > 1900 and (ang[ok] > 0.04 - 1e-6).all()
    z = kps[ok, 4:7].astype(np.float64)
    y = np.cross([0.0, 0.0, 1.0], z)
    x = np.cross(y, z)
    np.testing.assert_allclose(fr[ok, 0:3], x, atol=1e-6)
    np.testing.assert_allclose(fr[ok, 3:6], y, atol=1e-6)
    assert (fr[ok, 6:9] == kps[ok, 4:7]).all()
    # the 0.04 rad switch on both sides (tilted normals 0.039 and 0.041 rad off the vertical, up and down), and NaN normals
    t = np.array([0.039, 0.041, 0.039, 0.041, 0.0, 0.2])
    sgn = np.array([1, 1, -1, -1, 1, -1])
    kp2 = np.zeros((8, 12), np.float32)
    kp2[:6, 4] = np.sin(t); kp2[:6, 6] = sgn * np.cos(t)
    kp2[6, 4:7] = np.nan; kp2[7, 4:7] = [np.nan, 0, 1]
    _, fail2 = ref.gravity_only(kp2)
    assert list(fail2) == [True, False, True, False, True, False, True, True]
