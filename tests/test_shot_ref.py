"""CPU: the SHOT reference of the tests (tests/cpp/shot_ref.cpp) and the arithmetic it shares with the kernels (csrc/lgr_shot_math.h).

- fdlibm's acos / atan2 restated against the host's libm on 10^7 arguments plus edge cases: at most 1 ulp apart,
  the count of non-identical results printed;
- properties of the reference: unit rows, NaN rows below 5 neighbours and for NaN frames, invariance under a rigid motion (every key
  point whose frame is decided with a margin), orthonormal right-handed frames;
- the 352-d canonical distance equals a numpy emulation of OpenCV's SSE lane order bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shot_ref_lib as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulps(a, b):
    ia = a.view(np.int64).copy(); ib = b.view(np.int64).copy()
    ia = np.where(ia < 0, np.int64(-0x8000000000000000) - ia, ia)
    ib = np.where(ib < 0, np.int64(-0x8000000000000000) - ib, ib)
    return np.abs(ia - ib)


def test_acos_within_one_ulp_of_libm():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-1, 1, 7_000_000), rng.uniform(-1e-3, 1e-3, 1_500_000),
                        1 - rng.uniform(0, 1e-6, 750_000), -1 + rng.uniform(0, 1e-6, 750_000),
                        np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300])])
    a, b = ref.acos(x), ref.acos(x, "libm")
    u = _ulps(a, b)
    print(f"acos: {x.size} arguments, {int((u != 0).sum())} not identical to libm, max {int(u.max())} ulp")
    assert u.max() <= 1
    edge = np.array([0.0, -0.0, 1.0, -1.0])
    assert (ref.acos(edge) == np.arccos(edge)).all()


def test_atan2_within_one_ulp_of_libm():
    rng = np.random.default_rng(2)
    n = 10_000_000
    y = rng.uniform(-1, 1, n) * np.where(rng.random(n) < 0.2, 1e6, 1.0)
    x = rng.uniform(-1, 1, n) * np.where(rng.random(n) < 0.2, 1e-9, 1.0)
    ax = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e-300, 1e300])
    ey, ex = np.meshgrid(ax, ax)
    y = np.concatenate([y, ey.ravel()]); x = np.concatenate([x, ex.ravel()])
    a, b = ref.atan2(y, x), ref.atan2(y, x, "libm")
    u = _ulps(a, b)
    print(f"atan2: {x.size} arguments, {int((u != 0).sum())} not identical to libm, max {int(u.max())} ulp")
    assert u.max() <= 1
    zy, zx = np.meshgrid(ax[:4], ax[:4])                       # signs of zero and the axes: identical, sign of a zero result included
    a, b = ref.atan2(zy.ravel(), zx.ravel()), np.arctan2(zy.ravel(), zx.ravel())
    assert (a.view(np.int64) == b.view(np.int64)).all()


def _patch():
    d = np.load(os.path.join(ROOT, "tests", "golden", "patch2k.npz"))
    return d["surf_normals"].astype(np.float32), float(d["radius"])


def test_reference_rows_are_unit_and_frames_orthonormal():
    surf, r = _patch()
    rows, fr = ref.shot(surf, surf, r)
    ok = np.isfinite(rows).all(1)
    assert ok.sum() > 0.9 * len(rows)
    assert np.abs(np.linalg.norm(rows[ok].astype(np.float64), axis=1) - 1).max() <= 1e-6
    F = fr[ok].reshape(-1, 3, 3).astype(np.float64)
    assert np.abs(F @ F.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-5
    assert np.abs(np.linalg.det(F) - 1).max() <= 1e-5      # right-handed: y = z x x
    assert (rows[ok] >= 0).all()


def test_reference_nan_rows():
    surf, r = _patch()
    far = surf[:6].copy()
    far[:, :3] += 1000.0                                    # isolated key points: no neighbour at all
    rows, fr = ref.shot(far, surf, r)
    assert np.isnan(rows).all() and np.isnan(fr).all()
    # exactly 4 neighbours on the surface (the key point itself included): NaN frame and NaN row; 5 distinct ones + the key point: a frame
    rng = np.random.default_rng(3)
    base = np.zeros((6, 12), np.float32); base[:, 3] = 1; base[:, 6] = 1
    base[1:, :3] = rng.uniform(-0.3, 0.3, (5, 3))
    rows4, fr4 = ref.shot(base[:1], base[:4], 1.0)
    assert np.isnan(rows4).all() and np.isnan(fr4).all()
    rows6, fr6 = ref.shot(base[:1], base, 1.0)
    assert np.isfinite(fr6).all() and np.isfinite(rows6).all()
    # a given NaN frame: NaN row
    rows_n, _ = ref.shot(surf[:3], surf, r, lrf=np.full((3, 9), np.nan, np.float32))
    assert np.isnan(rows_n).all()


def test_reference_rigid_motion_invariance():
    surf, r = _patch()
    rng = np.random.default_rng(4)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = rng.uniform(-5, 5, 3)
    moved = surf.copy()
    moved[:, :3] = (surf[:, :3].astype(np.float64) @ q.T + t).astype(np.float32)
    moved[:, 4:7] = (surf[:, 4:7].astype(np.float64) @ q.T).astype(np.float32)
    a, _ = ref.shot(surf, surf, r)
    b, _ = ref.shot(moved, moved, r)
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    assert ok.mean() > 0.9
    diff = np.where(ok, np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max(1), np.inf)
    # SHOT is invariant through its frame.  Where rounding of the moved coordinates decides the frame -- two nearly equal eigenvalues (the
    # patch's flat parts), a sign vote at its tie -- the row changes as a whole; that is SHOT's own ambiguity, not an error.  Every key point
    # whose frame is decided with a margin (eigenvalue gaps above 2 % of the largest, both sign votes at least 2 from the tie) must agree
    # within 1e-5, and those must be most key points.
    M = ref.frame_margins(surf, surf, r)
    gap = np.minimum(M[:, 2] - M[:, 1], M[:, 1] - M[:, 0]) / M[:, 2]
    with np.errstate(invalid="ignore"):
        decided = ok & (gap > 0.02) & (np.abs(M[:, 3]) >= 2) & (np.abs(M[:, 4]) >= 2)
    print(f"rigid motion: {np.mean(diff[ok] <= 1e-5):.4f} of {ok.sum()} rows within 1e-5; {decided.sum()} decided frames, worst {diff[decided].max():.3g}")
    assert decided.sum() > 0.75 * len(a), decided.sum()
    assert (diff[decided] <= 1e-5).all(), np.flatnonzero(decided & (diff > 1e-5))[:10]
    c, _ = ref.shot(surf, surf, r)                             # and the same cloud twice: bit-identical
    assert (np.isnan(a) == np.isnan(c)).all() and (a[ok].view(np.uint32) == c[ok].view(np.uint32)).all()


def _l2sqr_sse(a, b):
    t = (a - b).astype(np.float32).reshape(22, 4, 4)           # [block][k][lane]
    acc = np.zeros((4, 4), np.float32)
    for blk in range(22):
        acc = (t[blk] * t[blk]).astype(np.float32) + acc
    s = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    return np.float32((s[0] + s[2]) + (s[1] + s[3]))


def test_canonical_distance_equals_the_sse_lane_order():
    rng = np.random.default_rng(5)
    for _ in range(300):
        a = rng.random(352).astype(np.float32); b = rng.random(352).astype(np.float32)
        a /= np.float32(np.linalg.norm(a)); b /= np.float32(np.linalg.norm(b))
        assert ref.l2sqr(a, b).view(np.uint32) == _l2sqr_sse(a, b).view(np.uint32)


def test_reference_matcher_tie_rule():
    rng = np.random.default_rng(6)
    t = rng.random((40, 352)).astype(np.float32)
    t[25] = t[3]; t[7] = t[3]                                 # the same row in blocks 0, 0 and 2 (block 10)
    idx, dist = ref.match(t[3:4], t, 10)
    assert idx[0] == 25 and dist[0] == 0                       # the later block wins a tie
    idx, _ = ref.match(t[3:4], t[:20], 10)
    assert idx[0] == 3                                         # inside a block the lower index
    q = t[:2].copy(); q[1, 5] = np.nan
    idx, _ = ref.match(q, t, 10)
    assert idx[1] == -1
