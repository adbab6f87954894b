"""GPU parity of the FPFH stage on small clouds built to reach the corners of its two kernels (lgr_features.hip): the weighting kernel's
candidate ring (whole rounds while a run streams, the remainder at its end), the SPFH kernel's per-tile bookkeeping (tile point by
readlane, neighbour count in a register) and the decision band of its bin filter (pair_bins_fast).

Bar: lgr.fpfh == oracle.fpfh bit for bit, NaN rows included; nothing is skipped or tolerated.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0.25
H = float(np.float32(1.001) * np.float32(R))     # cell size of the grid (lgr_grid_rule.h: h0 = fl(1.001f * r)); origin = the surface's bounding-box minimum


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows(xyz, nrm):
    from lgr_amd.synthetic import make_points
    p = make_points(np.asarray(xyz, np.float32))
    p[:, 4:7] = np.asarray(nrm, np.float32)
    return p


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def same_rows(lgr, oracle, kps, surf, r=R):
    want = oracle.fpfh(kps, surf, r)
    got = lgr.fpfh(cuda(kps), cuda(surf), r).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok])
    return want


# ---- 1. the weighting kernel's ring -----------------------------------------------------------------------------------------------------
COUNTS = (1, 3, 4, 15, 16, 17, 63, 64, 65, 130, 200)   # live candidates of a run; 130 and 200 wrap the 128-entry ring


def ring_cloud():
    """Isolated clusters, four cells apart, one per (count, layout): `count` surface points around the centre of a cell, either all inside
    that cell ("tight": the run's candidates arrive in chunks of 64, 64, ...) or in a ball of 0.9 r over the 27 cells ("wide": nine short
    chunks whose remainders carry over from one to the next), and five key points within 0.02 h of the centre: one run (same cell) whose
    bounding box every point of the cluster is within r of -- so the run's live candidates are exactly `count`.  Five key points per cell
    make every 16-key-point tile straddle at least three cells.  A surface point at the origin pins the grid's origin."""
    rng = np.random.default_rng(20)
    surf, nrm, kps, live = [np.zeros((1, 3))], [np.array([[0.0, 0.0, 1.0]])], [], []
    k = 0
    for layout in ("tight", "wide"):
        for n in COUNTS:
            centre = (np.array([4 + 4 * (k % 5), 4 + 4 * (k // 5), 4]) + 0.5) * H
            k += 1
            d = unit(rng.normal(size=(n, 3))) * (rng.uniform(0.05, 1.0, (n, 1)) ** (1 / 3))
            pts = centre + d * (0.3 * H if layout == "tight" else 0.9 * R)
            kp = centre + rng.uniform(-0.02, 0.02, (5, 3)) * H
            assert (np.floor(kp / H) == np.floor(centre / H)).all()
            if layout == "tight":
                assert (np.floor(pts / H) == np.floor(centre / H)).all()
            else:
                assert n < 15 or len(np.unique(np.floor(pts / H), axis=0)) > 3
            assert (np.linalg.norm(pts[None] - kp[:, None], axis=2).min(0) < 0.95 * R).all()   # every point is some key point's neighbour
            surf.append(pts); nrm.append(unit(rng.normal(size=(n, 3)))); kps.append(kp); live.append(n)
    # a cluster whose points are all between 1.2 r and 1.4 r from its key point: candidates are streamed, none is accepted -> NaN row
    centre = (np.array([4 + 4 * (k % 5), 4 + 4 * (k // 5), 4]) + 0.5) * H
    far = centre + unit(rng.normal(size=(40, 3))) * rng.uniform(1.2, 1.4, (40, 1)) * R
    surf.append(far); nrm.append(unit(rng.normal(size=(40, 3)))); kps.append(centre[None])
    kps.append(np.array([[30 * H, 2 * H, 2 * H]]))            # a key point in an empty corner of the grid -> NaN row
    kps.append(np.array([[np.nan, 1.0, 1.0]]))                # a non-finite key point -> NaN row
    kp_rows = rows(np.concatenate(kps), np.zeros((sum(len(q) for q in kps), 3)))
    return kp_rows, rows(np.concatenate(surf), np.concatenate(nrm)), live


def test_ring_carry_over(lgr, oracle):
    kps, surf, live = ring_cloud()
    m = len(kps)
    assert m % 16 != 0 and m > 64 and set(live) == set(COUNTS) and max(live) >= 130 and min(live) < 4
    want = same_rows(lgr, oracle, kps, surf)
    # the three key points without a neighbour (and only they) have NaN rows; every other row is a real histogram
    assert np.isnan(want[-3:]).all() and not np.isnan(want[:-3]).any()
    blocks = want[:-3].reshape(-1, 3, 11).sum(2)
    assert np.allclose(blocks[blocks.sum(1) > 0], 100, atol=1e-2)
    # the surface against itself: SPFH tiles that straddle the clusters, rows for the surface's own 16-point tiles
    same_rows(lgr, oracle, surf, surf)


# ---- 2. the SPFH kernel's tile point and neighbour count ------------------------------------------------------------------------------
def test_tile_points_in_sixteen_cells_and_duplicates(lgr, oracle):
    """A 6 x 6 x 6 lattice of pitch h with every point 0.05 .. 0.3 h inside its own cell: the 16 points of every SPFH tile lie in 16
    different cells (16 runs of one point per wave), neighbours are the lattice neighbours closer than r.  Exact duplicates (a pair and a
    triple; the copies count in k but give no pair features) sit in the lattice, 216 + 3 + 2 points: the last tile is partly beyond g.n
    and the grid's rounded-up launch has tiles that lie beyond it altogether."""
    rng = np.random.default_rng(21)
    ijk = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    xyz = (ijk + rng.uniform(0.05, 0.3, ijk.shape)) * H
    xyz[0] = 0.0                                                     # pins the origin
    assert len(np.unique(np.floor(xyz / H), axis=0)) == len(xyz)
    xyz = np.concatenate([xyz, xyz[[40, 40, 41]], xyz[[100, 215]]])  # a triple, a pair, and two more pairs
    nrm = unit(rng.normal(size=xyz.shape))
    surf = rows(xyz, nrm)
    assert len(surf) % 16 != 0
    d = np.linalg.norm(xyz[:, None].astype(np.float32) - xyz[None].astype(np.float32), axis=2)
    k = (d < R).sum(1)
    assert (k >= 3).mean() > 0.5 and (d[216:, :216] == 0).sum() == 5   # most points have neighbours (a few have none: k == 1); the copies are exact
    want = same_rows(lgr, oracle, surf, surf)
    assert not np.isnan(want).any()


# ---- 3. the decision band of the bin filter ------------------------------------------------------------------------------------------
def lattice(tilt, rng):
    """24 x 24 points of pitch r / 4 in the plane z = 0; normals (0, 0, 1) tilted by `tilt` rad towards a random azimuth"""
    ij = np.stack(np.meshgrid(np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([ij * (R / 4), np.zeros((len(ij), 1))], 1)
    phi = rng.uniform(0, 2 * np.pi, len(ij))
    nrm = np.stack([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.full(len(ij), np.cos(tilt))], 1)
    return rows(xyz, nrm)


@pytest.mark.parametrize("tilt", [0.0, 1e-7, 1e-6, 1e-5])
def test_flat_lattice_falls_back(lgr, oracle, tilt):
    """tilt 0: d is perpendicular to both normals, |angle1| == |angle2| == 0 for every pair -- no swap decision is certain, every pair takes
    the canonical sequence.  With the normals tilted the two magnitudes differ by up to 2 * tilt: below, around (1e-6) and above the
    2 DA = 2e-6 the filter asks for."""
    surf = lattice(tilt, np.random.default_rng(22))
    if tilt == 0.0:
        assert (surf[:, 4:7] == np.float32([0, 0, 1])).all()
    want = same_rows(lgr, oracle, surf, surf)
    assert not np.isnan(want).any()


def test_neighbours_along_the_normal(lgr, oracle):
    """Columns of points along z whose lateral offsets are below 1e-3 of their spacing: every neighbour direction is within 1e-3 rad of
    the even points' normals (0, 0, 1) (small |d x n|: vn2 ~ 1e-6 |d|^2); the odd points' normals are the direction of d x n to the point
    below, perpendicular to it (xx ~ 0, yy ~ 0: small rho2).  A few normals are not unit (length 1.5, 0): the filter's error budget is
    written for unit normals."""
    rng = np.random.default_rng(23)
    s = R / 12
    xyz, nrm = [], []
    for c in range(8):
        base = np.array([5 * H * (c % 4), 5 * H * (c // 4), 0.0])
        p = base + np.concatenate([rng.uniform(-1e-3, 1e-3, (40, 2)) * s, (np.arange(40) * s)[:, None]], 1)
        n = np.tile([0.0, 0.0, 1.0], (40, 1))
        for j in range(1, 40, 2):
            v = np.cross(p[j] - p[j - 1], [0.0, 0.0, 1.0])
            n[j] = unit(v) if np.linalg.norm(v) > 0 else [1.0, 0.0, 0.0]
        xyz.append(p); nrm.append(n)
    xyz, nrm = np.concatenate(xyz), np.concatenate(nrm)
    xyz[0] = 0.0
    nrm[10] *= 1.5; nrm[50] *= 1.5; nrm[90] = 0.0
    surf = rows(xyz, nrm)
    same_rows(lgr, oracle, surf, surf)
