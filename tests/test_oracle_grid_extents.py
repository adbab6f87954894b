"""The oracle's neighbourhood searches on stretched and lopsided bounding boxes (tests/grid_extents_lib.py), so that its grid is right
before tests/test_gpu_grid_extents.py compares the device with it.  No GPU.

* the scenes reach what they are built for: cell counts at the caller's cell, and the doublings the rule of DESIGN.md section 4 gives;
* no stray is anyone's neighbour, so what does not depend on the grid equals the `room` result bit for bit for every blob query: FPFH in
  PCL's arithmetic (neighbours by ascending distance), evaluate_plane's pairs, match_local;
* against brute force: every radius search of match_local finds exactly numpy's candidates' best, and `thin`'s constructed pair -- within
  the radius, two cells apart at the cell the caller asked for -- is found;
* the ring searches (knn, smoothed_densities, normals) against numpy's lexsort on (d2, index) on room, thin and flat, with the cloud's
  own points as queries;
* the ring searches away from there: queries on and outside the cloud's box (26 directions, three separations, the two corners), clouds of
  one to five points and of 70 coincident points plus one with k up to more than n, and queries up to 1e5 -- more than 2^31 cells --
  from a one-point cloud.  Lists against numpy bit for bit, and the walk's cost (orc::Grid::knn's visit counter) against what the grid's
  dims and the query's cell allow: the walk of orc_grid.h, as lgr_knn_query on the device, visits only cells that exist, from the first
  ring that touches the grid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_extents_lib as G  # noqa: E402

F = np.float32
SCENES = [("room", 0.25), ("room", 0.1), ("gap", 0.25), ("over", 0.25), ("many", 0.1), ("thin", 0.1), ("flat", 0.1)]
STRETCHED = [s for s in SCENES if s[0] != "room"]
DOUBLINGS = dict(room=0, gap=0, over=1, many=8, thin=1, flat=3)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def world(oracle):
    b = G.blob(oracle)
    con = G.constructed(b, 0.1)
    w = dict(blob=b, con=con, kps_blob=b[::13].copy(), scene={})
    for name, r in SCENES:
        extra = np.concatenate([con["p"][None], con["cluster"]]) if name == "thin" else None
        cloud = G.scene(b, name, r, extra)
        q = np.stack([con["q"], con["qc"]]) if name == "thin" else np.zeros((0, 12), F)
        h, d, k = G.check_scene(name, cloud, r, queries=np.concatenate([b, q]))
        assert k == DOUBLINGS[name], (name, r, h, d, k)
        w["scene"][(name, r)] = cloud
    return w


@pytest.fixture()
def pcl_oracle(oracle):
    oracle.set_arith_mode(oracle.ARITH_PCL)
    yield oracle
    oracle.set_arith_mode(oracle.ARITH_CANONICAL)


def test_scenes_reach_both_conditions_of_the_rule(world):
    """thin doubles by the per-axis bound alone (its box is below the cell cap); over, many and flat by the cap"""
    b = world["blob"]
    for name, r in SCENES:
        h0 = G.cell(r)
        d = G.dims(world["scene"][(name, r)][:, :3], h0)
        cells = float(d[0]) * float(d[1]) * float(d[2])
        assert (cells > G.MAX_CELLS) == (name in ("over", "many", "flat")), (name, d)
        assert (d.max() > G.MAX_DIM_H0) == (name in ("many", "thin", "flat")), (name, d)
    assert len(b) == G.N_BLOB


@pytest.mark.parametrize("name,r", STRETCHED, ids=[n for n, _ in STRETCHED])
def test_strays_change_nothing_for_the_blob(pcl_oracle, world, name, r):
    o = pcl_oracle
    b, kps = world["blob"], world["kps_blob"]
    room, cloud = world["scene"][("room", r)], world["scene"][(name, r)]
    want, got = o.fpfh(kps, room, r), o.fpfh(kps, cloud, r)
    assert np.isfinite(want).all() and np.array_equal(bits(got), bits(want))
    T = G.small_transform(0.01)
    rng = np.random.default_rng(3)
    qf, tf = rng.uniform(0, 100, (len(b), 33)).astype(F), rng.uniform(0, 100, (len(cloud), 33)).astype(F)
    wi, wd = o.match_local(b, room, qf, tf[: len(room)], T, r)
    gi, gd = o.match_local(b, cloud, qf, tf, T, r)
    assert (wi >= 0).all() and np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd))
    # evaluate_plane's threshold is the 0.8 quantile of the smoothed 8-NN distances over ALL target points: more than one added point moves
    # the quantile's rank (int(0.8f n - 1)), so a borderline point may change sides; the nearest target of an inlier under both does not
    pa = dict(map(tuple, o.evaluate_plane(b, room, T, 0, with_pairs=True)["pairs"]))
    pb = dict(map(tuple, o.evaluate_plane(b, cloud, T, 0, with_pairs=True)["pairs"]))
    both = set(pa) & set(pb)
    assert len(both) > 5 and all(pa[i] == pb[i] for i in both)


@pytest.mark.parametrize("name,r", SCENES, ids=[f"{n}-{r}" for n, r in SCENES])
def test_match_local_equals_brute_force(oracle, world, name, r):
    """match_local: among the targets within r of T q (strict, float32 d2), the one with the nearest descriptor; here the statement is the
    candidate SET, which numpy finds by brute force: the match is a member, and a query has a match exactly when the set is not empty"""
    b, cloud = world["blob"], world["scene"][(name, r)]
    T = np.eye(4, dtype=F)
    rng = np.random.default_rng(4)
    q = b[::5]
    qf, tf = rng.uniform(0, 100, (len(q), 33)).astype(F), rng.uniform(0, 100, (len(cloud), 33)).astype(F)
    idx, _ = oracle.match_local(q, cloud, qf, tf, T, 0.1 * r)        # about eight candidates per query
    inside = G.d2_f32(q, cloud) < F(F(0.1 * r) * F(0.1 * r))
    assert np.array_equal(idx >= 0, inside.any(1))
    assert inside[np.arange(len(q)), np.maximum(idx, 0)][idx >= 0].all()
    cnt = oracle.iss_keypoints(cloud, 0.1 * r, min_neighbors=1, gamma21=1e30, gamma32=1e30)
    assert len(cnt) > 0


def test_constructed_pair_is_found(oracle, world):
    r = 0.1
    cloud, con = world["scene"][("thin", r)], world["con"]
    h0, r2, ox, ip = G.cell(r), F(F(r) * F(r)), cloud[:, 0].min(), G.N_BLOB
    assert np.array_equal(cloud[ip], con["p"]) and np.array_equal(cloud[ip + 1: ip + 6], con["cluster"])
    for q, lo, hi in ((con["q"], ip, ip + 1), (con["qc"], ip + 1, ip + 6)):
        d2 = G.d2_f32(q[None], cloud)[0]
        assert list(np.flatnonzero(d2 < 4 * r2)) == list(range(lo, hi)) and (d2[lo:hi] < r2).all()
        assert (G.cellc(q[0], ox, h0) - G.cellc(cloud[lo:hi, 0], ox, h0) == 2).all()
    rows = oracle.fpfh(np.stack([con["q"], con["qc"]]), cloud, r)
    assert not np.isnan(rows).any(), "fpfh: a key point's only neighbours, two cells away at the caller's cell, were not found"
    rng = np.random.default_rng(5)
    qf, tf = rng.uniform(0, 100, (2, 33)).astype(F), rng.uniform(0, 100, (len(cloud), 33)).astype(F)
    idx, _ = oracle.match_local(np.stack([con["q"], con["qc"]]), cloud, qf, tf, np.eye(4, dtype=F), r)
    assert idx[0] == ip and ip + 1 <= idx[1] <= ip + 5


@pytest.mark.parametrize("name", ["room", "thin", "flat"])
def test_ring_searches_equal_numpy(oracle, world, name):
    cloud = world["scene"][(name, 0.1)]
    for k in (8, 40):
        want_i, want_d = G.knn_numpy(cloud, cloud, k)
        idx, d2 = oracle.knn(cloud, cloud, k)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(bits(d2), bits(want_d))
        dk = np.sqrt(want_d[:, k - 1])
        np.testing.assert_array_equal(bits(oracle.smoothed_densities(cloud, k)), bits(np.minimum(dk, dk[want_i[:, 1]])))
    nb = G.N_BLOB
    assert np.array_equal(bits(oracle.normals_knn(cloud, 30)[:nb, 4:7]), bits(oracle.normals_knn(world["scene"][("room", 0.1)], 30)[:nb, 4:7]))


# ---- ring searches outside the cloud's box, on tiny clouds and far from them ----------------------------------------------------------
def check_walk(oracle, q, cloud, k):
    """oracle.knn(q, cloud, k) == numpy bit for bit, on the grid numpy arrives at, and per query within the cost the grid allows:

        rings walked          == last - first + 1                       (G.ring_walk: from the dims, the query's cell and the rule's end)
        cells examined        == C, the in-grid cells of those rings     (each exactly once: nothing outside the grid, nothing twice)
        z and y iterations    <= 3 C + rings                             (a row visited holds a cell of its ring; one jump per z, one per ring)

    so the work per query, iterations + cells, is at most 4 C + rings: the in-grid cells of the rings walked plus the rings walked, up to
    the constant.  C is at most the whole grid and the rings at most the longest axis, wherever the query lies."""
    want_i, want_d = G.knn_padded(q, cloud, k)
    idx, d2, visits, (h, origin, dims) = oracle.knn(q, cloud, k, visits=True)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(bits(d2), bits(want_d))
    wh, wo, wd = G.grid_of(cloud, 4.0)
    assert bits(h) == bits(wh) and np.array_equal(bits(origin), bits(wo)) and list(dims) == list(wd), (h, origin, dims, wh, wo, wd)
    walk = G.ring_walk(q, cloud, k, h, origin, dims)
    first, last, cells = walk[:, 0], walk[:, 1], walk[:, 2]
    rings = last - first + 1
    np.testing.assert_array_equal(visits[:, 2], rings)
    np.testing.assert_array_equal(visits[:, 1], cells)
    assert (visits[:, 0] <= 3 * cells + rings).all(), (visits[visits[:, 0] > 3 * cells + rings], k)
    assert (cells <= int(dims[0]) * int(dims[1]) * int(dims[2])).all() and (rings <= max(dims)).all()
    return want_i, want_d, walk


@pytest.mark.parametrize("k", [8, 30])
def test_outside_queries_equal_numpy_at_bounded_cost(oracle, world, k):
    b = world["blob"]
    q = G.outside_queries(b)
    assert len(q) == 80
    mn, mx = b[:, :3].min(0), b[:, :3].max(0)
    assert ((q[:78, :3] < mn) | (q[:78, :3] > mx)).any(1).all(), "a query meant to lie outside the box lies inside it"
    _, _, walk = check_walk(oracle, q, b, k)
    assert (walk[:78:3, 0] <= 1).all() and (walk[2:78:3, 0] >= 5).all(), "the separations reach neither the first ring outside nor a gap of several"
    assert (walk[78:, 0] == 0).all()                                # the corners are points of the box


TINY = ["one", "two_same", "two", "line3", "plane5", "same70"]


@pytest.mark.parametrize("name", TINY)
def test_tiny_clouds_equal_numpy_at_bounded_cost(oracle, name):
    cloud = G.tiny_clouds()[name]
    n = len(cloud)
    h = G.auto_cell(cloud, 4.0)
    if name in ("one", "two_same"):
        assert h == (F(1) if name == "one" else max(np.sqrt(F(F(F(1e-12) * F(4)) / F(2))), F(1e-6)))   # nothing to measure: the floors
    q = G.tiny_queries(cloud, h)
    for k in (1, 2, 8):
        want_i, want_d, walk = check_walk(oracle, q, cloud, k)
        assert (want_i[:, min(k, n):] == -1).all() and np.isinf(want_d[:, min(k, n):]).all()
        assert walk[:, 0].max() >= 190, "no query is some 200 cells from the grid"
        if name == "same70":                                        # equal distances: the lower index first
            np.testing.assert_array_equal(want_i[:70], np.tile(np.arange(k, dtype=np.int32), (70, 1)))
        if name == "two_same":
            assert (want_i[:, :min(k, 2)] == np.arange(min(k, 2))).all()
    if n > 1:
        for k in range(2, min(n, 8) + 1):
            want_i, want_d = G.knn_numpy(cloud, cloud, k)
            dk = np.sqrt(want_d[:, k - 1])
            np.testing.assert_array_equal(bits(oracle.smoothed_densities(cloud, k)), bits(np.minimum(dk, dk[want_i[:, 1]])))
    pts = np.concatenate([cloud, q])
    got = oracle.normals_knn(pts, 8, surf=cloud)
    if n < 3:
        assert np.isnan(got[:, 4:7]).all() and np.isnan(got[:, 9]).all()
    else:
        assert np.isfinite(got[:, 9]).all()


@pytest.mark.parametrize("name", ["one", "two_same"])
def test_far_queries_equal_numpy_at_bounded_cost(oracle, name):
    cloud = G.tiny_clouds()[name]
    q = G.far_queries(cloud)
    for k in (1, 2, 8):
        _, want_d, walk = check_walk(oracle, q, cloud, k)
        assert (walk[:, 2] == 1).all() and (walk[:, 0] == walk[:, 1]).all()   # one cell, one ring: the ring that reaches it
    h = G.auto_cell(cloud, 4.0, device=True)
    assert 1e5 / float(h) > 2.0 ** 31 and np.isfinite(want_d[:, 0]).all()
    if name == "two_same":
        assert walk[:, 0].max() == G.RING_CELL_MAX                  # beyond 2^31 cells at the oracle's cell too: the centre is held
