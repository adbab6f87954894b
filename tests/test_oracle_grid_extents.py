"""The oracle's neighbourhood searches on stretched and lopsided bounding boxes (tests/grid_extents_lib.py), so that its grid is right
before tests/test_gpu_grid_extents.py compares the device with it.  No GPU.

* the scenes reach what they are built for: cell counts at the caller's cell, and the doublings the rule of DESIGN.md section 4 gives;
* no stray is anyone's neighbour, so what does not depend on the grid equals the `room` result bit for bit for every blob query: FPFH in
  PCL's arithmetic (neighbours by ascending distance), evaluate_plane's pairs, match_local;
* against brute force: every radius search of match_local finds exactly numpy's candidates' best, and `thin`'s constructed pair -- within
  the radius, two cells apart at the cell the caller asked for -- is found;
* the ring searches (knn, smoothed_densities, normals) against numpy's lexsort on (d2, index) on room, thin and flat only: the ring walk
  is cubic in the separation of a query from the points (orc_grid.h knn, as lgr_knn_query on the device)."""
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
