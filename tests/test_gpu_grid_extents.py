"""-m gpu: the neighbourhood searches of the device on stretched and lopsided bounding boxes (tests/grid_extents_lib.py: a 4000-point
blob plus stray points that take the uniform grid to the cell cap, past it, and to 1e5 cells along one or two axes), through the C ABI.

1. device == oracle bit for bit for the stages that sum in grid order (fpfh in the default arithmetic, iss_keypoints, evaluate_plane with
   its pairs, match_local with a finite radius): both builders must choose the same cell ("The cell size of a grid").
2. device == the brute-force CPU statements under tests/cpp (dense plane evaluation, temperature maps, nearest, overlap_rmse, SHOT rows and
   frames): a search that loses a neighbour to the rounding of the cell coordinate shows here even where the oracle loses it too.
3. no stray is anyone's neighbour, so every grid-independent result of a blob query equals the `room` result bit for bit.
4. `thin`'s constructed pair -- within the radius, two cells apart at the cell the caller asked for -- is found.
5. the ring searches (knn, normals_knn, smoothed_densities) against numpy's lexsort on (d2, index), k = 8 (heap kernel) and 40 (wave kernel),
   on room, thin and flat, with queries that are points of the cloud.
6. the ring searches away from there, k = 1, 2, 8 (heap kernel) and 16, 40 (wave kernel): queries on and outside the cloud's box (26
   directions, three separations, the two corners), clouds of one to five points and of 70 coincident points plus one (k > n: the slots a
   list cannot fill are -1 / +inf), and queries up to 1e5 -- more than 2^31 cells -- from a one-point cloud.  lgr_knn_query walks only the
   cells of a ring that exist, from the first ring that touches the grid (lgr_grid.cuh), so none of these costs more than the grid's cells;
   tests/test_oracle_grid_extents.py counts the visits of the same walk on the CPU.

The module uses a context of its own: the cell tables of these scenes grow to about 1 GB, which the session's shared context should not
carry into the other tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_extents_lib as G  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SCENES = [("room", 0.25), ("room", 0.1), ("gap", 0.25), ("over", 0.25), ("many", 0.1), ("thin", 0.1), ("flat", 0.1)]
STRETCHED = [s for s in SCENES if s[0] != "room"]
IDS = [f"{n}-{r}" for n, r in SCENES]
DOUBLINGS = dict(room=0, gap=0, over=1, many=8, thin=1, flat=3)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """bit for bit; NaNs in the same places count as equal"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN placement differs in {int((na != nb).sum())} values"
    bad = (bits(a) != bits(b)) & ~na
    assert not bad.any(), f"{int(bad.sum())} values differ, largest difference {np.abs(a[bad].astype(np.float64) - b[bad]).max()}"


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from lgr_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(oracle):
    """the blob, thin's constructed points, and per scene: the cloud, the key points / sources (every 13th blob point; thin: + q and qc)"""
    b = G.blob(oracle)
    con = G.constructed(b, 0.1)
    w = dict(blob=b, con=con, kps_blob=b[::13].copy(), scene={})
    for name, r in SCENES:
        extra = np.concatenate([con["p"][None], con["cluster"]]) if name == "thin" else None
        cloud = G.scene(b, name, r, extra)
        q = np.stack([con["q"], con["qc"]]) if name == "thin" else np.zeros((0, 12), F)
        h, d, k = G.check_scene(name, cloud, r, queries=np.concatenate([b, q]))
        assert k == DOUBLINGS[name], (name, r, h, d, k)
        w["scene"][(name, r)] = dict(cloud=cloud, kps=np.concatenate([w["kps_blob"], q]), src=np.concatenate([b, q]), h=h)
    return w


def dense_threshold(r):
    """evaluate_plane_dense searches 2 * threshold around a point: radius r, cell fl(1.001f * r)"""
    return float(F(r) / F(2))


# ---- 1. device == oracle in grid order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", SCENES, ids=IDS)
def test_fpfh_and_iss_equal_the_oracle(ctx, oracle, world, name, r):
    s = world["scene"][(name, r)]
    want = oracle.fpfh(s["kps"], s["cloud"], r)
    got = ctx.fpfh(cuda(s["kps"]), cuda(s["cloud"]), r).cpu().numpy()
    same(got, want)
    assert np.isfinite(want[: len(world["kps_blob"])]).all()
    np.testing.assert_array_equal(ctx.iss_keypoints(cuda(s["cloud"]), r).cpu().numpy(), oracle.iss_keypoints(s["cloud"], r))
    r_iss = 0.1 * r                                                   # a radius with about eight neighbours: key points exist
    want_iss = oracle.iss_keypoints(s["cloud"], r_iss)
    np.testing.assert_array_equal(ctx.iss_keypoints(cuda(s["cloud"]), r_iss).cpu().numpy(), want_iss)
    assert len(want_iss) > 10


@pytest.mark.parametrize("name,r", SCENES, ids=IDS)
def test_evaluate_plane_and_match_local_equal_the_oracle(ctx, oracle, world, name, r):
    s = world["scene"][(name, r)]
    T = G.small_transform(0.01)
    for score_id in (0, 3):
        want = oracle.evaluate_plane(s["src"], s["cloud"], T, score_id, with_pairs=True)
        got = ctx.evaluate_plane(cuda(s["src"]), cuda(s["cloud"]), T, score_id, with_pairs=True)
        assert got["n_inl"] == want["n_inl"] and want["n_inl"] > 5
        for f in ("rmse", "metric", "thr"):
            assert bits(got[f]) == bits(want[f]), (f, got[f], want[f])
        np.testing.assert_array_equal(got["pairs"], want["pairs"])
    rng = np.random.default_rng(3)
    qf, tf = rng.uniform(0, 100, (len(s["src"]), 33)).astype(F), rng.uniform(0, 100, (len(s["cloud"]), 33)).astype(F)
    gi, gd = [x.cpu().numpy() for x in ctx.match_local(cuda(s["src"]), cuda(s["cloud"]), cuda(qf), cuda(tf), T, r)]
    oi, od = oracle.match_local(s["src"], s["cloud"], qf, tf, T, r)
    np.testing.assert_array_equal(gi, oi)
    same(gd, od)
    assert (oi[: G.N_BLOB] >= 0).all()


# ---- 2. device == brute force -----------------------------------------------------------------------------------------------------------
def check_dense(dev, ref):
    assert dev.n_inliers == ref["n_inliers"], (dev.n_inliers, ref["n_inliers"])
    for f in ("rmse", "metric", "threshold", "score"):
        assert bits(getattr(dev, f)) == bits(ref[f]), (f, getattr(dev, f), ref[f])
    assert np.array_equal(dev.inliers.view(np.uint32), ref["inliers"].view(np.uint32)) and np.array_equal(dev.nn, ref["nn"])


@pytest.mark.parametrize("name,r", SCENES, ids=IDS)
def test_dense_plane_equals_the_statement(ctx, world, name, r):
    import plane_dense_ref_lib as P
    s = world["scene"][(name, r)]
    thr = dense_threshold(r)
    T = G.small_transform(thr)
    for score_id in (0, 3):
        ref = P.evaluate(s["src"], s["cloud"], T, score_id, thr)
        assert ref["n_inliers"] > G.N_BLOB // 10
        check_dense(ctx.evaluate_plane_dense(cuda(s["src"]), cuda(s["cloud"]), T, score_id, threshold=thr, with_inliers=True, with_nn=True), ref)


@pytest.mark.parametrize("name,r", SCENES, ids=IDS)
def test_debug_and_analysis_equal_the_statements(ctx, world, name, r):
    import analysis_ref_lib as A
    import debug_ref_lib as D
    s = world["scene"][(name, r)]
    thr = dense_threshold(r)                                          # both search 2 * thr
    T, T_gt = G.small_transform(thr), np.eye(4, dtype=F)
    d_src, d_tgt = cuda(s["src"]), cuda(s["cloud"])
    ref = D.temperature_maps(s["src"], s["cloud"], T, thr)
    dev = ctx.temperature_maps(d_src, d_tgt, T, thr)
    for side in ("src", "tgt"):
        for k in D.TEMP_FIELDS:
            assert np.array_equal(dev[side][k].view(np.uint32), ref[side][k].view(np.uint32)), (side, k)
        assert dev[side]["n_below"] == ref[side]["n_below"]
    assert ref["src"]["n_below"] > G.N_BLOB // 2
    ri, rd = D.nearest(s["src"], s["cloud"])
    idx, d2 = ctx.nearest(d_src, d_tgt)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(d2.cpu().numpy()), bits(rd))
    ro = A.overlap_rmse(s["src"], s["cloud"], T, T_gt, thr)
    rm, n, pe, oidx = ctx.overlap_rmse(d_src, d_tgt, T, T_gt, thr)
    assert bits(rm) == bits(ro["overlap_rmse"]) and n == ro["overlap_size"] and bits(pe) == bits(ro["pcd_err"]) and np.array_equal(oidx, ro["idx"])
    assert n > G.N_BLOB // 2


@pytest.mark.parametrize("name,r", SCENES, ids=IDS)
def test_shot_equals_the_statement(ctx, world, name, r):
    import shot_ref_lib as S
    s = world["scene"][(name, r)]
    want_rows, want_fr = S.shot(s["kps"], s["cloud"], r)
    rows, fr = ctx.shot(cuda(s["kps"]), cuda(s["cloud"]), r, with_lrf=True)
    same(fr.cpu().numpy(), want_fr)
    same(rows.cpu().numpy(), want_rows)
    assert np.isfinite(want_rows[: len(world["kps_blob"])]).all(1).mean() > 0.9   # a key point at the rim may have no frame


# ---- 3. the strays change nothing for the blob ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", STRETCHED, ids=IDS[2:])
def test_strays_change_nothing_for_the_blob(ctx, world, name, r):
    from lgr_amd import capi
    s, room = world["scene"][(name, r)], world["scene"][("room", r)]
    kps, nb = cuda(world["kps_blob"]), G.N_BLOB
    d_src, thr = cuda(world["blob"]), dense_threshold(r)
    T = G.small_transform(thr)
    out = []
    for c in (room, s):
        d = cuda(c["cloud"])
        e = ctx.evaluate_plane_dense(d_src, d, T, 3, threshold=thr, with_inliers=True, with_nn=True)
        t = ctx.temperature_maps(d_src, d, T, thr)
        ctx.set_options(arithmetic=capi.ARITH_PCL)
        try:
            f = ctx.fpfh(kps, d, r).cpu().numpy()
        finally:
            ctx.set_options()
        pl = ctx.evaluate_plane(d_src, d, G.small_transform(0.01), 0, with_pairs=True)
        out.append(dict(e=e, shot=ctx.shot(kps, d, r).cpu().numpy(), t=t, fpfh=f, plane=pl))
    a, b = out
    assert a["e"].n_inliers == b["e"].n_inliers and np.array_equal(a["e"].nn, b["e"].nn)
    assert np.array_equal(a["e"].inliers.view(np.uint32), b["e"].inliers.view(np.uint32))
    for f in ("rmse", "metric", "score"):
        assert bits(getattr(a["e"], f)) == bits(getattr(b["e"], f)), f
    same(b["shot"], a["shot"])
    same(b["fpfh"], a["fpfh"])
    for k in ("temp_distance", "temp_normal", "nn"):
        assert np.array_equal(a["t"]["src"][k].view(np.uint32), b["t"]["src"][k].view(np.uint32)), k
        assert np.array_equal(a["t"]["tgt"][k][:nb].view(np.uint32), b["t"]["tgt"][k][:nb].view(np.uint32)), k
    # evaluate_plane takes its threshold from the target's density, the 0.8 quantile of the smoothed 8-NN distances over ALL target points:
    # more than one added point moves the quantile's rank (int(0.8f n - 1)), so the threshold may differ in the last digits and a borderline
    # point may change sides.  Grid independent: the nearest target of a source point that is an inlier under both thresholds; the whole
    # list where the thresholds are equal.
    pa, pb = dict(map(tuple, a["plane"]["pairs"])), dict(map(tuple, b["plane"]["pairs"]))
    both = set(pa) & set(pb)
    assert len(both) > 5 and all(pa[i] == pb[i] for i in both)
    if bits(a["plane"]["thr"]) == bits(b["plane"]["thr"]):
        assert pa == pb


# ---- 4. the constructed pair ------------------------------------------------------------------------------------------------------------
def test_constructed_pair_is_found(ctx, world):
    r = 0.1
    s, con, b = world["scene"][("thin", r)], world["con"], world["blob"]
    cloud, h0, r2 = s["cloud"], G.cell(r), F(F(r) * F(r))
    ox = cloud[:, 0].min()
    ip = G.N_BLOB                                                     # p's index; the cluster follows
    assert np.array_equal(cloud[ip], con["p"]) and np.array_equal(cloud[ip + 1: ip + 6], con["cluster"])
    # the construction: within the radius in float32, two cells apart at the cell the caller asks for, and nothing else in reach
    for q, lo, hi in ((con["q"], ip, ip + 1), (con["qc"], ip + 1, ip + 6)):
        d2 = G.d2_f32(q[None], cloud)[0]
        assert list(np.flatnonzero(d2 < 4 * r2)) == list(range(lo, hi)) and (d2[lo:hi] < r2).all()
        assert (G.cellc(q[0], ox, h0) - G.cellc(cloud[lo:hi, 0], ox, h0) == 2).all()
    d_cloud = cuda(cloud)
    row = ctx.fpfh(cuda(con["q"][None]), d_cloud, r).cpu().numpy()
    assert not np.isnan(row).any(), "fpfh: the key point's only neighbour was not found"
    src = np.stack([con["q"], con["qc"]])
    for thr, want_nn in ((r, [ip, ip + 1]), (dense_threshold(r), [ip, ip + 1])):   # radius 2 r; radius r: the cell the pair was built for
        e = ctx.evaluate_plane_dense(cuda(src), d_cloud, np.eye(4, dtype=F), 0, threshold=float(thr), with_inliers=True, with_nn=True)
        assert e.n_inliers == 2 and list(e.nn) == want_nn, (thr, e.n_inliers, e.nn)
        assert list(e.inliers["index_query"]) == [0, 1] and list(e.inliers["index_match"]) == want_nn
    lrf = np.tile(np.eye(3, dtype=F).reshape(1, 9), (2, 1))
    rows = ctx.shot(cuda(src), d_cloud, r, lrf=cuda(lrf)).cpu().numpy()
    assert np.isnan(rows[0]).all(), "one neighbour: no SHOT row"
    assert not np.isnan(rows[1]).any(), "shot: the five neighbours of the cluster's query were not all found"


# ---- 5. ring searches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", [("room", 0.1), ("thin", 0.1), ("flat", 0.1)], ids=["room", "thin", "flat"])
def test_ring_searches_equal_numpy(ctx, oracle, world, name, r):
    cloud = world["scene"][(name, r)]["cloud"]
    n = len(cloud)
    d = cuda(cloud)
    for k in (8, 40):
        want_i, want_d = G.knn_numpy(cloud, cloud, k)
        idx, d2 = ctx.knn(d, d, k)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
        np.testing.assert_array_equal(bits(d2.cpu().numpy()), bits(want_d))
        qi, qd = ctx.knn(cuda(cloud[::7].copy()), d, k)               # queries that are not the cloud itself (points of it: inside its box)
        np.testing.assert_array_equal(qi.cpu().numpy(), want_i[::7])
        np.testing.assert_array_equal(bits(qd.cpu().numpy()), bits(want_d[::7]))
        dk = np.sqrt(want_d[:, k - 1])
        np.testing.assert_array_equal(bits(ctx.smoothed_densities(d, k).cpu().numpy()), bits(np.minimum(dk, dk[want_i[:, 1]])))
    # normals: the device's 30-NN estimate equals the oracle's, whose neighbour lists equal numpy's
    oi, _ = oracle.knn(cloud, cloud, 30)
    np.testing.assert_array_equal(oi, G.knn_numpy(cloud, cloud, 30)[0])
    got = ctx.normals_knn(cuda(cloud), 30).cpu().numpy()
    same(got, oracle.normals_knn(cloud, 30))
    assert np.isfinite(got[:n, 4:7]).all()


# ---- 6. ring searches outside the box, on tiny clouds, far from them ---------------------------------------------------------------------
RING_K = (1, 2, 8, 16, 40)                                            # below 16: knn_kernel (per-thread heaps); from 16: knn_wave_kernel
TINY = ["one", "two_same", "two", "line3", "plane5", "same70"]


def knn_target(k):
    """points per cell lgr_knn_lists asks of the automatic cell: max(4, 0.35f k)"""
    return max(F(4), F(F(0.35) * F(k)))


def check_knn(ctx, q, cloud, k, want=None):
    want_i, want_d = G.knn_padded(q, cloud, k) if want is None else (want[0][:, :k], want[1][:, :k])
    idx, d2 = ctx.knn(cuda(q), cuda(cloud), k)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(bits(d2.cpu().numpy()), bits(want_d))
    return want_i, want_d


@pytest.fixture(scope="module")
def outside(world):
    """the 80 outside queries of the blob and their 40 nearest by numpy (a list of k is its first k columns: the order is total)"""
    b = world["blob"]
    q = G.outside_queries(b)
    mn, mx = b[:, :3].min(0), b[:, :3].max(0)
    assert len(q) == 80 and ((q[:78, :3] < mn) | (q[:78, :3] > mx)).any(1).all()
    return dict(q=q, want=G.knn_padded(q, b, max(RING_K)))


@pytest.mark.parametrize("k", RING_K)
def test_knn_outside_the_box_equals_numpy(ctx, world, outside, k):
    check_knn(ctx, outside["q"], world["blob"], k, outside["want"])


@pytest.mark.parametrize("name", TINY)
def test_knn_on_tiny_clouds_equals_numpy(ctx, name):
    cloud = G.tiny_clouds()[name]
    n = len(cloud)
    for k in RING_K:
        q = G.tiny_queries(cloud, G.auto_cell(cloud, knn_target(k), device=True))   # 3 and 200 cells of the cell this k searches on
        want_i, want_d = check_knn(ctx, q, cloud, k)
        assert (want_i[:, min(k, n):] == -1).all() and np.isinf(want_d[:, min(k, n):]).all()
        if name == "same70":                                          # equal distances: the lower index first
            np.testing.assert_array_equal(want_i[:70], np.tile(np.arange(k, dtype=np.int32), (70, 1)))


@pytest.mark.parametrize("name", ["one", "two_same"])
def test_knn_far_from_a_tiny_cloud_equals_numpy(ctx, name):
    cloud = G.tiny_clouds()[name]
    q = G.far_queries(cloud)
    assert 1e5 / float(G.auto_cell(cloud, knn_target(40), device=True)) > 2.0 ** 31   # the coarsest cell any k here searches on
    for k in RING_K:
        _, want_d = check_knn(ctx, q, cloud, k)
        assert np.isfinite(want_d[:, 0]).all()


def test_normals_of_outside_queries_equal_the_oracle(ctx, oracle, world, outside):
    b = world["blob"]
    pts = np.concatenate([b[::40], outside["q"]])
    want = oracle.normals_knn(pts, 30, surf=b)
    same(ctx.normals_knn(cuda(pts.copy()), 30, surf=cuda(b)).cpu().numpy(), want)
    assert np.isfinite(want[:, 4:7]).all()


@pytest.mark.parametrize("name", ["one", "triangle"])
def test_normals_on_a_tiny_surface_equal_the_oracle(ctx, oracle, name):
    tiny = G.tiny_clouds()
    surf = tiny["one"] if name == "one" else np.ascontiguousarray(tiny["plane5"][:3])
    h = G.auto_cell(surf, 6.0, device=True)                           # lgr_normals_knn_dev: six points per cell under a given surface
    pts = np.concatenate([G.tiny_queries(surf, h), G.far_queries(surf)])
    for k in (3, 30):
        want = oracle.normals_knn(pts, k, surf=surf)
        same(ctx.normals_knn(cuda(pts.copy()), k, surf=cuda(surf)).cpu().numpy(), want)
        assert np.isnan(want[:, 4:7]).all() if name == "one" else np.isfinite(want[:, 4:7]).all()


@pytest.mark.parametrize("name", ["two_same", "two", "line3", "same70"])
def test_smoothed_densities_of_tiny_clouds_equal_numpy(ctx, name):
    cloud = G.tiny_clouds()[name]
    d = cuda(cloud)
    for k in [k for k in (2, 3, 8, 40) if k <= len(cloud)]:
        want_i, want_d = G.knn_numpy(cloud, cloud, k)
        dk = np.sqrt(want_d[:, k - 1])
        np.testing.assert_array_equal(bits(ctx.smoothed_densities(d, k).cpu().numpy()), bits(np.minimum(dk, dk[want_i[:, 1]])))
