"""GPU parity: bounding box, voxel downsample, k-NN, smoothed densities, k-NN normals, FPFH vs the oracle.

Bar: bit-exact (every stage is either integer/index work or a float sequence restated op for op; tolerance 0).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pair():
    from lgr_amd import synthetic
    return synthetic.make_pair(20000, seed=7)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_bbox_quirk(lgr, oracle):
    rng = np.random.default_rng(0)
    from lgr_amd.synthetic import make_points
    for shift in (0.0, -50.0, 50.0):       # all-negative clouds hit the FLT_MIN-initialised max (include/common.h:268-270)
        p = make_points(rng.normal(shift, 3, (5000, 3)))
        p[17, 0] = np.nan
        mn, mx = oracle.bbox(p)
        g = lgr.bbox(cuda(p)).cpu().numpy()
        np.testing.assert_array_equal(bits(g[:3]), bits(mn))
        np.testing.assert_array_equal(bits(g[3:]), bits(mx))


@pytest.mark.parametrize("voxel", [0.0236, 0.1, 5.0])
def test_downsample(lgr, oracle, pair, voxel):
    src = pair["src"].copy()
    src[:, 8] = np.random.default_rng(1).uniform(0.5, 2.0, src.shape[0]).astype(np.float32)   # intensity weights
    src[:, 4:7] = np.random.default_rng(2).normal(size=(src.shape[0], 3)).astype(np.float32)
    src[100, 1] = np.inf                                                                         # skipped (isValid)
    want = oracle.downsample(src, voxel, oracle.ORDER_CANONICAL)
    got = lgr.downsample(cuda(src), voxel).cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(bits(got), bits(want))
    # reference (libstdc++ unordered_map) output order through the host entry point
    want_ref = oracle.downsample(src, voxel, oracle.ORDER_LIBSTDCXX)
    got_ref = lgr.downsample_host(src, voxel, 0)
    np.testing.assert_array_equal(bits(got_ref), bits(want_ref))
    got_can = lgr.downsample_host(src, voxel, 1)
    np.testing.assert_array_equal(bits(got_can), bits(want))


def test_downsample_edge_cases(lgr, oracle):
    import torch
    from lgr_amd.synthetic import make_points
    empty = torch.zeros((0, 12), dtype=torch.float32, device="cuda")
    assert lgr.downsample(empty, 0.1).shape[0] == 0
    one = make_points(np.array([[1.0, 2.0, 3.0]]))
    np.testing.assert_array_equal(bits(lgr.downsample(cuda(one), 0.1).cpu().numpy()), bits(oracle.downsample(one, 0.1)))
    # duplicates collapse into one voxel; zero intensity gives 0/0 exactly like the reference
    dup = make_points(np.repeat(np.array([[0.5, 0.5, 0.5]]), 7, 0))
    np.testing.assert_array_equal(bits(lgr.downsample(cuda(dup), 0.1).cpu().numpy()), bits(oracle.downsample(dup, 0.1)))


@pytest.mark.parametrize("k", [1, 2, 8, 30, 40])
def test_knn(lgr, oracle, pair, k):
    src, tgt = pair["src"], pair["tgt"][:5000]
    oi, od = oracle.knn(tgt, src, k)
    gi, gd = lgr.knn(cuda(tgt), cuda(src), k)
    lgr.sync()
    np.testing.assert_array_equal(gi.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits(gd.cpu().numpy()), bits(od))


def test_knn_ties_on_grid(lgr, oracle):
    """regular lattice: many exactly equidistant neighbours -> (d2, index) tie rule"""
    from lgr_amd.synthetic import make_points
    g = np.stack(np.meshgrid(np.arange(30), np.arange(30), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    p = make_points(g)
    oi, od = oracle.knn(p, p, 12)
    gi, gd = lgr.knn(cuda(p), cuda(p), 12)
    lgr.sync()
    np.testing.assert_array_equal(gi.cpu().numpy(), oi)


@pytest.mark.parametrize("k", [5, 40, 64, 100, 128])
def test_knn_self_queries(lgr, oracle, pair, k):
    """queries = the cloud itself (grid-ordered launch), all three buffer widths of the wave search (k <= 40, <= 96, <= 128)"""
    p = pair["src"][:20000]
    oi, od = oracle.knn(p, p, k)
    t = cuda(p)
    gi, gd = lgr.knn(t, t, k)
    lgr.sync()
    np.testing.assert_array_equal(gi.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits(gd.cpu().numpy()), bits(od))


def test_knn_degenerate_clouds(lgr, oracle):
    """what the threshold search of the wave k-NN has to survive: hundreds of identical points (no radius separates k of them from
    the rest: only the index part of the key does), equal distances on a lattice, clusters of very different density, fewer points
    than k, non-finite points among queries and cloud"""
    from lgr_amd.synthetic import make_points
    rng = np.random.default_rng(5)
    blob = np.repeat(np.array([[0.25, -0.5, 1.0]], np.float32), 700, 0)                       # 700 copies of one point
    blob2 = np.repeat(np.array([[0.26, -0.5, 1.0]], np.float32), 90, 0)
    lattice = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(2), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.5
    dense = (rng.normal(size=(3000, 3)) * 1e-3 + np.array([5.0, 5.0, 0.0])).astype(np.float32)
    sparse = (rng.uniform(-40, 40, size=(400, 3))).astype(np.float32)
    xyz = np.concatenate([blob, lattice, dense, blob2, sparse])
    xyz = xyz[rng.permutation(len(xyz))]
    p = make_points(xyz)
    p[17, 0] = np.nan
    p[400, 2] = np.inf
    for k in (1, 7, 40, 64, 128):
        oi, od = oracle.knn(p, p, k)
        t = cuda(p)
        gi, gd = lgr.knn(t, t, k)
        lgr.sync()
        np.testing.assert_array_equal(gi.cpu().numpy(), oi, err_msg=f"k={k}")
        np.testing.assert_array_equal(bits(gd.cpu().numpy()), bits(od), err_msg=f"k={k}")
    # other queries than the cloud, in an order that jumps between the clusters
    q = make_points(np.concatenate([sparse[:50] + 0.01, blob[:3], dense[:40], lattice[:30] + 0.25]).astype(np.float32)[rng.permutation(123)])
    oi, od = oracle.knn(q, p, 40)
    gi, gd = lgr.knn(cuda(q), cuda(p), 40)
    lgr.sync()
    np.testing.assert_array_equal(gi.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits(gd.cpu().numpy()), bits(od))
    # fewer points than k: the lists end with -1 / +inf
    small = make_points(rng.normal(size=(9, 3)).astype(np.float32))
    oi, od = oracle.knn(small, small, 40)
    gi, gd = lgr.knn(cuda(small), cuda(small), 40)
    lgr.sync()
    np.testing.assert_array_equal(gi.cpu().numpy(), oi)
    np.testing.assert_array_equal(bits(gd.cpu().numpy()), bits(od))
    for k in (2, 5, 24):
        want = oracle.smoothed_densities(p, k)
        got = lgr.smoothed_densities(cuda(p), k).cpu().numpy()
        np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.parametrize("k", [2, 8, 20])
def test_smoothed_densities(lgr, oracle, pair, k):
    want = oracle.smoothed_densities(pair["src"], k)
    got = lgr.smoothed_densities(cuda(pair["src"]), k).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))


def test_normals(lgr, oracle, pair):
    ds = oracle.downsample(pair["src"], 0.0236)
    want = oracle.normals_knn(ds, 30, vp=pair["vp_src"])
    t = cuda(ds)
    lgr.normals_knn(t, 30, vp=pair["vp_src"])
    got = t.cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))
    # first-principles: unit normals pointing to the viewpoint side
    nrm = got[:, 4:7]
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-5)
    assert ((pair["vp_src"] - got[:, :3]) * nrm).sum(1).min() >= -1e-6
    # separate search surface (matching.h:244 form)
    q = pair["src"][:3000].copy()
    want2 = oracle.normals_knn(q, 30, surf=ds, vp=pair["vp_src"])
    tq = cuda(q)
    lgr.normals_knn(tq, 30, surf=cuda(ds), vp=pair["vp_src"])
    np.testing.assert_array_equal(bits(tq.cpu().numpy()), bits(want2))
    # the same with normals_available = 1: the call descriptor_dev makes for RoPS key points (include/matching.h:243-246)
    import ctypes as C
    from lgr_amd import capi
    want3 = oracle.normals_knn(q, 30, surf=ds, vp=pair["vp_src"], normals_available=True)
    tq3, tds = cuda(q), cuda(ds)
    v = (C.c_float * 3)(*[float(x) for x in pair["vp_src"]])
    lgr.check(capi.lib().lgr_normals_knn_dev(lgr.h, capi._ptr(tq3), tq3.shape[0], capi._ptr(tds), tds.shape[0], 30, v, 1))
    np.testing.assert_array_equal(bits(tq3.cpu().numpy()), bits(want3))


@pytest.mark.parametrize("k", [16, 41, 57, 58, 64])
def test_normals_other_k(lgr, oracle, pair, k):
    """the wave-per-query search at the edges of its two instantiations (k <= 40 / k > 40) and at the list sizes whose LDS passes 64 KB per
    workgroup (k >= 58: ADVICE r3)"""
    ds = oracle.downsample(pair["src"], 0.0236)
    want = oracle.normals_knn(ds, k, vp=pair["vp_src"])
    t = cuda(ds)
    lgr.normals_knn(t, k, vp=pair["vp_src"])
    np.testing.assert_array_equal(bits(t.cpu().numpy()), bits(want))


def test_fpfh(lgr, oracle, pair):
    ds = oracle.normals_knn(oracle.downsample(pair["src"], 0.0236), 30, vp=pair["vp_src"])
    kps = pair["src"][:6000].copy()
    kps[5, 2] = np.nan                      # non-finite keypoint -> NaN row
    kps[6, :3] = [1e3, 1e3, 1e3]            # no neighbours -> NaN row
    want = oracle.fpfh(kps, ds, 0.25)
    got = lgr.fpfh(cuda(kps), cuda(ds), 0.25).cpu().numpy()
    assert np.isnan(want[5]).all() and np.isnan(want[6]).all()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok])
    # each 11-bin block sums to 100
    blocks = got[~np.isnan(got).any(1)].reshape(-1, 3, 11).sum(2)
    assert np.allclose(blocks, 100, atol=1e-2)
    # keypoints == surface (the reference's tests/flann_bf_matcher.h:55-56 call shape), host entry point
    sub = ds[:4000]
    np.testing.assert_array_equal(bits(lgr.fpfh_host(sub, sub, 0.25)), bits(oracle.fpfh(sub, sub, 0.25)))


def test_fpfh_weight_reciprocal_is_the_division(lgr):
    """The weighting kernel computes 1 / d2 as v_rcp_f32 + one Newton step (lgr_rcp2, lgr_features.hip) in place of the IEEE division
    sequence; the canonical definition (oracle orc_fpfh; PCL's 1.0f / dists[idx]) is the division.  EVERY float of the range the kernel
    uses the sequence on, [1e-36, 1e36] (2.0e9 values), goes through both on the device: not one may differ."""
    bad, tested = lgr.selfcheck_rcp(1e-36, 1e36)
    assert tested == int(np.float32(1e36).view(np.uint32)) - int(np.float32(1e-36).view(np.uint32)) + 1
    assert bad == 0, f"{bad} of {tested} reciprocals differ from the division"


def test_fpfh_tiny_distances_divide(lgr, oracle):
    """squared distances below the checked range of the reciprocal (1e-36) take the division: two surface points 5e-19 apart"""
    rng = np.random.default_rng(11)
    from lgr_amd.synthetic import make_points
    xyz = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    xyz[1] = xyz[0]; xyz[1, 0] = np.nextafter(xyz[0, 0], np.float32(2))    # ~6e-8 apart: d2 ~ 3.5e-15 (inside the range)
    xyz[2] = [5e-19, 0, 0]; xyz[3] = [0, 0, 0]                            # d2 = 2.5e-37: a normal float below the range
    ds = oracle.normals_knn(make_points(xyz), 10)
    want = oracle.fpfh(ds, ds, 0.2)
    got = lgr.fpfh(cuda(ds), cuda(ds), 0.2).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok])
