"""-m gpu: matchLocal with a k-list (lgr_match_local_knn_dev, lgr_match_local_knn) and matchFLANN for every row length
(lgr_match_flann_rows_dev, lgr_match_flann_rows) against the CPU statement tests/cpp/local_match_ref.cpp, everything compared as uint32
bits: FPFH / RoPS135 / SHOT rows of a make_pair(1500) scene under a perturbed ground truth at a radius whose candidate counts span 0,
fewer than k, exactly k and more than a wave; both kernels (the 27-cell gather and the tiled scan), radius 0 and a train point exactly
on the radius; sizes around the wave and tile widths; descriptor ties; non-finite rows, points and moved points; equality with the
FPFH one-match entry points; the reference's three-way differential test for all three descriptors; the refusals; context reuse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_match_ref_lib as bf_ref  # noqa: E402
import local_match_ref_lib as ref  # noqa: E402
from refine_ref_lib import perturbed  # noqa: E402

pytestmark = pytest.mark.gpu
DIMS = [33, 135, 352]
FLT_MAX = ref.FLT_MAX
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5   # include/lgr.h
SEED = 77                                   # the scene of the differential test (chosen on the CPU: see test_reference_differential_test)


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()   # (a copy: the shared scene arrays are read-only)


def _dev(lgr, qp, tp, q, t, G, radius, k):
    i, d = lgr.match_local_knn(cuda(qp), cuda(tp), cuda(q), cuda(t), G, radius, k)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(ref.bits(got[1]), ref.bits(want[1]), err_msg=what)


def _both(lgr, qp, tp, q, t, G, radius, k, what=""):
    """the device entry and the host twin against the statement; returns the statement's (idx, dist, candidate counts)"""
    want = ref.match(qp, tp, q, t, G, radius, k, counts=True)
    _eq(_dev(lgr, qp, tp, q, t, G, radius, k), want, what + " dev")
    _eq(lgr.match_local_knn_host(qp, tp, q, t, G, radius, k), want, what + " host")
    return want


def _rows(rng, m, dim):
    return rng.random((m, dim)).astype(np.float32)


def _cloud(rng, m, scale=1.0):
    return ref.pts12(rng.random((m, 3)) * scale)


@pytest.fixture(scope="module")
def scene(lgr):
    """FPFH, RoPS135 (gravity frames) and SHOT rows of both clouds of make_pair(1500), computed on the device once"""
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(1500, seed=SEED)
    radius = 0.25
    voxel = float(np.sqrt(np.float32(np.pi * radius * radius / 352.0)))
    rows = {d: [] for d in DIMS}
    for side in ("src", "tgt"):
        vp = pair["vp_" + side]
        cloud = cuda(pair[side])
        surf = lgr.downsample(cloud, voxel).contiguous()
        lgr.normals_knn(surf, 30, vp=vp)
        kn = cloud.clone()
        v = (C.c_float * 3)(*[float(x) for x in vp])
        lgr.check(capi.lib().lgr_normals_knn_dev(lgr.h, capi._ptr(kn), kn.shape[0], capi._ptr(surf), surf.shape[0], 30, v, 1))
        rows[33].append(lgr.fpfh(kn, surf, radius))
        rows[135].append(lgr.rops(kn, surf, radius, lgr.gravity_lrf(kn, surf, radius)))
        rows[352].append(lgr.shot(kn, surf, radius))
    lgr.sync()
    out = dict(src=pair["src"], tgt=pair["tgt"], guess=perturbed(pair["T_gt"], 0.1), pair=pair)
    for d in DIMS:
        out[d] = [np.ascontiguousarray(r.cpu().numpy()) for r in rows[d]]
        for r in out[d]:
            assert r.shape == (1500, d) and np.isfinite(r).all(1).mean() > 0.5
            r.setflags(write=False)
    return out


def _span_radius(sc, dim, k):
    """the smallest radius of a fixed ladder at which the statement's candidate counts (valid queries) hold 0, a value in (0, k) when
    k > 1, exactly k and at least 65"""
    valid = np.isfinite(sc[dim][0]).all(1)
    for r in np.geomspace(0.004, 0.6, 30):
        r = float(np.float32(r))
        n = ref.match(sc["src"], sc["tgt"], sc[dim][0], sc[dim][1], sc["guess"], r, k, counts=True)[2][valid]
        if (n == 0).any() and (k == 1 or ((n > 0) & (n < k)).any()) and (n == k).any() and (n >= 65).any():
            return r
    pytest.fail("no radius of the ladder spans the candidate counts")


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("k", [1, 2, 8])
def test_scene_rows_and_k(lgr, scene, dim, k):
    r = _span_radius(scene, dim, k)
    want = _both(lgr, scene["src"], scene["tgt"], scene[dim][0], scene[dim][1], scene["guess"], r, k, f"r={r}")
    n = want[2][np.isfinite(scene[dim][0]).all(1)]
    assert (n == 0).any() and (n == k).any() and (n >= 65).any() and (k == 1 or ((n > 0) & (n < k)).any())   # asserted on the statement
    assert ((want[0] >= 0).sum(1) == np.minimum(want[2], k)).all()


@pytest.mark.parametrize("dim", DIMS)
def test_both_paths_radius_zero_and_the_boundary(lgr, scene, dim):
    sel_q, sel_t = slice(0, 300), slice(0, 400)
    args = (scene["src"][sel_q], scene["tgt"][sel_t], scene[dim][0][sel_q], scene[dim][1][sel_t], scene["guess"])
    for k in (1, 3):
        want = _both(lgr, *args, FLT_MAX, k, "FLT_MAX")          # the tiled scan: every finite train point
        valid_q, valid_t = np.isfinite(args[2]).all(1), np.isfinite(args[3]).all(1)
        assert (want[2][valid_q] == valid_t.sum()).all() and valid_t.sum() > 65
        want = _both(lgr, *args, 0.0, k, "radius 0")
        assert (want[0] == -1).all() and (want[1] == 0).all()
    # exactly one train point at s == r * r bit for bit: moved query + (r, 0, 0) in exactly representable values; it is excluded
    rng = np.random.default_rng(dim)
    G = np.array([[0, -1, 0, 2], [1, 0, 0, -1], [0, 0, 1, 0.5], [0, 0, 0, 1]], np.float32)
    qxyz = np.array([[1.0, 2.0, 3.0], [0.5, -0.25, 1.0]], np.float32)
    moved = (qxyz @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    r = np.float32(0.5)
    txyz = np.concatenate([moved[:1] + np.float32([r, 0, 0]), moved[:1] + np.float32([0.25, 0, 0]), moved[:1] + np.float32([0, 0.75, 0]),
                           moved[1:] + np.float32([0, 0, -0.125]), rng.random((70, 3)).astype(np.float32) + moved[0]]).astype(np.float32)
    d0 = moved[0] - txyz[0]
    assert np.float32(np.float32(d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]).view(np.uint32) == np.float32(r * r).view(np.uint32)
    q, t = _rows(rng, 2, dim), _rows(rng, len(txyz), dim)
    t[0] = q[0]                                                   # the boundary point would win on the descriptor
    t[1] = q[0]; t[1, 0] += np.float32(0.5)                       # the point inside: nearer than any random row
    for k in (1, 8):
        want = _both(lgr, ref.pts12(qxyz), ref.pts12(txyz), q, t, G, float(r), k, "boundary")
        assert 0 not in want[0][0] and 1 in want[0][0] and want[0][1, 0] == 3
        wide = ref.match(ref.pts12(qxyz), ref.pts12(txyz), q, t, G, float(np.nextafter(r, np.float32(1))), k)
        assert wide[0][0, 0] == 0                                 # one ulp more and it is the match


@pytest.mark.parametrize("dim", DIMS)
def test_sizes(lgr, dim):
    rng = np.random.default_rng(100 + dim)
    G = perturbed(np.eye(4), 0.1)
    for mq, mt in [(1, 1), (1, 257), (63, 64), (64, 65), (65, 63), (64, 64), (257, 1), (257, 257), (63, 257), (65, 65)]:
        qp, tp, q, t = _cloud(rng, mq), _cloud(rng, mt), _rows(rng, mq, dim), _rows(rng, mt, dim)
        for radius in (0.45, FLT_MAX):                           # the gather and the tiled scan
            _both(lgr, qp, tp, q, t, G, radius, 3, f"mq={mq} mt={mt} r={radius}")
    qp, q = _cloud(rng, 65), _rows(rng, 65, dim)
    for radius in (0.45, FLT_MAX):
        got = _dev(lgr, qp, np.zeros((0, 12), np.float32), q, np.zeros((0, dim), np.float32), G, radius, 2)        # mt = 0: -1 / 0
        assert got[0].shape == (65, 2) and (got[0] == -1).all() and (got[1] == 0).all()
        hi, hd = lgr.match_local_knn_host(qp, np.zeros((0, 12), np.float32), q, np.zeros((0, dim), np.float32), G, radius, 2)
        assert (hi == -1).all() and (hd == 0).all()
        got = _dev(lgr, np.zeros((0, 12), np.float32), qp, np.zeros((0, dim), np.float32), q, G, radius, 2)        # mq = 0: nothing
        assert got[0].shape == (0, 2)
        assert lgr.match_local_knn_host(np.zeros((0, 12), np.float32), qp, np.zeros((0, dim), np.float32), q, G, radius, 2)[0].shape == (0, 2)


@pytest.mark.parametrize("dim", DIMS)
def test_ties(lgr, dim):
    rng = np.random.default_rng(200 + dim)
    mt = 90
    qxyz = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    txyz = (rng.random((mt, 3)) * 0.5 + 0.25).astype(np.float32)
    txyz[mt // 2:, 0] += 10
    # query 0: equal rows at different spatial distances, the farther one has the lower index
    txyz[5] = [0.375, 0, 0]; txyz[30] = [0.125, 0, 0]
    # query 1: equal rows at mirrored positions, equal s
    txyz[60] = [10.25, 0, 0]; txyz[80] = [9.75, 0, 0]
    q, t = _rows(rng, 2, dim), _rows(rng, mt, dim)
    t[5] = q[0]; t[30] = q[0]; t[60] = q[1]; t[80] = q[1]
    for radius in (2.0, FLT_MAX):
        for k in (1, 2, 8):
            want = _both(lgr, ref.pts12(qxyz), ref.pts12(txyz), q, t, np.eye(4, dtype=np.float32), radius, k, f"r={radius} k={k}")
            assert want[0][0, 0] == 30 and want[0][1, 0] == 60 and (want[1][:, 0] == 0).all()   # the nearer; the lower index
            if k >= 2:
                assert list(want[0][0, :2]) == [30, 5] and list(want[0][1, :2]) == [60, 80] and (want[1][:, 1] == 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_non_finite_input(lgr, dim):
    rng = np.random.default_rng(300 + dim)
    mq, mt = 70, 150
    qp, tp, q, t = _cloud(rng, mq), _cloud(rng, mt), _rows(rng, mq, dim), _rows(rng, mt, dim)
    q[3] = np.nan; q[4, dim // 2] = np.nan; q[5, 1] = -np.inf; q[66, dim - 1] = np.inf
    t[30] = np.nan; t[32, dim - 1] = np.nan; t[64, 0] = np.inf; t[65, (dim - 1) // 4 * 4] = -np.inf
    tp[40, 0] = np.nan; tp[41, 1] = np.inf; tp[42, 2] = -np.inf
    qp[7, 0] = np.nan; qp[8, 2] = np.inf
    qp[9, 0] = 3e38                                               # finite; the guess moves it to +inf
    G = np.eye(4, dtype=np.float32)
    G[0, 0] = 2.0
    for radius in (0.6, FLT_MAX):
        for k in (1, 3, 8):
            want = _both(lgr, qp, tp, q, t, G, radius, k, f"r={radius} k={k}")
            assert (want[0][[3, 4, 5, 66, 7, 8, 9]] == -1).all() and not np.isin(want[0], [30, 32, 64, 65, 40, 41, 42]).any()
            assert (want[0][:, 0] >= 0).sum() > 10
        # a finite row whose distance overflows is a candidate at distance +inf: behind the other one
        t2 = np.stack([np.full(dim, 3e38, np.float32), t[0]])
        want = _both(lgr, qp[:1], tp[:2], q[:1], t2, np.eye(4, dtype=np.float32), radius if radius > 1 else 5.0, 2, "overflow")
        assert list(want[0][0]) == [1, 0] and np.isinf(want[1][0, 1])


def test_k1_is_the_fpfh_entry_point(lgr, scene):
    """lgr_match_local_knn_dev(33, 1) against lgr_match_local_dev on the same call: no CPU involved (the oracle pins the latter's bits
    in tests/test_gpu_match_dispatch.py, whichever kernel serves it)"""
    import torch
    for qs, ts, G in (("src", "tgt", scene["guess"]), ("tgt", "src", np.linalg.inv(scene["guess"].astype(np.float64)).astype(np.float32))):
        qp, tp = cuda(scene[qs]), cuda(scene[ts])
        q, t = cuda(scene[33][0 if qs == "src" else 1]), cuda(scene[33][1 if qs == "src" else 0])
        for radius in (0.03, 0.08, 0.3, FLT_MAX, 0.0):
            i1, d1 = lgr.match_local(qp, tp, q, t, G, radius)
            ik, dk = lgr.match_local_knn(qp, tp, q, t, G, radius, 1)
            lgr.sync()
            assert torch.equal(ik[:, 0], i1) and torch.equal(dk[:, 0].view(torch.int32), d1.view(torch.int32)), radius
        assert (i1 == -1).all() and float((ik >= 0).float().mean()) == 0.0


@pytest.mark.parametrize("dim", DIMS)
def test_flann_rows(lgr, scene, dim):
    import torch
    one = {33: lgr.match_bf, 135: lgr.match_rops, 352: lgr.match_shot}[dim]
    rng = np.random.default_rng(400 + dim)
    sets = [(scene[dim][0], scene[dim][1]), (scene[dim][1], scene[dim][0])]
    a, b = _rows(rng, 130, dim), _rows(rng, 257, dim)
    a[7] = np.nan; a[8, dim - 1] = np.inf; b[100] = np.nan; b[200] = b[3]; a[9] = b[3]
    sets += [(a, b), (b[:65], a[:1])]
    for q, t in sets:
        tq, tt = cuda(q), cuda(t)
        gi, gd = lgr.match_flann_rows(tq, tt)
        bi, _ = one(tq, tt, max(t.shape[0], 1))
        lgr.sync()
        assert torch.equal(gi, bi)
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        np.testing.assert_array_equal(ref.bits(gd), ref.bits(ref.flann_dist(q, t, gi)))
        _eq(lgr.match_flann_rows_host(q, t), (gi, gd), "host")
        if dim == 33:
            fi, fd = lgr.match_flann(tq, tt)
            lgr.sync()
            _eq((fi.cpu().numpy(), fd.cpu().numpy()), (gi, gd), "lgr_match_flann_dev")
    assert gi.shape == (65,) and (gi[~np.isnan(b[:65]).any(1)] == 0).all()
    gi, gd = lgr.match_flann_rows(cuda(a), cuda(np.zeros((0, dim), np.float32)))                # mt = 0: -1 / 0
    lgr.sync()
    assert (gi.cpu().numpy() == -1).all() and (gd.cpu().numpy() == 0).all()
    assert lgr.match_flann_rows(cuda(np.zeros((0, dim), np.float32)), cuda(a))[0].shape == (0,)   # mq = 0: nothing
    hi, hd = lgr.match_flann_rows_host(a, np.zeros((0, dim), np.float32))
    assert (hi == -1).all() and (hd == 0).all()


def _isclose(a, b):
    """tests/flann_bf_matcher.h:12-14"""
    a, b = np.float64(a), np.float64(b)
    return np.abs(a - b) <= 1e-8 + 1e-5 * np.abs(b)


@pytest.mark.parametrize("dim", DIMS)
def test_reference_differential_test(lgr, scene, dim):
    """tests/flann_bf_matcher.h:40-97 in full width: brute force, the FLANN contract and local(identity, FLT_MAX) give the same match
    index for every query, both directions; where two indices differ the two distances are the reference's isclose.  The number of such
    queries is the statement's (SEED was chosen on the CPU among make_pair(1500) scenes for showing few of them)."""
    one = {33: lgr.match_bf, 135: lgr.match_rops, 352: lgr.match_shot}[dim]
    eye = np.eye(4, dtype=np.float32)
    for qs, ts, a, b in (("src", "tgt", 0, 1), ("tgt", "src", 1, 0)):
        q, t = scene[dim][a], scene[dim][b]
        tq, tt = cuda(q), cuda(t)
        bf_i, bf_d = [x.cpu().numpy() for x in one(tq, tt, 200000)]
        fl_i, fl_d = [x.cpu().numpy() for x in lgr.match_flann_rows(tq, tt)]
        lo_i, lo_d = [x[:, 0] for x in _dev(lgr, scene[qs], scene[ts], q, t, eye, FLT_MAX, 1)]
        s_bf_i, s_bf_d = [x[:, 0] for x in bf_ref.match(q, t, 200000, 1)]
        s_lo_i, s_lo_d = [x[:, 0] for x in ref.match(scene[qs], scene[ts], q, t, eye, FLT_MAX, 1)]
        np.testing.assert_array_equal(bf_i, fl_i)
        assert ((bf_i >= 0) == (lo_i >= 0)).all() and (bf_i >= 0).mean() > 0.5
        differ = bf_i != lo_i
        print(f"dim {dim} {qs}->{ts}: {int(differ.sum())} of {len(q)} queries differ between brute force and local; the statement: {int((s_bf_i != s_lo_i).sum())}")
        assert differ.sum() == (s_bf_i != s_lo_i).sum()
        assert _isclose(bf_d[differ], lo_d[differ]).all() and _isclose(fl_d[differ], lo_d[differ]).all()
        np.testing.assert_array_equal(ref.bits(fl_d[~differ]), ref.bits(lo_d[~differ]))   # one row, one sequential sum


def test_refusals(lgr):
    from lgr_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(9)
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16).tolist())
    for dev in (True, False):
        conv = cuda if dev else (lambda x: x)
        local = L.lgr_match_local_knn_dev if dev else L.lgr_match_local_knn
        flann = L.lgr_match_flann_rows_dev if dev else L.lgr_match_flann_rows
        p = capi._ptr
        qp, tp, q, t = conv(_cloud(rng, 4)), conv(_cloud(rng, 6)), conv(_rows(rng, 4, 34)), conv(_rows(rng, 6, 34))
        idx, dist = conv(np.full((4, 9), 7, np.int32)), conv(np.zeros((4, 9), np.float32))
        f = C.c_float

        def call(row_len=33, qp_=qp, mq=4, tp_=tp, mt=6, q_=q, t_=t, g=eye, r=1.0, k=1, idx_=idx, dist_=dist):
            return local(lgr.h, row_len, p(qp_), mq, p(tp_), mt, p(q_), p(t_), g, f(r), k, p(idx_), p(dist_))
        assert call() == 0
        assert call(row_len=34) == ERR_UNSUPPORTED and call(k=0) == ERR_UNSUPPORTED and call(k=9) == ERR_UNSUPPORTED
        for kw in (dict(qp_=None), dict(tp_=None), dict(q_=None), dict(t_=None), dict(idx_=None), dict(dist_=None), dict(g=None),
                   dict(mq=-1), dict(mt=-1), dict(r=float("nan")), dict(r=-1.0)):
            assert call(**kw) == ERR_INVALID_ARG, kw
        assert flann(lgr.h, 33, p(q), 4, p(t), 6, p(idx), p(dist)) == 0
        assert flann(lgr.h, 34, p(q), 4, p(t), 6, p(idx), p(dist)) == ERR_UNSUPPORTED
        for args in ((None, 4, p(t), 6, p(idx), p(dist)), (p(q), 4, None, 6, p(idx), p(dist)), (p(q), 4, p(t), 6, None, p(dist)),
                     (p(q), 4, p(t), 6, p(idx), None), (p(q), -1, p(t), 6, p(idx), p(dist)), (p(q), 4, p(t), -1, p(idx), p(dist))):
            assert flann(lgr.h, 33, *args) == ERR_INVALID_ARG, args
        lgr.sync()
        out = idx.cpu().numpy() if dev else idx
        assert (out.reshape(-1)[4:] == 7).all()   # the refused calls wrote nothing (the two accepted ones: the first four entries)


def test_context_reuse(lgr, scene):
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(8000, seed=5)
    p = capi.default_params(matching_id=0, bf_block_size=200000, max_iterations=20000, distance_thr=0.1, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    src, tgt = cuda(pair["src"]), cuda(pair["tgt"])
    args = (scene["src"], scene["tgt"], scene[352][0], scene[352][1], scene["guess"], 0.08, 4)
    r1 = lgr.align(src, tgt, p)
    m1 = _dev(lgr, *args)
    r2 = lgr.align(src, tgt, p)
    m2 = _dev(lgr, *args)
    np.testing.assert_array_equal(r1.matrix().view(np.uint32), r2.matrix().view(np.uint32))
    assert (r1.n_inliers, r1.iterations, r1.converged) == (r2.n_inliers, r2.iterations, r2.converged) and r1.converged == 1
    _eq(m1, m2)
    _eq(m1, ref.match(*args))
