"""GPU: the reference's point order on the device (csrc/lgr_hash_order.hip).  lgr_hash_order_dev against a real libstdc++ container
(tests/cpp/hash_order_ref.cpp) at every rehash count +-1; lgr_downsample_order_dev / lgr_dedupe_order_dev / lgr_preprocess_order_dev
bit for bit against the oracle's ORDER_LIBSTDCXX (which IS the container) and against the host entries; the library's own self-check;
tools/register_ply.py --order reference.  Everything is exact: orders equal element by element, all 12 floats of every point bit-equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hash_order_ref_lib as H  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev_order(lgr, h, reserve=0):
    return lgr.hash_order(cuda(h.view(np.int64)), reserve=reserve).cpu().numpy()


# ---------------------------------------------------------------------------------------------- lgr_hash_order_dev
def final_buckets(n):
    """bucket count of an unreserved container holding n elements: max load factor 1, so the count a rehash fires at is the size before"""
    c = [k for k in H.rehash_counts(4 * n + 64) if k >= n]
    return c[0]


def codes(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if kind == "voxel":                                     # HashEigen of real voxel keys
        return H.hash_voxel(H.distinct_keys(n, 2000, seed))[1]
    if kind == "equal":                                     # everything in one bucket
        return np.full(n, 0x1234567, np.uint64)
    if kind == "multiples":                                 # one bucket under the final count, spread under the earlier ones
        return np.arange(n, dtype=np.uint64) * np.uint64(final_buckets(n))
    assert kind == "high"                                   # >= 2^63: the modulo must be unsigned
    return rng.integers(2 ** 63, 2 ** 64, n, dtype=np.uint64)


@pytest.mark.parametrize("kind", ["random", "voxel", "equal", "multiples", "high"])
def test_hash_order(lgr, kind):
    for n in H.sizes():
        h = codes(kind, n, seed=n + 1)
        for reserve in (0, n + (n % 5) * 211):               # 0 = grown by itself (also "reserve(0)"); else >= n, below and above the LDS limit
            # the real container; one bucket makes its insertions quadratic, so the 42 k case of "equal" takes the header's host rule,
            # which tests/test_hash_order_ref.py pins against the container on the same kind of codes
            want = H.rule(h, reserve) if kind == "equal" and n > 6000 else H.replay(h, reserve)
            got = dev_order(lgr, h, reserve)
            assert np.array_equal(got, want), (kind, n, reserve)
    # a reserve far above n: one epoch whose bucket table does not fit the one-workgroup kernel
    h = codes(kind, 300, seed=7)
    assert np.array_equal(dev_order(lgr, h, 100000), H.replay(h, 100000))


def test_hash_order_errors(lgr):
    import torch
    from lgr_amd import capi
    f = capi.lib().lgr_hash_order_dev
    h = torch.zeros(16, dtype=torch.int64, device="cuda")
    o = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    hp, op = C.c_void_p(h.data_ptr()), C.c_void_p(o.data_ptr())
    assert f(lgr.h, hp, 16, C.c_longlong(5), op) == capi.ERR_INVALID_ARG          # reserve in (0, n)
    assert f(lgr.h, hp, 16, C.c_longlong(15), op) == capi.ERR_INVALID_ARG
    assert f(lgr.h, hp, 16, C.c_longlong(-1), op) == capi.ERR_INVALID_ARG
    assert f(lgr.h, None, 16, C.c_longlong(0), op) == capi.ERR_INVALID_ARG
    assert f(lgr.h, hp, 16, C.c_longlong(0), None) == capi.ERR_INVALID_ARG
    assert f(lgr.h, hp, -1, C.c_longlong(0), op) == capi.ERR_INVALID_ARG
    assert f(lgr.h, None, 0, C.c_longlong(0), None) == 0                          # n = 0: LGR_OK ...
    assert f(lgr.h, hp, 0, C.c_longlong(0), op) == 0
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == -7).all()                                          # ... and nothing written
    assert f(lgr.h, hp, 16, C.c_longlong(16), op) == 0
    assert np.array_equal(o.cpu().numpy(), np.arange(15, -1, -1))                 # one bucket: newest first


def test_selfcheck(lgr):
    assert lgr.selfcheck_hash_order(50000, spread=2000, seed=3) == 0
    assert lgr.selfcheck_hash_order(50000, spread=2000, seed=3, reserve=50000) == 0
    assert lgr.selfcheck_hash_order(4000, spread=3, seed=4) == 0                  # 27 elements


# ---------------------------------------------------------------------------------------------- lgr_downsample_order_dev
@pytest.fixture(scope="module")
def pair_cloud():
    from lgr_amd import synthetic
    return np.ascontiguousarray(synthetic.make_pair(30000, seed=41)["src"])


def voxel_just_above(oracle, pts, count, slack=48):
    """a voxel size whose grid over pts has a few more than `count` voxels (bisection on the CPU; the count falls as the voxel grows)"""
    lo, hi = 1e-3, 10.0
    for _ in range(60):
        mid = np.float32(np.sqrt(lo * hi))
        nv = len(oracle.downsample(pts, float(mid)))
        if count < nv <= count + slack:
            return float(mid), nv
        lo, hi = (mid, hi) if nv > count else (lo, mid)
    raise AssertionError("no voxel size found")


def downsample_order_dev(lgr, d_pts, voxel, order, out=None):
    """lgr_downsample_order_dev itself, for both orders"""
    import torch
    from lgr_amd import capi
    out = torch.empty((d_pts.shape[0], 12), dtype=torch.float32, device="cuda") if out is None else out
    n = C.c_int(0)
    lgr.check(capi.lib().lgr_downsample_order_dev(lgr.h, C.c_void_p(d_pts.data_ptr()), d_pts.shape[0], C.c_float(voxel), int(order),
                                                  C.c_void_p(out.data_ptr()), C.byref(n)))
    return out[: n.value]


def test_downsample_reference_order(lgr, oracle, pair_cloud):
    from lgr_amd import capi
    pts = pair_cloud
    count = [c for c in H.rehash_counts(20000) if c > 6000][0]                    # past what the one-workgroup kernel holds
    v_edge, nv = voxel_just_above(oracle, pts, count)
    assert count < nv <= count + 48
    v_small = voxel_just_above(oracle, pts, 2000, slack=1500)[0]                  # a few thousand voxels: the one-workgroup kernel alone
    d = cuda(pts)
    for voxel in (v_edge, v_small):
        ref = oracle.downsample(pts, voxel, oracle.ORDER_LIBSTDCXX)
        got = lgr.downsample(d, voxel, order=capi.ORDER_REFERENCE).cpu().numpy()
        assert same(got, ref), voxel
        assert same(lgr.downsample_host(pts, voxel, order=capi.ORDER_REFERENCE), ref)
        can = lgr.downsample(d, voxel).cpu().numpy()
        assert same(downsample_order_dev(lgr, d, voxel, capi.ORDER_CANONICAL).cpu().numpy(), can)
        assert same(can, oracle.downsample(pts, voxel)) and not same(can, ref)
        for order, want in ((capi.ORDER_REFERENCE, ref), (capi.ORDER_CANONICAL, can)):   # in place
            buf = d.clone()
            assert same(downsample_order_dev(lgr, buf, voxel, order, out=buf).cpu().numpy(), want)


def test_downsample_reference_order_edges(lgr, oracle, pair_cloud):
    from lgr_amd import capi
    one = pair_cloud[:500].copy()
    one[:, :3] = one[:, :3] * np.float32(1e-3) + np.float32(5.0)                  # all points in one voxel
    got = lgr.downsample(cuda(one), 1.0, order=capi.ORDER_REFERENCE).cpu().numpy()
    assert len(got) == 1 and same(got, oracle.downsample(one, 1.0, oracle.ORDER_LIBSTDCXX))
    bad = pair_cloud[:6000].copy()
    bad[::7, 0] = np.nan; bad[5::11, 1] = np.inf; bad[3::13, 2] = np.nan          # non-finite points are skipped
    ref = oracle.downsample(bad, 0.4, oracle.ORDER_LIBSTDCXX)
    got = lgr.downsample(cuda(bad), 0.4, order=capi.ORDER_REFERENCE).cpu().numpy()
    assert same(got, ref) and len(ref) > 13
    nothing = bad[:40].copy()
    nothing[:, 0] = np.nan
    assert len(lgr.downsample(cuda(nothing), 0.4, order=capi.ORDER_REFERENCE)) == 0


# ---------------------------------------------------------------------------------------------- dedupe / preprocess
@pytest.fixture(scope="module")
def dup_cloud():
    """the cloud of tests/test_gpu_preprocess.py: 4 000 duplicates with another payload"""
    from lgr_amd import synthetic
    pair = synthetic.make_pair(30000, seed=41)
    pts = pair["src"]
    rng = np.random.default_rng(1)
    dup = pts[rng.integers(0, len(pts), 4000)].copy()
    dup[:, 4:7] = 0.5
    pts = np.concatenate([pts[:10000], dup[:2000], pts[10000:], dup[2000:]])
    pts[:, 8] = rng.uniform(0, 5, len(pts))
    return np.ascontiguousarray(pts), pair["vp_src"]


def test_dedupe_reference_order(lgr, oracle, dup_cloud):
    from lgr_amd import capi
    pts = dup_cloud[0].copy()
    pts[7, 0] = 0.0; pts[8, 0] = -0.0; pts[8, 1:3] = pts[7, 1:3]                  # -0 == +0: duplicates
    pts[20, 1] = np.nan; pts[21] = pts[20]                                         # NaN never equals: both kept
    ref = oracle.dedupe(pts, order=oracle.ORDER_LIBSTDCXX)
    ref[:, 8] = 1.0
    got = lgr.dedupe(cuda(pts), order=capi.ORDER_REFERENCE).cpu().numpy()
    assert same(got, ref) and len(ref) < len(pts)
    can = lgr.dedupe(cuda(pts)).cpu().numpy()
    assert len(can) == len(ref) and not same(can, ref)
    assert same(lgr.dedupe(cuda(pts), order=capi.ORDER_CANONICAL).cpu().numpy(), can)
    one = lgr.dedupe(cuda(pts[:1]), order=capi.ORDER_REFERENCE).cpu().numpy()
    assert len(one) == 1 and same(one[:, :8], pts[:1, :8]) and one[0, 8] == 1.0


def test_preprocess_reference_order_dev(lgr, oracle, dup_cloud):
    from lgr_amd import capi
    pts, vp = dup_cloud
    ref, vox = oracle.preprocess(pts, vp=vp, order=oracle.ORDER_LIBSTDCXX)
    got, vox_g = lgr.preprocess(cuda(pts), vp=vp, order=capi.ORDER_REFERENCE)
    assert np.float32(vox) == np.float32(vox_g)
    assert same(got.cpu().numpy(), ref) and 100 < len(ref) < len(pts)
    can, _ = lgr.preprocess(cuda(pts), vp=vp)
    assert len(can) == len(ref) and not same(can.cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------- the tool
def test_register_ply_reference_order(lgr, tmp_path):
    from lgr_amd import formats, profile, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp, out_csv = (str(tmp_path / n) for n in ("a.ply", "b.ply", "transformations.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided",
           "--iterations", "20000", "--order", "reference", "--out", out_csv]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    T = formats.get_transformation(out_csv, "a_b")
    assert T.shape == (4, 4) and np.isfinite(T).all() and np.allclose(T[3], [0, 0, 0, 1])
    ld = profile.load_pair(lgr, sp, tp)                                            # the canonical loader: the same point sets, another numbering
    for side, name in (("src", "a.ply"), ("tgt", "b.ply")):
        line = [ln for ln in out.stdout.splitlines() if ln.startswith(name + ":")][0]
        assert f"-> {ld[side].shape[0]} after preprocessing" in line, line
