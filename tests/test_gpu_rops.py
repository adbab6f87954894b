"""-m gpu: lgr_gravity_lrf_dev and lgr_rops_dev bit-identical to the CPU reference tests/cpp/rops_ref.cpp (gravity frames with the SHOT
frames of tests/cpp/shot_ref.cpp where the angle test fails; RoPS rows on those frames) on the patch fixture, on a 200k-point
bench-generator cloud, and on built edge cases: vertical normals (SHOT fallback), NaN normals, isolated points, collinear and coplanar
supports, a NaN key point, and key points with more support points than the kernel's LDS cache holds (1024)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rops_ref_lib as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all(), f"NaN placement differs in {int((na != nb).any(-1).sum())} rows"
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    assert not bad.any(), f"{int(bad.any(-1).sum())} rows differ, first {np.argwhere(bad.any(-1))[:5].ravel()}"


def _check(lgr, kps, surf, radius):
    import torch
    kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
    k, s = torch.from_numpy(kps).cuda(), torch.from_numpy(surf).cuda()
    fr = lgr.gravity_lrf(k, s, radius)
    rows = lgr.rops(k, s, radius, fr)
    lgr.sync()
    fr, rows = fr.cpu().numpy(), rows.cpu().numpy()
    want_fr = ref.gravity_lrf(kps, surf, radius)
    _same(fr, want_fr)
    _same(rows, ref.rops(kps, surf, radius, want_fr))
    return rows, fr


def test_patch_fixture_bit_identical(lgr):
    d = np.load(os.path.join(ROOT, "tests", "golden", "patch2k.npz"))
    surf, r = d["surf_normals"], float(d["radius"])
    rows, fr = _check(lgr, surf, surf, r)
    assert np.isfinite(rows).all() and (np.abs(rows).sum(1) > 0.5).mean() > 0.9
    _check(lgr, d["src"][:500], surf, r)                     # key points that are not surface points
    # host entry points
    fr_h = lgr.gravity_lrf_host(surf[:300], surf, r)
    _same(fr_h, fr[:300])
    _same(lgr.rops_host(surf[:300], surf, r, fr_h), rows[:300])


def test_bench_cloud_200k_bit_identical(lgr):
    import torch
    from lgr_amd import synthetic
    pts = synthetic.make_pair(200_000, seed=11)["src"]
    d = torch.from_numpy(pts).cuda()
    lgr.normals_knn(d, 30)
    lgr.sync()
    surf = d.cpu().numpy()
    dens = float(lgr.cloud_density(d))
    radius = float(np.sqrt(352 * dens * dens / np.pi))
    kps = surf[np.random.default_rng(0).choice(len(surf), 3000, replace=False)]
    _, fr = _check(lgr, kps, surf, radius)
    fail = ref.gravity_only(kps)[1]
    print(f"200k cloud: {int(fail.sum())} of {len(kps)} key points take the SHOT frame")
    assert 0 < fail.sum() < len(kps)


def _pt(xyz, n=(1.0, 0.0, 0.0)):
    p = np.zeros(12, np.float32)
    p[:3] = xyz; p[3] = 1; p[4:7] = n
    return p


def test_edge_cases_bit_identical(lgr):
    rng = np.random.default_rng(7)
    surf, kps = [], []
    kps.append(_pt((100, 100, 100)))                                  # isolated, horizontal normal
    kps.append(_pt((100, 100, 100), (0, 0, 1)))                       # isolated, vertical normal: SHOT fallback -> NaN frame
    c = np.array([0.0, 40.0, 0.0])                                    # NaN normal (SHOT fallback) and vertical normals with support
    for n in ((np.nan, 0, 0), (0, 0, 1), (0, 0, -1), (0.01, 0, 1), (0.05, 0, 1)):
        kps.append(_pt(c, n))
    for j in range(60):
        surf.append(_pt(c + rng.uniform(-0.6, 0.6, 3), rng.normal(size=3)))
    surf.append(_pt(c))
    c = np.array([20.0, 0.0, 0.0])                                    # collinear support
    kps.append(_pt(c, (0.3, 0.2, 0.9)))
    for t in np.linspace(-0.9, 0.9, 25):
        surf.append(_pt(c + t * np.array([0.3, -0.5, 0.2])))
    c = np.array([40.0, 0.0, 0.0])                                    # coplanar support (a horizontal plane through the key point)
    kps.append(_pt(c, (0.6, 0.0, 0.8)))
    kps.append(_pt(c, (0.0, 0.0, 1.0)))
    for q in rng.uniform(-0.6, 0.6, (80, 2)):
        surf.append(_pt(c + np.array([q[0], q[1], 0.0]), (0, 0, 1)))
    c = np.array([60.0, 0.0, 0.0])                                    # a key point with one support point: itself
    kps.append(_pt(c, (1, 0, 0)))
    surf.append(_pt(c))
    c = np.array([0.0, -50.0, 0.0])                                   # 3000 support points: more than the LDS cache holds
    kps.append(_pt(c, (0.0, 0.7, 0.7)))
    kps.append(_pt(c, (0.0, 0.0, 1.0)))
    for q in rng.uniform(-0.5, 0.5, (3000, 3)):
        surf.append(_pt(c + q, rng.normal(size=3)))
    kps.append(_pt((np.nan, 0, 0)))
    kps, surf = np.stack(kps), np.stack(surf).astype(np.float32)
    rows, fr = _check(lgr, kps, surf, 1.0)
    assert (rows[0] == 0).all() and (rows[1] == 0).all() and np.isnan(fr[1]).all() and (rows[-1] == 0).all()
    assert not np.isnan(rows).any()
    _check(lgr, kps, surf[:0], 1.0)                                   # an empty surface: zero rows everywhere
