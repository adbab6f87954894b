"""-m gpu: lgr_shot_lrf_dev / lgr_shot_dev bit-identical to the CPU reference tests/cpp/shot_ref.cpp (frames and rows, NaN rows in the
same places) on the patch fixture, on a 200k-point bench-generator cloud, and on built edge cases: isolated points, exactly 4 and 5
neighbours, NaN normals, duplicate points, the sign tie-break of the frame (s == 0), more neighbours than one sorted shell holds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shot_ref_lib as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all(), f"NaN placement differs in {int((na != nb).any(-1).sum())} rows"
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    assert not bad.any(), f"{int(bad.any(-1).sum())} rows differ, first {np.argwhere(bad.any(-1))[:5].ravel()}"


def _run(lgr, kps, surf, radius, lrf=None):
    import torch
    k = torch.from_numpy(np.ascontiguousarray(kps, np.float32)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(surf, np.float32)).cuda()
    fr_only = lgr.shot_lrf(k, s, radius)
    rows, fr = lgr.shot(k, s, radius, lrf=None if lrf is None else torch.from_numpy(lrf).cuda(), with_lrf=True)
    lgr.sync()
    return rows.cpu().numpy(), fr.cpu().numpy(), fr_only.cpu().numpy()


def _check(lgr, kps, surf, radius, lrf=None):
    rows, fr, fr_only = _run(lgr, kps, surf, radius, lrf)
    want_rows, want_fr = ref.shot(kps, surf, radius, lrf)
    _same(fr, want_fr)
    _same(rows, want_rows)
    if lrf is None:
        _same(fr_only, want_fr)
    return rows, fr


def test_patch_fixture_bit_identical(lgr):
    d = np.load(os.path.join(ROOT, "tests", "golden", "patch2k.npz"))
    surf, r = d["surf_normals"], float(d["radius"])
    rows, fr = _check(lgr, surf, surf, r)
    assert np.isfinite(rows).all(1).mean() > 0.9
    _check(lgr, d["src"][:500], surf, r)                     # key points that are not surface points
    _check(lgr, surf[:300], surf, r, lrf=fr[:300][::-1].copy())   # given frames (someone else's)


def test_bench_cloud_200k_bit_identical(lgr):
    import torch
    from lgr_amd import synthetic
    pts = synthetic.make_pair(200_000, seed=11)["src"]
    d = torch.from_numpy(pts).cuda()
    lgr.normals_knn(d, 30)
    lgr.sync()
    surf = d.cpu().numpy()
    dens = float(lgr.cloud_density(d))
    radius = float(np.sqrt(352 * dens * dens / np.pi))       # the feature radius rule of the multi-scale matching (include/matching.h:180-188)
    kps = surf[np.random.default_rng(0).choice(len(surf), 3000, replace=False)]
    rows, _ = _check(lgr, kps, surf, radius)
    assert np.isfinite(rows).all(1).mean() > 0.9


def _pt(xyz, n=(0.0, 0.0, 1.0)):
    p = np.zeros(12, np.float32)
    p[:3] = xyz; p[3] = 1; p[4:7] = n
    return p


def test_edge_cases_bit_identical(lgr):
    rng = np.random.default_rng(7)
    surf = []
    kps = []
    # isolated key point
    kps.append(_pt((100, 100, 100)))
    # exactly 4 and exactly 5 neighbours in total (the key point itself included), and 6 (5 that differ from it)
    for i, cnt in enumerate((4, 5, 6)):
        c = np.array([20.0 * (i + 1), 0, 0])
        kps.append(_pt(c))
        surf.append(_pt(c))
        for _ in range(cnt - 1):
            surf.append(_pt(c + rng.uniform(-0.5, 0.5, 3), rng.normal(size=3)))
    # NaN normals among the neighbours, duplicates of the key point and of neighbours
    c = np.array([0.0, 40.0, 0.0])
    kps.append(_pt(c))
    for j in range(40):
        q = c + rng.uniform(-0.6, 0.6, 3)
        surf.append(_pt(q, (np.nan, 0, 1) if j % 5 == 0 else rng.normal(size=3)))
        if j % 7 == 0:
            surf.append(_pt(q, rng.normal(size=3)))
    surf += [_pt(c), _pt(c)]
    # s == 0 on both axes: neighbours in +- pairs about the key point (the tie-break over the median positions decides)
    c = np.array([0.0, 0.0, 60.0])
    kps.append(_pt(c))
    for v in ((0.5, 0.1, 0.02), (0.05, 0.3, -0.01), (0.1, -0.05, 0.2), (-0.2, 0.4, 0.1)):
        surf.append(_pt(c + np.array(v))); surf.append(_pt(c - np.array(v)))
    # more neighbours than one sorted shell holds (1024): 3000 points in the ball
    c = np.array([0.0, -50.0, 0.0])
    kps.append(_pt(c))
    for q in rng.uniform(-0.5, 0.5, (3000, 3)):
        surf.append(_pt(c + q, rng.normal(size=3)))
    kps.append(_pt((np.nan, 0, 0)))
    kps, surf = np.stack(kps), np.stack(surf).astype(np.float32)
    rows, fr = _check(lgr, kps, surf, 1.0)
    assert np.isnan(rows[0]).all() and np.isnan(rows[1]).all() and np.isnan(fr[2]).all() and np.isfinite(fr[3]).all()
    assert np.isfinite(rows[4:7]).all() and np.isnan(rows[-1]).all()
    _check(lgr, kps, surf[:0], 1.0)                          # an empty surface


def test_iss_keypoints_equal_keypoint_any_rows(lgr):
    """keypoint_extraction (the reference's test): SHOT at the ISS key points equals the rows of the same points computed with every
    point as a key point, on the same surface."""
    import torch
    d = np.load(os.path.join(ROOT, "tests", "golden", "patch2k.npz"))
    surf, r = d["surf_normals"], float(d["radius"])
    s = torch.from_numpy(surf).cuda()
    idx = lgr.iss_keypoints(s, r / 2).cpu().numpy()
    assert len(idx) > 0
    every = lgr.shot(s, s, r).cpu().numpy()
    at = lgr.shot(torch.from_numpy(surf[idx]).cuda(), s, r).cpu().numpy()
    _same(at, every[idx])
