"""GPU: tools/register_ply.py --save-features on a small synthetic pair writes the reference's histogram files -- names as
include/matching.h:274-278 gives them, rows that parse back to the prepared clouds' rows under the writer's %g rounding -- and, with a
ground truth, ids.csv equal to Context.extracted_point_ids for the target cloud."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rounded(a):
    """what a float32 reads back as after `ostream << float` (six significant digits); NaN stays NaN"""
    return np.array([float("%g" % float(v)) for v in np.asarray(a, F).reshape(-1)], np.float64).reshape(np.shape(a))


@pytest.mark.parametrize("radius", [0.25, 0.0])
def test_register_ply_save_features(lgr, tmp_path, radius):
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp, gt, out_dir = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv", "features"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "lr", "--iterations", "5000",
           "--feature-radius", str(radius), "--ground-truth", gt, "a_b", "--results", str(tmp_path / "results.csv"), "--save-features", out_dir]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    # the same clouds and parameters the tool builds
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="lr", feature_radius=radius if radius > 0 else None,
                                  iterations=5000, normals_available=ld["normals_available"])
    expected = {"ids.csv"}
    with lgr.prepare_cloud(ld["src"], prm, 0) as a, lgr.prepare_cloud(ld["tgt"], prm, 1) as b:
        levels = [{li.log2_radius: i for i, li in enumerate(c.levels())} for c in (a, b)]
        common = sorted(set(levels[0]) & set(levels[1]))
        assert len(common) == 1 if radius > 0 else len(common) >= 2
        for l2 in common:
            for c, lv, side in ((a, levels[0], "src"), (b, levels[1], "tgt")):
                name = ("histograms_%s.csv" % side) if radius > 0 else ("histograms%d_%s.csv" % (l2, side))
                expected.add(name)
                rows = c.level(lv[l2])[2]
                got = np.array([[float(v) for v in ln.split(",")] for ln in open(os.path.join(out_dir, name)).read().splitlines()])
                assert got.shape == (rows.shape[0], 34)
                np.testing.assert_array_equal(got[:, 0], np.arange(rows.shape[0]))
                np.testing.assert_array_equal(got[:, 1:], rounded(rows))      # (NaN == NaN for assert_array_equal)
    assert set(os.listdir(out_dir)) == expected
    ids = lgr.extracted_point_ids(ld["src"], ld["tgt"], formats.get_transformation(gt, "a_b"), ld["tgt"])
    lines = open(os.path.join(out_dir, "ids.csv")).read().splitlines()
    assert lines[0] == "id_src,id_tgt,x_src,x_tgt,y_src,y_tgt,z_src,z_tgt" and len(lines) == 1 + ld["tgt"].shape[0]
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    np.testing.assert_array_equal(got[:, 0], ids["id_src"])
    np.testing.assert_array_equal(got[:, 1], ids["id_tgt"])
    np.testing.assert_array_equal(got[:, 1], np.arange(ld["tgt"].shape[0]))      # the extracted points ARE the target cloud
    np.testing.assert_array_equal(got[:, 2::2], rounded(ids["xyz_src"]))
    np.testing.assert_array_equal(got[:, 3::2], rounded(ids["xyz_tgt"]))
    # the moved source point really is the nearest one
    moved = (p["T_gt"].astype(np.float64) @ np.c_[ld["src"].cpu().numpy()[:, :3], np.ones(ld["src"].shape[0])].T).T[:, :3]
    tgt = ld["tgt"].cpu().numpy()[:, :3].astype(np.float64)
    for i in (0, 17, len(tgt) - 1):
        d = np.linalg.norm(moved - tgt[i], axis=1)
        assert d[ids["id_src"][i]] <= d.min() + 1e-5
