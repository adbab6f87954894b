"""GPU: tools/register_ply.py --alignment teaser on PLY files written from make_pair(20000, seed 11), with --matching lr and --distance-thr
0.1 (after the loader's voxel grid the smaller pairs and the automatic threshold, 4 x density, leave the search a handful of true
correspondences among hundreds compatible with each other by chance): the search, then lgr_teaser on its correspondences.  The
transformations.csv row is the text of the transform Context.teaser gives for the same steps made here (loader, profile and search are
deterministic), the ground-truth analysis is printed and its results.csv row names the alignment."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from lgr_amd import formats, synthetic
    d = tmp_path_factory.mktemp("teaser_tool")
    p = synthetic.make_pair(n_points=20000, seed=11)
    sp, tp, gt = (str(d / n) for n in ("a.ply", "b.ply", "gt.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    return dict(dir=d, src=sp, tgt=tp, gt=gt)


def tool(files, *more):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), files["src"], files["tgt"], "--keypoint", "any", "--matching", "lr",
           "--distance-thr", "0.1", "--alignment", "teaser", *more]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_tool_runs_teaser(lgr, files):
    from lgr_amd import capi, formats, profile
    out_csv, results = str(files["dir"] / "transformations.csv"), str(files["dir"] / "results.csv")
    run = tool(files, "--out", out_csv, "--ground-truth", files["gt"], "a_b", "--results", results)
    assert run.returncode == 0, run.stderr[-2000:]
    # the same steps through the binding
    ld = profile.load_pair(lgr, files["src"], files["tgt"])
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="lr", distance_thr=0.1,
                                  normals_available=ld["normals_available"])
    corr = lgr.correspondences(ld["src"], ld["tgt"], prm)
    res, info, clique, nodes, mask = lgr.teaser(ld["src"], ld["tgt"], corr, capi.default_teaser_params(prm.distance_thr))
    assert info.valid == 1 and info.n_clique >= 3 and res.n_correspondences == corr.shape[0]
    line = (f"teaser: valid=1 nodes={info.n_nodes} max_core={info.max_core} core_nodes={info.n_core} clique={info.n_clique} "
            f"rotation_iterations={info.rotation_iterations} rotation_inliers={info.n_rotation_inliers}/{info.n_clique - 1} "
            f"translation_inliers={info.n_translation_inliers}/{info.n_clique}")
    assert line in run.stdout, run.stdout
    assert f"correspondences={corr.shape[0]} inliers={res.n_inliers} " in run.stdout
    # transformations.csv holds that transform; it is the ground truth's within the noise bound
    T = formats.get_transformation(out_csv, "a_b")
    check = str(files["dir"] / "check.csv")
    formats.save_transformation(check, "a_b", res.matrix())
    assert np.array_equal(T, formats.get_transformation(check, "a_b"))
    T_gt = formats.get_transformation(files["gt"], "a_b")
    assert np.abs(T[:3, 3] - T_gt[:3, 3]).max() < prm.distance_thr and np.abs(T[:3, :3] - T_gt[:3, :3]).max() < 0.05
    # the analysis ran and its row names the alignment
    assert "rotation error (deg):" in run.stdout and "success (converged and overlap error" in run.stdout
    lines = open(results).read().splitlines()
    assert len(lines) == 2 and lines[0] == formats.RESULTS_HEADER
    row = dict(zip(formats.csv_row(lines[0]), formats.csv_row(lines[1])))
    assert row["alignment_type"] == "teaser" and row["testname"] == "a_b" and row["converged"] == "1"
    assert int(row["iteration"]) == info.rotation_iterations


def test_tool_refuses_what_lgr_align_would_refuse(files):
    for more in (("--measure", "2", "--ground-truth", files["gt"], "a_b"), ("--save-features", str(files["dir"] / "feat")), ("--hypotheses", "3")):
        run = tool(files, *more)
        assert run.returncode != 0 and ("teaser" in run.stderr or "--alignment ransac" in run.stderr), run.stderr[-500:]
