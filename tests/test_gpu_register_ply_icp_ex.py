"""GPU: tools/register_ply.py --icp N with the options of the ICP variants on two small generated PLY files: plane-to-plane residuals, a Huber
kernel, the normal gate given as an angle, the curvature weight map and a plane_eps.  The transformations.csv row named <name>_icp holds
what Context.icp_ex returns for the same steps made here, and the tool prints that run's pairs and rmse."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_icp_ex_row(lgr, tmp_path):
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=20000, seed=5)   # (the pair of tests/test_gpu_register_ply_icp.py: the coarse alignment succeeds on it)
    sp, tp = (str(tmp_path / n) for n in ("a.ply", "b.ply"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    out_csv = str(tmp_path / "tn.csv")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--out", out_csv, "--icp", "10", "--icp-shrink", "0.9", "--icp-variant", "plane2plane", "--icp-robust", "huber", "--icp-robust-scale", "0.5",
           "--icp-normal-angle", "30", "--icp-weight", "curvature", "--icp-plane-eps", "0.01"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    tn = open(out_csv).read().splitlines()[-2:]   # (behind the file's header line)
    assert [line.split(",")[0] for line in tn] == ["a_b", "a_b_icp"]
    # the same steps here
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", iterations=20000,
                                  normals_available=ld["normals_available"])
    T = lgr.align(ld["src"], ld["tgt"], prm).matrix()
    w, _ = lgr.weights(ld["src"], "curvature", with_sum=False)
    kw = dict(variant="plane2plane", robust="huber", robust_scale=0.5, min_normal_cos=math.cos(math.radians(30.0)), plane_eps=0.01, weights=w,
              max_iterations=10, shrink=0.9, min_dist=0.5 * ld["density_tgt"])
    r = lgr.icp_ex(ld["src"], ld["tgt"], T, **kw)
    assert r.iterations >= 1 and r.pairs0 > 200   # not vacuous
    plain = lgr.icp_plane(ld["src"], ld["tgt"], T, max_iterations=10, shrink=0.9, min_dist=0.5 * ld["density_tgt"])
    assert not np.array_equal(plain.matrix(), r.matrix())   # the options reached the library
    for line, name, M in ((tn[0], "a_b", T), (tn[1], "a_b_icp", r.matrix())):
        assert line == name + "".join("," + formats._g(M[i][j]) for i in range(4) for j in range(4)), name
    assert f"{r.iterations} iterations of at most 10, stopped by {capi.ICP_STOP_NAMES[r.stop]} (max_dist {r.max_dist:.6g})" in out.stdout
    assert "icp (plane2plane, robust huber 0.5, normals within 30 deg, weights curvature) in" in out.stdout
    assert f"first: pairs={r.pairs0} rmse={r.rmse0:.7f}" in out.stdout and f" last: pairs={r.pairs} rmse={r.rmse:.7f}" in out.stdout
