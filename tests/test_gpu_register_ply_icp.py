"""GPU: tools/register_ply.py --icp N on two small generated PLY files, combined with --refine (the ICP runs first).  The tool prints the
pairs and rmse of the first and the last iteration, appends a transformations.csv row named <name>_icp that holds lgr_icp_plane's transform
for the same steps made here, then refines from that transform (row <name>_icp_refined), and with --ground-truth writes a results.csv row
under each name."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_icp_rows(lgr, tmp_path):
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=20000, seed=5)   # (a pair the tool's coarse alignment succeeds on: about 11 degrees off, which the ICP takes below 1)
    sp, tp, gt = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    out_csv, res_csv = str(tmp_path / "tn.csv"), str(tmp_path / "results.csv")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--out", out_csv, "--ground-truth", gt, "a_b", "--results", res_csv, "--icp", "10", "--icp-shrink", "0.9", "--refine", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    tn = open(out_csv).read().splitlines()[-3:]   # (behind the file's header line)
    res = [formats.csv_row(line) for line in open(res_csv).read().splitlines()]
    assert [line.split(",")[0] for line in tn] == ["a_b", "a_b_icp", "a_b_icp_refined"]
    assert [dict(zip(res[0], row))["testname"] for row in res[1:]] == ["a_b", "a_b_icp", "a_b_icp_refined"]
    # the same steps here
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", iterations=20000,
                                  normals_available=ld["normals_available"])
    T = lgr.align(ld["src"], ld["tgt"], prm).matrix()
    r = lgr.icp_plane(ld["src"], ld["tgt"], T, max_iterations=10, shrink=0.9, min_dist=0.5 * ld["density_tgt"])
    assert r.iterations >= 1 and r.pairs0 > 500   # not vacuous
    rr = lgr.refine_plane(ld["src"], ld["tgt"], r.matrix(), score_id=prm.score_id, max_steps=2)
    for line, name, M in ((tn[0], "a_b", T), (tn[1], "a_b_icp", r.matrix()), (tn[2], "a_b_icp_refined", rr.matrix())):
        assert line == name + "".join("," + formats._g(M[i][j]) for i in range(4) for j in range(4)), name
    assert f"{r.iterations} iterations of at most 10, stopped by {capi.ICP_STOP_NAMES[r.stop]} (max_dist {r.max_dist:.6g})" in out.stdout
    assert f"first: pairs={r.pairs0} rmse={r.rmse0:.7f}" in out.stdout and f" last: pairs={r.pairs} rmse={r.rmse:.7f}" in out.stdout
    assert out.stdout.count("rotation error (deg):") == 3   # the alignment's analysis, the ICP's, the refinement's
