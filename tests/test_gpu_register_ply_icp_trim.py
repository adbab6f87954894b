"""GPU: tools/register_ply.py --icp 5 --icp-trim 0.7 on two small generated PLY files.  The transformations.csv row named <name>_icp holds
what Context.icp_trim returns for the same steps made here, and the tool prints that run's pairs and rmse and, beyond what --icp prints,
the candidates, the kept pairs, the cut and the scale of the first and the last iteration."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_icp_trim_row(lgr, tmp_path):
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=20000, seed=5)   # (the pair of tests/test_gpu_register_ply_icp.py: the coarse alignment succeeds on it)
    sp, tp = (str(tmp_path / n) for n in ("a.ply", "b.ply"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    out_csv = str(tmp_path / "tn.csv")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--out", out_csv, "--icp", "5", "--icp-trim", "0.7"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    tn = open(out_csv).read().splitlines()[-2:]   # (behind the file's header line)
    assert [line.split(",")[0] for line in tn] == ["a_b", "a_b_icp"]
    # the same steps here
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", iterations=20000,
                                  normals_available=ld["normals_available"])
    T = lgr.align(ld["src"], ld["tgt"], prm).matrix()
    r = lgr.icp_trim(ld["src"], ld["tgt"], T, keep=0.7, max_iterations=5)
    assert r.iterations >= 1 and r.pairs0 > 200 and r.info[0].kept < r.info[0].candidates   # not vacuous
    plain = lgr.icp_plane(ld["src"], ld["tgt"], T, max_iterations=5)
    assert not np.array_equal(plain.matrix(), r.matrix())   # the option reached the library
    for line, name, M in ((tn[0], "a_b", T), (tn[1], "a_b_icp", r.matrix())):
        assert line == name + "".join("," + formats._g(M[i][j]) for i in range(4) for j in range(4)), name
    assert f"{r.iterations} iterations of at most 5, stopped by {capi.ICP_STOP_NAMES[r.stop]} (max_dist {r.max_dist:.6g})" in out.stdout
    assert "icp (plane, robust none, keep 0.7) in" in out.stdout
    assert f"first: pairs={r.pairs0} rmse={r.rmse0:.7f}" in out.stdout and f" last: pairs={r.pairs} rmse={r.rmse:.7f}" in out.stdout
    for label, s in (("first", r.info[0]), (" last", r.info[-1])):
        assert f"{label} trim: candidates={s.candidates} kept={s.kept} cut={s.cut:.7f} scale={s.scale:.7f}" in out.stdout, out.stdout
