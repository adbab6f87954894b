"""GPU: tools/register_ply.py --refine N.  Without the flag the tool prints and writes what it did before; with it, the same lines and rows
come first, then the refinement's: the evaluation before and after, a second transformations.csv row named <name>_refined holding
lgr_refine_plane's transform for the same steps made here, and with --ground-truth a second results.csv row under that name."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refine_rows(lgr, tmp_path):
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=20000, seed=12)
    sp, tp, gt = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    runs = {}
    for tag, extra in (("plain", []), ("refined", ["--refine", "5"])):
        out_csv, res_csv = str(tmp_path / f"{tag}_tn.csv"), str(tmp_path / f"{tag}_results.csv")
        cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
               "--out", out_csv, "--ground-truth", gt, "a_b", "--results", res_csv] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        timeless = [re.sub(r"in [0-9.]+ ms", "in # ms", line).replace(tag + "_", "") for line in out.stdout.splitlines()]
        res = [formats.csv_row(line) for line in open(res_csv).read().splitlines()]
        keep = [k for k, c in enumerate(res[0]) if c not in ("time_cs", "time_te")]   # wall-clock columns
        runs[tag] = (timeless, open(out_csv).read().splitlines(), [[row[k] for k in keep] for row in res])
    (plain_out, plain_tn, plain_res), (ref_out, ref_tn, ref_res) = runs["plain"], runs["refined"]
    # without the flag: nothing about a refinement; with it: the same output first, the same rows first
    assert not any("refined" in line for line in plain_out + plain_tn + [",".join(row) for row in plain_res])
    assert ref_out[: len(plain_out)] == plain_out and ref_tn[: len(plain_tn)] == plain_tn and ref_res[: len(plain_res)] == plain_res
    assert len(ref_tn) == len(plain_tn) + 1 and len(ref_res) == len(plain_res) + 1
    # the same steps here
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", iterations=20000,
                                  normals_available=ld["normals_available"])
    T = lgr.align(ld["src"], ld["tgt"], prm).matrix()
    r = lgr.refine_plane(ld["src"], ld["tgt"], T, score_id=prm.score_id, max_steps=5)
    for line, name, M in ((ref_tn[-2], "a_b", T), (ref_tn[-1], "a_b_refined", r.matrix())):
        assert line == name + "".join("," + formats._g(M[i][j]) for i in range(4) for j in range(4))
    tail = "\n".join(ref_out[len(plain_out):])
    assert f"{r.steps} steps of at most 5, stopped by {capi.REFINE_STOP_NAMES[r.stop]}" in tail
    assert f"before: metric={r.first.metric:.7f} inliers_rmse={r.first.rmse:.7f} inliers={r.first.n_inliers}" in tail
    assert f" after: metric={r.metric:.7f} inliers_rmse={r.rmse:.7f} inliers={r.n_inliers}" in tail
    assert "rotation error (deg):" in tail and "translation error:" in tail   # the analysis of the refined transformation
    row = dict(zip(ref_res[0], ref_res[-1]))
    assert row["testname"] == "a_b_refined"
