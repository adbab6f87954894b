"""tools/register_ply.py --matching ratio --ratio-k K.  On the CPU: formats writes the matching id as the reference's name logic does
(constructName src/common.cpp:1195-1196, operator<< src/analysis.cpp:304-305: 'ratio' followed by ratio_k).  On the GPU: a run with
--matching ratio --ratio-k 3 writes ratio3 into the matching_type column of results.csv and reports the correspondences that
lgr_correspondences gives for the same steps made here."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_matching_name_carries_ratio_k():
    from lgr_amd import formats
    assert formats.matching_name("ratio", 3) == "ratio3" and formats.matching_name("ratio") == "ratio2"
    assert [formats.matching_name(m, 3) for m in ("lr", "one_sided", "cluster")] == ["lr", "one_sided", "cluster"]
    cols = formats.RESULTS_HEADER.split(",")
    at = cols.index("matching_type")
    assert formats.results_row(matching_type="ratio", ratio_k=5, randomness=1).split(",")[at] == "ratio5"
    assert formats.results_row(matching_type="ratio", randomness=1).split(",")[at] == "ratio2"
    assert formats.results_row(matching_type="cluster", ratio_k=5).split(",")[at] == "cluster"
    assert len(formats.results_row(matching_type="ratio", ratio_k=5).split(",")) == len(cols)      # ratio_k is no column


@pytest.mark.gpu
def test_register_ply_ratio(lgr, tmp_path):
    from lgr_amd import capi, formats, profile, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp, gt, res_csv = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv", "results.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "ratio", "--ratio-k", "3",
           "--iterations", "20000", "--ground-truth", gt, "a_b", "--results", res_csv]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ld = profile.load_pair(lgr, sp, tp)
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="ratio", iterations=20000,
                                  normals_available=ld["normals_available"])
    assert prm.matching_id == capi.MATCH_RATIO
    corr3 = lgr.correspondences(ld["src"], ld["tgt"], prm, descriptor=capi.feature_params("fpfh", ratio_k=3))
    corr2 = lgr.correspondences(ld["src"], ld["tgt"], prm, descriptor=capi.feature_params("fpfh", ratio_k=2))
    assert len(corr3) > 0 and len(corr3) != len(corr2)
    lines = open(res_csv).read().splitlines()
    assert len(lines) == 2 and lines[0] == formats.RESULTS_HEADER
    got = dict(zip(formats.csv_row(lines[0]), formats.csv_row(lines[1])))
    assert got["matching_type"] == "ratio3" and got["randomness"] == "1" and got["correspondences"] == str(len(corr3))
    # the flags are checked before any work
    bad = subprocess.run(cmd[:4] + ["--matching", "ratio", "--ratio-k", "9"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--ratio-k takes 2 .. 8" in bad.stderr
