"""GPU: tools/register_ply.py --hypotheses N --hypotheses-plane under a plane metric lists the set of distinct hypotheses -- one line per
member, at most one of them chosen."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_ply_hypotheses_under_combination(lgr, tmp_path):
    from lgr_amd import formats, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp = (str(tmp_path / n) for n in ("a.ply", "b.ply"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--metric", "combination", "--hypotheses", "64", "--hypotheses-plane"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    head = re.search(r"^(\d+) distinct hypotheses in ", out.stdout, flags=re.M)
    assert head, out.stdout[-1500:]
    n = int(head.group(1))
    rows = re.findall(r"^\t(\d+)\t(-?\d+)\t([\d.]+)\t([\d.naninf-]+)\t(\d+)\t([\d.]+)\t(\*?)$", out.stdout, flags=re.M)
    assert 1 <= n <= 64 and len(rows) == n and [int(r[0]) for r in rows] == list(range(n))
    assert sum(r[6] == "*" for r in rows) <= 1
