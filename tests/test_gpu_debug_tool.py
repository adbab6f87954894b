"""GPU: tools/register_ply.py --debug-dir on a small synthetic pair writes the files of generateDebugFiles / compareHypotheses: the expected
names, coloured clouds of the right sizes, distance CSVs whose rows are the temperatures below the threshold, compareOverlaps' two lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_ply_debug_dir(lgr, tmp_path):
    from lgr_amd import formats, synthetic
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp, gt, dbg = (str(tmp_path / n) for n in ("a.ply", "b.ply", "gt.csv", "debug"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), sp, tp, "--keypoint", "any", "--matching", "one_sided", "--iterations", "20000",
           "--metric", "weighted_closest_plane", "--weight", "curvature", "--ground-truth", gt, "a_b", "--results", str(tmp_path / "results.csv"),
           "--debug-dir", dbg]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    expected = {"downsampled_src.ply", "downsampled_tgt.ply", "weights.ply"}
    for stem in ("temperature", "temperature_gt"):
        for side in ("src", "tgt"):
            expected |= {f"{stem}_distances_{side}.csv", f"{stem}_dists_{side}.ply", f"{stem}_normal_diffs_{side}.ply"}
    assert set(os.listdir(dbg)) == expected
    src, _ = formats.read_ply(os.path.join(dbg, "downsampled_src.ply"))
    tgt, _ = formats.read_ply(os.path.join(dbg, "downsampled_tgt.ply"))
    for stem in ("temperature", "temperature_gt"):
        for side, n in (("src", len(src)), ("tgt", len(tgt))):
            a, fa = formats.read_ply(os.path.join(dbg, f"{stem}_dists_{side}.ply"))
            b, _ = formats.read_ply(os.path.join(dbg, f"{stem}_normal_diffs_{side}.ply"))
            assert len(a) == len(b) == n and formats.has_normals(fa) and np.array_equal(a.view(np.uint32), b.view(np.uint32))   # ASCII reads back exactly
            assert open(os.path.join(dbg, f"{stem}_dists_{side}.ply"), "rb").read(40).startswith(b"ply\nformat ascii")
            rows = open(os.path.join(dbg, f"{stem}_distances_{side}.csv")).read().splitlines()
            col = formats.read_ply_colors(os.path.join(dbg, f"{stem}_dists_{side}.ply"))
            # getColor(distance_max) is black; a temperature within 1 / 765 of it still rounds to black, anything else below it does not.
            # The clouds overlap at the ground truth; whether the found transformation is any good is not this test's business.
            lit = int((col != 0).sum())
            assert rows[0] == "value" and lit <= len(rows) - 1 <= lit + max(8, n // 50), (stem, side, lit, len(rows) - 1)
            assert lit >= n // 10 or stem == "temperature", (stem, side, lit, out.stdout[-1500:])
    # the ground-truth-aligned source of downsampled_src.ply is the moved cloud of the temperature_gt files
    g, _ = formats.read_ply(os.path.join(dbg, "temperature_gt_normal_diffs_src.ply"))
    assert np.array_equal(g[:, :3].view(np.uint32), src[:, :3].view(np.uint32))
    assert set(np.unique(formats.read_ply_colors(os.path.join(dbg, "downsampled_tgt.ply")))) - {0xf8c471} != set()   # some point is not a plain key point
    assert "\tincorrect hypothesis: " in out.stdout and "\t  correct hypothesis: " in out.stdout and "weighted points" in out.stdout
