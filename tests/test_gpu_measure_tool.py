"""GPU: tools/register_ply.py --measure and --hypotheses with a ground truth, on PLY files written from make_pair(4000, seed 12).  The tool's
test_measurements.csv row holds the text formats.measurements_row gives for Context.measure over the same steps made here (loader, profile,
seeds: all deterministic) -- in every column but the two running-time columns, which no two runs share; a second invocation appends a
row without repeating the header; the listed hypotheses carry the numbers of Context.evaluate_gt_batch on the same set."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 119
ITERATIONS = 20000   # the tool's profile (4 x density as distance_thr, 543 correspondences) needs some thousand iterations for a first hypothesis


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from lgr_amd import formats, synthetic
    d = tmp_path_factory.mktemp("measure_tool")
    p = synthetic.make_pair(n_points=4000, seed=12)
    sp, tp, gt = (str(d / n) for n in ("a.ply", "b.ply", "gt.csv"))
    formats.write_ply(sp, p["src"], with_normals=False)
    formats.write_ply(tp, p["tgt"], with_normals=False)
    formats.save_transformation(gt, "a_b", p["T_gt"].astype(F))
    return dict(dir=d, src=sp, tgt=tp, gt=gt)


def run_tool(files, *more):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), files["src"], files["tgt"], "--keypoint", "any", "--matching", "one_sided",
           "--iterations", str(ITERATIONS), "--ground-truth", files["gt"], "a_b", "--results", str(files["dir"] / "results.csv"), *more]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def same_steps(lgr, files):
    from lgr_amd import capi, formats, profile
    ld = profile.load_pair(lgr, files["src"], files["tgt"])
    prm = profile.default_profile(capi, ld["density_src"], ld["density_tgt"], keypoint="any", matching="one_sided", iterations=ITERATIONS,
                                  normals_available=ld["normals_available"])
    return ld, prm, formats.get_transformation(files["gt"], "a_b")


def test_measure_row_and_append(lgr, files):
    from lgr_amd import formats
    path = str(files["dir"] / "test_measurements.csv")
    out = run_tool(files, "--measure", "3", "--measure-seed", str(SEED0), "--measurements", path)
    ld, prm, T_gt = same_steps(lgr, files)
    m, runs = lgr.measure(ld["src"], ld["tgt"], prm, T_gt, n_times=3, seeds=[SEED0, SEED0 + 1, SEED0 + 2])
    want = formats.csv_row(formats.measurements_row("a_b_measure", m))
    lines = open(path).read().splitlines()
    assert len(lines) == 2 and lines[0] == formats.MEASUREMENTS_HEADER == "testname,success_rate,mae,sae,mte,ste,mrmse,srmse,mtime,stime"
    got = formats.csv_row(lines[1])
    assert len(got) == len(want) == 10 and got[:8] == want[:8], (got, want)
    assert float(got[8]) > 0 and float(got[9]) >= 0   # mtime, stime: this invocation's own times
    assert m.n_success >= 1 and not np.isnan(m.mae)   # not vacuous: the row holds numbers
    assert lines[1] in out and f"success: {m.n_success}/3" in out
    for i, r in enumerate(runs):   # one line per run
        assert f"\t{i}\t{SEED0 + i}\t{r.result.converged}\t{r.eval.converged_and_overlap_ok}\t{r.result.n_inliers}\t" in out, i
    # a second invocation appends a row and leaves the header alone
    run_tool(files, "--measure", "3", "--measure-seed", str(SEED0), "--measurements", path)
    lines = open(path).read().splitlines()
    assert len(lines) == 3 and lines[0] == formats.MEASUREMENTS_HEADER and formats.csv_row(lines[2])[:8] == want[:8]
    assert sum(line == formats.MEASUREMENTS_HEADER for line in lines) == 1


def test_measure_needs_a_ground_truth(files):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "register_ply.py"), files["src"], files["tgt"], "--measure", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--measure needs --ground-truth" in out.stderr


def test_hypotheses_are_judged_in_one_batch(lgr, files):
    out = run_tool(files, "--hypotheses", "4")
    ld, prm, T_gt = same_steps(lgr, files)
    corr = lgr.correspondences(ld["src"], ld["tgt"], prm)
    res, hyps, best = lgr.ransac_multi(ld["src"], ld["tgt"], corr, prm, max_set=4)
    assert 1 <= len(hyps) <= 4 and any(h.converged for h in hyps)
    evals = lgr.evaluate_gt_batch(ld["src"], ld["tgt"], corr, [h.matrix() for h in hyps], T_gt, prm.distance_thr, [h.converged for h in hyps])
    lines = [line for line in out.splitlines() if line.startswith("\thypothesis ") and " analysis:" in line]
    assert len(lines) == len(hyps)
    for k, (line, e) in enumerate(zip(lines, evals)):
        want = (f"\thypothesis {k} analysis:\t{180.0 / np.pi * e.r_err:.7f}\t{e.t_err:.7f}\t{e.overlap_rmse:.7f}\t{e.converged_and_overlap_ok}"
                f"\t{'*' if k == best else ''}")
        assert line == want, (line, want)
