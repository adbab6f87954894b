"""The header-only C++ shim on prepared clouds: FeatureBasedCorrespondenceSearch::calculateCorrespondences goes through two lgr_cloud
objects, and AlignmentParameters::save_features writes the reference's histogram files.  On the CPU: the program compiles and links
against the library, lgr_io.hpp registers its writer.  On the GPU (tests/cpp/shim_prepared_smoke.cpp): the correspondences are those of
lgr_correspondences_ex with and without save_features, which writes both files, and saveExtractedPointIds writes ids.csv."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")


def build(tmp_path):
    """links against the in-tree library (built by __graft_entry__.build(); a missing library fails the link)"""
    exe = os.path.join(str(tmp_path), "shim_prepared_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_prepared_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_compiles_and_registers_the_writer(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "compiled" in out.stdout, out.stdout + out.stderr
    assert "saver_registered=1 stems=histograms_src,histograms-2_tgt" in out.stdout, out.stdout


@pytest.mark.gpu
def test_shim_save_features(tmp_path):
    d = tmp_path / "features"
    d.mkdir()
    out = subprocess.run([build(tmp_path), str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"corr=(\d+) equal_to_c_call=1 equal_with_save_features=1 nothing_written_without=1 src_lines=4800 tgt_lines=4800 points=4800", out.stdout)
    assert m and int(m.group(1)) > 50, out.stdout
    assert "ids_lines=4801" in out.stdout
    assert sorted(os.listdir(d)) == ["histograms_src.csv", "histograms_tgt.csv", "ids.csv"]
    first = open(d / "histograms_src.csv").readline().rstrip("\n").split(",")
    assert first[0] == "0" and len(first) == 34
    ids = [ln.split(",") for ln in open(d / "ids.csv").read().splitlines()[1:]]
    assert [int(r[1]) for r in ids] == list(range(4800))     # the extracted points are the target cloud
    # the source is the jittered scene moved; moved back by the ground truth, point i lies within the jitter of target point i
    assert sum(int(r[0]) == i for i, r in enumerate(ids)) > 4000
