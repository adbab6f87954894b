"""The header-only C++ shim with matching_id "ratio": it maps to LGR_MATCH_RATIO with AlignmentParameters::ratio_k in
lgr_feature_params.ratio_k (it became "lr" before the matcher existed).  On the CPU: the mapping, compiled and linked by the caller.  On the
GPU: FeatureBasedCorrespondenceSearch with "ratio" and ratio_k 3 returns the correspondences of the C call."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")


def build(tmp_path):
    """links against the in-tree library (built by __graft_entry__.build(); a missing library fails the link)"""
    exe = os.path.join(str(tmp_path), "shim_ratio_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_ratio_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_maps_ratio_to_its_matcher(tmp_path):
    out = subprocess.run([build(tmp_path), "compile-only"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "compiled" in out.stdout, out.stdout + out.stderr
    assert "matching_id=3 ratio_k=3" in out.stdout, out.stdout


@pytest.mark.gpu
def test_shim_ratio_gives_the_correspondences_of_the_c_call(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"ratio3=(\d+) equal_to_c_call=1 differs_from_k2=1 differs_from_lr=1", out.stdout)
    assert m and int(m.group(1)) > 50, out.stdout
