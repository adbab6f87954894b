"""The header-only C++ shim with randomness > 1: matchBF<FPFH | SHOT | RoPS135> returns k-valued MultivaluedCorrespondence lists in the
reference's order (it threw before the k-nearest matcher existed); matchFLANN keeps throwing.  On the CPU: the caller compiles and links."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")


def build(tmp_path):
    """links against the in-tree library (built by __graft_entry__.build(); a missing library fails the link)"""
    exe = os.path.join(str(tmp_path), "shim_knn_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-O0", os.path.join(ROOT, "tests", "cpp", "shim_knn_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_knn_compiles_and_links(tmp_path):
    out = subprocess.run([build(tmp_path), "compile-only"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "compiled" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_match_bf_returns_k_lists(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fpfh_lists=1 shot_lists=1 rops_lists=1" in out.stdout, out.stdout
    assert "flann_k3 threw=1" in out.stdout and "bf_k9 threw=1" in out.stdout, out.stdout
