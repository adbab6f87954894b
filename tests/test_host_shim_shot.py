"""The header-only C++ shim with the reference's default AlignmentParameters (descriptor "shot", include/common.h:148).  On the CPU: a
reference-style caller of the SHOT surface (lgr::SHOT, estimateFeatures<SHOT>, matchBF<SHOT>, the lrf_id rules) compiles and links with
plain g++.  On the GPU: it registers the corner scene of tests/point2plane_distance.cpp through alignPointClouds (the shim threw for 'shot'
before the SHOT path existed); FPFH with lrf_id "gravity" still registers (FPFH never reads the frames), SHOT with it is refused; the
SHOT rows of estimateFeatures<SHOT> match themselves through matchBF<SHOT>."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_shot_smoke")
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_shot_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_shot_compiles_and_links(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_shim_registers_corner_scene_with_default_descriptor(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"descriptor=shot converged=1 correspondences=(\d+) rot_err=(\S+) trans_err=(\S+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) > 100 and float(m.group(2)) < 0.01 and float(m.group(3)) < 1.0
    m = re.search(r"fpfh_gravity converged=(\d+) correspondences=(\d+)", out.stdout)
    assert m and int(m.group(2)) > 0, out.stdout
    assert "shot_gravity unsupported=1" in out.stdout
    m = re.search(r"shot_rows=(\d+) finite=(\d+) framed=(\d+) self_distance_zero=(\d+)", out.stdout)
    assert m, out.stdout
    rows, finite, framed, self_zero = (int(g) for g in m.groups())
    assert rows > 100 and finite > 0.5 * rows and framed >= finite and self_zero == finite
