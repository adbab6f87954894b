"""The header-only C++ shim's refineTransformation (both overloads).  On the CPU: the caller tests/cpp/shim_refine_smoke.cpp compiles,
links and sees the ABI's defaults.  On the GPU: every figure it prints for closest_plane and weighted_closest_plane equals the C ABI's
lgr_refine_plane on the same pair bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref_lib as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_refine_smoke")
    assert os.path.exists(os.path.join(CSRC, "liblgr_hip.so")), "build the library first (__graft_entry__.build())"
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_refine_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_refine_builds(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_refine_equals_c_abi(tmp_path, lgr, oracle):
    from lgr_amd import capi
    exe = build(tmp_path)
    p = R.make_pair(oracle)
    src, tgt, T0 = p["src"], p["tgt"], p["T0"]
    m = R.GROUP + 2
    path = os.path.join(str(tmp_path), "pair.bin")
    with open(path, "wb") as f:
        for a in (src, tgt):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.ascontiguousarray(T0.T.reshape(16), F).tobytes())
    out = subprocess.run([exe, path, str(m)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(re.findall(r"(\w+)=(\w+)", out.stdout))

    def bits(v):
        return "%08x" % int(np.asarray(v, F).view(np.uint32))
    for name, mp in (("closest_plane", None), ("weighted_closest_plane", capi.metric_params("exp_curvature"))):
        r = lgr.refine_plane_host(src, tgt, T0, capi.SCORE_MSE, m, metric_params=mp)
        assert 1 <= r.steps <= m and r.metric > r.first.metric > 0   # not vacuous
        assert (int(got[name + "_steps"]), int(got[name + "_stop"]), int(got[name + "_inliers"]), int(got[name + "_first_inliers"])) == (
            r.steps, r.stop, r.n_inliers, r.first.n_inliers)
        for k, v in (("metric", r.metric), ("rmse", r.rmse), ("first_metric", r.first.metric), ("threshold", r.threshold)):
            assert got[f"{name}_{k}"] == bits(v), (name, k)
        assert got[name + "_T"] == "".join(bits(v) for v in r.transformation)
    assert got["closest_plane_metric"] != got["weighted_closest_plane_metric"]
