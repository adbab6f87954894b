"""The header-only C++ shim's hypothesis-set mode under a plane metric: SampleConsensusPrerejectiveOMP::align() with
LGR_SAVE_MULTIPLE_HYPOTHESES calls lgr_ransac_multi_ex for every metric_id.  tests/cpp/shim_hypotheses_plane_smoke.cpp defines the macro.
On the CPU: it compiles and links.  On the GPU: align() under metric_id "combination" returns lgr_ransac_multi_ex's bytes."""
import os
import re
import subprocess

import numpy as np
import pytest

import hypotheses_plane_ref_lib as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_hypotheses_plane_smoke")
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_hypotheses_plane_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_hypotheses_plane_builds(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built ok" in out.stdout, out.stdout + out.stderr


def hex16(M):
    return "".join("%08x" % int(v) for v in np.ascontiguousarray(np.asarray(M, F).T.reshape(16)).view(np.uint32))


def bits(v):
    return "%08x" % int(np.asarray(v, F).view(np.uint32))


@pytest.mark.gpu
def test_shim_align_under_combination(tmp_path, lgr):
    from lgr_amd import capi
    prob = HP.scene_a(4000, 0.30, 0.18)
    iters = 6000
    path = os.path.join(str(tmp_path), "problem.bin")
    with open(path, "wb") as f:
        for a in (prob["src"], prob["tgt"]):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.int32(prob["corr"].shape[0]).tobytes()); f.write(np.ascontiguousarray(prob["corr"]).tobytes())
        f.write(np.int32(iters).tobytes())
    out = subprocess.run([build(tmp_path), path, "combination"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    g = dict(re.findall(r"^(\w+)=(.*)$", out.stdout, flags=re.M))
    p = capi.default_params(metric_id=capi.METRIC_COMBINATION, score_id=capi.SCORE_MSE, distance_thr=0.05, max_iterations=iters)
    mres, hyps, bi = lgr.ransac_multi_ex_host(prob["src"], prob["tgt"], prob["corr"], p, 64)
    assert len(hyps) >= 2 and bi >= 0
    assert g["T0"] == hex16(mres.matrix()) and int(g["iterations"]) == mres.iterations and int(g["converged"]) == mres.converged
    assert int(g["n_hypotheses"]) == len(hyps) and int(g["best"]) == bi
    for k, h in enumerate(hyps):
        assert g["H%d" % k] == hex16(h.matrix()) and g["L%d" % k] == hex16(h.loop_matrix())
        assert g["h%d" % k] == "%d %s %s %d %d %s" % (h.iteration, bits(h.loop_metric), bits(h.metric), h.n_inliers, h.converged, bits(h.uniformity))
