"""The header-only C++ shim's hypothesis-set mode: chooseBestHypothesis (include/hypotheses.h:14-16) and
SampleConsensusPrerejectiveOMP::align() under LGR_SAVE_MULTIPLE_HYPOTHESES, the shim's mirror of the reference's SAVE_MULTIPLE_HYPOTHESES
(src/sac_prerejective_omp.cpp:11).  tests/cpp/shim_hypotheses_smoke.cpp is compiled with the macro and without it.  On the CPU: both
compile and link.  On the GPU: the build with the macro returns lgr_ransac_multi's bytes, the build without it what align() returned
before the mode existed (lgr_ransac_ex's bytes, an empty set)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32


def build(tmp_path, multi):
    exe = os.path.join(str(tmp_path), "shim_hypotheses_smoke_%d" % multi)
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    subprocess.check_call(["g++", "-std=c++17", "-O1"] + (["-DLGR_SAVE_MULTIPLE_HYPOTHESES"] if multi else []) +
                          [os.path.join(ROOT, "tests", "cpp", "shim_hypotheses_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


@pytest.mark.parametrize("multi", [0, 1])
def test_shim_hypotheses_builds(tmp_path, multi):
    out = subprocess.run([build(tmp_path, multi)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built multi=%d ok" % multi in out.stdout, out.stdout + out.stderr


def hex16(M):
    return "".join("%08x" % int(v) for v in np.ascontiguousarray(np.asarray(M, F).T.reshape(16)).view(np.uint32))


def bits(v):
    return "%08x" % int(np.asarray(v, F).view(np.uint32))


@pytest.mark.gpu
def test_shim_align_with_and_without_the_macro(tmp_path, lgr):
    from lgr_amd import capi, synthetic
    prob = synthetic.make_two_mode_problem(n_pts=4000, c=1500, f1=0.30, f2=0.18, seed=11)
    iters = 6000
    path = os.path.join(str(tmp_path), "problem.bin")
    with open(path, "wb") as f:
        for a in (prob["src"], prob["tgt"]):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.int32(prob["corr"].shape[0]).tobytes()); f.write(np.ascontiguousarray(prob["corr"]).tobytes())
        f.write(np.int32(iters).tobytes())
    p = capi.default_params(metric_id=capi.METRIC_UNIFORMITY, score_id=capi.SCORE_MSE, distance_thr=0.05, max_iterations=iters)
    got = {}
    for multi in (0, 1):
        out = subprocess.run([build(tmp_path, multi), path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        got[multi] = dict(re.findall(r"^(\w+)=(.*)$", out.stdout, flags=re.M))
        assert int(got[multi]["multi"]) == multi
    # without the macro: align() is the single-hypothesis call it has always been
    res, _ = lgr.ransac_ex(lgr.torch.from_numpy(prob["src"]).cuda(), lgr.torch.from_numpy(prob["tgt"]).cuda(), prob["corr"], p)
    g = got[0]
    assert g["T0"] == hex16(res.matrix()) and int(g["iterations"]) == res.iterations and int(g["converged"]) == res.converged
    assert int(g["n_hypotheses"]) == 0 and int(g["best"]) == -1
    assert g["C0"] == hex16(np.eye(4))   # chooseBestHypothesis of no hypotheses: identity
    # with it: lgr_ransac_multi's set, member by member, and its choice
    mres, hyps, bi = lgr.ransac_multi_host(prob["src"], prob["tgt"], prob["corr"], p, 64)
    g = got[1]
    assert len(hyps) >= 2 and bi >= 0
    assert g["T0"] == hex16(mres.matrix()) and int(g["iterations"]) == mres.iterations and int(g["converged"]) == mres.converged
    assert int(g["n_hypotheses"]) == len(hyps) and int(g["best"]) == bi
    for k, h in enumerate(hyps):
        assert g["H%d" % k] == hex16(h.matrix()) and g["L%d" % k] == hex16(h.loop_matrix())
        assert g["h%d" % k] == "%d %s %s %d %d %s" % (h.iteration, bits(h.loop_metric), bits(h.metric), h.n_inliers, h.converged, bits(h.uniformity))
    assert g["C0"] == hex16(hyps[bi].matrix())
