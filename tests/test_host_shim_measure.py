"""The header-only C++ shim's measureAlignment, calculateMean and calculateStandardDeviation.  On the CPU: the caller
tests/cpp/shim_measure_smoke.cpp compiles, links and gets the hand-derived answers of tests/test_measure_ref.py from the two templates.  On the
GPU: the aggregate and every run it prints for fixed seeds equal the C ABI's lgr_measure on the same pair bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32
SEEDS = [119, 120, 121, 122]   # chosen with the oracle's RANSAC, max_iterations 150: see tests/test_gpu_measure.py


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_measure_smoke")
    assert os.path.exists(os.path.join(CSRC, "liblgr_hip.so")), "build the library first (__graft_entry__.build())"
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_measure_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_measure_builds(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_measure_equals_c_abi(tmp_path, lgr):
    import torch
    from lgr_amd import capi, synthetic
    exe = build(tmp_path)
    p = synthetic.make_pair(n_points=4000, seed=12)
    clouds = {}
    for side in ("src", "tgt"):
        d = torch.from_numpy(np.ascontiguousarray(p[side])).cuda()
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        clouds[side] = d.cpu().numpy()
    thr = F(2 * lgr.cloud_density(torch.from_numpy(clouds["tgt"]).cuda()))
    G = p["T_gt"].astype(F)
    path = os.path.join(str(tmp_path), "pair.bin")
    with open(path, "wb") as f:
        for a in (clouds["src"], clouds["tgt"]):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.ascontiguousarray(G.T.reshape(16), F).tobytes())
        f.write(thr.tobytes())
        f.write(np.asarray(p["vp_src"], F).tobytes()); f.write(np.asarray(p["vp_tgt"], F).tobytes())
    out = subprocess.run([exe, path, "150"] + [str(s) for s in SEEDS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(re.findall(r"(\w+)=(\w+)", out.stdout))
    prm = capi.default_params(matching_id=capi.MATCH_ONE_SIDED, bf_block_size=200000, distance_thr=float(thr), vp_src=p["vp_src"], vp_tgt=p["vp_tgt"],
                              max_iterations=150, fix_seed=0)
    m, runs = lgr.measure_host(clouds["src"], clouds["tgt"], prm, G, n_times=len(SEEDS), seeds=SEEDS)

    def bits(v):
        return "%08x" % int(np.asarray(v, F).view(np.uint32))
    assert 0 < m.n_success < len(SEEDS)   # not vacuous: some runs succeed, some fail
    assert (int(got["n_times"]), int(got["n_success"])) == (m.n_times, m.n_success), out.stdout
    for k in ("success_rate", "mae", "sae", "mte", "ste", "mrmse", "srmse"):   # (the two time columns belong to each call)
        assert got[k] == bits(getattr(m, k)), k
    for i, r in enumerate(runs):
        assert (int(got[f"run{i}_seed"]), int(got[f"run{i}_converged"]), int(got[f"run{i}_ok"]), int(got[f"run{i}_inliers"])) == (
            SEEDS[i], r.result.converged, r.eval.converged_and_overlap_ok, r.result.n_inliers)
        assert got[f"run{i}_r_err"] == bits(r.eval.r_err)
        assert got[f"run{i}_overlap_rmse"] == bits(r.eval.overlap_rmse) or (np.isnan(r.eval.overlap_rmse) and np.isnan(np.uint32(int(got[f"run{i}_overlap_rmse"], 16)).view(F)))
        assert got[f"run{i}_T"] == "".join(bits(v) for v in r.result.transformation)
