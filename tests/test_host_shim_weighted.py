"""The header-only C++ shim with metric_id "weighted_closest_plane".  On the CPU: the shim maps the name to
LGR_METRIC_WEIGHTED_CLOSEST_PLANE (it used to map it to the correspondences metric without a word) and an unknown weight_id to constant,
as getWeightFunction does.  On the GPU: alignRansac through the shim with weight_id "nss" gives bit for bit the C ABI's
lgr_ransac_ex_dev result with LGR_WEIGHT_NSS."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_weighted_smoke")
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_weighted_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_maps_weighted_closest_plane(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "metric_abi=4" in out.stdout and "unknown_weight_abi=0" in out.stdout, out.stdout


@pytest.mark.gpu
def test_shim_weighted_nss_equals_c_abi(tmp_path, lgr):
    import torch
    from lgr_amd import capi, synthetic
    exe = build(tmp_path)
    p = synthetic.make_pair(40000, seed=51)
    clouds = {}
    for side in ("src", "tgt"):
        d = torch.from_numpy(np.ascontiguousarray(p[side], np.float32)).cuda()
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        clouds[side] = d
    kw = dict(matching_id=0, bf_block_size=10000, max_iterations=30000, distance_thr=0.1, score_id=2, n_samples=3, edge_thr_coef=0.95,
              confidence=0.999)
    corr = lgr.correspondences(clouds["src"], clouds["tgt"], capi.default_params(metric_id=4, **kw))
    path = os.path.join(str(tmp_path), "pair.bin")
    with open(path, "wb") as f:
        for side in ("src", "tgt"):
            a = clouds[side].cpu().numpy()
            f.write(np.int32(a.shape[0]).tobytes()); f.write(a.tobytes())
        c = corr.cpu().numpy()
        f.write(np.int32(c.shape[0]).tobytes()); f.write(np.ascontiguousarray(c).tobytes())
    res, _ = lgr.ransac_ex(clouds["src"], clouds["tgt"], corr, capi.default_params(metric_id=4, **kw), capi.metric_params("nss"))
    out = subprocess.run([exe, path, "nss"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"converged=(\d) iterations=(\d+) T=(\S+)", out.stdout)
    assert m, out.stdout
    T = np.array([int(x, 16) for x in m.group(3).split(",")], np.uint32)
    assert int(m.group(1)) == res.converged == 1 and int(m.group(2)) == res.iterations
    assert np.array_equal(T, np.array(list(res.transformation), np.float32).view(np.uint32))
    # and it is not the correspondences metric the shim used to substitute
    r0, _ = lgr.ransac(clouds["src"], clouds["tgt"], corr, capi.default_params(metric_id=0, **kw))
    assert not np.array_equal(T, np.array(list(r0.transformation), np.float32).view(np.uint32))
