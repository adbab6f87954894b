"""The header-only C++ shim's metric estimators: MetricEstimator and its five subclasses in their dense form,
getMetricEstimatorFromParameters, AlignmentAnalysis::getMetricEstimator() and the figures start() fills, under the reference's names and
signatures (include/metric.h, include/analysis.h).  On the CPU: the caller tests/cpp/shim_metric_smoke.cpp compiles, links and finds the
sparse form refused by name.  On the GPU: every figure it prints for closest_plane, weighted_closest_plane and combination equals the C
ABI's on the same pair bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_metric_smoke")
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_metric_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_metric_builds(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_metric_equals_c_abi(tmp_path, lgr):
    import torch
    from lgr_amd import capi, synthetic
    exe = build(tmp_path)
    p = synthetic.make_pair(n_points=4000, seed=12)
    clouds = {}
    for side in ("src", "tgt"):
        d = torch.from_numpy(np.ascontiguousarray(p[side], F)).cuda()
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        clouds[side] = d
    thr = float(F(2 * lgr.cloud_density(clouds["tgt"])))
    params = capi.default_params(matching_id=capi.MATCH_ONE_SIDED, bf_block_size=200000, distance_thr=thr, vp_src=p["vp_src"], vp_tgt=p["vp_tgt"])
    corr = lgr.correspondences(clouds["src"], clouds["tgt"], params).cpu().numpy().view(capi.CORR_DTYPE).reshape(-1)
    src, tgt = clouds["src"].cpu().numpy(), clouds["tgt"].cpu().numpy()
    G = p["T_gt"].astype(F)
    T = G.copy()
    T[:3, 3] += F(0.15 * thr) * np.array([0.6, 0.0, 0.8], F)
    path = os.path.join(str(tmp_path), "pair.bin")
    with open(path, "wb") as f:
        for a in (src, tgt):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.int32(corr.shape[0]).tobytes()); f.write(np.ascontiguousarray(corr).tobytes())
        f.write(np.ascontiguousarray(T.T.reshape(16), F).tobytes()); f.write(np.ascontiguousarray(G.T.reshape(16), F).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(re.findall(r"(\w+)=(\w+)", out.stdout))

    def bits(v):
        return "%08x" % int(np.asarray(v, F).view(np.uint32))
    ids = {"closest_plane": capi.METRIC_CLOSEST_PLANE, "weighted_closest_plane": capi.METRIC_WEIGHTED_CLOSEST_PLANE, "combination": capi.METRIC_COMBINATION}
    for name, mid in ids.items():
        kw = dict(weight="curvature") if name == "weighted_closest_plane" else {}
        m = lgr.analysis_metric_host(src, tgt, corr, T, G, metric_id=mid, score_id=capi.SCORE_MSE, **kw)
        assert m.n_inliers > 0 and m.n_correct_inliers > 0 and m.metric > 0   # not vacuous
        for pre in ("", "a_", "g_"):   # the estimator alone, the analysis' figures, the analysis' estimator asked again
            assert got[f"{name}_{pre}metric"] == bits(m.metric) and got[f"{name}_{pre}rmse"] == bits(m.rmse), (name, pre)
            assert int(got[f"{name}_{pre}inliers"]) == m.n_inliers, (name, pre)
        assert int(got[f"{name}_correct"]) == int(got[f"{name}_a_correct"]) == m.n_correct_inliers
        assert got[f"{name}_class"] == {"closest_plane": "ClosestPlaneMetricEstimator", "weighted_closest_plane": "WeightedClosestPlaneMetricEstimator",
                                        "combination": "CombinationMetricEstimator"}[name]
        if name != "combination":   # the inlier list is the dense evaluation's
            d = lgr.evaluate_plane_dense_host(src, tgt, T, capi.SCORE_MSE, with_inliers=True, **kw)
            assert got[f"{name}_metric"] == bits(d.metric) and int(got[f"{name}_inliers"]) == d.n_inliers
            h = 0
            for q, t in zip(d.inliers["index_query"].tolist(), d.inliers["index_match"].tolist()):
                h = (h * 31 + q * 7 + t) & 0xFFFFFFFF
            assert int(got[f"{name}_hash"]) == h
