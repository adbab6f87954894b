"""The header-only C++ shim's icpRegistration (its two overloads).  On the CPU: the caller tests/cpp/shim_icp_ex_smoke.cpp compiles, links
and sees the ABI's defaults and struct size.  On the GPU: with every field of lgr_icp_ex_params set away from its default -- variant,
robust kernel, scale, gate cosine, plane_eps, weights, two base fields -- every figure it prints equals the C ABI's lgr_icp_ex_host on
the same pair bit for bit, and differs from the call that leaves any one option out (so a field the shim dropped would show)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref_lib as I  # noqa: E402
import refine_ref_lib as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_icp_ex_smoke")
    assert os.path.exists(os.path.join(CSRC, "liblgr_hip.so")), "build the library first (__graft_entry__.build())"
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "shim_icp_ex_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_icp_ex_builds(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_icp_ex_equals_c_abi(tmp_path, lgr, oracle):
    exe = build(tmp_path)
    p = R.make_pair(oracle)
    src, tgt, T0 = p["src"], p["tgt"], I.perturb(p["T_gt"], 0.5, 0.04)
    w = np.random.default_rng(7).uniform(0.25, 1.0, len(src)).astype(F)
    m, max_dist = 4, float(F(2 * p["thr"]))
    opt = dict(variant=2, robust=1, robust_scale=0.15, min_normal_cos=0.97, plane_eps=0.01)
    path = os.path.join(str(tmp_path), "pair.bin")
    with open(path, "wb") as f:
        for a in (src, tgt):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        f.write(np.ascontiguousarray(T0.T.reshape(16), F).tobytes())
        f.write(w.tobytes())
    out = subprocess.run([exe, path, repr(max_dist), str(m)] + [repr(opt[k]) for k in ("variant", "robust", "robust_scale", "min_normal_cos", "plane_eps")] + ["1"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(re.findall(r"(\w+)=(\w+)", out.stdout))

    def bits(v):
        return "%08x" % int(np.asarray(v, F).view(np.uint32))
    r = lgr.icp_ex_host(src, tgt, T0, weights=w, max_dist=max_dist, max_iterations=m, **opt)
    assert r.iterations == m and r.pairs0 > 1000   # not vacuous
    assert (int(got["iterations"]), int(got["stop"]), int(got["pairs"]), int(got["pairs0"])) == (r.iterations, r.stop, r.pairs, r.pairs0)
    for k, v in (("rmse", r.rmse), ("rmse0", r.rmse0), ("max_dist", r.max_dist)):
        assert got[k] == bits(v), k
    assert got["T"] == "".join(bits(v) for v in r.transformation)
    # every option matters to these bits
    for drop in (dict(variant=0), dict(robust=0), dict(robust_scale=0.3), dict(min_normal_cos=-1.0), dict(plane_eps=0.0), dict(weights=None), dict(max_dist=2 * max_dist),
                 dict(max_iterations=m - 1)):
        o = lgr.icp_ex_host(src, tgt, T0, **dict(dict(opt, weights=w, max_dist=max_dist, max_iterations=m), **drop))
        assert "".join(bits(v) for v in o.transformation) != got["T"], drop
