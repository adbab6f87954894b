"""The header-only C++ shim's debug layer: getColor / setPointColor / mixPointColor, calculateTemperatureMap, saveTemperatureMaps,
compareOverlaps, savePointCloudWithCorrespondences, saveColorizedWeights and saveColorizedPointCloud under the reference's names.  On the
CPU: the caller tests/cpp/shim_debug_smoke.cpp compiles and links.  On the GPU: every file it writes equals, byte for byte, the file the
Python host writes from the C ABI's results for the same pair, and the printed numbers equal lgr_compare_overlaps'."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_ref_lib as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
F = np.float32


def build(tmp_path):
    exe = os.path.join(str(tmp_path), "shim_debug_smoke")
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "shim_debug_smoke.cpp"), "-o", exe,
                           "-L", CSRC, "-llgr_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_shim_debug_builds(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "built" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_debug_files_equal_python_host(tmp_path, lgr):
    import torch
    from lgr_amd import formats, synthetic
    exe = build(tmp_path)
    p = synthetic.make_pair(n_points=2000, seed=12)
    clouds = {}
    for side in ("src", "tgt"):
        d = torch.from_numpy(np.ascontiguousarray(p[side], F)).cuda()
        lgr.normals_knn(d, 30, vp=p["vp_" + side])
        clouds[side] = d.cpu().numpy()
    src, tgt = clouds["src"], clouds["tgt"]
    thr = float(F(2 * lgr.cloud_density(torch.from_numpy(tgt).cuda())))
    G = p["T_gt"].astype(F)
    T = G.copy()
    T[:3, 3] += F(0.3 * thr) * np.array([0.6, 0.0, 0.8], F)
    rng = np.random.default_rng(2)
    ns, nt = len(src), len(tgt)
    corr = np.zeros(300, D.CORR_DTYPE)
    corr["index_query"] = rng.integers(0, ns, 300); corr["index_match"] = rng.integers(0, nt, 300)
    correct, inl = corr[rng.random(300) < 0.3], corr[rng.random(300) < 0.4]
    kp = np.unique(rng.integers(0, ns, 200)).astype(np.int32)
    w = rng.random(ns).astype(F)
    path, outdir = os.path.join(str(tmp_path), "pair.bin"), os.path.join(str(tmp_path), "out")
    os.makedirs(outdir)
    with open(path, "wb") as f:
        for a in (src, tgt):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a, F).tobytes())
        for a in (kp, corr, correct, inl, w):
            f.write(np.int32(a.shape[0]).tobytes()); f.write(np.ascontiguousarray(a).tobytes())
        f.write(D.T16(T).tobytes()); f.write(D.T16(G).tobytes()); f.write(F(thr).tobytes())
    out = subprocess.run([exe, path, outdir], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr

    def same(name, write):
        mine = os.path.join(str(tmp_path), "py_" + name)
        write(mine)
        assert open(os.path.join(outdir, name), "rb").read() == open(mine, "rb").read(), name
    for stem, Tk in (("temperature_gt", G), ("temperature", T)):
        m = lgr.temperature_maps_host(src, tgt, Tk, thr)
        for side, cloud in (("src", m["moved"]), ("tgt", tgt)):
            s = m[side]
            same(f"{stem}_distances_{side}.csv", lambda q, s=s: formats.save_vector(q, s["temp_distance"][s["temp_distance"] < F(thr)]))
            same(f"{stem}_dists_{side}.ply", lambda q, s=s, c=cloud: formats.write_ply_colored(q, c, s["color_distance"], binary=False))
            same(f"{stem}_normal_diffs_{side}.ply", lambda q, s=s, c=cloud: formats.write_ply_colored(q, c, s["color_normal"], binary=True))
            assert len(open(os.path.join(outdir, f"{stem}_distances_{side}.csv")).read().splitlines()) == 1 + s["n_below"] and s["n_below"] > 0
    m = lgr.temperature_maps_host(src, tgt, T, thr)
    same("map_dists_src.ply", lambda q: formats.write_ply_colored(q, m["moved"], m["src"]["color_distance"], binary=False))
    same("map_normal_diffs_src.ply", lambda q: formats.write_ply_colored(q, m["moved"], m["src"]["color_normal"], binary=True))
    assert f"below_distance={m['src']['n_below']} below_normal={m['src']['n_below']}" in out.stdout
    o = lgr.compare_overlaps_host(src, tgt, [T, G], thr, with_masks=False)
    vals = dict(re.findall(r"(\w+)=(\w+)", out.stdout))
    assert (int(vals["count0"]), int(vals["count1"])) == tuple(o["counts"]) and o["counts"][1] > 0
    assert [int(vals["weighted0"], 16), int(vals["weighted1"], 16)] == list(o["weighted"].view(np.uint32))
    assert f"\tincorrect hypothesis: {o['counts'][0]} points, {formats._g(o['weighted'][0])}weighted points" in out.stderr
    assert f"\t  correct hypothesis: {o['counts'][1]} points, {formats._g(o['weighted'][1])}weighted points" in out.stderr
    same("downsampled_src.ply", lambda q: formats.write_ply_colored(q, D.move(src, G), lgr.color_correspondences_host(ns, kp, corr, correct, inl, True)))
    same("downsampled_tgt.ply", lambda q: formats.write_ply_colored(q, D.move(tgt, np.eye(4, dtype=F)),
                                                                     lgr.color_correspondences_host(nt, None, corr, correct, inl, False)))
    same("weights.ply", lambda q: formats.write_ply_colored(q, D.move(src, T), lgr.color_map_host(w)[0]))
    same("red_src.ply", lambda q: formats.write_ply_colored(q, D.move(src, G), np.full(ns, D.COLOR_RED, np.int32)))
