"""GPU timing of matchLocal with a k-list (lgr_match_local_knn_dev) on the 1M-point bench pair: every point a key point, the ground truth
as the guess, match_search_radius = the alignment's distance_thr (0.1), descriptors computed on the device as the pipeline does
(surface = voxel downsample + 30-NN normals, radius 0.25; RoPS on gravity frames).

  (a) lgr_match_local_knn_dev(33, k = 1) beside lgr_match_local_dev.  With --parent-lib the latter runs on ANOTHER build of liblgr_hip.so
      (the parent commit's) loaded into the same process, on a context of its own; without it, on this build (whose lgr_match_local_dev
      is then the same code).  The two results must be equal bit for bit.  The old entry point may move to the new kernel only if the
      new median lies within the parent's own spread (min..max of its calls) or below it.  The same comparison is made for the entry
      point's other path, the scan of every train point under a FLT_MAX radius, on the first --scan-points points of each cloud.
  (b) the cost of rows 135 and 352 (and 33) at k = 1 and k = 8, and for scale the dense lgr_match_knn_dev on the same rows: its first
      --dense-queries queries against all train rows (an exact scan is linear in the queries; the figure for all of them is that time
      times mq / dense-queries and is marked as extrapolated).

One warm-up, then --calls timed calls per side, the sides of (a) ALTERNATING, every call ended by a device synchronise; a call includes
the guess upload and the grid build.  

    python tools/bench_match_local.py [--points 1000000] [--parent-lib PATH] [--out profiles/match_local_knn.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.1, help="match_search_radius: bench.py's distance_thr")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dense-queries", type=int, default=16384)
    ap.add_argument("--scan-points", type=int, default=32768, help="size of the FLT_MAX comparison of (a)")
    ap.add_argument("--rows", default="33,135,352")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_local_knn.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgr_amd import capi, synthetic
    assert torch.cuda.is_available(), "this is a GPU measurement: there is no CPU figure to fall back to"
    ctx = capi.Context(0)
    lib = capi.lib()
    p = capi._ptr

    def say(*x):
        print(*x, flush=True)

    def timed(f):
        t = time.perf_counter()
        r = f()
        ctx.sync(); torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def stats(ms):
        s = sorted(ms)
        return dict(call_ms=[round(t, 3) for t in ms], median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))

    pair = synthetic.make_pair(a.points, seed=synthetic.SEED)   # the bench pair of rank 0
    src, tgt = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    feature_radius = 0.25
    voxel = float(np.sqrt(np.float32(np.pi * feature_radius * feature_radius / 352.0)))
    dims = [int(d) for d in a.rows.split(",")]
    rows = {d: [] for d in dims}
    for side, cloud in (("src", src), ("tgt", tgt)):
        vp = pair["vp_" + side]
        surf = ctx.downsample(cloud, voxel).clone()
        ctx.normals_knn(surf, 30, vp=vp)
        kn = cloud.clone()
        v = (C.c_float * 3)(*[float(x) for x in vp])
        ctx.check(lib.lgr_normals_knn_dev(ctx.h, p(kn), kn.shape[0], p(surf), surf.shape[0], 30, v, 1))
        for d in dims:
            t, f = timed(lambda: ctx.fpfh(kn, surf, feature_radius) if d == 33 else ctx.shot(kn, surf, feature_radius) if d == 352 else
                         ctx.rops(kn, surf, feature_radius, ctx.gravity_lrf(kn, surf, feature_radius)))
            rows[d].append(f)
            say(f"# {side}: {d}-float rows of {kn.shape[0]} key points on {surf.shape[0]} surface points in {t:.0f} ms")
    mq, mt = src.shape[0], tgt.shape[0]
    G = (C.c_float * 16)(*pair["T_gt"].astype(np.float32).T.reshape(16).tolist())
    radius = C.c_float(a.radius)

    def local_knn(d, k, n=None, r=radius):
        """all queries against all train points, or the first n of each"""
        nq, nt = (mq, mt) if n is None else (min(n, mq), min(n, mt))
        idx = torch.empty((nq, k), dtype=torch.int32, device="cuda"); dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        ctx.check(lib.lgr_match_local_knn_dev(ctx.h, d, p(src), nq, p(tgt), nt, p(rows[d][0]), p(rows[d][1]), G, r, k, p(idx), p(dist)))
        return idx, dist

    out = dict(points=a.points, device=torch.cuda.get_device_name(0), match_search_radius=a.radius, feature_radius=feature_radius,
               calls_per_figure=a.calls, figure="ms per call, host clock around a call ended by a device synchronise; guess upload and grid build included")

    if 33 in dims:   # ---- (a)
        ylib = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else lib
        yh = C.c_void_p()
        assert ylib.lgr_ctx_create(0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream), C.byref(yh)) == 0

        def old(n=None, r=radius):
            nq, nt = (mq, mt) if n is None else (min(n, mq), min(n, mt))
            idx = torch.empty((nq,), dtype=torch.int32, device="cuda"); dist = torch.empty((nq,), dtype=torch.float32, device="cuda")
            assert ylib.lgr_match_local_dev(yh, p(src), nq, p(tgt), nt, p(rows[33][0]), p(rows[33][1]), G, r, p(idx), p(dist)) == 0
            return idx, dist

        def compare(new_f, old_f):
            sides = [("local_knn_33_k1", new_f), ("match_local_parent", old_f)]
            res = {n: timed(f)[1] for n, f in sides}   # the warm-up
            ms = {n: [] for n, _ in sides}
            for _ in range(a.calls):
                for n, f in sides:
                    ms[n].append(timed(f)[0])
            new_i, new_d = res["local_knn_33_k1"]
            old_i, old_d = res["match_local_parent"]
            equal = bool(torch.equal(new_i[:, 0], old_i) and torch.equal(new_d[:, 0].view(torch.int32), old_d.view(torch.int32)))
            sn, so = stats(ms["local_knn_33_k1"]), stats(ms["match_local_parent"])
            return dict(local_knn_33_k1=sn, match_local_parent=so, parent_library="another build (--parent-lib)" if a.parent_lib else "this build",
                        queries=int(old_i.shape[0]), results_bit_equal=equal, matched_fraction=float((old_i >= 0).float().mean()),
                        new_over_parent=round(sn["median"] / so["median"], 3), reroute_allowed=bool(equal and sn["median"] <= so["max"]),
                        rule="re-route lgr_match_local* only if the new median is within the parent's min..max or below it")

        out["a"] = compare(lambda: local_knn(33, 1), old)
        say("# (a)", json.dumps(out["a"]))
        # the other path of the same entry point: a radius whose square is not finite scans every train point (the reference test's
        # FLT_MAX); an exact scan is quadratic, so on the first --scan-points points of each cloud
        big = C.c_float(3.4028234663852886e38)
        out["a_scan"] = compare(lambda: local_knn(33, 1, a.scan_points, big), lambda: old(a.scan_points, big))
        say("# (a) FLT_MAX", json.dumps(out["a_scan"]))
        ylib.lgr_ctx_destroy(yh)

    out["b"] = {}   # ---- (b)
    for d in dims:
        for k in (1, 8):
            timed(lambda: local_knn(d, k))
            ms = [timed(lambda: local_knn(d, k))[0] for _ in range(a.calls)]
            out["b"][f"local_knn_{d}_k{k}"] = stats(ms)
            say(f"# (b) local_knn {d} k={k}", json.dumps(out["b"][f"local_knn_{d}_k{k}"]))
        nq = min(a.dense_queries, mq)
        q = rows[d][0][:nq].contiguous()
        for k in (1, 8):
            timed(lambda: ctx.match_knn(q, rows[d][1], 200000, k))
            ms = [timed(lambda: ctx.match_knn(q, rows[d][1], 200000, k))[0] for _ in range(a.calls)]
            s = stats(ms)
            s.update(queries=nq, train_rows=mt, all_queries_ms_extrapolated=round(s["median"] * mq / nq, 1))
            out["b"][f"dense_knn_{d}_k{k}"] = s
            say(f"# (b) dense knn {d} k={k}", json.dumps(s))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
