"""GPU timing of the iterated closest-plane refinement (lgr_refine_plane_dev) on the 1M-point bench pair at the perturbed ground truth
(0.5 degrees about z, 0.3 x threshold along (0.6, 0, 0.8)), MSE score, max_steps 10, threshold supplied -- beside the yardstick: the same
loop composed from lgr_evaluate_plane_dense_dev (inlier list kept on the device) + lgr_refit_svd_dev, driven from Python through ctypes.
With --yardstick-lib the yardstick runs on ANOTHER build of liblgr_hip.so (the parent commit's) loaded into the same process; without it,
on this build (whose two entry points keep the parent's device code).  One warm-up each, then five timed calls each, ALTERNATING, every
call ended by a device synchronise.  Per-step ms = call time / candidates evaluated; the call includes the set-up and T0's evaluation in
both.  

    python tools/bench_refine.py [--points 1000000] [--steps 10] [--yardstick-lib PATH] [--out profiles/refine_bench1m.json]
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--yardstick-lib", default=None)
    ap.add_argument("--only", choices=("refine", "yardstick"), default=None, help="run one side only (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench1m.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgr_amd import capi, synthetic
    assert torch.cuda.is_available(), "this is a GPU measurement: there is no CPU figure to fall back to"
    ctx = capi.Context(0)
    F = np.float32

    pair = synthetic.make_pair(a.points, seed=synthetic.SEED)   # the bench pair of rank 0
    src, tgt = torch.from_numpy(pair["src"]).cuda(), torch.from_numpy(pair["tgt"]).cuda()
    ctx.normals_knn(src, 30, vp=pair["vp_src"])
    ctx.normals_knn(tgt, 30, vp=pair["vp_tgt"])
    thr = float(F(ctx.cloud_density(tgt)))
    ang = np.deg2rad(0.5)
    dT = np.eye(4)
    dT[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    dT[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    T0 = (dT @ pair["T_gt"]).astype(F)
    ns, nt = src.shape[0], tgt.shape[0]

    # the yardstick's library and context
    ylib = C.CDLL(os.path.abspath(a.yardstick_lib)) if a.yardstick_lib else capi.lib()
    yh = C.c_void_p()
    assert ylib.lgr_ctx_create(0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream), C.byref(yh)) == 0
    d_inl = torch.empty((ns, 4), dtype=torch.int32, device="cuda")

    def yardstick():
        """the statement, driven from the host: -> (accepted steps, candidates evaluated, metric, transform words)"""
        T = (C.c_float * 16)(*T0.T.reshape(16).tolist())
        e, e2 = capi.PlaneDenseEval(), capi.PlaneDenseEval()
        ev = lambda t, o: ylib.lgr_evaluate_plane_dense_dev(yh, capi._ptr(src), ns, capi._ptr(tgt), nt, t, capi.SCORE_MSE, None, C.c_float(thr),  # noqa: E731
                                                            C.byref(o), capi._ptr(d_inl), None)
        assert ev(T, e) == 0
        steps = cands = 0
        while steps < a.steps and e.n_inliers >= 3:
            Tn = (C.c_float * 16)()
            assert ylib.lgr_refit_svd_dev(yh, capi._ptr(src), capi._ptr(tgt), capi._ptr(d_inl), e.n_inliers, None, Tn) == 0
            assert ev(Tn, e2) == 0
            cands += 1
            if not (e2.metric > e.metric):
                break
            T, steps = Tn, steps + 1
            e, e2 = e2, e
        return steps, cands, e.metric, np.array(T, F).view(np.uint32).tolist()

    def refine():
        r = ctx.refine_plane(src, tgt, T0, capi.SCORE_MSE, a.steps, threshold=thr, trace=True)
        return r.steps, len(r.trace) - 1, r.metric, np.array(r.transformation, F).view(np.uint32).tolist()

    def timed(f):
        t = time.perf_counter()
        r = f()
        ctx.sync(); torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    sides = [("refine", refine), ("yardstick", yardstick)]
    if a.only:
        sides = [s for s in sides if s[0] == a.only]
    res = {n: timed(f)[1] for n, f in sides}   # the warm-up
    ms = {n: [] for n, _ in sides}
    for _ in range(a.calls):
        for n, f in sides:
            t, r = timed(f)
            assert r == res[n]
            ms[n].append(t)
    if not a.only:
        assert res["refine"] == res["yardstick"], "the two loops disagree"
    out = dict(points=a.points, device=torch.cuda.get_device_name(0), max_steps=a.steps, threshold=thr, calls_per_figure=a.calls,
               yardstick_library="another build (--yardstick-lib)" if a.yardstick_lib else "this build",
               figure="per-step ms = call time / candidates evaluated; the calls of the two sides alternate")
    for n, _ in sides:
        steps, cands, metric, _T = res[n]
        per = sorted(t / max(cands, 1) for t in ms[n])
        out[n] = dict(steps=steps, candidates=cands, metric=metric, call_ms=[round(t, 3) for t in ms[n]],
                      per_step_ms=dict(median=round(per[len(per) // 2], 3), min=round(per[0], 3), max=round(per[-1], 3)))
    if not a.only:
        out["refine_over_yardstick"] = round(out["refine"]["per_step_ms"]["median"] / out["yardstick"]["per_step_ms"]["median"], 3)
    print(json.dumps(out))
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ylib.lgr_ctx_destroy(yh)
    ctx.close()


if __name__ == "__main__":
    main()
