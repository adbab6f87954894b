"""What the reference point order costs: the bench generator's cloud (lgr_amd.synthetic.make_pair, source side) plus 10 % exact duplicates
through the loader entries in LGR_ORDER_REFERENCE.

    python tools/bench_hash_order.py [--points N] [--repeats R] [--parent-lib PATH/liblgr_hip.so] [--out FILE.json]

Host entries (lgr_preprocess, lgr_downsample with LGR_ORDER_REFERENCE): one child process per sample -- a library is loaded once per
process -- each of which warms the entry up and times one call; with --parent-lib the children alternate between that build (the parent
commit's, where the order is a replay through std::unordered_set / unordered_map on one host thread) and this tree's, --repeats samples
each, and the medians are reported side by side.  Device entries of this tree (lgr_downsample_order_dev, lgr_dedupe_order_dev,
lgr_preprocess_order_dev) in both orders and lgr_hash_order_dev alone: one process, a warm-up, then the median of --repeats calls, each
timed to the end of the stream.  The voxel of the down-sampling rows is the bench pipeline's (feature radius 0.25, 352 points)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))
VOXEL = math.sqrt(math.pi * 0.25 * 0.25 / 352.0)


def make_cloud(points):
    import numpy as np
    from lgr_amd import synthetic
    pair = synthetic.make_pair(points, seed=synthetic.SEED)
    pts = pair["src"]
    rng = np.random.default_rng(1)
    dup = pts[rng.integers(0, len(pts), points // 10)].copy()
    at = np.sort(rng.integers(0, len(pts), len(dup)))
    return np.ascontiguousarray(np.insert(pts, at, dup, axis=0)), pair["vp_src"]


def child_host(path):
    """one sample of the two host entries in LGR_ORDER_REFERENCE on the library LGR_HIP_LIB names"""
    import numpy as np
    from lgr_amd import capi
    d = np.load(path)
    pts, vp = d["pts"], d["vp"]
    ctx = capi.Context(0)
    out = {}
    for name, fn in (("lgr_preprocess", lambda: ctx.preprocess_host(pts, vp=vp, order=capi.ORDER_REFERENCE)[0]),
                     ("lgr_downsample", lambda: ctx.downsample_host(pts, VOXEL, order=capi.ORDER_REFERENCE))):
        fn()
        t = time.perf_counter()
        r = fn()
        out[name] = dict(ms=1e3 * (time.perf_counter() - t), n_out=int(len(r)))
    ctx.close()
    print("SAMPLE " + json.dumps(out), flush=True)


def device_rows(pts, vp, repeats):
    import torch
    from lgr_amd import capi
    ctx = capi.Context(0)
    d = torch.from_numpy(pts).cuda()

    def timed(fn):
        fn(); ctx.sync()
        ms = []
        for _ in range(repeats):
            t = time.perf_counter()
            r = fn()
            ctx.sync()
            ms.append(1e3 * (time.perf_counter() - t))
        return dict(ms=statistics.median(ms), ms_min_max=[min(ms), max(ms)], n_out=int(r[0].shape[0] if isinstance(r, tuple) else r.shape[0]))

    rows = {}
    for label, order in (("canonical", capi.ORDER_CANONICAL), ("reference", capi.ORDER_REFERENCE)):
        rows["lgr_downsample_order_dev " + label] = timed(lambda: ctx.downsample(d, VOXEL, order=order))
        rows["lgr_dedupe_order_dev " + label] = timed(lambda: ctx.dedupe(d, order=order))
        rows["lgr_preprocess_order_dev " + label] = timed(lambda: ctx.preprocess(d, vp=vp, order=order))
    for n in (rows["lgr_downsample_order_dev reference"]["n_out"], rows["lgr_dedupe_order_dev reference"]["n_out"]):
        h = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device="cuda")
        rows[f"lgr_hash_order_dev n={n}"] = timed(lambda: ctx.hash_order(h))
        rows[f"lgr_hash_order_dev n={n} reserve=n"] = timed(lambda: ctx.hash_order(h, reserve=n))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="liblgr_hip.so of the parent commit: its host entries are timed in alternation with this tree's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-host", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_host:
        return child_host(a.child_host)
    import numpy as np
    pts, vp = make_cloud(a.points)
    out = dict(points=int(len(pts)), duplicates=a.points // 10, voxel=VOXEL, repeats=a.repeats, host_entries_reference_order={})
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.npz")
        np.savez(path, pts=pts, vp=np.asarray(vp, np.float32))
        builds = ([("parent", a.parent_lib)] if a.parent_lib else []) + [("this", None)]
        samples = {b: [] for b, _ in builds}
        for _ in range(a.repeats):
            for b, lib in builds:   # alternating
                env = dict(os.environ)
                env.pop("LGR_HIP_LIB", None)
                if lib:
                    env["LGR_HIP_LIB"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-host", path], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f"{b} child failed ({r.returncode}): {r.stderr[-2000:]}")
                samples[b].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SAMPLE ")][0][7:]))
        for b, _ in builds:
            out["host_entries_reference_order"][b] = {
                k: dict(ms=statistics.median(s[k]["ms"] for s in samples[b]), ms_all=[s[k]["ms"] for s in samples[b]], n_out=samples[b][0][k]["n_out"])
                for k in samples[b][0]}
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    out["device_entries"] = device_rows(pts, vp, a.repeats)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
