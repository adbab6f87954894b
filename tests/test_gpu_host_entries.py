"""Host entry point == its _dev twin, byte for byte.

Every function of include/lgr.h that takes host arrays uploads them, calls a `_dev` twin, downloads and synchronises.  Each row of ROWS
below calls one host form with numpy arrays and its twin with torch tensors of the same bytes on the same context, and asserts equal
return codes and byte-identical outputs -- arrays, counts, scalars and result structs alike.  Only the wall-clock fields of lgr_result
(time_cs, time_te, stage_ms) and the two columns of lgr_measurement that are computed from them (mtime, stime) are left out.

Cases per row: `full`; `absent` (every optional input and output NULL); `zero:<count>` and `one:<count>` for every array count of the
signature; `null` (the first array NULL under a positive count: the host form's own return code, recorded in NULL_RC).  An empty array is
handed over as a valid pointer with count 0 on both sides.  Outputs are compared when the call succeeds; a refused call compares the code.  Output buffers start from one byte pattern on both sides, so entries neither
side writes compare equal; where a host form copies back only the first *n_out entries the comparison stops there.

test_table_is_complete parses include/lgr.h: every lgr_X with an lgr_X_dev / lgr_X_order_dev declared is a row or is listed in
NO_STAGING (the host form stages no array).  lgr_selfcheck_rcp and lgr_selfcheck_libm stage arrays but have no twin: their rows compare
with the documented contract and with the oracle's restatement of the same routines.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT = {"p": C.c_void_p, "i": C.c_int, "f": C.c_float, "q": C.c_longlong, "u": C.c_uint, "Q": C.c_uint64}
PATTERN = 0xCD          # what every output buffer holds before the call, on both sides
K = 3                   # list length of the k-nearest matchers
MQ, MT = 70, 90         # descriptor table rows: neither a multiple of 64
N_CLOUD = 1500
N_CORR = 50

_state = {}


def lib():
    """a CDLL handle of this file's own: the argtypes set here do not reach lgr_amd.capi's calls"""
    if "lib" not in _state:
        from lgr_amd import capi
        _state["lib"] = C.CDLL(capi.LIB_PATH)
    return _state["lib"]


class Data:
    """the inputs every row draws from, built once"""

    def __init__(self, ctx):
        from lgr_amd import capi, synthetic
        rng = np.random.default_rng(7)
        pair = synthetic.make_pair(N_CLOUD, seed=5)
        self.pair = pair
        self.src, self.tgt = pair["src"].copy(), pair["tgt"].copy()
        for pts, vp in ((self.src, pair["vp_src"]), (self.tgt, pair["vp_tgt"])):   # k = 30 normals, in place
            fn = lib().lgr_normals_knn
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
            vp = np.ascontiguousarray(vp, np.float32)
            assert fn(ctx.h, pts.ctypes.data, len(pts), None, 0, 30, vp.ctypes.data, 0) == 0
        T = pair["T_gt"].astype(np.float32)
        self.Tgt = np.ascontiguousarray(T.T.reshape(16))   # column-major
        Tn = T.copy()
        Tn[:3, 3] += np.float32(0.004)
        self.T = np.ascontiguousarray(Tn.T.reshape(16))
        self.tns = np.ascontiguousarray(np.stack([self.Tgt, np.eye(4, dtype=np.float32).reshape(16), self.T]))
        # correspondences: source points with their nearest target under the ground truth, every fifth one scrambled
        moved = self.src[:, :3] @ T[:3, :3].T + T[:3, 3]
        iq = rng.choice(N_CLOUD, N_CORR, replace=False).astype(np.int32)
        d2 = ((moved[iq, None, :] - self.tgt[None, :, :3]) ** 2).sum(-1)
        im = d2.argmin(1).astype(np.int32)
        im[::5] = rng.integers(0, N_CLOUD, len(im[::5]))
        self.corr = np.zeros(N_CORR, capi.CORR_DTYPE)
        self.corr["index_query"], self.corr["index_match"] = iq, im
        self.corr["distance"] = rng.random(N_CORR).astype(np.float32)
        self.corr["threshold"] = np.float32(0.03)
        self.rows = {L: (rng.random((MQ, L)).astype(np.float32), rng.random((MT, L)).astype(np.float32)) for L in (33, 135, 352)}
        self.cand_idx = rng.integers(-1, MT, (MQ, K)).astype(np.int32)
        self.cand_dist = np.sort(rng.random((MQ, K)).astype(np.float32), axis=1)
        self.mask = (rng.random(N_CORR) < 0.5).astype(np.uint8)
        self.weights = (0.5 + rng.random(N_CLOUD)).astype(np.float32)
        self.values = rng.normal(size=N_CLOUD).astype(np.float32)
        self.poses, self.pose_metrics = (np.ascontiguousarray(a, np.float32) for a in synthetic.make_pose_list(n=60, k=4, seed=1))
        self.lrf = None   # filled by the first row that needs frames
        self.kw = dict(matching_id=0, bf_block_size=200000, max_iterations=2000, distance_thr=0.03, feature_radius=0.08,
                       vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])


def data(ctx):
    if "data" not in _state:
        _state["data"] = Data(ctx)
    return _state["data"]


class Case:
    def __init__(self, kind, which=None):
        self.kind, self.which = kind, which

    def n(self, name, full):
        """the count called `name`: 0 / 1 in that count's zero / one case, else `full`"""
        if self.which == name:
            return 0 if self.kind == "zero" else 1
        return full

    @property
    def absent(self):
        return self.kind == "absent"

    def __str__(self):
        return self.kind if self.which is None else f"{self.kind}:{self.which}"


class Side:
    """one side of a comparison: dev = False hands out host (numpy) pointers, dev = True device (torch) pointers"""

    def __init__(self, ctx, dev, case):
        import torch
        self.torch, self.ctx, self.dev, self.case = torch, ctx, dev, case
        self.null_pending = case.kind == "null"
        self.alive, self.outs, self.houts, self.kept = [], {}, {}, {}
        self.rc = None

    def _bytes_to_ptr(self, raw):
        buf = np.frombuffer(raw + bytes(max(0, 16 - len(raw))), np.uint8).copy()   # never empty: an empty array keeps a valid pointer
        if self.dev:
            buf = self.torch.from_numpy(buf).cuda()
            self.alive.append(buf)
            return buf, buf.data_ptr()
        self.alive.append(buf)
        return buf, buf.ctypes.data

    def arr(self, a):
        """an input array (None: NULL)"""
        if self.null_pending:
            self.null_pending = False
            return None
        if a is None:
            return None
        return self._bytes_to_ptr(np.ascontiguousarray(a).tobytes())[1]

    def out(self, name, shape, dtype, present=True, init=None):
        """an output array of the side's kind, compared after the call (init: the bytes of an in / out array)"""
        if not present:
            return None
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = bytes([PATTERN]) * nbytes if init is None else np.ascontiguousarray(init).tobytes()
        buf, ptr = self._bytes_to_ptr(raw)
        self.outs[name] = (buf, nbytes)
        return ptr

    def inout(self, name, a):
        if self.null_pending:
            self.null_pending = False
            return None
        return self.out(name, a.shape, a.dtype, init=a)

    def host(self, a):
        """an argument that lives in host memory for both forms (transforms, view points, seeds)"""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        self.alive.append(a)
        return a.ctypes.data

    def hout(self, name, obj, present=True, skip=()):
        """a host output of both forms: a ctypes object; skip = (offset, size) byte ranges left out of the comparison"""
        if not present:
            return None
        self.houts[name] = (obj, skip)
        return C.addressof(obj)

    def keep(self, name, count, itemsize):
        """compare only the first `count` entries of output `name` (the host form copies back no more)"""
        self.kept[name] = max(0, int(count)) * itemsize

    def call(self, name, sig, *args, twin=None):
        fn = getattr(lib(), (twin or name + "_dev") if self.dev else name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [CT[c] for c in sig]
        assert len(sig) == len(args), (name, len(sig), len(args))
        self.rc = fn(self.ctx.h, *args)
        return self.rc

    def results(self):
        self.ctx.sync()
        res = {}
        for name, (buf, nbytes) in self.outs.items():
            raw = (buf.cpu().numpy() if self.dev else buf).tobytes()[:nbytes]
            res[name] = raw[:self.kept.get(name, nbytes)]
        for name, (obj, skip) in self.houts.items():
            raw = bytearray(C.string_at(C.addressof(obj), C.sizeof(obj)))
            for off, size in skip:
                raw[off:off + size] = bytes(size)
            res[name] = bytes(raw)
        return res


def _field_ranges(struct, names, base=0):
    return [(base + getattr(struct, n).offset, getattr(struct, n).size) for n in names]


def result_skip(base=0):
    from lgr_amd import capi
    return _field_ranges(capi.Result, ("time_cs", "time_te", "stage_ms"), base)


def metric_params(s, d, ns, weighted):
    """lgr_metric_params with ns caller weights of the side's kind (None: the absent case / no weights)"""
    from lgr_amd import capi
    if not weighted:
        return None
    mp = capi.metric_params("constant")
    mp.weights = s.arr(d.weights[:ns])
    s.alive.append(mp)
    return C.addressof(mp)


def params(s, d, **kw):
    from lgr_amd import capi
    p = capi.default_params(**dict(d.kw, **kw))
    s.alive.append(p)
    return C.addressof(p)


def clouds(s, d):
    c = s.case
    ns, nt = c.n("ns", N_CLOUD), c.n("nt", N_CLOUD)
    return s.arr(d.src[:ns]), ns, s.arr(d.tgt[:nt]), nt


def problem(s, d):
    """clouds and correspondences; the correspondences stay in range when a cloud shrinks"""
    ps, ns, pt, nt = clouds(s, d)
    cc = s.case.n("c", N_CORR)
    corr = d.corr[:cc].copy()
    corr["index_query"] = np.minimum(corr["index_query"], max(ns - 1, 0))
    corr["index_match"] = np.minimum(corr["index_match"], max(nt - 1, 0))
    return ps, ns, pt, nt, s.arr(corr), cc


# ---------------------------------------------------------------------------------------------------------------- rows
# Each row: fn(side, data) makes one call through side.call and registers what is compared.  `counts` names the array counts of the
# signature (the zero / one cases), `optional` says whether the signature has optional arrays (the absent case).
ROWS = {}
TWIN = {}


def row(name, counts, optional=True, twin=None, label=None):
    def deco(fn):
        ROWS[label or name] = (name, fn, counts, optional)
        if twin:
            TWIN[name] = twin
        return fn
    return deco


# ---- lgr_align.hip
@row("lgr_correspondences_ex", ("ns", "nt"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt = clouds(s, d)
    fp = None if s.case.absent else capi.feature_params("fpfh")
    n_out = C.c_int(-7)
    out = s.out("out", (max(ns, 1),), capi.CORR_DTYPE)
    s.call("lgr_correspondences_ex", "pipipppp", ps, ns, pt, nt, params(s, d), None if fp is None else C.addressof(fp), out, s.hout("n_out", n_out))
    s.keep("out", n_out.value, 16)


@row("lgr_align_ex2", ("ns", "nt"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt = clouds(s, d)
    full = not s.case.absent
    fp = capi.feature_params("fpfh") if full else None
    res = capi.Result()
    s.call("lgr_align_ex2", "pipipppp", ps, ns, pt, nt, params(s, d, metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE if full else capi.METRIC_UNIFORMITY),
           None if fp is None else C.addressof(fp), metric_params(s, d, ns, full), s.hout("res", res, skip=result_skip()))


@row("lgr_measure", ("ns", "nt"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt = clouds(s, d)
    full = not s.case.absent
    n_times = 2
    runs = (capi.MeasureRun * n_times)()
    out = capi.Measurement()
    skip = []
    for i in range(n_times):
        skip += result_skip(i * C.sizeof(capi.MeasureRun) + capi.MeasureRun.result.offset)
    seeds = np.array([11, 12], np.uint64)
    s.call("lgr_measure", "pipipppppipp", ps, ns, pt, nt, params(s, d, metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE if full else capi.METRIC_UNIFORMITY),
           None, metric_params(s, d, ns, full), s.host(d.Tgt), s.host(seeds) if full else None, n_times,
           s.hout("runs", runs, skip=skip), s.hout("out", out, skip=_field_ranges(capi.Measurement, ("mtime", "stime"))))


# ---- lgr_analysis.hip
THR = 0.03


@row("lgr_overlap_rmse", ("ns", "nt"))
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    opt = not s.case.absent
    s.call("lgr_overlap_rmse", "pipippfpppp", ps, ns, pt, nt, s.host(d.T), s.host(d.Tgt), THR, s.hout("rmse", C.c_float(-1)), s.hout("size", C.c_int(-1)),
           s.hout("pcd_err", C.c_float(-1), opt), s.out("idx", (ns,), np.int32, opt))


@row("lgr_merge_overlaps", ("ns", "nt"))
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    opt = not s.case.absent
    s.call("lgr_merge_overlaps", "pipipfppppp", ps, ns, pt, nt, s.host(d.Tgt), THR, s.out("mask_src", (ns,), np.uint8, opt), s.out("mask_tgt", (nt,), np.uint8, opt),
           s.hout("n2", (C.c_int * 2)(-1, -1)), s.hout("overlap", C.c_float(-1)), s.hout("area", C.c_float(-1), opt))


@row("lgr_normal_difference", ("ns", "nt"), optional=False)
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    s.call("lgr_normal_difference", "pipipfpp", ps, ns, pt, nt, s.host(d.Tgt), THR, s.hout("diff", C.c_float(-1)), s.hout("n", C.c_int(-1)))


@row("lgr_correct_correspondences", ("ns", "nt", "c"))
def _(s, d):
    ps, ns, pt, nt, pc, cc = problem(s, d)
    opt = not s.case.absent
    s.call("lgr_correct_correspondences", "pipipipppp", ps, ns, pt, nt, pc, cc, s.host(d.Tgt), s.arr(d.mask[:cc]) if opt else None,
           s.out("correct", (cc,), np.uint8, opt), s.hout("n3", (C.c_int * 3)(-1, -1, -1)))


@row("lgr_evaluate_gt_batch", ("ns", "nt", "c", "n"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt, pc, cc = problem(s, d)
    opt = not s.case.absent
    n = s.case.n("n", 3)
    masks = np.stack([d.mask[:cc], 1 - d.mask[:cc], d.mask[:cc]])[:n] if n else np.zeros((0, cc), np.uint8)
    conv = np.array([1, 0, 1], np.int32)[:n]
    out = (capi.GtEval * max(n, 1))()
    s.call("lgr_evaluate_gt_batch", "pipipipipfpppp", ps, ns, pt, nt, pc, cc, s.host(d.tns[:n]), n, s.host(d.Tgt), THR, s.host(conv),
           s.arr(masks) if opt else None, s.hout("out", out), s.out("correct", (cc,), np.uint8, opt))


@row("lgr_evaluate_gt", ("ns", "nt", "c"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt, pc, cc = problem(s, d)
    opt = not s.case.absent
    s.call("lgr_evaluate_gt", "pipipippfippp", ps, ns, pt, nt, pc, cc, s.host(d.T), s.host(d.Tgt), THR, 1, s.arr(d.mask[:cc]) if opt else None,
           s.hout("out", capi.GtEval()), s.out("correct", (cc,), np.uint8, opt))


# ---- lgr_debug.hip
def temperature_out(s, tag, n, present):
    from lgr_amd import capi
    if not present:
        return None
    t = capi.TemperatureOut()
    for f in capi.TEMP_FIELDS:
        setattr(t, f, s.out(f"{tag}.{f}", (n,), np.float32))
    s.alive.append(t)
    return C.addressof(t)


@row("lgr_nearest", ("nq", "n"))
def _(s, d):
    nq, n = s.case.n("nq", 300), s.case.n("n", N_CLOUD)
    s.call("lgr_nearest", "pipipp", s.arr(d.src[:nq]), nq, s.arr(d.tgt[:n]), n, s.out("idx", (nq,), np.int32), s.out("d2", (nq,), np.float32, not s.case.absent))


@row("lgr_temperature_map", ("ns", "nt"))
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    s.call("lgr_temperature_map", "pipifpp", ps, ns, pt, nt, 0.05, temperature_out(s, "out", ns, not s.case.absent), s.hout("below", C.c_int(-1)))


@row("lgr_temperature_maps", ("ns", "nt"))
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    opt = not s.case.absent
    s.call("lgr_temperature_maps", "pipipfpppp", ps, ns, pt, nt, s.host(d.T), 0.05, temperature_out(s, "src", ns, opt), temperature_out(s, "tgt", nt, opt),
           s.out("moved", (ns, 12), np.float32, opt), s.hout("below2", (C.c_int * 2)(-1, -1)))


@row("lgr_compare_overlaps", ("ns", "nt", "n"))
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    opt = not s.case.absent
    n = s.case.n("n", 3)
    s.call("lgr_compare_overlaps", "pipipifppppp", ps, ns, pt, nt, s.host(d.tns[:n]), n, THR, s.hout("counts", (C.c_int32 * 3)(-1, -1, -1)),
           s.hout("weighted", (C.c_float * 3)(-1, -1, -1)), s.hout("counts2", (C.c_int32 * 6)(*([-1] * 6)), opt),
           s.out("mask_src", (n, ns), np.uint8, opt), s.out("mask_tgt", (n, nt), np.uint8, opt))


@row("lgr_color_correspondences", ("n", "n_kp", "c", "n_correct", "n_inl"))
def _(s, d):
    cs = s.case
    n, n_kp, cc, n_correct, n_inl = cs.n("n", N_CLOUD), cs.n("n_kp", 40), cs.n("c", N_CORR), cs.n("n_correct", 20), cs.n("n_inl", 30)
    kp = np.arange(0, 400, 10, dtype=np.int32)[:n_kp]
    # (the key points come first: the null case withholds them under n_kp > 0; the absent case has none at all)
    pk = None if cs.absent else s.arr(kp)
    s.call("lgr_color_correspondences", "ipipipipiip", n, pk, 0 if cs.absent else n_kp, s.arr(d.corr[:cc]), cc, s.arr(d.corr[5:5 + n_correct]), n_correct,
           s.arr(d.corr[10:10 + n_inl]), n_inl, 1, s.out("colors", (n,), np.int32))


@row("lgr_color_map", ("n",), optional=False)
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    s.call("lgr_color_map", "piffp", s.arr(d.values[:n]), n, -1.0, 1.5, s.out("colors", (n,), np.int32))


@row("lgr_color_weights", ("n",))
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    s.call("lgr_color_weights", "pipp", s.arr(d.weights[:n]), n, s.out("colors", (n,), np.int32), s.hout("range2", (C.c_float * 2)(-1, -1), not s.case.absent))


# ---- lgr_features.hip
@row("lgr_downsample", ("n",), optional=False, twin="lgr_downsample_order_dev")
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    n_out = C.c_int(-7)
    s.call("lgr_downsample", "pifipp", s.arr(d.src[:n]), n, 0.05, 0, s.out("out", (max(n, 1), 12), np.float32), s.hout("n_out", n_out),
           twin="lgr_downsample_order_dev")
    s.keep("out", n_out.value, 48)


@row("lgr_normals_knn", ("n", "ns"))
def _(s, d):
    n, ns = s.case.n("n", 400), s.case.n("ns", N_CLOUD)
    opt = not s.case.absent
    pts = s.inout("pts", d.src[:n].copy())
    s.call("lgr_normals_knn", "pipiipi", pts, n, s.arr(d.src[:ns]) if opt else None, ns if opt else 0, 30, s.host(d.pair["vp_src"]) if opt else None, 0)


@row("lgr_fpfh", ("m", "n"), optional=False)
def _(s, d):
    m, n = s.case.n("m", 300), s.case.n("n", N_CLOUD)
    s.call("lgr_fpfh", "pipifp", s.arr(d.src[:m]), m, s.arr(d.src[:n]), n, 0.08, s.out("out", (m, 33), np.float32))


# ---- lgr_grid.hip
@row("lgr_smoothed_densities", ("n",), optional=False)
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    s.call("lgr_smoothed_densities", "piip", s.arr(d.src[:n]), n, 2, s.out("out", (n,), np.float32))


# ---- lgr_gror.hip, lgr_teaser.hip
@row("lgr_gror", ("ns", "nt", "c"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt, pc, cc = problem(s, d)
    s.call("lgr_gror", "pipipifipp", ps, ns, pt, nt, pc, cc, THR, 800, s.hout("res", capi.Result(), skip=result_skip()),
           s.out("mask", (cc,), np.uint8, not s.case.absent))


@row("lgr_teaser", ("ns", "nt", "c"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt, pc, cc = problem(s, d)
    opt = not s.case.absent
    tp = capi.default_teaser_params(THR)
    s.call("lgr_teaser", "pipipippppp", ps, ns, pt, nt, pc, cc, C.addressof(tp), s.hout("res", capi.Result(), skip=result_skip()),
           s.hout("info", capi.TeaserInfo(), opt), s.out("clique", (2 * capi.TEASER_NODES_MAX,), np.int32, opt), s.out("mask", (cc,), np.uint8, opt))


# ---- lgr_hypotheses.hip
@row("lgr_fold_hypotheses", ("n",), optional=False)
def _(s, d):
    n = s.case.n("n", len(d.poses))
    max_set = 64
    n_out = C.c_int(-7)
    s.call("lgr_fold_hypotheses", "ppifipppp", s.arr(d.poses[:n]), s.arr(d.pose_metrics[:n]), n, 0.05, max_set, s.out("set_tns", (max_set, 16), np.float32),
           s.out("set_metrics", (max_set,), np.float32), s.out("set_index", (max_set,), np.int32), s.hout("n_out", n_out))
    s.keep("set_tns", n_out.value, 64)
    s.keep("set_metrics", n_out.value, 4)
    s.keep("set_index", n_out.value, 4)


# ---- lgr_iss.hip
@row("lgr_iss_keypoints", ("n",), optional=False)
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    n_out = C.c_int(-7)
    s.call("lgr_iss_keypoints", "pifffipp", s.arr(d.src[:n]), n, 0.06, 0.975, 0.975, 4, s.out("idx", (max(n, 1),), np.int32), s.hout("n_out", n_out))
    s.keep("idx", n_out.value, 4)


# ---- the matchers: lgr_match.hip, lgr_match_knn.hip, lgr_match_local.hip, lgr_match_local_knn.hip, lgr_match_dense.hip
def tables(s, d, row_len):
    mq, mt = s.case.n("mq", MQ), s.case.n("mt", MT)
    q, t = d.rows[row_len]
    return q[:mq], mq, t[:mt], mt


def one_match(name, row_len, with_block):
    def fn(s, d):
        q, mq, t, mt = tables(s, d, row_len)
        args = (s.arr(q), mq, s.arr(t), mt) + ((40,) if with_block else ()) + (s.out("idx", (mq,), np.int32), s.out("dist", (mq,), np.float32))
        s.call(name, "pipiipp" if with_block else "pipipp", *args)
    return fn


row("lgr_match_bf", ("mq", "mt"), optional=False)(one_match("lgr_match_bf", 33, True))
row("lgr_match_shot", ("mq", "mt"), optional=False)(one_match("lgr_match_shot", 352, True))
row("lgr_match_rops", ("mq", "mt"), optional=False)(one_match("lgr_match_rops", 135, True))
row("lgr_match_flann", ("mq", "mt"), optional=False)(one_match("lgr_match_flann", 33, False))


def by_row_len(name, counts, make):
    for L in (33, 135, 352):
        row(name, counts, optional=False, label=f"{name}[{L}]")(make(L))


def knn_row(L):
    def fn(s, d):
        q, mq, t, mt = tables(s, d, L)
        s.call("lgr_match_knn", "ipipiiipp", L, s.arr(q), mq, s.arr(t), mt, 40, K, s.out("idx", (mq, K), np.int32), s.out("dist", (mq, K), np.float32))
    return fn


def ratio_row(L):
    def fn(s, d):
        q, mq, t, mt = tables(s, d, L)
        s.call("lgr_match_ratio", "ipipiiifpp", L, s.arr(q), mq, s.arr(t), mt, 40, K, 1.01, s.out("idx", (mq,), np.int32), s.out("dist", (mq,), np.float32))
    return fn


def flann_rows_row(L):
    def fn(s, d):
        q, mq, t, mt = tables(s, d, L)
        s.call("lgr_match_flann_rows", "ipipipp", L, s.arr(q), mq, s.arr(t), mt, s.out("idx", (mq,), np.int32), s.out("dist", (mq,), np.float32))
    return fn


def local_knn_row(L):
    def fn(s, d):
        q, mq, t, mt = tables(s, d, L)
        s.call("lgr_match_local_knn", "ipipipppfipp", L, s.arr(d.src[:mq]), mq, s.arr(d.tgt[:mt]), mt, s.arr(q), s.arr(t), s.host(d.Tgt), 0.3, K,
               s.out("idx", (mq, K), np.int32), s.out("dist", (mq, K), np.float32))
    return fn


by_row_len("lgr_match_knn", ("mq", "mt"), knn_row)
by_row_len("lgr_match_ratio", ("mq", "mt"), ratio_row)
by_row_len("lgr_match_flann_rows", ("mq", "mt"), flann_rows_row)
by_row_len("lgr_match_local_knn", ("mq", "mt"), local_knn_row)


@row("lgr_match_local", ("mq", "mt"), optional=False)
def _(s, d):
    q, mq, t, mt = tables(s, d, 33)
    s.call("lgr_match_local", "pipipppfpp", s.arr(d.src[:mq]), mq, s.arr(d.tgt[:mt]), mt, s.arr(q), s.arr(t), s.host(d.Tgt), 0.3,
           s.out("idx", (mq,), np.int32), s.out("dist", (mq,), np.float32))


@row("lgr_vote_matches", ("mq", "mt"), optional=False)
def _(s, d):
    mq, mt = s.case.n("mq", MQ), s.case.n("mt", MT)
    cand = np.minimum(d.cand_idx[:mq], mt - 1)   # entries stay below mt
    s.call("lgr_vote_matches", "ppiipifpp", s.arr(cand), s.arr(d.cand_dist[:mq]), mq, K, s.arr(d.tgt[:mt]), mt, 0.06,
           s.out("idx", (mq,), np.int32), s.out("dist", (mq,), np.float32))


@row("lgr_ratio_test", ("mq",), optional=False)
def _(s, d):
    mq = s.case.n("mq", MQ)
    s.call("lgr_ratio_test", "ppiifpp", s.arr(d.cand_idx[:mq]), s.arr(d.cand_dist[:mq]), mq, K, 1.01, s.out("idx", (mq,), np.int32), s.out("dist", (mq,), np.float32))


# ---- lgr_plane_dense.hip, lgr_refine.hip
@row("lgr_evaluate_plane_dense", ("ns", "nt"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt = clouds(s, d)
    opt = not s.case.absent
    out = capi.PlaneDenseEval()
    s.call("lgr_evaluate_plane_dense", "pipipipfppp", ps, ns, pt, nt, s.host(d.T), capi.SCORE_MSE, metric_params(s, d, ns, opt), 0.0, s.hout("out", out),
           s.out("inliers", (max(ns, 1),), capi.CORR_DTYPE, opt), s.out("nn", (ns,), np.int32, opt))
    s.keep("inliers", out.n_inliers, 16)


def analysis_metric_row(plane):
    def fn(s, d):
        from lgr_amd import capi
        ps, ns, pt, nt, pc, cc = problem(s, d)
        opt = not s.case.absent
        out = capi.MetricEval()
        s.call("lgr_analysis_metric", "pipipippiipppp", ps, ns, pt, nt, pc, cc, s.host(d.T), s.host(d.Tgt) if opt else None,
               capi.METRIC_WEIGHTED_CLOSEST_PLANE if plane else capi.METRIC_UNIFORMITY, capi.SCORE_MSE, metric_params(s, d, ns, opt and plane),
               s.hout("out", out), s.out("mask", (cc,), np.uint8, opt), s.out("inliers", (max(ns, 1),), capi.CORR_DTYPE, opt))
        s.keep("inliers", out.n_inliers if plane else 0, 16)
    return fn


row("lgr_analysis_metric", ("ns", "nt", "c"), label="lgr_analysis_metric[uniformity]")(analysis_metric_row(False))
row("lgr_analysis_metric", ("ns", "nt", "c"), label="lgr_analysis_metric[weighted_plane]")(analysis_metric_row(True))


@row("lgr_refine_plane", ("ns", "nt"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt = clouds(s, d)
    opt = not s.case.absent
    rp = capi.refine_params(max_steps=3)
    s.call("lgr_refine_plane", "pipipppppp", ps, ns, pt, nt, s.host(d.T), C.addressof(rp), metric_params(s, d, ns, opt),
           s.hout("out", capi.RefineResult()), s.hout("trace", (capi.RefineStep * 5)(), opt), s.hout("n_trace", C.c_int(-7), opt))


# ---- lgr_preprocess.hip
@row("lgr_preprocess", ("n",), twin="lgr_preprocess_order_dev")
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    opt = not s.case.absent
    n_out = C.c_int(0)
    s.call("lgr_preprocess", "pipiippp", s.arr(d.pair["src"][:n]), n, s.host(d.pair["vp_src"]) if opt else None, 0, 0, s.out("out", (max(n, 1), 12), np.float32),
           s.hout("n_out", n_out), s.hout("voxel", C.c_float(-1), opt), twin="lgr_preprocess_order_dev")
    s.keep("out", n_out.value, 48)


# ---- lgr_ransac.hip
@row("lgr_ransac_ex", ("ns", "nt", "c"))
def _(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt, pc, cc = problem(s, d)
    opt = not s.case.absent
    s.call("lgr_ransac_ex", "pipipipppp", ps, ns, pt, nt, pc, cc, params(s, d, metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE if opt else capi.METRIC_UNIFORMITY),
           metric_params(s, d, ns, opt), s.hout("res", capi.Result(), skip=result_skip()),
           # fewer correspondences than a sample: the twin leaves the mask alone, the host form zeroes the caller's
           s.out("mask", (cc,), np.uint8, opt, init=np.zeros(cc, np.uint8) if s.dev and 0 < cc < 3 else None))


# (the twin takes no cloud sizes, so only the list's count has a zero / one case: an empty cloud is refused by the host form alone)
@row("lgr_refit_svd", ("n",), optional=False)
def _(s, d):
    ps, ns, pt, nt = clouds(s, d)
    cc = s.case.n("n", N_CORR)
    pc = s.arr(d.corr[:cc])
    T = s.hout("T", (C.c_float * 16)(*([-1.0] * 16)))
    if s.dev:   # the twin has no sizes: (d_src, d_tgt, d_corr, c, d_mask, T16)
        s.call("lgr_refit_svd", "pppipp", ps, pt, pc, cc, None, T)
    else:
        s.call("lgr_refit_svd", "ppiipip", ps, pt, ns, nt, pc, cc, T)


@row("lgr_choose_best_hypothesis", ("ns", "nt", "c", "n"))
def _(s, d):
    ps, ns, pt, nt, pc, cc = problem(s, d)
    n = s.case.n("n", 3)
    s.call("lgr_choose_best_hypothesis", "pipipipippp", ps, ns, pt, nt, pc, cc, s.host(d.tns[:n]), n, s.hout("T", (C.c_float * 16)(*([-1.0] * 16))),
           s.hout("best", C.c_int(-7)), s.hout("uniformities", (C.c_float * 3)(-1, -1, -1), not s.case.absent))


def multi_row(ex):
    def fn(s, d):
        from lgr_amd import capi
        ps, ns, pt, nt, pc, cc = problem(s, d)
        opt = ex and not s.case.absent
        max_set = 16
        tail = (max_set, s.hout("res", capi.Result(), skip=result_skip()), s.hout("out", (capi.Hypothesis * max_set)()), s.hout("n_out", C.c_int(-7)),
                s.hout("best", C.c_int(-7)))
        p = params(s, d, metric_id=capi.METRIC_WEIGHTED_CLOSEST_PLANE if opt else capi.METRIC_UNIFORMITY)
        if ex:
            s.call("lgr_ransac_multi_ex", "pipipippipppp", ps, ns, pt, nt, pc, cc, p, metric_params(s, d, ns, opt), *tail)
        else:
            s.call("lgr_ransac_multi", "pipipipipppp", ps, ns, pt, nt, pc, cc, p, *tail)
    return fn


row("lgr_ransac_multi", ("ns", "nt", "c"), optional=False)(multi_row(False))
row("lgr_ransac_multi_ex", ("ns", "nt", "c"))(multi_row(True))


# ---- lgr_rops.hip, lgr_shot.hip
def frames(s, d, m):
    """m x 9 frames for the rows that take them: the SHOT frames of the first m source points, computed once by the host form"""
    if d.lrf is None:
        lrf = np.zeros((300, 9), np.float32)
        fn = lib().lgr_shot_lrf
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        assert fn(s.ctx.h, d.src.ctypes.data, 300, d.src.ctypes.data, N_CLOUD, 0.08, lrf.ctypes.data) == 0
        d.lrf = lrf
    return d.lrf[:m]


def kps_surf(s, d):
    m, n = s.case.n("m", 300), s.case.n("n", N_CLOUD)
    return s.arr(d.src[:m]), m, s.arr(d.src[:n]), n


@row("lgr_gravity_lrf", ("m", "n"), optional=False)
def _(s, d):
    pk, m, psf, n = kps_surf(s, d)
    s.call("lgr_gravity_lrf", "pipifp", pk, m, psf, n, 0.08, s.out("out", (m, 9), np.float32))


@row("lgr_rops", ("m", "n"), optional=False)
def _(s, d):
    pk, m, psf, n = kps_surf(s, d)
    s.call("lgr_rops", "pipifpp", pk, m, psf, n, 0.08, s.arr(frames(s, d, m)), s.out("out", (m, 135), np.float32))


@row("lgr_shot_lrf", ("m", "n"), optional=False)
def _(s, d):
    pk, m, psf, n = kps_surf(s, d)
    s.call("lgr_shot_lrf", "pipifp", pk, m, psf, n, 0.08, s.out("out", (m, 9), np.float32))


@row("lgr_shot", ("m", "n"))
def _(s, d):
    pk, m, psf, n = kps_surf(s, d)
    opt = not s.case.absent
    s.call("lgr_shot", "pipifppp", pk, m, psf, n, 0.08, s.arr(frames(s, d, m)) if opt else None, s.out("out", (m, 352), np.float32),
           s.out("out_lrf", (m, 9), np.float32, opt))


# ---- lgr_weights.hip
@row("lgr_principal_curvatures", ("n",), optional=False)
def _(s, d):
    n = s.case.n("n", N_CLOUD)
    s.call("lgr_principal_curvatures", "piipp", s.arr(d.src[:n]), n, 30, s.out("pc1", (n,), np.float32), s.out("pc2", (n,), np.float32))


@row("lgr_weights", ("n",))
def _(s, d):
    from lgr_amd import capi
    n = s.case.n("n", N_CLOUD)
    s.call("lgr_weights", "piiipp", s.arr(d.src[:n]), n, capi.WEIGHT_IDS["curvedness"], 30, s.out("out", (n,), np.float32),
           s.hout("sum", C.c_float(-1), not s.case.absent))


# ---- no twin: compared with the documented contract / the oracle's restatement (NO_TWIN)
def selfcheck_rcp(ctx, case):
    out2 = (C.c_ulonglong * 2)(7, 7)
    lo, hi = (int(np.float32(v).view(np.uint32)) for v in (1.0, 1.001))
    fn = lib().lgr_selfcheck_rcp
    fn.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    rc = fn(ctx.h, lo, hi, None if case.kind == "null" else out2)
    return rc, lambda: list(out2) == [0, hi - lo + 1]


def selfcheck_libm(ctx, case, oracle):
    n = case.n("n", 1000)
    a = np.linspace(-1, 1, 1000, dtype=np.float32)[:n].copy()
    b = np.linspace(0.5, 2, 1000, dtype=np.float32)[:n].copy()
    out = np.full(max(n, 1), -7, np.float32)
    fn = lib().lgr_selfcheck_libm
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    f = 0 if case.absent else 2   # acosf takes no second array; atan2f does
    rc = fn(ctx.h, f, None if case.kind == "null" else a.ctypes.data, None if case.absent else b.ctypes.data, n, out.ctypes.data)

    def same():
        want = oracle.libm_eval(oracle.LIBM_ACOSF, a) if case.absent else oracle.libm_eval(oracle.LIBM_ATAN2F, a, b)
        return out[:n].tobytes() == np.asarray(want, np.float32).tobytes() and (n > 0 or out[0] == -7)
    return rc, same


NO_TWIN = {"lgr_selfcheck_rcp": ((), False), "lgr_selfcheck_libm": (("n",), True)}

# host forms with a twin that are no rows: they stage no array
NO_STAGING = {
    "lgr_correspondences": "forwards to the host form lgr_correspondences_ex, stages no array itself",
    "lgr_ransac": "forwards to the host form lgr_ransac_ex, stages no array itself",
    "lgr_align": "forwards to the host form lgr_align_ex2 (through lgr_align_ex), stages no array itself",
    "lgr_align_ex": "forwards to the host form lgr_align_ex2, stages no array itself",
    "lgr_cloud_prepare": "copies the points into the prepared cloud's own allocation, stages no array in the context",
    "lgr_cloud_keypoints": "copies out of the prepared cloud's own memory, stages no array",
    "lgr_cloud_level": "copies out of the prepared cloud's own memory, stages no array",
    "lgr_correspondences_prepared": "takes prepared clouds, stages no array (the result is read from the pipeline's own slot)",
}

# return code of the host form when its first array is NULL under a positive count, as recorded on the commit that added this file
NULL_RC = {name: -1 for name in list(ROWS) + list(NO_TWIN)}   # LGR_ERR_INVALID_ARG everywhere


def cases_of(counts, optional):
    out = [Case("full")] + ([Case("absent")] if optional else [])
    for c in counts:
        out += [Case("zero", c), Case("one", c)]
    return out + [Case("null")]


PARAMS = [pytest.param(label, case, id=f"{label}-{case}") for label, (_, _, counts, optional) in ROWS.items()
          for case in cases_of(counts, optional)]


@pytest.mark.parametrize("label,case", PARAMS)
def test_host_form_equals_dev_twin(lgr, label, case):
    name, fn = ROWS[label][:2]
    d = data(lgr)
    host = Side(lgr, False, case)
    fn(host, d)
    got = host.results()
    if case.kind == "null":
        assert host.rc == NULL_RC[label]
        return
    dev = Side(lgr, True, case)
    fn(dev, d)
    want = dev.results()
    print(f"{label} {case}: rc host {host.rc} twin {dev.rc}, outputs {sorted(got)}")
    assert host.rc == dev.rc
    if case.kind == "full":
        assert host.rc == 0   # the full case compares results, not two refusals
    if host.rc != 0:
        return   # a refused call: the host form returns before its download, what the twin had written by then is nobody's result
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k] == want[k], f"{name}: output {k!r} differs between the host form and the twin"


@pytest.mark.parametrize("name,case", [pytest.param(n, c, id=f"{n}-{c}") for n, (counts, optional) in NO_TWIN.items() for c in cases_of(counts, optional)])
def test_host_form_without_twin(lgr, oracle, name, case):
    rc, same = selfcheck_rcp(lgr, case) if name == "lgr_selfcheck_rcp" else selfcheck_libm(lgr, case, oracle)
    if case.kind == "null":
        assert rc == NULL_RC[name]
        return
    assert rc == 0
    assert same()


# ---------------------------------------------------------------------------------------------------------------- completeness
# the host entry points the layer consists of (the refactor's list): every one must be a row
LISTED = """lgr_correspondences_ex lgr_align_ex2 lgr_measure lgr_overlap_rmse lgr_merge_overlaps lgr_normal_difference lgr_correct_correspondences
lgr_evaluate_gt_batch lgr_evaluate_gt lgr_nearest lgr_temperature_map lgr_temperature_maps lgr_compare_overlaps lgr_color_correspondences lgr_downsample
lgr_selfcheck_rcp lgr_selfcheck_libm lgr_normals_knn lgr_fpfh lgr_smoothed_densities lgr_gror lgr_fold_hypotheses lgr_iss_keypoints lgr_match_bf
lgr_match_knn lgr_vote_matches lgr_ratio_test lgr_match_ratio lgr_match_flann lgr_match_local lgr_match_local_knn lgr_match_flann_rows
lgr_evaluate_plane_dense lgr_analysis_metric lgr_preprocess lgr_ransac_ex lgr_refit_svd lgr_choose_best_hypothesis lgr_ransac_multi lgr_ransac_multi_ex
lgr_refine_plane lgr_gravity_lrf lgr_rops lgr_teaser lgr_principal_curvatures lgr_weights
lgr_shot lgr_shot_lrf lgr_match_shot lgr_match_rops lgr_color_map lgr_color_weights""".split()


def test_table_is_complete():
    text = open(os.path.join(ROOT, "include", "lgr.h")).read()
    declared = set(re.findall(r"\b(lgr_\w+)\s*\(", text))
    hosts = {x for x in declared if not x.endswith("_dev") and (x + "_dev" in declared or x + "_order_dev" in declared)}
    in_table = {r[0] for r in ROWS.values()} | set(NO_TWIN)
    assert len(LISTED) == 52 and set(LISTED) <= in_table
    assert not (in_table & set(NO_STAGING))
    missing = hosts - in_table - set(NO_STAGING)
    assert not missing, f"host forms with a twin that are neither a row nor in NO_STAGING: {sorted(missing)}"
    assert (in_table - set(NO_TWIN)) <= hosts, sorted(in_table - set(NO_TWIN) - hosts)
    for name in in_table - set(NO_TWIN):   # every twin a row calls is declared
        assert TWIN.get(name, name + "_dev") in declared, name
