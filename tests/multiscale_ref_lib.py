"""CPU statement of the multi-scale correspondence search (feature_radius unset) with a pluggable descriptor.

Restates include/matching.h:176-262 (initialize) and :264-352 (match_multiscale) from pieces that are already pinned on their own:
oracle.knn / downsample / normals_knn / fpfh / match_bf / filter_matches / iss_keypoints, tests/shot_ref_lib.py and
tests/rops_ref_lib.py.  The host arithmetic of the level assignment calls the running libm's log2f and powf (as the pipeline's host
code and the oracle do), the proximity vote is float32 throughout.

With the fpfh adapter the composition equals oracle.correspondences(feature_radius = 0) bit for bit (tests/test_multiscale_ref.py);
with the shot and rops adapters it is the reference for the device path (tests/test_gpu_multiscale_descriptors.py)."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

_libm = C.CDLL("libm.so.6")
_libm.log2f.restype = C.c_float
_libm.log2f.argtypes = [C.c_float]
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]
F = np.float32


def log2f(x):
    return F(_libm.log2f(float(x)))


def powf(x, y):
    return F(_libm.powf(float(x), float(y)))


def level_of(d2_4th, nr, scale):
    """:183-185 per key point: density = sqrtf(d2); feature_radius = sqrtf((float) nr * d * d / M_PI) (the product in float, the
    division in double, rounded to float before sqrtf); floor(log2f(r) / log2f(scale))"""
    d = np.sqrt(np.asarray(d2_4th, F))
    fr = np.sqrt(((F(nr) * d * d).astype(np.float64) / math.pi).astype(F))
    ls = log2f(scale)
    return np.array([int(math.floor(F(log2f(r) / ls))) for r in fr], np.int64)


def radius_voxel(level, nr, scale):
    """:229-230 search radius powf(scale, level) and voxel sqrtf(M_PI * r * r / (float) nr) (double product, rounded to float)"""
    r = powf(scale, F(level))
    v = np.sqrt(F(math.pi * float(r) * float(r) / float(F(nr))))
    return r, F(v)


# ---- descriptor adapters: rows(kps_level, surf, radius, vp) and match(q, t, block)
class Fpfh:
    name, dim = "fpfh", 33

    def __init__(self, oracle):
        self.o = oracle

    def rows(self, kps, surf, radius, vp):
        return self.o.fpfh(kps, surf, float(radius))

    def match(self, q, t, block):
        return self.o.match_bf(q, t, int(block))


class Shot:
    name, dim = "shot", 352

    def __init__(self, oracle):
        import shot_ref_lib
        self.ref = shot_ref_lib

    def rows(self, kps, surf, radius, vp):
        return self.ref.shot(kps, surf, float(radius))[0]

    def match(self, q, t, block):
        return self.ref.match(q, t, int(block))


class Rops:
    """gravity frames; :243-246: the key points' normals are re-estimated on the level's surface first (normals_available = true)"""
    name, dim = "rops", 135

    def __init__(self, oracle, normal_k=30, reestimate=True):
        import rops_ref_lib
        self.o, self.ref, self.k, self.reestimate = oracle, rops_ref_lib, normal_k, reestimate
        self.frames = []            # (kps with re-estimated normals, gravity-test failure mask) per rows() call, for fixture checks

    def rows(self, kps, surf, radius, vp):
        kn = self.o.normals_knn(kps, self.k, surf=surf, vp=vp, normals_available=True) if self.reestimate else kps
        _, fail = self.ref.gravity_only(kn)
        self.frames.append((kn, fail))
        fr = self.ref.gravity_lrf(kn, surf, float(radius))
        return self.ref.rops(kn, surf, float(radius), fr)

    def match(self, q, t, block):
        return self.ref.match(q, t, int(block))


ADAPTERS = {"fpfh": Fpfh, "shot": Shot, "rops": Rops}

# the fixtures of lgr_amd/synthetic.py (F1 make_two_density_pair, F2 make_pruned_pair, F3 make_disjoint_levels_pair,
# F4 make_duplicates_pair, F5 make_lattice_pair) x key points -> ISS / vote radii of source and target.  F3's target is about 80 times
# sparser: its ISS radius follows.  F4 'any' and F5: a vote window (32 r) below the point spacing, so that candidates of one query
# count 1 each and the distance tie-break decides.
CASES = {("F1", "any"): (0.05, 0.05), ("F1", "iss"): (0.06, 0.06), ("F2", "any"): (0.05, 0.05), ("F2", "iss"): (0.06, 0.06),
         ("F3", "any"): (0.05, 0.05), ("F3", "iss"): (0.06, 0.5), ("F4", "any"): (0.01, 0.01), ("F4", "iss"): (0.06, 0.06),
         ("F5", "any"): (0.001, 0.001)}


def fixture(name):
    from lgr_amd import synthetic as S
    return {"F1": S.make_two_density_pair, "F2": S.make_pruned_pair, "F3": S.make_disjoint_levels_pair, "F4": S.make_duplicates_pair,
            "F5": S.make_lattice_pair}[name]()


class Side:
    """initialize() of one cloud: level per key point, pruning, per-level key-point lists, surfaces and rows"""

    def __init__(self, oracle, cloud, kps, iss_radius, adapter, vp=None, nr=352, normal_k=30, scale=2.0, normals_available=False):
        self.kps, self.iss_radius = kps, F(iss_radius)
        _, d2 = oracle.knn(kps, cloud, 5)
        lv = level_of(d2[:, 4], nr, scale)
        lo, hi = int(lv.min()), int(lv.max())
        count = np.bincount(lv - lo, minlength=hi - lo + 1)
        mx = int(count.max())
        f, b = 0, len(count)
        while 10 * count[f] < mx:       # :195-198
            f += 1
        while 1000 * count[b - 1] < mx:  # :199-202
            b -= 1
        self.raw = dict(min_l2=lo, max_l2=hi, count=count.tolist())
        self.min_l2, self.max_l2 = lo + f, lo + b - 1
        cl = np.clip(lv, self.min_l2, self.max_l2)
        self.n_clamped_up = int((lv < self.min_l2).sum())
        self.n_clamped_down = int((lv > self.max_l2).sum())
        self.level = cl
        n_scales = self.max_l2 - self.min_l2 + 1
        # :219-223 key point i takes part in every level from its own up to the largest
        self.lists = [np.nonzero(cl <= self.min_l2 + s)[0].astype(np.int32) for s in range(n_scales)]
        self.radius, self.voxel, self.surf, self.rows = [], [], [], []
        prev = cloud
        for s in range(n_scales):
            r, v = radius_voxel(self.min_l2 + s, nr, scale)
            ds = oracle.normals_knn(oracle.downsample(prev, float(v)), normal_k, vp=vp, normals_available=normals_available)
            self.radius.append(r); self.voxel.append(v); self.surf.append(ds)
            self.rows.append(adapter.rows(kps[self.lists[s]], ds, r, vp))
            prev = ds

    def record(self):
        return dict(raw=self.raw, min_l2=self.min_l2, max_l2=self.max_l2, sizes=[len(x) for x in self.lists],
                    n_clamped_up=self.n_clamped_up, n_clamped_down=self.n_clamped_down,
                    radius=[float(r) for r in self.radius], voxel=[float(v) for v in self.voxel])


def level_tables(q, t, adapter, block):
    """:267-315 per common level the 1-NN table of q's level rows against t's; NaN query rows and unmatched rows add nothing
    (matchBF leaves them empty).  Returns per query key point the candidate lists (train key point, distance), level order."""
    cand = [[] for _ in range(len(q.kps))]
    lo, hi = max(q.min_l2, t.min_l2), min(q.max_l2, t.max_l2)
    for level in range(lo, hi + 1):
        iq, it = level - q.min_l2, level - t.min_l2
        qr = q.rows[iq]
        idx, dist = adapter.match(qr, t.rows[it], block)
        ok = np.isfinite(qr).all(1) & (idx >= 0)
        for a in np.nonzero(ok)[0]:
            cand[q.lists[iq][a]].append((int(t.lists[it][idx[a]]), F(dist[a])))
    return cand


def vote(cand, t):
    """:316-349 in float32: counter[m1] sums over m2 from m1 on, (dx*dx + dy*dy) + dz*dz, the 32 * iss_radius window; the largest
    count wins, ties by the smaller distance under a strict '<' from {0, 0}"""
    xyz = np.ascontiguousarray(t.kps[:, :3], F)
    r = t.iss_radius
    win = F(32) * r
    idx = np.full(len(cand), -1, np.int32)
    dist = np.zeros(len(cand), F)
    stats = dict(count_ties=0, dist_ties=0, decisive_ties=0)   # equal counts; and equal distances; and a different train key point
    for i, c in enumerate(cand):
        best_c, best_d, best = F(0), F(0), -1
        for m1 in range(len(c)):
            cnt = F(0)
            a = xyz[c[m1][0]]
            for m2 in range(m1, len(c)):
                d = a - xyz[c[m2][0]]
                dl = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                if dl < win:
                    cnt = F(cnt + r / max(dl, r))
            dm = c[m1][1]
            if best >= 0 and cnt == best_c:
                stats["count_ties"] += 1
                stats["dist_ties"] += int(dm == best_d)
                stats["decisive_ties"] += int(dm == best_d and c[m1][0] != c[best][0])   # '<=' would pick another key point
            if cnt > best_c or (cnt == best_c and dm < best_d):
                best_c, best_d, best = cnt, dm, m1
        if best >= 0:
            idx[i], dist[i] = c[best]
    return idx, dist, stats


class Statement:
    """the multi-scale search of one (src, tgt, key points, descriptor) case; tables cached per block size, filters run from them"""

    def __init__(self, oracle, src, tgt, descriptor="fpfh", keypoints="any", iss_radius=(0.05, 0.05), vp=(None, None),
                 nr=352, normal_k=30, scale=2.0, normals_available=False, adapter=None):
        self.o, self.src, self.tgt = oracle, src, tgt
        self.adapter = adapter or ADAPTERS[descriptor](oracle)
        self.kidx = [None, None]
        kps = [src, tgt]
        if keypoints == "iss":
            for c, cloud in enumerate((src, tgt)):
                self.kidx[c] = oracle.iss_keypoints(cloud, float(F(iss_radius[c])))
                kps[c] = np.ascontiguousarray(cloud[self.kidx[c]])
        self.kps = kps
        self.empty = len(kps[0]) == 0 or len(kps[1]) == 0
        self.sides = None
        if not self.empty:
            self.sides = [Side(oracle, cloud, k, r, self.adapter, v, nr, normal_k, scale, normals_available)
                          for cloud, k, r, v in zip((src, tgt), kps, iss_radius, vp)]
        self._tables = {}
        self.vote_stats = {}

    def records(self):
        return None if self.empty else [s.record() for s in self.sides]

    def tables(self, block):
        if block not in self._tables:
            s, t = self.sides
            ij, dij, st_ij = vote(level_tables(s, t, self.adapter, block), t)
            ji, dji, st_ji = vote(level_tables(t, s, self.adapter, block), s)
            self._tables[block] = (ij, dij, ji, dji)
            self.vote_stats[block] = (st_ij, st_ji)
        return self._tables[block]

    def correspondences(self, matching_id, block, distance_thr=0.1, cluster_k=40):
        if self.empty:
            return np.zeros(0, self.o.CORR_DTYPE)
        ij, dij, ji, dji = self.tables(block)
        out = self.o.filter_matches(matching_id, self.kps[0], self.kps[1], ij, dij, ji, dji, distance_thr, cluster_k)
        if self.kidx[0] is not None:        # finalize(): local key-point indices -> cloud indices
            out["query"] = self.kidx[0][out["query"]]
            out["match"] = self.kidx[1][out["match"]]
        return out
