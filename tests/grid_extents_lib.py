"""Scenes for tests/test_oracle_grid_extents.py and tests/test_gpu_grid_extents.py: a compact blob plus a few stray points that stretch
the bounding box the uniform grid is laid over ("The cell size of a grid").  numpy only.

A scene is the blob (synthetic.make_pair(4000)["src"], about 1 x 1 x 0.8 m, normals estimated on the blob alone), then -- `thin` only --
the constructed points, then the strays, so a blob point keeps its index in every scene.  A stray is a copy of blob point 0 with ONE
coordinate moved to (box minimum - extent), which becomes the grid's origin along that axis; the extents are given in multiples of the search radius r, whose cell is h0 = fl(1.001f * r):

  room   no strays                                       a few cells per axis: the control
  gap    640 x 640 x 400 r                               1.28e8 < cells <= 2.56e8: between the cap the oracle had and the device's
  over   1200 x 1200 x 800 r                             1.15e9 cells: one doubling at the cap, 27 cells of 2.002 r
  many   1e5 r along every axis                          1e15 cells: eight doublings, the blob in one or two cells per axis
  thin   1e5 r along x only                              1e5 x 11 x 28 cells, below the cap: the per-axis bound alone doubles h
  flat   1e5 r along x and y                             8e10 cells: three doublings at the cap, the blob one cell thick along z

`thin` also holds constructed points above the blob, 1e5 cells from the origin along x, where the float cell coordinate fl(fl(v - o) / h0) has an error of several thousandths
of a cell: a target p and a query q with fl(d2) < fl(r * r) whose x cells at h0 are TWO apart (a 27-cell visit at h0 misses p), and a
cluster of five targets c0..c4 (equal x, y a few tenths of a millimetre apart) with the same relation to a query qc (SHOT needs five
neighbours).  p and the cluster are part of the cloud; q and qc are queries only."""
import numpy as np

F = np.float32
N_BLOB = 4000
EXTENTS = dict(room=None, gap=(640, 640, 400), over=(1200, 1200, 800), many=(1e5, 1e5, 1e5), thin=(1e5, 0, 0), flat=(1e5, 1e5, 0))
# cells at h0 (before any doubling) that each scene is built to have: (more than, at most)
CELLS = dict(room=(1, 1e5), gap=(1.28e8, 2.56e8), over=(2.56e8, 8 * 2.56e8), many=(1e14, 1e16), thin=(1e6, 1.28e8),
             flat=(1e10, 1e12))
MAX_CELLS, MAX_DIM_H0, MAX_DIM = 256e6, 4096, 1 << 20


def cell(r):
    """h0 = fl(1.001f * r), the cell the radius searches ask for"""
    return F(F(1.001) * F(r))


def cellc(v, o, h):
    """the builders' float expression (int) floorf(fl(fl(v - o) / h)), element-wise"""
    return np.floor((np.asarray(v, F) - F(o)) / F(h)).astype(np.int64)


def dims(xyz, h):
    """cells per axis of the box of xyz at cell h (no doubling)"""
    xyz = np.asarray(xyz, F)
    mn, mx = xyz.min(0), xyz.max(0)
    return np.array([cellc(mx[a], mn[a], h) + 1 for a in range(3)], np.int64)


def rule(xyz, h0):
    """DESIGN.md section 4 restated: (h, dims, doublings) the builders must arrive at from the box of xyz and the cell h0"""
    h, k = F(h0), 0
    while True:
        d = dims(xyz, h)
        if float(d[0]) * float(d[1]) * float(d[2]) <= MAX_CELLS and d.max() <= (MAX_DIM_H0 if k == 0 else MAX_DIM):
            return h, d, k
        h, k = F(h * F(2)), k + 1


def blob(oracle, seed=12):
    """the blob with the oracle's normals (30-NN, towards the scene's viewpoint), n x 12 float32"""
    from lgr_amd import synthetic
    p = synthetic.make_pair(N_BLOB, seed=seed)
    return oracle.normals_knn(p["src"], 30, vp=p["vp_src"])


def strays(b, name, r):
    """the stray points of scene `name` for the radius r: copies of blob point 0 with one coordinate at box minimum - extent * r (the grid's origin moves there)"""
    ext = EXTENTS[name]
    out = []
    if ext is not None:
        mn = b[:, :3].min(0)
        for a in range(3):
            if ext[a]:
                s = b[0].copy()
                s[a] = F(mn[a] - F(ext[a]) * F(r))
                out.append(s)
    return np.stack(out).astype(F) if out else np.zeros((0, 12), F)


def point(xyz, normal=(0.0, 0.0, 1.0)):
    p = np.zeros(12, F)
    p[:3] = xyz; p[3] = 1; p[4:7] = normal; p[8] = 1
    return p


def d2_f32(a, b):
    """lgr_dist2 / orc::dist2: ((dx dx) + dy dy) + dz dz in float32; a [m, >= 3] against b [n, >= 3] -> [m, n]"""
    d = np.asarray(a, F)[:, None, :3] - np.asarray(b, F)[None, :, :3]
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def constructed(b, r, seed=1):
    """`thin`'s constructed points for the blob b and radius r: dict(p, q, cluster [5, 12], qc).  Seeded search: x of the target uniform
    over the blob's x range, the query up to 1 % of r short of r farther along x, y and z equal (10 r and 20 r above the blob, so the
    blob is out of reach); the origin is the x stray's coordinate, 1e5 r below the blob."""
    rng = np.random.default_rng(seed)
    h0, r2 = cell(r), F(F(r) * F(r))
    mn, mx = b[:, :3].min(0), b[:, :3].max(0)
    ox = strays(b, "thin", r)[0, 0]
    c = ((mn + mx) / 2).astype(F)
    found = []
    for _ in range(100):
        xp = rng.uniform(mn[0], mx[0], 1000000).astype(F)
        xq = (xp + rng.uniform(0.99 * r, 0.9999 * r, len(xp)).astype(F)).astype(F)
        dx = (xq - xp).astype(F)
        ok = (F(1.0001) * (dx * dx) < r2) & (cellc(xq, ox, h0) - cellc(xp, ox, h0) == 2)
        found += [(xp[i], xq[i]) for i in np.flatnonzero(ok)[:2]]
        if len(found) >= 2:
            break
    assert len(found) >= 2, "no pair two cells apart within the radius: the scene no longer reaches the rounding it was built for"
    (xp, xq), (xc, xqc) = found[:2]
    p, q = point((xp, c[1], mx[2] + F(10 * r))), point((xq, c[1], mx[2] + F(10 * r)))
    cl = np.stack([point((xc, c[1] + F(k * 2e-3 * r), mx[2] + F(20 * r))) for k in range(5)])   # 8e-3 r across: d2 grows by less than 1e-4 r^2
    qc = point((xqc, c[1], mx[2] + F(20 * r)))
    return dict(p=p, q=q, cluster=cl, qc=qc)


def scene(b, name, r, extra=None):
    """blob + extra (thin's constructed targets) + strays -> n x 12 float32"""
    parts = [b] + ([] if extra is None else [np.atleast_2d(extra)]) + [strays(b, name, r)]
    return np.ascontiguousarray(np.concatenate(parts).astype(F))


def check_scene(name, cloud, r, queries=None):
    """what every test asserts of its scene before using it: the cell count at h0 lies in the scene's range, and no stray is within r of a
    blob point, a constructed point or a query.  Returns the (h, dims, doublings) the rule gives."""
    ns = 0 if EXTENTS[name] is None else sum(1 for e in EXTENTS[name] if e)
    h0 = cell(r)
    d = dims(cloud[:, :3], h0)
    cells = float(d[0]) * float(d[1]) * float(d[2])
    lo, hi = CELLS[name]
    assert lo < cells <= hi, (name, d, cells)
    if ns:
        rest = cloud[: len(cloud) - ns] if queries is None else np.concatenate([cloud[: len(cloud) - ns, :3], np.asarray(queries)[:, :3]])
        assert d2_f32(cloud[len(cloud) - ns:], rest).min() > 4 * F(r) * F(r), name
        if ns > 1:
            s = cloud[len(cloud) - ns:]
            dd = d2_f32(s, s) + np.eye(ns, dtype=F) * F(1e30)
            assert dd.min() > 4 * F(r) * F(r), name
    return rule(cloud[:, :3], h0)


def small_transform(thr):
    """half a degree about z and 0.3 thr of shift: 'the blob moved by a small known transform'"""
    a = np.deg2rad(0.5)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = 0.3 * thr * np.array([0.6, 0.0, 0.8])
    return T.astype(F)


def knn_numpy(q, pts, k):
    """the numpy statement of the exact k-NN: lexsort on (d2, index) -> (idx [m, k], d2 [m, k])"""
    d2 = d2_f32(q, pts)
    order = np.lexsort((np.broadcast_to(np.arange(d2.shape[1]), d2.shape), d2), axis=1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(d2, order, 1)


# ---- ring searches outside the cloud's box and on tiny clouds (the knn walk of orc_grid.h / lgr_grid.cuh) ------------------------------
RING_CELL_MAX = 1 << 29        # the walk's centre is held to +-2^29 cells (lgr_ring_cellc / orc::Grid::ring_cellc)
FAR_DISTANCES = (0.1, 1.0, 100.0, 1e5)


def knn_padded(q, pts, k):
    """knn_numpy with the slots a list cannot fill (k > n): index -1, d2 +inf"""
    idx, d2 = knn_numpy(q, pts, k)
    pad = k - idx.shape[1]
    if pad > 0:
        idx = np.concatenate([idx, np.full((len(idx), pad), -1, np.int32)], 1)
        d2 = np.concatenate([d2, np.full((len(d2), pad), np.inf, F)], 1)
    return idx, d2


def auto_cell(xyz, target, device=False):
    """the automatic cell of the k-NN grids restated in float32: sqrt(area * target / n) with area = the product of the two longest extents
    (at least 1e-12), at least 1/1024 of the longest extent and 1e-6.  orc::auto_cell (oracle) answers 1 for fewer than two points;
    lgr_grid_build (device=True) has no such case and arrives at sqrt(1e-12 * target)."""
    xyz = np.asarray(xyz, F)[:, :3]
    n = len(xyz)
    if n < 2 and not device:
        return F(1)
    e = np.sort((xyz.max(0) - xyz.min(0)).astype(F))
    area = max(F(e[2] * e[1]), F(1e-12))
    h = np.sqrt(F(F(area * F(target)) / F(max(n, 1))))
    return max(F(h), max(F(e[2] / F(1024)), F(1e-6)))


def grid_of(xyz, target, device=False):
    """(h, origin, dims) of the k-NN grid over xyz: the automatic cell, then the rule of DESIGN.md section 4"""
    xyz = np.asarray(xyz, F)[:, :3]
    h, d, _ = rule(xyz, auto_cell(xyz, target, device))
    return h, xyz.min(0), d


def outside_queries(b):
    """80 queries on and outside the box of b: for each of the 26 sign directions of {-1, 0, 1}^3 the box centre plus the direction times
    (half extent + delta), delta = 1e-4, 0.05 and 0.3 of the largest extent; then the box's min and max corners themselves"""
    mn, mx = b[:, :3].min(0).astype(np.float64), b[:, :3].max(0).astype(np.float64)
    c, half, ext = (mn + mx) / 2, (mx - mn) / 2, (mx - mn).max()
    dirs = [np.array((i, j, k), np.float64) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
    q = [point(c + d * (half + delta * ext)) for d in dirs for delta in (1e-4, 0.05, 0.3)]
    q += [point(b[:, :3].min(0)), point(b[:, :3].max(0))]
    return np.stack(q).astype(F)


def tiny_clouds():
    """name -> n x 12: one point, two coincident, two distinct, three collinear along x, five coplanar, 70 coincident plus one other"""
    p = (0.3, -0.2, 0.5)
    return dict(
        one=np.stack([point(p)]),
        two_same=np.stack([point(p), point(p)]),
        two=np.stack([point(p), point((0.31, -0.18, 0.505))]),
        line3=np.stack([point((0.1, 0.2, 0.3)), point((0.6, 0.2, 0.3)), point((1.4, 0.2, 0.3))]),
        plane5=np.stack([point((x, y, 0.25)) for x, y in ((0, 0), (1, 0), (0, 1), (1, 1), (0.4, 0.7))]),
        same70=np.stack([point(p)] * 70 + [point((0.35, -0.1, 0.52))]),
    )


def tiny_queries(cloud, h):
    """the cloud's own points, then its first and last point displaced along one, two and three axes, both ways, by 3 and by 200 cells h"""
    q = [cloud]
    for p in (cloud[0], cloud[-1]):
        for m in (3, 200):
            for axes in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1)):
                for sign in (1, -1):
                    q.append(point(p[:3].astype(np.float64) + sign * m * float(h) * np.array(axes, np.float64))[None])
    return np.concatenate(q).astype(F)


def far_queries(cloud):
    """the cloud's first point displaced by 0.1, 1, 100 and 1e5 along all three axes at once (both ways) and along each axis alone; at the
    one-point cloud's cell 1e5 is more than 2^31 cells"""
    p = cloud[0, :3].astype(np.float64)
    q = []
    for d in FAR_DISTANCES:
        for v in ((1, 1, 1), (-1, -1, -1), (1, 0, 0), (0, -1, 0), (0, 0, 1)):
            q.append(point(p + d * np.array(v, np.float64)))
    return np.stack(q).astype(F)


def ring_walk(q, pts, k, h, origin, dims):
    """What the ring walk may cost, from the grid and the query's cell alone.  Per query (first ring, last ring, in-grid cells of those rings):
      centre c = clip(floor(fl(fl(q - o) / h)), +-2^29) per axis                       (the walk's own float expression)
      first  = max over the axes of max(-c, c - (d - 1), 0)                             (Chebyshev gap between the centre and the cell box)
      last   = the first ring s >= first after which k candidates are held and the k-th d2 <= fl(fl(fl(s) h) 0.999)^2, at most
               max over the axes of max(c, d - 1 - c)                                   (the termination rule, restated)
      cells  = B(last) - B(first - 1),  B(s) = prod over the axes of |[c - s, c + s] & [0, d - 1]|
    A point is held after ring s when its (clamped) cell is at most s cells from c along every axis."""
    q, pts = np.asarray(q, F)[:, :3], np.asarray(pts, F)[:, :3]
    h, origin = F(h), np.asarray(origin, F)
    d = [int(x) for x in dims]
    pc = np.clip(np.floor((pts - origin) / h), 0, np.array(d, np.float64) - 1).astype(np.int64)
    cq = np.clip(np.floor((q - origin) / h), -RING_CELL_MAX, RING_CELL_MAX).astype(np.int64)
    d2 = d2_f32(q, pts)
    out = []
    for i in range(len(q)):
        c = [int(x) for x in cq[i]]
        first = max(max(-c[a], c[a] - (d[a] - 1), 0) for a in range(3))
        maxring = max(max(c[a], d[a] - 1 - c[a]) for a in range(3))
        last = maxring
        if k <= len(pts):
            ring = np.abs(pc - cq[i]).max(1)
            for s in range(first, maxring):
                held = d2[i][ring <= s]
                if len(held) >= k:
                    lim = F(F(F(s) * h) * F(0.999))
                    if np.partition(held, k - 1)[k - 1] <= F(lim * lim):
                        last = s
                        break

        def box(s):
            n = 1
            for a in range(3):
                n *= max(min(c[a] + s, d[a] - 1) - max(c[a] - s, 0) + 1, 0)
            return n
        out.append((first, last, box(last) - (box(first - 1) if first > 0 else 0)))
    return np.array(out, np.int64)
