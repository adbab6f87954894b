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
