"""Synthetic scan pairs (SURVEY.md section 8d / BASELINE.md): height-field + boxes scene, random SE(3), noise.

The reference ships no point clouds (its .gitignore excludes them), so every config runs on this generator.
numpy only -- this module is used by tests, bench.py and the oracle-side baseline alike.
"""
import numpy as np

SEED = 566  # SEED of include/common.h:25


def make_points(xyz, intensity=1.0):
    """n x 12 float32 in pcl::PointXYZINormal layout {x,y,z,1 | nx,ny,nz,0 | intensity,curvature,pad,pad}."""
    xyz = np.asarray(xyz, dtype=np.float32)
    p = np.zeros((xyz.shape[0], 12), dtype=np.float32)
    p[:, 0:3] = xyz
    p[:, 3] = 1.0
    p[:, 8] = intensity
    return p


class Scene:
    """z = sum_k A_k sin(a_k x + b_k y + phi_k) over [0, 24 s] x [0, 16 s] plus axis-aligned boxes resting on it."""

    def __init__(self, rng, scale=1.0, n_waves=12, n_boxes=40):
        self.scale = float(scale)
        self.lx, self.ly = 24.0 * self.scale, 16.0 * self.scale
        self.A = rng.uniform(0.05, 0.6, n_waves) * min(1.0, self.scale * 2.0)
        wl = rng.uniform(0.8, 6.0, n_waves) * min(1.0, max(self.scale, 0.25))
        ang = rng.uniform(0, 2 * np.pi, n_waves)
        self.a = 2 * np.pi / wl * np.cos(ang)
        self.b = 2 * np.pi / wl * np.sin(ang)
        self.phi = rng.uniform(0, 2 * np.pi, n_waves)
        nb = n_boxes
        size = rng.uniform(0.5, 2.0, (nb, 3)) * min(1.0, max(self.scale, 0.25))
        cx = rng.uniform(0, self.lx, nb)
        cy = rng.uniform(0, self.ly, nb)
        self.box = np.stack([cx - size[:, 0] / 2, cx + size[:, 0] / 2, cy - size[:, 1] / 2, cy + size[:, 1] / 2], 1)
        self.box_h = size[:, 2]

    def height(self, x, y):
        z = np.zeros_like(x)
        for k in range(len(self.A)):
            z += self.A[k] * np.sin(self.a[k] * x + self.b[k] * y + self.phi[k])
        for i in range(self.box.shape[0]):
            x0, x1, y0, y1 = self.box[i]
            inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
            if inside.any():
                base = 0.0
                for k in range(len(self.A)):
                    base += self.A[k] * np.sin(self.a[k] * 0.5 * (x0 + x1) + self.b[k] * 0.5 * (y0 + y1) + self.phi[k])
                z = np.where(inside, np.maximum(z, base + self.box_h[i]), z)
        return z

    def sample(self, rng, n, x_lo, x_hi):
        x = rng.uniform(x_lo * self.lx, x_hi * self.lx, n)
        y = rng.uniform(0, self.ly, n)
        return np.stack([x, y, self.height(x, y)], 1)


def random_se3(rng, t_range=5.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.uniform(-t_range, t_range, 3)
    return T


def make_pair(n_points=1_000_000, seed=SEED, noise=0.005, overlap=0.5, constant_density=True, yaw_only=False):
    """Returns dict(src, tgt [n x 12 float32], T_gt [4x4: maps src frame -> tgt frame], vp_src, vp_tgt).

    src covers x in [0, 2/3] of the scene, tgt covers [1/3, 1] (50 % overlap), both in the scene frame; tgt is then
    moved by a random rigid T (so T_gt = T).  With constant_density the scene shrinks with sqrt(n / 1e6) so the
    point density (and therefore the FPFH neighbourhood size at r = 0.25 m) is that of the 1M-point configuration.
    yaw_only: T's rotation is about the vertical (z) axis only, the motion of a levelled scanner (what gravity-aligned frames assume);
    the default output does not change.
    """
    rng = np.random.default_rng(seed)
    scale = np.sqrt(n_points / 1.0e6) if constant_density else 1.0
    scene = Scene(rng, scale)
    lo_t = (1.0 - overlap) * (2.0 / 3.0)
    src = scene.sample(rng, n_points, 0.0, 2.0 / 3.0)
    tgt = scene.sample(rng, n_points, lo_t, lo_t + 2.0 / 3.0)
    src += rng.normal(0, noise, src.shape)
    tgt += rng.normal(0, noise, tgt.shape)
    T = random_se3(rng)
    if yaw_only:
        a = rng.uniform(-np.pi, np.pi)
        T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    vp_scene = np.array([0.0, 0.0, 10.0])
    tgt_m = tgt @ T[:3, :3].T + T[:3, 3]
    vp_tgt = T[:3, :3] @ vp_scene + T[:3, 3]
    return dict(src=make_points(src), tgt=make_points(tgt_m), T_gt=T.astype(np.float64),
                vp_src=vp_scene.astype(np.float32), vp_tgt=vp_tgt.astype(np.float32), scale=scale)


class PlanarScene:
    """A man-made scene of PLANES -- the shape of the reference's real configs (data/tests.yaml: WHU-TLS SubwayStation / Residence / ..., kizhi, arch,
    office): a flat ground rectangle, `n_boxes` buildings (four walls and a roof each: 5 n_boxes + 1 rectangles), and a few Gaussian blobs of
    clutter ("vegetation").  plane_frac of the points lie exactly on rectangles (before noise), sampled uniformly in area."""

    def __init__(self, rng, scale=1.0, n_boxes=8, plane_frac=0.85):
        self.lx, self.ly = 16.0 * scale, 10.0 * scale
        self.plane_frac = plane_frac
        w = rng.uniform(1.5, 3.0, (n_boxes, 2)) * min(1.0, max(scale, 0.25))
        h = rng.uniform(1.5, 3.0, n_boxes) * min(1.0, max(scale, 0.25))
        cx = rng.uniform(0.1 * self.lx, 0.9 * self.lx, n_boxes)
        cy = rng.uniform(0.15 * self.ly, 0.85 * self.ly, n_boxes)
        rects = [(np.array([0.0, 0.0, 0.0]), np.array([self.lx, 0.0, 0.0]), np.array([0.0, self.ly, 0.0]))]   # origin, edge u, edge v
        for i in range(n_boxes):
            x0, x1, y0, y1 = cx[i] - w[i, 0] / 2, cx[i] + w[i, 0] / 2, cy[i] - w[i, 1] / 2, cy[i] + w[i, 1] / 2
            z = np.array([0.0, 0.0, h[i]])
            rects += [(np.array([x0, y0, 0.0]), np.array([x1 - x0, 0.0, 0.0]), z), (np.array([x0, y1, 0.0]), np.array([x1 - x0, 0.0, 0.0]), z),
                      (np.array([x0, y0, 0.0]), np.array([0.0, y1 - y0, 0.0]), z), (np.array([x1, y0, 0.0]), np.array([0.0, y1 - y0, 0.0]), z),
                      (np.array([x0, y0, h[i]]), np.array([x1 - x0, 0.0, 0.0]), np.array([0.0, y1 - y0, 0.0]))]
        self.rects = rects
        self.area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in rects])
        self.blob_c = np.stack([rng.uniform(0, self.lx, 12), rng.uniform(0, self.ly, 12), rng.uniform(0.3, 1.5, 12)], 1)
        self.blob_s = rng.uniform(0.15, 0.5, 12) * min(1.0, max(scale, 0.25))

    def n_planes(self):
        return len(self.rects)

    def sample(self, rng, n, x_lo, x_hi):
        out = np.empty((0, 3))
        lo, hi = x_lo * self.lx, x_hi * self.lx
        while out.shape[0] < n:
            m = int((n - out.shape[0]) * 1.8) + 1024
            on_plane = rng.uniform(size=m) < self.plane_frac
            r = rng.choice(len(self.rects), m, p=self.area / self.area.sum())
            O = np.stack([self.rects[k][0] for k in range(len(self.rects))])[r]
            U = np.stack([self.rects[k][1] for k in range(len(self.rects))])[r]
            V = np.stack([self.rects[k][2] for k in range(len(self.rects))])[r]
            p = O + U * rng.uniform(size=(m, 1)) + V * rng.uniform(size=(m, 1))
            b = rng.integers(0, len(self.blob_s), m)
            q = self.blob_c[b] + rng.normal(size=(m, 3)) * self.blob_s[b, None]
            q[:, 2] = np.abs(q[:, 2])
            p = np.where(on_plane[:, None], p, q)
            p = p[(p[:, 0] >= lo) & (p[:, 0] <= hi)]
            out = np.concatenate([out, p])
        return out[:n]


def make_planar_pair(n_points=1_000_000, seed=SEED, noise=0.005, overlap=0.5, plane_frac=0.85, n_boxes=8):
    """make_pair's layout on a PlanarScene: >= 70 % of the points on >= 20 planes; returns the same dict + n_planes, plane_frac"""
    rng = np.random.default_rng(seed)
    scale = np.sqrt(n_points / 1.0e6)
    scene = PlanarScene(rng, scale, n_boxes=n_boxes, plane_frac=plane_frac)
    lo_t = (1.0 - overlap) * (2.0 / 3.0)
    src = scene.sample(rng, n_points, 0.0, 2.0 / 3.0)
    tgt = scene.sample(rng, n_points, lo_t, lo_t + 2.0 / 3.0)
    src += rng.normal(0, noise, src.shape)
    tgt += rng.normal(0, noise, tgt.shape)
    T = random_se3(rng)
    vp_scene = np.array([0.5 * scene.lx, 0.5 * scene.ly, 10.0])
    tgt_m = tgt @ T[:3, :3].T + T[:3, 3]
    vp_tgt = T[:3, :3] @ vp_scene + T[:3, 3]
    return dict(src=make_points(src), tgt=make_points(tgt_m), T_gt=T.astype(np.float64), vp_src=vp_scene.astype(np.float32), vp_tgt=vp_tgt.astype(np.float32),
                scale=scale, n_planes=scene.n_planes(), plane_frac=plane_frac)


def make_correspondence_problem(n_pts=20000, c=5000, inlier_frac=0.4, sigma=0.01, thr=0.05, seed=SEED, extent=10.0):
    """Directly synthesised correspondences for RANSAC stress (BASELINE config 4):
    inlier_frac of the c correspondences are true (t = T s + N(0, sigma)), the rest point at random targets."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-extent, extent, (n_pts, 3))
    src[:, 2] *= 0.2
    T = random_se3(rng)
    tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, sigma, src.shape)
    perm = rng.permutation(n_pts)[:c]
    match = perm.copy()
    n_out = c - int(round(inlier_frac * c))
    out_idx = rng.permutation(c)[:n_out]
    match[out_idx] = rng.integers(0, n_pts, n_out)
    corr = np.zeros(c, dtype=[("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4"), ("threshold", "<f4")])
    corr["index_query"] = perm
    corr["index_match"] = match
    corr["distance"] = rng.uniform(0, 50, c).astype(np.float32)
    corr["threshold"] = thr
    return dict(src=make_points(src), tgt=make_points(tgt), corr=corr, T_gt=T)


def make_two_mode_problem(n_pts=4000, c=1500, f1=0.30, f2=0.18, sigma=0.01, thr=0.05, seed=11, extent=10.0):
    """Correspondences with TWO plausible poses (the scenes the set of distinct hypotheses is for): the target holds the source under T1
    and, behind it, under T2; a fraction f1 of the c correspondences follows T1, f2 follows T2, the rest point at random targets."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-extent, extent, (n_pts, 3))
    src[:, 2] *= 0.2
    T1, T2 = random_se3(rng), random_se3(rng)
    tgt = np.concatenate([src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, sigma, src.shape) for T in (T1, T2)])
    perm = rng.permutation(n_pts)[:c]
    match = rng.integers(0, 2 * n_pts, c)
    order = rng.permutation(c)
    n1, n2 = int(round(f1 * c)), int(round(f2 * c))
    match[order[:n1]] = perm[order[:n1]]
    match[order[n1:n1 + n2]] = perm[order[n1:n1 + n2]] + n_pts
    corr = np.zeros(c, dtype=[("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4"), ("threshold", "<f4")])
    corr["index_query"] = perm
    corr["index_match"] = match
    corr["distance"] = rng.uniform(0, 50, c).astype(np.float32)
    corr["threshold"] = thr
    return dict(src=make_points(src), tgt=make_points(tgt), corr=corr, T1=T1, T2=T2)


def make_pose_list(n=3000, k=12, seed=1):
    """A list of n (transform, metric) items for the fold of updateHypotheses alone: poses scattered around k centres (rotations up to
    25 degrees, translations up to 15 x 0.05 away: on both sides of the similarity thresholds at distance_thr = 0.05), metrics that tie,
    fall below the 0.1 x best floor and keep producing new bests.  Returns (tns [n, 16] float32 column-major, metrics [n] float32)."""
    rng = np.random.default_rng(seed)
    centres = [random_se3(rng) for _ in range(k)]
    tns = np.zeros((n, 16), np.float32)
    metrics = np.zeros(n, np.float32)
    for i in range(n):
        T = centres[int(rng.integers(0, k))].copy()
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad(rng.uniform(0, 25))
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        dR = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        T[:3, :3] = dR @ T[:3, :3]
        T[:3, 3] = T[:3, 3] + rng.normal(size=3) * 0.05 * rng.uniform(0, 15)
        m = [rng.uniform(0, 1), round(rng.uniform(0, 1), 1), rng.uniform(0, 0.05)][int(rng.integers(0, 3))]
        tns[i] = T.astype(np.float32).T.reshape(16)
        metrics[i] = np.float32(m * (0.2 + 0.8 * i / n))
    return tns, metrics


# tests/point2plane_distance.cpp:29-58 of the reference: its ground-truth transform and corner scene
CORNER_GT = np.array([[0.0803703, -0.996763, -0.00201846, 1.2143], [0.996758, 0.080377, -0.00349969, -6.13404],
                      [0.00365057, -0.00173067, 0.999992, -1.17221], [0, 0, 0, 1]], np.float32)


def make_corner_scene(n=100, shift=5):
    """The reference's end-to-end scene: three orthogonal n x n lattices (spacing 2), the target shifted by 1 in-plane, the source moved
    by CORNER_GT^-1 (emplace_back order of :33-40).  Returns (src, tgt, vp_src, vp_tgt); normals are left to the caller (:66-67)."""
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    i, j = ij[:, 0], ij[:, 1]
    z = np.zeros_like(i)
    s = np.stack([np.stack([2 * i, 2 * j, z], 1), np.stack([shift + 2 * i, z, shift + 2 * j], 1),
                  np.stack([z, 2 * shift + 2 * i, 2 * shift + 2 * j], 1)], 1).reshape(-1, 3)
    t = np.stack([np.stack([2 * i + 1, 2 * j, z], 1), np.stack([shift + 2 * i, z, shift + 2 * j + 1], 1),
                  np.stack([z, 2 * shift + 2 * i + 1, 2 * shift + 2 * j], 1)], 1).reshape(-1, 3)
    gi = np.linalg.inv(CORNER_GT).astype(np.float64)
    src = make_points((s @ gi[:3, :3].T + gi[:3, 3]).astype(np.float32))
    tgt = make_points(t.astype(np.float32))
    vp_tgt = np.full(3, 2.0 * n, np.float32)
    vp_src = (CORNER_GT[:3, :3].T.astype(np.float64) @ (vp_tgt - CORNER_GT[:3, 3]).astype(np.float64)).astype(np.float32)
    return src, tgt, vp_src, vp_tgt


# ---- fixtures of the multi-scale correspondence search (feature_radius unset; tests/test_multiscale_ref.py)
def make_two_density_pair(n=6000, seed=31, keep=0.3, n_islands=8, island=6, lift=0.3):
    """make_pair whose far half (x above the median) keeps only `keep` of its points: the key points fall on two radius levels.
    Plus `n_islands` islands of `island` points within a centimetre, `lift` above the surface: their key points sit on the finest
    level, where the down-sampled surface leaves them fewer than 5 neighbours (a NaN SHOT row), while the coarser radii reach the
    surface."""
    a = make_pair(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    out = dict(a)
    for name in ("src", "tgt"):
        pts = a[name]
        x = pts[:, 0]
        sel = (x <= np.median(x)) | (rng.random(len(pts)) < keep)
        pts = pts[sel]
        up = np.array([0.0, 0.0, lift]) if name == "src" else a["T_gt"][:3, :3] @ np.array([0.0, 0.0, lift])
        c = pts[rng.choice(len(pts), n_islands, replace=False), :3].astype(np.float64) + up
        isl = (c[:, None, :] + rng.uniform(-0.005, 0.005, (n_islands, island, 3))).reshape(-1, 3)
        out[name] = np.ascontiguousarray(np.concatenate([pts, make_points(isl)]))
    return out


def make_pruned_pair(n=6000, seed=32, blob=120, blob_sigma=0.002, n_outliers=3, outlier_lift=5.0):
    """make_pair plus, per cloud, a tight Gaussian blob of `blob` points on the surface (radius levels far below the bulk, fewer than
    10 % of the largest level: pruned, clamped up) and `n_outliers` isolated points `outlier_lift` above it (levels far above, under
    0.1 %: pruned, clamped down)"""
    a = make_pair(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    out = dict(a)
    for name in ("src", "tgt"):
        pts = a[name]
        c = pts[rng.integers(len(pts)), :3].astype(np.float64)
        b = c + rng.normal(0, blob_sigma, (blob, 3))
        lo, hi = pts[:, :3].min(0), pts[:, :3].max(0)
        o = np.stack([rng.uniform(lo[0], hi[0], n_outliers), rng.uniform(lo[1], hi[1], n_outliers),
                      np.full(n_outliers, hi[2] + outlier_lift)], 1) + rng.normal(0, 1.0, (n_outliers, 3))
        out[name] = np.ascontiguousarray(np.concatenate([pts, make_points(b), make_points(o)]))
    return out


def make_disjoint_levels_pair(n=6000, seed=33):
    """source at the 1M configuration's density, target spread over the full-size scene (about 80 times sparser): their radius levels
    have no level in common"""
    return dict(make_pair(n, seed=seed), tgt=make_pair(n, seed=seed, constant_density=False)["tgt"])


def make_duplicates_pair(n=6000, seed=34, n_dup=400):
    """make_pair with `n_dup` points of each cloud appended a second time (equal positions, so equal rows on every level): the
    matcher's block tie rule and the vote's count ties.  Also returns the (original, copy) index pairs."""
    a = make_pair(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    out = dict(a)
    for name in ("src", "tgt"):
        pts = a[name]
        pick = np.sort(rng.choice(len(pts), n_dup, replace=False))
        out[name] = np.ascontiguousarray(np.concatenate([pts, pts[pick]]))
        out["dup_" + name] = np.stack([pick, len(pts) + np.arange(n_dup)], 1)
    return out


def make_lattice_pair(n_coarse=24, n_fine=48, spacing=1.0 / 16):
    """two exact square lattices in the plane z = 0, an n_coarse^2 one of twice the spacing and an n_fine^2 one beside it, and the
    target equal to the source.  Coordinates are small multiples of a power of two, so interior points of one lattice have
    bit-identical rows: a query ties at distance 0 with several train key points on every level, the block rule picks a different one
    per level (the level lists differ), and with a vote window below the spacing the vote meets equal counts at equal distances."""
    coarse = np.stack(np.meshgrid(np.arange(n_coarse), np.arange(n_coarse), indexing="ij"), -1).reshape(-1, 2) * (2 * spacing)
    fine = np.stack(np.meshgrid(np.arange(n_fine), np.arange(n_fine), indexing="ij"), -1).reshape(-1, 2) * spacing
    fine = fine + np.array([2 * spacing * n_coarse + 1.0, 0.0])
    xy = np.concatenate([coarse, fine])
    pts = make_points(np.concatenate([xy, np.zeros((len(xy), 1))], 1))
    vp = np.array([1.0, 1.0, 5.0], np.float32)
    return dict(src=pts, tgt=pts.copy(), T_gt=np.eye(4), vp_src=vp, vp_tgt=vp.copy())
