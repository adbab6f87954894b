"""An independent statement of the rigid fit (float64 Kabsch on numpy's SVD) and the input families the fits are pinned on
(tests/test_fit_ref.py on the CPU, tests/test_gpu_fit_edges.py on the device).  numpy only.

The three fits of the library (umeyama_n, refit_kernel, gror_umeyama_kernel) and their statements in the oracle share one 3x3 SVD that
is restated op for op, so device == oracle cannot see a flaw both carry.  kabsch() shares nothing with either."""
import numpy as np

from lgr_amd import synthetic

F = np.float32
FAMILIES = ("generic", "generic_noise", "coplanar", "coplanar_noise", "collinear", "coincident", "mirror", "rot180", "cube",
            "scale_1e-4", "scale_1e-6", "offset_1e3", "offset_1e5", "sliver")
SIGMA = 0.01   # of the *_noise families, added to the target


def xyz(pts):
    return np.asarray(pts, np.float64)[:, :3]


def _svd_fit(P, Q):
    P, Q = xyz(P), xyz(Q)
    pm, qm = P.mean(0), Q.mean(0)
    U, S, Vt = np.linalg.svd((Q - qm).T @ (P - pm))
    d = np.linalg.det(U @ Vt)
    R = U @ np.diag([1.0, 1.0, -1.0 if d < 0 else 1.0]) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = qm - R @ pm
    return T, S, d


def kabsch(P, Q):
    """the proper rotation and translation that take P onto Q with the least sum of squares, in float64 -> (T 4x4, singular values of the
    covariance (Q - mean)^T (P - mean)).  T is unique when S[1] + S[2] > 0 without the sign flip and when S[1] - S[2] > 0 with it."""
    T, S, _ = _svd_fit(P, Q)
    return T, S


def kabsch_det(P, Q):
    """det(U V^T) of the float64 fit: negative when the fit had to take its sign flip"""
    return _svd_fit(P, Q)[2]


def rms(T, P, Q):
    P, Q, T = xyz(P), xyz(Q), np.asarray(T, np.float64)
    r = Q - (P @ T[:3, :3].T + T[:3, 3])
    return float(np.sqrt((r * r).sum(1).mean()))


def same_bits(a, b):
    """NaN in the same places (the payload of a NaN belongs to the platform), equal uint32 words everywhere else"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def case_seed(name, n):
    """one fixed seed per (family, size)"""
    return 7919 * (FAMILIES.index(name) + 1) + n


def _rot180(rng):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    return 2.0 * np.outer(a, a) - np.eye(3)


def family(name, n, seed):
    """(src, tgt) as [n, 12] float32 point arrays and the exact 4x4 the target was made with (tgt = T src, then rounded to float32;
    for mirror, T applied to the source reflected in z).  Coordinates are of order 1 unless the name says otherwise.
    cube: n = 8 only; an even seed leaves the cube where it is, an odd one moves it.
    sliver: 1 x 0.03 x 0.03, the second and third singular values of its covariance near 1e-3 of the first."""
    assert name in FAMILIES, name
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, 3))
    T = synthetic.random_se3(rng, t_range=2.0)
    noise = rng.normal(0.0, SIGMA, (n, 3))      # drawn for every family so that a family and its _noise twin share X and T
    scale = 1.0
    if name.startswith("coplanar"):
        X[:, 2] = 0.0
    elif name == "collinear":
        d = rng.normal(size=3)
        X = np.outer(X[:, 0], d / np.linalg.norm(d)) + rng.uniform(-1.0, 1.0, 3)
    elif name == "coincident":
        X = np.repeat(X[:1], n, 0)
    elif name == "rot180":
        T[:3, :3] = _rot180(rng)
    elif name == "cube":
        assert n == 8
        X = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
        if seed % 2 == 0:
            T = np.eye(4)
    elif name.startswith("scale_"):
        scale = float(name[6:])
    elif name.startswith("offset_"):
        X = X + float(name[7:])
    elif name == "sliver":
        X[:, 1:] *= 0.03
    Y = X * np.array([1.0, 1.0, -1.0]) if name == "mirror" else X
    Y = Y @ T[:3, :3].T + T[:3, 3]
    if name.endswith("_noise"):
        Y = Y + noise
    T = T.copy()
    T[:3, 3] *= scale
    return synthetic.make_points(X * scale), synthetic.make_points(Y * scale), T


def identity_corr(dtype, n):
    """correspondence i -> i with the fields of either CORR_DTYPE (the oracle's or the library's)"""
    corr = np.zeros(n, dtype)
    corr[dtype.names[0]] = np.arange(n)
    corr[dtype.names[1]] = np.arange(n)
    corr["threshold"] = 0.05
    return corr
