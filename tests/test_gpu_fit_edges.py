"""GPU parity: the three rigid fits (umeyama_n through lgr_ransac_replay_dev, refit_kernel through lgr_refit_svd_dev / lgr_refit_svd,
gror_umeyama_kernel through lgr_gror_dev) against the oracle, bit for bit, where the well-conditioned problems of the other modules
never go: inlier counts on both sides of every staging-chunk boundary (256 threads; 1024 pairs per chunk of the refit's second pass and
of GROR's Umeyama; 2048 of the refit's first pass; the first chunk of a third round), empty sets and sets of 1 and 2 pairs, and every
input family of tests/fit_ref_lib.py: collinear and coincident samples (the rank-deficient completions of lgr_svd3), mirrored pairs
(the sign flip of both Umeyamas, the column negation of the refit), equal singular values, coordinates of 1e-4 and 1e-6 (the skip
rule's products below f32's normal range; the power-of-two scaling of lgr_svd3) and of 1e3 and 1e5.

tests/test_fit_ref.py holds the oracle's side of these inputs against float64.  NaN compares by position (same_bits)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_ref_lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4097)
N_ROWS = 4200


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def lib_corr(n):
    from lgr_amd import capi
    return L.identity_corr(capi.CORR_DTYPE, n)


def orc_corr(oracle, corr):
    out = np.zeros(corr.shape[0], oracle.CORR_DTYPE)
    out["query"] = corr["index_query"]; out["match"] = corr["index_match"]
    out["distance"] = corr["distance"]; out["threshold"] = corr["threshold"]
    return out


def refit_dev(lgr, src, tgt, corr, mask):
    """lgr_refit_svd_dev -> (return code, 4x4)"""
    from lgr_amd import capi
    d_corr = lgr._corr_dev(corr)
    T = (C.c_float * 16)()
    rc = capi.lib().lgr_refit_svd_dev(lgr.h, capi._ptr(src), capi._ptr(tgt), capi._ptr(d_corr), corr.shape[0], capi._ptr(mask), T)
    return rc, np.array(T, np.float32).reshape(4, 4).T.copy()


def refit_host(lgr, src, tgt, corr):
    """lgr_refit_svd on host arrays -> (return code, 4x4)"""
    from lgr_amd import capi
    corr = np.ascontiguousarray(corr)
    T = (C.c_float * 16)()
    rc = capi.lib().lgr_refit_svd(lgr.h, vp(src), vp(tgt), src.shape[0], tgt.shape[0], vp(corr), len(corr), T)
    return rc, np.array(T, np.float32).reshape(4, 4).T.copy()


@pytest.fixture(scope="module")
def rows():
    src, tgt, _ = L.family("generic_noise", N_ROWS, L.case_seed("generic_noise", N_ROWS))
    return dict(src=src, tgt=tgt, d_src=cuda(src), d_tgt=cuda(tgt))


@pytest.mark.parametrize("m", COUNTS)
def test_refit_counts(lgr, oracle, rows, m):
    from lgr_amd import capi
    src, tgt = rows["src"], rows["tgt"]
    corr = lib_corr(N_ROWS)
    ocorr = orc_corr(oracle, corr)
    # (a) m ones spread over the 4200 rows; a masked-out row's points are NaN (source) and inf (target): read into a sum they would show
    mask = np.zeros(N_ROWS, np.uint8)
    mask[(np.arange(m) * N_ROWS) // max(m, 1)] = 1
    assert int(mask.sum()) == m
    psrc, ptgt = src.copy(), tgt.copy()
    psrc[mask == 0, :3] = np.nan
    ptgt[mask == 0, :3] = np.inf
    want_a = oracle.refit(psrc, ptgt, ocorr, mask)
    keep = np.flatnonzero(mask)
    assert L.same_bits(want_a, oracle.refit(src[keep], tgt[keep], ocorr[:m], np.ones(m, np.uint8)))   # the oracle skipped them too
    # (b), (c): no mask, the first m correspondences
    want_b = oracle.refit(src, tgt, ocorr[:m], np.ones(m, np.uint8))
    if m == 0:
        assert np.isnan(want_a).all() and np.isnan(want_b).all()   # sixteen NaNs
    else:
        assert np.isfinite(want_a).all() and np.isfinite(want_b).all()
    runs = (("mask", refit_dev(lgr, cuda(psrc), cuda(ptgt), corr, cuda(mask)), want_a),
            ("no mask", refit_dev(lgr, rows["d_src"], rows["d_tgt"], corr[:m], None), want_b),
            ("host entry", refit_host(lgr, src, tgt, corr[:m]), want_b))
    for name, (rc, T), want in runs:
        if m == 0 and rc != 0:
            assert rc == capi.ERR_INVALID_ARG, (name, rc)   # an entry that refuses an empty set
            continue
        assert rc == 0, (name, rc)
        assert L.same_bits(T, want), (name, m, T, want)


def family_cases():
    out = []
    for name in L.FAMILIES:
        out += [(name, 8, 0), (name, 8, 1)] if name == "cube" else [(name, n, L.case_seed(name, n)) for n in (3, 100, 2049)]
    return out


@pytest.mark.parametrize("name,n,seed", family_cases())
def test_refit_families(lgr, oracle, name, n, seed):
    src, tgt, _ = L.family(name, n, seed)
    corr = lib_corr(n)
    want = oracle.refit(src, tgt, orc_corr(oracle, corr), np.ones(n, np.uint8))
    d_src, d_tgt = cuda(src), cuda(tgt)
    assert L.same_bits(lgr.refit(d_src, d_tgt, corr), want), (name, n)
    assert L.same_bits(lgr.refit(d_src, d_tgt, corr, cuda(np.ones(n, np.uint8))), want), (name, n)


def hypothesis_cloud(ns):
    """the families side by side, one block of ns points each -> (src, tgt, {family: first row})"""
    names = ["generic", "collinear", "mirror", "rot180", "scale_1e-4", "scale_1e-6", "offset_1e3", "coincident", "sliver"]
    if ns >= 4:
        names.append("coplanar")
    S, T, first = [], [], {}
    for name in names:
        s, t, _ = L.family(name, ns, L.case_seed(name, ns))
        first[name] = sum(len(x) for x in S)
        S.append(s); T.append(t)
    if ns == 8:
        for seed in (0, 1):
            s, t, _ = L.family("cube", 8, seed)
            first["cube%d" % seed] = sum(len(x) for x in S)
            S.append(s); T.append(t)
    return np.concatenate(S), np.concatenate(T), first


@pytest.mark.parametrize("ns", (3, 4, 6, 8))
def test_hypothesis_fits(lgr, oracle, ns):
    from lgr_amd import capi
    src, tgt, first = hypothesis_cloud(ns)
    c = src.shape[0]
    corr = lib_corr(c)
    ocorr = orc_corr(oracle, corr)
    names = list(first)
    tup = np.array([np.arange(first[k], first[k] + ns) for k in names], np.int32)
    rep = tup[0].copy()
    rep[-1] = rep[0]                                      # a repeated index: the closing edge has length 0 on both sides, 0/0
    tup = np.concatenate([tup, rep[None]])
    pad = lgr.ransac_samples(566, 0, 257 - len(tup), c, n_samples=ns).cpu().numpy()
    tup = np.ascontiguousarray(np.concatenate([tup, pad]), np.int32)
    assert tup.shape == (257, ns)                         # more than four waves of 64
    d_src, d_tgt = cuda(src), cuda(tgt)
    for metric in (0, 1):
        p_o = oracle.default_params(rng_mode=oracle.RNG_PHILOX, metric_id=metric, score_id=2, n_samples=ns)
        p_g = capi.default_params(metric_id=metric, score_id=2, n_samples=ns)
        ok, Ts, ninl, met = lgr.ransac_replay(d_src, d_tgt, corr, p_g, cuda(tup))
        ook, oTs, oninl, omet = oracle.replay(src, tgt, ocorr, p_o, tup)
        np.testing.assert_array_equal(ok, ook)
        for k, name in enumerate(names):
            # exact copies keep their edge lengths: every family's tuple passes the polygon test, coincident points (0/0) apart
            assert ok[k] == (0 if name == "coincident" else 1), (ns, name)
            assert L.same_bits(Ts[k], oTs[k]), (ns, name, Ts[k], oTs[k])
        k = len(names)
        assert ok[k] == 0 and np.array_equal(Ts[k].reshape(4, 4), np.eye(4, dtype=np.float32))
        assert L.same_bits(Ts, oTs)
        np.testing.assert_array_equal(ninl, oninl)
        assert L.same_bits(met, omet)


GROR_RES = 0.05


def gror_problem(m, seed):
    """c = m + 300 correspondences i -> i: m of them, scattered over the rows, have tgt = src + a jitter shorter than res / 2; every
    other target is moved by 20 to 4000 res in a direction of its own (far and unevenly, so that no four of them keep their mutual
    distances by accident and the edge stage finds no set of its own).  Under any transform that stays within 1.5 res of the identity
    over the cloud, the refinement's inliers (|tgt - G src| < 2 res) are those m pairs."""
    rng = np.random.default_rng(seed)
    c = m + 300
    X = rng.uniform(-3.0, 3.0, (c, 3))
    d = rng.normal(size=(c, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = X + d * rng.uniform(20 * GROR_RES, 4000 * GROR_RES, (c, 1))
    true = np.sort(rng.permutation(c)[:m])
    j = rng.normal(size=(m, 3))
    j /= np.linalg.norm(j, axis=1, keepdims=True)
    Y[true] = X[true] + j * rng.uniform(0.0, 0.45 * GROR_RES, (m, 1))
    from lgr_amd import synthetic
    mask = np.zeros(c, np.uint8)
    mask[true] = 1
    return synthetic.make_points(X), synthetic.make_points(Y), mask


@pytest.mark.parametrize("m", (0, 1, 2, 3, 1023, 1024, 1025, 2049))
def test_gror_refine_counts(lgr, oracle, m):
    src, tgt, want_mask = gror_problem(m, 500 + m)
    c = m + 300                                           # on both sides of k_optimal = 800
    corr = lib_corr(c)
    T_o, d = oracle.gror(src, tgt, orc_corr(oracle, corr), GROR_RES, 800)
    assert d["n_inliers"] == m and d["K"] == min(c, 800)  # a condition on the input: checked on the CPU
    res, mask = lgr.gror(cuda(src), cuda(tgt), corr, GROR_RES)
    assert res.n_inliers == m
    np.testing.assert_array_equal(mask, want_mask)
    assert int(res.metric) == d["best_count"] and res.best_iteration == d["tcfs_rows"] and res.estimated_iters == d["K"]
    assert L.same_bits(res.matrix(), T_o), (m, res.matrix(), T_o)
    if m == 0:
        assert np.isnan(T_o[:3]).all()                    # the 1/0 mean: 0 * inf in every sum
