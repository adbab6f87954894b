"""GPU parity: lgr_teaser_dev against the CPU statement of the TEASER alignment (tests/cpp/teaser_ref.cpp).

Bar: bit-identical -- the transform's bits, the clique, the node list, the inlier mask and every lgr_teaser_info / lgr_result field.  Both
sides run the arithmetic of lgr_teaser_math.h in the stated order, so there is no tolerance to choose."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import teaser_ref_lib as tr  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def problem(c, frac, seed, n_pts=None, sigma=0.01):
    from lgr_amd import synthetic
    return synthetic.make_correspondence_problem(n_pts=n_pts or max(400, c + c // 4), c=c, inlier_frac=frac, seed=seed, sigma=sigma)


def params(beta, **kw):
    from lgr_amd import capi
    return capi.default_teaser_params(beta, **kw)


def run_both(ctx, pr, beta, k_select=0, **kw):
    p = params(beta, k_select=k_select, **kw)
    dev = ctx.teaser(cuda(pr["src"]), cuda(pr["tgt"]), pr["corr"], p)
    ref = tr.teaser(pr["src"], pr["tgt"], pr["corr"], beta, k_select, p.rotation_max_iterations, p.rotation_gnc_factor, p.rotation_cost_threshold)
    return dev, ref


def assert_same(dev, ref, c):
    res, info, clique, nodes, mask = dev
    assert ref["rc"] == 0
    for k in tr.INFO_INT:
        assert getattr(info, k) == ref[k], k
    assert np.array_equal(clique, ref["clique"])
    assert np.array_equal(nodes, ref["nodes"])
    assert np.array_equal(mask, ref["mask"])
    assert np.array_equal(tr.bits(res.matrix()), tr.bits(ref["T"])), np.abs(res.matrix() - ref["T"]).max()
    assert tr.bits(np.float32(info.rotation_cost)) == tr.bits(ref["rotation_cost"])
    assert np.array_equal(tr.bits(np.array(info.translation_cost, np.float32)), tr.bits(ref["translation_cost"]))
    assert list(info.reserved) == [0, 0, 0, 0]
    assert res.iterations == ref["rotation_iterations"] and res.converged == ref["valid"] and res.n_inliers == ref["n_inliers"]
    assert res.metric == ref["n_clique"] and res.best_iteration == ref["max_core"]
    assert res.estimated_iters == ref["n_nodes"] and res.n_correspondences == c


# c, inlier_frac, k_select, beta, sigma: 3 = the smallest solvable input; 64 / 65 = the word boundary of a bit row; 2500 with 256 = the
# selection cuts; 2100 with 2048 = the LDS maximum (32 words per row, 2 nodes per thread); beta = 0.02 at sigma = 0.01 = residuals above
# e2 / 2, so the GNC loop goes past its first solve (asserted below)
CASES = [(3, 1.0, 0, 0.05, 0.01), (64, 0.5, 0, 0.05, 0.01), (65, 0.5, 0, 0.05, 0.01), (300, 0.4, 0, 0.05, 0.01), (300, 0.4, 0, 0.02, 0.01),
         (2500, 0.4, 256, 0.05, 0.01), (2100, 0.4, 2048, 0.05, 0.01), (1500, 0.4, 0, 0.03, 0.01)]


@pytest.mark.parametrize("c,frac,k_select,beta,sigma", CASES)
def test_matches_statement(lgr, c, frac, k_select, beta, sigma):
    pr = problem(c, frac, 100 + c, sigma=sigma)
    dev, ref = run_both(lgr, pr, beta, k_select)
    assert_same(dev, ref, c)
    assert ref["valid"] == 1 and ref["n_nodes"] == min(c, k_select or 1024)
    if beta < 0.05:
        assert ref["rotation_iterations"] > 1
    if c >= 300:   # the ground truth is recovered
        T = dev[0].matrix()
        assert np.abs(T[:3, :3] - pr["T_gt"][:3, :3]).max() < 5e-3 and np.abs(T[:3, 3] - pr["T_gt"][:3, 3]).max() < beta


def test_no_inliers(lgr):
    """inlier_frac = 0: whatever the random graph's maximum core and greedy clique are, both sides agree on them"""
    pr = problem(300, 0.0, 77)
    dev, ref = run_both(lgr, pr, 0.05)
    assert_same(dev, ref, 300)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_fewer_than_three(lgr, c):
    pr = problem(300, 0.4, 5)
    pr["corr"] = pr["corr"][:c]
    dev, ref = run_both(lgr, pr, 0.05)
    assert_same(dev, ref, c)
    res, info, clique, nodes, mask = dev
    assert info.valid == 0 and res.converged == 0 and np.array_equal(res.matrix(), np.eye(4, dtype=np.float32))
    assert len(clique) == 0 and not mask.any()


def test_nan_source_row(lgr):
    """a node with a NaN coordinate is isolated: degree 0, ranked last, in no clique and not in the mask"""
    pr = problem(300, 0.4, 9)
    truth = np.flatnonzero(pr["corr"]["index_query"] == pr["corr"]["index_match"])
    victim = int(truth[3])
    pr["src"][pr["corr"]["index_query"][victim], :3] = np.nan
    dev, ref = run_both(lgr, pr, 0.05)
    assert_same(dev, ref, 300)
    res, info, clique, nodes, mask = dev
    assert info.valid == 1 and victim not in clique.tolist() and mask[victim] == 0 and np.isfinite(res.matrix()).all()


def test_device_against_host_twin(lgr):
    pr = problem(700, 0.3, 13)
    p = params(0.05)
    d = lgr.teaser(cuda(pr["src"]), cuda(pr["tgt"]), pr["corr"], p)
    h = lgr.teaser_host(pr["src"], pr["tgt"], pr["corr"], p)
    assert np.array_equal(tr.bits(d[0].matrix()), tr.bits(h[0].matrix()))
    assert bytes(d[1]) == bytes(h[1])
    for a, b in zip(d[2:], h[2:]):
        assert np.array_equal(a, b)
    assert d[0].n_inliers == h[0].n_inliers == int(h[4].sum()) and d[1].valid == 1


def test_argument_codes(lgr):
    from lgr_amd import capi
    pr = problem(300, 0.4, 21)
    s, t = cuda(pr["src"]), cuda(pr["tgt"])

    def rc(p, corr=pr["corr"]):
        cd = lgr._corr_dev(corr)
        res, info = capi.Result(), capi.TeaserInfo()
        return capi._lib.lgr_teaser_dev(lgr.h, capi._ptr(s), s.shape[0], capi._ptr(t), t.shape[0], capi._ptr(cd), cd.shape[0],
                                        C.byref(p) if p is not None else None, C.byref(res), C.byref(info), None, None)

    assert rc(params(0.05)) == 0   # the clique and mask outputs are optional
    assert rc(None) == INVALID_ARG
    for beta in (0.0, -1.0, float("nan"), float("inf"), 2e18):
        assert rc(params(beta)) == INVALID_ARG
    assert rc(params(1e18)) == 0
    for it in (0, -1, 1001):
        assert rc(params(0.05, rotation_max_iterations=it)) == INVALID_ARG
    assert rc(params(0.05, rotation_max_iterations=1)) == 0 and rc(params(0.05, rotation_max_iterations=1000)) == 0
    for g in (1.0, 0.5, float("nan"), float("inf")):
        assert rc(params(0.05, rotation_gnc_factor=g)) == INVALID_ARG
    for th in (-1e-3, float("nan"), float("inf")):
        assert rc(params(0.05, rotation_cost_threshold=th)) == INVALID_ARG
    assert rc(params(0.05, rotation_cost_threshold=0.0)) == 0
    for k in (1, 2, -1, 2049):
        assert rc(params(0.05, k_select=k)) == UNSUPPORTED
    assert rc(params(0.05, k_select=3)) == 0 and rc(params(0.05, k_select=2048)) == 0
    # an index outside its cloud, as lgr_gror* reports it
    for field, n in (("index_query", pr["src"].shape[0]), ("index_match", pr["tgt"].shape[0])):
        for v in (n, -1):
            bad = pr["corr"].copy()
            bad[field][17] = v
            assert rc(params(0.05), bad) == INVALID_ARG
    # the defaults are the reference's commented values (src/alignment.cpp:48-55)
    p = params(0.25)
    assert (p.noise_bound, p.k_select, p.rotation_max_iterations) == (0.25, 0, 100)
    assert p.rotation_gnc_factor == np.float32(1.4) and p.rotation_cost_threshold == np.float32(0.005) and list(p.reserved) == [0, 0, 0]


def test_gror_degrees_are_the_ranking(lgr):
    """lgr_gror_node_degree_dev(resolution = beta) still returns the degrees TEASER ranks by: the node list is their stable descending
    order, cut at k_select -- and they are the statement's degrees"""
    pr = problem(900, 0.3, 31)
    beta, k = 0.05, 200
    s, t = cuda(pr["src"]), cuda(pr["tgt"])
    deg = lgr.gror_node_degree(s, t, pr["corr"], beta)
    assert np.array_equal(deg, tr.degrees(pr["src"], pr["tgt"], pr["corr"], beta))
    res, info, clique, nodes, mask = lgr.teaser(s, t, pr["corr"], params(beta, k_select=k))
    assert info.n_nodes == k and np.array_equal(nodes, np.argsort(-deg.astype(np.int64), kind="stable")[:k])
    assert set(clique.tolist()) <= set(nodes.tolist())
