"""-m gpu: the MFMA-filtered nearest-row matcher of 352- and 135-float rows (lgr_ctx_set_dense_filter) against the CPU references
tests/cpp/shot_ref.cpp and tests/cpp/rops_ref.cpp, on index and distance bits.  Mode 1 (filtered at any size) with the device self-check
unless stated: small shapes (fewer rows than a tile, tile boundaries on either side, bf blocks that straddle tiles, more bf blocks than
tiles), ties / NaN / one-ulp rows, rows the operands cannot carry, a row whose candidates overflow the list, 5000 identical rows, many
tiles with the counters of lgr_match_dense_last held to their caps, the three modes against each other, the pipeline and prepared clouds
under modes 0 and 1, the host twins, the refusals.  Every test restores (-1, 0)."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rops_ref_lib  # noqa: E402
import shot_ref_lib  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_INVALID_ARG = -1   # include/lgr.h
F = np.float32
REF = {352: shot_ref_lib, 135: rops_ref_lib}
DIMS = (352, 135)


@contextlib.contextmanager
def dense_filter(lgr, mode, self_check=1):
    lgr.set_dense_filter(mode, self_check)
    try:
        yield
    finally:
        lgr.set_dense_filter(-1, 0)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(rng, m, dim=352):
    """test_gpu_match_shot.py's generator (non-negative, sparse-ish, unit norm), at either row length"""
    x = rng.random((m, dim)).astype(F) ** 4
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F)


def _match(lgr, dim):
    return lgr.match_shot if dim == 352 else lgr.match_rops


def _match2(lgr, dim):
    return lgr.match2_shot if dim == 352 else lgr.match2_rops


def _dev(lgr, q, t, block):
    i, d = _match(lgr, q.shape[1])(cuda(q), cuda(t), block)
    lgr.sync()
    return i.cpu().numpy(), d.cpu().numpy()


def _eq(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32), err_msg=what)


@pytest.fixture(scope="module")
def many():
    """per row length: 5000 x 7000 rows with exact hits and duplicated train rows, and the reference on 1500 sampled queries"""
    out = {}
    for dim in DIMS:
        rng = np.random.default_rng(5000)
        q, t = _rows(rng, 5000, dim), _rows(rng, 7000, dim)
        q[:500] = t[rng.choice(7000, 500)]
        t[3000:3200] = t[100:300]
        sel = np.concatenate([np.arange(0, 600), rng.choice(5000, 900, replace=False)])
        out[dim] = dict(q=q, t=t, sel=sel, want=REF[dim].match(q[sel], t, 2000))
    return out


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mq,mt", [(1, 1), (1, 65), (31, 33), (33, 31), (63, 64), (65, 129), (300, 2100)])
def test_shapes(lgr, mq, mt, dim):
    rng = np.random.default_rng(35200 + mq * 7 + mt)
    q, t = _rows(rng, mq, dim), _rows(rng, mt, dim)
    with dense_filter(lgr, 1):
        for block in (7, 64, 10000):
            _eq(_dev(lgr, q, t, block), REF[dim].match(q, t, block), f"block={block}")
            last = lgr.match_dense_last()
            assert last[0] == 1 and last[6] == 0 and last[2] + last[3] == mq, last
    assert lgr.dense_filter() == (-1, 0)


@pytest.mark.parametrize("dim", DIMS)
def test_ties_nan_and_ulp_rows(lgr, dim):
    rng = np.random.default_rng(3)
    t = _rows(rng, 300, dim)
    t[[10, 15, 120, 250]] = t[5]                              # duplicates inside block 0 and across blocks (block 100)
    t[200] = np.nextafter(t[5], F(2))                         # one ulp away in every element
    t[201] = t[5]; t[201, 17] = np.nextafter(t[5, 17], F(0))  # one ulp away in one element
    t[[30, 31]] = np.nan
    t[32, 100] = np.nan
    q = np.concatenate([t[[5, 10, 200, 201, 30, 32]], _rows(rng, 50, dim)])
    with dense_filter(lgr, 1):
        for block in (100, 7, 1, 1000):
            _eq(_dev(lgr, q, t, block), REF[dim].match(q, t, block), f"block={block}")
            assert lgr.match_dense_last()[6] == 0
        i, _ = _dev(lgr, q, t, 100)
    assert i[0] == 250 and i[4] == -1 and i[5] == -1


@pytest.mark.parametrize("dim", DIMS)
def test_irregular_rows(lgr, dim):
    rng = np.random.default_rng(35)
    q, t = _rows(rng, 70, dim), _rows(rng, 150, dim)
    t[[30, 31]] = np.nan
    t[32, 100] = np.nan
    t[64, 0] = np.inf
    t[40] = F(3e38)
    q[[3, 66]] = np.nan
    q[4, 16] = np.nan
    q[5, 1] = -np.inf
    t[50] = t[50] * F(1e18)                      # finite distances (about 1e18) that the operands cannot carry inside the bound
    q[7] = q[7] * F(1e18)
    t[51] = F(1e18) * _rows(rng, 1, dim)[0]      # a pair of such rows near each other: q[8]'s nearest row is t[51]
    q[8] = t[51] * F(1.0 + 2.0 ** -20)
    with dense_filter(lgr, 1):
        for block in (1000, 33, 64):
            want = REF[dim].match(q, t, block)
            _eq(_dev(lgr, q, t, block), want, f"block={block}")
            last = lgr.match_dense_last()
            assert last[0] == 1 and last[3] > 0 and last[4] > 0 and last[6] == 0, last
            assert (want[0][[3, 4, 5, 66]] == -1).all() and not np.isin(want[0], [30, 31, 32, 40, 64]).any()
            assert want[0][8] == 51 and np.isfinite(want[1][8])


@pytest.mark.parametrize("dim", DIMS)
def test_capacity_overflow_goes_to_the_fallback(lgr, dim):
    rng = np.random.default_rng(36)
    with dense_filter(lgr, 1):
        _dev(lgr, _rows(rng, 64, dim), _rows(rng, 64, dim), 64)
        cap = lgr.match_dense_last()[5]
        assert 0 < cap < 2000
        t = _rows(rng, 1000 + cap + 1, dim)
        at = rng.choice(len(t), cap + 1, replace=False)
        t[at] = t[at[0]]
        q = _rows(rng, 200, dim)
        q[:50] = t[at[0]]
        for block in (1000, 64):
            _eq(_dev(lgr, q, t, block), REF[dim].match(q, t, block), f"block={block}")
            last = lgr.match_dense_last()
            assert last[0] == 1 and last[3] >= 50 and last[2] + last[3] == 200 and last[6] == 0, last


@pytest.mark.parametrize("dim", DIMS)
def test_identical_rows(lgr, dim):
    rng = np.random.default_rng(4)
    t = np.repeat(_rows(rng, 1, dim), 5000, axis=0)
    q = np.concatenate([t[:3], _rows(rng, 3, dim)])
    with dense_filter(lgr, 1):
        for block in (200000, 333):
            _eq(_dev(lgr, q, t, block), REF[dim].match(q, t, block), f"block={block}")
            last = lgr.match_dense_last()
            assert (last[0] == 1 and last[6] == 0) or last[7] in (1, 2), last   # whichever path answered: the exact one says why


@pytest.mark.parametrize("dim", DIMS)
def test_many_tiles(lgr, many, dim):
    m = many[dim]
    with dense_filter(lgr, 1):
        got = _dev(lgr, m["q"], m["t"], 2000)
        last, worst = lgr.match_dense_last(), lgr.match_dense_last_check()
    _eq((got[0][m["sel"]], got[1][m["sel"]]), m["want"])
    print("match_dense_last", dim, last, "worst |f - d2| / e", worst)
    assert last[0] == 1 and last[6] == 0 and last[2] + last[3] == 5000 and last[5] > 0
    assert 0 <= worst <= 1
    # conditions, not measurements: an ideal filter with any e <= 4e-3 (x + y)^2 and a capacity >= 46 stays far inside them on these rows
    # (float64 on the CPU: at most 46 (352) / 22 (135) candidates per query, 0.11 % of the pairs); one that lets everything through does not
    assert last[3] <= 50, last
    assert last[1] < 5000 * 7000 // 100, last


@pytest.mark.parametrize("dim", DIMS)
def test_modes_return_the_same_bytes(lgr, many, dim):
    q, t = cuda(many[dim]["q"]), cuda(many[dim]["t"])
    sel = many[dim]["sel"]
    out = {}
    for mode in (0, 1, -1):
        with dense_filter(lgr, mode, 0):
            res = [_match(lgr, dim)(q, t, 2000)]
            flag = lgr.match_dense_last()[0]
            ab_i, ab_d, ba_i, ba_d = _match2(lgr, dim)(q, t, 2000)
            res += [(ab_i, ab_d), (ba_i, ba_d), _match(lgr, dim)(t, q, 2000)]
            lgr.sync()
            out[mode] = (flag, [(i.cpu().numpy(), d.cpu().numpy()) for i, d in res])
    assert out[0][0] == 0 and out[1][0] == 1
    for mode in (0, 1, -1):
        r = out[mode][1]
        _eq((r[0][0][sel], r[0][1][sel]), many[dim]["want"], f"mode {mode}")
        _eq(r[1], r[0], f"mode {mode}: a -> b")
        _eq(r[2], r[3], f"mode {mode}: b -> a")
        for got, want in zip(r, out[0][1]):
            _eq(got, want, f"mode {mode} against mode 0")


RESULT_FIELDS = ("iterations", "converged", "n_inliers", "best_iteration", "num_rejections", "estimated_iters", "n_correspondences")
RESULT_FLOATS = ("metric", "best_metric_before_refit")


def _same_result(got, want):
    np.testing.assert_array_equal(got.matrix().astype(F).view(np.uint32), want.matrix().astype(F).view(np.uint32))
    for f in RESULT_FIELDS:
        assert getattr(got, f) == getattr(want, f), f
    for f in RESULT_FLOATS:
        assert np.float32(getattr(got, f)).view(np.uint32) == np.float32(getattr(want, f)).view(np.uint32), f


@pytest.mark.parametrize("case", ["shot", "rops"])
def test_pipeline_and_prepared_clouds(lgr, case):
    from lgr_amd import capi, synthetic
    pair = synthetic.make_pair(4000, 12)
    s, t = cuda(pair["src"]), cuda(pair["tgt"])
    p = capi.default_params(randomness=1, matching_id=0, feature_radius=0.25, bf_block_size=1500, distance_thr=0.1, max_iterations=2000,
                            iss_radius_src=0.02, iss_radius_tgt=0.03, vp_src=pair["vp_src"], vp_tgt=pair["vp_tgt"])
    desc = capi.feature_params("shot") if case == "shot" else capi.feature_params("rops", lrf_id=capi.LRF_GRAVITY)
    got = {}
    for mode in (0, 1):
        with dense_filter(lgr, mode):
            corr = lgr.correspondences(s, t, p, descriptor=desc).cpu().numpy()
            flag = lgr.match_dense_last()[0]
            res = lgr.align_ex2(s, t, p, descriptor=desc)
            with lgr.prepare_cloud(s, p, 0, desc) as a, lgr.prepare_cloud(t, p, 1, desc) as b:
                pcorr = lgr.correspondences_prepared(a, b, p, descriptor=desc).cpu().numpy()
                pres = lgr.align_prepared(a, b, p, descriptor=desc)
            got[mode] = (corr, res, pcorr, pres, flag)
    assert got[0][4] == 0 and got[1][4] == 1 and len(got[0][0]) > 50
    for x in (0, 2):
        assert got[0][x].shape == got[1][x].shape and (got[0][x].view(np.uint8) == got[1][x].view(np.uint8)).all()
    _same_result(got[1][1], got[0][1])
    _same_result(got[1][3], got[0][3])
    assert (got[0][0].view(np.uint8) == got[0][2].view(np.uint8)).all()


def test_host_twins(lgr):
    rng = np.random.default_rng(38)
    with dense_filter(lgr, 1):
        for dim, host in ((352, lgr.match_shot_host), (135, lgr.match_rops_host)):
            q, t = _rows(rng, 100, dim), _rows(rng, 700, dim)
            _eq(host(q, t, 64), REF[dim].match(q, t, 64))
            last = lgr.match_dense_last()
            assert last[0] == 1 and last[6] == 0, last


def test_refusals(lgr):
    from lgr_amd import capi
    lib = capi.lib()
    try:
        for mode, check in ((-2, 0), (2, 0), (0, 2), (1, -1), (7, 7)):
            assert lib.lgr_ctx_set_dense_filter(lgr.h, mode, check) == ERR_INVALID_ARG
            assert lgr.dense_filter() == (-1, 0)
        lgr.set_dense_filter(1, 1)
        assert lib.lgr_ctx_set_dense_filter(lgr.h, 3, 0) == ERR_INVALID_ARG and lgr.dense_filter() == (1, 1)
        assert lib.lgr_ctx_get_dense_filter(lgr.h, None, None) == ERR_INVALID_ARG
        assert lib.lgr_match_dense_last(lgr.h, None) == ERR_INVALID_ARG and lib.lgr_match_dense_last_check(lgr.h, None) == ERR_INVALID_ARG
        rng = np.random.default_rng(9)
        for dim in DIMS:                                  # the context stays usable
            q = _rows(rng, 10, dim)
            i, _ = _dev(lgr, q, q, 10)
            assert (i == np.arange(10)).all() and lgr.knn_filter() == (-1, 0)
    finally:
        lgr.set_dense_filter(-1, 0)
