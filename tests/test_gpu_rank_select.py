"""GPU: the exact rank select (lgr_rank_select_dev / lgr_rank_select_host, csrc/lgr_rank_select.cuh) against numpy.lexsort((index, key bits))
over the counted elements: the index and the key at every requested rank, the `below` flags and n_valid, at the sizes where the select
takes another path (one lane, wave and workgroup boundaries, one group of 4096, several groups, the index digits 0 / 1 / 2 / 3 wide) and on
key sets an ICP run cannot produce: all equal (every decision falls on the index), two and five distinct values (heavy ties across
workgroups), keys that differ in the lowest mantissa bit, 0 / denormals / 1 / FLT_MAX mixed, masks with holes, and NaN, negative and
infinite keys, which are not counted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
BIG = 70001
FAMILIES = ("equal", "two", "five", "lsb", "mixed", "holes", "skipped")


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def make(family, n, seed):
    """(keys float32 [n], valid uint8 [n] or None)"""
    rng = np.random.default_rng(seed)
    if family == "equal":
        return np.full(n, 0.25, F), None
    if family == "two":
        return rng.choice(np.array([0.5, 2.0], F), n), None
    if family == "five":
        return rng.choice(np.array([0.0, 0.125, 0.5, 3.0, 1e30], F), n), None
    if family == "lsb":
        return (np.uint32(0x3F800000) + rng.integers(0, 2, n).astype(np.uint32)).view(F), None
    if family == "mixed":
        return rng.choice(np.array([0.0, 1e-45, 1e-40, 1.0, np.finfo(F).max], F), n), None
    keys = rng.random(n).astype(F)
    if family == "holes":
        return keys, rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), n)
    assert family == "skipped"
    bad = rng.random(n) < 0.3
    keys[bad] = rng.choice(np.array([np.nan, -1.0, np.inf, -np.inf, -0.0], F), int(bad.sum()))
    return keys, None


def order_of(keys, valid):
    """the counted elements in (key bits, index) order"""
    bits = keys.view(np.uint32)
    ok = bits <= 0x7F7FFFFF
    if valid is not None:
        ok &= valid != 0
    idx = np.nonzero(ok)[0]
    return idx[np.lexsort((idx, bits[idx]))]


def check(lgr, d_keys, d_valid, keys, order, r0, r1=None, flags=True, call=None):
    ranks = [r0] if r1 is None else [r0, r1]
    got = (call or lgr.rank_select)(d_keys, ranks, d_valid)
    assert got["n_valid"] == len(order)
    for q, r in enumerate(ranks):
        if r == len(order):
            assert q == 0 and got["index"][0] == -1 and got["key"][0] == 0
            continue
        assert got["index"][q] == order[r], (ranks, q)
        assert got["key"][q].view(np.uint32) == keys[order[r]].view(np.uint32), (ranks, q)
    if flags:
        want = np.zeros(len(keys), np.uint8)
        want[order[:r0]] = 1
        below = got["below"]
        below = below if isinstance(below, np.ndarray) else below.cpu().numpy()
        assert int(below.sum()) == r0 and np.array_equal(below, want), ranks
    return got


@pytest.mark.parametrize("family", FAMILIES)
def test_every_rank_at_the_boundary_sizes(lgr, family):
    for n in SIZES:
        keys, valid = make(family, n, 100 + n)
        order = order_of(keys, valid)
        d_keys, d_valid = cuda(keys), cuda(valid) if valid is not None else None
        nv = len(order)
        if family in ("holes", "skipped"):
            assert nv < n or n <= 2
        if nv == 0:
            check(lgr, d_keys, d_valid, keys, order, 0)
            continue
        for r in range((nv + 1) // 2):   # every rank, two a call: r from below, its mirror from above
            check(lgr, d_keys, d_valid, keys, order, r, nv - 1 - r, flags=n <= 65 or r % 61 == 0)
        check(lgr, d_keys, d_valid, keys, order, nv - 1, 0)    # the flags of the last rank
        check(lgr, d_keys, d_valid, keys, order, nv)           # ranks[0] == n_valid: every counted element is below


@pytest.mark.parametrize("family", FAMILIES)
def test_several_groups(lgr, family):
    """70 001 elements: 18 groups of 4096, an index of three digits"""
    keys, valid = make(family, BIG, 7)
    order = order_of(keys, valid)
    d_keys, d_valid = cuda(keys), cuda(valid) if valid is not None else None
    nv = len(order)
    assert nv > BIG // 3
    rng = np.random.default_rng(11)
    ranks = [0, (nv - 1) // 2, nv - 1] + rng.integers(0, nv, 50).tolist()
    for k, r in enumerate(ranks):
        check(lgr, d_keys, d_valid, keys, order, r, ranks[-1 - k], flags=k < 6)
    check(lgr, d_keys, d_valid, keys, order, nv)
    got = check(lgr, keys, valid, keys, order, ranks[4], ranks[5], call=lgr.rank_select_host)   # the host twin
    dev = lgr.rank_select(d_keys, [ranks[4], ranks[5]], d_valid)
    assert (got["index"], got["key"], got["n_valid"]) == (dev["index"], dev["key"], dev["n_valid"]) and np.array_equal(got["below"], dev["below"].cpu().numpy())


def test_host_twin_equals_the_device(lgr):
    for family, n in (("skipped", 257), ("holes", 1000), ("equal", 65), ("mixed", 1)):
        keys, valid = make(family, n, 3)
        order = order_of(keys, valid)
        nv = len(order)
        d_keys, d_valid = cuda(keys), cuda(valid) if valid is not None else None
        for ranks in ([0], [nv // 2, nv - 1], [nv], [nv - 1, 0]):
            got = check(lgr, keys, valid, keys, order, *ranks, call=lgr.rank_select_host)
            dev = lgr.rank_select(d_keys, ranks, d_valid)
            assert (got["index"], got["n_valid"]) == (dev["index"], dev["n_valid"]) and np.array_equal(got["below"], dev["below"].cpu().numpy())
            assert [k.view(np.uint32) for k in got["key"]] == [k.view(np.uint32) for k in dev["key"]]


def test_refusals_and_empty_input(lgr):
    import torch
    from lgr_amd import capi
    keys, valid = make("holes", 300, 5)
    nv = len(order_of(keys, valid))
    d_keys, d_valid = cuda(keys), cuda(valid)
    for call, k, v in ((lgr.rank_select, d_keys, d_valid), (lgr.rank_select_host, keys, valid)):
        for ranks in ([-1], [nv + 1], [300], [0, nv], [0, -1], [nv, nv], [2 ** 40]):
            with pytest.raises(capi.LgrError, match="rc=-1"):
                call(k, ranks, v)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            call(k, [0, 1, 2], v)   # n_ranks 3
        assert call(k, [nv], v)["n_valid"] == nv   # a good call afterwards works
    # nothing counted: rank 0 == n_valid is the only rank there is
    none = np.full(70, np.nan, F)
    got = lgr.rank_select(cuda(none), [0])
    assert (got["index"], got["n_valid"], int(got["below"].sum())) == ([-1], 0, 0)
    with pytest.raises(capi.LgrError, match="rc=-1"):
        lgr.rank_select(cuda(none), [0, 0])
    # n = 0: no launch, the same answers
    for call, k in ((lgr.rank_select, torch.empty(0, dtype=torch.float32, device="cuda")), (lgr.rank_select_host, np.zeros(0, F))):
        got = call(k, [0])
        assert (got["index"], got["n_valid"]) == ([-1], 0)
        with pytest.raises(capi.LgrError, match="rc=-1"):
            call(k, [1])
