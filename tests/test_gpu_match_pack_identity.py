"""The operand packing kernel against its reference (pack16_kernel / pack16_ref_kernel, lgr_match_pack.cuh).

pack16_kernel forms the same f16 fragments, norms and tile shells as the reference kernel it replaced, with less live at once.  Under
lgr_match_options.self_check every match call packs with both and compares on the device, bit for bit: any differing 16-byte piece
fails the call, and lgr_match_last_pack_check reports how many pieces were compared.  Every case here runs both directions with
self_check=2, prune=1, near=2, leaves=4 and requires

  * the call to succeed (no differing piece),
  * more than zero pieces compared and zero differing,
  * indices and distances equal to the oracle's brute force (run_both, as in test_gpu_match_norm_terms.py).

Except for the single row against 257, no side is a multiple of 32 or of 256: padding positions sit beside real rows in both roles.
"""
import numpy as np
import pytest

from test_gpu_match import fpfh_like, run_both
from test_gpu_match_norm_terms import norm_rows

pytestmark = pytest.mark.gpu

BASE = dict(self_check=2, prune=1, near=2, leaves=4)
FMT = {"f16": 1, "f16r": 2}


@pytest.fixture
def pack_opts(lgr):
    def set_fmt(fmt):
        lgr.set_match_options(operand_format=FMT[fmt], **BASE)
    yield set_fmt
    lgr.set_match_options()


def identical(lgr, oracle, a, b, block, fmt):
    """both directions against the oracle; then the packing comparison of a two-direction call"""
    import torch
    run_both(lgr, oracle, a, b, block)
    lgr.match_bf2(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), block)
    lgr.sync()
    assert lgr.match_format() == fmt
    compared, differing = lgr.match_pack_check()
    print(f"pack check [{fmt} {len(a)} x {len(b)}]: {compared} pieces compared, {differing} differing")
    assert compared > 0 and differing == 0, (compared, differing)
    return compared


def test_fpfh_rows_rotated(lgr, oracle, pack_opts):
    rng = np.random.default_rng(101)
    pack_opts("f16r")
    compared = identical(lgr, oracle, fpfh_like(rng, 1000), fpfh_like(rng, 1537), 700, "f16r")
    # at least: the 4 stored fragments (8 pieces a row) of the row side and of the 16 column sets, padding included
    assert compared >= 8 * (1000 + 16 * 1537)


@pytest.mark.parametrize("rows", ["fpfh", "floats"])
def test_plain_format(lgr, oracle, pack_opts, rows):
    rng = np.random.default_rng(102)
    if rows == "fpfh":
        a, b = fpfh_like(rng, 1000), fpfh_like(rng, 1537)
    else:   # arbitrary floats: no block sums, mixed signs and magnitudes
        a = (rng.normal(0.0, 1.0, (1000, 33)) * 10.0 ** rng.uniform(-2, 2, (1000, 1))).astype(np.float32)
        b = (rng.normal(0.0, 1.0, (1537, 33)) * 10.0 ** rng.uniform(-2, 2, (1537, 1))).astype(np.float32)
        b[11] = a[5]; a[900] = b[1500]
    pack_opts("f16")
    compared = identical(lgr, oracle, a, b, 700, "f16")
    assert compared >= 14 * (1000 + 16 * 1537)   # 7 stored fragments


@pytest.mark.parametrize("ma,mb", [(31, 2050), (1, 257)])
@pytest.mark.parametrize("fmt", ["f16r", "f16"])
def test_side_smaller_than_a_tile(lgr, oracle, pack_opts, fmt, ma, mb):
    rng = np.random.default_rng(103 + ma)
    pack_opts(fmt)
    identical(lgr, oracle, fpfh_like(rng, ma), fpfh_like(rng, mb), 1000, fmt)


@pytest.mark.parametrize("kind", ["centres", "subnormal", "far"])
def test_norm_expansion_corners(lgr, oracle, pack_opts, kind):
    """rows at their centre, at the largest |x'|^2 of the call, with N / c0 an f16 subnormal (the construction of
    test_gpu_match_norm_terms.py), and non-finite rows that become padding: n1 = 65504, n2 = +inf in both roles"""
    rng = np.random.default_rng({"centres": 21, "subnormal": 22, "far": 23}[kind])
    modes, far_rows = fpfh_like(rng, 12).astype(np.float64), fpfh_like(rng, 2, spread=0.05)
    a, b = norm_rows(rng, modes, far_rows, 1003, kind), norm_rows(rng, modes, far_rows, 1601, kind)
    b[100] = a[7]; a[900] = b[1500]
    a[50, 7] = np.nan; a[333, :] = np.inf; a[1002, 32] = -np.inf
    b[20, :] = np.nan; b[21, 3] = np.inf; b[1600, 0] = np.nan
    pack_opts("f16r")
    identical(lgr, oracle, a, b, 600, "f16r")


def test_every_set_packed_one_read(lgr, oracle, pack_opts):
    """train rows spread over all 16 clusters, the query side inside one of them: all 16 column sets are packed (and compared)
    although the row blocks' centres name one"""
    rng = np.random.default_rng(105)
    modes = fpfh_like(rng, 40, spread=0.3).astype(np.float64)
    d = rng.normal(0.0, 0.05, (1537, 3, 11)); d -= d.mean(2, keepdims=True)
    b = (modes[rng.integers(0, 40, 1537)] + d.reshape(1537, 33)).astype(np.float32)
    d = rng.normal(0.0, 0.05, (1000, 3, 11)); d -= d.mean(2, keepdims=True)
    a = (modes[3] + d.reshape(1000, 33)).astype(np.float32)
    pack_opts("f16r")
    compared = identical(lgr, oracle, a, b, 700, "f16r")
    assert compared >= 8 * (1000 + 16 * 1537)
