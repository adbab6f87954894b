"""The rotated operand format's two-term norm expansion (pack16_kernel, FMT_F16R): rows whose centred norm |x'|^2 sits at the
ends of what the two f16 terms n1 = f16(N / c0), n2 = f16((N - c0 n1) / c0) can hold.

  * rows AT their cluster centre: N = 0, both terms 0;
  * rows at the largest |x'|^2 of the call: n1 at the top of the f16 range (N_max <= 2^15 c0);
  * rows within ~1e-4 of a centre beside far rows that set N_max: N / c0 in the f16 subnormal range (the absolute floor of the bound);

with row counts that are not multiples of the 32-row tile, so that padding positions (n1 = 65504, n2 = +inf) sit beside them.
Matches and distances must equal the oracle's, and every computed filter value must lie within the proven eps of the exact
minimum (lgr_match_options.self_check).  The first test checks the bound the error term is built from on the host.
"""
import numpy as np
import pytest

from test_gpu_match import checked, fpfh_like, run_both


def two_term(N, c0):
    """the rotated format's norm terms, as pack16_kernel computes them (f32 arithmetic, f16 round to nearest)"""
    N = np.asarray(N, np.float32); c0 = np.float32(c0)
    n1 = (N / c0).astype(np.float16)
    r1 = (N.astype(np.float64) - np.float64(c0) * n1.astype(np.float64)).astype(np.float32)   # exact: the kernel's fma
    n2 = (r1 / c0).astype(np.float16)
    return n1, n2


def test_two_term_norm_error_bound():
    """|N - c0 (n1 + n2)| <= 2^-22 N + 2^-25 c0 (1 + 2^-11) over the whole range N in [0, 2^15 c0], subnormal terms included
    (match_impl: the rotated format's EpsExtra states 2^-22 N + 2^-14 c0 (1 + 2^-10), which also covers flushed subnormals)"""
    rng = np.random.default_rng(5)
    for e1 in (0, 4, 11, 13, 15):
        c0 = 2.0 ** e1
        N = np.concatenate([[0.0, 2.0 ** -149, 2.0 ** -24 * c0, 2.0 ** -14 * c0, 2.0 ** 15 * c0],
                            c0 * 2.0 ** rng.uniform(-40, 15, 20000)]).astype(np.float32)
        N = N[N <= np.float32(2.0 ** 15 * c0)]
        n1, n2 = two_term(N, c0)
        assert np.isfinite(n1).all() and np.isfinite(n2).all()
        err = np.abs(N.astype(np.float64) - c0 * (n1.astype(np.float64) + n2.astype(np.float64)))
        bound = 2.0 ** -22 * N.astype(np.float64) + 2.0 ** -25 * c0 * (1 + 2.0 ** -11)
        assert (err <= bound).all(), (e1, N[err > bound][:4], err[err > bound][:4])
        # the leading term is the three-term expansion's: the coarse d2~ of the first two MFMA steps is unchanged
        assert (n1 == (N / np.float32(c0)).astype(np.float16)).all()


def zero_sum_noise(rng, m, scale):
    """noise that keeps every 11-bin block's sum: the rows stay on the rotated format's hyperplanes"""
    d = rng.normal(0.0, scale, (m, 3, 11))
    d -= d.mean(2, keepdims=True)
    return d.reshape(m, 33)


def norm_rows(rng, modes, far_rows, m, kind):
    """rows about the shared modes (both sets: near pairs across them); far_rows: the two shared rows of the kind 'far'"""
    lab = rng.integers(0, len(modes), m)
    x = modes[lab].copy()
    if kind == "centres":
        # symmetric pairs about each mode and the mode itself: the exact (integer-sum) centre of such a cluster is the mode
        half = m // 3
        d = zero_sum_noise(rng, half, 0.5)
        x[:half] += d
        x[half:2 * half] = modes[lab[:half]] - d
    elif kind == "subnormal":
        # rows within ~1e-4 of a mode beside a few far rows (|x'| ~ 1e3) that set the largest |x'|^2: N / c0 ~ 2^15 |x'|^2 / max |x'|^2
        # of the near rows is an f16 subnormal (< 2^-14) even where a far row pulls their centre off the mode by ~0.1
        x += zero_sum_noise(rng, m, 1e-4)
        far = rng.choice(m, 24, replace=False)
        x[far] += zero_sum_noise(rng, 24, 300.0)
    else:   # "far": tight clusters, and rows at the largest |x'|^2, duplicated (exact ties at the top of the n1 range)
        x += zero_sum_noise(rng, m, 0.05)
        far = rng.choice(m, 40, replace=False)
        x[far] = far_rows[0]
        x[far[::2]] = far_rows[1]
    return x.astype(np.float32)


@pytest.fixture(params=["auto", "prune_sub4", "prune_sub4_sweep"])
def norm_mode(request, lgr):
    base = {"operand_format": 2, "self_check": 2}
    if request.param.startswith("prune"):
        base.update(prune=1, near=2, leaves=4, poison_tables=1)
    if request.param.endswith("_sweep"):
        base["coarse_rejection"] = 2   # the coarse sweep also when the pass schedules most of the tiles
    lgr._base_opts = base
    lgr.set_match_options(**base)
    yield request.param
    lgr._base_opts = {}
    lgr.set_match_options()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["centres", "subnormal", "far"])
def test_norm_extremes_parity_and_bound(lgr, oracle, norm_mode, kind):
    import torch
    rng = np.random.default_rng({"centres": 11, "subnormal": 12, "far": 13}[kind])
    modes, far_rows = fpfh_like(rng, 12).astype(np.float64), fpfh_like(rng, 2, spread=0.05)
    a, b = norm_rows(rng, modes, far_rows, 5003, kind), norm_rows(rng, modes, far_rows, 7001, kind)
    b[100] = a[7]; a[4000] = b[6500]   # exact ties across the sets
    run_both(lgr, oracle, a, b, 2000)
    lgr.match_bf2(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 2000)
    lgr.sync()
    assert lgr.match_format() == "f16r"
    # (auto: the skipping path is not taken at this size -- no coarse rejection, no column-stage rows)
    auto = norm_mode == "auto"
    checked(lgr, f"f16r {kind} {norm_mode}", coarse=not auto, colstage=False if auto else None)
