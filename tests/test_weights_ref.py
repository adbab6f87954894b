"""CPU: pins the statement of weighted_closest_plane's point weights (tests/cpp/weights_ref.cpp): quantile against hand-worked values of
include/utils.h's double formula, findBin on crafted normals (251 bins, |nz| > 1 declared), principal curvatures on a plane and a
cylinder, the constant weights' sum, and the device's expf / logf restatements against the host libm."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weights_ref_lib as W  # noqa: E402


def formula(values, q=0.8):
    """utils.h quantile<float>: ith (n q - i) + jth (j - n q) in double, rounded to float"""
    v = sorted(np.float32(x) for x in values)
    n = len(v)
    if n == 1:
        return np.float32(v[0])
    i = math.floor(q * (n - 1)); j = min(i + 1, n - 1)
    if i < j:
        return np.float32(float(v[i]) * (n * q - i) + float(v[j]) * (j - n * q))
    return np.float32(v[i])


@pytest.mark.parametrize("values, expected", [
    ([0.5], 0.5),                                   # n = 1: the value itself
    ([3.0, 1.0], 1.0 * (2 * 0.8 - 0) + 3.0 * (1 - 2 * 0.8)),   # n = 2: i = 0, j = 1
    ([1, 2, 3, 4, 5], 4.0 * (5 * 0.8 - 3) + 5.0 * (4 - 5 * 0.8)),
    ([2, 2, 2, 7, 7], 7.0 * (5 * 0.8 - 3) + 7.0 * (4 - 5 * 0.8)),   # duplicates
    (list(range(10, 0, -1)), 8.0 * (10 * 0.8 - 7) + 9.0 * (8 - 10 * 0.8)),   # n = 10: i = 7, j = 8
])
def test_quantile_hand_worked(values, expected):
    got = W.quantile(values)
    assert np.float32(got) == np.float32(expected) == formula(values)


def test_quantile_i_equals_j():
    # q = 1: i = j = n - 1, the largest value without interpolation
    v = np.array([0.25, 4.0, 1.5], np.float32)
    assert W.lib().wref_quantile(1.0, W._p(v), 3) == np.float32(4.0)


def test_nss_bins_crafted():
    assert W.nss_bin(0.0, 0.0, 1.0) == 0
    assert W.nss_bin(0.0, 0.0, -1.0) == 200            # theta = (float) pi > M_PI: the clamp keeps it, the `== M_PI` test never fires
    assert W.nss_bin(1e-4, -1e-12, -1.0) == 250        # and phi rounds to (float) 2 pi: the last of the 251 bins
    assert W.nss_bin(1.0, -1e-8, 0.0) == 12 * 8 + 50   # phi = (float) 2 pi, theta = pi / 2
    assert W.nss_bin(0.0, 1.0, 0.0) >= 64               # most normals land past the reference's 64 entries
    assert W.nss_bin(0.0, 0.0, np.nextafter(np.float32(1), np.float32(2))) == -1   # |nz| > 1: NaN polar angle, not counted
    assert W.nss_bin(0.0, 0.0, np.float32(-1.0000001)) == -1


def test_nss_weights_divisor_64():
    pts = np.zeros((5, 12), np.float32)
    pts[:, 6] = 1.0                       # four normals in bin 0
    pts[4, 6] = np.float32(1.0000001)     # one with |nz| > 1: weight 0
    w, s = W.weights(pts, "nss")
    assert np.array_equal(w, np.array([np.float32(1) / np.float32(4) / np.float32(64)] * 4 + [0], np.float32))
    assert s == np.float32(4 * (1 / 4 / 64))


def test_principal_curvatures_plane_and_cylinder():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12)), -1).reshape(-1, 2).astype(np.float32) * 0.1
    plane = np.zeros((g.shape[0], 12), np.float32)
    plane[:, :2] = g; plane[:, 3] = 1; plane[:, 6] = 1
    pc1, pc2 = W.principal_curvatures(plane)
    assert (pc1 == 0).all() and (pc2 == 0).all()
    a = np.linspace(0, 2 * np.pi, 40, endpoint=False)
    z = np.arange(10) * 0.1
    A, Z = np.meshgrid(a, z)
    cyl = np.zeros((A.size, 12), np.float32)
    cyl[:, 0] = np.cos(A.ravel()); cyl[:, 1] = np.sin(A.ravel()); cyl[:, 2] = Z.ravel(); cyl[:, 3] = 1
    cyl[:, 4] = np.cos(A.ravel()); cyl[:, 5] = np.sin(A.ravel())
    pc1, pc2 = W.principal_curvatures(cyl)
    assert (pc1 > 1e-3).all() and (np.abs(pc2) < 1e-5).all() and (pc2 < pc1).all()


def test_constant_sum_is_n():
    pts = np.zeros((1000, 12), np.float32)
    w, s = W.weights(pts, "constant")
    assert (w == 1).all() and s == 1000.0


def test_curvature_weights_nonfinite_zero():
    pts = np.zeros((4, 12), np.float32)
    pts[:, 9] = [0.5, np.nan, np.inf, 0.25]
    w, s = W.weights(pts, "curvature")
    assert np.array_equal(w, np.array([0.5, 0, 0, 0.25], np.float32)) and s == np.float32(0.75)


def test_expf_restatement_is_libm():
    """csrc/lgr_weights_math.h's expf equals the host's on every float <= 0 down past the underflow threshold (and to -inf)."""
    assert W.count_libm_mismatch(5, 0x80000000, 0xC2D00000) == 0     # -0 .. -104: subnormal results and the flush to +0
    assert W.count_libm_mismatch(5, 0xFF800000, 0xFF800000) == 0     # -inf
    assert W.count_libm_mismatch(5, 0x00000000, 0x42B17217) == 0     # and the positive side up to the overflow threshold


def test_logf_restatement_is_libm_on_1_2():
    assert W.count_libm_mismatch(6, 0x3F800000, 0x40000000) == 0
