"""CPU: csrc/lgr_stdhash.h against the compiler's own library -- std::hash<float>, the folded HashEigen / PointHash of the reference
(include/common.h:202-223) and the iteration order of std::unordered_map / std::unordered_set (src/downsample.cpp:20,32-34,
src/common.cpp:417-427).  Everything is exact: hash codes equal, orders equal element by element."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hash_order_ref_lib as H  # noqa: E402

INT_MAX = 2 ** 31 - 1


def test_hash_float():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x00000001, 0x80000001, 0x007fffff, 0x7f7fffff, 0xff7fffff,
                        0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fa00001], np.uint32)   # +-0, +-1, denormals, FLT_MAX, inf, NaNs
    s, h = H.hash_float(np.concatenate([special, bits]))
    assert np.array_equal(s, h)
    assert s[0] == 0 and s[1] == 0 and s[2] != 0


def test_hash_voxel_and_point():
    rng = np.random.default_rng(4)
    xyz = rng.integers(-2 ** 31, 2 ** 31, (200_000, 3), dtype=np.int64).astype(np.int32)
    xyz[:8] = [[0, 0, 0], [-1, -1, -1], [INT_MAX, INT_MAX, INT_MAX], [-INT_MAX - 1, 0, 5], [1, 2, 3], [3, 2, 1], [0, -7, INT_MAX], [2097151, 2097151, 2097151]]
    s, h = H.hash_voxel(xyz)
    assert np.array_equal(s, h)
    b3 = rng.integers(0, 2 ** 32, (200_000, 3), dtype=np.uint64).astype(np.uint32)
    b3[:4] = [[0, 0x80000000, 0], [0x7fc00000, 0x3f800000, 0x80000000], [1, 0x80000001, 0x7f7fffff], [0x3f800000, 0x3f800000, 0x3f800000]]
    s, h = H.hash_point(b3)
    assert np.array_equal(s, h)
    assert (s >= np.uint64(2 ** 63)).any()          # the 64-bit float codes and the seed shifts reach the top bit
    assert s[0] == H.hash_point(np.zeros((1, 3), np.uint32))[0][0]     # -0 hashes like +0


def test_schedule_comes_from_the_policy():
    c = H.rehash_counts(5088)
    assert c[0] == 0 and c == sorted(set(c)) and len(c) >= 8          # a first rehash on the first insertion, growing after that
    ns = H.sizes()
    assert {0, 1, 2} <= set(ns) and all(x in ns for k in c for x in (max(k - 1, 0), k, k + 1)) and max(ns) > 42043


@pytest.mark.parametrize("spread", [3, 40, 2000])
@pytest.mark.parametrize("reserve", [False, True])
def test_map_order(spread, reserve):
    """the header's epoch rule == std::unordered_map, at every rehash count +-1, with and without reserve"""
    checked = 0
    for n in H.sizes():
        n_el = min(n, spread ** 3)
        xyz = H.distinct_keys(n_el, spread, seed=n + spread)
        seq, cut = xyz, n_el // 2
        if cut:    # repeats of keys that are already in change nothing
            rng = np.random.default_rng(n)
            seq = np.concatenate([xyz[:cut], xyz[rng.integers(0, cut, n_el // 3)], xyz[cut:]])
        res = (len(seq) + (n % 3) * 17) if reserve else 0
        h, oc, orr = H.map_order(seq, reserve=res)
        assert len(h) == n_el
        assert np.array_equal(oc, orr), (n, spread, reserve)
        assert np.array_equal(np.sort(oc), np.arange(n_el))
        checked += 1
    assert checked >= 30


def test_set_order():
    """the same for the point set of filterDuplicatePoints: reserve(n), duplicates, +-0 and NaN points"""
    for n in H.sizes():
        rng = np.random.default_rng(n + 9)
        xyz = rng.normal(size=(n, 3)).astype(np.float32)
        if n >= 32:
            xyz[1] = [0.0, 1.0, 2.0]; xyz[3] = [-0.0, 1.0, 2.0]          # equal: one element
            xyz[5] = [np.nan, 1.0, 2.0]; xyz[6] = xyz[5]                 # never equal: two elements
            xyz[n // 2:n // 2 + n // 4] = xyz[: n // 4]                 # duplicates -- but for the copies of the two NaN points
        h, oc, orr = H.set_order(xyz)
        assert np.array_equal(oc, orr), n
        if n >= 32:
            assert len(h) == n - n // 4 - 1 + 2
            # the real container == the generic replay over the same hash codes
            assert np.array_equal(H.replay(h, reserve=n), oc)


def test_replay_matches_rule_on_adversarial_codes():
    """what the GPU test feeds lgr_hash_order_dev: one bucket, multiples of the final bucket count, codes >= 2^63"""
    n = 1500
    final = 2357                                                         # checked below against the policy's own schedule
    assert 1109 in H.rehash_counts(3000) and 2357 in H.rehash_counts(3000)
    rng = np.random.default_rng(5)
    for h in (np.full(n, 12345, np.uint64), (np.arange(n, dtype=np.uint64) * np.uint64(final)),
              rng.integers(2 ** 63, 2 ** 64, n, dtype=np.uint64), rng.integers(0, 2 ** 64, n, dtype=np.uint64)):
        for res in (0, n, n + 1000):
            assert np.array_equal(H.replay(h, res), H.rule(h, res))
