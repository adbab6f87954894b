"""Generates tests/golden/ref_utils.json: what the REFERENCE'S OWN CODE returns for the inputs of tests/test_oracle_ref.py (and the CSV
lines of tests/test_host_io.py), recorded through oracle/_ref/liblgr_ref_utils.so -- the reference's std-only translation units
behind oracle/ref/ref_utils_shim.cpp (recipe: `make -C oracle ref REF=<reference checkout>`).  The tests compare the oracle and the
format code against this record, so they run wherever the repository is checked out; the library is only needed to write it.

    python tests/golden/make_ref_fixtures.py            # rewrites the fixture
    python tests/golden/make_ref_fixtures.py --check    # re-records in memory and compares with the committed file
"""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lidar-global-registration_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import oracle as o  # noqa: E402
from lgr_amd import formats  # noqa: E402

PATH = os.path.join(HERE, "ref_utils.json")
INT_MAX = 2**31 - 1
RNG_SEEDS = [0, 1, 566, 567, 566 + 7, 566 + 255, 2**32 - 1]
RNG_N = 30000
RNG_N_566 = 60000     # the REJECT-subsequence test reads 3 x 20 000 draws of seed 566
CSV_TEXT = ("reading,gT00,gT01\n" "a.ply,1,2\n" "b.ply,,3,\n" ",,\n" "\n" "quoted \"x,y\",7\n" "crlf,1,2\r\n" "last,no,newline")
SPLIT_CASES = [("a,b,c", ","), ("a,,c,", ","), ("", ","), ("x::y::", "::"), ("fpfh shot rops", " ")]


def stream_digest(a):
    """sha256 of an int32 stream's little-endian bytes (the streams themselves are incompressible: 120 kB per seed)"""
    return hashlib.sha256(np.ascontiguousarray(a, "<i4").tobytes()).hexdigest()


def comb_cases():
    cases = [(0, 3), (1, 3), (2, 3), (3, 3), (4, 3), (10, 3), (100, 3), (2344, 3), (2345, 3), (2346, 3), (10000, 3), (200000, 3),
             (298000, 3), (INT_MAX, 3), (50, 0), (50, 1), (50, 2), (50, 4), (60, 30), (5, 7)]
    rng = np.random.default_rng(0)
    cases += [(int(n), 3) for n in rng.integers(0, 5000, 300)] + [(int(n), int(k)) for n, k in zip(rng.integers(0, 200, 300), rng.integers(0, 9, 300))]
    return cases


def hash_inputs():
    rng = np.random.default_rng(1)
    keys = np.concatenate([rng.integers(-2**31, 2**31 - 1, (300, 3)), rng.integers(-50, 50, (300, 3)), [[0, 0, 0], [-1, -1, -1], [INT_MAX, -INT_MAX - 1, 0]]])
    pts = np.concatenate([rng.normal(0, 10, (300, 3)), [[0.0, -0.0, 1.0], [np.inf, -np.inf, 1e-45], [1e38, -1e38, 3.0]]]).astype(np.float32)
    return keys.astype(np.int64), pts


def format_inputs():
    vals = np.array([0.0, 1.0, -1.0, 0.1, 1.0 / 3.0, 2.0 / 3.0, 123456.0, 1234567.0, 999999.5, 1e-5, 1.5e-5, 9.9999e-5, 1e-4, 100000.0,
                     1e6, 1e20, -2.5e-20, 3.4e38, 1e-45, 1.17549435e-38, np.inf, -np.inf, 0.02362, 566.0, 1e-4 + 1e-9], np.float32)
    vals = np.concatenate([vals, np.random.default_rng(2).normal(0, 1, 200).astype(np.float32) * np.float32(10.0) ** np.random.default_rng(3).integers(-8, 8, 200).astype(np.float32)])
    return vals, vals.astype(np.float64) * 1.000000123


def transformation_input():
    return np.random.default_rng(3).normal(size=(4, 4)).astype(np.float32)


def _stream(ref, seed, n):
    out = np.zeros(n, np.int32)
    ref.ref_rng_stream(0, INT_MAX, seed, n, out.ctypes.data_as(C.c_void_p))
    return out


def _rows(ref, text):
    buf = C.create_string_buffer(1 << 16)
    n = ref.ref_csv_rows(text.encode(), buf, len(buf))
    assert n >= 0
    return [] if n == 0 else [row.split("\x1f") for row in buf.value.decode().split("\x1e")]


def _saved_lines(ref, fn, a, tmp):
    p = os.path.join(tmp, "v.csv")
    fn(a.ctypes.data_as(C.c_void_p), len(a), p.encode())
    return open(p).read().split("\n")


def record(ref):
    out = {"rng": []}
    for seed in RNG_SEEDS:
        s = _stream(ref, seed, RNG_N_566 if seed == 566 else RNG_N)
        out["rng"].append({"seed": seed, "n": len(s), "sha256": stream_digest(s), "head": s[:32].tolist(), "min": int(s.min())})
    out["comb_or_max"] = [[n, k, ref.ref_comb_or_max_int(n, k)] for n, k in comb_cases()]
    keys, pts = hash_inputs()
    hk = []
    for ix, iy, iz in keys:
        h = 0
        for e in (ix, iy, iz):
            h = ref.ref_combine_hash_int(h, int(e))
        hk.append([int(ix), int(iy), int(iz), int(h)])
    hp = []
    for x, y, z in pts:
        h = 0
        for e in (x, y, z):
            h = ref.ref_combine_hash_float(h, float(e))
        hp.append([int(v) for v in np.array([x, y, z], np.float32).view(np.uint32)] + [int(h)])
    out["voxel_hash"], out["point_hash"] = hk, hp
    out["csv_rows"] = [{"text": CSV_TEXT, "rows": _rows(ref, CSV_TEXT)}]
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "gt.csv")
        formats.save_transformation(p, "scan_7.ply", transformation_input())
        text = open(p).read()
        out["transformation_csv"] = {"text": text, "rows": _rows(ref, text)}
        vals, dv = format_inputs()
        out["save_vector_float"] = _saved_lines(ref, ref.ref_save_vector_float, vals, tmp)
        out["save_vector_double"] = _saved_lines(ref, ref.ref_save_vector_double, dv, tmp)
        out["save_vector_float_neg_zero"] = _saved_lines(ref, ref.ref_save_vector_float, np.array([-0.0], np.float32), tmp)
    buf = C.create_string_buffer(4096)
    out["split"] = []
    for text, delim in SPLIT_CASES:
        n = ref.ref_split(text.encode(), delim.encode(), buf, len(buf))
        out["split"].append({"text": text, "delim": delim, "n": n, "tokens": buf.value.decode().split("\x1f") if n else []})
    msg = C.create_string_buffer(256)
    out["rassert"] = []
    for cond in (1, 0):
        msg.value = b""
        rc = ref.ref_rassert(cond, msg, 256)
        out["rassert"].append({"condition": cond, "threw": rc, "message": msg.value.decode()})
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    ref = o.ref_utils()
    if ref is None:
        raise SystemExit("oracle/_ref/liblgr_ref_utils.so is not built (make -C oracle ref REF=<reference checkout>)")
    fx = record(ref)
    if "--check" in sys.argv[1:]:
        same = fx == load()
        print("ref_utils.json", "matches" if same else "DIFFERS FROM", "the reference library")
        raise SystemExit(0 if same else 1)
    with open(PATH, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
