"""CPU: the coloured PLY writer (PointXYZRGBNormal) and saveVector.  formats.write_ply_colored against host/lgr_io.hpp's savePLYFileBinary /
savePLYFileASCII byte for byte, a read back through read_ply / read_ply_colors, and the shim's getColor / mixPointColor against the
statement's."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_ref_lib as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from lgr_amd import formats
    d = tmp_path_factory.mktemp("colored")
    exe = str(d / "colored_ply_write")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "colored_ply_write.cpp"),
                           "-o", exe])
    rng = np.random.default_rng(4)
    n = 257
    pts = np.zeros((n, 12), F)
    pts[:, 0:3] = rng.standard_normal((n, 3)) * 10
    pts[:, 3] = 1
    pts[:, 4:7] = rng.standard_normal((n, 3))
    pts[:, 8] = rng.random(n)          # intensity: no field of the coloured point
    pts[:, 9] = rng.random(n) * 0.1
    pts[3, 4:7] = np.nan
    pts[5, 0] = 1e-30; pts[6, 1] = -123456.789
    colors = rng.integers(0, 1 << 24, n).astype(np.int32)
    colors[:3] = (0, 0xffffff, D.COLOR_PARAKEET)
    with open(d / "cloud.bin", "wb") as f:
        f.write(np.int32(n).tobytes()); f.write(pts.tobytes()); f.write(colors.tobytes())
    formats.write_ply_colored(str(d / "py_bin.ply"), pts, colors, binary=True)
    formats.write_ply_colored(str(d / "py_ascii.ply"), pts, colors, binary=False)
    formats.save_vector(str(d / "py_vector.csv"), np.array([0.5, 1.25, 1e-7], F))
    out = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return d, pts, colors, out.stdout


def test_python_writer_equals_cpp_writer(files):
    d, _, _, _ = files
    for kind in ("bin", "ascii"):
        a, b = open(d / f"py_{kind}.ply", "rb").read(), open(d / f"cpp_{kind}.ply", "rb").read()
        assert a == b, kind
    head = open(d / "py_bin.ply", "rb").read().split(b"end_header\n")[0].decode().splitlines()
    assert [h.split()[-1] for h in head if h.startswith("property")] == ["x", "y", "z", "red", "green", "blue", "normal_x", "normal_y", "normal_z", "curvature"]
    assert open(d / "py_vector.csv").read() == open(d / "cpp_vector.csv").read() == "value\n0.5\n1.25\n1e-07\n"


def test_read_back(files):
    from lgr_amd import formats
    d, pts, colors, _ = files
    for kind in ("bin", "ascii"):
        got, fields = formats.read_ply(str(d / f"py_{kind}.ply"))
        assert fields == ["x", "y", "z", "normal_x", "normal_y", "normal_z", "curvature"] and formats.has_normals(fields)
        for sl in (slice(0, 3), slice(4, 7), slice(9, 10)):
            assert np.array_equal(got[:, sl].view(np.uint32), pts[:, sl].view(np.uint32)), (kind, sl)
        assert (got[:, 8] == 0).all()
        assert np.array_equal(formats.read_ply_colors(str(d / f"py_{kind}.ply")), colors)
    formats.write_ply_colored(str(d / "empty.ply"), np.zeros((0, 12), F), np.zeros(0, np.int32))
    got, _ = formats.read_ply(str(d / "empty.ply"))
    assert got.shape == (0, 12)


def test_shim_colour_functions(files):
    _, _, _, stdout = files
    lines = dict(line.split(" ", 1) for line in stdout.splitlines())
    for k in range(4):
        assert int(lines[f"mix{k}"], 16) == D.mix_color(D.COLOR_RED, D.COLOR_WHITE, k)
    assert [int(x, 16) for x in lines["color"].split()] == [D.get_color(0, 0, 1), D.get_color(1, 0, 1), D.get_color(0.5, 0, 1)]
