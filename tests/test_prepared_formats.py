"""CPU: the files of save_features.  formats.write_histograms (saveFeatures, include/feature_analysis.h:11-27) and
formats.write_extracted_ids (saveExtractedPointIds, src/feature_analysis.cpp:46-54) against hand-written bytes, and the C++ writers of
host/lgr_io.hpp against the Python ones byte for byte (tests/cpp/prepared_formats.cpp)."""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-global-registration_amd"))
from lgr_amd import formats  # noqa: E402

F = np.float32
# a NaN, a denormal, 1e-7, 100.0, a negative zero -- and values that show the six significant digits
ROWS = np.array([[np.nan, 1e-45, 1e-7, 100.0], [-0.0, 0.1, 123456.789, -1.5e10], [1.0, 2.5, 1e6, 3.4028235e38]], F)
ROWS_TEXT = ("0,nan,1.4013e-45,1e-07,100\n"
             "1,-0,0.1,123457,-1.5e+10\n"
             "2,1,2.5,1e+06,3.40282e+38\n")
IDS = dict(id_src=np.array([2, 0], np.int32), id_tgt=np.array([1, 1], np.int32),
           xyz_src=np.array([[1e-7, -0.0, 100.0], [0.25, 1e-45, -3.5]], F), xyz_tgt=np.array([[1.5, 2.5, np.nan], [1.5, 2.5, np.nan]], F))
IDS_TEXT = ("id_src,id_tgt,x_src,x_tgt,y_src,y_tgt,z_src,z_tgt\n"
            "2,1,1e-07,1.5,-0,2.5,100,nan\n"
            "0,1,0.25,1.5,1.4013e-45,2.5,-3.5,nan\n")


def test_write_histograms_bytes(tmp_path):
    p = str(tmp_path / "h.csv")
    formats.write_histograms(p, ROWS)
    assert open(p, "rb").read() == ROWS_TEXT.encode()
    formats.write_histograms(p, ROWS, indices=[7, 5, 3])
    want = "".join(str(i) + ln[1:] for i, ln in zip((7, 5, 3), ROWS_TEXT.splitlines(True)))
    assert open(p, "rb").read() == want.encode()
    formats.write_histograms(p, np.zeros((0, 33), F))
    assert open(p, "rb").read() == b""
    neg_nan = np.array([[0xffc00000]], np.uint32).view(F)     # `ostream << float` prints the sign of a NaN
    formats.write_histograms(p, neg_nan)
    assert open(p, "rb").read() == b"0,-nan\n"


def test_histograms_names():
    assert formats.histograms_name() == "histograms_src" and formats.histograms_name(is_source=False) == "histograms_tgt"
    assert formats.histograms_name(-3) == "histograms-3_src" and formats.histograms_name(2, False) == "histograms2_tgt"


def test_write_extracted_ids_bytes(tmp_path):
    p = str(tmp_path / "ids.csv")
    formats.write_extracted_ids(p, IDS)
    assert open(p, "rb").read() == IDS_TEXT.encode()


def test_cpp_writers_equal_the_python_writers(tmp_path):
    exe = str(tmp_path / "prepared_formats")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "prepared_formats.cpp"), "-o", exe])
    rng = np.random.default_rng(3)
    rows = np.concatenate([ROWS.reshape(-1), np.array([0xffc00000], np.uint32).view(F), (rng.normal(size=383) * 10.0 ** rng.integers(-8, 8, 383)).astype(F)])
    rows = rows.reshape(12, 33)
    with open(tmp_path / "rows.bin", "wb") as f:
        f.write(struct.pack("<ii", *rows.shape) + rows.tobytes())
    src = (rng.normal(size=(50, 3)) * 30).astype(F)
    tgt = (rng.normal(size=(40, 3)) * 1e-3).astype(F)
    src[0], tgt[0] = IDS["xyz_src"][0], IDS["xyz_tgt"][0]
    ids = dict(id_src=rng.integers(0, 50, 25).astype(np.int32), id_tgt=rng.integers(0, 40, 25).astype(np.int32))
    ids["id_src"][0] = ids["id_tgt"][0] = 0
    ids["xyz_src"], ids["xyz_tgt"] = src[ids["id_src"]], tgt[ids["id_tgt"]]
    with open(tmp_path / "ids.bin", "wb") as f:
        f.write(struct.pack("<i", 25) + np.stack([ids["id_src"], ids["id_tgt"]], 1).tobytes())
        f.write(struct.pack("<i", 50) + src.tobytes() + struct.pack("<i", 40) + tgt.tobytes())
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == [formats.histograms_name(), formats.histograms_name(is_source=False), formats.histograms_name(2)]
    formats.write_histograms(str(tmp_path / "py_a.csv"), rows)
    formats.write_histograms(str(tmp_path / "py_b.csv"), rows, indices=[1000 - 7 * i for i in range(12)])
    formats.write_extracted_ids(str(tmp_path / "py_ids.csv"), ids)
    assert (tmp_path / "cpp_histograms_src.csv").read_bytes() == (tmp_path / "py_a.csv").read_bytes()
    assert (tmp_path / "cpp_histograms-3_tgt.csv").read_bytes() == (tmp_path / "py_b.csv").read_bytes()
    assert (tmp_path / "cpp_ids.csv").read_bytes() == (tmp_path / "py_ids.csv").read_bytes()
