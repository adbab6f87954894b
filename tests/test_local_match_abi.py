"""CPU: the C ABI of matchLocal with a k-list and of matchFLANN for every row length, as the Python binding sees it.  include/lgr.h
declares the four entry points (a C++ probe takes their addresses with the declared types), the built library exports them and they
refuse a NULL context, capi.Context binds them with the declared number of arguments, and the revision stays 5."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgr.h")

# entry point -> (number of C arguments, the binding method, that method's parameters after self)
ENTRY = {
    "lgr_match_local_knn_dev": (13, "match_local_knn", ["qpts", "tpts", "qf", "tf", "guess", "radius", "k"]),
    "lgr_match_local_knn": (13, "match_local_knn_host", ["qpts", "tpts", "qf", "tf", "guess", "radius", "k"]),
    "lgr_match_flann_rows_dev": (8, "match_flann_rows", ["q", "t"]),
    "lgr_match_flann_rows": (8, "match_flann_rows_host", ["q", "t"]),
}
PROBE = """#include <cstdint>
#include <cstdio>
#include "lgr.h"
using local_fn = int (*)(lgr_ctx*, int, const float*, int, const float*, int, const float*, const float*, const float*, float, int, int32_t*, float*);
using flann_fn = int (*)(lgr_ctx*, int, const float*, int, const float*, int, int32_t*, float*);
int main() {
    local_fn a = &lgr_match_local_knn, b = &lgr_match_local_knn_dev;
    flann_fn c = &lgr_match_flann_rows, d = &lgr_match_flann_rows_dev;
    std::printf("%d %d %d\\n", LGR_VERSION, (int) LGR_RANDOMNESS_MAX, (int) (a && b && c && d));
    return 0;
}
"""


def test_header_declares_the_entry_points(tmp_path):
    text = open(HEADER).read()
    for name, (argc, _, _) in ENTRY.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == argc, (name, args)
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(src, "w").write(PROBE)
    csrc = os.path.join(ROOT, "lidar-global-registration_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", csrc, "-llgr_hip", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    assert subprocess.check_output([exe], text=True).split() == ["5", "8", "1"]


def test_binding_matches_the_declarations():
    from lgr_amd import capi
    assert capi.ABI_VERSION == 5 and capi.lib().lgr_version() == 5   # additive: the revision stays
    source = inspect.getsource(capi.Context)
    for name, (argc, method, params) in ENTRY.items():
        fn = getattr(capi.lib(), name)
        assert fn is not None, name
        assert list(inspect.signature(getattr(capi.Context, method)).parameters)[1:] == params, method
        assert inspect.signature(getattr(capi.Context, "match_local_knn")).parameters["k"].default == 1
        # the call site in the binding passes exactly the declared number of arguments
        call = re.search(r"_lib\." + name + r"\((.*?)\)\)\n", source, flags=re.S)
        assert call, name
        depth, n = 0, 1
        for ch in call.group(1):
            depth += ch in "(["
            depth -= ch in ")]"
            n += ch == "," and depth == 0
        assert n == argc, (name, n)
        # no context: refused before anything is touched
        if argc == 13:
            assert fn(None, 33, None, 0, None, 0, None, None, None, C.c_float(1.0), 1, None, None) == -1, name
        else:
            assert fn(None, 33, None, 0, None, 0, None, None) == -1, name
