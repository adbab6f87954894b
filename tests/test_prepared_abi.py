"""CPU: the C ABI of the prepared clouds as the Python binding sees it.  sizeof and every field offset of struct lgr_cloud_info and
lgr_cloud_level_info, taken from include/lgr.h by a C and a C++ compiler (the info struct is a tag: its getter carries the same name), equal
those of the ctypes structures in lgr_amd/capi.py; the entry points resolve in the built library; lgr_cloud_destroy(NULL) is LGR_OK and
the other calls refuse NULL objects; the revision stays 5."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    "struct lgr_cloud_info": ("n", "keypoints", "row_len", "levels", "first_log2_radius", "multiscale", "bytes", "reserved"),
    "lgr_cloud_level_info": ("log2_radius", "radius", "voxel", "rows", "surface", "reserved"),
}
PROBE = "#include <stddef.h>\n#include <stdio.h>\n#include \"lgr.h\"\nint main() {\n" + "".join(
    f'    printf("{s}|%zu\\n", sizeof({s}));\n' + "".join(f'    printf("{s}.{f}|%zu\\n", offsetof({s}, {f}));\n' for f in fs) for s, fs in FIELDS.items()) + """
    printf("LGR_VERSION|%d\\n", LGR_VERSION);
    return sizeof(&lgr_cloud_info) == 0;   /* the function, next to the struct tag of the same name (unevaluated: nothing to link) */
}
"""
SYMBOLS = ("lgr_cloud_prepare", "lgr_cloud_prepare_dev", "lgr_cloud_destroy", "lgr_cloud_info", "lgr_cloud_keypoints", "lgr_cloud_keypoints_dev",
           "lgr_cloud_level", "lgr_cloud_level_dev", "lgr_correspondences_prepared", "lgr_correspondences_prepared_dev", "lgr_align_prepared")


@pytest.mark.parametrize("compiler,ext", [("gcc", "c"), ("g++", "cpp")])
def test_struct_layout(tmp_path, compiler, ext):
    from lgr_amd import capi
    src, exe = str(tmp_path / ("probe." + ext)), str(tmp_path / "probe")
    open(src, "w").write(PROBE)
    subprocess.check_call([compiler, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = dict(line.rsplit("|", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    for name, cls in (("struct lgr_cloud_info", capi.CloudInfo), ("lgr_cloud_level_info", capi.CloudLevelInfo)):
        assert int(got[name]) == C.sizeof(cls), name
        assert tuple(f for f, _ in cls._fields_) == FIELDS[name]
        for f in FIELDS[name]:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    assert int(got["LGR_VERSION"]) == capi.ABI_VERSION == 5 == capi.lib().lgr_version()   # additions only: the revision stays


def test_symbols_resolve_and_null_objects():
    from lgr_amd import capi
    lib = capi.lib()
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None, sym
    for m in ("prepare_cloud", "prepare_cloud_host", "correspondences_prepared", "align_prepared"):
        assert callable(getattr(capi.Context, m)), m
    for m in ("info", "keypoints", "levels", "level", "close", "__enter__", "__exit__"):
        assert callable(getattr(capi.PreparedCloud, m)), m
    assert lib.lgr_cloud_destroy(None) == 0
    info, li, m = capi.CloudInfo(), capi.CloudLevelInfo(), C.c_int(7)
    info.n = 77
    assert lib.lgr_cloud_info(None, C.byref(info)) == capi.ERR_INVALID_ARG and info.n == 77
    assert lib.lgr_cloud_keypoints(None, None, C.byref(m)) == capi.ERR_INVALID_ARG and m.value == 7
    assert lib.lgr_cloud_level(None, 0, C.byref(li), None, None) == capi.ERR_INVALID_ARG
    p, h = capi.default_params(), C.c_void_p()
    assert lib.lgr_cloud_prepare_dev(None, None, 0, 0, C.byref(p), None, C.byref(h)) == capi.ERR_INVALID_ARG
    assert lib.lgr_cloud_prepare(None, None, 0, 0, C.byref(p), None, C.byref(h)) == capi.ERR_INVALID_ARG
    res, n = capi.Result(), C.c_int(0)
    assert lib.lgr_correspondences_prepared_dev(None, None, None, C.byref(p), None, None, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.lgr_correspondences_prepared(None, None, None, C.byref(p), None, None, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.lgr_align_prepared(None, None, None, C.byref(p), None, None, C.byref(res)) == capi.ERR_INVALID_ARG
