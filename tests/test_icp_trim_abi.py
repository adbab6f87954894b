"""CPU: the C ABI of trimmed ICP and the rank select as the Python binding sees it.  sizeof and every field offset of lgr_icp_trim_params and
lgr_icp_trim_step, taken from include/lgr.h by g++, equal those of capi.IcpTrimParams / capi.IcpTrimStep and of the statement's loader;
the entry points resolve in the built library and refuse a NULL context; the default filler writes keep = 1, scale_from_median = 0 and
lgr_default_icp_ex_params into `ex`; the suffix-less names stay free; the revision stays 5."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_trim_ref_lib as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ex", "keep", "scale_from_median", "reserved")
STEP = ("candidates", "kept", "cut", "scale")
PROBE = "#include <stddef.h>\n#include <stdio.h>\n#include \"lgr.h\"\nint main() {\n" + \
    '    printf("sizeof %zu %zu\\n", sizeof(lgr_icp_trim_params), sizeof(lgr_icp_trim_step));\n' + \
    "".join(f'    printf("{f} %zu\\n", offsetof(lgr_icp_trim_params, {f}));\n' for f in FIELDS) + \
    "".join(f'    printf("{f} %zu\\n", offsetof(lgr_icp_trim_step, {f}));\n' for f in STEP) + \
    '    printf("LGR_VERSION %d\\n", LGR_VERSION);\n    return 0;\n}\n'


def test_struct_layout_and_symbols(tmp_path):
    from lgr_amd import capi
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(src, "w").write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = dict(line.split(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    assert [int(v) for v in got["sizeof"].split()] == [C.sizeof(capi.IcpTrimParams), C.sizeof(capi.IcpTrimStep)] == [88, 16]
    assert tuple(f for f, _ in capi.IcpTrimParams._fields_) == FIELDS and tuple(f for f, _ in capi.IcpTrimStep._fields_) == STEP
    for f in FIELDS:
        assert int(got[f]) == getattr(capi.IcpTrimParams, f).offset, f
    for f in STEP:
        assert int(got[f]) == getattr(capi.IcpTrimStep, f).offset == getattr(TR.TrimStep, f).offset, f
    assert capi.IcpTrimParams.ex.size == C.sizeof(capi.IcpExParams) and C.sizeof(TR.TrimStep) == 16
    assert int(got["LGR_VERSION"]) == capi.ABI_VERSION == 5   # additive: the revision stays
    for sym in ("lgr_icp_trim_dev", "lgr_icp_trim_host", "lgr_default_icp_trim_params", "lgr_rank_select_dev", "lgr_rank_select_host"):
        assert getattr(capi.lib(), sym) is not None, sym
    assert not hasattr(capi.lib(), "lgr_icp_trim") and not hasattr(capi.lib(), "lgr_rank_select")   # the plain names stay free
    for m in ("icp_trim", "icp_trim_host", "rank_select", "rank_select_host"):
        assert callable(getattr(capi.Context, m)), m


def test_defaults_and_null_context():
    from lgr_amd import capi
    p = capi.IcpTrimParams()
    C.memset(C.byref(p), 0xff, C.sizeof(p))
    capi.lib().lgr_default_icp_trim_params(C.byref(p))
    d = capi.IcpExParams()
    capi.lib().lgr_default_icp_ex_params(C.byref(d))
    assert bytes(p.ex) == bytes(d) and (p.keep, p.scale_from_median, list(p.reserved)) == (1.0, 0.0, [0, 0])
    capi.lib().lgr_default_icp_trim_params(None)   # tolerated, like the other default fillers
    q = capi.icp_trim_params(keep=0.75, scale_from_median=1.5, variant="point", robust="cauchy", min_normal_cos=0.25, max_iterations=3, max_dist=0.25)
    assert (q.keep, q.scale_from_median, q.ex.variant, q.ex.robust, q.ex.min_normal_cos, q.ex.base.max_iterations, q.ex.base.max_dist) == (0.75, 1.5, 1, 2, 0.25, 3, 0.25)
    # no context: refused before anything is touched, nothing written
    pts = np.zeros((4, 12), np.float32)
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16).tolist())
    out = capi.IcpResult()
    out.iterations = 77
    ptr = pts.ctypes.data_as(C.c_void_p)
    for fn in (capi.lib().lgr_icp_trim_dev, capi.lib().lgr_icp_trim_host):
        assert fn(None, ptr, 4, ptr, 4, T, C.byref(p), C.byref(out), None, None, None) == -1
        assert fn(None, None, -1, None, 0, None, None, None, None, None, None) == -1
    assert out.iterations == 77
    ranks, idx, key, nv = (C.c_int64 * 1)(0), (C.c_int32 * 1)(77), (C.c_float * 1)(), C.c_int64(77)
    for fn in (capi.lib().lgr_rank_select_dev, capi.lib().lgr_rank_select_host):
        assert fn(None, ptr, None, 4, ranks, 1, idx, key, None, C.byref(nv)) == -1
    assert (idx[0], nv.value) == (77, 77)
