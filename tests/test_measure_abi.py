"""CPU: the C ABI of the measure test type and of the batched ground-truth evaluation as the Python binding sees it.  sizeof and every
field offset of lgr_measure_run and lgr_measurement, taken from include/lgr.h by g++, equal those of the ctypes structures in
lgr_amd/capi.py; the constants agree; the entry points resolve in the built library and refuse a NULL context; the revision stays 5."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    "lgr_measure_run": ("seed", "result", "eval"),
    "lgr_measurement": ("n_times", "n_success", "success_rate", "mae", "sae", "mte", "ste", "mrmse", "srmse", "mtime", "stime", "reserved"),
}
PROBE = "#include <stddef.h>\n#include <stdio.h>\n#include \"lgr.h\"\nint main() {\n" + "".join(
    f'    printf("{s} %zu\\n", sizeof({s}));\n' + "".join(f'    printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n' for f in fs) for s, fs in FIELDS.items()) + """
    printf("lgr_result %zu\\nlgr_gt_eval %zu\\n", sizeof(lgr_result), sizeof(lgr_gt_eval));
    printf("BATCH_MAX %d\\nBATCH_CHUNK %d\\n", LGR_GT_BATCH_MAX, LGR_GT_BATCH_CHUNK);
    printf("LGR_VERSION %d\\n", LGR_VERSION);
    return 0;
}
"""


def test_struct_layout_constants_and_symbols(tmp_path):
    from lgr_amd import capi
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(src, "w").write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    for name, cls in (("lgr_measure_run", capi.MeasureRun), ("lgr_measurement", capi.Measurement)):
        assert int(got[name]) == C.sizeof(cls), name
        assert tuple(f for f, _ in cls._fields_) == FIELDS[name]
        for f in FIELDS[name]:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    assert int(got["lgr_result"]) == C.sizeof(capi.Result) and int(got["lgr_gt_eval"]) == C.sizeof(capi.GtEval)
    assert int(got["BATCH_MAX"]) == capi.GT_BATCH_MAX == 64 and int(got["BATCH_CHUNK"]) == capi.GT_BATCH_CHUNK == 8
    assert int(got["LGR_VERSION"]) == capi.ABI_VERSION == 5 == capi.lib().lgr_version()   # additive: the revision stays
    for sym in ("lgr_evaluate_gt_batch_dev", "lgr_evaluate_gt_batch", "lgr_measure_dev", "lgr_measure", "lgr_measure_mean", "lgr_measure_deviation"):
        assert getattr(capi.lib(), sym) is not None, sym
    for m in ("evaluate_gt_batch", "evaluate_gt_batch_host", "measure", "measure_host"):
        assert callable(getattr(capi.Context, m)), m


def test_null_context_is_refused():
    from lgr_amd import capi
    pts = np.zeros((4, 12), np.float32)
    ptr = pts.ctypes.data_as(C.c_void_p)
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16).tolist())
    conv = (C.c_int32 * 1)(1)
    ev = capi.GtEval()
    ev.overlap_size = 77
    for fn in (capi.lib().lgr_evaluate_gt_batch_dev, capi.lib().lgr_evaluate_gt_batch):
        assert fn(None, ptr, 4, ptr, 4, None, 0, T, 1, T, C.c_float(0.1), conv, None, C.byref(ev), None) == -1
    assert ev.overlap_size == 77
    p = capi.default_params()
    runs, m = (capi.MeasureRun * 2)(), capi.Measurement()
    m.n_times = 77
    for fn in (capi.lib().lgr_measure_dev, capi.lib().lgr_measure):
        assert fn(None, ptr, 4, ptr, 4, C.byref(p), None, None, T, None, 2, runs, C.byref(m)) == -1
    assert m.n_times == 77
