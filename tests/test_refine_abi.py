"""CPU: the C ABI of the refinement as the Python binding sees it.  sizeof and every field offset of lgr_refine_params, lgr_refine_step and
lgr_refine_result, taken from include/lgr.h by g++, equal those of the ctypes structures in lgr_amd/capi.py; the constants agree; the entry
points resolve in the built library and refuse a NULL context; the defaults are the documented ones; the revision stays 5."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    "lgr_refine_params": ("score_id", "max_steps", "threshold", "reserved"),
    "lgr_refine_step": ("transformation", "metric", "rmse", "score", "n_inliers"),
    "lgr_refine_result": ("transformation", "metric", "rmse", "score", "n_inliers", "threshold", "steps", "stop", "reserved0", "first", "rejected", "reserved"),
}
PROBE = "#include <stddef.h>\n#include <stdio.h>\n#include \"lgr.h\"\nint main() {\n" + "".join(
    f'    printf("{s} %zu\\n", sizeof({s}));\n' + "".join(f'    printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n' for f in fs) for s, fs in FIELDS.items()) + """
    printf("MAX_STEPS %d\\nGROUP %d\\nSTOP_MAX_STEPS %d\\nSTOP_NO_GAIN %d\\nSTOP_NO_PAIRS %d\\n", LGR_REFINE_MAX_STEPS, LGR_REFINE_GROUP,
           LGR_REFINE_STOP_MAX_STEPS, LGR_REFINE_STOP_NO_GAIN, LGR_REFINE_STOP_NO_PAIRS);
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
    for name, cls in (("lgr_refine_params", capi.RefineParams), ("lgr_refine_step", capi.RefineStep), ("lgr_refine_result", capi.RefineResult)):
        assert int(got[name]) == C.sizeof(cls), name
        assert tuple(f for f, _ in cls._fields_) == FIELDS[name]
        for f in FIELDS[name]:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    assert int(got["MAX_STEPS"]) == capi.REFINE_MAX_STEPS == 1024 and int(got["GROUP"]) == capi.REFINE_GROUP == 4
    for c in ("MAX_STEPS", "NO_GAIN", "NO_PAIRS"):
        assert int(got["STOP_" + c]) == getattr(capi, "REFINE_STOP_" + c), c
    assert len(capi.REFINE_STOP_NAMES) == 3
    assert int(got["LGR_VERSION"]) == capi.ABI_VERSION == 5   # additive: the revision stays
    for sym in ("lgr_refine_plane_dev", "lgr_refine_plane", "lgr_default_refine_params"):
        assert getattr(capi.lib(), sym) is not None, sym
    for m in ("refine_plane", "refine_plane_host"):
        assert callable(getattr(capi.Context, m)), m


def test_defaults_and_null_context():
    from lgr_amd import capi
    p = capi.RefineParams(score_id=7, max_steps=-3, threshold=5.0)
    p.reserved[2] = 9
    capi.lib().lgr_default_refine_params(C.byref(p))
    assert (p.score_id, p.max_steps, p.threshold, list(p.reserved)) == (capi.SCORE_MSE, 10, 0.0, [0] * 5)
    capi.lib().lgr_default_refine_params(None)   # tolerated, like the other default fillers
    q = capi.refine_params(score_id=1, max_steps=3, threshold=0.25)
    assert (q.score_id, q.max_steps, q.threshold) == (1, 3, 0.25)
    # no context: refused before anything is touched (good and bad arguments alike), nothing written
    pts = np.zeros((4, 12), np.float32)
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16).tolist())
    out = capi.RefineResult()
    out.steps = 77
    ptr = pts.ctypes.data_as(C.c_void_p)
    for fn in (capi.lib().lgr_refine_plane_dev, capi.lib().lgr_refine_plane):
        assert fn(None, ptr, 4, ptr, 4, T, C.byref(p), None, C.byref(out), None, None) == -1
        assert fn(None, None, -1, None, 0, None, None, None, None, None, None) == -1
    assert out.steps == 77
