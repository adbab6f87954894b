"""CPU: the C ABI of the dense closest-plane evaluation as the Python binding sees it.  sizeof and every field offset of
lgr_plane_dense_eval and lgr_metric_eval, taken from include/lgr.h by g++, equal those of the ctypes structures in lgr_amd/capi.py, and the
new entry points resolve in the built library."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "lgr.h"
#define F(S, f) printf(#S "." #f " %zu\n", offsetof(S, f))
int main() {
    printf("lgr_plane_dense_eval %zu\n", sizeof(lgr_plane_dense_eval));
    F(lgr_plane_dense_eval, n_inliers); F(lgr_plane_dense_eval, rmse); F(lgr_plane_dense_eval, metric); F(lgr_plane_dense_eval, threshold);
    F(lgr_plane_dense_eval, score); F(lgr_plane_dense_eval, reserved);
    printf("lgr_metric_eval %zu\n", sizeof(lgr_metric_eval));
    F(lgr_metric_eval, metric); F(lgr_metric_eval, rmse); F(lgr_metric_eval, n_inliers); F(lgr_metric_eval, n_correct_inliers); F(lgr_metric_eval, reserved);
    printf("LGR_VERSION %d\n", LGR_VERSION);
    return 0;
}
"""


def test_struct_layouts_and_symbols(tmp_path):
    from lgr_amd import capi
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(src, "w").write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    for name, cls in (("lgr_plane_dense_eval", capi.PlaneDenseEval), ("lgr_metric_eval", capi.MetricEval)):
        assert int(got[name]) == C.sizeof(cls), name
        fields = [f for f, _ in cls._fields_]
        assert sorted(k.split(".")[1] for k in got if k.startswith(name + ".")) == sorted(fields)
        for f in fields:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    assert int(got["LGR_VERSION"]) == capi.ABI_VERSION == 5   # additive: the revision stays
    for sym in ("lgr_evaluate_plane_dense_dev", "lgr_evaluate_plane_dense", "lgr_analysis_metric_dev", "lgr_analysis_metric"):
        assert getattr(capi.lib(), sym) is not None, sym
    for m in ("evaluate_plane_dense", "evaluate_plane_dense_host", "analysis_metric", "analysis_metric_host"):
        assert callable(getattr(capi.Context, m))
