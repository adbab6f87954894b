"""The hypothesis-set entry points of the C ABI without a GPU: the exports resolve, arguments are refused before any device is touched,
lgr_hypothesis has the layout the ctypes binding mirrors, and the ABI revision has not moved (exports only)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("lgr_ransac_multi_dev", "lgr_ransac_multi", "lgr_fold_hypotheses_dev", "lgr_fold_hypotheses", "lgr_choose_best_hypothesis")


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from lgr_amd import capi
    return capi


def test_exports_resolve_and_the_revision_stays(capi):
    lib = capi.lib()
    for name in EXPORTS:
        assert hasattr(lib, name), name
    assert lib.lgr_version() == 5 and capi.HYPOTHESES_MAX == 2048


def test_null_context_and_bad_max_set_are_invalid_arguments(capi):
    lib = capi.lib()
    n, bi = C.c_int(7), C.c_int(7)
    res = capi.Result()
    p = capi.default_params()
    out = (capi.Hypothesis * 4)()
    for max_set in (0, 1, 64, capi.HYPOTHESES_MAX, capi.HYPOTHESES_MAX + 1):   # a NULL context is refused whatever max_set is
        for f in (lib.lgr_ransac_multi_dev, lib.lgr_ransac_multi):
            assert f(None, None, 0, None, 0, None, 0, C.byref(p), max_set, C.byref(res), out, C.byref(n), C.byref(bi)) == capi.ERR_INVALID_ARG
        for f in (lib.lgr_fold_hypotheses_dev, lib.lgr_fold_hypotheses):
            assert f(None, None, None, 0, C.c_float(0.05), max_set, None, None, None, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.lgr_choose_best_hypothesis(None, None, 0, None, 0, None, 0, None, 0, None, None, None) == capi.ERR_INVALID_ARG


def test_hypothesis_layout_matches_c_compiler(capi, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lgr.h"\nint main(){'
                    'printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(lgr_hypothesis), offsetof(lgr_hypothesis, transformation), '
                    'offsetof(lgr_hypothesis, iteration), offsetof(lgr_hypothesis, loop_metric), offsetof(lgr_hypothesis, metric), '
                    'offsetof(lgr_hypothesis, n_inliers), offsetof(lgr_hypothesis, converged), offsetof(lgr_hypothesis, uniformity), '
                    'LGR_HYPOTHESES_MAX);return 0;}')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    Hy = capi.Hypothesis
    assert got == [C.sizeof(Hy), Hy.transformation.offset, Hy.iteration.offset, Hy.loop_metric.offset, Hy.metric.offset, Hy.n_inliers.offset,
                   Hy.converged.offset, Hy.uniformity.offset, capi.HYPOTHESES_MAX]
    assert C.sizeof(Hy) == 152
