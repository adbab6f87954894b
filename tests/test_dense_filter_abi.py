"""The dense filter's control entry points are additions to the C ABI: exported by liblgr_hip.so, declared in include/lgr.h, reachable from
lgr_amd.capi.Context, and no struct changed -- sizeof(lgr_match_options) is 64 bytes and lgr_version() stays 5."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgr_ctx_set_dense_filter", "lgr_ctx_get_dense_filter", "lgr_match_dense_last", "lgr_match_dense_last_check")


def test_exported_and_declared():
    from lgr_amd import capi
    header = open(os.path.join(ROOT, "include", "lgr.h")).read()
    for name in NAMES:
        assert getattr(capi.lib(), name) is not None
        assert re.search(r"^int\s+%s\(lgr_ctx\*" % name, header, re.M), name
    for method in ("set_dense_filter", "dense_filter", "match_dense_last", "match_dense_last_check"):
        assert callable(getattr(capi.Context, method))


def test_no_struct_changed():
    from lgr_amd import capi
    assert C.sizeof(capi.MatchOptions) == 64
    assert capi.lib().lgr_version() == 5
