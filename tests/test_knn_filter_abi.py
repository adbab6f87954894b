"""The k-nearest filter's control entry points are additions to the C ABI: exported by liblgr_hip.so, declared in include/lgr.h, and no
struct changed -- sizeof(lgr_match_options) as lgr_amd.capi defines it is what it was before them (64 bytes: sixteen int32 words)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lgr_ctx_set_knn_filter", "lgr_ctx_get_knn_filter", "lgr_match_knn_last", "lgr_match_knn_last_check")


def test_exported_and_declared():
    from lgr_amd import capi
    header = open(os.path.join(ROOT, "include", "lgr.h")).read()
    for name in NAMES:
        assert getattr(capi.lib(), name) is not None
        assert re.search(r"^int\s+%s\(lgr_ctx\*" % name, header, re.M), name
    for method in ("set_knn_filter", "knn_filter", "match_knn_last", "match_knn_last_check"):
        assert callable(getattr(capi.Context, method))


def test_no_struct_changed():
    from lgr_amd import capi
    assert C.sizeof(capi.MatchOptions) == 64
    header = open(os.path.join(ROOT, "include", "lgr.h")).read()
    body = header[:header.index("} lgr_match_options;")].rsplit("typedef struct {", 1)[1]
    assert len(re.findall(r"^\s*int32_t\s+\w+;", body, re.M)) == 16
    assert capi.lib().lgr_version() == 5
