"""CPU: the C ABI of the debug layer as the Python binding sees it.  sizeof and every field offset of lgr_temperature_out, taken from
include/lgr.h by g++, equal those of the ctypes structure in lgr_amd/capi.py; the colour constants agree; the new entry points resolve in
the built library; the revision stays 5."""
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
    printf("lgr_temperature_out %zu\n", sizeof(lgr_temperature_out));
    F(lgr_temperature_out, temp_distance); F(lgr_temperature_out, temp_normal); F(lgr_temperature_out, color_distance);
    F(lgr_temperature_out, color_normal); F(lgr_temperature_out, nn);
    printf("BEIGE %d\nRED %d\nPARAKEET %d\nBLUE %d\nWHITE %d\n", LGR_COLOR_BEIGE, LGR_COLOR_RED, LGR_COLOR_PARAKEET, LGR_COLOR_BLUE, LGR_COLOR_WHITE);
    printf("LGR_VERSION %d\n", LGR_VERSION);
    return 0;
}
"""

SYMBOLS = ("lgr_temperature_map_dev", "lgr_temperature_map", "lgr_temperature_maps_dev", "lgr_temperature_maps", "lgr_compare_overlaps_dev",
           "lgr_compare_overlaps", "lgr_nearest_dev", "lgr_color_map_dev", "lgr_color_map", "lgr_color_weights_dev", "lgr_color_weights",
           "lgr_color_correspondences_dev", "lgr_color_correspondences")
METHODS = ("temperature_map", "temperature_map_host", "temperature_maps", "temperature_maps_host", "compare_overlaps", "compare_overlaps_host", "nearest",
           "color_map", "color_map_host", "color_correspondences", "color_correspondences_host")


def test_struct_layout_constants_and_symbols(tmp_path):
    from lgr_amd import capi
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(src, "w").write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    name, cls = "lgr_temperature_out", capi.TemperatureOut
    assert int(got[name]) == C.sizeof(cls)
    fields = [f for f, _ in cls._fields_]
    assert sorted(k.split(".")[1] for k in got if k.startswith(name + ".")) == sorted(fields) and tuple(fields) == capi.TEMP_FIELDS
    for f in fields:
        assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f
    for c in ("BEIGE", "RED", "PARAKEET", "BLUE", "WHITE"):
        assert int(got[c]) == getattr(capi, "COLOR_" + c), c
    assert int(got["LGR_VERSION"]) == capi.ABI_VERSION == 5   # additive: the revision stays
    for sym in SYMBOLS:
        assert getattr(capi.lib(), sym) is not None, sym
    for m in METHODS:
        assert callable(getattr(capi.Context, m)), m
