"""CPU: the aggregates of the measure test type.  Hand-derived known answers pin the two accumulation widths of the restatement
tests/measure_ref_lib.py (double sum for the mean, float sum for the deviation) and the library's own two functions (lgr_measure_mean,
lgr_measure_deviation: plain host code) against them; the CSV header and a row's text are literal."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_ref_lib as M  # noqa: E402

F = np.float32


def lib_mean(v):
    from lgr_amd import capi
    a = np.ascontiguousarray(v, F)
    if len(a) == 0:
        return F(capi.lib().lgr_measure_mean(None, 0))
    return F(capi.lib().lgr_measure_mean(a.ctypes.data_as(C.c_void_p), len(a)))


def lib_deviation(v):
    from lgr_amd import capi
    a = np.ascontiguousarray(v, F)
    if len(a) == 0:
        return F(capi.lib().lgr_measure_deviation(None, 0, C.c_float(0.0)))
    return F(capi.lib().lgr_measure_deviation(a.ctypes.data_as(C.c_void_p), len(a), C.c_float(float(lib_mean(v)))))


def test_mean_is_a_double_sum():
    # 2^24 + 1 + 1: a float sum stays at 2^24 (each 1 is half a unit in the last place there, ties to even) and gives 16777216 / 3 =
    # 5592405.33 -> 5592405.5; the double sum is 16777218 and 16777218 / 3 = 5592406 exactly
    v = [16777216.0, 1.0, 1.0]
    want = F(16777218.0 / 3)
    assert want == F(5592406.0) and F(F(16777216.0) / F(3)) == F(5592405.5)
    assert M.mean(v) == want and lib_mean(v) == want
    # ... divided by (float) size, in double, rounded once: 0.1f + 0.2f + 0.4f in double, over 3
    v = [F(0.1), F(0.2), F(0.4)]
    want = F((np.float64(v[0]) + np.float64(v[1]) + np.float64(v[2])) / 3.0)
    assert M.same_float(M.mean(v), want) and M.same_float(lib_mean(v), want)


def test_deviation_is_a_float_sum():
    # mean 0 exactly; the squares are 2^24, 2^24 and six ones.  In float 2^25 + 1 rounds back to 2^25 (the spacing there is 4), six times:
    # sum 2^25, / 8 = 2^22, sqrt = 2048 exactly.  A double sum keeps the ones: 33554438 / 8 = 4194304.75, whose root 2048.000183 rounds to
    # the float after 2048 (spacing 2^-12 = 0.000244): the two widths differ in the last bit.
    v = [4096.0, -4096.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0]
    assert M.mean(v) == 0 and lib_mean(v) == 0
    wide = F(np.sqrt(np.float64(33554438.0) / 8.0))
    assert wide == np.nextafter(F(2048.0), F(np.inf))
    assert M.deviation(v) == F(2048.0) and lib_deviation(v) == F(2048.0)
    # the population form (divide by n, not n - 1), and a single value has deviation 0
    assert M.deviation([1.0, 3.0]) == F(1.0) and lib_deviation([1.0, 3.0]) == F(1.0)
    assert M.deviation([0.3]) == 0 and lib_deviation([0.3]) == 0


def test_empty_list_is_nan():
    assert np.isnan(M.mean([])) and np.isnan(M.deviation([]))
    from lgr_amd import capi
    assert np.isnan(capi.lib().lgr_measure_mean(None, 0)) and np.isnan(capi.lib().lgr_measure_deviation(None, 0, C.c_float(0.0)))


def run(success, r, t, o, cs=0.5, te=0.25):
    return dict(success=success, r_err=r, t_err=t, overlap_rmse=o, time_cs=cs, time_te=te)


def aggregate(runs):
    """measure_ref_lib.aggregate, after checking it column by column against the library's lgr_measure_mean / lgr_measure_deviation over the
    lists the reference forms (the errors of the successful runs, the times of all runs)"""
    a = M.aggregate(runs)
    ok = [r for r in runs if r["success"]]
    lists = dict(mae=[r["r_err"] for r in ok], mte=[r["t_err"] for r in ok], mrmse=[r["overlap_rmse"] for r in ok],
                 mtime=[F(r["time_cs"] + r["time_te"]) for r in runs])
    for (mean_name, values), dev_name in zip(lists.items(), ("sae", "ste", "srmse", "stime")):
        assert M.same_float(lib_mean(values), a[mean_name]), mean_name
        assert M.same_float(lib_deviation(values), a[dev_name]), dev_name
    return a


def test_all_runs_succeed():
    a = aggregate([run(True, 1.0, 2.0, 0.5), run(True, 3.0, 2.0, 1.5, te=0.75)])
    assert (a["n_times"], a["n_success"], a["success_rate"]) == (2, 2, 1.0)
    assert (a["mae"], a["sae"], a["mte"], a["ste"], a["mrmse"], a["srmse"]) == (2.0, 1.0, 2.0, 0.0, 1.0, 0.5)
    assert (a["mtime"], a["stime"]) == (1.0, 0.25)   # 0.75 and 1.25


def test_no_run_succeeds():
    a = aggregate([run(False, 1.0, 2.0, 0.5), run(False, 3.0, 2.0, np.nan), run(False, 0.0, 0.0, 0.0, cs=1.0, te=1.0)])
    assert (a["n_times"], a["n_success"], a["success_rate"]) == (3, 0, 0.0)
    for k in ("mae", "sae", "mte", "ste", "mrmse", "srmse"):
        assert np.isnan(a[k]), k
    assert a["mtime"] == F((0.75 + 0.75 + 2.0) / 3) and not np.isnan(a["stime"])   # the running times count every run


def test_failed_runs_stay_out_of_the_error_lists():
    a = aggregate([run(True, 1.0, 1.0, 1.0), run(False, 100.0, 100.0, 100.0), run(True, 3.0, 1.0, 1.0)])
    assert (a["n_success"], a["mae"], a["sae"], a["mte"], a["ste"]) == (2, 2.0, 1.0, 1.0, 0.0)
    assert M.same_float(a["success_rate"], F(2) / F(3))


def test_csv_header_and_row():
    from lgr_amd import formats
    assert formats.MEASUREMENTS_HEADER == "testname,success_rate,mae,sae,mte,ste,mrmse,srmse,mtime,stime"
    m = dict(success_rate=F(0.5), mae=F(0.1), sae=F(1e-5), mte=F(123456789.0), ste=F(np.nan), mrmse=F(0.0), srmse=F(2.5), mtime=F(1.0) / F(3.0), stime=F(12.0))
    assert formats.measurements_row("a_b_measure", m) == "a_b_measure,0.5,0.1,1e-05,1.23457e+08,nan,0,2.5,0.333333,12"
    from lgr_amd import capi
    s = capi.Measurement(n_times=4, n_success=2, success_rate=0.5, mae=0.25, sae=0.0, mte=1.5, ste=0.125, mrmse=0.0625, srmse=0.0, mtime=2.0, stime=1e-3)
    row = formats.measurements_row("x", s)
    assert row == "x,0.5,0.25,0,1.5,0.125,0.0625,0,2,0.001"
    assert len(formats.csv_row(row)) == len(formats.csv_row(formats.MEASUREMENTS_HEADER))
