"""A numpy restatement of the aggregates of the measure test type (measureTestResults, reference src/main.cpp:345-380, with
calculateMean / calculateStandardDeviation of include/utils.h:68-88 for float), the yardstick of lgr_measure*:

  * mean: std::accumulate from the DOUBLE 0.0 in list order, divided by (float) size (a double division), returned as float;
  * deviation: the FLOAT sum of (x - mean) * (x - mean) in list order, then std::sqrt(sum / (float) size): the population form;
  * an empty list gives quiet NaN for both;
  * a run succeeds when it converged and its overlap error is below distance_thr; the error lists hold the successful runs in run order, the
    running-time list (float) (time_cs + time_te) of every run; success_rate = (float) n_success / (float) n_times.
"""
import numpy as np

F = np.float32
FIELDS = ("success_rate", "mae", "sae", "mte", "ste", "mrmse", "srmse", "mtime", "stime")


def mean(values):
    v = [F(x) for x in values]
    if not v:
        return F(np.nan)
    s = np.float64(0.0)
    for x in v:
        s = s + np.float64(x)
    return F(s / np.float64(F(len(v))))


def deviation(values):
    v = [F(x) for x in values]
    if not v:
        return F(np.nan)
    m = mean(v)
    d = F(0.0)
    for x in v:
        d = F(d + F(F(x - m) * F(x - m)))
    return F(np.sqrt(F(d / F(len(v)))))


def aggregate(runs):
    """runs: one dict per run with success (bool), r_err, t_err, overlap_rmse (floats) and time_cs, time_te (doubles), in run order.
    Returns a dict of n_times, n_success and the nine float32 columns of test_measurements.csv."""
    ok = [r for r in runs if r["success"]]
    out = dict(n_times=len(runs), n_success=len(ok), success_rate=F(F(len(ok)) / F(len(runs))))
    for mname, sname, lst in (("mae", "sae", [r["r_err"] for r in ok]), ("mte", "ste", [r["t_err"] for r in ok]),
                              ("mrmse", "srmse", [r["overlap_rmse"] for r in ok]),
                              ("mtime", "stime", [F(np.float64(r["time_cs"]) + np.float64(r["time_te"])) for r in runs])):
        out[mname], out[sname] = mean(lst), deviation(lst)
    return out


def same_float(x, y):
    x, y = F(x), F(y)
    return bool((np.isnan(x) and np.isnan(y)) or x.view(np.uint32) == y.view(np.uint32))
