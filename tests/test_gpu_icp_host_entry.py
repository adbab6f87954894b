"""Host entry point == its _dev twin, byte for byte, for the point-to-plane ICP: lgr_icp_plane_host against lgr_icp_plane_dev under the rule
and with the machinery of tests/test_gpu_host_entries.py (its Side / Case classes, its data, its cases): equal return codes and
byte-identical result, trace and count in the `full` case, with the trace `absent`, with an empty and a one-point source, with an empty and
a one-point target (both forms refuse), and the host form's own refusal of a NULL source under a positive count."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_host_entries as H  # noqa: E402

pytestmark = pytest.mark.gpu
NAME, TWIN = "lgr_icp_plane_host", "lgr_icp_plane_dev"
MAX_IT = 3


def icp_row(s, d):
    from lgr_amd import capi
    ps, ns, pt, nt = H.clouds(s, d)
    opt = not s.case.absent
    ip = capi.icp_params(max_iterations=MAX_IT)   # max_dist 0: the density is computed on both sides
    s.alive.append(ip)
    s.call(NAME, "pipippppp", ps, ns, pt, nt, s.host(d.T), C.addressof(ip), s.hout("out", capi.IcpResult()), s.hout("trace", (capi.IcpStep * MAX_IT)(), opt),
           s.hout("n_trace", C.c_int(-7), opt), twin=TWIN)


@pytest.mark.parametrize("case", [pytest.param(c, id=str(c)) for c in H.cases_of(("ns", "nt"), True)])
def test_icp_host_form_equals_dev_twin(lgr, case):
    from lgr_amd import capi
    d = H.data(lgr)
    host = H.Side(lgr, False, case)
    icp_row(host, d)
    got = host.results()
    if case.kind == "null":
        assert host.rc == -1
        return
    dev = H.Side(lgr, True, case)
    icp_row(dev, d)
    want = dev.results()
    print(f"{NAME} {case}: rc host {host.rc} twin {dev.rc}, outputs {sorted(got)}")
    assert host.rc == dev.rc
    refused = case.which == "nt"   # fewer than two target points
    assert host.rc == (-1 if refused else 0)
    if refused:
        return
    assert sorted(got) == sorted(want) == (["n_trace", "out", "trace"] if not case.absent else ["out"])
    for k in got:
        assert got[k] == want[k], f"{NAME}: output {k!r} differs between the host form and the twin"
    out = capi.IcpResult.from_buffer_copy(got["out"])
    if case.which == "ns":   # an empty source: nothing computed; one point: one iteration without six pairs
        assert (out.iterations, out.stop) == (0, capi.ICP_STOP_NO_PAIRS) and out.pairs <= 1
    else:
        assert out.iterations == MAX_IT and out.pairs0 > H.N_CLOUD // 8 and out.max_dist > 0   # not vacuous
