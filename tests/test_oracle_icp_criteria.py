"""CPU suite: the oracle's ICP with the call's convergence criteria (oracle/oracle.cpp: orc_icp_criteria; csrc/icp.hip: icp_update).
With the reference's bounds (+inf, 1e-6f) the new entry is orc_icp_ex - and orc_icp in the float mode - byte for byte, trace included,
in both sum modes, on the golden suite's ICP scene and on the exact-sum suite's; FLT_MAX for the fitness bound is +inf (two fitness
values lie in [0, 1]); and the rule itself is held to the trace of a run it never fires in."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_oracle_exact_sums import _scene

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FLT_MAX = float(np.finfo(F).max)
ITERS = 40


def _fixtures(synth):
    p = json.load(open(os.path.join(HERE, "golden", "meta.json")))["params"]
    tgt, nrm = synth.sample_object(512, 7)
    src, T_gt = synth.make_scene(p["n"], 7)
    yield "golden", src, tgt, nrm, synth.perturb(T_gt, 7).astype(F), p["icp_thr"]
    src, tgt, nrm, T0 = _scene(synth, 600, 500, 3)
    yield "exact sums", src, tgt, nrm, T0, 0.004


def _raw(orc, entry, src, tgt, nrm, T0, thr, p2plane, exact, bounds=None):
    """One call of an exported entry on its own buffers: every byte it wrote, and its return value."""
    lib = orc.lib()
    src, tgt, nrm = (np.ascontiguousarray(a, F) for a in (src, tgt, nrm))
    T = np.full(16, 7, F); tr = np.full((ITERS, 20), 7, F); fit = C.c_float(7); rmse = C.c_float(7); amb = C.c_int(7)
    t0 = orc.to_colmajor16(T0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(src), len(src), p(tgt), p(nrm), len(tgt), p(t0), C.c_float(thr), ITERS, int(p2plane), p(T), C.byref(fit), C.byref(rmse), p(tr)]
    if entry != "orc_icp":
        args += [int(exact), C.byref(amb)]
    if bounds is not None:
        args += [C.c_float(bounds[0]), C.c_float(bounds[1])]
    fn = getattr(lib, entry); fn.restype = C.c_int
    it = fn(*args)
    return (T.tobytes(), tr.tobytes(), F(fit.value).tobytes(), F(rmse.value).tobytes(), amb.value, it)


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("exact", [False, True])
def test_default_bounds_are_orc_icp_ex_to_the_byte(orc, synth, exact, p2plane):
    for name, src, tgt, nrm, T0, thr in _fixtures(synth):
        old = _raw(orc, "orc_icp_ex", src, tgt, nrm, T0, thr, p2plane, exact)
        assert 2 <= old[-1] <= ITERS, (name, old[-1])
        assert _raw(orc, "orc_icp_criteria", src, tgt, nrm, T0, thr, p2plane, exact, (np.inf, 1e-6)) == old, name
        assert _raw(orc, "orc_icp_criteria", src, tgt, nrm, T0, thr, p2plane, exact, (FLT_MAX, 1e-6)) == old, name
        if not exact:
            plain = _raw(orc, "orc_icp", src, tgt, nrm, T0, thr, p2plane, exact)
            assert plain[:4] + plain[5:] == old[:4] + old[5:], name
        # ... and pyoracle.icp's defaults go through the new entry
        r = orc.icp(src, tgt, nrm, T0, thr, ITERS, p2plane, trace=True, exact=exact)
        assert (r["T"].tobytes(), r["iterations"]) == (orc.from_colmajor16(np.frombuffer(old[0], F)).tobytes(), old[-1]), name
        assert np.ascontiguousarray(r["trace"]).tobytes() == old[1][:80 * old[-1]], name


def _stop(trace, rf, rr):
    """The rule on a recorded trace (rmse in column 16, fitness in 17): the first k >= 2 whose two differences are below their bounds."""
    for k in range(2, len(trace) + 1):
        if abs(F(trace[k - 2, 17] - trace[k - 1, 17])) < F(rf) and abs(F(trace[k - 2, 16] - trace[k - 1, 16])) < F(rr):
            return k
    return len(trace)


@pytest.mark.parametrize("exact", [False, True])
def test_the_rule_stops_where_the_free_run_says(orc, synth, exact):
    for name, src, tgt, nrm, T0, thr in _fixtures(synth):
        free = orc.icp(src, tgt, nrm, T0, thr, 12, True, trace=True, exact=exact, relative_rmse=0.0)
        assert free["iterations"] == 12, name          # |d rmse| < 0 never holds
        tr = free["trace"]
        d = np.abs(np.diff(tr[:, 16]).astype(F))
        for rf, rr in ((np.inf, float(d[2])), (np.inf, float(np.nextafter(d[2], F(np.inf)))), (np.inf, np.inf), (1e-3, np.inf), (1e-3, float(d[1]) * 2)):
            k = _stop(tr, rf, rr)
            got = orc.icp(src, tgt, nrm, T0, thr, 12, True, trace=True, exact=exact, relative_fitness=rf, relative_rmse=rr)
            assert got["iterations"] == k, (name, rf, rr, got["iterations"], k)
            assert got["trace"].tobytes() == tr[:k].tobytes() and got["T"].tobytes() == orc.from_colmajor16(tr[k - 1, :16]).tobytes(), (name, rf, rr)
        assert _stop(tr, np.inf, np.inf) == 2
