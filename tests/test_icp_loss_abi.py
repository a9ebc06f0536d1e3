"""CPU suite: ICP's robust loss (include/tdv_hip.h: tdv_ctx_set_icp_loss).  The ABI refuses a null ctx; the restatement of a weighted
iteration (tests/icp_loss_restatement.py) is proven against the exact-sum oracle with L2, its weights against their definitions, and
it shows the case for the feature: on a scan with a bin floor inside a wide threshold, point-to-plane L2 misses the ground truth and
Tukey meets it.  No compute entry point of the library runs here; tests/test_gpu_icp_loss.py holds the device to this restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_loss_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32


# ---------------------------------------------------------------- ABI
def test_symbols_and_null_ctx(tdv):
    lib = tdv.lib()
    assert hasattr(lib, "tdv_ctx_set_icp_loss") and hasattr(lib, "tdv_ctx_get_icp_loss")
    assert {"tdv_ctx_set_icp_loss", "tdv_ctx_get_icp_loss"} <= set(tdv.ABI_SYMBOLS)
    k = C.c_int(-7); s = C.c_float(-7.0)
    assert lib.tdv_ctx_set_icp_loss(None, 2, C.c_float(0.01)) == TDV_ERR_BAD_ARG
    assert lib.tdv_ctx_set_icp_loss(None, 0, C.c_float(0.0)) == TDV_ERR_BAD_ARG
    assert lib.tdv_ctx_get_icp_loss(None, C.byref(k), C.byref(s)) == TDV_ERR_BAD_ARG
    assert (k.value, s.value) == (-7, -7.0)


def test_python_kinds(tdv):
    assert tdv.Context.ICP_LOSS == {"l2": 0, "huber": 1, "tukey": 2, "cauchy": 3}


# ---------------------------------------------------------------- the restatement, with L2, against the exact-sum oracle
def _problem(synth, ns, nt, seed):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(ns, seed)
    T0 = synth.perturb(T_gt, seed=seed + 1, angle_deg=2.0, trans=0.003).astype(np.float32)
    return src, tgt, nrm, T0


@pytest.mark.parametrize("iters", [1, 30])
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,nt,seed", [(300, 400, 1), (700, 300, 9), (1025, 500, 3)])
def test_l2_restatement_equals_exact_oracle(orc, synth, ns, nt, seed, p2plane, iters):
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed)
    o = orc.icp(src, tgt, nrm if p2plane else None, T0, 0.004, iters, p2plane, trace=True, exact=True)
    assert not o["ambiguous"]
    r = R.icp(orc, src, tgt, nrm, T0, 0.004, iters, p2plane, "l2")
    assert r["T"].tobytes() == o["T"].tobytes()
    assert r["rmse"].tobytes() == o["rmse"].tobytes() and r["fitness"].tobytes() == o["fitness"].tobytes()
    assert r["iterations"] == o["iterations"] and r["n_corr"] == int(o["trace"][-1, 18])
    if iters > 1:
        assert r["iterations"] >= 3


# ---------------------------------------------------------------- weights
def test_tukey_weights():
    k = F(0.002)
    w = R.weight("tukey", k, np.array([0.0, k, -k, np.nextafter(k, F(1)), 0.01, -0.5 * k], F))
    assert w.dtype == F
    assert w[0] == 1.0 and w[1] == 0.0 and w[2] == 0.0 and w[3] == 0.0 and w[4] == 0.0
    assert w[5] == F(F(1) - F(0.25)) ** 2 and w[5] == F(0.5625)


def test_huber_weights():
    k = F(0.003)
    below, above = np.nextafter(k, F(0)), np.nextafter(k, F(1))
    w = R.weight("huber", k, np.array([0.0, below, k, above, -2 * k, 4 * k], F))
    assert list(w[:3]) == [1.0, 1.0, 1.0]
    assert w[3] == F(k / above) and 1.0 - 1e-6 < w[3] < 1.0          # continuous at k: one ulp past it, one ulp under 1
    assert w[4] == F(0.5) and w[5] == F(0.25)


def test_cauchy_weights():
    k = F(0.0015)
    w = R.weight("cauchy", k, np.array([0.0, k, -k, 3 * k], F))
    assert w[0] == 1.0 and w[1] == F(0.5) and w[2] == F(0.5)
    assert abs(float(w[3]) - 0.1) < 1e-6


def test_l2_weights_are_one():
    assert np.all(R.weight("l2", 0.0, np.array([0.0, 1.0, -3.0], F)) == 1.0)


# ---------------------------------------------------------------- the scenario
@pytest.fixture(scope="module")
def scene(synth):
    return R.clutter_scene(synth)


def test_scenario_l2_misses_tukey_meets(orc, synth, scene):
    """Point-to-plane from a start 2 deg / 3 mm off, threshold 10 mm, a bin floor 4 mm under the part: L2 settles towards the floor, Tukey
    (2.5 mm) ignores it.  Gate: 2e-3 rad and 0.5 mm from the ground truth."""
    src, tgt, nrm, T0, T_gt = scene
    S = R.SCENE
    assert not R.within_gate(synth, T0, T_gt)[0]
    l2 = R.icp(orc, src, tgt, nrm, T0, S["thr"], S["iterations"], True, "l2")
    tk = R.icp(orc, src, tgt, nrm, T0, S["thr"], S["iterations"], True, "tukey", S["tukey_scale"])
    ok_l2, err_l2 = R.within_gate(synth, l2["T"], T_gt)
    ok_tk, err_tk = R.within_gate(synth, tk["T"], T_gt)
    assert not ok_l2, err_l2
    assert ok_tk, err_tk
    assert err_l2[1] > 2 * S["gate_m"]                    # not a near miss: L2 is biased by the floor
    assert 3 <= tk["iterations"] < S["iterations"] and 3 <= l2["iterations"] < S["iterations"]   # both stopped by the rule, not the cap
    n_corr, n_eff = tk["counts"][-1]
    assert n_eff < n_corr                                 # the floor is accepted by the threshold and weighted out


def test_n_eff_break(orc, synth, scene):
    """Tukey with a scale far below every residual: accepted correspondences, none with weight > 0 - no update, pose kept."""
    src, tgt, nrm, T0, _ = scene
    r = R.icp(orc, src, tgt, nrm, T0, R.SCENE["thr"], 5, True, "tukey", 1e-9)
    assert r["iterations"] == 0 and r["T"].tobytes() == np.asarray(T0, np.float32).tobytes()
    assert r["counts"][0][0] >= 3 and r["counts"][0][1] < 3 and len(r["counts"]) == 1
    rf = R.icp(orc, src, tgt, nrm, T0, R.SCENE["thr"], 5, True, "tukey", 1e-9, fixed=True)
    assert rf["iterations"] == 0 and len(rf["counts"]) == 5
    assert math.isfinite(float(rf["rmse"]))
