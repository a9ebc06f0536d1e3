"""CPU suite: generalized ICP (include/tdv_hip.h: tdv_gicp).  The ABI exports the three entry points and refuses a null ctx; the
restatement of a GICP iteration (tests/gicp_restatement.py) is proven against f64 evaluations of its definition, it reaches the ground
truth on a noiseless scene, and it shows a scene where GICP lands nearer the ground truth than point-to-plane.  No compute entry point of
the library runs here; tests/test_gpu_gicp.py holds the device to this restatement."""
import ctypes as C

import numpy as np
import pytest

import gicp_restatement as G
import icp_loss_restatement as L

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_gicp", "tdv_gicp_dev", "tdv_gicp_batch_dev")

# The scenario: a start 8 deg / 5 mm off the ground truth, threshold 20 mm, 30 iterations at most, source normals estimated
# from the scan (k = 30).  GICP ends nearer the ground truth than point-to-plane in rotation and translation.  It is not the rule on these
# scenes: among the scenes tried (sensor noise, a bin floor, starts 5 and 8 deg off; two seeds each) GICP was nearer in four of nine.
SCENARIO = dict(n_scan=2000, n_model=3000, seed=2, angle=8.0, trans=0.005, thr=0.02, iterations=30)


def scenario(orc, synth, n_scan=None, n_model=None):
    S = SCENARIO
    tgt, nrm = synth.sample_object(n_model or S["n_model"], S["seed"])
    src, T_gt = synth.make_scene(n_scan or S["n_scan"], S["seed"])
    sn = orc.estimate_normals(src)
    T0 = synth.perturb(T_gt, seed=S["seed"] + 1, angle_deg=S["angle"], trans=S["trans"]).astype(F)
    return src, sn, tgt, nrm, T0, T_gt


def exact_scene(synth, n=2000, seed=42):
    """The model itself seen from the inverse ground truth, normals rotated with it: a correspondence's residual is 0 at the truth."""
    tgt, nrm = synth.sample_object(n, seed)
    T_gt = synth.gt_transform(seed)
    Ti = np.linalg.inv(T_gt.astype(np.float64))
    src = (tgt.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    sn = (nrm.astype(np.float64) @ Ti[:3, :3].T).astype(F)
    return src, sn, tgt, nrm, T_gt


# ---------------------------------------------------------------- ABI
def test_symbols_and_null_ctx(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    pts = np.zeros((4, 3), F); T0 = (C.c_float * 16)(*tdv.to_colmajor16(np.eye(4)))
    p = pts.ctypes.data_as(C.c_void_p)
    out = tdv.IcpResultC(); C.memset(C.byref(out), 0x5A, C.sizeof(out)); before = bytes(out)
    assert lib.tdv_gicp(None, p, p, 4, p, p, 4, T0, C.c_float(0.01), 10, C.c_float(1e-3), C.byref(out)) == TDV_ERR_BAD_ARG
    assert lib.tdv_gicp_dev(None, p, p, 4, p, p, 4, T0, C.c_float(0.01), 10, C.c_float(1e-3), 0, C.byref(out)) == TDV_ERR_BAD_ARG
    off = (C.c_int * 2)(0, 4)
    assert lib.tdv_gicp_batch_dev(None, p, p, off, 1, p, p, 4, T0, C.c_float(0.01), 10, C.c_float(1e-3), 0, C.byref(out)) == TDV_ERR_BAD_ARG
    assert bytes(out) == before


# ---------------------------------------------------------------- the restatement against f64 evaluations of its definition
def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.parametrize("epsilon", [1e-3, 0.1, 1.0])
def test_inverse_matches_numpy(epsilon):
    rng = np.random.default_rng(int(epsilon * 1000))
    k = 20000
    a = _unit(rng, k); n = _unit(rng, k)
    a[::7] = 0.0; n[::11] = 0.0                               # zero normals: that cloud's covariance is I
    a[3::13] = n[3::13]; a[4::17] = -n[4::17]                 # parallel normals: C's condition number is 1 / epsilon
    a = a.astype(F); n = n.astype(F)
    C_ = G.covariance(a, n, F(F(1) - F(epsilon)))
    M = G.full(G.inverse(C_), "M").astype(np.float64)
    Mi = np.linalg.inv(G.full(C_, "C").astype(np.float64))
    rel = np.abs(M - Mi).max(axis=(1, 2)) / np.abs(Mi).max(axis=(1, 2))
    assert rel.max() <= 1e-5, rel.max()
    both0 = (np.abs(a).sum(1) == 0) & (np.abs(n).sum(1) == 0)
    assert both0.any() and np.all(M[both0] == 0.5 * np.eye(3))


def test_sums_match_f64(orc, synth):
    src, T_gt = synth.make_scene(1500, 7)
    tgt, nrm = synth.sample_object(2000, 7)
    sn = orc.estimate_normals(src)
    T = synth.perturb(T_gt, seed=8, angle_deg=2.0, trans=0.003).astype(F)
    s = G.iteration_sums(orc, src, sn, tgt, nrm, T, 0.01)
    assert s["n_corr"] > 500
    # f64 from the same f32 inputs: p, a = R ns and the correspondences; M = inv(C) in f64, J = [-[p]x | I]
    c = orc.icp_correspondences(src, tgt, None, T, 0.01, False)
    acc = c["accepted"]; idx = c["corr"][acc]
    p = L.transform(T, src)[acc].astype(np.float64)
    a = G.rotate(T, sn[acc]).astype(np.float64)
    q = tgt[idx].astype(np.float64); nt = nrm[idx].astype(np.float64)
    cc = 1.0 - 1e-3
    Cm = 2.0 * np.eye(3) - cc * (a[:, :, None] * a[:, None, :] + nt[:, :, None] * nt[:, None, :])
    M = np.linalg.inv(Cm)
    px = np.zeros((len(p), 3, 3))
    px[:, 0, 1], px[:, 0, 2], px[:, 1, 2] = -p[:, 2], p[:, 1], -p[:, 0]
    px[:, 1, 0], px[:, 2, 0], px[:, 2, 1] = p[:, 2], -p[:, 1], p[:, 0]
    J = np.concatenate([-px, np.broadcast_to(np.eye(3), px.shape)], 2)
    H = np.einsum("kia,kij,kjb->ab", J, M, J)
    v = np.einsum("kia,kij,kj->a", J, M, p - q)
    assert np.abs(s["ATA"] - H).max() <= 1e-4 * np.abs(H).max(), np.abs(s["ATA"] - H).max() / np.abs(H).max()
    assert np.abs(s["ATb"] - v).max() <= 1e-4 * np.abs(v).max(), np.abs(s["ATb"] - v).max() / np.abs(v).max()


def test_terms_are_point_to_plane_in_the_limit(orc, synth):
    """epsilon = 1 (C = 2 I - 0 = 2 I): M = I / 2 and H, v are half point-to-point's linearisation; epsilon -> 0 with a source normal
    equal to the target's: M -> n n^T / (2 epsilon) + ..., so 2 epsilon H's rotation block approaches point-to-plane's J^T J."""
    rng = np.random.default_rng(3)
    p = rng.uniform(-0.1, 0.1, (50, 3)).astype(F); q = (p + rng.normal(0, 1e-3, (50, 3))).astype(F)
    n = _unit(rng, 50).astype(F)
    t, _ = G.terms(p, q, n, n, F(0.0))
    assert np.all(t[:, 15] == F(0.5)) and np.all(t[:, 16] == 0) and np.all(t[:, 20] == F(0.5))   # H33, H34, H55
    eps = F(1e-4)
    t, _ = G.terms(p, q, n, n, F(F(1) - eps))
    J = np.concatenate([np.cross(p.astype(np.float64), n), n], 1)
    k = 0
    for a_ in range(6):
        for b in range(a_, 6):
            got = 2 * float(eps) * t[:, k].astype(np.float64)
            assert np.allclose(got, J[:, a_] * J[:, b], rtol=0, atol=2e-3 * (1 + np.abs(J[:, a_] * J[:, b]).max())), (a_, b)
            k += 1


# ---------------------------------------------------------------- convergence and the scenario
def test_noiseless_scene_reaches_ground_truth(orc, synth):
    src, sn, tgt, nrm, T_gt = exact_scene(synth)
    T0 = synth.perturb(T_gt, seed=43, angle_deg=2.0, trans=0.003).astype(F)
    r = G.gicp(orc, src, sn, tgt, nrm, T0, 0.01, 60)
    ang, tr = synth.pose_error(r["T"], T_gt)
    assert ang <= 1e-5 and tr <= 1e-6, (ang, tr)
    assert 3 <= r["iterations"] < 60 and not r["ambiguous"]


def test_scenario_gicp_nearer_than_point_to_plane(orc, synth):
    src, sn, tgt, nrm, T0, T_gt = scenario(orc, synth)
    S = SCENARIO
    g = G.gicp(orc, src, sn, tgt, nrm, T0, S["thr"], S["iterations"])
    p = L.icp(orc, src, tgt, nrm, T0, S["thr"], S["iterations"], True, "l2")
    eg, ep = synth.pose_error(g["T"], T_gt), synth.pose_error(p["T"], T_gt)
    assert eg[0] < 0.8 * ep[0] and eg[1] < 0.8 * ep[1], (eg, ep)
    assert g["iterations"] < S["iterations"] and p["iterations"] < S["iterations"]     # both stopped by the rule, not the cap
