"""CPU suite: colored ICP (include/tdv_hip.h: tdv_color_gradients, tdv_colored_icp).  The ABI exports the five entry points and refuses a
null ctx; the restatement (tests/colored_icp_restatement.py) is proven against f64 evaluations of its definition: the gradients are the
least-squares solution of their rows and recover a linear ramp's slope, the terms are J^T J and J^T r of the two rows, lambda = 1 is
point-to-plane, and on the textured lid colored ICP ends near the ground truth where point-to-plane does not.  No compute entry point of
the library runs here; tests/test_gpu_colored_icp.py holds the device to this restatement."""
import ctypes as C

import numpy as np
import pytest

import colored_icp_restatement as R
import icp_loss_restatement as L

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_color_gradients", "tdv_color_gradients_dev", "tdv_colored_icp", "tdv_colored_icp_dev", "tdv_colored_icp_batch_dev")

# The textured lid (colored_icp_restatement.SCENE, seed 1): the start is 3 deg / 11.9 mm (the pose's translation) off.  Colored ICP (lambda 0.968) ends 0.76 mrad /
# 0.36 mm off, point-to-plane 20 mrad / 4.2 mm.  Over seeds 1-3 colored ICP ended within 0.9 mrad / 0.45 mm and point-to-plane 8-20 mrad.
COLORED_BOUND = (1.5e-3, 1.0e-3)      # rad, m: colored ICP ends within both
PLANE_FLOOR = 5e-3                    # rad: point-to-plane ends at least this far off in rotation


def textured(orc):
    S = R.SCENE
    src, rgb, tgt, nrm, T0, T_gt = R.lid_scene(S["seed"])
    return src, rgb, tgt, nrm, R.lid_target_color(orc), T0, T_gt


# ---------------------------------------------------------------- ABI
def test_symbols_and_null_ctx(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    pts = np.zeros((4, 4), F); T0 = (C.c_float * 16)(*tdv.to_colmajor16(np.eye(4)))
    p = pts.ctypes.data_as(C.c_void_p)
    out = tdv.IcpResultC(); C.memset(C.byref(out), 0x5A, C.sizeof(out)); before = bytes(out)
    assert lib.tdv_color_gradients(None, p, p, p, 4, 3, p) == TDV_ERR_BAD_ARG
    assert lib.tdv_color_gradients_dev(None, p, p, p, 4, 3, None, p) == TDV_ERR_BAD_ARG
    assert lib.tdv_colored_icp(None, p, p, 4, p, p, p, 4, T0, C.c_float(0.01), 10, C.c_float(0.968), C.byref(out)) == TDV_ERR_BAD_ARG
    assert lib.tdv_colored_icp_dev(None, p, p, 4, p, p, p, 4, T0, C.c_float(0.01), 10, C.c_float(0.968), 0, C.byref(out)) == TDV_ERR_BAD_ARG
    off = (C.c_int * 2)(0, 4)
    assert lib.tdv_colored_icp_batch_dev(None, p, p, off, 1, p, p, p, 4, T0, C.c_float(0.01), 10, C.c_float(0.968), 0,
                                         C.byref(out)) == TDV_ERR_BAD_ARG
    assert bytes(out) == before


# ---------------------------------------------------------------- gradients
def _cloud(rng, n=600):
    """A gently curved patch with random normals-ish jitter and colours."""
    xy = rng.uniform(-0.05, 0.05, (n, 2))
    z = 0.2 * xy[:, 0] ** 2 - 0.1 * xy[:, 0] * xy[:, 1]
    return np.c_[xy, z].astype(F), rng.uniform(0, 1, (n, 3)).astype(F)


def test_gradients_are_the_least_squares_solution(orc):
    rng = np.random.default_rng(4)
    xyz, rgb = _cloud(rng)
    nrm, knn = orc.estimate_normals(xyz, R.K, want_knn=True)
    g = R.gradients(xyz, rgb, nrm, knn)
    I = R.intensity(rgb)
    assert np.array_equal(g[:, 0], I)
    worst = 0.0
    for i in range(len(xyz)):
        js = [j for j in knn[i] if j >= 0 and j != i]
        assert len(js) >= 3
        n = nrm[i].astype(np.float64)
        # the rows in f64 from the same f32 u_j, b_j: the tangent projections, then the m n row with right-hand side 0
        d = (xyz[js] - xyz[i]).astype(F)
        t = (d[:, 0] * nrm[i, 0] + (d[:, 1] * nrm[i, 1] + d[:, 2] * nrm[i, 2])).astype(F)
        u = (d - t[:, None] * nrm[i]).astype(np.float64)
        b = (I[js] - I[i]).astype(F).astype(np.float64)
        A = np.vstack([u, len(js) * n]); rhs = np.r_[b, 0.0]
        sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
        worst = max(worst, np.abs(g[i, 1:] - sol).max() / max(1.0, np.abs(sol).max()))
    assert worst <= 1e-5, worst


def test_gradients_recover_a_ramp():
    """A plane tilted in space with I linear along it: d is the ramp's slope on the plane, exactly up to f32."""
    rng = np.random.default_rng(5)
    n = 800
    uv = rng.uniform(-0.05, 0.05, (n, 2))
    e1 = np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0); e2 = np.array([0.0, 1.0, 0.0]); nn = np.cross(e1, e2)
    xyz = (uv[:, :1] * e1 + uv[:, 1:] * e2 + np.array([0.0, 0.0, 0.5])).astype(F)
    slope = 3.0 * e1 - 2.0 * e2                         # dI / dx on the plane, per metre
    I = 0.5 + (xyz.astype(np.float64) - [0.0, 0.0, 0.5]) @ slope
    rgb = np.repeat(I[:, None], 3, 1).astype(F)
    nrm = np.broadcast_to(nn, (n, 3)).astype(F)
    d2 = ((xyz[:, None, :].astype(np.float64) - xyz[None, :, :]) ** 2).sum(-1)
    knn = np.argsort(d2, axis=1, kind="stable")[:, :R.K]
    g = R.gradients(xyz, rgb, nrm, knn)
    err = np.abs(g[:, 1:] - slope).max()
    assert err <= 2e-3 * np.abs(slope).max(), err
    few = R.gradients(xyz[:3], rgb[:3], nrm[:3], np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1]]))   # m = 2 < 3: d = 0
    assert np.all(few[:, 1:] == 0)


# ---------------------------------------------------------------- the terms
def _rows(orc, synth, lam=R.LAMBDA):
    rng = np.random.default_rng(6)
    src, T_gt = synth.make_scene(1500, 7)
    tgt, nrm = synth.sample_object(2000, 7)
    tc = R.gradients_of(orc, tgt, rng.uniform(0, 1, (len(tgt), 3)).astype(F), nrm)
    srgb = rng.uniform(0, 1, (len(src), 3)).astype(F)
    T = synth.perturb(T_gt, seed=8, angle_deg=2.0, trans=0.003).astype(F)
    c = orc.icp_correspondences(src, tgt, None, T, 0.01, False)
    acc = c["accepted"]; idx = c["corr"][acc]
    p = L.transform(T, src)[acc]
    lg, lc = R.weights_of_lambda(lam)
    return p, tgt[idx], nrm[idx], tc[idx], R.intensity(srgb)[acc], lg, lc, (src, srgb, tgt, nrm, tc, T)


def test_terms_are_jtj_and_jtr(orc, synth):
    p, q, n, tc, Is, lg, lc, _ = _rows(orc, synth)
    assert len(p) > 500
    t = R.terms(*R.rows(p, q, n, tc, Is, lg, lc))
    # f64 from the same f32 inputs
    P, Q, N, D = (a.astype(np.float64) for a in (p, q, n, tc[:, 1:]))
    lgd, lcd = float(lg), float(lc)
    e = P - Q
    en = (e * N).sum(1)
    et = e - en[:, None] * N
    m = D - (D * N).sum(1)[:, None] * N
    JG = lgd * np.c_[np.cross(P, N), N]; rG = lgd * en
    JC = lcd * np.c_[np.cross(P, -m), -m]; rC = lcd * (Is - (tc[:, 0] + (D * et).sum(1)))
    H = JG.T @ JG + JC.T @ JC
    v = JG.T @ rG + JC.T @ rC
    Hs = np.array([H[a, b] for a in range(6) for b in range(a, 6)])
    got = t.sum(0)
    assert np.abs(got[:21] - Hs).max() <= 1e-5 * np.abs(Hs).max(), np.abs(got[:21] - Hs).max() / np.abs(Hs).max()
    assert np.abs(got[21:] - v).max() <= 1e-5 * np.abs(v).max(), np.abs(got[21:] - v).max() / np.abs(v).max()


def test_lambda_one_is_point_to_plane(orc, synth):
    """lambda = 1: lg = 1, lc = 0 - the terms, the sums and the loop equal point-to-plane's in value."""
    _, _, _, _, _, lg, lc, (src, srgb, tgt, nrm, tc, T) = _rows(orc, synth, 1.0)
    assert lg == 1 and lc == 0
    for kind, k in (("l2", 0.0), ("huber", 0.002)):
        a = R.iteration_sums(orc, src, srgb, tgt, nrm, tc, T, 0.01, 1.0, kind, k)
        b = L.iteration_sums(orc, src, tgt, nrm, T, 0.01, True, kind, k)
        assert np.array_equal(a["ATA"], b["ATA"]) and np.array_equal(a["ATb"], b["ATb"]) and a["te"] == b["te"], kind
    r = R.colored_icp(orc, src, srgb, tgt, nrm, tc, T, 0.01, 20, 1.0)
    q = L.icp(orc, src, tgt, nrm, T, 0.01, 20, True, "l2")
    assert np.array_equal(r["T"], q["T"]) and r["rmse"] == q["rmse"] and (r["iterations"], r["n_corr"]) == (q["iterations"], q["n_corr"])


def test_robust_weights_per_row(orc, synth):
    """Tukey: each row is weighted by its own residual; n_eff counts a correspondence when either row keeps a weight."""
    p, q, n, tc, Is, lg, lc, _ = _rows(orc, synth)
    JG, rG, JC, rC = R.rows(p, q, n, tc, Is, lg, lc)
    wG = L.weight("tukey", 0.002, rG); wC = L.weight("tukey", 0.002, rC)
    t = R.terms(JG, rG, JC, rC, wG, wC)
    assert (wG == 0).any() and (wC == 0).any() and ((wG > 0) != (wC > 0)).any()
    k = 2                                              # slot of H02
    ref = wG.astype(np.float64) * (JG[:, 0] * JG[:, 2]).astype(np.float64) + wC.astype(np.float64) * (JC[:, 0] * JC[:, 2]).astype(np.float64)
    assert np.array_equal(t[:, k], ref)


# ---------------------------------------------------------------- the textured scene
def test_gradients_on_the_lid_follow_the_texture(orc):
    tgt, nrm, rgb = R.lid_model()
    tc = R.lid_target_color(orc)
    top = (tgt[:, 2] == 0) & (np.abs(tgt[:, :2]).max(1) < 0.04)
    x = tgt[top].astype(np.float64); w = 2 * np.pi / R.WAVE
    slope = 0.25 * w * np.c_[np.cos(w * x[:, 0]) * np.sin(w * x[:, 1]), np.sin(w * x[:, 0]) * np.cos(w * x[:, 1])]
    # The fit follows the slope's direction everywhere; its size is the slope averaged over the 30 neighbours (about 7.7 mm around the
    # point on this 2.5 mm grid, a quarter of the wavelength), which the sinusoid shrinks to 0.63 of the point's own.
    for a in range(2):
        assert np.corrcoef(tc[top, 1 + a], slope[:, a])[0, 1] > 0.99
    gain = (tc[top, 1:3] * slope).sum() / (slope * slope).sum()
    assert 0.55 < gain < 0.7, gain
    assert np.all(tc[top, 3] == 0)


def test_textured_scene_colored_beats_point_to_plane(orc, synth):
    S = R.SCENE
    src, rgb, tgt, nrm, tc, T0, T_gt = textured(orc)
    c = R.colored_icp(orc, src, rgb, tgt, nrm, tc, T0, S["thr"], S["iterations"])
    p = L.icp(orc, src, tgt, nrm, T0, S["thr"], S["iterations"], True, "l2")
    ec, ep, e0 = synth.pose_error(c["T"], T_gt), synth.pose_error(p["T"], T_gt), synth.pose_error(T0, T_gt)
    assert e0[0] > 0.05 and e0[1] > 0.005, e0
    assert ec[0] <= COLORED_BOUND[0] and ec[1] <= COLORED_BOUND[1], ec
    assert ep[0] > PLANE_FLOOR, ep
    assert c["iterations"] < S["iterations"] and not c["ambiguous"]
