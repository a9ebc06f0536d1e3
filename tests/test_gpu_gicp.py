"""Generalized ICP on the device (include/tdv_hip.h: tdv_gicp), against the restatement of tests/gicp_restatement.py.

The terms are f32 in the header's order and exact in f64 after the weight; their tree sums round to the exact sums' f32 unless exact_sum
reports an ambiguity, so T, rmse, fitness, iterations and n_corr must be the restatement's bytes on every search path and batch path.
Every test runs on a Context of its own."""
import ctypes as C

import numpy as np
import pytest
import torch

import gicp_restatement as G
import icp_loss_restatement as L
from test_gicp_abi import SCENARIO, exact_scene, scenario

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
LOSSES = {"l2": 0.0, "tukey": 0.1}
PATHS = {   # search mode, TDV_ICP_SMALL, expected search
    "small": ("auto", None, "brute"),
    "brute": ("brute", "0", "brute"),
    "pruned": ("pruned", None, "pruned"),
    "grid": ("grid", None, "grid"),
}


@pytest.fixture
def gctx(tdv, monkeypatch):
    c = tdv.Context(0)
    yield c, monkeypatch
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 3), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def _normals(orc, src, seed):
    """Estimated normals (k = 30) where the cloud allows, else random unit ones; every 9th zero (covariance I)."""
    if len(src) > 30:
        n = orc.estimate_normals(src)
    else:
        v = np.random.default_rng(seed).normal(size=(max(len(src), 1), 3))
        n = (v / np.linalg.norm(v, axis=1, keepdims=True))[:len(src)]
    n = np.asarray(n, F).copy()
    n[::9] = 0.0
    return n


def _problem(orc, synth, ns, nt, seed=42, angle=2.0, trans=0.003):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(max(ns, 1), seed)
    src = src[:ns].copy()
    T0 = synth.perturb(T_gt, seed=seed + 1, angle_deg=angle, trans=trans).astype(F)
    return src, _normals(orc, src, seed), tgt, nrm, T0


def _set_path(ctx, mp, path):
    search, small, _ = PATHS[path]
    ctx.set_icp_search(search)
    if small is None:
        mp.delenv("TDV_ICP_SMALL", raising=False)
    else:
        mp.setenv("TDV_ICP_SMALL", small)


def _gicp_dev(ctx, src, sn, tgt, nrm, T0, thr, iters, fixed=False, eps=G.EPSILON):
    ks, ps = _up(src); kn, pn = _up(sn); kt, pt = _up(tgt); km, pm = _up(nrm)
    return ctx.gicp_dev(ps, pn, len(src), pt, pm, len(tgt), T0, thr, iters, eps, fixed)


def _icp_dev(ctx, src, tgt, nrm, T0, thr, iters, fixed=False):
    ks, ps = _up(src); kt, pt = _up(tgt); km, pm = _up(nrm)
    return ctx.icp_dev(ps, len(src), pt, pm, len(tgt), T0, thr, iters, True, fixed)


def _batch(ctx, clouds, normals, tgt, nrm, T0s, thr, iters, fixed):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    cat = np.concatenate(clouds) if off[-1] else np.zeros((0, 3), F)
    catn = np.concatenate(normals) if off[-1] else np.zeros((0, 3), F)
    ks, ps = _up(cat); kn, pn = _up(catn); kt, pt = _up(tgt); km, pm = _up(nrm)
    return ctx.gicp_batch_dev(ps, pn, off, pt, pm, len(tgt), T0s, thr, iters, G.EPSILON, fixed)


def _key(r):
    return (r.transformation.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), r.iterations, r.n_corr)


def _against(got, ref, what):
    """got (device result) against the restatement's ref; False (nothing asserted) when a sum of ref is ambiguous."""
    if ref["ambiguous"]:
        return False
    assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), (what, got.iterations, ref["iterations"], got.n_corr, ref["n_corr"])
    assert np.float32(got.rmse).tobytes() == ref["rmse"].tobytes(), (what, got.rmse, ref["rmse"])
    assert np.float32(got.fitness).tobytes() == ref["fitness"].tobytes(), (what, got.fitness, ref["fitness"])
    assert got.transformation.tobytes() == ref["T"].tobytes(), (what, got.transformation, ref["T"])
    return True


# ---------------------------------------------------------------- one iteration against the restatement
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration(gctx, orc, synth, path, loss):
    ctx, mp = gctx
    _set_path(ctx, mp, path)
    if loss != "l2":
        ctx.set_icp_loss(loss, LOSSES[loss])
    nt, thr = 127, 0.02
    held = 0
    sizes = [3, 64, 255, 256, 257, 1025, 2048] if path == "small" else [3, 64, 257, 1025, 2049, 5000]
    for ns in sizes:
        src, sn, tgt, nrm, T0 = _problem(orc, synth, ns, nt, seed=ns + 100)
        ref = G.gicp(orc, src, sn, tgt, nrm, T0, thr, 1, kind=loss, scale=LOSSES[loss])
        for fixed in (False, True):
            got = _gicp_dev(ctx, src, sn, tgt, nrm, T0, thr, 1, fixed)
            held += _against(got, ref, "%s %s ns %d fixed=%s" % (path, loss, ns, fixed))
        assert ctx.last_icp_search() == PATHS[path][2]
    assert held >= 2 * (len(sizes) - 1)


@pytest.mark.parametrize("path", ["brute", "grid"])
def test_one_iteration_fold_second_round(gctx, orc, synth, path):
    """More blocks than one round of the last block's fold (40,000 points: 157 slabs brute, 40 grid)."""
    ctx, mp = gctx
    _set_path(ctx, mp, path)
    src, sn, tgt, nrm, T0 = _problem(orc, synth, 40000, 2000, seed=5)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        ref = G.gicp(orc, src, sn, tgt, nrm, T0, 0.006, 1, kind=loss, scale=k)
        assert _against(_gicp_dev(ctx, src, sn, tgt, nrm, T0, 0.006, 1, True), ref, "%s %s" % (path, loss))
        assert ctx.last_icp_search() == PATHS[path][2]


# ---------------------------------------------------------------- fixed K equals K chained single iterations; host = dev
@pytest.mark.parametrize("ns,nt", [(500, 500), (3000, 2500)])
def test_fixed_k_equals_chained_iterations(gctx, orc, synth, ns, nt):
    ctx, _ = gctx
    src, sn, tgt, nrm, T0 = _problem(orc, synth, ns, nt, seed=23)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for K in (1, 4, 33):
            T, last = T0, None
            for i in range(K):
                r = _gicp_dev(ctx, src, sn, tgt, nrm, T, 0.004, 1, True)
                if r.iterations:
                    T, last = r.transformation, (r.transformation.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), i + 1, r.n_corr)
            got = _gicp_dev(ctx, src, sn, tgt, nrm, T0, 0.004, K, True)
            assert last is not None
            assert _key(got) == last, (loss, K, ns)


def test_host_equals_dev(gctx, orc, synth):
    ctx, mp = gctx
    for path in PATHS:
        _set_path(ctx, mp, path)
        for ns, nt in ((400, 380), (3000, 2500)):
            src, sn, tgt, nrm, T0 = _problem(orc, synth, ns, nt, seed=ns)
            a = ctx.gicp(src, sn, tgt, nrm, T0, 0.004, 30)
            b = _gicp_dev(ctx, src, sn, tgt, nrm, T0, 0.004, 30)
            assert _key(a) == _key(b) and a.iterations > 0, (path, ns)


# ---------------------------------------------------------------- batched equals single
@pytest.mark.parametrize("kind", ["multi", "small", "fallback_brute"])
def test_batch_equals_single(gctx, orc, synth, kind):
    ctx, _ = gctx
    ctx.set_icp_search({"multi": "grid", "small": "auto", "fallback_brute": "brute"}[kind])
    nt = 500 if kind == "small" else 6000          # (the one-launch path: at most 2^20 point pairs per instance)
    sizes = [3, 300, 0, 2048, 1500, 255] if kind == "small" else [3, 300, 20000, 0, 2049, 1500]
    tgt, nrm = synth.sample_object(nt, 42)
    clouds, normals, T0s = [], [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), 800 + b)
        clouds.append(src[:n].copy())
        normals.append(_normals(orc, clouds[-1], 800 + b))
        T0s.append(synth.perturb(T_gt, seed=900 + b, angle_deg=2.0, trans=0.003))
    T0s = np.stack(T0s).astype(F)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for fixed in ((False,) if kind == "small" else (False, True)):
            got = _batch(ctx, clouds, normals, tgt, nrm, T0s, 0.004, 25, fixed)
            assert ctx.last_icp_search() == ("grid" if kind == "multi" else "brute")
            for b, n in enumerate(sizes):
                if n == 0:
                    assert got[b].iterations == 0 and got[b].transformation.tobytes() == T0s[b].tobytes()
                    continue
                single = _gicp_dev(ctx, clouds[b], normals[b], tgt, nrm, T0s[b], 0.004, 25, fixed)
                assert _key(got[b]) == _key(single), (kind, loss, b, fixed)
    # one iteration of the batch against the restatement
    ctx.set_icp_loss("l2")
    got = _batch(ctx, clouds, normals, tgt, nrm, T0s, 0.004, 1, False)
    for b, n in enumerate(sizes):
        if n:
            _against(got[b], G.gicp(orc, clouds[b], normals[b], tgt, nrm, T0s[b], 0.004, 1), "%s instance %d" % (kind, b))


# ---------------------------------------------------------------- argument checks, empty cases, ICP untouched
def test_argument_checks_leave_out_untouched(gctx, tdv, orc, synth):
    ctx, _ = gctx
    lib = tdv.lib(); h = ctx._h
    src, sn, tgt, nrm, T0 = _problem(orc, synth, 500, 400)
    ks, ps = _up(src); kn, pn = _up(sn); kt, pt = _up(tgt); km, pm = _up(nrm)
    T0c = (C.c_float * 16)(*tdv.to_colmajor16(T0))
    off = (C.c_int * 2)(0, 500)
    s_, n_, t_, m_ = (np.ascontiguousarray(x, F) for x in (src, sn, tgt, nrm))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def calls(psn, ptn, hsn, htn, eps):
        o1, o2, o3 = tdv.IcpResultC(), tdv.IcpResultC(), (tdv.IcpResultC * 1)()
        for o in (o1, o2):
            C.memset(C.byref(o), 0x5A, C.sizeof(o))
        C.memset(o3, 0x5A, C.sizeof(o3))
        raw = bytes(o1)
        r = [lib.tdv_gicp(h, hp(s_), hsn, 500, hp(t_), htn, 400, T0c, C.c_float(0.004), 10, C.c_float(eps), C.byref(o1)),
             lib.tdv_gicp_dev(h, C.c_void_p(ps), psn, 500, C.c_void_p(pt), ptn, 400, T0c, C.c_float(0.004), 10, C.c_float(eps), 0, C.byref(o2)),
             lib.tdv_gicp_batch_dev(h, C.c_void_p(ps), psn, off, 1, C.c_void_p(pt), ptn, 400, T0c, C.c_float(0.004), 10, C.c_float(eps), 0, o3)]
        return r, [bytes(o1) == raw, bytes(o2) == raw, bytes(o3) == raw]
    good = (C.c_void_p(pn), C.c_void_p(pm), hp(n_), hp(m_))
    for what, args in (("src normals", (None, good[1], None, good[3], 1e-3)), ("tgt normals", (good[0], None, good[2], None, 1e-3))):
        r, untouched = calls(*args)
        assert r == [TDV_ERR_BAD_ARG] * 3 and all(untouched), what
    for eps in (0.0, -1e-3, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf")):
        r, untouched = calls(*good, eps)
        assert r == [TDV_ERR_BAD_ARG] * 3 and all(untouched), eps
    ctx.set_icp_accumulation("reference")
    r, untouched = calls(*good, 1e-3)
    assert r == [TDV_ERR_BAD_ARG] * 3 and all(untouched)
    assert "reference" in lib.tdv_last_error(h).decode()
    ctx.set_icp_accumulation("tree")
    r, untouched = calls(*good, 1.0)                       # epsilon = 1: C = 2 I, accepted
    assert r == [0, 0, 0] and not any(untouched)


def test_empty_cases_are_icps(gctx, orc, synth):
    ctx, _ = gctx
    src, sn, tgt, nrm, T0 = _problem(orc, synth, 500, 400)
    for s, n, t, m, it in ((src[:0], sn[:0], tgt, nrm, 10), (src, sn, tgt[:0], nrm[:0], 10), (src, sn, tgt, nrm, 0)):
        g = _gicp_dev(ctx, s, n, t, m, T0, 0.004, it)
        i = _icp_dev(ctx, s, t, m, T0, 0.004, it)
        assert _key(g) == _key(i) and g.iterations == 0
        assert _key(ctx.gicp(s, n, t, m, T0, 0.004, it)) == _key(ctx.icp(s, t, m, T0, 0.004, it, True))
    got = ctx.gicp_batch([src[:0], src], [sn[:0], sn], tgt, nrm, np.stack([T0, T0]), 0.004, 0)
    assert all(g.iterations == 0 and g.transformation.tobytes() == T0.tobytes() for g in got)


def test_icp_unchanged_around_gicp(gctx, orc, synth, monkeypatch):
    ctx, mp = gctx
    src, sn, tgt, nrm, T0 = _problem(orc, synth, 3000, 2500, seed=9)
    for path in PATHS:
        _set_path(ctx, mp, path)
        before = _key(_icp_dev(ctx, src, tgt, nrm, T0, 0.004, 30))
        _gicp_dev(ctx, src, sn, tgt, nrm, T0, 0.004, 30)
        assert _key(_icp_dev(ctx, src, tgt, nrm, T0, 0.004, 30)) == before, path


# ---------------------------------------------------------------- convergence and the scenario on the device
def test_noiseless_scene_reaches_ground_truth(gctx, orc, synth):
    ctx, _ = gctx
    src, sn, tgt, nrm, T_gt = exact_scene(synth)
    T0 = synth.perturb(T_gt, seed=43, angle_deg=2.0, trans=0.003).astype(F)
    got = _gicp_dev(ctx, src, sn, tgt, nrm, T0, 0.01, 60)
    ang, tr = synth.pose_error(got.transformation, T_gt)
    assert ang <= 1e-5 and tr <= 1e-6, (ang, tr)
    assert _against(got, G.gicp(orc, src, sn, tgt, nrm, T0, 0.01, 60), "noiseless")


@pytest.mark.parametrize("path", ["brute", "grid"])
def test_scenario_on_the_device(gctx, orc, synth, path):
    ctx, mp = gctx
    _set_path(ctx, mp, path)
    S = SCENARIO
    src, sn, tgt, nrm, T0, T_gt = scenario(orc, synth)
    g = _gicp_dev(ctx, src, sn, tgt, nrm, T0, S["thr"], S["iterations"])
    p = _icp_dev(ctx, src, tgt, nrm, T0, S["thr"], S["iterations"])
    assert _against(g, G.gicp(orc, src, sn, tgt, nrm, T0, S["thr"], S["iterations"]), "scenario " + path)
    eg, ep = synth.pose_error(g.transformation, T_gt), synth.pose_error(p.transformation, T_gt)
    assert eg[0] < 0.8 * ep[0] and eg[1] < 0.8 * ep[1], (eg, ep)
    ref_p = L.icp(orc, src, tgt, nrm, T0, S["thr"], S["iterations"], True, "l2")
    if not ref_p["ambiguous"]:
        assert p.transformation.tobytes() == ref_p["T"].tobytes()
