"""Colored ICP on the device (include/tdv_hip.h: tdv_color_gradients, tdv_colored_icp), against the restatement of
tests/colored_icp_restatement.py.

The gradients are one thread's f64 sums in list order, so they are the restatement's bytes.  The ICP terms are f32 products widened and
added in f64 in the header's order; their tree sums round to the exact sums' f32 unless exact_sum reports an ambiguity, so T, rmse,
fitness, iterations and n_corr must be the restatement's bytes on every search path and batch path.  Every test runs on a Context of its
own."""
import ctypes as C

import numpy as np
import pytest
import torch

import colored_icp_restatement as R
import gicp_restatement as G
import icp_loss_restatement as L
from test_colored_icp_abi import COLORED_BOUND, PLANE_FLOOR, textured
from test_gpu_nonfinite import ICP_KINDS, _poison_icp, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
LOSSES = {"l2": 0.0, "tukey": 0.02}
PATHS = {   # search mode, TDV_ICP_SMALL, expected search
    "small": ("auto", None, "brute"),
    "brute": ("brute", "0", "brute"),
    "pruned": ("pruned", None, "pruned"),
    "grid": ("grid", None, "grid"),
}


@pytest.fixture
def cctx(tdv, monkeypatch):
    c = tdv.Context(0)
    yield c, monkeypatch
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def _texture(x):
    """A smooth grey texture over space (the model frame)."""
    x = np.asarray(x, np.float64)
    I = 0.5 + 0.2 * np.sin(x[:, 0] / 0.007) * np.cos(x[:, 1] / 0.011) + 0.1 * np.sin(x[:, 2] / 0.005)
    return np.repeat(I[:, None], 3, 1).astype(F)


def _problem(orc, synth, ns, nt, seed=42, angle=2.0, trans=0.003):
    """(src, src_rgb, tgt, nrm, tgt_color, T0); the target's colour table from the restatement (k = 30, or its own size)."""
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(max(ns, 1), seed)
    src = src[:ns].copy()
    srgb = _texture(L.transform(T_gt.astype(F), src)) if ns else np.zeros((0, 3), F)
    tc = R.gradients_of(orc, tgt, _texture(tgt), nrm, min(R.K, nt))
    T0 = synth.perturb(T_gt, seed=seed + 1, angle_deg=angle, trans=trans).astype(F)
    return src, srgb, tgt, nrm, tc, T0


def _set_path(ctx, mp, path):
    search, small, _ = PATHS[path]
    ctx.set_icp_search(search)
    if small is None:
        mp.delenv("TDV_ICP_SMALL", raising=False)
    else:
        mp.setenv("TDV_ICP_SMALL", small)


def _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, thr, iters, fixed=False, lam=R.LAMBDA):
    ks, ps = _up(src); kc, pc = _up(srgb); kt, pt = _up(tgt); km, pm = _up(nrm); kk, pk = _up(tc)
    return ctx.colored_icp_dev(ps, pc, len(src), pt, pm, pk, len(tgt), T0, thr, iters, lam, fixed)


def _icp_dev(ctx, src, tgt, nrm, T0, thr, iters, fixed=False):
    ks, ps = _up(src); kt, pt = _up(tgt); km, pm = _up(nrm)
    return ctx.icp_dev(ps, len(src), pt, pm, len(tgt), T0, thr, iters, True, fixed)


def _batch(ctx, clouds, rgbs, tgt, nrm, tc, T0s, thr, iters, fixed):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    cat = np.concatenate(clouds) if off[-1] else np.zeros((0, 3), F)
    catc = np.concatenate(rgbs) if off[-1] else np.zeros((0, 3), F)
    ks, ps = _up(cat); kc, pc = _up(catc); kt, pt = _up(tgt); km, pm = _up(nrm); kk, pk = _up(tc)
    return ctx.colored_icp_batch_dev(ps, pc, off, pt, pm, pk, len(tgt), T0s, thr, iters, R.LAMBDA, fixed)


def _key(r):
    T = np.where(np.isnan(r.transformation), F(np.nan), r.transformation).astype(F)
    return (T.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), r.iterations, r.n_corr)


def _against(got, ref, what):
    """got (device result) against the restatement's ref (NaN positions equal, every other value byte for byte); False (nothing
    asserted) when a sum of ref is ambiguous."""
    if ref["ambiguous"]:
        return False
    assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), (what, got.iterations, ref["iterations"], got.n_corr, ref["n_corr"])
    _same(np.float32(got.rmse), ref["rmse"], what); _same(np.float32(got.fitness), ref["fitness"], what)
    _same(got.transformation, ref["T"], what)
    return True


# ---------------------------------------------------------------- gradients
@pytest.mark.parametrize("n", [5, 257, 3000, 20000])
def test_gradients_equal_the_restatement(cctx, orc, synth, n):
    ctx, _ = cctx
    xyz, nrm = synth.sample_object(n, n)
    rgb = np.random.default_rng(n).uniform(0, 1, (n, 3)).astype(F)
    k = min(R.K, n)
    _, knn = orc.estimate_normals(xyz, k, want_knn=True)
    ref = R.gradients(xyz, rgb, nrm, knn)
    kx, px = _up(xyz); kc, pc = _up(rgb); km, pm = _up(nrm)
    out = torch.full((n * 4,), 7.0, device=DEV)
    ctx.color_gradients_dev(px, pc, pm, n, k, out.data_ptr())
    _same(out.cpu().numpy().reshape(n, 4), ref, "knn searched")
    # with estimate_normals_dev's list for the same k
    dn = torch.zeros(n * 3, device=DEV); dk = torch.zeros(n * k, dtype=torch.int32, device=DEV)
    ctx.estimate_normals_dev(px, n, k, dn.data_ptr(), dk.data_ptr())
    assert np.array_equal(dk.cpu().numpy().reshape(n, k), knn)
    out.fill_(7.0)
    ctx.color_gradients_dev(px, pc, pm, n, k, out.data_ptr(), dk.data_ptr())
    _same(out.cpu().numpy().reshape(n, 4), ref, "knn given")
    _same(ctx.color_gradients(xyz, rgb, nrm, k), ref, "host")


def test_gradients_poisoned(cctx, orc, synth):
    """NaN / inf colours, normals and coordinates: the restatement's bytes (NaN positions equal)."""
    ctx, _ = cctx
    n = 2000
    xyz, nrm = synth.sample_object(n, 3)
    rgb = np.random.default_rng(3).uniform(0, 1, (n, 3)).astype(F)
    rgb[[0, 17, 900]] = [np.nan, 0.5, 0.5]; rgb[[5, 1999], 2] = np.inf
    nrm = nrm.copy(); nrm[[40, 41]] = np.nan; nrm[60] = [np.inf, 0, 0]
    _, knn = orc.estimate_normals(xyz, R.K, want_knn=True)
    ref = R.gradients(xyz, rgb, nrm, knn)
    assert np.isnan(ref).any()
    _same(ctx.color_gradients(xyz, rgb, nrm, R.K), ref, "poisoned colours and normals")
    # NaN points: the gradients of the lists the device's kNN search gives them (what that search does with NaN is
    # tdv_estimate_normals' business, held elsewhere)
    bad = xyz.copy(); bad[[7, 1500], 1] = np.nan
    kx, px = _up(bad); kc, pc = _up(rgb); km, pm = _up(nrm)
    dn = torch.zeros(n * 3, device=DEV); dk = torch.zeros(n * R.K, dtype=torch.int32, device=DEV)
    ctx.estimate_normals_dev(px, n, R.K, dn.data_ptr(), dk.data_ptr())
    out = torch.zeros(n * 4, device=DEV)
    ctx.color_gradients_dev(px, pc, pm, n, R.K, out.data_ptr())
    ref = R.gradients(bad, rgb, nrm, dk.cpu().numpy().reshape(n, R.K))
    _same(out.cpu().numpy().reshape(n, 4), ref, "poisoned points")


# ---------------------------------------------------------------- one iteration against the restatement
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration(cctx, orc, synth, path, loss):
    ctx, mp = cctx
    _set_path(ctx, mp, path)
    if loss != "l2":
        ctx.set_icp_loss(loss, LOSSES[loss])
    nt, thr = 127, 0.02
    held = 0
    sizes = [3, 64, 255, 256, 257, 1025, 2048] if path == "small" else [3, 64, 257, 1025, 2049, 5000]
    for ns in sizes:
        src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, ns, nt, seed=ns + 100)
        ref = R.colored_icp(orc, src, srgb, tgt, nrm, tc, T0, thr, 1, kind=loss, scale=LOSSES[loss])
        for fixed in (False, True):
            got = _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, thr, 1, fixed)
            held += _against(got, ref, "%s %s ns %d fixed=%s" % (path, loss, ns, fixed))
        assert ctx.last_icp_search() == PATHS[path][2]
    assert held >= 2 * (len(sizes) - 1)


@pytest.mark.parametrize("path", ["brute", "grid"])
def test_one_iteration_fold_second_round(cctx, orc, synth, path):
    """More blocks than one round of the last block's fold (40,000 points: 157 slabs brute, 40 grid)."""
    ctx, mp = cctx
    _set_path(ctx, mp, path)
    src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, 40000, 2000, seed=5)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        ref = R.colored_icp(orc, src, srgb, tgt, nrm, tc, T0, 0.006, 1, kind=loss, scale=k)
        assert _against(_cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, 0.006, 1, True), ref, "%s %s" % (path, loss))
        assert ctx.last_icp_search() == PATHS[path][2]


# ---------------------------------------------------------------- fixed K equals K chained single iterations; host = dev
@pytest.mark.parametrize("ns,nt", [(500, 500), (3000, 2500)])
def test_fixed_k_equals_chained_iterations(cctx, orc, synth, ns, nt):
    ctx, _ = cctx
    src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, ns, nt, seed=23)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for K in (1, 4, 33):
            T, last = T0, None
            for i in range(K):
                r = _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T, 0.004, 1, True)
                if r.iterations:
                    T, last = r.transformation, (r.transformation.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), i + 1, r.n_corr)
            got = _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, 0.004, K, True)
            assert last is not None
            assert _key(got) == last, (loss, K, ns)


def test_host_equals_dev(cctx, orc, synth):
    ctx, mp = cctx
    for path in PATHS:
        _set_path(ctx, mp, path)
        for ns, nt in ((400, 380), (3000, 2500)):
            src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, ns, nt, seed=ns)
            a = ctx.colored_icp(src, srgb, tgt, nrm, tc, T0, 0.004, 30)
            b = _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, 0.004, 30)
            assert _key(a) == _key(b) and a.iterations > 0, (path, ns)


# ---------------------------------------------------------------- batched equals single
@pytest.mark.parametrize("kind", ["multi", "small", "fallback_brute"])
def test_batch_equals_single(cctx, orc, synth, kind):
    ctx, _ = cctx
    ctx.set_icp_search({"multi": "grid", "small": "auto", "fallback_brute": "brute"}[kind])
    nt = 500 if kind == "small" else 6000          # (the one-launch path: at most 2^20 point pairs per instance)
    sizes = [3, 300, 0, 2048, 1500, 255] if kind == "small" else [3, 300, 20000, 0, 2049, 1500]
    tgt, nrm = synth.sample_object(nt, 42)
    tc = R.gradients_of(orc, tgt, _texture(tgt), nrm)
    clouds, rgbs, T0s = [], [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), 800 + b)
        clouds.append(src[:n].copy())
        rgbs.append(_texture(L.transform(T_gt.astype(F), clouds[-1])) if n else np.zeros((0, 3), F))
        T0s.append(synth.perturb(T_gt, seed=900 + b, angle_deg=2.0, trans=0.003))
    T0s = np.stack(T0s).astype(F)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for fixed in ((False,) if kind == "small" else (False, True)):
            got = _batch(ctx, clouds, rgbs, tgt, nrm, tc, T0s, 0.004, 25, fixed)
            assert ctx.last_icp_search() == ("grid" if kind == "multi" else "brute")
            for b, n in enumerate(sizes):
                if n == 0:
                    assert got[b].iterations == 0 and got[b].transformation.tobytes() == T0s[b].tobytes()
                    continue
                single = _cicp_dev(ctx, clouds[b], rgbs[b], tgt, nrm, tc, T0s[b], 0.004, 25, fixed)
                assert _key(got[b]) == _key(single), (kind, loss, b, fixed)
    ctx.set_icp_loss("l2")
    got = _batch(ctx, clouds, rgbs, tgt, nrm, tc, T0s, 0.004, 1, False)
    for b, n in enumerate(sizes):
        if n:
            _against(got[b], R.colored_icp(orc, clouds[b], rgbs[b], tgt, nrm, tc, T0s[b], 0.004, 1), "%s instance %d" % (kind, b))
    host = ctx.colored_icp_batch(clouds, rgbs, tgt, nrm, tc, T0s, 0.004, 25)
    assert [_key(r) for r in host] == [_key(r) for r in _batch(ctx, clouds, rgbs, tgt, nrm, tc, T0s, 0.004, 25, False)]


# ---------------------------------------------------------------- argument checks, empty cases, lambda = 1, ICP and GICP untouched
def test_argument_checks_leave_out_untouched(cctx, tdv, orc, synth):
    ctx, _ = cctx
    lib = tdv.lib(); h = ctx._h
    src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, 500, 400)
    ks, ps = _up(src); kc, pc = _up(srgb); kt, pt = _up(tgt); km, pm = _up(nrm); kk, pk = _up(tc)
    T0c = (C.c_float * 16)(*tdv.to_colmajor16(T0))
    off = (C.c_int * 2)(0, 500)
    s_, c_, t_, m_, k_ = (np.ascontiguousarray(x, F) for x in (src, srgb, tgt, nrm, tc))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def calls(d_rgb, d_nrm, d_tc, h_rgb, h_nrm, h_tc, lam):
        o1, o2, o3 = tdv.IcpResultC(), tdv.IcpResultC(), (tdv.IcpResultC * 1)()
        for o in (o1, o2):
            C.memset(C.byref(o), 0x5A, C.sizeof(o))
        C.memset(o3, 0x5A, C.sizeof(o3))
        raw = bytes(o1)
        lf = C.c_float(lam)
        r = [lib.tdv_colored_icp(h, hp(s_), h_rgb, 500, hp(t_), h_nrm, h_tc, 400, T0c, C.c_float(0.004), 10, lf, C.byref(o1)),
             lib.tdv_colored_icp_dev(h, C.c_void_p(ps), d_rgb, 500, C.c_void_p(pt), d_nrm, d_tc, 400, T0c, C.c_float(0.004), 10, lf, 0, C.byref(o2)),
             lib.tdv_colored_icp_batch_dev(h, C.c_void_p(ps), d_rgb, off, 1, C.c_void_p(pt), d_nrm, d_tc, 400, T0c, C.c_float(0.004), 10, lf, 0, o3)]
        return r, [bytes(o1) == raw, bytes(o2) == raw, bytes(o3) == raw]
    good = [C.c_void_p(pc), C.c_void_p(pm), C.c_void_p(pk), hp(c_), hp(m_), hp(k_)]
    for i, what in enumerate(("rgb", "normals", "colour table")):
        args = list(good); args[i] = None; args[i + 3] = None
        r, untouched = calls(*args, 0.968)
        assert r == [TDV_ERR_BAD_ARG] * 3 and all(untouched), what
    for lam in (-1e-3, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf")):
        r, untouched = calls(*good, lam)
        assert r == [TDV_ERR_BAD_ARG] * 3 and all(untouched), lam
    odd = list(good); odd[2] = C.c_void_p(pk + 4)      # a device colour table off its float4 alignment
    r, untouched = calls(*odd, 0.968)
    assert r[1:] == [TDV_ERR_BAD_ARG] * 2 and all(untouched[1:])
    ctx.set_icp_accumulation("reference")
    r, untouched = calls(*good, 0.968)
    assert r == [TDV_ERR_BAD_ARG] * 3 and all(untouched)
    assert "reference" in lib.tdv_last_error(h).decode()
    ctx.set_icp_accumulation("tree")
    for lam in (0.0, 1.0):
        r, untouched = calls(*good, lam)
        assert r == [0, 0, 0] and not any(untouched), lam
    n = 100
    kx, px = _up(tgt[:n]); out = torch.zeros(n * 4, device=DEV)
    for k in (0, -1, 256):
        assert lib.tdv_color_gradients_dev(h, C.c_void_p(px), C.c_void_p(pc), C.c_void_p(pm), n, k, None, C.c_void_p(out.data_ptr())) == TDV_ERR_BAD_ARG
    assert lib.tdv_color_gradients_dev(h, C.c_void_p(px), None, C.c_void_p(pm), n, 30, None, C.c_void_p(out.data_ptr())) == TDV_ERR_BAD_ARG
    assert not out.any()


def test_empty_cases_are_icps(cctx, orc, synth):
    ctx, _ = cctx
    src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, 500, 400)
    for s, c, t, m, k, it in ((src[:0], srgb[:0], tgt, nrm, tc, 10), (src, srgb, tgt[:0], nrm[:0], tc[:0], 10), (src, srgb, tgt, nrm, tc, 0)):
        g = _cicp_dev(ctx, s, c, t, m, k, T0, 0.004, it)
        i = _icp_dev(ctx, s, t, m, T0, 0.004, it)
        assert _key(g) == _key(i) and g.iterations == 0
        assert _key(ctx.colored_icp(s, c, t, m, k, T0, 0.004, it)) == _key(ctx.icp(s, t, m, T0, 0.004, it, True))
    got = ctx.colored_icp_batch([src[:0], src], [srgb[:0], srgb], tgt, nrm, tc, np.stack([T0, T0]), 0.004, 0)
    assert all(g.iterations == 0 and g.transformation.tobytes() == T0.tobytes() for g in got)


def test_lambda_one_is_point_to_plane(cctx, orc, synth):
    ctx, mp = cctx
    for path in PATHS:
        _set_path(ctx, mp, path)
        for ns, nt in ((400, 380), (3000, 2500)):
            src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, ns, nt, seed=ns + 7)
            for fixed in (False, True):
                a = _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, 0.004, 20, fixed, lam=1.0)
                b = _icp_dev(ctx, src, tgt, nrm, T0, 0.004, 20, fixed)
                assert np.array_equal(a.transformation, b.transformation) and a.rmse == b.rmse and a.fitness == b.fitness, (path, ns, fixed)
                assert (a.iterations, a.n_corr) == (b.iterations, b.n_corr) and a.iterations > 0, (path, ns, fixed)


def test_icp_and_gicp_unchanged_around_colored_icp(cctx, orc, synth):
    ctx, mp = cctx
    src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, 3000, 2500, seed=9)
    sn = orc.estimate_normals(src)
    ks, ps = _up(src); kn, pn = _up(sn); kt, pt = _up(tgt); km, pm = _up(nrm)
    for path in PATHS:
        _set_path(ctx, mp, path)
        before = (_key(_icp_dev(ctx, src, tgt, nrm, T0, 0.004, 30)),
                  _key(ctx.gicp_dev(ps, pn, len(src), pt, pm, len(tgt), T0, 0.004, 30, G.EPSILON)))
        _cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, 0.004, 30)
        after = (_key(_icp_dev(ctx, src, tgt, nrm, T0, 0.004, 30)),
                 _key(ctx.gicp_dev(ps, pn, len(src), pt, pm, len(tgt), T0, 0.004, 30, G.EPSILON)))
        assert after == before, path


# ---------------------------------------------------------------- the textured scene on the device
@pytest.mark.parametrize("path", ["small", "brute", "grid"])
def test_textured_scene_on_the_device(cctx, orc, synth, path):
    ctx, mp = cctx
    _set_path(ctx, mp, path)
    S = R.SCENE
    src, rgb, tgt, nrm, tc, T0, T_gt = textured(orc)
    # the model's colour table from the device equals the restatement's
    mrgb = R.lid_model()[2]
    _same(ctx.color_gradients(tgt, mrgb, nrm, R.K), tc, "lid gradients")
    c = _cicp_dev(ctx, src, rgb, tgt, nrm, tc, T0, S["thr"], S["iterations"])
    p = _icp_dev(ctx, src, tgt, nrm, T0, S["thr"], S["iterations"])
    assert _against(c, R.colored_icp(orc, src, rgb, tgt, nrm, tc, T0, S["thr"], S["iterations"]), "textured " + path)
    ec, ep = synth.pose_error(c.transformation, T_gt), synth.pose_error(p.transformation, T_gt)
    assert ec[0] <= COLORED_BOUND[0] and ec[1] <= COLORED_BOUND[1], ec
    assert ep[0] > PLANE_FLOOR, ep


# ---------------------------------------------------------------- poisoned input
@pytest.mark.parametrize("kind", ICP_KINDS + ["rgb_nan", "rgb_inf", "color_nan", "color_inf"])
def test_poisoned(cctx, orc, synth, kind):
    """NaN / inf in coordinates, normals, source colours and the target's colour table, on every path, against the restatement."""
    ctx, mp = cctx
    src, srgb, tgt, nrm, tc, T0 = _problem(orc, synth, 1500, 1200, seed=9)
    rng = np.random.default_rng(1)
    if kind in ICP_KINDS:
        src, tgt, nrm = _poison_icp(src, tgt, nrm, kind, rng)
    else:
        srgb = srgb.copy(); tc = tc.copy()
        val = np.nan if kind.endswith("nan") else np.inf
        if kind.startswith("rgb"):
            srgb[rng.choice(len(src), 20, replace=False), rng.integers(0, 3, 20)] = val
        else:
            tc[rng.choice(len(tgt), 20, replace=False), rng.integers(0, 4, 20)] = val
    held = 0
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for fixed in (False, True):
            ref = R.colored_icp(orc, src, srgb, tgt, nrm, tc, T0, 0.004, 6, kind=loss, scale=k, fixed=fixed)
            for path in PATHS:
                _set_path(ctx, mp, path)
                held += _against(_cicp_dev(ctx, src, srgb, tgt, nrm, tc, T0, 0.004, 6, fixed), ref, (kind, loss, fixed, path))
    assert held >= 8, "%s: too many restated sums are ambiguous" % kind
