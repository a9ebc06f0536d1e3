"""ICP with a robust loss on the device (include/tdv_hip.h: tdv_ctx_set_icp_loss), against the restatement of tests/icp_loss_restatement.py.

Every test runs on a Context of its own (the session's `ctx` keeps L2).  Point-to-plane: the weighted terms are exact products in f64
and their tree sums round to the exact sums' f32 unless exact_sum reports an ambiguity, so T, rmse, fitness, iterations and n_corr
must be the restatement's bytes.  Point-to-point: the device divides f64 tree sums by the tree sum W of the weights and centres in f64,
the restatement evaluates the same expressions on the exactly rounded sums, so T agrees to 1e-4 rad and 1e-6 m (test_gpu_icp.py's
tolerances) while rmse, fitness and n_corr - unweighted - stay bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_loss_restatement as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
LOSSES = {"huber": 0.004, "tukey": 0.008, "cauchy": 0.004}
EDGE_NS = [3, 64, 255, 256, 257, 1023, 1024, 1025, 2048, 2049]
PATHS = {   # search mode, TDV_ICP_SMALL, expected search
    "small": ("auto", None, "brute"),
    "brute": ("brute", "0", "brute"),
    "pruned": ("pruned", None, "pruned"),
    "grid": ("grid", None, "grid"),
}


@pytest.fixture
def lctx(tdv, monkeypatch):
    c = tdv.Context(0)
    yield c, monkeypatch
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 3), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def _problem(synth, ns, nt, seed=42, angle=2.0, trans=0.003):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(max(ns, 1), seed)
    T0 = synth.perturb(T_gt, seed=seed + 1, angle_deg=angle, trans=trans).astype(np.float32)
    return src[:ns].copy(), tgt, nrm, T0


def _set_path(ctx, mp, path):
    search, small, _ = PATHS[path]
    ctx.set_icp_search(search)
    if small is None:
        mp.delenv("TDV_ICP_SMALL", raising=False)
    else:
        mp.setenv("TDV_ICP_SMALL", small)


def _icp_dev(ctx, src, tgt, nrm, T0, thr, iters, p2plane, fixed=False):
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    return ctx.icp_dev(ps, len(src), pt, pn if p2plane else None, len(tgt), T0, thr, iters, p2plane, fixed_iterations=fixed)


def _batch(ctx, clouds, tgt, nrm, T0s, thr, iters, p2plane, fixed):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    cat = np.concatenate(clouds) if off[-1] else np.zeros((0, 3), np.float32)
    ks, ps = _up(cat); kt, pt = _up(tgt); kn, pn = _up(nrm)
    return ctx.icp_batch_dev(ps, off, pt, pn if p2plane else None, len(tgt), T0s, thr, iters, p2plane, fixed)


def _key(r):
    return (r.transformation.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), r.iterations, r.n_corr)


def _against(got, ref, p2plane, synth, what):
    """got (device result) against the restatement's result ref."""
    assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), (what, got.iterations, ref["iterations"], got.n_corr, ref["n_corr"])
    assert np.float32(got.rmse).tobytes() == ref["rmse"].tobytes(), (what, got.rmse, ref["rmse"])
    assert np.float32(got.fitness).tobytes() == ref["fitness"].tobytes(), (what, got.fitness, ref["fitness"])
    if p2plane:
        assert not ref["ambiguous"], "%s: a sum lies within the tree's bound of an f32 rounding midpoint; pick another input" % what
        assert got.transformation.tobytes() == ref["T"].tobytes(), (what, got.transformation, ref["T"])
    else:
        ang, tr = synth.pose_error(got.transformation, ref["T"])
        assert ang <= 1e-4 and tr <= 1e-6, (what, ang, tr)


# ---------------------------------------------------------------- L2 is untouched
def test_l2_after_a_loss_is_todays_l2(tdv, synth, monkeypatch):
    fresh, used = tdv.Context(0), tdv.Context(0)
    try:
        used.set_icp_loss("tukey", 0.002)
        used.set_icp_loss("l2")
        assert used.icp_loss() == ("l2", 0.0) and fresh.icp_loss() == ("l2", 0.0)
        for path in PATHS:
            for c in (fresh, used):
                _set_path(c, monkeypatch, path)
            for p2plane in (True, False):
                for ns, nt in ((700, 300), (3000, 2500)):
                    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=ns)
                    for fixed in (False, True):
                        a = _icp_dev(fresh, src, tgt, nrm, T0, 0.004, 30, p2plane, fixed)
                        b = _icp_dev(used, src, tgt, nrm, T0, 0.004, 30, p2plane, fixed)
                        assert _key(a) == _key(b), (path, p2plane, ns, fixed)
        for search in ("grid", "auto", "pruned"):
            fresh.set_icp_search(search); used.set_icp_search(search)
            tgt, nrm = synth.sample_object(6000, 42)
            clouds = [synth.make_scene(n, 70 + n)[0] for n in (3, 300, 2049, 5000)]
            T0s = np.stack([synth.perturb(synth.make_scene(1, 70 + n)[1], seed=n, angle_deg=2.0, trans=0.003) for n in (3, 300, 2049, 5000)]).astype(np.float32)
            for fixed in (False, True):
                a = _batch(fresh, clouds, tgt, nrm, T0s, 0.004, 20, True, fixed)
                b = _batch(used, clouds, tgt, nrm, T0s, 0.004, 20, True, fixed)
                assert [_key(x) for x in a] == [_key(x) for x in b], (search, fixed)
    finally:
        fresh.close(); used.close()


# ---------------------------------------------------------------- one iteration against the restatement
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration(lctx, orc, synth, path, loss, p2plane):
    ctx, mp = lctx
    _set_path(ctx, mp, path)
    ctx.set_icp_loss(loss, LOSSES[loss])
    nt, thr = 127, 0.02
    for ns in EDGE_NS:
        src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=ns + 100)
        ref = R.icp(orc, src, tgt, nrm, T0, thr, 1, p2plane, loss, LOSSES[loss])
        for fixed in (False, True):
            got = _icp_dev(ctx, src, tgt, nrm, T0, thr, 1, p2plane, fixed)
            _against(got, ref, p2plane, synth, "%s %s ns %d fixed=%s" % (path, loss, ns, fixed))
        assert ctx.last_icp_search() == PATHS[path][2]


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,path", [(32769, "brute"), (131073, "grid"), (131073, "pruned")])
def test_one_iteration_fold_second_round(lctx, orc, synth, ns, path, p2plane):
    ctx, mp = lctx
    _set_path(ctx, mp, path)
    nt = 2000 if ns < 100000 else 1500
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=5)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        ref = R.icp(orc, src, tgt, nrm, T0, 0.006, 1, p2plane, loss, k)
        _against(_icp_dev(ctx, src, tgt, nrm, T0, 0.006, 1, p2plane, True), ref, p2plane, synth, "%s %s ns %d" % (path, loss, ns))
        assert ctx.last_icp_search() == PATHS[path][2]


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("kind", ["multi", "small_batch", "fallback_pruned", "fallback_brute_fixed"])
def test_batch_one_iteration(lctx, orc, synth, kind, p2plane):
    """k_icp_accumulate_multi (grid), icp_small_batch_dev and the per-instance fallback, one iteration, against the restatement."""
    ctx, _ = lctx
    ctx.set_icp_search({"multi": "grid", "small_batch": "auto", "fallback_pruned": "pruned", "fallback_brute_fixed": "brute"}[kind])
    sizes, nt = ([3, 64, 257, 0, 1025, 2048, 255], 500) if kind == "small_batch" else ([3, 64, 257, 0, 1025, 2049, 4097, 255], 6000)
    tgt, nrm = synth.sample_object(nt, 42)
    clouds, T0s = [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), 300 + b)
        clouds.append(src[:n].copy())
        T0s.append(synth.perturb(T_gt, seed=400 + b, angle_deg=2.0, trans=0.003))
    T0s = np.stack(T0s).astype(np.float32)
    fixeds = (True,) if kind == "fallback_brute_fixed" else ((False,) if kind == "small_batch" else (False, True))
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for fixed in fixeds:
            got = _batch(ctx, clouds, tgt, nrm, T0s, 0.004, 1, p2plane, fixed)
            if kind == "multi":
                assert ctx.last_icp_search() == "grid"
            for b, n in enumerate(sizes):
                if n == 0:
                    assert got[b].iterations == 0 and got[b].transformation.tobytes() == T0s[b].tobytes()
                    continue
                ref = R.icp(orc, clouds[b], tgt, nrm, T0s[b], 0.004, 1, p2plane, loss, k)
                _against(got[b], ref, p2plane, synth, "%s %s instance %d fixed=%s" % (kind, loss, b, fixed))


# ---------------------------------------------------------------- fixed K equals K chained single iterations
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,nt", [(500, 500), (3000, 2500)])
def test_fixed_k_equals_chained_iterations(lctx, synth, ns, nt, p2plane):
    ctx, _ = lctx
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=23)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for K in (1, 4, 31, 32, 33, 70):
            T, last = T0, None
            for i in range(K):
                r = _icp_dev(ctx, src, tgt, nrm, T, 0.004, 1, p2plane, True)
                if r.iterations:
                    T, last = r.transformation, (r.transformation.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), i + 1, r.n_corr)
            got = _icp_dev(ctx, src, tgt, nrm, T0, 0.004, K, p2plane, True)
            assert last is not None
            assert _key(got) == last, (loss, K, ns)


# ---------------------------------------------------------------- batched equals single
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("search", ["auto", "grid", "pruned", "brute"])
def test_batch_equals_single(lctx, synth, search, p2plane):
    """A batch mixing the brute-force regime (small instances) and the grid regime (20,000 points against 6,000): per instance the
    single call's bits, under each loss, free-running and fixed."""
    ctx, _ = lctx
    ctx.set_icp_search(search)
    tgt, nrm = synth.sample_object(6000, 42)
    sizes = [3, 300, 20000, 0, 2049, 1500]
    clouds, T0s = [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), 800 + b)
        clouds.append(src[:n].copy())
        T0s.append(synth.perturb(T_gt, seed=900 + b, angle_deg=2.0, trans=0.003))
    T0s = np.stack(T0s).astype(np.float32)
    for loss, k in LOSSES.items():
        ctx.set_icp_loss(loss, k)
        for fixed in (False, True):
            got = _batch(ctx, clouds, tgt, nrm, T0s, 0.004, 25, p2plane, fixed)
            for b, n in enumerate(sizes):
                single = _icp_dev(ctx, clouds[b], tgt, nrm, T0s[b], 0.004, 25, p2plane, fixed) if n else None
                if single is None:
                    assert got[b].iterations == 0
                    continue
                assert _key(got[b]) == _key(single), (loss, search, b, fixed)


# ---------------------------------------------------------------- the chain entry points
def _scene(synth, n_inst, w=640, h=480):
    f = 600.0
    cx, cy = w / 2.0, h / 2.0
    depth = np.zeros((h, w), np.uint16)
    masks = np.zeros((n_inst, h, w), np.uint8)
    model, _ = synth.sample_object(60000, 42)
    poses = []
    for b in range(n_inst):
        T = synth.make_transform([0.3 + 0.2 * b, 1.0, 0.4 - 0.3 * b], 25.0 + 10 * b, (-0.15 + 0.15 * (b % 3), -0.08 + 0.08 * (b // 3), 0.55 + 0.03 * b))
        poses.append(T)
        p = model.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3]
        u = np.round(p[:, 0] / p[:, 2] * f + cx).astype(int); v = np.round(p[:, 1] / p[:, 2] * f + cy).astype(int)
        ok = (u >= 0) & (u < w) & (v >= 0) & (v < h) & (p[:, 2] > 0)
        zb = np.full((h, w), np.inf)
        np.minimum.at(zb, (v[ok], u[ok]), p[ok, 2])
        hit = np.isfinite(zb) & (depth == 0)
        depth[hit] = np.round(zb[hit] * 1000.0).astype(np.uint16)
        masks[b][hit] = 255
    return depth, masks, dict(fx=f, fy=f, cx=cx, cy=cy, width=w, height=h), poses


def _model(ctx, tdv, synth, voxel):
    raw, _ = synth.sample_object(20000, 7)
    d_raw = torch.from_numpy(raw).to(DEV)
    d_mx = torch.empty_like(d_raw); d_mn = torch.empty_like(d_raw)
    d_mf = torch.empty((len(raw), 33), dtype=torch.float32, device=DEV)
    nm = ctx.prepare_model_dev(d_raw.data_ptr(), len(raw), voxel, 30, 5.0, d_mx.data_ptr(), d_mn.data_ptr(), d_mf.data_ptr(), order=tdv.TDV_VOXEL_ORDER_FIRST)
    return d_mx, d_mn, d_mf, nm


def _voxels(ctx, depth, mask, intr, voxel):
    xyz, _ = ctx.depth_to_cloud(depth, mask, None, 1000.0, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 1.5)
    src, _ = ctx.voxel_downsample(xyz, None, voxel)
    return src


def test_refine_and_register_equal_stagewise_chains_under_tukey(lctx, tdv, synth):
    """tdv_refine_batch_dev and tdv_register_batch_dev (three host lanes, not staged: helper lanes run ICP of their own instances) under
    Tukey equal ICP from the same start on the same voxels; and the loss changes something."""
    ctx, mp = lctx
    voxel, n_inst = 0.004, 5
    depth, masks, intr, poses = _scene(synth, n_inst)
    d_mx, d_mn, d_mf, nm = _model(ctx, tdv, synth, voxel)
    mx = d_mx[:nm].cpu().numpy(); mn = d_mn[:nm].cpu().numpy()
    d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)
    srcs = [_voxels(ctx, depth, masks[b], intr, voxel) for b in range(n_inst)]
    thr, scale = voxel * 0.4, 0.001
    T0s = np.stack([synth.perturb(np.linalg.inv(poses[b].astype(np.float64)).astype(np.float32), seed=300 + b, angle_deg=0.5, trans=0.001)
                    for b in range(n_inst)])
    prm = tdv.batch_params(voxel_size=voxel, zmax=1.5, icp_max_iterations=30, ransac_max_iterations=3000, **intr)
    changed = 0
    # refine
    ctx.set_icp_loss("tukey", scale)
    res = ctx.refine_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm, T0s, d_mx.data_ptr(), d_mn.data_ptr(), nm)
    for b in range(n_inst):
        fine = ctx.icp(srcs[b], mx, mn, T0s[b], thr, 30, True)
        assert res[b]["n_voxels"] == len(srcs[b]) and res[b]["icp_iterations"] == fine.iterations > 0, b
        assert res[b]["T"].tobytes() == fine.transformation.tobytes() and res[b]["fitness"] == fine.fitness and res[b]["rmse"] == fine.rmse, b
    # register: the coarse poses (ICP with 0 iterations returns them), then ICP under Tukey from them
    mp.setenv("TDV_BATCH_LANES", "3")
    mp.setenv("TDV_BATCH_STAGED", "0")
    ctx.set_icp_loss("l2")
    prm0 = tdv.batch_params(voxel_size=voxel, zmax=1.5, icp_max_iterations=0, ransac_max_iterations=3000, **intr)
    coarse = ctx.register_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm0, d_mx.data_ptr(), d_mn.data_ptr(), d_mf.data_ptr(), nm)
    l2 = ctx.register_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm, d_mx.data_ptr(), d_mn.data_ptr(), d_mf.data_ptr(), nm)
    ctx.set_icp_loss("tukey", scale)
    reg = ctx.register_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm, d_mx.data_ptr(), d_mn.data_ptr(), d_mf.data_ptr(), nm)
    assert ctx.last_batch_lanes() == 3
    for b in range(n_inst):
        fine = ctx.icp(srcs[b], mx, mn, coarse[b]["T"], thr, 30, True)
        assert reg[b]["icp_iterations"] == fine.iterations > 0, b
        assert reg[b]["T"].tobytes() == fine.transformation.tobytes() and reg[b]["fitness"] == fine.fitness and reg[b]["rmse"] == fine.rmse, b
        changed += reg[b]["T"].tobytes() != l2[b]["T"].tobytes()
    assert changed > 0


# ---------------------------------------------------------------- n_eff < 3
def test_no_weighted_correspondence_keeps_the_pose(lctx, orc, synth):
    ctx, mp = lctx
    ctx.set_icp_loss("tukey", 1e-9)
    for path in ("small", "brute", "grid"):
        _set_path(ctx, mp, path)
        src, tgt, nrm, T0, _ = R.clutter_scene(synth, n_scan=340, n_model=500, n_floor=170) if path == "small" else R.clutter_scene(synth)
        for p2plane in (True, False):
            for fixed in (False, True):
                got = _icp_dev(ctx, src, tgt, nrm, T0, R.SCENE["thr"], 5, p2plane, fixed)
                assert got.transformation.tobytes() == T0.tobytes(), (path, p2plane, fixed)
                assert (got.iterations, got.n_corr, float(got.fitness), float(got.rmse)) == (0, 0, 0.0, 0.0), (path, p2plane, fixed)
    src, tgt, nrm, T0, _ = R.clutter_scene(synth)
    ctx.set_icp_search("grid")
    got = _batch(ctx, [src, src[:500]], tgt, nrm, np.stack([T0, T0]), R.SCENE["thr"], 5, True, True)
    assert all(g.iterations == 0 and g.transformation.tobytes() == T0.tobytes() for g in got)


# ---------------------------------------------------------------- refusals
def test_reference_order_with_a_loss_is_refused(lctx, tdv, synth):
    ctx, _ = lctx
    lib = tdv.lib()
    ctx.set_icp_accumulation("reference")
    ctx.set_icp_loss("huber", 0.003)
    src, tgt, nrm, T0 = _problem(synth, 500, 400)
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    T0c = (C.c_float * 16)(*tdv.to_colmajor16(T0))

    def sentinel():
        o = tdv.IcpResultC()
        C.memset(C.byref(o), 0x5A, C.sizeof(o))
        return o
    raw = bytes(sentinel())
    h = ctx._h
    s = np.ascontiguousarray(src, np.float32); t = np.ascontiguousarray(tgt, np.float32); n = np.ascontiguousarray(nrm, np.float32)
    o = sentinel()
    assert lib.tdv_icp(h, s.ctypes.data_as(C.c_void_p), 500, t.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), 400, T0c,
                       C.c_float(0.004), 10, 1, C.byref(o)) == TDV_ERR_BAD_ARG
    assert bytes(o) == raw and "reference" in lib.tdv_last_error(h).decode()
    o = sentinel()
    assert lib.tdv_icp_dev(h, C.c_void_p(ps), 500, C.c_void_p(pt), C.c_void_p(pn), 400, T0c, C.c_float(0.004), 10, 1, 0, C.byref(o)) == TDV_ERR_BAD_ARG
    assert bytes(o) == raw
    off = (C.c_int * 2)(0, 500)
    ob = (tdv.IcpResultC * 1)(); C.memset(ob, 0x5A, C.sizeof(ob))
    assert lib.tdv_icp_batch_dev(h, C.c_void_p(ps), off, 1, C.c_void_p(pt), C.c_void_p(pn), 400, T0c, C.c_float(0.004), 10, 1, 0, ob) == TDV_ERR_BAD_ARG
    assert bytes(ob) == raw
    depth, masks, intr, poses = _scene(synth, 2)
    d_mx, d_mn, d_mf, nm = _model(ctx, tdv, synth, 0.004)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)
    prm = tdv.batch_params(voxel_size=0.004, zmax=1.5, icp_max_iterations=10, ransac_max_iterations=500, **intr)
    T0s = (C.c_float * 32)(*np.concatenate([tdv.to_colmajor16(np.eye(4))] * 2))
    for call in ("refine", "register"):
        res = (tdv.InstanceResultC * 2)(); C.memset(res, 0x5A, C.sizeof(res)); before = bytes(res)
        if call == "refine":
            st = lib.tdv_refine_batch_dev(h, C.c_void_p(d_depth.data_ptr()), None, C.c_void_p(d_masks.data_ptr()), 2, C.byref(prm), T0s,
                                          C.c_void_p(d_mx.data_ptr()), C.c_void_p(d_mn.data_ptr()), nm, res)
        else:
            st = lib.tdv_register_batch_dev(h, C.c_void_p(d_depth.data_ptr()), None, C.c_void_p(d_masks.data_ptr()), 2, C.byref(prm),
                                            C.c_void_p(d_mx.data_ptr()), C.c_void_p(d_mn.data_ptr()), C.c_void_p(d_mf.data_ptr()), nm, res)
        assert st == TDV_ERR_BAD_ARG, call
        assert bytes(res) == before, call
        assert "reference" in lib.tdv_last_error(h).decode()
    # the correspondence pass is unaffected; back to tree sums, the loss runs
    assert ctx.icp_correspondences(src, tgt, T0, 0.004)["n_corr"] > 0
    ctx.set_icp_accumulation("tree")
    assert _icp_dev(ctx, src, tgt, nrm, T0, 0.004, 10, True).iterations > 0


def test_bad_setter_arguments_leave_the_setting(lctx, tdv):
    ctx, _ = lctx
    lib = tdv.lib()
    ctx.set_icp_loss("tukey", 0.01)
    for kind, scale in ((7, 1.0), (-1, 1.0), (1, float("nan")), (1, float("inf")), (2, 0.0), (3, -0.5), (1, float("-inf"))):
        assert lib.tdv_ctx_set_icp_loss(ctx._h, kind, C.c_float(scale)) == TDV_ERR_BAD_ARG, (kind, scale)
        assert ctx.icp_loss() == ("tukey", float(np.float32(0.01)))
    with pytest.raises(ValueError):
        ctx.set_icp_loss("huber")
    with pytest.raises(ValueError):
        ctx.set_icp_loss("biweight", 0.1)
    with pytest.raises(tdv.TdvError):
        ctx.set_icp_loss("cauchy", -1.0)
    assert ctx.icp_loss() == ("tukey", float(np.float32(0.01)))
    ctx.set_icp_loss("l2", float("nan"))                           # L2 ignores the scale
    assert ctx.icp_loss() == ("l2", 0.0)


# ---------------------------------------------------------------- the CPU scenario on the device
@pytest.mark.parametrize("path", ["small", "brute", "grid"])
def test_scenario_on_the_device(lctx, orc, synth, path):
    ctx, mp = lctx
    _set_path(ctx, mp, path)
    S = R.SCENE
    # (k_icp_small runs a single problem up to 2^18 point pairs: a smaller scan, floor and model)
    src, tgt, nrm, T0, T_gt = R.clutter_scene(synth, n_scan=340, n_model=500, n_floor=170) if path == "small" else R.clutter_scene(synth)
    l2 = _icp_dev(ctx, src, tgt, nrm, T0, S["thr"], S["iterations"], True)
    ctx.set_icp_loss("tukey", S["tukey_scale"])
    tk = _icp_dev(ctx, src, tgt, nrm, T0, S["thr"], S["iterations"], True)
    assert not R.within_gate(synth, l2.transformation, T_gt)[0], R.within_gate(synth, l2.transformation, T_gt)
    assert R.within_gate(synth, tk.transformation, T_gt)[0], R.within_gate(synth, tk.transformation, T_gt)
    ref = R.icp(orc, src, tgt, nrm, T0, S["thr"], S["iterations"], True, "tukey", S["tukey_scale"])
    _against(tk, ref, True, synth, "scenario " + path)
