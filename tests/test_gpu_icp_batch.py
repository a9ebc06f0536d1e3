"""Batched ICP against one shared model (include/tdv_hip.h: tdv_icp_batch_dev, tdv_refine_batch_dev).

The bar is the single call: per instance, tdv_icp_batch_dev returns what tdv_icp_dev returns for that cloud on the same ctx, bit
for bit (T, fitness, rmse, iterations, n_corr), whichever search and accumulation mode the ctx holds; tdv_refine_batch_dev returns
what the stagewise chain depth_to_cloud -> voxel_downsample(order) -> icp(T0) returns.  With reference-order sums both equal the
CPU oracle.  In the regime the batched path is for (tree sums, AUTO or GRID search, a usable grid, a model above 2,048 points) the
correspondence search must run once per iteration for the whole batch, not once per instance."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2


# ---------------------------------------------------------------- helpers
def _up(a):
    """a (float32 rows of 3) on the device, 12 bytes into a larger buffer: (tensor, device pointer)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    base = torch.zeros(a.size + 6, dtype=torch.float32, device=DEV)
    if a.size:
        base[3:3 + a.size].copy_(torch.from_numpy(a).to(DEV))
    return base, base.data_ptr() + 12


def _instances(synth, sizes, spread=1.0):
    """Clouds of the given sizes, each a noisy view of the object under its own pose, and start poses near the truth."""
    clouds, T0s = [], []
    for b, n in enumerate(sizes):
        T_gt = synth.gt_transform(100 + b)
        src, T_gt = synth.make_scene(max(n, 1), 100 + b, T_gt=T_gt)
        clouds.append(src[:n].copy())
        T0s.append(synth.perturb(T_gt, seed=200 + b, angle_deg=3.0 * spread, trans=0.005 * spread))
    return clouds, np.stack(T0s)


def _concat(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    cat = np.concatenate(clouds) if off[-1] else np.zeros((0, 3), np.float32)
    return cat, off


def _same(a, b, what=""):
    assert a.transformation.tobytes() == b.transformation.tobytes(), what
    assert np.float32(a.fitness).tobytes() == np.float32(b.fitness).tobytes(), what
    assert np.float32(a.rmse).tobytes() == np.float32(b.rmse).tobytes(), what
    assert a.iterations == b.iterations and a.n_corr == b.n_corr, (what, a.iterations, b.iterations, a.n_corr, b.n_corr)


def _batch_vs_single(ctx, clouds, T0s, tgt, nrm, thr, iters, p2p=True, fixed=False):
    cat, off = _concat(clouds)
    keep_s, d_src = _up(cat)
    keep_t, d_tgt = _up(tgt)
    keep_n, d_nrm = (None, None) if nrm is None else _up(nrm)
    got = ctx.icp_batch_dev(d_src, off, d_tgt, d_nrm, len(tgt), T0s, thr, iters, p2p, fixed)
    batch_search = ctx.last_icp_search()
    assert len(got) == len(clouds)
    for b in range(len(clouds)):
        ref = ctx.icp_dev(d_src + 12 * int(off[b]), int(off[b + 1] - off[b]), d_tgt, d_nrm, len(tgt), T0s[b], thr, iters, p2p, fixed)
        _same(got[b], ref, "instance %d (%d points)" % (b, off[b + 1] - off[b]))
    return got, batch_search


@pytest.fixture
def modes(ctx):
    yield ctx
    ctx.set_icp_search("auto")
    ctx.set_icp_accumulation("tree")


# ---------------------------------------------------------------- 1. bits against single calls
@pytest.mark.parametrize("search", ["auto", "brute", "pruned", "grid"])
@pytest.mark.parametrize("acc", ["tree", "reference"])
@pytest.mark.parametrize("kind", ["plane", "point", "no_normals"])
def test_batch_equals_single_calls(modes, synth, search, acc, kind):
    ctx = modes
    ctx.set_icp_search(search)
    ctx.set_icp_accumulation(acc)
    tgt, nrm = synth.sample_object(6000, 42)
    clouds, T0s = _instances(synth, [3000, 20000, 700, 9000])      # 20,000 x 6,000 >= 1e8: grid shape; the others: brute-force shape
    _, s = _batch_vs_single(ctx, clouds, T0s, tgt, None if kind == "no_normals" else nrm, 0.004, 30, kind == "plane")
    if acc == "tree" and search in ("auto", "grid"):
        assert s == "grid"


@pytest.mark.parametrize("K", [1, 4, 33])
@pytest.mark.parametrize("search", ["auto", "grid", "brute"])
def test_fixed_iterations_equal_single_calls(modes, synth, K, search):
    ctx = modes
    ctx.set_icp_search(search)
    tgt, nrm = synth.sample_object(6000, 42)
    clouds, T0s = _instances(synth, [2500, 18000, 400])
    got, _ = _batch_vs_single(ctx, clouds, T0s, tgt, nrm, 0.004, K, True, True)
    assert all(g.iterations == K for g in got)


# ---------------------------------------------------------------- 2. mixed batches
@pytest.mark.parametrize("acc", ["tree", "reference"])
def test_mixed_batch(modes, synth, acc):
    """Stragglers, a start pose too far off for 3 correspondences, an empty cloud in the middle, and instance sizes either side of
    the brute / pruned split ns * nt = 1e8 at nt = 20,000 (both accumulation shapes in one batch)."""
    ctx = modes
    ctx.set_icp_accumulation(acc)
    tgt, nrm = synth.sample_object(20000, 42)
    clouds, T0s = _instances(synth, [4999, 5000, 0, 5001, 3000, 6000, 2000])
    T0s[4] = synth.perturb(T0s[4], seed=5, angle_deg=1.0, trans=0.5)        # 0.5 m off: no correspondence within the threshold
    T0s[5] = synth.perturb(T0s[5], seed=6, angle_deg=12.0, trans=0.02)      # far: a straggler
    got, s = _batch_vs_single(ctx, clouds, T0s, tgt, nrm, 0.004, 25)
    assert got[2].iterations == 0 and got[2].transformation.tobytes() == T0s[2].astype(np.float32).tobytes()
    assert got[4].iterations == 0 and got[4].transformation.tobytes() == T0s[4].astype(np.float32).tobytes()
    its = [g.iterations for g in got]
    assert len(set(its) - {0}) >= 2, its
    if acc == "tree":
        assert s == "grid"
    print("iterations", its)


# ---------------------------------------------------------------- 3. bits against the oracle
@pytest.mark.parametrize("p2p", [True, False])
def test_reference_sums_equal_the_oracle(modes, synth, orc, p2p):
    ctx = modes
    ctx.set_icp_accumulation("reference")
    tgt, nrm = synth.sample_object(5000, 42)
    clouds, T0s = _instances(synth, [3000, 0, 12000, 800])
    cat, off = _concat(clouds)
    keep_s, d_src = _up(cat)
    keep_t, d_tgt = _up(tgt)
    keep_n, d_nrm = _up(nrm)
    got = ctx.icp_batch_dev(d_src, off, d_tgt, d_nrm, len(tgt), T0s, 0.004, 30, p2p)
    for b, c in enumerate(clouds):
        r = orc.icp(c, tgt, nrm, T0s[b], 0.004, 30, p2p)
        assert got[b].transformation.tobytes() == r["T"].tobytes(), b
        assert got[b].iterations == r["iterations"] and np.float32(got[b].rmse).tobytes() == np.float32(r["rmse"]).tobytes(), b


# ---------------------------------------------------------------- 4. launch count
@pytest.mark.parametrize("B", [1, 32])
def test_one_search_launch_per_iteration_for_the_whole_batch(modes, tdv, synth, B):
    ctx = modes
    tgt, nrm = synth.sample_object(6000, 42)
    clouds, T0s = _instances(synth, [3000 + 50 * b for b in range(B)])
    cat, off = _concat(clouds)
    keep_s, d_src = _up(cat)
    keep_t, d_tgt = _up(tgt)
    keep_n, d_nrm = _up(nrm)
    ctx.timing_enable(True)
    try:
        ctx.timing_read(tdv.TIMER_ICP_NN)                     # reset
        got = ctx.icp_batch_dev(d_src, off, d_tgt, d_nrm, len(tgt), T0s, 0.004, 40, True, True)
        _, launches = ctx.timing_read(tdv.TIMER_ICP_NN)
    finally:
        ctx.timing_enable(False)
    assert ctx.last_icp_search() == "grid"
    assert launches == 40, launches
    assert all(g.iterations == 40 for g in got)


# ---------------------------------------------------------------- 5. full size
def test_full_size(modes, synth):
    ctx = modes
    tgt, nrm = synth.sample_object(150000, 42)
    sizes = [100000 + 7000 * b for b in range(8)]
    clouds, T0s = _instances(synth, sizes, spread=0.1)                       # 0.3 deg, 0.5 mm
    thr = synth.mean_spacing(150000)                                          # 0.8 mm: the model's point spacing
    got, s = _batch_vs_single(ctx, clouds, T0s, tgt, nrm, thr, 30)
    assert s == "grid"
    print("iterations", [g.iterations for g in got], "fitness", [float(g.fitness) for g in got])


# ---------------------------------------------------------------- 6. the refine call
def _scene(synth, n_inst, w=640, h=480, far=()):
    """A depth frame with n_inst copies of the object, one mask each; instance poses in the camera frame.  Instances listed in `far`
    are pushed beyond zmax (status 2); a last extra mask over an empty region gives status 1 when asked for with n_inst + 1."""
    f = 600.0
    cx, cy = w / 2.0, h / 2.0
    depth = np.zeros((h, w), np.uint16)
    masks = np.zeros((n_inst + 1, h, w), np.uint8)
    model, _ = synth.sample_object(60000, 42)
    poses = []
    for b in range(n_inst):
        z = 2.0 if b in far else 0.55 + 0.03 * b
        T = synth.make_transform([0.3 + 0.2 * b, 1.0, 0.4 - 0.3 * b], 25.0 + 10 * b, (-0.15 + 0.15 * (b % 3), -0.08 + 0.08 * (b // 3), z))
        poses.append(T)
        p = model.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3]
        u = np.round(p[:, 0] / p[:, 2] * f + cx).astype(int); v = np.round(p[:, 1] / p[:, 2] * f + cy).astype(int)
        ok = (u >= 0) & (u < w) & (v >= 0) & (v < h) & (p[:, 2] > 0)
        zb = np.full((h, w), np.inf)
        np.minimum.at(zb, (v[ok], u[ok]), p[ok, 2])
        hit = np.isfinite(zb) & (depth == 0)
        depth[hit] = np.round(zb[hit] * 1000.0).astype(np.uint16)
        masks[b][hit] = 255
    masks[n_inst][:4, :4] = 255                               # no depth there: status 1
    return depth, masks, dict(fx=f, fy=f, cx=cx, cy=cy, width=w, height=h), poses


def _model(ctx, tdv, synth, voxel):
    raw, _ = synth.sample_object(20000, 7)
    d_raw = torch.from_numpy(raw).to(DEV)
    d_mx = torch.empty_like(d_raw); d_mn = torch.empty_like(d_raw)
    d_mf = torch.empty((len(raw), 33), dtype=torch.float32, device=DEV)
    nm = ctx.prepare_model_dev(d_raw.data_ptr(), len(raw), voxel, 30, 5.0, d_mx.data_ptr(), d_mn.data_ptr(), d_mf.data_ptr(), order=tdv.TDV_VOXEL_ORDER_FIRST)
    return d_mx, d_mn, nm


def _start_poses(synth, poses, n):
    out = []
    for b in range(n):
        T = np.linalg.inv(poses[b].astype(np.float64)).astype(np.float32) if b < len(poses) else np.eye(4, dtype=np.float32)
        out.append(synth.perturb(T, seed=300 + b, angle_deg=0.5, trans=0.001))
    return np.stack(out)


@pytest.mark.parametrize("order", ["first", "reference"])
@pytest.mark.parametrize("layout", ["stacked", "u8_labels", "u16_labels", "resized", "two_frames"])
def test_refine_equals_stagewise_chain(modes, tdv, synth, order, layout):
    ctx = modes
    voxel = 0.004
    vo = tdv.TDV_VOXEL_ORDER_FIRST if order == "first" else tdv.TDV_VOXEL_ORDER_REFERENCE
    depth, masks, intr, poses = _scene(synth, 4, far=(2,))
    n_inst = len(masks)                                       # 4 rendered instances (one beyond zmax) + one mask without depth
    d_mx, d_mn, nm = _model(ctx, tdv, synth, voxel)
    mx = d_mx[:nm].cpu().numpy(); mn = d_mn[:nm].cpu().numpy()
    T0s = _start_poses(synth, poses, n_inst)
    extra = {}
    frames = [depth] * n_inst
    inst_masks = list(masks)
    if layout == "stacked":
        d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)
    elif layout in ("u8_labels", "u16_labels"):
        lab = np.zeros(depth.shape, np.uint8 if layout == "u8_labels" else np.uint16)
        for b in range(n_inst):
            lab[masks[b] > 0] = b + 1
        inst_masks = [np.where(lab == b + 1, 255, 0).astype(np.uint8) for b in range(n_inst)]
        d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV)
        d_masks = torch.from_numpy(lab.view(np.uint8).reshape(-1).copy()).to(DEV)
        extra = dict(mask_format=1 if layout == "u8_labels" else 2)
    elif layout == "resized":
        small = np.stack([ctx.mask_resize_nearest(m[None], 320, 240)[0] for m in masks])
        inst_masks = [ctx.mask_resize_nearest(m[None], 640, 480)[0] for m in small]
        d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(small).to(DEV)
        extra = dict(mask_width=320, mask_height=240)
    else:                                                     # two frames: the second is the first shifted by 0.5 mm in depth
        depth2 = np.where(depth > 0, depth + 1, 0).astype(np.uint16)
        fmap = np.array([0, 1, 0, 1, 1][:n_inst], np.int32)
        frames = [depth if f == 0 else depth2 for f in fmap]
        d_depth = torch.from_numpy(np.stack([depth, depth2]).view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)
        extra = dict(n_frames=2, frame_of_instance=fmap)
    prm = tdv.batch_params(voxel_size=voxel, zmax=1.5, icp_max_iterations=30, voxel_order=vo, **intr, **extra)
    res = ctx.refine_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm, T0s, d_mx.data_ptr(), d_mn.data_ptr(), nm)
    assert len(res) == n_inst
    for b, r in enumerate(res):
        assert r["coarse_fitness"] == -1 and r["coarse_inliers"] == -1
        xyz, _ = ctx.depth_to_cloud(frames[b], inst_masks[b], None, 1000.0, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 1.5)
        assert r["n_points"] == len(xyz), b
        if len(xyz) == 0:
            assert r["status"] == (2 if b == 2 else 1), (b, r["status"])
            assert r["T"].tobytes() == T0s[b].tobytes() and r["fitness"] == 0 and r["rmse"] == 0 and r["icp_iterations"] == 0
            continue
        assert r["status"] == 0
        src, _ = ctx.voxel_downsample(xyz, None, voxel, vo)
        assert r["n_voxels"] == len(src)
        fine = ctx.icp(src, mx, mn, T0s[b], voxel * 0.4, 30, True)
        assert r["icp_iterations"] == fine.iterations, b
        assert fine.iterations > 0 or b == 2, b               # (instance 2 lies beyond zmax: a resized mask only catches a neighbour's edge)
        assert r["T"].tobytes() == fine.transformation.tobytes() and r["fitness"] == fine.fitness and r["rmse"] == fine.rmse, b


def test_refine_reference_sums_equal_the_oracle_chain(modes, tdv, synth, orc):
    ctx = modes
    ctx.set_icp_accumulation("reference")
    voxel = 0.004
    depth, masks, intr, poses = _scene(synth, 3)
    n_inst = 3
    masks = masks[:n_inst]
    d_mx, d_mn, nm = _model(ctx, tdv, synth, voxel)
    mx = d_mx[:nm].cpu().numpy(); mn = d_mn[:nm].cpu().numpy()
    T0s = _start_poses(synth, poses, n_inst)
    prm = tdv.batch_params(voxel_size=voxel, zmax=1.5, icp_max_iterations=30, voxel_order=tdv.TDV_VOXEL_ORDER_REFERENCE, **intr)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)
    res = ctx.refine_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm, T0s, d_mx.data_ptr(), d_mn.data_ptr(), nm)
    for b, r in enumerate(res):
        xyz, _ = orc.unproject(orc.depth_preprocess(depth, masks[b], 1000.0), None, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 1.5)
        src, _, _ = orc.voxel_downsample(xyz, None, voxel)
        e = orc.icp(src, mx, mn, T0s[b], voxel * 0.4, 30, True)
        assert r["n_voxels"] == len(src)
        assert r["T"].tobytes() == e["T"].tobytes() and r["icp_iterations"] == e["iterations"], b
        assert np.float32(r["rmse"]).tobytes() == np.float32(e["rmse"]).tobytes(), b


# ---------------------------------------------------------------- 7. edge cases and hygiene
def _raw_call(tdv, ctx, d_src, off, n, d_tgt, d_nrm, nt, T0, iters, fixed=0):
    """tdv_icp_batch_dev with n + 1 result slots, every byte NaN; returns (status, results array)."""
    res = (tdv.IcpResultC * (n + 1))()
    C.memset(res, 0xFF, C.sizeof(res))
    offs = None if off is None else (C.c_int * len(off))(*[int(x) for x in off])
    t0 = None if T0 is None else np.ascontiguousarray(np.concatenate([tdv.to_colmajor16(T) for T in T0]) if len(T0) else np.zeros(16, np.float32))
    st = tdv.lib().tdv_icp_batch_dev(ctx._h, C.c_void_p(d_src), offs, n, C.c_void_p(d_tgt), C.c_void_p(d_nrm) if d_nrm else None, nt,
                                      None if t0 is None else t0.ctypes.data_as(C.c_void_p), C.c_float(0.004), iters, 1, fixed, res)
    return st, res


def _untouched(res, slots):
    raw = np.frombuffer(res, np.uint8).reshape(len(res), -1)
    return all((raw[s] == 0xFF).all() for s in slots)


def test_edge_cases_and_bad_arguments(modes, tdv, synth):
    ctx = modes
    tgt, nrm = synth.sample_object(6000, 42)
    clouds, T0s = _instances(synth, [3000, 4000])
    cat, off = _concat(clouds)
    keep_s, d_src = _up(cat)
    keep_t, d_tgt = _up(tgt)
    keep_n, d_nrm = _up(nrm)
    # B = 0
    st, res = _raw_call(tdv, ctx, d_src, [0], 0, d_tgt, d_nrm, len(tgt), T0s[:0], 30)
    assert st == 0 and _untouched(res, [0])
    assert ctx.icp_batch_dev(d_src, [0], d_tgt, d_nrm, len(tgt), np.zeros((0, 4, 4), np.float32), 0.004, 30) == []
    # B = 1: the single call's bits, the extra slot untouched
    st, res = _raw_call(tdv, ctx, d_src, off[:2], 1, d_tgt, d_nrm, len(tgt), T0s[:1], 30)
    assert st == 0 and _untouched(res, [1])
    ref = ctx.icp_dev(d_src, int(off[1]), d_tgt, d_nrm, len(tgt), T0s[0], 0.004, 30)
    assert tdv.from_colmajor16(res[0].T).tobytes() == ref.transformation.tobytes() and res[0].iterations == ref.iterations
    # max_iterations = 0: the start poses back
    st, res = _raw_call(tdv, ctx, d_src, off, 2, d_tgt, d_nrm, len(tgt), T0s, 0)
    assert st == 0 and _untouched(res, [2])
    for b in range(2):
        assert tdv.from_colmajor16(res[b].T).tobytes() == T0s[b].astype(np.float32).tobytes() and res[b].iterations == 0 and res[b].n_corr == 0
    # bad arguments: nothing written
    for bad_off, T0, nt in (([1, 3000, 7000], T0s, len(tgt)),            # not starting at 0
                            ([0, 4000, 3000], T0s, len(tgt)),            # decreasing
                            (off, None, len(tgt)),                      # no start poses
                            (off, T0s, -1)):                            # negative nt
        st, res = _raw_call(tdv, ctx, d_src, bad_off, 2, d_tgt, d_nrm, nt, T0, 30)
        assert st == TDV_ERR_BAD_ARG and _untouched(res, [0, 1, 2]), (bad_off, nt)
    # refine: a null T0 and a bad voxel order are refused before anything runs, the results untouched
    depth, masks, intr, poses = _scene(synth, 2)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)
    d_mx, d_mn, nm = _model(ctx, tdv, synth, 0.004)
    for T0, vo in ((None, tdv.TDV_VOXEL_ORDER_FIRST), (_start_poses(synth, poses, 3), 7)):
        prm = tdv.batch_params(voxel_size=0.004, zmax=1.5, icp_max_iterations=30, voxel_order=vo, **intr)
        rr = (tdv.InstanceResultC * 4)()
        C.memset(rr, 0xFF, C.sizeof(rr))
        t0 = None if T0 is None else np.concatenate([tdv.to_colmajor16(T) for T in T0])
        st = tdv.lib().tdv_refine_batch_dev(ctx._h, C.c_void_p(d_depth.data_ptr()), None, C.c_void_p(d_masks.data_ptr()), 3, C.byref(prm),
                                            None if t0 is None else t0.ctypes.data_as(C.c_void_p), C.c_void_p(d_mx.data_ptr()), C.c_void_p(d_mn.data_ptr()), nm, rr)
        assert st == TDV_ERR_BAD_ARG and _untouched(rr, [0, 1, 2, 3])
    # refine with B = 0
    prm = tdv.batch_params(voxel_size=0.004, zmax=1.5, icp_max_iterations=30, **intr)
    assert ctx.refine_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), 0, prm, np.zeros((0, 4, 4), np.float32), d_mx.data_ptr(), d_mn.data_ptr(), nm) == []
