"""Every stage against the CPU oracle on poisoned input: NaN, +-inf, finite coordinates whose voxel index lies outside int
range, coordinates whose square overflows f32 (1e19), -0.0 and subnormals, in one coordinate or a whole row, at row 0, the
last row and rows on workgroup and tile edges.  This is where the device and x86 can give different answers for the same C++.

Comparison: NaN positions equal, every other value equal byte for byte (NaN payloads are not compared: x86's default NaN is
negative, the GPU's positive); indices, counts, order and status exactly equal.

The voxel key is the reference's static_cast<int>(std::floor(x * inv)), which is undefined in C++ for NaN and out-of-range
values; the project's rule (include/tdv_hip.h, tdv_voxel_downsample) is x86's cvttss2si: such a coordinate gets INT_MIN."""
import os

import numpy as np
import pytest
import torch
from test_gpu_batch import _scene as _batch_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

NEG_NAN = np.frombuffer(np.uint32(0xffc00000).tobytes(), np.float32)[0]     # x86's default NaN: sign bit set
POISON = {"nan": NEG_NAN, "inf": np.inf, "ninf": -np.inf, "big": 3e7, "nbig": -3e7, "sq_overflow": 1e19,
          "negzero": -0.0, "subnormal": 1e-40}


def _same(got, ref, what=""):
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, np.argwhere(gn != rn)[:5])
    assert got[~gn].tobytes() == ref[~rn].tobytes(), what


def _rows(n, where):
    return {"first": [0], "last": [n - 1], "edges": [r for r in (255, 256, 4095, 4096) if r < n],
            "few": [3, n // 3, n - 2], "half": list(range(0, n, 2))}[where]


def _poison(pts, val, rows, col):
    p = pts.copy()
    if col == "row":
        p[rows] = np.float32(val)
    else:
        p[rows, col] = np.float32(val)
    return p


def _env(**kv):
    class _E:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kv}
            os.environ.update({k: str(v) for k, v in kv.items()})

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- voxel keys
def test_six_point_cloud_one_poisoned_voxel(ctx, orc, tdv):
    """NaN, +inf, -inf and x = 3e7 m at 1 cm voxels all key (INT_MIN, 0, 0) on x86: one voxel with a NaN centroid; the two
    points near the origin are their own clean voxel."""
    pts = np.array([[0.001, 0.002, 0.003], [np.nan, 0.001, 0.001], [np.inf, 0.002, 0.002], [-np.inf, 0.003, 0.003],
                    [3e7, 0.004, 0.004], [0.002, 0.001, 0.001]], np.float32)
    ref, _, first = orc.voxel_downsample(pts, None, 0.01)
    assert len(ref) == 2 and sorted(first.tolist()) == [0, 1]
    for order in (tdv.TDV_VOXEL_ORDER_REFERENCE, tdv.TDV_VOXEL_ORDER_FIRST):
        exp = ref if order == tdv.TDV_VOXEL_ORDER_REFERENCE else ref[np.argsort(first, kind="stable")]
        for dev_order in ("0", "1"):
            with _env(TDV_VOXEL_DEVICE_ORDER=dev_order):
                got, _ = ctx.voxel_downsample(pts, None, 0.01, order)
            _same(got, exp, (order, dev_order))


def test_int_range_edges_of_the_key(ctx, orc, tdv):
    """At 1 m voxels: -2^31 is a real key that the poisoned values share; 2^31 and below -2^31 are out of range; the largest float
    below 2^31 is in range."""
    vals = [2147483648.0, 2147483520.0, -2147483648.0, -2147483904.0, 1e19, -1e19, np.nan, -0.0, 1e-40, -1e-40, 0.5, 1.5]
    pts = np.zeros((len(vals) * 3, 3), np.float32)
    for i, v in enumerate(vals):
        for c in range(3):
            pts[3 * i + c, c] = v
    rgb = np.random.default_rng(0).random(pts.shape).astype(np.float32)
    ref_xyz, ref_rgb, first = orc.voxel_downsample(pts, rgb, 1.0)
    perm = np.argsort(first, kind="stable")
    for dev_order in ("0", "1"):
        with _env(TDV_VOXEL_DEVICE_ORDER=dev_order):
            got_xyz, got_rgb = ctx.voxel_downsample(pts, rgb, 1.0, tdv.TDV_VOXEL_ORDER_REFERENCE)
        _same(got_xyz, ref_xyz, dev_order); _same(got_rgb, ref_rgb, dev_order)
    got_xyz, got_rgb = ctx.voxel_downsample(pts, rgb, 1.0, tdv.TDV_VOXEL_ORDER_FIRST)
    _same(got_xyz, ref_xyz[perm]); _same(got_rgb, ref_rgb[perm])


@pytest.mark.parametrize("kind", list(POISON))
@pytest.mark.parametrize("where", ["first", "last", "edges", "few", "half"])
def test_voxel_downsample_poisoned(ctx, orc, synth, tdv, kind, where):
    """Host replay and device order (reference order), first-occurrence order, the device entry point in both orders."""
    n, voxel = 5000, 0.004
    base, _ = synth.sample_object(n, 3)
    base = base - np.float32(0.05)                       # mixed-sign keys
    rows = _rows(n, where)
    for col in (0, 2, "row"):
        pts = _poison(base, POISON[kind], rows, col)
        rgb = np.random.default_rng(n).random((n, 3)).astype(np.float32)
        ref_xyz, ref_rgb, first = orc.voxel_downsample(pts, rgb, voxel)
        perm = np.argsort(first, kind="stable")
        m = len(ref_xyz)
        for dev_order in ("0", "1"):
            with _env(TDV_VOXEL_DEVICE_ORDER=dev_order):
                got_xyz, got_rgb = ctx.voxel_downsample(pts, rgb, voxel, tdv.TDV_VOXEL_ORDER_REFERENCE)
            _same(got_xyz, ref_xyz, (kind, where, col, dev_order)); _same(got_rgb, ref_rgb, (kind, where, col, dev_order))
        got_xyz, _ = ctx.voxel_downsample(pts, None, voxel, tdv.TDV_VOXEL_ORDER_FIRST)
        _same(got_xyz, ref_xyz[perm], (kind, where, col, "first"))
        d_in = _dev(pts)
        for order, exp in ((tdv.TDV_VOXEL_ORDER_FIRST, ref_xyz[perm]), (tdv.TDV_VOXEL_ORDER_REFERENCE, ref_xyz)):
            d_out = torch.empty((m, 3), dtype=torch.float32, device=DEV)
            assert ctx.voxel_downsample_dev(d_in.data_ptr(), None, n, voxel, d_out.data_ptr(), None, m, order=order) == m
            _same(d_out.cpu().numpy(), exp, (kind, where, col, "dev", order))


@pytest.mark.parametrize("kind", ["nan", "inf", "big", "sq_overflow"])
def test_voxel_batch_poisoned_and_clean_clouds(ctx, orc, synth, kind):
    """One batch of clouds, some poisoned: every cloud's voxels equal the oracle's in first-occurrence order."""
    voxel = 0.004
    clouds = []
    for b, (n, where) in enumerate(((5000, "edges"), (300, "first"), (4097, "last"), (1000, None), (2600, "half"))):
        pts, _ = synth.sample_object(n, 10 + b)
        if where is not None:
            pts = _poison(pts, POISON[kind], _rows(n, where), b % 3)
        clouds.append(pts)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    d_xyz = _dev(np.concatenate(clouds, 0))
    d_out = torch.empty_like(d_xyz)
    voff = ctx.voxel_downsample_batch_dev(d_xyz.data_ptr(), off, voxel, d_out.data_ptr())
    out = d_out.cpu().numpy()
    for b, c in enumerate(clouds):
        ref, _, first = orc.voxel_downsample(c, None, voxel)
        _same(out[voff[b]:voff[b + 1]], ref[np.argsort(first, kind="stable")], (kind, b))


def test_depth_to_voxels_with_nan_and_inf_depth(ctx, orc):
    """Float depth holding NaN and +-inf: deproject keeps the NaN pixels (as the reference does) and drops the infinite ones; the
    voxel stage on that cloud equals the oracle through the operator API, the batch table and the pinhole batch, which must hand a
    poisoned cloud to the table."""
    h, w, fx, fy, cx, cy = 120, 160, 500.0, 500.0, 80.0, 60.0
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (0.5 + 0.0002 * xx + 0.0001 * yy).astype(np.float32)
    clean_xyz, _ = ctx.deproject(depth, None, fx, fy, cx, cy, 1.5)
    d = depth.copy()
    d[0, 0] = np.nan; d[h - 1, w - 1] = np.nan; d[1, 95] = np.nan; d[50, 3] = np.inf; d[60, 7] = -np.inf; d[25, 100] = np.nan
    xyz, _ = ctx.deproject(d, None, fx, fy, cx, cy, 1.5)
    ref_cloud, _ = orc.unproject(d, None, fx, fy, cx, cy, 1.5)
    _same(xyz, ref_cloud)
    assert len(xyz) == h * w - 2 and np.isnan(xyz).any()
    voxel = 0.0015
    for cloud, poisoned in ((clean_xyz, False), (xyz, True)):
        ref, _, first = orc.voxel_downsample(cloud, None, voxel)
        _same(ctx.voxel_downsample(cloud, None, voxel)[0], ref)
        exp = ref[np.argsort(first, kind="stable")]
        off = np.array([0, len(cloud)], np.int32)
        d_xyz = _dev(cloud)
        for pinhole in (None, (fx, fy, cx, cy)):
            d_out = torch.empty_like(d_xyz)
            voff = ctx.voxel_downsample_batch_dev(d_xyz.data_ptr(), off, voxel, d_out.data_ptr(), pinhole=pinhole)
            _same(d_out.cpu().numpy()[:voff[1]], exp, (poisoned, pinhole))
            if pinhole is not None:
                assert ctx.last_voxel_grouping() == ("table" if poisoned else "pixels")


# ---------------------------------------------------------------- descriptor match
@pytest.mark.parametrize("ns,nt", [(300, 200), (4500, 2500)])
def test_feature_match_overflowing_descriptors(ctx, orc, synth, ns, nt):
    """1e19 descriptors: every squared distance to them is +inf, so the lowest-index rule decides."""
    fs = synth.random_features(ns, 3); ft = synth.random_features(nt, 4)
    big_t = np.full_like(ft, 1e19)
    assert np.array_equal(ctx.feature_match(fs, big_t), orc.feature_match(fs, big_t))
    assert not orc.feature_match(fs, big_t).any()
    ft2 = ft.copy(); ft2[::3] = 1e19
    fs2 = fs.copy(); fs2[::5] = 1e19
    assert np.array_equal(ctx.feature_match(fs2, ft2), orc.feature_match(fs2, ft2))


# ---------------------------------------------------------------- RANSAC
def _ransac_scene(ctx, synth, n, seed, kind):
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < 0.5, nn, rng.integers(0, n, n)).astype(np.int32)
    rows = rng.choice(n, 60, replace=False)
    src = src.copy(); tgt = tgt.copy()
    if kind in ("inf_target", "both"):
        tgt[corr[rows[:30]], rng.integers(0, 3, 30)] = np.where(rng.random(30) < 0.5, np.inf, -np.inf).astype(np.float32)
        tgt[corr[rows[30]]] = np.inf
    if kind in ("nan_source", "both"):                 # one coordinate per row, no whole NaN row; most of them negative NaNs (x86's default
        cols = rng.integers(0, 3, 29)                  # NaN, 0xffc00000), whose sign bit the fast pass must not read as "inlier"
        src[rows[31:], cols] = np.where(rng.random(29) < 0.7, NEG_NAN, np.nan).astype(np.float32)
        src[0, 1] = NEG_NAN
        assert np.signbit(src[rows[31:], cols]).any()
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _result(r):
    return (r.best_iteration, r.iterations_run, r.inliers, r.fitness, r.transformation.tobytes(), np.float32(r.rmse).tobytes())


@pytest.mark.parametrize("kind", ["inf_target", "nan_source", "both"])
def test_ransac_non_finite(ctx, orc, synth, kind):
    """Every hypothesis' count (trace) and the winner - iteration, iterations run, inliers, fitness, T, rmse - equal the oracle's with
    the fast pass, the exact pass, the leaf bound off and on."""
    src, tgt, corr, voxel = _ransac_scene(ctx, synth, 20000, 11, kind)
    iters = 20000
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True, exact=True)
    assert ref["best_iter"] >= 0 and not ref["rmse_ambiguous"]
    traced = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True)
    assert np.array_equal(traced.trace_inliers, ref["inliers"]), np.nonzero(traced.trace_inliers != ref["inliers"])[0][:5]
    runs = {"fast": ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)}
    with _env(TDV_RANSAC_BOUND=0):
        runs["no bound"] = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
    try:
        ctx.set_ransac_score("exact")
        runs["exact"] = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
    finally:
        ctx.set_ransac_score("fast")
    inl = int(ref["inliers"][ref["best_iter"]])
    exp = (ref["best_iter"], ref["iters_run"], inl, ref["fitness"], ref["T"].tobytes(), ref["rmse"].tobytes())
    for name, r in runs.items():
        assert _result(r) == exp, (name, _result(r)[:4], exp[:4])
    # an early exit: the confidence bound stops the loop at the first hypothesis past it
    conf = float(np.float32(inl) / np.float32(len(src))) * 0.5
    ref2 = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=conf, exact=True)
    got2 = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=conf)
    assert (got2.best_iteration, got2.iterations_run, got2.transformation.tobytes()) == (ref2["best_iter"], ref2["iters_run"], ref2["T"].tobytes())


# ---------------------------------------------------------------- ICP
def _icp_problem(synth, ns, nt, seed):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(ns, seed)
    return src, tgt, nrm, synth.perturb(T_gt)


def _poison_icp(src, tgt, nrm, kind, rng):
    src = src.copy(); tgt = tgt.copy(); nrm = nrm.copy()
    rs = np.unique(np.concatenate([[0, len(src) - 1], rng.choice(len(src), 20, replace=False)]))
    rt = np.unique(np.concatenate([[0, len(tgt) - 1], rng.choice(len(tgt), 20, replace=False)]))
    if kind == "src_nan":
        src[rs, rng.integers(0, 3, len(rs))] = np.nan
    elif kind == "src_inf":
        src[rs, rng.integers(0, 3, len(rs))] = np.inf
    elif kind == "tgt_inf":
        tgt[rt, rng.integers(0, 3, len(rt))] = -np.inf
    elif kind == "tgt_nan":
        tgt[rt] = np.nan
    elif kind == "tgt_huge":
        tgt[rt, rng.integers(0, 3, len(rt))] = 1e19
    elif kind == "nrm_nan":
        nrm[rt] = np.nan
    elif kind == "nrm_inf":                             # r = (p - q) . n and J are infinite or NaN
        nrm[rt, rng.integers(0, 3, len(rt))] = np.where(rng.random(len(rt)) < 0.5, np.inf, -np.inf).astype(np.float32)
    elif kind == "nrm_huge":                            # r finite, J[a] * J[b] overflows f32 to +inf
        nrm[rt, rng.integers(0, 3, len(rt))] = 1e20
    return src, tgt, nrm


ICP_KINDS = ["src_nan", "src_inf", "tgt_inf", "tgt_nan", "tgt_huge", "nrm_nan", "nrm_inf", "nrm_huge"]


@pytest.mark.parametrize("kind", ICP_KINDS)
@pytest.mark.parametrize("ns,nt", [(3000, 2500), (300, 200)])
def test_icp_correspondences_poisoned(ctx, orc, synth, kind, ns, nt):
    """Every search on poisoned clouds; a grid that flags a target hands over to the box walk and says so."""
    src, tgt, nrm, T0 = _icp_problem(synth, ns, nt, 5)
    src, tgt, nrm = _poison_icp(src, tgt, nrm, kind, np.random.default_rng(ns))
    thr = 0.004
    ref = orc.icp_correspondences(src, tgt, None, T0, thr, point_to_plane=False)
    acc = ref["accepted"].astype(bool)
    try:
        for search in ("auto", "brute", "pruned", "grid"):
            ctx.set_icp_search(search)
            got = ctx.icp_correspondences(src, tgt, T0, thr)
            assert np.array_equal(got["accepted"], ref["accepted"]), (search, kind)
            assert np.array_equal(got["corr"][acc], ref["corr"][acc]), (search, kind)
            assert got["d2"][acc].tobytes() == ref["d2"][acc].tobytes(), (search, kind)
            assert got["n_corr"] == ref["n_corr"], (search, kind)
            if search == "grid" and kind in ("tgt_inf", "tgt_nan", "tgt_huge"):
                assert ctx.last_icp_search() == "pruned", kind
    finally:
        ctx.set_icp_search("auto")


@pytest.mark.parametrize("kind", ICP_KINDS)
@pytest.mark.parametrize("p2plane", [True, False])
def test_icp_loop_poisoned(ctx, orc, synth, kind, p2plane):
    """Full loops: reference-order sums equal the oracle bit for bit under every search; the default tree sums equal the
    exact-sum oracle (no sum of these cases lies within the tree's bound of an f32 rounding midpoint)."""
    src, tgt, nrm, T0 = _icp_problem(synth, 3000, 2500, 9)
    src, tgt, nrm = _poison_icp(src, tgt, nrm, kind, np.random.default_rng(1))
    thr = 0.004
    ref = orc.icp(src, tgt, nrm, T0, thr, 30, p2plane)
    try:
        ctx.set_icp_accumulation("reference")
        for search in ("auto", "brute", "pruned", "grid"):
            ctx.set_icp_search(search)
            g = ctx.icp(src, tgt, nrm, T0, thr, 30, p2plane)
            assert g.iterations == ref["iterations"], (search, kind)
            _same(g.transformation, ref["T"], (search, kind))
            _same(np.float32(g.rmse), ref["rmse"], (search, kind)); _same(np.float32(g.fitness), ref["fitness"], (search, kind))
    finally:
        ctx.set_icp_accumulation("tree")
        ctx.set_icp_search("auto")
    ex = orc.icp(src, tgt, nrm, T0, thr, 30, p2plane, exact=True)
    assert not ex["ambiguous"], "%s: a sum lies within the f64 tree's bound of an f32 rounding midpoint - pick another seed" % kind
    g = ctx.icp(src, tgt, nrm, T0, thr, 30, p2plane)
    assert g.iterations == ex["iterations"], kind
    _same(g.transformation, ex["T"], kind)
    _same(np.float32(g.rmse), ex["rmse"], kind)


# ---------------------------------------------------------------- the batch against a poisoned model
@pytest.mark.parametrize("knobs", [dict(), dict(TDV_RANSAC_BATCH=0), dict(TDV_BATCH_VOXEL=0), dict(TDV_RANSAC_BATCH=0, TDV_BATCH_VOXEL=0)])
def test_register_batch_poisoned_model(ctx, tdv, synth, knobs):
    """Model rows with +-inf and (negative) NaN coordinates, normals and descriptors from the clean model: every instance of
    tdv_register_batch_dev equals the operator chain on the same inputs (ctx.ransac, held to the oracle above and checked by its
    own rmse pass; ctx.icp) - with the small-cloud RANSAC batch, which has no rmse pass, and without it; with the batched voxel
    stage and without it."""
    depth, masks, intr = _batch_scene(synth, None)
    voxel = 0.004
    prm = tdv.batch_params(voxel_size=voxel, zmax=1.5, ransac_max_iterations=4000, icp_max_iterations=30, voxel_order=tdv.TDV_VOXEL_ORDER_FIRST, **intr)
    model_raw, _ = synth.sample_object(20000, 7)
    d_raw = _dev(model_raw)
    d_mx = torch.empty_like(d_raw); d_mn = torch.empty_like(d_raw)
    d_mf = torch.empty((len(model_raw), 33), dtype=torch.float32, device=DEV)
    nm = ctx.prepare_model_dev(d_raw.data_ptr(), len(model_raw), voxel, 30, 5.0, d_mx.data_ptr(), d_mn.data_ptr(), d_mf.data_ptr(),
                               order=tdv.TDV_VOXEL_ORDER_FIRST)
    mx = d_mx[:nm].cpu().numpy().copy(); mn = d_mn[:nm].cpu().numpy(); mf = d_mf[:nm].cpu().numpy()
    rng = np.random.default_rng(4)
    rows = rng.choice(nm, nm // 8, replace=False)
    vals = np.array([np.inf, -np.inf, NEG_NAN, np.nan], np.float32)
    mx[rows, rng.integers(0, 3, len(rows))] = vals[rng.integers(0, 4, len(rows))]
    d_mx[:nm].copy_(torch.from_numpy(mx).to(DEV))
    d_depth, d_masks = _dev(depth.view(np.int16)), _dev(masks)          # (held: a temporary's memory goes back to the allocator at once)
    with _env(**knobs):
        res = ctx.register_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), len(masks), prm, d_mx.data_ptr(), d_mn.data_ptr(),
                                     d_mf.data_ptr(), nm)
    for b, r in enumerate(res):
        xyz, _ = ctx.depth_to_cloud(depth, masks[b], None, 1000.0, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 1.5)
        src, _ = ctx.voxel_downsample(xyz, None, voxel, tdv.TDV_VOXEL_ORDER_FIRST)
        assert r["status"] == 0 and r["n_voxels"] == len(src), (knobs, b)
        nrm = ctx.estimate_normals(src, 30)
        fp = ctx.compute_fpfh(src, nrm, voxel * 5.0)
        corr = ctx.feature_match(fp, mf)
        assert np.isin(corr, rows).any(), "no poisoned model row is matched: the case tests nothing"
        coarse = ctx.ransac(src, mx, fs=fp, ft=mf, voxel=voxel, max_iterations=4000, confidence=0.999)
        assert (r["coarse_inliers"], r["coarse_fitness"]) == (coarse.inliers, coarse.fitness), (knobs, b)
        fine = ctx.icp(src, mx, mn, coarse.transformation, voxel * 0.4, 30, True)
        assert r["icp_iterations"] == fine.iterations, (knobs, b)
        _same(r["T"], fine.transformation, (knobs, b))
        _same(np.float32(r["fitness"]), np.float32(fine.fitness)); _same(np.float32(r["rmse"]), np.float32(fine.rmse))


# ---------------------------------------------------------------- FPFH
# The three bins are static_cast<int> of (alpha + 1) * 5.5, (phi + 1) * 5.5 and (theta / pi + 1) * 5.5 in the reference, undefined in
# C++ for NaN and outside int range; the rule (include/tdv_hip.h, tdv_compute_fpfh) is x86's: INT_MIN there, so bin 0.  A normal with
# an infinite component or one far from unit length puts alpha or phi there (+inf, or >= ~3.9e8: the device's own conversion
# saturates those to bin 10).  Poisoned points are in no radius list but their own (d2 <= r2 is false for NaN and for 1e19's
# overflowing square), so every descriptor row is defined.
NORMAL_POISON = {"inf": np.inf, "ninf": -np.inf, "nan": NEG_NAN, "pnan": np.nan, "huge": 1e19, "len3e4": None, "zero": 0.0,
                 "negzero": -0.0, "subnormal": 1e-40}
FPFH_N, FPFH_RADIUS = 5000, 0.008


def _fpfh_cloud(synth):
    from test_gpu_features import _cloud
    return _cloud(synth, FPFH_N)


def _fpfh_rows(where):
    if where == "half":
        return _rows(FPFH_N, "half")
    return _rows(FPFH_N, "first") + _rows(FPFH_N, "last") + _rows(FPFH_N, "edges") + _rows(FPFH_N, "few")


def _poison_normals(nrm, kind, rows, seed):
    nrm = nrm.copy()
    rng = np.random.default_rng(seed)
    if kind == "len3e4":                       # random directions of length 3e4: |alpha| reaches ~9e8
        v = rng.normal(size=(len(rows), 3))
        nrm[rows] = (v / np.linalg.norm(v, axis=1, keepdims=True) * 3e4).astype(np.float32)
    elif kind in ("zero", "negzero", "subnormal"):
        nrm[rows] = np.float32(NORMAL_POISON[kind])
    else:                                      # one component, alternating columns
        nrm[rows, np.arange(len(rows)) % 3] = np.float32(NORMAL_POISON[kind])
    return nrm


def _fpfh_all_entry_points(ctx, orc, pts, nrm, what):
    """tdv_compute_fpfh and tdv_compute_fpfh_dev against the oracle: neighbour lists exact, descriptors bit for bit."""
    ref_d, ref_nb, ref_cnt = orc.compute_fpfh(pts, nrm, FPFH_RADIUS, want_neighbors=True)
    got_d, got_nb, got_cnt = ctx.compute_fpfh(pts, nrm, FPFH_RADIUS, want_neighbors=True)
    assert np.array_equal(got_cnt, ref_cnt) and np.array_equal(got_nb, ref_nb), what
    assert not np.isnan(ref_d).any(), what
    bad = np.nonzero((got_d.view(np.uint32) != ref_d.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (what, "host entry: %d rows differ, first %s" % (len(bad), bad[:8].tolist()))
    n = len(pts)
    d_x, d_n = _dev(pts), _dev(nrm)
    d_f = torch.empty((n, 33), dtype=torch.float32, device=DEV)
    d_nb = torch.empty((n, 100), dtype=torch.int32, device=DEV); d_c = torch.empty(n, dtype=torch.int32, device=DEV)
    ctx.compute_fpfh_dev(d_x.data_ptr(), d_n.data_ptr(), n, FPFH_RADIUS, d_f.data_ptr(), d_nb.data_ptr(), d_c.data_ptr())
    assert np.array_equal(d_c.cpu().numpy(), ref_cnt) and np.array_equal(d_nb.cpu().numpy(), ref_nb), what
    assert d_f.cpu().numpy().tobytes() == ref_d.tobytes(), (what, "device entry")
    return ref_d


@pytest.mark.parametrize("kind", list(NORMAL_POISON))
@pytest.mark.parametrize("where", ["ends_and_edges", "half"])
def test_fpfh_poisoned_normals(ctx, orc, synth, kind, where):
    pts = _fpfh_cloud(synth)
    nrm = orc.estimate_normals(pts, 30)
    rows = _fpfh_rows(where)
    _fpfh_all_entry_points(ctx, orc, pts, _poison_normals(nrm, kind, rows, 1), (kind, where))


def _pairs_where_the_rules_differ(orc, pts, nrm):
    """Pairs (i, j) of the radius lists whose alpha or phi bin a saturating conversion puts in bin 10 and x86's in bin 0:
    (x + 1) * 5.5 = +inf or >= 2^31, in f32 as the kernels form it."""
    _, nb, cnt = orc.compute_fpfh(pts, nrm, FPFH_RADIUS, want_neighbors=True)
    i = np.repeat(np.arange(len(pts)), cnt)
    j = nb[np.arange(100)[None, :] < cnt[:, None]]
    keep = i != j
    i, j = i[keep], j[keep]
    with np.errstate(all="ignore"):
        d = pts[j] - pts[i]
        e = (d / np.sqrt((d * d).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
        u, nj = nrm[i], nrm[j]
        v = np.cross(u, e).astype(np.float32)
        alpha = (v * nj).sum(1, dtype=np.float32); phi = (u * e).sum(1, dtype=np.float32)
        far = lambda x: ((x + np.float32(1)) * np.float32(5.5)) >= np.float32(2147483648.0)   # noqa: E731  (+inf included)
        return int((far(alpha) | far(phi)).sum())


def test_fpfh_saturating_bins_are_reached(orc, synth):
    """The normal poisons above reach the bins where a saturating conversion and x86's differ: else they would test nothing."""
    pts = _fpfh_cloud(synth)
    nrm = orc.estimate_normals(pts, 30)
    for kind, where in (("inf", "ends_and_edges"), ("inf", "half"), ("huge", "ends_and_edges"), ("huge", "half"), ("len3e4", "half")):
        assert _pairs_where_the_rules_differ(orc, pts, _poison_normals(nrm, kind, _fpfh_rows(where), 1)) > 0, (kind, where)


@pytest.mark.parametrize("kind", ["nan", "inf", "ninf", "sq_overflow"])
@pytest.mark.parametrize("col", [0, "row"])
def test_fpfh_poisoned_points(ctx, orc, synth, kind, col):
    """Poisoned coordinates with clean normals, and with infinite normals on the same cloud's half rows."""
    pts = _fpfh_cloud(synth)
    nrm = orc.estimate_normals(pts, 30)
    rows = _rows(FPFH_N, "first") + _rows(FPFH_N, "last") + _rows(FPFH_N, "edges") + list(range(1, FPFH_N, 7))
    bad = _poison(pts, POISON[kind], rows, col)
    _fpfh_all_entry_points(ctx, orc, bad, nrm, (kind, col, "clean normals"))
    _fpfh_all_entry_points(ctx, orc, bad, _poison_normals(nrm, "inf", _rows(FPFH_N, "half"), 2), (kind, col, "inf normals"))


@pytest.mark.parametrize("kind", ["inf", "ninf", "sq_overflow"])
@pytest.mark.parametrize("col", [1, "row"])
def test_normals_fpfh_dev_poisoned_points(ctx, orc, synth, kind, col):
    """tdv_normals_fpfh_dev on a cloud with +-inf / 1e19 rows: normals equal the oracle's on the finite rows (an infinite row's own
    kNN list meets NaN distances, which the reference's partial_sort does not order: test_gpu_fuzz.py); descriptors equal the
    oracle's FPFH of the device's normals on every row."""
    pts = _fpfh_cloud(synth)
    rows = _rows(FPFH_N, "first") + _rows(FPFH_N, "last") + _rows(FPFH_N, "edges") + list(range(2, FPFH_N, 11))
    bad = _poison(pts, POISON[kind], rows, col)
    d_x = _dev(bad); d_n = torch.empty_like(d_x); d_f = torch.empty((FPFH_N, 33), dtype=torch.float32, device=DEV)
    ctx.normals_fpfh_dev(d_x.data_ptr(), FPFH_N, 30, FPFH_RADIUS, d_n.data_ptr(), d_f.data_ptr())
    got_n, got_f = d_n.cpu().numpy(), d_f.cpu().numpy()
    q = np.isfinite(bad).all(1)
    _same(got_n[q], orc.estimate_normals(bad, 30)[q], (kind, col, "normals"))
    assert got_f.tobytes() == orc.compute_fpfh(bad, got_n, FPFH_RADIUS).tobytes(), (kind, col, "descriptors")


@pytest.mark.study
@pytest.mark.parametrize("kind", ["inf", "nan", "huge", "len3e4"])
def test_fpfh_one_point_per_wave_poisoned(ctx, orc, synth, kind):
    """The study library's one-point-per-wave SPFH / FPFH (TDV_FPFH_PAIRS=0) holds the same bins on poisoned normals."""
    pts = _fpfh_cloud(synth)
    nrm = _poison_normals(orc.estimate_normals(pts, 30), kind, _rows(FPFH_N, "half"), 3)
    with _env(TDV_FPFH_PAIRS=0):
        _fpfh_all_entry_points(ctx, orc, pts, nrm, (kind, "one point per wave"))
    _fpfh_all_entry_points(ctx, orc, pts, nrm, (kind, "two points per wave"))
