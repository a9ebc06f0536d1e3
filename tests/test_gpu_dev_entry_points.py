"""The device-resident entry points (include/tdv_hip.h: tdv_*_dev) against their host twins and the CPU oracle.

bench.py times tdv_icp_dev (fixed_iterations) and tdv_ransac_dev (untraced, confidence 2: the exact bail-out); the batch and the
integrators call the feature, voxel and mask entry points.  Every call here takes its inputs from device buffers that start one
point (12 bytes) into a larger allocation, and writes into outputs one element longer than needed and pre-filled with a NaN
sentinel that must survive.  Bars: the host twin bit for bit, the oracle at the precision the host test of the stage uses.

Fixed-iteration ICP has semantics of its own (csrc/icp.hip: icp_update): no convergence stop, an update skipped (pose kept) when
n_corr < 3, and bursts of 32 launches on the multi-launch path.  K fixed iterations are held against K chained one-iteration calls."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = np.frombuffer(np.float32(np.nan).tobytes(), np.int32)[0]     # the NaN bit pattern, also written into int outputs
ROT_TOL, TRANS_TOL = 1e-4, 1e-6                                         # tests/test_gpu_icp.py (BASELINE.json)
RS_HYP_PER_BLOCK = 1024                                                 # csrc/ransac.hip: hypotheses per workgroup; the bail-out's first batch is 8x


# ---------------------------------------------------------------- buffers
def _up(a):
    """a on the device, one row into a buffer one row longer at each end: (tensor view, device pointer)."""
    a = np.ascontiguousarray(a)
    row = int(np.prod(a.shape[1:]))
    base = torch.zeros((len(a) + 2) * row, dtype=getattr(torch, str(a.dtype)), device=DEV)
    if a.size:
        base[row:row + a.size].copy_(torch.from_numpy(a.reshape(-1)).to(DEV))
    torch.cuda.synchronize()                                           # filled on the null stream; the ctx reads it on its own non-blocking stream
    return base, base.data_ptr() + row * a.itemsize                    # (from the base: an empty view's data_ptr() is 0)


def _out(n, row, dtype=torch.float32):
    """An output for n rows of `row` elements plus one more, every element the sentinel's bits."""
    t = torch.full(((n + 1) * row,), int(SENTINEL), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()                                           # the fill must have landed before the ctx's stream writes the buffer
    return t.view(dtype)


def _got(t, n, row, dtype=np.float32):
    """The first n rows, after checking that the element after them still holds the sentinel."""
    h = t.cpu().numpy()
    assert h.view(np.int32)[n * row:].tolist() == [int(SENTINEL)] * row, "write past the end of the output"
    return h.view(dtype)[:n * row].reshape(n, row) if row > 1 else h.view(dtype)[:n]


def _cloud(synth, n, seed=42):
    pts, _ = synth.sample_object(max(n, 1), seed)
    T = synth.gt_transform(seed)
    Ti = np.linalg.inv(T.astype(np.float64))
    return (pts.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)[:n].copy()


def _pair(synth, ns, nt, seed=42):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(ns, seed)
    return src, tgt, nrm, T_gt


# ---------------------------------------------------------------- ICP
@pytest.fixture()
def icp_ctx(ctx):
    yield ctx
    ctx.set_icp_accumulation("tree")
    ctx.set_icp_search("auto")


def _icp_dev(ctx, bufs, T0, thr, iters, p2plane, fixed):
    (ps, ns), (pt, nt), pn = bufs
    return ctx.icp_dev(ps, ns, pt, pn, nt, T0, thr, iters, p2plane, fixed_iterations=fixed)


def _icp_bufs(src, tgt, nrm):
    (bs, ps), (bt, pt), (bn, pn) = _up(src), _up(tgt), _up(nrm)
    return (bs, bt, bn), ((ps, len(src)), (pt, len(tgt)), pn)


def _same_icp(a, b):
    assert a.transformation.tobytes() == b.transformation.tobytes(), (a.transformation, b.transformation)
    assert (a.iterations, a.n_corr) == (b.iterations, b.n_corr)
    assert np.float32(a.rmse).tobytes() == np.float32(b.rmse).tobytes() and np.float32(a.fitness).tobytes() == np.float32(b.fitness).tobytes()


# one-launch loop (k_icp_small: ns, nt <= 2,048 and ns * nt <= 2^18) and the multi-launch loop (bursts; > 2^18 pairs)
PATHS = [(500, 500, "brute"), (5000, 5000, "brute"), (5000, 5000, "pruned"), (5000, 5000, "grid")]


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,nt,search", PATHS + [(500, 500, "pruned")])
def test_icp_dev_equals_host_and_oracle(icp_ctx, orc, synth, ns, nt, search, p2plane):
    src, tgt, nrm, T_gt = _pair(synth, ns, nt)
    T0 = synth.perturb(T_gt)
    keep, bufs = _icp_bufs(src, tgt, nrm)
    icp_ctx.set_icp_search(search)
    got = _icp_dev(icp_ctx, bufs, T0, 0.004, 60, p2plane, False)
    _same_icp(got, icp_ctx.icp(src, tgt, nrm, T0, 0.004, 60, p2plane))
    ref = orc.icp(src, tgt, nrm, T0, 0.004, 60, p2plane)
    assert synth.rotation_angle(ref["T"][:3, :3], got.transformation[:3, :3]) <= ROT_TOL
    assert np.abs(ref["T"][:3, 3].astype(np.float64) - got.transformation[:3, 3]).max() <= TRANS_TOL
    assert abs(got.iterations - ref["iterations"]) <= 1 and abs(float(got.rmse) - float(ref["rmse"])) <= 1e-6
    icp_ctx.set_icp_accumulation("reference")                               # the reference's sums: the oracle to the bit
    e = _icp_dev(icp_ctx, bufs, T0, 0.004, 60, p2plane, False)
    assert e.transformation.tobytes() == ref["T"].tobytes() and e.iterations == ref["iterations"]
    assert np.float32(e.rmse).tobytes() == np.float32(ref["rmse"]).tobytes() and np.float32(e.fitness).tobytes() == np.float32(ref["fitness"]).tobytes()


KS = (1, 4, 31, 32, 33, 70)                                                 # 32: the burst of the multi-launch loop
_CHAINS = {}


def _oracle_chain(orc, src, tgt, nrm, T0, thr, p2plane, kmax):
    """The oracle run one iteration at a time from the pose it left: (T, rmse, fitness, n_corr) after step k, for k = 1..kmax."""
    out, T = [], T0
    for _ in range(kmax):
        r = orc.icp(src, tgt, nrm, T, thr, 1, p2plane, trace=True)
        if r["iterations"] == 0:
            out.append(None)
            continue
        T = r["T"]
        out.append((T, r["rmse"], r["fitness"], int(r["trace"][0, 18])))
    return out


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,nt,search", PATHS)
def test_icp_dev_fixed_iterations(icp_ctx, orc, synth, ns, nt, search, p2plane):
    """K fixed iterations == K chained oracle calls of one iteration (reference sums: bit for bit; tree sums: the north-star
    tolerance, for point-to-point up to the oracle's own stop) and == K chained one-iteration icp_dev calls (tree sums, bit for bit);
    `iterations` is K although the oracle's stopping rule fires earlier."""
    src, tgt, nrm, T_gt = _pair(synth, ns, nt, seed=7)
    T0 = synth.perturb(T_gt, seed=7)
    thr = 0.004
    keep, bufs = _icp_bufs(src, tgt, nrm)
    icp_ctx.set_icp_search(search)
    key = (ns, nt, p2plane)
    if key not in _CHAINS:                                                  # (the oracle scans every pair: one chain per problem, whatever the search)
        _CHAINS[key] = _oracle_chain(orc, src, tgt, nrm, T0, thr, p2plane, max(KS))
    chain = _CHAINS[key]
    assert all(c is not None and c[3] >= 3 for c in chain)
    stop = orc.icp(src, tgt, nrm, T0, thr, max(KS), p2plane)["iterations"]
    assert stop < max(KS), stop                                             # the oracle's own rule stops before the longest run
    icp_ctx.set_icp_accumulation("reference")
    for K in KS:
        g = _icp_dev(icp_ctx, bufs, T0, thr, K, p2plane, True)
        T, rmse, fit, nc = chain[K - 1]
        assert g.iterations == K and g.n_corr == nc, (K, g.iterations, g.n_corr, nc)
        assert g.transformation.tobytes() == T.tobytes(), (K, g.transformation, T)
        assert np.float32(g.rmse).tobytes() == np.float32(rmse).tobytes() and np.float32(g.fitness).tobytes() == np.float32(fit).tobytes(), K
    icp_ctx.set_icp_accumulation("tree")
    steps, T = [], T0
    for _ in range(max(KS)):
        r = _icp_dev(icp_ctx, bufs, T, thr, 1, p2plane, False)
        assert r.iterations == 1
        steps.append(r); T = r.transformation
    for K in KS:
        g = _icp_dev(icp_ctx, bufs, T0, thr, K, p2plane, True)
        s = steps[K - 1]
        assert g.iterations == K and g.n_corr == s.n_corr, (K, g.iterations)
        assert g.transformation.tobytes() == s.transformation.tobytes(), K
        assert np.float32(g.rmse).tobytes() == np.float32(s.rmse).tobytes() and np.float32(g.fitness).tobytes() == np.float32(s.fitness).tobytes()
        if not p2plane and K > stop:
            continue        # point-to-point past the oracle's own stop: the tree's f64 sums and the f32 chain drift apart
        Tr = chain[K - 1][0]
        assert synth.rotation_angle(Tr[:3, :3], g.transformation[:3, :3]) <= ROT_TOL, K
        assert np.abs(Tr[:3, 3].astype(np.float64) - g.transformation[:3, 3]).max() <= TRANS_TOL, K


def _collapsing_case(n_far):
    """30 source points near 40 targets whose normals are random: the point-to-plane updates walk the cloud away, and after 7 updates
    fewer than 3 correspondences remain (found by running the oracle one step at a time).  n_far points far from everything, in
    both clouds, move the problem onto the multi-launch path without changing any correspondence."""
    rng = np.random.default_rng(63)
    tgt = rng.uniform(-0.02, 0.02, (40, 3)).astype(np.float32)
    nrm = rng.normal(size=(40, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    src = (tgt[:30] + rng.normal(0, 0.002, (30, 3))).astype(np.float32)
    if n_far:
        far = np.random.default_rng(5).uniform(-1, 1, (n_far, 3)).astype(np.float32)
        src = np.concatenate([src, far + np.float32(20.0)]); tgt = np.concatenate([tgt, far - np.float32(20.0)])
        nrm = np.concatenate([nrm, np.tile(np.float32([0, 0, 1]), (n_far, 1))])
    return src, tgt, nrm


@pytest.mark.parametrize("n_far", [0, 700])
def test_icp_dev_fixed_iterations_through_too_few_correspondences(icp_ctx, orc, n_far):
    """n_corr drops below 3 at step 8: the fixed run keeps the pose of step 7 (and its rmse, fitness, n_corr), reports 7 applied
    iterations, and runs to its budget without an error - the oracle chain, bit for bit, whatever the budget beyond."""
    src, tgt, nrm = _collapsing_case(n_far)
    T0 = np.eye(4, dtype=np.float32)
    keep, bufs = _icp_bufs(src, tgt, nrm)
    chain = _oracle_chain(orc, src, tgt, nrm, T0, 0.004, True, 12)
    drop = next(k for k, c in enumerate(chain) if c is None)
    assert drop == 7 and all(c is None for c in chain[drop:])
    icp_ctx.set_icp_search("brute")
    icp_ctx.set_icp_accumulation("reference")
    for K in (drop, drop + 1, 33, 40):
        g = _icp_dev(icp_ctx, bufs, T0, 0.004, K, True, True)
        T, rmse, fit, nc = chain[drop - 1]
        assert g.iterations == drop and g.n_corr == nc, (K, g.iterations, g.n_corr)
        assert g.transformation.tobytes() == T.tobytes(), K
        assert np.float32(g.rmse).tobytes() == np.float32(rmse).tobytes() and np.float32(g.fitness).tobytes() == np.float32(fit).tobytes()


@pytest.mark.parametrize("ns,nt", [(0, 5), (5, 0), (1, 1), (1, 40)])
def test_icp_dev_tiny(icp_ctx, synth, ns, nt):
    src, tgt, nrm, T_gt = _pair(synth, max(ns, 1), max(nt, 1))
    src, tgt, nrm = src[:ns], tgt[:nt], nrm[:nt]
    T0 = synth.perturb(T_gt)
    keep, bufs = _icp_bufs(src, tgt, nrm)
    for fixed in (False, True):
        _same_icp(_icp_dev(icp_ctx, bufs, T0, 0.05, 5, True, fixed), icp_ctx.icp(src, tgt, nrm, T0, 0.05, 5, True))


# ---------------------------------------------------------------- RANSAC
def _ransac_case(synth, n, seed=42, good_frac=0.5):
    """Scene = the model moved by T_gt^-1 plus noise; correspondence i -> i for good_frac of the points, random otherwise."""
    tgt, _ = synth.sample_object(n, seed)
    T = synth.gt_transform(seed).astype(np.float64)
    Ti = np.linalg.inv(T)
    rng = np.random.default_rng(seed)
    src = (tgt.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 2e-4, (n, 3))).astype(np.float32)
    corr = np.where(rng.random(n) < good_frac, np.arange(n), rng.integers(0, n, n)).astype(np.int32)
    return src, tgt, corr


def _same_ransac(a, b):
    assert (a.best_iteration, a.iterations_run, a.inliers) == (b.best_iteration, b.iterations_run, b.inliers)
    assert a.transformation.tobytes() == b.transformation.tobytes()
    assert np.float32(a.fitness).tobytes() == np.float32(b.fitness).tobytes() and np.float32(a.rmse).tobytes() == np.float32(b.rmse).tobytes()


@pytest.mark.parametrize("iters", [RS_HYP_PER_BLOCK - 1, RS_HYP_PER_BLOCK, RS_HYP_PER_BLOCK + 1,
                                   8 * RS_HYP_PER_BLOCK - 1, 8 * RS_HYP_PER_BLOCK, 8 * RS_HYP_PER_BLOCK + 1,
                                   16 * RS_HYP_PER_BLOCK + 1, 24 * RS_HYP_PER_BLOCK + 1])
def test_ransac_dev_bench_call_shape(ctx, orc, synth, iters):
    """ransac_dev(corr=..., no features, confidence 2, seed 42) as bench.py calls it: untraced (above 16,384 hypotheses this is the
    bail-out, whose first batch is 8 x RS_HYP_PER_BLOCK), traced, the host call and the oracle agree."""
    n = 20000
    src, tgt, corr = _ransac_case(synth, n)
    (bs, ps), (bt, pt), (bc, pc) = _up(src), _up(tgt), _up(corr)
    a = ctx.ransac_dev(ps, n, pt, n, None, None, pc, 0.004, iters, 2.0, 42)
    b = ctx.ransac_dev(ps, n, pt, n, None, None, pc, 0.004, iters, 2.0, 42, trace=True)
    _same_ransac(a, b)
    _same_ransac(a, ctx.ransac(src, tgt, corr=corr, voxel=0.004, max_iterations=iters, confidence=2.0, seed=42))
    ref = orc.ransac(src, tgt, corr=corr, voxel=0.004, max_iterations=iters, confidence=2.0, trace=True)
    assert np.array_equal(b.trace_inliers, ref["inliers"])
    assert (a.best_iteration, a.iterations_run, a.inliers) == (ref["best_iter"], ref["iters_run"], int(ref["inliers"][ref["best_iter"]]))
    assert a.iterations_run == iters and a.inliers > 0.3 * n
    assert a.transformation.tobytes() == ref["T"].tobytes() and a.fitness == ref["fitness"]
    assert abs(float(a.rmse) - float(ref["rmse"])) <= 1e-7


def test_ransac_dev_feature_path(ctx, orc, synth):
    """d_fs / d_ft instead of a correspondence list: the device matches the descriptors itself; the host call, bit for bit."""
    ns, nt = 3000, 2500
    src, T_gt = synth.make_scene(ns, 3)
    tgt, _ = synth.sample_object(nt, 3)
    fs, ft = synth.random_features(ns, 5), synth.random_features(nt, 6)
    bufs = [_up(x) for x in (src, tgt, fs, ft)]
    (_, ps), (_, pt), (_, pfs), (_, pft) = bufs
    a = ctx.ransac_dev(ps, ns, pt, nt, pfs, pft, None, 0.004, 3000, 0.999, 42)
    h = ctx.ransac(src, tgt, fs=fs, ft=ft, voxel=0.004, max_iterations=3000, confidence=0.999, seed=42)
    _same_ransac(a, h)
    ref = orc.ransac(src, tgt, fs=fs, ft=ft, voxel=0.004, max_iterations=3000, confidence=0.999)
    assert (a.best_iteration, a.iterations_run) == (ref["best_iter"], ref["iters_run"])
    assert a.transformation.tobytes() == ref["T"].tobytes() and a.fitness == ref["fitness"]


# ---------------------------------------------------------------- features
@pytest.mark.parametrize("n,k", [(1500, 30), (257, 7), (1, 30), (0, 30)])
def test_estimate_normals_dev(ctx, orc, synth, tdv, n, k):
    pts = _cloud(synth, n)
    bx, px = _up(pts)
    d_n, d_knn = _out(n, 3), _out(n, k, torch.int32)
    try:
        h_n, h_knn = ctx.estimate_normals(pts, k, want_knn=True)
    except tdv.TdvError:
        with pytest.raises(tdv.TdvError):
            ctx.estimate_normals_dev(px, n, k, d_n.data_ptr(), d_knn.data_ptr())
        return
    ctx.estimate_normals_dev(px, n, k, d_n.data_ptr(), d_knn.data_ptr())
    g_n, g_knn = _got(d_n, n, 3), _got(d_knn, n, k, np.int32)
    assert g_n.tobytes() == h_n.tobytes() and np.array_equal(g_knn, h_knn)
    r_n, r_knn = orc.estimate_normals(pts, k, want_knn=True)
    assert g_n.tobytes() == r_n.tobytes() and np.array_equal(g_knn, r_knn)
    d_n2 = _out(n, 3)
    ctx.estimate_normals_dev(px, n, k, d_n2.data_ptr(), None)                  # without the neighbour lists
    assert _got(d_n2, n, 3).tobytes() == h_n.tobytes()


@pytest.mark.parametrize("n,radius", [(1500, 0.012), (1500, 0.05), (1, 0.01), (0, 0.01)])
def test_compute_fpfh_and_normals_fpfh_dev(ctx, orc, synth, tdv, n, radius):
    pts = _cloud(synth, n)
    nrm = orc.estimate_normals(pts, 30) if n else np.zeros((0, 3), np.float32)
    (bx, px), (bn, pn) = _up(pts), _up(nrm)
    d_d, d_nb, d_c = _out(n, 33), _out(n, 100, torch.int32), _out(n, 1, torch.int32)
    try:
        h_d, h_nb, h_c = ctx.compute_fpfh(pts, nrm, radius, want_neighbors=True)
    except tdv.TdvError:
        with pytest.raises(tdv.TdvError):
            ctx.compute_fpfh_dev(px, pn, n, radius, d_d.data_ptr(), d_nb.data_ptr(), d_c.data_ptr())
        return
    ctx.compute_fpfh_dev(px, pn, n, radius, d_d.data_ptr(), d_nb.data_ptr(), d_c.data_ptr())
    g_d, g_nb, g_c = _got(d_d, n, 33), _got(d_nb, n, 100, np.int32), _got(d_c, n, 1, np.int32)
    assert g_d.tobytes() == h_d.tobytes() and np.array_equal(g_c, h_c)
    for i in range(n):                                                      # the lists: the first cnt entries are defined
        assert np.array_equal(g_nb[i, :g_c[i]], h_nb[i, :h_c[i]])
    r_d, r_nb, r_c = orc.compute_fpfh(pts, nrm, radius, want_neighbors=True)
    assert g_d.tobytes() == r_d.tobytes() and np.array_equal(g_c, r_c)
    for i in range(n):
        assert np.array_equal(g_nb[i, :g_c[i]], r_nb[i, :r_c[i]])
    d_d2 = _out(n, 33)
    ctx.compute_fpfh_dev(px, pn, n, radius, d_d2.data_ptr())                 # without the neighbour outputs
    assert _got(d_d2, n, 33).tobytes() == h_d.tobytes()
    # one walk for both stages == estimateNormals(30) then computeFPFH(radius)
    h_n = ctx.estimate_normals(pts, 30)
    h_f = ctx.compute_fpfh(pts, h_n, radius)
    d_n3, d_f3 = _out(n, 3), _out(n, 33)
    ctx.normals_fpfh_dev(px, n, 30, radius, d_n3.data_ptr(), d_f3.data_ptr())
    assert _got(d_n3, n, 3).tobytes() == h_n.tobytes() and _got(d_f3, n, 33).tobytes() == h_f.tobytes()


@pytest.mark.parametrize("ns,nt", [(700, 500), (4500, 2500), (1, 1), (0, 3)])
def test_feature_match_dev(ctx, orc, synth, tdv, ns, nt):
    fs, ft = synth.random_features(max(ns, 1), 1)[:ns], synth.random_features(nt, 2)
    if nt > 10 and ns > 10:
        ft[7] = ft[3]; fs[0] = ft[7]                                           # duplicate descriptors: the lowest index wins
    (bfs, pfs), (bft, pft) = _up(fs), _up(ft)
    d_c = _out(ns, 1, torch.int32)
    try:
        h = ctx.feature_match(fs, ft)
    except tdv.TdvError:
        with pytest.raises(tdv.TdvError):
            ctx.feature_match_dev(pfs, ns, pft, nt, d_c.data_ptr())
        return
    ctx.feature_match_dev(pfs, ns, pft, nt, d_c.data_ptr())
    g = _got(d_c, ns, 1, np.int32)
    assert np.array_equal(g, h) and np.array_equal(g, orc.feature_match(fs, ft))


# ---------------------------------------------------------------- voxels and masks
@pytest.mark.parametrize("with_rgb", [False, True])
@pytest.mark.parametrize("order", ["first", "reference"])
@pytest.mark.parametrize("n,voxel", [(3000, 0.004), (20000, 0.002), (1, 0.004), (0, 0.004)])
def test_voxel_downsample_dev(ctx, orc, synth, tdv, n, voxel, order, with_rgb):
    pts = _cloud(synth, n)
    rgb = np.random.default_rng(3).random((n, 3)).astype(np.float32) if with_rgb else None
    o = tdv.TDV_VOXEL_ORDER_FIRST if order == "first" else tdv.TDV_VOXEL_ORDER_REFERENCE
    (bx, px), (bc, pc) = _up(pts), (_up(rgb) if with_rgb else (None, None))
    ref_xyz, ref_rgb, first = orc.voxel_downsample(pts, rgb, voxel)
    m = len(ref_xyz)
    perm = np.argsort(first, kind="stable") if order == "first" else np.arange(m)
    d_x, d_c = _out(m, 3), (_out(m, 3) if with_rgb else None)
    got = ctx.voxel_downsample_dev(px, pc, n, voxel, d_x.data_ptr(), None if d_c is None else d_c.data_ptr(), m, order=o)
    assert got == m
    assert _got(d_x, m, 3).tobytes() == ref_xyz[perm].tobytes()
    if with_rgb:
        assert _got(d_c, m, 3).tobytes() == ref_rgb[perm].tobytes()
    h_xyz, h_rgb = ctx.voxel_downsample(pts, rgb, voxel, order=o)
    assert h_xyz.tobytes() == ref_xyz[perm].tobytes()
    if m < 2:
        return
    # one voxel short: an error, the true count, and nothing written past the capacity
    d_x, d_c = _out(m - 1, 3), (_out(m - 1, 3) if with_rgb else None)         # m - 1 rows + the sentinel row
    cnt = C.c_int(-1)
    st = tdv.lib().tdv_voxel_downsample_dev(ctx._h, C.c_void_p(px), None if pc is None else C.c_void_p(pc), n, C.c_float(voxel), o,
                                            C.c_void_p(d_x.data_ptr()), None if d_c is None else C.c_void_p(d_c.data_ptr()), m - 1, C.byref(cnt))
    torch.cuda.synchronize()
    assert st != 0 and cnt.value == m
    for t in (d_x, d_c) if with_rgb else (d_x,):
        h = t.cpu().numpy().view(np.int32)
        assert len(h) == 3 * m and (h[3 * (m - 1):] == SENTINEL).all(), "write past the capacity"


@pytest.mark.parametrize("sw,sh,dw,dh", [(1280, 720, 640, 360), (640, 360, 1280, 720), (1280, 720, 853, 479), (97, 61, 211, 37), (1, 1, 5, 3)])
def test_mask_resize_nearest_dev(ctx, orc, tdv, sw, sh, dw, dh):
    B = 3
    rng = np.random.default_rng(sw + dh)
    masks = (rng.random((B, sh, sw)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (B, sh, sw)).astype(np.uint8)
    base = torch.zeros(B * sh * sw + 24, dtype=torch.uint8, device=DEV)
    view = base[12:12 + B * sh * sw]
    view.copy_(torch.from_numpy(masks.reshape(-1)).to(DEV))
    out = torch.full((B * dh * dw + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    tdv._check(ctx._h, tdv.lib().tdv_mask_resize_nearest_dev(ctx._h, C.c_void_p(view.data_ptr()), B, sw, sh, dw, dh, C.c_void_p(out.data_ptr())),
               "tdv_mask_resize_nearest_dev")
    h = out.cpu().numpy()
    assert (h[B * dh * dw:] == 0xA5).all(), "write past the end of the output"
    got = h[:B * dh * dw].reshape(B, dh, dw)
    assert np.array_equal(got, ctx.mask_resize_nearest(masks, dw, dh))
    for b in range(B):
        assert np.array_equal(got[b], orc.mask_resize_nearest(masks[b], dw, dh)), b
