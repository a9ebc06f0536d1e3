"""The default ICP accumulation (f64 tree sums) and RANSAC's rmse, bit for bit against the oracle's exact-sum mode.

The device adds f32 terms in f64 along a fixed tree (csrc/icp.hip: acc_terms, acc_slab_fold, k_icp_small; csrc/ransac.hip:
k_ransac_rmse_partial / _final).  That is within the tree's error bound of the exact sum, so every f32 the device takes from it is the
exact sum rounded once - unless the exact sum lies within that bound of an f32 rounding midpoint, which the oracle detects
(oracle.cpp: XSum, x32).  Every input here must report no such sum, so the device's T, rmse, fitness, iteration count and n_corr
must equal the exact-sum oracle's as bytes.  A dropped point, a product in the wrong precision or a stale slab fails here, where the
tolerances of tests/test_gpu_icp.py let it through.

Paths: k_icp_small (one launch, ns * nt <= 2^18), the multi-launch brute force (1 point per thread; TDV_ICP_SMALL=0 forces it), the
pruned and grid searches (4 points per thread), k_icp_accumulate_multi (icp_batch_dev, grid), icp_small_batch_dev (a non-fixed batch of
small problems) and the per-instance fallback of icp_batch_dev.  Sizes straddle the block (256 points), the 4-point block (1,024), the
one-launch limits and the fold's second round of 128 slabs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
THR = 0.004
EDGE_NS = [3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049]


# ---------------------------------------------------------------- helpers
def _up(a, dtype=np.float32):
    """a on the device: (tensor, pointer); an empty array still gets a buffer."""
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 3), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


@pytest.fixture
def modes(ctx, monkeypatch):
    ctx.set_icp_accumulation("tree")
    yield ctx, monkeypatch
    ctx.set_icp_search("auto")
    ctx.set_icp_accumulation("tree")


def _problem(synth, ns, nt, seed=42, offset=0.0, angle=2.0, trans=0.003):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(max(ns, 1), seed)
    T0 = synth.perturb(T_gt, seed=seed + 1, angle_deg=angle, trans=trans).astype(np.float32)
    if offset:
        S = np.eye(4, dtype=np.float32); S[2, 3] = offset
        T0 = (S @ T0).astype(np.float32)
        tgt = tgt + np.float32([0.0, 0.0, offset])
    return src[:ns].copy(), tgt, nrm, T0


def _oracle(orc, src, tgt, nrm, T0, thr, iters, p2plane, what):
    """The exact-sum oracle as a device result would read: (T, rmse, fitness, iterations, n_corr); no ambiguous sum allowed."""
    r = orc.icp(src, tgt, nrm if p2plane else None, T0, thr, iters, p2plane, trace=True, exact=True)
    assert not r["ambiguous"], ("%s: a sum lies within the f64 tree's error bound of an f32 rounding midpoint (iterations %s); "
                                "this input cannot hold the device bit for bit - pick another" % (what, np.nonzero(r["trace"][:, 19])[0]))
    nc = int(r["trace"][-1, 18]) if r["iterations"] else 0
    return r["T"], np.float32(r["rmse"]), np.float32(r["fitness"]), r["iterations"], nc


def _chain(orc, src, tgt, nrm, T0, thr, K, p2plane, what):
    """K fixed iterations as K one-iteration exact-sum oracle calls: an update skipped (pose kept) where n_corr < 3."""
    T, last = T0, (T0, np.float32(0), np.float32(0), 0, 0)
    for k in range(K):
        Tn, rmse, fit, it, nc = _oracle(orc, src, tgt, nrm, T, thr, 1, p2plane, "%s step %d" % (what, k + 1))
        if it:
            T, last = Tn, (Tn, rmse, fit, k + 1, nc)
    return last


def _same(got, ref, what):
    T, rmse, fit, it, nc = ref
    assert got.transformation.tobytes() == T.tobytes(), (what, got.transformation, T)
    assert np.float32(got.rmse).tobytes() == rmse.tobytes(), (what, got.rmse, rmse)
    assert np.float32(got.fitness).tobytes() == fit.tobytes(), (what, got.fitness, fit)
    assert (got.iterations, got.n_corr) == (it, nc), (what, got.iterations, it, got.n_corr, nc)


def _icp_dev(ctx, src, tgt, nrm, T0, thr, iters, p2plane, fixed):
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    return ctx.icp_dev(ps, len(src), pt, pn if p2plane else None, len(tgt), T0, thr, iters, p2plane, fixed_iterations=fixed)


PATHS = {   # search mode, TDV_ICP_SMALL, expected search
    "small": ("auto", None, "brute"),
    "brute": ("brute", "0", "brute"),
    "pruned": ("pruned", None, "pruned"),
    "grid": ("grid", None, "grid"),
}


def _set_path(ctx, mp, path):
    search, small, _ = PATHS[path]
    ctx.set_icp_search(search)
    if small is None:
        mp.delenv("TDV_ICP_SMALL", raising=False)
    else:
        mp.setenv("TDV_ICP_SMALL", small)


def _thresholds(orc, src, tgt, T0):
    """Thresholds that accept exactly 2, exactly 3, a few and most source points (midway between neighbouring distances)."""
    d = np.sort(np.sqrt(orc.icp_correspondences(src, tgt, None, T0, 1e9, False)["d2"].astype(np.float64)))
    out = {}
    for name, k in (("two", 2), ("three", 3), ("few", max(4, len(d) // 20)), ("most", max(4, 9 * len(d) // 10))):
        if k < len(d) and d[k] - d[k - 1] > 1e-6 * d[k]:
            out[name] = np.float32(0.5 * (d[k - 1] + d[k]))
    return out


# ---------------------------------------------------------------- one iteration, every accumulation path
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("path", list(PATHS))
def test_one_iteration_at_block_edges(modes, orc, synth, path, p2plane, fixed):
    ctx, mp = modes
    _set_path(ctx, mp, path)
    nt, thr = 127, 0.02                               # 2,048 x 127 < 2^18: every size up to 2,048 fits k_icp_small; a sparse target, a wide threshold
    for ns in EDGE_NS:
        src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=ns + 100)
        ref = _oracle(orc, src, tgt, nrm, T0, thr, 1, p2plane, "ns %d" % ns)
        got = _icp_dev(ctx, src, tgt, nrm, T0, thr, 1, p2plane, fixed)
        _same(got, ref, "%s ns %d" % (path, ns))
        if path != "small" or ns <= 2048:
            assert ctx.last_icp_search() == PATHS[path][2]


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("path", ["small", "brute", "grid"])
def test_one_iteration_acceptance_counts(modes, orc, synth, path, p2plane):
    """Thresholds accepting exactly 2 (no update), exactly 3, a few and most points."""
    ctx, mp = modes
    _set_path(ctx, mp, path)
    src, tgt, nrm, T0 = _problem(synth, 700, 300, seed=9, angle=4.0, trans=0.01)
    ths = _thresholds(orc, src, tgt, T0)
    assert set(ths) == {"two", "three", "few", "most"}, ths
    for name, thr in ths.items():
        ref = _oracle(orc, src, tgt, nrm, T0, thr, 1, p2plane, name)
        for fixed in (False, True):
            got = _icp_dev(ctx, src, tgt, nrm, T0, thr, 1, p2plane, fixed)
            _same(got, ref, "%s %s fixed=%s" % (path, name, fixed))
        assert ref[4] == {"two": 0, "three": 3}.get(name, ref[4])


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,nt", [(511, 512), (512, 512), (513, 512)])
def test_one_iteration_across_the_one_launch_limit(modes, orc, synth, ns, nt, p2plane):
    """ns * nt just below, at and just above 2^18: k_icp_small, then the multi-launch brute force, same bits."""
    ctx, _ = modes
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=ns + 7)
    ref = _oracle(orc, src, tgt, nrm, T0, THR, 1, p2plane, "%d x %d" % (ns, nt))
    for fixed in (False, True):
        _same(_icp_dev(ctx, src, tgt, nrm, T0, THR, 1, p2plane, fixed), ref, "%d x %d fixed=%s" % (ns, nt, fixed))


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns,path", [(32767, "brute"), (32768, "brute"), (32769, "brute"),
                                     (131071, "pruned"), (131072, "grid"), (131073, "grid"), (131073, "pruned")])
def test_one_iteration_fold_second_round(modes, orc, synth, ns, path, p2plane):
    """128 slabs and one more: the fold's second round (1 point per thread at 32,768, 4 at 131,072)."""
    ctx, mp = modes
    _set_path(ctx, mp, path)
    nt = 2000 if ns < 100000 else 1500
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=5)
    ref = _oracle(orc, src, tgt, nrm, T0, 0.006, 1, p2plane, "ns %d" % ns)
    for fixed in (False, True):
        _same(_icp_dev(ctx, src, tgt, nrm, T0, 0.006, 1, p2plane, fixed), ref, "%s ns %d fixed=%s" % (path, ns, fixed))
    assert ctx.last_icp_search() == PATHS[path][2]


# ---------------------------------------------------------------- batches
def _batch(ctx, clouds, tgt, nrm, T0s, thr, iters, p2plane, fixed):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    cat = np.concatenate(clouds) if off[-1] else np.zeros((0, 3), np.float32)
    ks, ps = _up(cat); kt, pt = _up(tgt); kn, pn = _up(nrm)
    return ctx.icp_batch_dev(ps, off, pt, pn if p2plane else None, len(tgt), T0s, thr, iters, p2plane, fixed)


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("kind", ["multi", "small_batch", "fallback_pruned", "fallback_brute_fixed"])
def test_batch_one_iteration(modes, orc, synth, kind, p2plane):
    """Mixed sizes and an empty instance in one call: k_icp_accumulate_multi (grid), icp_small_batch_dev (non-fixed, small) and the
    per-instance fallback (pruned search; brute force with fixed iterations)."""
    ctx, _ = modes
    ctx.set_icp_search({"multi": "grid", "small_batch": "auto", "fallback_pruned": "pruned", "fallback_brute_fixed": "brute"}[kind])
    if kind == "small_batch":
        sizes, nt = [3, 64, 257, 0, 1025, 2048, 255], 500
    else:
        sizes, nt = [3, 64, 257, 0, 1025, 2049, 4097, 255], 6000
    tgt, nrm = synth.sample_object(nt, 42)
    clouds, T0s = [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), 300 + b)
        clouds.append(src[:n].copy())
        T0s.append(synth.perturb(T_gt, seed=400 + b, angle_deg=2.0, trans=0.003))
    T0s = np.stack(T0s).astype(np.float32)
    for fixed in ((False,) if kind == "small_batch" else (False, True)) if kind != "fallback_brute_fixed" else (True,):
        got = _batch(ctx, clouds, tgt, nrm, T0s, THR, 1, p2plane, fixed)
        if kind == "multi":
            assert ctx.last_icp_search() == "grid"
        for b, n in enumerate(sizes):
            ref = _oracle(orc, clouds[b], tgt, nrm, T0s[b], THR, 1, p2plane, "instance %d" % b) if n else (T0s[b], np.float32(0), np.float32(0), 0, 0)
            _same(got[b], ref, "%s instance %d (%d points) fixed=%s" % (kind, b, n, fixed))


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("search", ["grid", "auto"])
def test_batch_full_loops(modes, orc, synth, search, p2plane):
    """Non-fixed loops to convergence in one batch: the grid path (k_icp_accumulate_multi) and AUTO's small-batch path."""
    ctx, _ = modes
    ctx.set_icp_search(search)
    nt = 1500
    tgt, nrm = synth.sample_object(nt, 42)
    sizes = [900, 0, 1800, 300]
    clouds, T0s = [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), 500 + b)
        clouds.append(src[:n].copy())
        T0s.append(synth.perturb(T_gt, seed=600 + b, angle_deg=3.0, trans=0.005))
    T0s = np.stack(T0s).astype(np.float32)
    got = _batch(ctx, clouds, tgt, nrm, T0s, THR, 40, p2plane, False)
    for b, n in enumerate(sizes):
        ref = _oracle(orc, clouds[b], tgt, nrm, T0s[b], THR, 40, p2plane, "instance %d" % b) if n else (T0s[b], np.float32(0), np.float32(0), 0, 0)
        _same(got[b], ref, "%s instance %d" % (search, b))


# ---------------------------------------------------------------- full loops
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("path", list(PATHS))
def test_full_loop(modes, orc, synth, path, p2plane):
    """Non-fixed runs to the stopping rule: iteration count included."""
    ctx, mp = modes
    _set_path(ctx, mp, path)
    ns, nt = (500, 500) if path == "small" else (3000, 2500)
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=21, angle=3.0, trans=0.005)
    ref = _oracle(orc, src, tgt, nrm, T0, THR, 60, p2plane, path)
    got = _icp_dev(ctx, src, tgt, nrm, T0, THR, 60, p2plane, False)
    _same(got, ref, path)
    assert ctx.last_icp_search() == PATHS[path][2]
    assert ref[3] >= 3


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("offset", [0.0, 0.8, 3.0])
def test_full_loop_away_from_the_origin(modes, orc, synth, offset, p2plane):
    """The object at the origin, at 0.8 m and at 3 m: the f64 centring sum PQ - n * mean P * mean Q must keep its f32 bits."""
    ctx, _ = modes
    for ns, nt in ((500, 500), (4000, 3000)):
        src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=33, offset=offset)
        ref = _oracle(orc, src, tgt, nrm, T0, THR, 60, p2plane, "%d x %d at %.1f m" % (ns, nt, offset))
        _same(_icp_dev(ctx, src, tgt, nrm, T0, THR, 60, p2plane, False), ref, "%d x %d at %.1f m" % (ns, nt, offset))


@pytest.mark.parametrize("K", [31, 70])
@pytest.mark.parametrize("ns,nt", [(500, 500), (5000, 5000)])
def test_fixed_point_to_point_drift_cases(modes, orc, synth, ns, nt, K):
    """DESIGN.md 2's drift cases: K fixed point-to-point iterations equal K chained one-iteration exact-sum oracle calls, bit for bit."""
    ctx, _ = modes
    src, tgt, nrm, T0 = _problem(synth, ns, nt)
    ref = _chain(orc, src, tgt, nrm, T0, THR, K, False, "%d x %d" % (ns, nt))
    got = _icp_dev(ctx, src, tgt, nrm, T0, THR, K, False, True)
    _same(got, ref, "%d x %d K %d" % (ns, nt, K))


@pytest.mark.parametrize("p2plane", [True, False])
def test_fixed_full_loop_point_to_plane_and_point(modes, orc, synth, p2plane):
    """Fixed K = 33 on the multi-launch path (a burst of 32 launches and one more)."""
    ctx, _ = modes
    src, tgt, nrm, T0 = _problem(synth, 3000, 2500, seed=23)
    ref = _chain(orc, src, tgt, nrm, T0, THR, 33, p2plane, "3000 x 2500")
    _same(_icp_dev(ctx, src, tgt, nrm, T0, THR, 33, p2plane, True), ref, "K 33")


# ---------------------------------------------------------------- RANSAC rmse
def _ransac_problem(synth, ns, seed, far=False):
    src, T_gt = synth.make_scene(ns, seed)
    tgt = (src.astype(np.float64) @ T_gt[:3, :3].T.astype(np.float64) + T_gt[:3, 3]).astype(np.float32)
    tgt += np.random.default_rng(seed).normal(0, 0.0006, tgt.shape).astype(np.float32)
    if far:                                      # unrelated targets metres apart: every hypothesis scores 0 inliers
        tgt = np.random.default_rng(seed).uniform(-10.0, 10.0, tgt.shape).astype(np.float32)
    corr = np.random.default_rng(seed + 1).permutation(ns).astype(np.int32)
    corr[: (4 * ns) // 5] = np.arange((4 * ns) // 5)   # 80% true correspondences
    return src, tgt, corr


# seeds 259 and 4098: inputs where summing the squared distance d2 instead of the reference's err * err (err = sqrtf(d2))
# changes the f32 error sum - a term formed in the wrong arithmetic fails here
@pytest.mark.parametrize("ns,seed", [(255, 255), (257, 257), (257, 259), (511, 511), (513, 513), (4095, 4095), (4097, 4097), (4097, 4098),
                                     (65535, 65535), (65537, 65537), (70001, 70001), (131073, 131073)])
def test_ransac_rmse(ctx, orc, synth, ns, seed):
    """ransac and ransac_dev: the winner's rmse equals sqrt(f32(exact error sum) / inliers); above 65,536 points
    k_ransac_rmse_final's strided loop takes more than one slab per thread."""
    iters = 200 if ns < 60000 else 60
    src, tgt, corr = _ransac_problem(synth, ns, seed)
    ref = orc.ransac(src, tgt, corr=corr, voxel=0.001, max_iterations=iters, confidence=2.0, exact=True)
    assert not ref["rmse_ambiguous"], "ns %d: the error sum lies within the f64 tree's bound of an f32 rounding midpoint" % ns
    assert ref["best_iter"] >= 0 and ref["fitness"] > 0
    host = ctx.ransac(src, tgt, corr=corr, voxel=0.001, max_iterations=iters, confidence=2.0)
    ks, ps = _up(src); kt, pt = _up(tgt); kc, pc = _up(corr, np.int32)
    dev = ctx.ransac_dev(ps, ns, pt, ns, None, None, pc, 0.001, iters, 2.0)
    for what, got in (("ransac", host), ("ransac_dev", dev)):
        assert got.transformation.tobytes() == ref["T"].tobytes(), what
        assert np.float32(got.fitness).tobytes() == ref["fitness"].tobytes(), what
        assert got.best_iteration == ref["best_iter"], what
        assert np.float32(got.rmse).tobytes() == ref["rmse"].tobytes(), (what, got.rmse, ref["rmse"])


def test_ransac_rmse_no_inliers(ctx, orc, synth):
    """No hypothesis scores an inlier: no winner, and the reported rmse is the default 0 on both sides (registration.cpp's 999.0
    belongs to a hypothesis without inliers, which can never become the best)."""
    src, tgt, corr = _ransac_problem(synth, 1000, 3, far=True)
    ref = orc.ransac(src, tgt, corr=corr, voxel=0.001, max_iterations=100, confidence=2.0, exact=True)
    assert ref["best_iter"] == -1
    ks, ps = _up(src); kt, pt = _up(tgt); kc, pc = _up(corr, np.int32)
    for got in (ctx.ransac(src, tgt, corr=corr, voxel=0.001, max_iterations=100, confidence=2.0),
                ctx.ransac_dev(ps, 1000, pt, 1000, None, None, pc, 0.001, 100, 2.0)):
        assert got.best_iteration == -1 and got.inliers == 0
        assert np.float32(got.rmse).tobytes() == ref["rmse"].tobytes() and np.float32(got.fitness) == 0.0
        assert got.transformation.tobytes() == ref["T"].tobytes()
