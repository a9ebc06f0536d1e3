"""RansacLeafBound (csrc/ransac.hip): hypotheses whose leaf-box bound cannot beat the best count of the earlier batches are not
scored at all.  The run with the bound returns what the run without it (TDV_RANSAC_BOUND=0), the exact kernel
(set_ransac_score("exact"), which never leaves a test out) and the oracle return: best iteration, iterations run, inliers,
fitness, rmse and the transform's bits.  Cases: 50k-200k pairs at true shares 0.02 / 0.5 / 0.9, clouds at 0 m, 250 m and
100 km from the origin, matches placed on the threshold shell, infinite and NaN coordinates, tiny clouds and early exits."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _result(r):
    return (r.best_iteration, r.iterations_run, r.inliers, r.fitness, r.rmse, r.transformation.tobytes())


def _scene(ctx, synth, n, share, seed, offset=0.0):
    """The bench's kind of workload: true nearest matches for `share` of the pairs, uniform random ones for the rest."""
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < share, nn, rng.integers(0, n, n)).astype(np.int32)
    if offset:
        src = (src.astype(np.float64) + offset).astype(np.float32)
        tgt = (tgt.astype(np.float64) + offset).astype(np.float32)
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _runs(ctx, src, tgt, corr, voxel, iters, confidence):
    """(bounded result, its scored share), the result without the bound (and its share), the exact kernel's result"""
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    scored = ctx.last_ransac_scored()
    try:
        os.environ["TDV_RANSAC_BOUND"] = "0"
        plain = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
        plain_scored = ctx.last_ransac_scored()
    finally:
        os.environ.pop("TDV_RANSAC_BOUND", None)
    try:
        ctx.set_ransac_score("exact")
        exact = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    finally:
        ctx.set_ransac_score("fast")
    assert _result(got) == _result(exact), (_result(got)[:5], _result(exact)[:5])
    assert _result(plain) == _result(exact)
    return got, scored, plain_scored


def _same_as_oracle(a, ref):
    assert (a.best_iteration, a.iterations_run) == (ref["best_iter"], ref["iters_run"])
    assert a.inliers == (int(ref["inliers"][ref["best_iter"]]) if ref["best_iter"] >= 0 else 0)
    assert a.fitness == ref["fitness"] and abs(float(a.rmse) - float(ref["rmse"])) <= 1e-7
    assert a.transformation.tobytes() == ref["T"].tobytes()


@pytest.mark.parametrize("n,share,iters", [(50000, 0.5, 17000), (50000, 0.9, 20000)])
def test_leaf_bound_matches_the_oracle(ctx, orc, synth, n, share, iters):
    src, tgt, corr, voxel = _scene(ctx, synth, n, share, 42)
    got, scored, plain_scored = _runs(ctx, src, tgt, corr, voxel, iters, 2.0)
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True)
    _same_as_oracle(got, ref)
    print("n %d share %.2f: scored %.3f with the bound, %.3f without" % (n, share, scored, plain_scored))
    assert scored <= plain_scored


_SIZES = [(n, share, offset) for n in (50000, 200000) for share in (0.02, 0.5, 0.9) for offset in (0.0, 250.0, 1e5)] \
    + [(120000, share, 0.0) for share in (0.02, 0.5, 0.9)]


@pytest.mark.parametrize("n,share,offset", _SIZES)
def test_leaf_bound_equals_the_exact_kernel(ctx, synth, n, share, offset):
    src, tgt, corr, voxel = _scene(ctx, synth, n, share, 7 + n % 1000, offset)
    got, scored, plain_scored = _runs(ctx, src, tgt, corr, voxel, 70000, 2.0)
    print("n %d share %.2f offset %g: best %d @ %d, scored %.3f with the bound, %.3f without"
          % (n, share, offset, got.inliers, got.best_iteration, scored, plain_scored))
    if offset >= 1e4:
        assert scored == plain_scored          # the band is off 100 km out: so is the bound, nothing more is left out
    assert scored <= plain_scored
    if share == 0.5 and offset == 0.0:
        assert scored < 0.6 * plain_scored


def test_leaf_bound_fires_on_the_headline_workload(ctx, synth):
    """bench.py's workload (200k x 200k, half the pairs true, the bench's seeds) at 100,000 hypotheses: the share of the tests
    scored falls well below the 0.63 of the bail-out alone."""
    src, tgt, corr, voxel = _scene(ctx, synth, 200000, 0.5, 42)
    got, scored, plain_scored = _runs(ctx, src, tgt, corr, voxel, 100000, 2.0)
    print("headline: scored %.3f with the bound, %.3f without; best %d @ %d" % (scored, plain_scored, got.inliers, got.best_iteration))
    assert scored < 0.35 and plain_scored > 0.5


@pytest.mark.parametrize("seed", range(4))
def test_leaf_bound_matches_on_the_threshold_shell(ctx, orc, seed):
    """Every good pair sits at the threshold from its transformed point (to a few ulps either side), so that leaf boxes touch the
    shell for the poses near the true one; the rest is garbage.  Equal to the oracle."""
    rng = np.random.default_rng(900 + seed)
    ns = int(rng.integers(3000, 9000))
    voxel = 0.004
    thr = np.float32(voxel * 1.5)
    src = ((rng.random((ns, 3)) - 0.5) * 40 * voxel + rng.choice([0.0, 3.0, 250.0])).astype(np.float32)
    ang = rng.random() * 2.0; ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    t = rng.normal(size=3) * 0.1
    d = rng.normal(size=(ns, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = float(thr) * (1.0 + rng.choice([-2e-7, -6e-8, 0.0, 6e-8, 2e-7], ns))
    tgt = src.astype(np.float64) @ R.T + t + d * scale[:, None]
    bad = rng.random(ns) >= float(rng.choice([0.5, 0.9]))
    tgt[bad] = (rng.random((int(bad.sum()), 3)) - 0.5) * 2.0 + 5.0
    tgt = tgt.astype(np.float32)
    # one exact triple past the first batch gives a pose whose matches lie right on the shell
    iters = 40000
    tri = orc.sample_triples(ns, iters).astype(np.int64)
    ok = np.nonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2]))[0]
    k = int(rng.choice(ok[(ok > 9000) & (ok < iters - 10)]))
    tgt[tri[k]] = (src[tri[k]].astype(np.float64) @ R.T + t).astype(np.float32)
    corr = np.arange(ns, dtype=np.int32)
    got, scored, plain_scored = _runs(ctx, src, tgt, corr, voxel, iters, 2.0)
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True)
    _same_as_oracle(got, ref)
    print("shell seed %d ns %d: best %d @ %d (planted %d), scored %.3f / %.3f" % (seed, ns, got.inliers, got.best_iteration, k, scored, plain_scored))


@pytest.mark.parametrize("kind", ["nan_target", "inf_source", "ninf_source"])
def test_leaf_bound_non_finite_coordinates(ctx, orc, synth, kind):
    """A NaN anywhere or an infinite source coordinate turns the band, and with it the bound, off.  Equal to the oracle.
    (Infinite target and NaN source coordinates: tests/test_gpu_nonfinite.py.)"""
    src, tgt, corr, voxel = _scene(ctx, synth, 20000, 0.5, 11)
    rng = np.random.default_rng(5)
    rows = rng.choice(len(src), 40, replace=False)
    val = {"nan_target": np.nan, "inf_source": np.inf, "ninf_source": -np.inf}[kind]
    if kind.endswith("target"):
        tgt = tgt.copy(); tgt[corr[rows], rng.integers(0, 3, 40)] = val
    else:
        src = src.copy(); src[rows, rng.integers(0, 3, 40)] = val
    got, scored, plain_scored = _runs(ctx, src, tgt, corr, voxel, 20000, 2.0)
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=20000, confidence=2.0, trace=True)
    _same_as_oracle(got, ref)
    print("%s: best %d @ %d, scored %.3f / %.3f" % (kind, got.inliers, got.best_iteration, scored, plain_scored))


@pytest.mark.parametrize("ns,share,iters,confidence", [
    (40, 1.0, 80000, 2.0), (40, 0.5, 20000, 0.5), (257, 1.0, 70000, 0.9), (257, 0.5, 40000, 2.0),
    (50000, 0.5, 70000, 0.3), (50000, 0.5, 140000, 0.47), (50000, 0.9, 70000, 0.8), (120000, 0.5, 70000, 0.45),
])
def test_leaf_bound_tiny_clouds_and_early_exits(ctx, synth, ns, share, iters, confidence):
    if ns < 1000:
        rng = np.random.default_rng(ns)
        src = (rng.random((ns, 3)) - 0.5).astype(np.float32) * np.float32(0.2)
        tgt = src.copy()
        corr = np.where(rng.random(ns) < share, np.arange(ns), rng.integers(0, ns, ns)).astype(np.int32)
        voxel = 0.01
    else:
        src, tgt, corr, voxel = _scene(ctx, synth, ns, share, 3)
    got, scored, plain_scored = _runs(ctx, src, tgt, corr, voxel, iters, confidence)
    print("ns %d confidence %g: best %d @ %d, run %d, scored %.3f / %.3f"
          % (ns, confidence, got.inliers, got.best_iteration, got.iterations_run, scored, plain_scored))
