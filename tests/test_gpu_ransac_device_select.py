"""RANSAC's selection on the device (csrc/ransac.hip: RansacFinish, k_ransac_finish) against the oracle's loop
(registration.cpp:281-290): the batch's winner, the iteration the early exit fires at, the inlier count, the fitness and the
transform come from one record per batch instead of a host walk over every count.  Each case runs with the bail-out on (the
default: bounded batches end on their live list), with the leaf bound off (TDV_RANSAC_BOUND=0: every batch is walked whole) and
traced (the host loop, whose per-iteration counts must be the oracle's); the last test runs the file again in a process of its
own with TDV_RANSAC_BAILOUT=0, which is read once per process.

Batches: with the bail-out (calls of more than 16,384 iterations) the first batch is 8,192 iterations, the others 65,536 - batch
boundaries at 8,192 and 73,728.  The planted-jump construction of tests/test_gpu_ransac.py puts the best hypothesis, and with it
the early exit, at a chosen iteration: every true pair is off by 0.9 thresholds except the three drawn at that iteration."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL = 0.004
FIRST, BATCH = 8192, 65536


def _valid(tri):
    return (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])


def _planted(orc, ns, iters, planted, seed):
    """Source, target and identity correspondences whose only exact pairs are those drawn at the iterations in `planted`."""
    rng = np.random.default_rng(seed)
    tri = orc.sample_triples(ns, iters).astype(np.int64)
    assert _valid(tri)[planted].all(), "a planted iteration draws a repeated index: choose another cloud size"
    src = (rng.random((ns, 3)).astype(np.float32) - 0.5) * np.float32(40 * VOXEL)
    ang = rng.random() * 2.0; ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    t = rng.normal(size=3) * 0.1
    d = rng.normal(size=(ns, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tgt = src.astype(np.float64) @ R.T + t + d * (0.9 * 1.5 * VOXEL)
    bad = rng.random(ns) >= 0.5
    tgt[bad] = (rng.random((int(bad.sum()), 3)) - 0.5) * 2.0 + 5.0
    tgt = tgt.astype(np.float32)
    for k in planted:
        tgt[tri[k]] = (src[tri[k]].astype(np.float64) @ R.T + t).astype(np.float32)
    return src, tgt, np.arange(ns, dtype=np.int32)


def _same_result(a, ref, what):
    want_inl = int(ref["inliers"][ref["best_iter"]]) if ref["best_iter"] >= 0 else 0
    print("%s: best %d @ %d, run %d (oracle: %d @ %d, run %d)" % (what, a.inliers, a.best_iteration, a.iterations_run, want_inl, ref["best_iter"], ref["iters_run"]))
    assert (a.best_iteration, a.iterations_run, a.inliers) == (ref["best_iter"], ref["iters_run"], want_inl), what
    assert a.fitness == ref["fitness"] and abs(float(a.rmse) - float(ref["rmse"])) <= 1e-7, what
    assert a.transformation.tobytes() == ref["T"].tobytes(), what


def _all_modes(ctx, ref, src, tgt, corr, iters, confidence, voxel=VOXEL):
    """The call with the bail-out (and the bound), with the bound off, and traced: each the oracle's result; the trace the oracle's."""
    kw = dict(corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    _same_result(ctx.ransac(src, tgt, **kw), ref, "default")
    try:
        os.environ["TDV_RANSAC_BOUND"] = "0"
        _same_result(ctx.ransac(src, tgt, **kw), ref, "bound off")
    finally:
        os.environ.pop("TDV_RANSAC_BOUND", None)
    traced = ctx.ransac(src, tgt, trace=True, **kw)
    _same_result(traced, ref, "traced")
    n = ref["iters_run"]
    assert np.array_equal(traced.trace_inliers[:n], ref["inliers"][:n])


# (cloud size, iterations, planted iteration): the sizes are such that the planted iteration draws three distinct indices
EXIT_CASES = [
    ("last of the first batch", 2000, 20000, FIRST - 1),
    ("first of the second batch", 2000, 20000, FIRST),
    ("last of a 65,536 batch", 1800, 80000, FIRST + BATCH - 1),
    ("first after a 65,536 batch", 1800, 80000, FIRST + BATCH),
    ("inside a batch", 2200, 80000, 30011),
]


@pytest.mark.parametrize("name,ns,iters,k_star", EXIT_CASES, ids=[c[0].replace(" ", "_").replace(",", "") for c in EXIT_CASES])
def test_early_exit_fires_where_the_oracle_stops(ctx, orc, name, ns, iters, k_star):
    src, tgt, corr = _planted(orc, ns, iters, [k_star], seed=900 + k_star % 97)
    full = orc.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=iters, confidence=2.0, trace=True)
    top = int(full["inliers"][k_star]); before = int(full["inliers"][:k_star].max())
    assert top == int(full["inliers"].max()) and top > before > 0, (top, before)
    # between the two levels: the exit fires at the planted iteration; never: the whole call runs
    between = float(np.float32((before + top) / 2 / ns))
    ref = orc.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=iters, confidence=between, trace=True)
    assert ref["iters_run"] == k_star + 1 and ref["best_iter"] == k_star, name
    _all_modes(ctx, ref, src, tgt, corr, iters, between)
    assert full["iters_run"] == iters and full["best_iter"] == k_star
    _all_modes(ctx, full, src, tgt, corr, iters, 2.0)


@pytest.mark.parametrize("k1,k2", [(20011, 40009), (20011, FIRST + BATCH + 777)], ids=["one_batch", "two_batches"])
def test_a_tie_in_count_goes_to_the_earlier_iteration(ctx, orc, k1, k2):
    ns, iters = 2100, 80000
    src, tgt, corr = _planted(orc, ns, iters, [k1, k2], seed=321)
    full = orc.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=iters, confidence=2.0, trace=True)
    assert full["inliers"][k1] == full["inliers"][k2] == full["inliers"].max(), "the two planted iterations must tie"
    assert full["best_iter"] == k1
    _all_modes(ctx, full, src, tgt, corr, iters, 2.0)


@pytest.mark.parametrize("ns,iters", [(40, 80000), (5, 20000), (3, 20000)])
def test_small_clouds_with_many_skipped_iterations(ctx, orc, synth, ns, iters):
    """Most triples of a tiny cloud repeat an index and are skipped; counts tie all the time, the first best has to stay."""
    nt = 30
    tgt, _ = synth.sample_object(nt, 5)
    src, T_gt = synth.make_scene(ns, 5, outlier_frac=0.0)
    p = src.astype(np.float64) @ T_gt[:3, :3].astype(np.float64).T + T_gt[:3, 3]
    corr = ((p[:, None, :] - tgt[None].astype(np.float64)) ** 2).sum(-1).argmin(1).astype(np.int32)
    for confidence in (2.0, 0.7):
        ref = orc.ransac(src, tgt, corr=corr, voxel=0.01, max_iterations=iters, confidence=confidence, trace=True)
        assert (ref["inliers"][:ref["iters_run"]] == -1).sum() > ref["iters_run"] // 20
        if ns == 5 and confidence == 2.0:      # the best so far is followed at once by a run of skipped iterations
            b = ref["best_iter"]
            assert b >= 0 and (ref["inliers"][b + 1:b + 3] == -1).all(), ref["inliers"][b:b + 4]
        _all_modes(ctx, ref, src, tgt, corr, iters, confidence, voxel=0.01)


def test_every_hypothesis_scores_zero(ctx, orc):
    """No pair is ever within the threshold, not even a hypothesis' own three: best_iteration -1 and the identity, as the oracle."""
    ns, iters = 700, 20000
    rng = np.random.default_rng(11)
    src = rng.random((ns, 3)).astype(np.float32)
    tgt = (rng.random((ns, 3)) * 3.0 + 2.0).astype(np.float32)
    corr = np.arange(ns, dtype=np.int32)
    ref = orc.ransac(src, tgt, corr=corr, voxel=0.0, max_iterations=iters, confidence=0.999, trace=True)
    assert ref["best_iter"] == -1 and ref["iters_run"] == iters and ref["inliers"].max() == 0
    _all_modes(ctx, ref, src, tgt, corr, iters, 0.999, voxel=0.0)
    got = ctx.ransac(src, tgt, corr=corr, voxel=0.0, max_iterations=iters, confidence=0.999)
    assert got.best_iteration == -1 and got.inliers == 0 and got.fitness == 0.0
    assert np.array_equal(got.transformation, np.eye(4, dtype=np.float32))


def test_a_bad_correspondence_index_is_an_error_and_the_context_lives_on(ctx, tdv, orc):
    ns, iters = 2000, 20000
    src, tgt, corr = _planted(orc, ns, iters, [9001], seed=77)
    for bad in (ns, -1, 1 << 30):
        c = corr.copy(); c[1234] = bad
        for env, trace in ((None, False), ("0", False), (None, True)):
            try:
                if env is not None: os.environ["TDV_RANSAC_BOUND"] = env
                with pytest.raises(tdv.TdvError, match="bad argument"):
                    ctx.ransac(src, tgt, corr=c, voxel=VOXEL, max_iterations=iters, trace=trace)
            finally:
                os.environ.pop("TDV_RANSAC_BOUND", None)
    ref = orc.ransac(src, tgt, corr=corr, voxel=VOXEL, max_iterations=iters, confidence=2.0, trace=True)
    _all_modes(ctx, ref, src, tgt, corr, iters, 2.0)          # the ctx is still usable, and right


def test_all_of_the_above_without_bailout():
    """TDV_RANSAC_BAILOUT is read once per process (csrc/ransac.hip): the cases above run again in a process of their own with
    the bail-out off - every batch is then scored in one dispatch and ended by RansacFinish over all its counts."""
    if os.environ.get("TDV_RANSAC_BAILOUT") == "0":
        return                                  # this IS that process
    env = dict(os.environ, TDV_RANSAC_BAILOUT="0")
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q",
                        "-k", "not without_bailout", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    print(tail)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert " passed" in tail and "skipped" not in tail and "deselected" in tail, tail
