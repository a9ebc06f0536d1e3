"""The order of the scored points (csrc/ransac.hip, RansacPointOrder): after the first batch of a call with bail-out the packed pair
array is written again, the running best's outliers first and its inliers behind them.  Counts do not depend on that order, so every
case holds the result - best iteration, iterations run, inliers, fitness, the transform's bytes - to the oracle's traced loop AND to
the exact kernel, which leaves no test out.  The cases that set the two orders against each other get the natural order
(TDV_RANSAC_ORDER=0, read per call through getenv) from a process of their own.  Shapes: a class boundary inside a pair, a chunk
and a block of the partition (odd point counts, no multiple of 8 or 256), clouds of under one block, an empty outlier class, no
best at all, an outlier class smaller than the prefix, non-finite points, an early exit inside the bounded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, BATCH = 8192, 65536          # the first batch of a call with bail-out, and every later one (csrc/ransac.hip)
SHORT = 17000                       # FIRST + one bounded batch of 8,808
ODD_SEED = 11                       # a 9,999-point scene whose best of 17,000 iterations lies in the bounded batch
EXIT_SEED = 7                       # a scene whose bounded batch holds a new best: an exit can fire there (the default seed's best is in the first batch)


def _result(r):
    return [int(r.best_iteration), int(r.iterations_run), int(r.inliers), float(r.fitness), r.transformation.tobytes().hex()]


def _oracle(orc, src, tgt, corr, voxel, iters, confidence=2.0):
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, trace=True)
    inl = int(ref["inliers"][ref["best_iter"]]) if ref["best_iter"] >= 0 else 0
    return [int(ref["best_iter"]), int(ref["iters_run"]), inl, float(ref["fitness"]), ref["T"].tobytes().hex()], ref


def _noisy(ns):
    rng = np.random.default_rng(ns)
    src = ((rng.random((ns, 3)) - 0.5) * 0.2).astype(np.float32)
    tgt = (src + rng.normal(size=(ns, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    return src, tgt, np.arange(ns, dtype=np.int32), 0.004


def _scene(ctx, synth, n, share, seed=5):
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < share, nn, rng.integers(0, n, n)).astype(np.int32)
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _same_cloud():
    """source == target under the identity correspondences: every point is an inlier of every valid hypothesis"""
    rng = np.random.default_rng(1000)
    src = ((rng.random((1000, 3)) - 0.5) * 0.2).astype(np.float32)
    return src, src.copy(), np.arange(1000, dtype=np.int32), 0.004


def _run(ctx, src, tgt, corr, voxel, iters, confidence=2.0):
    """the fast pass (bail-out, bound and point order as the environment sets them), its scored share, and the exact kernel"""
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    scored = ctx.last_ransac_scored()
    try:
        ctx.set_ransac_score("exact")
        exact = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    finally:
        ctx.set_ransac_score("fast")
    return _result(got), scored, _result(exact)


def _check(ctx, orc, src, tgt, corr, voxel, iters, confidence=2.0, ref=None):
    got, scored, exact = _run(ctx, src, tgt, corr, voxel, iters, confidence)
    if ref is None:
        ref = _oracle(orc, src, tgt, corr, voxel, iters, confidence)[0]
    print("iters %d scored share %.6f result %s" % (iters, scored, got[:4]))
    assert got == ref, (got[:4], ref[:4])
    assert got == exact, (got[:4], exact[:4])
    return scored


# the cases that are also run in the natural order: name -> (inputs, iterations)
def _both_orders(ctx, synth):
    return {"main": (_scene(ctx, synth, 30000, 0.5), SHORT),
            "same_cloud": (_same_cloud(), SHORT),
            "no_best": (_noisy(2), FIRST + BATCH + 1)}


@pytest.fixture(scope="module")
def scenes(ctx, synth):
    return {share: _scene(ctx, synth, 30000, share) for share in (0.5, 1.0)}


@pytest.fixture(scope="module")
def main_ref(orc, scenes):
    return _oracle(orc, *scenes[0.5], SHORT)[0]


@pytest.fixture(scope="module")
def natural():
    """The cases of _both_orders under TDV_RANSAC_ORDER=0, from one child process: name -> {got, exact, scored}"""
    env = dict(os.environ, TDV_RANSAC_ORDER="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


@pytest.mark.gpu
def test_main_fewer_tests_same_result(ctx, orc, scenes, main_ref, natural):
    """Half of the correspondences true, one bounded batch: the result is the oracle's, the exact kernel's and the natural order's,
    and strictly fewer tests are scored (the CPU study: about an eighth of the survivors)"""
    on = _check(ctx, orc, *scenes[0.5], SHORT, ref=main_ref)
    off = natural["main"]
    print("scored share: order on %.6f, off %.6f" % (on, off["scored"]))
    assert off["got"] == main_ref and off["exact"] == main_ref
    assert on < off["scored"], (on, off["scored"])


@pytest.mark.gpu
def test_two_bounded_batches_on_both_buffer_sets(ctx, orc):
    """4,097 points: odd, no multiple of 8 or 256 - the class boundary falls inside a pair, a chunk and a block; the two
    bounded batches (one on each buffer set) both score the array written after the first batch"""
    _check(ctx, orc, *_noisy(4097), FIRST + BATCH + 1025)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [3, 500, 513])
def test_tiny_clouds(ctx, orc, ns):
    """partitions of under a chunk, just under and just over two blocks of the partition; the pads stay last"""
    _check(ctx, orc, *_noisy(ns), SHORT)


@pytest.mark.gpu
def test_empty_outlier_class(ctx, orc, natural):
    """every point is an inlier of the best: the partition is the identity, result and scored share equal the natural order's"""
    (src, tgt, corr, voxel), iters = _same_cloud(), SHORT
    on = _check(ctx, orc, src, tgt, corr, voxel, iters)
    off = natural["same_cloud"]
    assert off["got"] == off["exact"] == _oracle(orc, src, tgt, corr, voxel, iters)[0]
    assert on == off["scored"], (on, off["scored"])


@pytest.mark.gpu
def test_no_best(ctx, orc, natural):
    """two points: no valid hypothesis, state[0] stays 0, every point is classed an outlier - the identity; only the first batch (8 of
    the call's 8 + 64 + 1 blocks) is scored, in either order"""
    on = _check(ctx, orc, *_noisy(2), FIRST + BATCH + 1)
    off = natural["no_best"]
    assert off["got"] == off["exact"] == _oracle(orc, *_noisy(2), FIRST + BATCH + 1)[0]
    assert abs(on - 8.0 / 73.0) < 1e-9 and abs(off["scored"] - 8.0 / 73.0) < 1e-9, (on, off["scored"])


@pytest.mark.gpu
def test_every_hypothesis_good(ctx, orc, scenes):
    """every correspondence true: the outlier class is about a tenth of the cloud, the prefix reaches into the best's inliers"""
    _check(ctx, orc, *scenes[1.0], SHORT)


@pytest.mark.gpu
def test_non_finite_points(ctx, orc):
    """five NaN and five infinite source points: a comparison with NaN classes the point an outlier of the best"""
    src, tgt, corr, voxel = _noisy(4097)
    src = src.copy()
    src[[7, 600, 1023, 2048, 4096], [0, 1, 2, 0, 1]] = np.nan
    src[[8, 601, 1024, 2049, 4095], [0, 1, 2, 0, 1]] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]
    _check(ctx, orc, src, tgt, corr, voxel, SHORT)


@pytest.mark.gpu
def test_early_exit_inside_the_bounded_batch(ctx, orc, synth):
    """the confidence is the fitness of the first batch's best, and the bounded batch holds a better hypothesis: the loop stops there"""
    src, tgt, corr, voxel = _scene(ctx, synth, 30000, 0.5, seed=EXIT_SEED)
    inl = _oracle(orc, src, tgt, corr, voxel, SHORT)[1]["inliers"]
    m0 = int(inl[:FIRST].max())
    later = [j for j in range(FIRST, SHORT) if inl[j] > m0]
    assert later, "the scene's bounded batch holds no new best: no exit can fire there (m0 %d)" % m0
    confidence = float(np.float32(m0) / np.float32(len(src)))        # strict >: the first batch's best does not pass, inl[later[0]] does
    ref = _oracle(orc, src, tgt, corr, voxel, SHORT, confidence)[0]
    assert ref[0] == later[0] and ref[1] == later[0] + 1, (ref[:3], later[0])
    _check(ctx, orc, src, tgt, corr, voxel, SHORT, confidence, ref=ref)


@pytest.mark.gpu
def test_best_found_after_the_partition_on_an_odd_cloud(ctx, orc, synth):
    """9,999 points (odd, mixed classes, a class boundary inside a pair), a scene whose best hypothesis lies in the bounded batch: the
    winner's count is summed over the rewritten array, so a point the scatter misplaced, dropped or wrote twice would change the
    result against the oracle"""
    src, tgt, corr, voxel = _scene(ctx, synth, 9999, 0.5, seed=ODD_SEED)
    ref, trace = _oracle(orc, src, tgt, corr, voxel, SHORT)
    assert ref[0] >= FIRST, "the scene's best lies in the first batch (iteration %d): pick another seed" % ref[0]
    _check(ctx, orc, src, tgt, corr, voxel, SHORT, ref=ref)


@pytest.mark.gpu
def test_determinism(ctx, orc, scenes, main_ref):
    """the partition takes its positions from a scan, not from atomics: the scored share of two calls is equal to the last bit"""
    a = _check(ctx, orc, *scenes[0.5], SHORT, ref=main_ref)
    b = _check(ctx, orc, *scenes[0.5], SHORT, ref=main_ref)
    assert a == b, (a, b)


def _main():
    import importlib
    sys.path.insert(0, ROOT)
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    assert os.environ.get("TDV_RANSAC_ORDER") == "0"
    ctx = tdv.Context(0)
    out = {}
    for name, (inputs, iters) in _both_orders(ctx, synth).items():
        got, scored, exact = _run(ctx, *inputs, iters)
        out[name] = {"got": got, "exact": exact, "scored": scored}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    _main()
