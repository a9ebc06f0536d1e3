"""The batch schedule of a RANSAC call with bail-out (csrc/ransac_cut.hpp: ransac_batch_size; csrc/ransac.hip: RansacRun): 8,192
hypotheses, then batches of 65,536, and from iteration G = 270,336 on grown batches of GROWN.  A grown batch has its own stride-wide
buffers, grids sized by its own count, lists that may pass the register form of the one-workgroup kernels, and - when the call stops
inside it - up to two more grown batches enqueued behind the stop.  None of that may show in a result: every case holds best
iteration, iterations run, inliers, fitness and the transform's bytes to the oracle's traced loop and to the exact kernel, which
runs no grown batch, and the bound's counter of bounded hypotheses to iterations - 8,192.
Clouds of 500 and 2,500 pairs - the oracle's loop takes 9 s per 10^9 tests, so the smallest the cases allow, and one trace shared
by the five iteration counts: the builders of tests/test_gpu_ransac_bound_lists.py, restated.  Not covered here: int4 triples (a
cloud past 2^21 points: the oracle's loop over it at these iteration counts takes hours)."""
import numpy as np
import pytest

FIRST, BATCH = 8192, 65536
G = FIRST + 4 * BATCH               # 270,336: the first iteration of the first grown batch
VOXEL = 0.004
THR = 1.5 * VOXEL
EXIT_SEED = 10                      # _noisy(2500, seed): a scene whose best of G + 131,072 iterations is iteration 350,648 (the test asserts >= G)


def _result(r):
    return [int(r.best_iteration), int(r.iterations_run), int(r.inliers), float(r.fitness), r.transformation.tobytes().hex()]


def _oracle(orc, src, tgt, corr, voxel, iters, confidence=2.0):
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, trace=True)
    inl = int(ref["inliers"][ref["best_iter"]]) if ref["best_iter"] >= 0 else 0
    return [int(ref["best_iter"]), int(ref["iters_run"]), inl, float(ref["fitness"]), ref["T"].tobytes().hex()]


def _scene(ctx, synth, n, share, seed=5):
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < share, nn, rng.integers(0, n, n)).astype(np.int32)
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _noisy(ns, seed=None):
    """every pair true, a voxel of noise"""
    rng = np.random.default_rng(ns if seed is None else seed)
    src = ((rng.random((ns, 3)) - 0.5) * 0.2).astype(np.float32)
    tgt = (src + rng.normal(size=(ns, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    return src, tgt, np.arange(ns, dtype=np.int32), 0.004


def _classes(n_far, n_mid, n_in, seed=3):
    """under the identity I matches itself, M lies three thresholds from its match, F twenty to sixty"""
    rng = np.random.default_rng(seed)
    n = n_far + n_mid + n_in
    src = ((rng.random((n, 3)) - 0.5) * 0.2).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([rng.uniform(20.0, 60.0, n_far), np.full(n_mid, 3.0), np.zeros(n_in)]) * THR
    p = rng.permutation(n)
    tgt = (src.astype(np.float64) + d * r[:, None]).astype(np.float32)
    return src[p], tgt[p], np.arange(n, dtype=np.int32), VOXEL


def _all_close():
    """500 true pairs in a cube of 5 voxels, 0.6 voxel of noise: every bounded hypothesis lies within the rule's radius of the best and
    goes live unwalked - a grown batch's live list is the whole batch, far past the register form"""
    rng = np.random.default_rng(500)
    src = ((rng.random((500, 3)) - 0.5) * 5 * VOXEL).astype(np.float32)
    tgt = (src + rng.normal(size=(500, 3)).astype(np.float32) * np.float32(0.6 * VOXEL)).astype(np.float32)
    return src, tgt, np.arange(500, dtype=np.int32), VOXEL


@pytest.fixture(scope="module")
def grown(tdv):
    n = int(tdv.lib().tdv_ransac_batch_size(G))
    assert n in (131072, 262144) and int(tdv.lib().tdv_ransac_batch_size(G - 1)) == BATCH
    return n


def _run(ctx, inputs, iters, confidence=2.0):
    src, tgt, corr, voxel = inputs
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    scored, bound = ctx.last_ransac_scored(), list(ctx.last_ransac_bound())
    try:
        ctx.set_ransac_score("exact")
        ex = _result(ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence))
    finally:
        ctx.set_ransac_score("fast")
    return {"got": _result(got), "scored": scored, "bound": bound, "exact": ex}


def _check(ctx, orc, inputs, iters, confidence=2.0, ref=None, counted=None):
    """the call against the oracle and the exact kernel.  counted: the iterations of the batches the loop reached - all of them
    unless the call stops early, when the batches enqueued behind the stop add nothing to the counters"""
    run = _run(ctx, inputs, iters, confidence)
    if ref is None:
        ref = _oracle(orc, *inputs, iters, confidence)
    print("iters %d confidence %r scored share %.6f bounded, close, fine, live %s result %s" % (iters, confidence, run["scored"], run["bound"], run["got"][:4]))
    assert run["got"] == ref, (run["got"][:4], ref[:4])
    assert run["got"] == run["exact"], (run["got"][:4], run["exact"][:4])
    bounded, close, fine, live = run["bound"]
    assert bounded == (iters if counted is None else counted) - FIRST, (run["bound"], iters, counted)   # every batch behind the first is bounded
    assert 0 <= close <= live <= bounded and 0 <= fine <= bounded - close, run["bound"]
    return run


@pytest.fixture(scope="module")
def shared(ctx, orc, synth, grown):
    """One 2,500-pair scene and ONE run of the oracle's traced loop over the longest call, G + 2 GROWN + 1,025 iterations.  The loop's
    state at iteration m is a function of the trace up to m, so a call of m iterations has the long run's record - its best, and
    with the same best its transform - whenever the long run's best lies in front of m; where it does not, the oracle runs again."""
    inputs = _scene(ctx, synth, 2500, 0.5)
    longest = G + 2 * grown + 1025
    ref = orc.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=longest, confidence=2.0, trace=True)
    assert ref["iters_run"] == longest and len(ref["inliers"]) >= longest

    def record(iters):
        if ref["best_iter"] < 0 or ref["best_iter"] >= iters:
            return _oracle(orc, *inputs, iters)
        b = int(ref["best_iter"])
        assert b == int(np.argmax(ref["inliers"][:iters]))        # the first largest count of the prefix
        return [b, iters, int(ref["inliers"][b]), float(ref["fitness"]), ref["T"].tobytes().hex()]
    return inputs, record


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["G", "G+1", "G+GROWN", "G+GROWN+1", "G+2GROWN+1025"])
def test_the_iteration_counts_around_a_grown_batch(ctx, orc, shared, grown, shape):
    """G: no grown batch.  G + 1: a grown batch of one hypothesis.  G + GROWN (+ 1): a whole one (and one more hypothesis).
    G + 2 GROWN + 1,025: grown batches in both buffer sets, the third with one hypothesis in its second scoring block."""
    iters = {"G": G, "G+1": G + 1, "G+GROWN": G + grown, "G+GROWN+1": G + grown + 1, "G+2GROWN+1025": G + 2 * grown + 1025}[shape]
    inputs, record = shared
    _check(ctx, orc, inputs, iters, ref=record(iters))


@pytest.mark.gpu
def test_a_grown_batch_of_one_hypothesis_over_three_classes(ctx, orc, grown):
    _check(ctx, orc, _classes(626, 313, 1561), G + 1)


@pytest.mark.gpu
def test_a_second_call_gives_the_same_lists(ctx, orc, shared, grown):
    """the lists' lengths do not depend on the order the workgroups append in: the same counters and scored share"""
    inputs, record = shared
    ref = record(G + grown + 1)
    first = _check(ctx, orc, inputs, G + grown + 1, ref=ref)
    again = _check(ctx, orc, inputs, G + grown + 1, ref=ref)
    assert again["bound"] == first["bound"], (again["bound"], first["bound"])
    assert again["scored"] == first["scored"], (again["scored"], first["scored"])


@pytest.mark.gpu
def test_a_live_list_past_the_register_form(ctx, orc, grown):
    """every valid hypothesis of the grown batch is live by the rule, unwalked: the one-workgroup kernels walk a list of some hundred
    thousand entries by their loops (at least nine tenths of the bounded hypotheses are live, so the grown batch's list holds at
    least 0.9 x (3 x 65,536 + 808 + GROWN + 1) - 3 x 65,536 - 808 > 16,384 entries)"""
    run = _check(ctx, orc, _all_close(), G + grown + 1)
    bounded, close, fine, live = run["bound"]
    assert fine == 0 and close == live and live * 10 >= bounded * 9, run["bound"]


@pytest.mark.gpu
@pytest.mark.parametrize("last", [8000, 12000, 17000])
def test_a_grown_batch_whose_list_ends_in_each_round_of_the_register_form(ctx, orc, grown, last):
    """the same cloud, the grown batch cut short by the call's end: its list - every valid hypothesis, a triple in 170 repeats an
    index - ends inside the first round of 8,192 entries, inside the second, and past both (17,000 x 169 / 170 > 16,384)"""
    run = _check(ctx, orc, _all_close(), G + last)
    bounded, close, fine, live = run["bound"]
    assert fine == 0 and close == live and live * 100 >= bounded * 99, run["bound"]


@pytest.mark.gpu
def test_the_bound_off(ctx, orc, shared, grown):
    """the scene 100 km out: the rounding band is wider than the threshold, so the band is off and the bound with it - nothing is
    close, nothing walked"""
    src, tgt, corr, voxel = shared[0]
    far = (src + np.float32(1e5)).astype(np.float32), (tgt + np.float32(1e5)).astype(np.float32), corr, voxel
    run = _check(ctx, orc, far, G + grown + 1)
    assert run["bound"][1] == 0 and run["bound"][2] == 0, run["bound"]


@pytest.mark.gpu
def test_an_early_exit_inside_a_grown_batch(ctx, orc, grown):
    """a scene whose best of G + GROWN iterations lies in the grown batch (the oracle says so).  With the confidence just under that
    fitness a call of G + 3 GROWN + 1 iterations stops there, inside its first grown batch, with two more enqueued behind it that
    still run: they change nothing."""
    inputs = _noisy(2500, seed=EXIT_SEED)
    trace = orc.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=G + grown, confidence=2.0, trace=True)
    b, inl = int(trace["best_iter"]), trace["inliers"][:G + grown]
    full = [b, G + grown, int(inl[b]), float(trace["fitness"]), trace["T"].tobytes().hex()]
    assert b >= G, "the scene's best lies in front of the grown batch (iteration %d): pick another seed" % b
    _check(ctx, orc, inputs, G + grown, ref=full)
    # The loop stops at the first iteration whose fitness, float(count) / float(ns), passes the confidence (registration.cpp:290).
    # Just under the best's fitness that is the best's own iteration, by the oracle's trace: the stopping call's record is the
    # whole call's with iterations run = b + 1, and no second loop of the oracle is needed for it.
    confidence = (full[2] - 0.5) / 2500.0
    passes = np.nonzero(inl.astype(np.float32) / np.float32(2500) > np.float32(confidence))[0]
    assert len(passes) and int(passes[0]) == b, (passes[:3], b)
    ref = [b, b + 1, full[2], full[3], full[4]]
    # the counters hold the batches up to the one the stop lies in, the first grown batch: G + GROWN iterations
    _check(ctx, orc, inputs, G + 3 * grown + 1, confidence=confidence, ref=ref, counted=G + grown)


@pytest.mark.gpu
def test_the_driver_runs_the_exported_schedule(ctx, tdv, shared, grown):
    """the score timer counts the scoring dispatches a call enqueued, two per batch with bail-out: a call of G + 2 GROWN + 1,025
    iterations runs the batches the exported function gives - 1 + 4 + 3 - and not the 1 + 4 + 5 of batches that do not grow"""
    src, tgt, corr, voxel = shared[0]
    iters = G + 2 * grown + 1025
    n_batches, it0 = 0, 0
    while it0 < iters:
        it0 += min(int(tdv.lib().tdv_ransac_batch_size(it0)), iters - it0); n_batches += 1
    assert n_batches == 8
    ctx.timing_enable(True)
    try:
        ctx.timing_read(tdv.TIMER_RANSAC_SCORE)
        ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
        _, launches = ctx.timing_read(tdv.TIMER_RANSAC_SCORE)
    finally:
        ctx.timing_enable(False)
    assert launches == 2 * n_batches, (launches, n_batches)
