"""How a RANSAC batch's index triples reach the device, as a per-context mode (Context.set_ransac_triples: auto, direct, staged -
csrc/ransac.hip: RansacStage).  DIRECT: the batch's hypothesis kernel reads them from the host's pinned memory.  STAGED: the host
draws a batch further ahead into three pinned slots in rotation, and the coarse level of the leaf-box bound of batch n carries batch
n + 1's triples into its device buffer while it walks; every batch behind the second of a call with bail-out and bound then runs
from the device copy.  None of that may show in a result: every case holds transformation, fitness, rmse, inliers, best iteration,
iterations run, the four counters of Context.last_ransac_bound() and the scored share of a STAGED and an AUTO call to the DIRECT call
on the same context, and - seed 42, the oracle's only one - to the oracle's traced loop.  Context.last_ransac_staged() says how many
of the batches the loop reached ran from staged triples.
The batch schedule is 8,192, then 65,536 each, then 131,072 from iteration 270,336 (csrc/ransac_cut.hpp).  Clouds of 300, 9,999 and
30,001 pairs at a true share of 0.5.  The oracle's loop takes about 9 s per 10^9 tests: it runs over every iteration count on the
300-pair cloud (one trace of the longest call, shared) and over the two short counts on the larger ones.  On 300 pairs one triple in
a hundred repeats an index and is invalid: validity has to survive the staging.  (The coarse level's waves per 64 hypotheses stay 16
for every batch: the issue's other half measured slower and was not built - profiles/r30/ransac_batch_front.md.)"""
import numpy as np
import pytest

FIRST, BATCH = 8192, 65536
G = FIRST + 4 * BATCH               # 270,336: the first iteration of the first grown batch
GROWN = 131072
ITERS = {"a staged last batch of one": FIRST + 2 * BATCH + 1,
         "a batch of 65,536 stages one of 131,072": G + GROWN + 5,
         "two grown batches less one": G + 2 * GROWN - 1,
         "16,384: nothing bounded": 16384,
         "16,385": 16385}
SHORT = ("16,384: nothing bounded", "16,385")
SIZES = (300, 9999, 30001)
EXIT_NS, EXIT_SEED = 1000, 1        # _noisy(1000, 1): the running best is beaten inside the third batch (the test asserts it)


def _result(r):
    return [int(r.best_iteration), int(r.iterations_run), int(r.inliers), float(r.fitness), float(r.rmse), r.transformation.tobytes().hex()]


def _scene(ctx, synth, n, share, seed=5):
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < share, nn, rng.integers(0, n, n)).astype(np.int32)
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _noisy(ns, seed):
    """every pair true, a voxel of noise"""
    rng = np.random.default_rng(seed)
    src = ((rng.random((ns, 3)) - 0.5) * 0.2).astype(np.float32)
    tgt = (src + rng.normal(size=(ns, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    return src, tgt, np.arange(ns, dtype=np.int32), 0.004


def _batches(tdv, iters, reached=None):
    """the sizes of the call's batches (the exported schedule); reached: only those that start in front of that iteration"""
    out, it0 = [], 0
    while it0 < iters and (reached is None or it0 < reached):
        cnt = min(int(tdv.lib().tdv_ransac_batch_size(it0)), iters - it0)
        out.append(cnt); it0 += cnt
    return out


def _staged_batches(tdv, iters, reached=None):
    """a call of more than 16,384 iterations runs with bail-out and bound: every batch behind its second is staged"""
    return max(0, len(_batches(tdv, iters, reached)) - 2) if iters > 16384 else 0


def _run(ctx, inputs, iters, mode, seed=42, confidence=2.0, trace=False):
    src, tgt, corr, voxel = inputs
    ctx.set_ransac_triples(mode)
    try:
        got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, seed=seed, trace=trace)
    finally:
        ctx.set_ransac_triples("auto")
    return {"got": _result(got), "bound": list(ctx.last_ransac_bound()), "scored": ctx.last_ransac_scored(), "staged": ctx.last_ransac_staged(),
            "trace": got.trace_inliers}


def _same(a, b):
    return a["got"] == b["got"] and a["bound"] == b["bound"] and a["scored"] == b["scored"]


def _modes(tdv, ctx, inputs, iters, seed=42, confidence=2.0, reached=None):
    """DIRECT, STAGED and AUTO on the same context: equal results, lists and scored share; the staged batches counted"""
    direct = _run(ctx, inputs, iters, "direct", seed, confidence)
    staged = _run(ctx, inputs, iters, "staged", seed, confidence)
    auto = _run(ctx, inputs, iters, "auto", seed, confidence)
    want = _staged_batches(tdv, iters, reached)
    print("iters %d seed %d: %s bounded, close, fine, live %s scored %.6f staged batches %d / %d / %d (want 0 / %d / %d)" %
          (iters, seed, direct["got"][:4], direct["bound"], direct["scored"], direct["staged"], staged["staged"], auto["staged"], want, want))
    assert _same(staged, direct), (staged["got"][:5], direct["got"][:5], staged["bound"], direct["bound"], staged["scored"], direct["scored"])
    assert _same(auto, direct), (auto["got"][:5], direct["got"][:5], auto["bound"], direct["bound"])
    assert direct["staged"] == 0 and staged["staged"] == want and auto["staged"] == want, (direct["staged"], staged["staged"], auto["staged"], want)
    return direct


@pytest.fixture(scope="module")
def own(tdv):
    """a context of this module's own: the mode it sets is no other test's business"""
    c = tdv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(own, synth):
    return {n: _scene(own, synth, n, 0.5) for n in SIZES}


@pytest.fixture(scope="module")
def records(orc, scenes):
    """per cloud: ONE run of the oracle's traced loop over the longest call it is asked about - every count on 300 pairs, the two
    short ones above.  The loop's state at iteration m is a function of the trace up to m, so a call of m iterations has the long
    run's record whenever the long run's best lies in front of m; where it does not, the oracle runs again."""
    out = {}
    for n, inputs in scenes.items():
        longest = max(ITERS.values()) if n == 300 else max(ITERS[k] for k in SHORT)
        ref = orc.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=longest, confidence=2.0, trace=True)
        assert ref["iters_run"] == longest

        def record(iters, ref=ref, inputs=inputs, longest=longest):
            assert iters <= longest
            if ref["best_iter"] < 0 or ref["best_iter"] >= iters:
                r = orc.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=iters, confidence=2.0, trace=True)
                inl = int(r["inliers"][r["best_iter"]]) if r["best_iter"] >= 0 else 0
                return [int(r["best_iter"]), int(r["iters_run"]), inl, float(r["fitness"]), r["T"].tobytes().hex()]
            b = int(ref["best_iter"])
            assert b == int(np.argmax(ref["inliers"][:iters]))        # the first largest count of the prefix
            return [b, iters, int(ref["inliers"][b]), float(ref["fitness"]), ref["T"].tobytes().hex()]
        out[n] = record
    return out


def _against_oracle(run, ref):
    got = run["got"]
    assert got[:4] + got[5:] == ref, (got[:4], ref[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", list(ITERS))
def test_staged_is_direct(tdv, own, scenes, records, n, shape):
    """the five iteration counts on the three clouds, seeds 42 and 7: a staged last batch of one hypothesis; a batch of 65,536 whose
    coarse level carries 131,072 triples - its threads are eight times as many, the grid-stride loop's first trip takes them all;
    grown batches in both buffers and all three slots; a call without bail-out, which has no bound and stages nothing; and the
    shortest call with one: 8,192 and a bounded batch of 8,193, whose only staged-to-be successor does not exist."""
    iters = ITERS[shape]
    for seed in (42, 7):
        direct = _modes(tdv, own, scenes[n], iters, seed)
        assert direct["got"][1] == iters
        assert direct["bound"][0] == (iters - FIRST if iters > 16384 else 0), direct["bound"]
        if seed == 42 and (n == 300 or shape in SHORT):
            _against_oracle(direct, records[n](iters))


def test_invalid_triples_lie_in_the_staged_batches(tdv):
    """what the 300-pair cases rest on (host only): the index stream of seed 42 over 300 pairs has triples that repeat an index -
    invalid, the word's top bit clear - in the first staged batch (the call's third) as in every other"""
    out, packed = tdv.sample_triples_batch(300, FIRST + 2 * BATCH, seed=42)
    assert packed
    invalid = (out[FIRST + BATCH:] >> np.uint64(63)) == 0
    print("invalid triples in the third batch: %d of %d" % (int(invalid.sum()), BATCH))
    assert 100 < int(invalid.sum()) < BATCH // 20


@pytest.mark.gpu
def test_an_early_stop_inside_the_third_batch_and_the_call_after_it(tdv, own, orc, scenes):
    """_noisy(1000, 1): the oracle's trace has an iteration b inside the third batch whose count beats everything before it.  With
    the confidence just under that fitness the call stops there - its third batch ran from staged triples, the fourth is drawn,
    staged and enqueued behind the stop and changes nothing.  iterations run and result are DIRECT's and the oracle's.  The next call
    on the same context - another seed, another cloud - equals the same call on a fresh context: nothing of the staging is left."""
    inputs = _noisy(EXIT_NS, EXIT_SEED)
    lo, hi = FIRST + BATCH, FIRST + 2 * BATCH
    trace = orc.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=hi, confidence=2.0, trace=True)
    inl = np.maximum(trace["inliers"][:hi].astype(np.int64), 0)
    before = np.maximum.accumulate(inl)
    new_best = [i for i in range(lo + BATCH // 4, hi) if inl[i] > before[i - 1]]
    assert new_best, "no new best inside the third batch: pick another scene"
    b = new_best[0]
    confidence = (int(inl[b]) - 0.5) / EXIT_NS
    passes = np.nonzero(inl.astype(np.float32) / np.float32(EXIT_NS) > np.float32(confidence))[0]
    assert int(passes[0]) == b, (passes[:3], b)
    iters = G + GROWN                                    # far past the stop
    direct = _modes(tdv, own, inputs, iters, 42, confidence, reached=b + 1)
    assert direct["got"][:3] == [b, b + 1, int(inl[b])], (direct["got"][:4], b, int(inl[b]))
    assert direct["bound"][0] == hi - FIRST, direct["bound"]          # the counters hold the batches up to the one the stop lies in
    whole = orc.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=iters, confidence=confidence, trace=True)
    assert [int(whole["best_iter"]), int(whole["iters_run"])] == [b, b + 1]
    assert direct["got"][3] == float(whole["fitness"]) and direct["got"][5] == whole["T"].tobytes().hex()
    # ... and the call after it
    nxt, n_iters = scenes[9999], FIRST + 2 * BATCH + 1
    after = _run(own, nxt, n_iters, "staged", seed=7)
    fresh_ctx = tdv.Context(0)
    try:
        fresh = _run(fresh_ctx, nxt, n_iters, "staged", seed=7)
    finally:
        fresh_ctx.close()
    assert _same(after, fresh) and after["staged"] == fresh["staged"] == 2, (after["got"][:5], fresh["got"][:5], after["staged"], fresh["staged"])


@pytest.mark.gpu
def test_a_traced_call_does_not_stage(own, scenes):
    """a trace makes the call score every test, without bail-out or bound: no carrier, and the host reads the slots itself"""
    iters = FIRST + BATCH + 100
    direct = _run(own, scenes[300], iters, "direct", trace=True)
    staged = _run(own, scenes[300], iters, "staged", trace=True)
    assert staged["staged"] == 0 and direct["staged"] == 0
    assert staged["got"] == direct["got"] and np.array_equal(staged["trace"], direct["trace"])


@pytest.mark.gpu
def test_the_bound_off_does_not_stage(tdv, own, scenes, monkeypatch):
    """TDV_RANSAC_BOUND=0: bail-out without the bound - no coarse level to carry the triples; the result is the bounded call's"""
    iters = FIRST + 2 * BATCH + 1
    with_bound = _run(own, scenes[9999], iters, "staged")
    monkeypatch.setenv("TDV_RANSAC_BOUND", "0")
    off = _run(own, scenes[9999], iters, "staged")
    monkeypatch.delenv("TDV_RANSAC_BOUND")
    assert off["staged"] == 0 and off["bound"] == [0, 0, 0, 0], (off["staged"], off["bound"])
    assert with_bound["staged"] == 2 and off["got"] == with_bound["got"], (with_bound["staged"], off["got"][:5], with_bound["got"][:5])


@pytest.mark.gpu
def test_a_band_wider_than_the_threshold_still_stages(tdv, own, scenes):
    """the 9,999-pair scene 100 km out: no hypothesis is bounded, every one is live without a walk - the coarse level still runs, so
    it still carries the triples"""
    src, tgt, corr, voxel = scenes[9999]
    far = (src + np.float32(1e5)).astype(np.float32), (tgt + np.float32(1e5)).astype(np.float32), corr, voxel
    direct = _modes(tdv, own, far, FIRST + 2 * BATCH + 1)
    assert direct["bound"][1] == 0 and direct["bound"][2] == 0, direct["bound"]


@pytest.mark.gpu
def test_bad_mode(tdv, own):
    assert tdv.lib().tdv_ctx_set_ransac_triples(own._h, 3) < 0 and tdv.lib().tdv_ctx_set_ransac_triples(own._h, -1) < 0
    assert tdv.lib().tdv_ctx_last_ransac_staged(None) == 0
