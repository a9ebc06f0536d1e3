"""A RANSAC batch crosses no event (csrc/ransac.hip): k_ransac_finish stores the batch's sequence number behind its record in pinned
memory and the host waits for that word (csrc/host_wait.hpp) where it used to synchronise with an event, and TDV_TIMER_RANSAC_SCORE
is fed by clock stamps that k_ransac_score_fast takes inside the dispatch, not by an event on either side of it.  Neither may change
a result: every case holds the call - best iteration, iterations run, inliers, fitness, the transform's bytes - to the oracle's
traced loop.  FIRST = 8,192 and BATCH = 65,536: a call above 16,384 iterations takes the bail-out path, whose batches end without
an event; shorter calls run as one batch through score_all, traced calls keep the event.
The wait loop itself runs on the CPU under the thread sanitiser, a std::thread in the device's part (tests/csrc/record_wait_tsan.cpp)."""
import os
import platform
import subprocess
import time

import numpy as np
import pytest

try:
    import torch
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, BATCH = 8192, 65536
MAIN_ITERS = FIRST + BATCH + 1      # batches of 8,192, 65,536 and 1
ONE_BATCH = 10000                   # one batch, every test scored (score_all)
N_MAIN = 4097
KINDS = ["own", "torch"]


def _result(r):
    return [int(r.best_iteration), int(r.iterations_run), int(r.inliers), float(r.fitness), r.transformation.tobytes().hex()]


def _oracle(orc, src, tgt, corr, voxel, iters, confidence=2.0):
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, trace=True)
    inl = int(ref["inliers"][ref["best_iter"]]) if ref["best_iter"] >= 0 else 0
    return [int(ref["best_iter"]), int(ref["iters_run"]), inl, float(ref["fitness"]), ref["T"].tobytes().hex()], ref


def _scene(ctx, synth, n, share, seed=5):
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < share, nn, rng.integers(0, n, n)).astype(np.int32)
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _call(c, inputs, iters, confidence=2.0, **kw):
    src, tgt, corr, voxel = inputs
    return c.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, seed=42, **kw)


@pytest.fixture(scope="module")
def scene(ctx, synth):
    return _scene(ctx, synth, N_MAIN, 0.5)


@pytest.fixture(scope="module")
def main_ref(orc, scene):
    """the oracle's result of the main call, and its per-iteration counts"""
    return _oracle(orc, *scene, MAIN_ITERS)


@pytest.fixture(scope="module")
def ctxs(tdv):
    """a context on a stream of its own and one bound to a torch stream, as tests/test_gpu_ctx_state.py builds it"""
    assert tdv.device_count() > 0, "no HIP device visible"
    torch.cuda.synchronize()
    ts = torch.cuda.Stream(torch.device("cuda", 0))
    made = {"own": tdv.Context(0), "torch": tdv.Context(0, stream=int(ts.cuda_stream))}
    assert int(made["torch"].stream or 0) == int(ts.cuda_stream) != 0
    yield made
    for c in made.values():
        c.close()
    ts.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_results_and_dispatch_counts(tdv, ctxs, scene, main_ref, kind):
    """three batches with timing off and on: the oracle's result both times; with timing on two scoring dispatches per batch, a time
    inside the call's own host-clock time, and nothing on the second read"""
    c = ctxs[kind]
    c.timing_enable(False)
    off = _result(_call(c, scene, MAIN_ITERS))
    c.timing_enable(True)
    try:
        c.timing_read(tdv.TIMER_RANSAC_SCORE)
        t0 = time.perf_counter()
        on = _result(_call(c, scene, MAIN_ITERS))        # (synchronised: the result is on the host)
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, launches = c.timing_read(tdv.TIMER_RANSAC_SCORE)
        again = c.timing_read(tdv.TIMER_RANSAC_SCORE)
    finally:
        c.timing_enable(False)
    print("%s stream: timing off %s, on %s; timer %.4f ms over %d dispatches, the call %.3f ms" % (kind, off[:4], on[:4], ms, launches, wall_ms))
    assert off == main_ref[0], (off[:4], main_ref[0][:4])
    assert on == off, (on[:4], off[:4])
    assert launches == 6, launches
    assert 0.0 < ms <= wall_ms, (ms, wall_ms)
    assert tuple(again) == (0.0, 0), again


@pytest.mark.gpu
def test_one_batch_call(tdv, orc, ctxs, scene):
    """10,000 iterations are one batch through score_all: one dispatch on the timer, and the oracle's result"""
    c = ctxs["own"]
    ref = _oracle(orc, *scene, ONE_BATCH)[0]
    c.timing_enable(True)
    try:
        c.timing_read(tdv.TIMER_RANSAC_SCORE)
        got = _result(_call(c, scene, ONE_BATCH))
        ms, launches = c.timing_read(tdv.TIMER_RANSAC_SCORE)
    finally:
        c.timing_enable(False)
    print("one batch: timer %.4f ms over %d dispatches" % (ms, launches))
    assert got == ref, (got[:4], ref[:4])
    assert launches == 1, launches
    assert ms > 0.0, ms


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_sequence_reuse(ctxs, scene, main_ref, kind):
    """the three-batch call three times in a row on one context, then a traced call (the event path) between two more: every result is
    the oracle's - a stale sequence word would show as an early or a wrong record - and so is every traced count"""
    c = ctxs[kind]
    ref, full = main_ref
    runs = [_result(_call(c, scene, MAIN_ITERS)) for _ in range(3)]
    traced = _call(c, scene, 2000, trace=True)
    runs.append(_result(_call(c, scene, MAIN_ITERS)))
    traced2 = _call(c, scene, BATCH + 1, trace=True)     # two traced batches, both buffer sets' events
    runs.append(_result(_call(c, scene, MAIN_ITERS)))
    for i, r in enumerate(runs):
        assert r == ref, (i, r[:4], ref[:4])
    assert np.array_equal(traced.trace_inliers, full["inliers"][:2000])
    assert np.array_equal(traced2.trace_inliers, full["inliers"][:BATCH + 1])


@pytest.mark.gpu
def test_early_stop_drains_the_speculative_batch(orc, ctxs, scene, main_ref):
    """a confidence that the first batch's best does not pass and a hypothesis of the second batch does: the loop stops there with the
    third batch drawn and enqueued.  Best iteration, iterations run and transform are the exact-mode call's and the oracle's, and the
    next call on the context is right: the abandoned batch's sequence number is not taken for the next call's"""
    c = ctxs["own"]
    inl = main_ref[1]["inliers"]
    m0 = int(inl[:FIRST].max())
    later = [j for j in range(FIRST, FIRST + BATCH) if inl[j] > m0]
    assert later, "the scene's second batch holds no new best: no exit can fire there (m0 %d)" % m0
    confidence = float(np.float32(m0) / np.float32(N_MAIN))     # strict >: the first batch's best does not pass, inl[later[0]] does
    iters = FIRST + 2 * BATCH
    ref = _oracle(orc, *scene, iters, confidence)[0]
    assert ref[0] == later[0] and ref[1] == later[0] + 1, (ref[:3], later[0])
    got = _result(_call(c, scene, iters, confidence))
    nxt = _result(_call(c, scene, MAIN_ITERS))
    try:
        c.set_ransac_score("exact")
        exact = _result(_call(c, scene, iters, confidence))
    finally:
        c.set_ransac_score("fast")
    print("stop at iteration %d of the second batch: %s, exact %s, the next call %s" % (later[0], got[:4], exact[:4], nxt[:4]))
    assert got == exact, (got[:4], exact[:4])
    assert got == ref, (got[:4], ref[:4])
    assert nxt == main_ref[0], (nxt[:4], main_ref[0][:4])


@pytest.mark.gpu
def test_bad_index_comes_through_the_record(tdv, ctxs, scene, main_ref):
    """a correspondence index outside [0, nt): the bad-argument error, which the host reads from the record behind the same wait; the
    next call on the context succeeds"""
    c = ctxs["own"]
    src, tgt, corr, voxel = scene
    for bad_value in (len(tgt), -1):
        bad = corr.copy(); bad[1234] = bad_value
        with pytest.raises(tdv.TdvError, match="bad argument"):
            _call(c, (src, tgt, bad, voxel), MAIN_ITERS)
        got = _result(_call(c, scene, MAIN_ITERS))
        assert got == main_ref[0], (got[:4], main_ref[0][:4])


def test_wait_loop_under_the_thread_sanitiser(tmp_path):
    """csrc/host_wait.hpp with a thread as the producer: the hand-over, a stale word of an earlier sequence, a producer that ends
    without writing (the error, no hang) and one that fails - clean under -fsanitize=thread.  No GPU, no Python in the checked code."""
    exe = str(tmp_path / "record_wait_tsan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(ROOT, "3dvision_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "record_wait_tsan.cpp"), "-o", exe, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if r.returncode != 0 and "unexpected memory mapping" in r.stderr:
        # the sanitiser's runtime could not lay out its shadow memory under this kernel's address-space randomisation (it gives up
        # before main): the same program once more with the randomisation off for this one process
        r = subprocess.run(["setarch", platform.machine(), "-R", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-2000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]
