"""A RANSAC batch's path between its kernels (csrc/ransac.hip): k_ransac_hypotheses reads the batch's triples from the pinned buffer
the host drew them into and leaves the device copy for the later kernels - no copy in front of it - and the two one-workgroup kernels,
k_ransac_select_live and k_ransac_finish, hold a thread's list entries in registers where the far and the near list together have at
most 8,192 entries.  Neither may change a
result, so every case holds the call - best iteration, iterations run, inliers, fitness, the transform's bytes - to the oracle's traced
loop and to the exact kernel (set_ransac_score("exact")), which leaves no test out.  Shapes: both buffer sets twice each; an early exit
with the next batch drawn and in flight, then another call on the same context; a traced call over three batches; list lengths on both
sides of 8,192; a bounded batch of one hypothesis and empty lists; two equal calls; the study library's TDV_RANSAC_UPLOAD=inline (the
copy on the compute stream, as it was) from a child process.
The oracle draws the reference's one index stream (seed 42).  So the call behind the abandoned batch is held to the oracle with that
seed, and a second time, behind another abandoned batch, with another seed to the exact kernel's call with that seed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, BATCH = 8192, 65536          # the first batch of a call with bail-out, and every later one (csrc/ransac.hip)
SHORT = 17000                       # FIRST + one bounded batch of 8,808
IN_REGS = 8192                      # the longest far + near list the two kernels hold in registers (LIVE_REG x 1,024)
MAIN_ITERS = FIRST + 3 * BATCH + 1  # four bounded batches: both buffer sets twice each, the last of one hypothesis
EXIT_SEED = 7                       # test_gpu_ransac_far_bound.py's scene whose bounded batch holds a new best
OTHER_SEED = 7                      # an index stream the oracle does not draw
# Bounded batches of the cube, live totals on both sides of IN_REGS.  A call of up to 16,384 iterations runs as one batch without the
# bound, so a bounded batch has at least 8,193 hypotheses: batches of 8,000 and 8,192 do not exist.  The cube's index stream (seed 42,
# 500 pairs) has 8,139 valid triples in a bounded batch of 8,193, exactly 8,192 in one of 8,246 and 8,193 in one of 8,247.
LIST_SIZES = [8193, 8246, 8247, 65536]
VOXEL = 0.004


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


def _main_scene(ctx, synth):
    return _scene(ctx, synth, 4097, 0.5)


def _noisy(ns):
    """test_gpu_ransac_bound_lists.py's: every pair true, a voxel of noise"""
    rng = np.random.default_rng(ns)
    src = ((rng.random((ns, 3)) - 0.5) * 0.2).astype(np.float32)
    tgt = (src + rng.normal(size=(ns, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    return src, tgt, np.arange(ns, dtype=np.int32), 0.004


def _all_close():
    """test_gpu_ransac_bound_lists.py's cube: 500 true pairs in 5 voxels, 0.6 voxel of noise - every bounded hypothesis goes live"""
    rng = np.random.default_rng(500)
    src = ((rng.random((500, 3)) - 0.5) * 5 * VOXEL).astype(np.float32)
    tgt = (src + rng.normal(size=(500, 3)).astype(np.float32) * np.float32(0.6 * VOXEL)).astype(np.float32)
    return src, tgt, np.arange(500, dtype=np.int32), VOXEL


def _run(ctx, src, tgt, corr, voxel, iters, confidence=2.0, exact=True, seed=42):
    """the fast pass: result, scored share, counters - and the exact kernel's result"""
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, seed=seed)
    scored, bound = ctx.last_ransac_scored(), list(ctx.last_ransac_bound())
    ex = None
    if exact:
        try:
            ctx.set_ransac_score("exact")
            ex = _result(ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence, seed=seed))
        finally:
            ctx.set_ransac_score("fast")
    return {"got": _result(got), "scored": scored, "bound": bound, "exact": ex}


def _check(ctx, orc, inputs, iters, confidence=2.0, ref=None):
    """the call against the oracle and the exact kernel; returns the run"""
    run = _run(ctx, *inputs, iters, confidence)
    if ref is None:
        ref = _oracle(orc, *inputs, iters, confidence)[0]
    print("iters %d scored share %.6f bounded, close, fine, live %s result %s" % (iters, run["scored"], run["bound"], run["got"][:4]))
    assert run["got"] == ref, (run["got"][:4], ref[:4])
    assert run["got"] == run["exact"], (run["got"][:4], run["exact"][:4])
    return run


@pytest.fixture(scope="module")
def main_scene(ctx, synth):
    return _main_scene(ctx, synth)


@pytest.fixture(scope="module")
def main_ref(orc, main_scene):
    return _oracle(orc, *main_scene, MAIN_ITERS)[0]


@pytest.fixture(scope="module")
def main_run(ctx, orc, main_scene, main_ref):
    return _check(ctx, orc, main_scene, MAIN_ITERS, ref=main_ref)


@pytest.mark.gpu
def test_both_buffer_sets_twice_each(main_run):
    """4,097 points, half of the correspondences true, FIRST + 3 BATCH + 1 iterations: five batches, each buffer set's pinned triples
    drawn, read by the device and drawn over again at least twice; every bounded hypothesis is counted"""
    assert main_run["bound"][0] == 3 * BATCH + 1, main_run["bound"]


def _exit_case(ctx, orc, synth):
    inputs = _scene(ctx, synth, 30000, 0.5, seed=EXIT_SEED)
    inl = _oracle(orc, *inputs, SHORT)[1]["inliers"]
    m0 = int(inl[:FIRST].max())
    later = [j for j in range(FIRST, SHORT) if inl[j] > m0]
    assert later, "the scene's bounded batch holds no new best: no exit can fire there (m0 %d)" % m0
    confidence = float(np.float32(m0) / np.float32(len(inputs[0])))        # strict >: the first batch's best does not pass, inl[later[0]] does
    iters = FIRST + 2 * BATCH                                               # the batch behind the exit's has been drawn and enqueued
    ref = _oracle(orc, *inputs, iters, confidence)[0]
    assert ref[0] == later[0] and ref[1] == later[0] + 1, (ref[:3], later[0])
    return inputs, iters, confidence, ref


@pytest.mark.gpu
def test_exit_with_an_upload_in_flight_then_the_next_call(ctx, orc, synth, main_scene):
    """the loop stops inside the first bounded batch with the second one drawn and enqueued; the call that follows on the same
    context - another scene, 4,097 points against the 30,000 the abandoned triples index - is the oracle's: no triple of the abandoned
    batch reaches it.  Once more with an index stream of another seed, which only the exact kernel can be asked about."""
    inputs, iters, confidence, ref = _exit_case(ctx, orc, synth)
    nxt_iters = FIRST + BATCH + 1
    nxt_ref = _oracle(orc, *main_scene, nxt_iters)[0]
    got = _result(ctx.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=iters, confidence=confidence))
    nxt = _result(ctx.ransac(*main_scene[:2], corr=main_scene[2], voxel=main_scene[3], max_iterations=nxt_iters, confidence=2.0))
    print("exit call %s, the call behind it %s" % (got[:4], nxt[:4]))
    assert got == ref, (got[:4], ref[:4])
    assert nxt == nxt_ref, (nxt[:4], nxt_ref[:4])
    got = _result(ctx.ransac(*inputs[:2], corr=inputs[2], voxel=inputs[3], max_iterations=iters, confidence=confidence))
    other = _run(ctx, *main_scene, nxt_iters, seed=OTHER_SEED)
    print("exit call %s, the call behind it, seed %d: %s" % (got[:4], OTHER_SEED, other["got"][:4]))
    assert got == ref, (got[:4], ref[:4])
    assert other["got"] == other["exact"], (other["got"][:4], other["exact"][:4])
    assert other["got"] != nxt, "seed %d draws the stream of seed 42" % OTHER_SEED


@pytest.mark.gpu
def test_traced_call_over_three_batches(ctx, orc, synth):
    """a traced call scores every test in batches of BATCH: 2 BATCH + 1 iterations are three batches, the last of one triple, and
    the host reads the pinned triples again behind each batch (consume_trace); every per-iteration count is the oracle's"""
    src, tgt, corr, voxel = _scene(ctx, synth, 1000, 0.5)
    iters = 2 * BATCH + 1
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True)
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True)
    assert got.iterations_run == ref["iters_run"] == iters
    assert np.array_equal(got.trace_inliers, ref["inliers"]), "first difference at iteration %d" % int(np.nonzero(got.trace_inliers != ref["inliers"])[0][0])
    assert got.best_iteration == ref["best_iter"] and got.transformation.tobytes() == ref["T"].tobytes()


@pytest.mark.gpu
def test_list_lengths_on_both_sides_of_the_register_form(ctx, orc):
    """the cube in which every bounded hypothesis goes live, bounded batches of 8,193, 8,246, 8,247 and 65,536 hypotheses (see
    LIST_SIZES): live lists under, at and over the 8,192 entries the two kernels hold in registers"""
    inputs = _all_close()
    live = []
    for size in LIST_SIZES:
        run = _check(ctx, orc, inputs, FIRST + size)
        assert run["bound"][0] == size, run["bound"]
        live.append(run["bound"][3])
    print("bounded %s -> live %s" % (LIST_SIZES, live))
    assert any(0 < v <= IN_REGS for v in live), live
    assert any(v > IN_REGS for v in live), live


@pytest.mark.gpu
def test_a_bounded_batch_of_one_hypothesis(ctx, orc, main_scene):
    """FIRST + BATCH + 1 iterations: the last batch is one triple and lists of at most one entry.  (FIRST + 1 iterations
    have no bounded batch: a call of up to 16,384 iterations runs as one batch without the bound, and reports no bounded hypothesis.)"""
    run = _check(ctx, orc, main_scene, FIRST + BATCH + 1)
    assert run["bound"][0] == BATCH + 1, run["bound"]
    short = _check(ctx, orc, main_scene, FIRST + 1)
    assert short["bound"] == [0, 0, 0, 0], short["bound"]


@pytest.mark.gpu
def test_empty_lists_on_both_buffer_sets(ctx, orc):
    """two points: no valid triple, no best, and empty lists in the bounded batches of both buffer sets"""
    run = _check(ctx, orc, _noisy(2), FIRST + BATCH + 1)
    assert run["got"][0] == -1 and run["got"][2] == 0, run["got"][:4]


@pytest.mark.gpu
def test_determinism(ctx, orc, main_scene, main_ref, main_run):
    """the same call twice: the result, the scored share and the lists' counters are equal"""
    again = _check(ctx, orc, main_scene, MAIN_ITERS, ref=main_ref)
    assert again["got"] == main_run["got"]
    assert again["scored"] == main_run["scored"], (again["scored"], main_run["scored"])
    assert again["bound"] == main_run["bound"], (again["bound"], main_run["bound"])


@pytest.fixture(scope="module")
def inline_child(tdv):
    """the main call from a process on the study library under TDV_RANSAC_UPLOAD=inline: {got, scored, bound}"""
    assert not tdv.STUDY_BUILD, "this process must run the PRODUCT library"
    assert os.path.exists(os.path.join(ROOT, "3dvision_amd", "lib3dvision_hip_study.so")), "run __graft_entry__.build()"
    env = dict(os.environ, TDV_LIB_VARIANT="study", TDV_RANSAC_UPLOAD="inline")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


@pytest.mark.gpu
def test_the_study_knob_restores_the_inline_copy(main_run, main_ref, inline_child):
    """TDV_RANSAC_UPLOAD=inline on the study library: the same result, scored share and counters as the product library's run"""
    assert inline_child["got"] == main_ref, (inline_child["got"][:4], main_ref[:4])
    assert inline_child["got"] == main_run["got"]
    assert inline_child["scored"] == main_run["scored"], (inline_child["scored"], main_run["scored"])
    assert inline_child["bound"] == main_run["bound"], (inline_child["bound"], main_run["bound"])


def _main():
    import importlib
    sys.path.insert(0, ROOT)
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    assert tdv.STUDY_BUILD and os.environ.get("TDV_RANSAC_UPLOAD") == "inline"
    ctx = tdv.Context(0)
    run = _run(ctx, *_main_scene(ctx, synth), MAIN_ITERS, exact=False)
    print(json.dumps({"got": run["got"], "scored": run["scored"], "bound": run["bound"]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    _main()
