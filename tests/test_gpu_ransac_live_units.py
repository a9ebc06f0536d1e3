"""Job B of k_ransac_score_fast as resident workgroups that pull units of chunks (csrc/ransac.hip, round 10): untraced calls - the
bail-out and the leaf-box bound on, so that phase 1 scores the live list and phase 2 the survivors through the ticket words - against
the oracle's traced loop and against the same call on the exact kernel, which leaves no test out.  Shapes: the smallest at which the
schedule can go wrong - fewer chunks than XCDs, a prefix shorter than one unit, one chunk past a unit, live lists of one block and of
many (the move to the next block), a last bounded batch at, one below and one above a block boundary, one short bounded batch, a
batch whose live list is empty, and phase 2 behind a job-A phase 1 (the bound off, in a process of its own)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, BATCH = 8192, 65536          # the first batch of a call with bail-out, and every later one (csrc/ransac.hip)


def _result(r):
    return [int(r.best_iteration), int(r.iterations_run), int(r.inliers), float(r.fitness), r.transformation.tobytes().hex()]


def _oracle(orc, src, tgt, corr, voxel, iters):
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0, trace=True)
    inl = int(ref["inliers"][ref["best_iter"]]) if ref["best_iter"] >= 0 else 0
    return [int(ref["best_iter"]), int(ref["iters_run"]), inl, float(ref["fitness"]), ref["T"].tobytes().hex()]


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


def _check(ctx, orc, src, tgt, corr, voxel, iters):
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
    scored = ctx.last_ransac_scored()
    try:
        ctx.set_ransac_score("exact")
        exact = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
    finally:
        ctx.set_ransac_score("fast")
    ref = _oracle(orc, src, tgt, corr, voxel, iters)
    print("iters %d scored share %.4f result %s" % (iters, scored, _result(got)[:4]))
    assert _result(got) == ref, (_result(got)[:4], ref[:4])
    assert _result(got) == _result(exact), (_result(got)[:4], _result(exact)[:4])
    return scored


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [3, 500, 513, 4097])
def test_small_clouds(ctx, orc, ns):
    """64, 64, 128 and 576 chunks: shares of 8, 8, 16 and 72 chunks per XCD - under a unit, a unit, and units with a short tail; a
    prefix of them in phase 1 where the best count allows a cut"""
    _check(ctx, orc, *_noisy(ns), FIRST + BATCH + 1025)


@pytest.fixture(scope="module")
def scenes(ctx, synth):
    return {share: _scene(ctx, synth, 30000, share) for share in (0.5, 1.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("share", [0.5, 1.0])
@pytest.mark.parametrize("iters", [FIRST + BATCH + 1, FIRST + BATCH + 1024, FIRST + BATCH + 1025, 17000])
def test_live_lists_of_one_and_many_blocks(ctx, orc, scenes, share, iters):
    """share 0.5: an eighth of a batch is live; share 1.0: every hypothesis is, so a workgroup moves through many blocks.  The third
    batch of 1, 1,024 and 1,025 hypotheses puts the last live list below, at and above a block boundary at share 1.0; 17,000
    iterations give one short bounded batch."""
    _check(ctx, orc, *scenes[share], iters)


@pytest.mark.gpu
def test_empty_live_list(ctx, orc):
    """Two points: every triple repeats an index, no hypothesis is valid, so the bounded batches' live lists are empty and their
    scoring dispatches return before they draw a ticket: only the first batch (8 of the call's 8 + 64 + 1 blocks) is scored."""
    scored = _check(ctx, orc, *_noisy(2), FIRST + BATCH + 1)
    assert abs(scored - 8.0 / 73.0) < 1e-9, scored


@pytest.mark.gpu
def test_phase_2_after_a_job_a_phase_1(ctx, orc, scenes):
    """TDV_RANSAC_BOUND=0 (read per call through getenv: a process of its own): phase 1 is job A over the whole batch, phase 2 pulls
    units over k_ransac_select's list"""
    src, tgt, corr, voxel = scenes[0.5]
    iters = FIRST + BATCH + 1025
    env = dict(os.environ, TDV_RANSAC_BOUND="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(iters)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    row = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print(row["scored"], row["got"][:4])
    assert row["got"] == _oracle(orc, src, tgt, corr, voxel, iters)
    assert row["got"] == row["exact"]
    assert row["scored"] < 1.0, row["scored"]              # the bail-out left tests out: phase 2 ran over a list


def _main(iters):
    import importlib
    sys.path.insert(0, ROOT)
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    assert os.environ.get("TDV_RANSAC_BOUND") == "0"
    ctx = tdv.Context(0)
    src, tgt, corr, voxel = _scene(ctx, synth, 30000, 0.5)
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
    scored = ctx.last_ransac_scored()
    ctx.set_ransac_score("exact")
    exact = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
    print(json.dumps({"got": _result(got), "exact": _result(exact), "scored": scored}), flush=True)
    ctx.close()


if __name__ == "__main__":
    _main(int(sys.argv[1]))
