"""RANSAC after round 6: the index stream drawn in bulk on the host and the leaf-box bound in two levels (csrc/ransac.hip,
k_ransac_bound: coarse leaves of 128 pairs, then the fine leaves for the undecided hypotheses only).
  * Runs of several batches with a per-iteration trace equal the oracle iteration for iteration (every count, every skipped
    iteration), on clouds small enough that triples repeat indices and across the 65,536-hypothesis batch boundaries.
  * The two-level bound leaves exactly the one-level bound's hypotheses to score: the study library's one-level walk
    (TDV_RANSAC_BOUND_LEVELS=1) gives the same result and the same scored share on the headline workload, the threshold shell,
    non-finite data and clouds 250 m and 100 km out.  That part runs in a process of its own that loads the study library."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("ns,iters", [(3, 140000), (7, 140000), (640, 140000), (5000, 70000)])
def test_multi_batch_trace_equals_the_oracle(ctx, orc, ns, iters):
    rng = np.random.default_rng(ns)
    src = ((rng.random((ns, 3)) - 0.5) * 0.2).astype(np.float32)
    tgt = (src + rng.normal(size=(ns, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    corr = np.arange(ns, dtype=np.int32)
    got = ctx.ransac(src, tgt, corr=corr, voxel=0.004, max_iterations=iters, confidence=2.0, trace=True)
    ref = orc.ransac(src, tgt, corr=corr, voxel=0.004, max_iterations=iters, confidence=2.0, trace=True)
    assert np.array_equal(got.trace_inliers, ref["inliers"])
    assert (got.best_iteration, got.iterations_run) == (ref["best_iter"], ref["iters_run"])
    assert got.transformation.tobytes() == ref["T"].tobytes()


@pytest.mark.gpu
def test_multi_batch_run_equals_the_oracle(ctx, orc, synth):
    """no trace: the bail-out and the two-level bound on, three batches and more"""
    n = 30000
    tgt, _ = synth.sample_object(n, 5)
    src, T_gt = synth.make_scene(n, 5)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(5)
    corr = np.where(rng.random(n) < 0.5, nn, rng.integers(0, n, n)).astype(np.int32)
    voxel = float(np.float32(synth.mean_spacing(n)))
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=150000, confidence=2.0)
    ref = orc.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=150000, confidence=2.0, trace=True)
    assert (got.best_iteration, got.iterations_run) == (ref["best_iter"], ref["iters_run"])
    assert got.inliers == int(ref["inliers"][ref["best_iter"]]) and got.fitness == ref["fitness"]
    assert abs(float(got.rmse) - float(ref["rmse"])) <= 1e-7 and got.transformation.tobytes() == ref["T"].tobytes()


@pytest.mark.gpu
def test_two_levels_leave_the_one_level_live_set(tdv):
    assert not tdv.STUDY_BUILD, "this process must run the PRODUCT library"
    assert os.path.exists(os.path.join(ROOT, "3dvision_amd", "lib3dvision_hip_study.so")), "run __graft_entry__.build()"
    env = dict(os.environ, TDV_LIB_VARIANT="study")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(rows) == len(_CASES), r.stdout[-2000:]
    for row in rows:
        print(row)
        assert row["two"] == row["one"], row
        assert row["scored_two"] == row["scored_one"], row
    head = [x for x in rows if x["case"] == "headline"][0]
    assert head["scored_two"] < 0.35


_CASES = ["headline", "shell", "nan_target", "inf_source", "offset250", "offset1e5"]


def _scene(ctx, synth, n, share, seed, offset=0.0):
    tgt, _ = synth.sample_object(n, seed)
    src, T_gt = synth.make_scene(n, seed)
    nn = ctx.icp_correspondences(src, tgt, T_gt, 1.0)["corr"]
    rng = np.random.default_rng(seed)
    corr = np.where(rng.random(n) < share, nn, rng.integers(0, n, n)).astype(np.int32)
    if offset:
        src = (src.astype(np.float64) + offset).astype(np.float32)
        tgt = (tgt.astype(np.float64) + offset).astype(np.float32)
    return src, tgt, corr, float(np.float32(synth.mean_spacing(n)))


def _shell(rng):
    """every good pair at the threshold from its transformed point, to a few ulps either side (tests/test_gpu_ransac_leaf_bound.py)"""
    ns, voxel = 8000, 0.004
    thr = np.float32(voxel * 1.5)
    src = ((rng.random((ns, 3)) - 0.5) * 40 * voxel).astype(np.float32)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    d = rng.normal(size=(ns, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = float(thr) * (1.0 + rng.choice([-2e-7, -6e-8, 0.0, 6e-8, 2e-7], ns))
    tgt = src.astype(np.float64) @ R.T + 0.05 + d * scale[:, None]
    bad = rng.random(ns) >= 0.6
    tgt[bad] = (rng.random((int(bad.sum()), 3)) - 0.5) * 2.0 + 5.0
    return src, tgt.astype(np.float32), np.arange(ns, dtype=np.int32), voxel


def _main():
    import importlib
    sys.path.insert(0, ROOT)
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    assert tdv.STUDY_BUILD
    ctx = tdv.Context(0)
    for case in _CASES:
        iters = 70000
        if case == "headline":
            src, tgt, corr, voxel = _scene(ctx, synth, 200000, 0.5, 42); iters = 100000
        elif case == "shell":
            src, tgt, corr, voxel = _shell(np.random.default_rng(3))
        elif case in ("nan_target", "inf_source"):
            src, tgt, corr, voxel = _scene(ctx, synth, 20000, 0.5, 11)
            rng = np.random.default_rng(5)
            rows = rng.choice(len(src), 40, replace=False)
            if case == "nan_target":
                tgt = tgt.copy(); tgt[corr[rows], rng.integers(0, 3, 40)] = np.nan
            else:
                src = src.copy(); src[rows, rng.integers(0, 3, 40)] = np.inf
        else:
            src, tgt, corr, voxel = _scene(ctx, synth, 50000, 0.5, 17, 250.0 if case == "offset250" else 1e5)
        res = {}
        for levels in ("2", "1"):
            os.environ["TDV_RANSAC_BOUND_LEVELS"] = levels
            r = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=2.0)
            res[levels] = ([r.best_iteration, r.iterations_run, r.inliers, float(r.fitness), float(r.rmse), r.transformation.tobytes().hex()],
                           ctx.last_ransac_scored())
        os.environ.pop("TDV_RANSAC_BOUND_LEVELS", None)
        print(json.dumps({"case": case, "two": res["2"][0], "one": res["1"][0], "scored_two": res["2"][1], "scored_one": res["1"][1]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    _main()
