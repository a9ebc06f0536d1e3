"""The lists of the leaf-box bound (csrc/ransac.hip, RansacBoundLists): a bounded hypothesis close to the running best pose goes live
without a verdict of the walk, and the leaves are built once per call in front of the first bounded batch - in the study library
with TDV_RANSAC_LEAF_CLASSES=1 along a class-major Morton order (the ordering pose's outliers first, its inliers behind them).
Live needs no proof and a dead verdict is a leaf's own, so every case holds the result - best iteration, iterations run, inliers, fitness, the transform's bytes - to the
oracle's traced loop and to the exact kernel, which leaves no test out.  What the rule and the leaves change is seen in the
counters of Context.last_ransac_bound(): hypotheses bounded, close, put on the fine level's list, live.  The runs they are set
against - the rule off (TDV_RANSAC_LIVE_RADIUS=0), the natural order (TDV_RANSAC_ORDER=0), the one-level walk
(TDV_RANSAC_BOUND_LEVELS=1), the class-major leaves - come from ONE child process on the study library, which reads them per call.
Shapes: one bounded batch (17,000 iterations) unless a case says otherwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, BATCH = 8192, 65536          # the first batch of a call with bail-out, and every later one (csrc/ransac.hip)
SHORT = 17000                       # FIRST + one bounded batch of 8,808
ODD_SEED = 11                       # a 9,999-point scene whose best of 17,000 iterations lies in the bounded batch (test_gpu_ransac_far_bound.py)
VOXEL = 0.004
THR = 1.5 * VOXEL
RADIUS = 20.0                       # the rule's default radius, in thresholds

# the child's runs: configuration name -> environment
CONFIGS = {"off": {"TDV_RANSAC_LIVE_RADIUS": "0", "TDV_RANSAC_ORDER": "0"},       # no rule, Morton leaves: the bound before RansacBoundLists
           "radius0": {"TDV_RANSAC_LIVE_RADIUS": "0"},
           "natural": {"TDV_RANSAC_ORDER": "0"},
           "one_level": {"TDV_RANSAC_BOUND_LEVELS": "1"},
           "classes": {"TDV_RANSAC_LEAF_CLASSES": "1"}}
CHILD_RUNS = [("main", "off"), ("main", "one_level"), ("main", "classes"), ("noisy", "classes"), ("odd_classes", "classes"),
              ("same_cloud", "classes"), ("no_best", "classes"), ("same_cloud", "natural"), ("no_best", "natural"), ("all_close", "radius0"),
              ("far_out", "radius0"), ("non_finite", "radius0")]


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


def _noisy(ns):
    """test_gpu_ransac_point_order.py's: every pair true, a voxel of noise"""
    rng = np.random.default_rng(ns)
    src = ((rng.random((ns, 3)) - 0.5) * 0.2).astype(np.float32)
    tgt = (src + rng.normal(size=(ns, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
    return src, tgt, np.arange(ns, dtype=np.int32), 0.004


def _classes(n_far, n_mid, n_in, seed=3):
    """test_gpu_ransac_far_bound.py's: under the identity I matches itself, M lies three thresholds from its match, F twenty to sixty"""
    rng = np.random.default_rng(seed)
    n = n_far + n_mid + n_in
    src = ((rng.random((n, 3)) - 0.5) * 0.2).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([rng.uniform(20.0, 60.0, n_far), np.full(n_mid, 3.0), np.zeros(n_in)]) * THR
    p = rng.permutation(n)
    tgt = (src.astype(np.float64) + d * r[:, None]).astype(np.float32)
    return src[p], tgt[p], np.arange(n, dtype=np.int32), VOXEL


def _same_cloud():
    """source == target under the identity correspondences: every pair is an inlier of the best - one class"""
    rng = np.random.default_rng(1000)
    src = ((rng.random((1000, 3)) - 0.5) * 0.2).astype(np.float32)
    return src, src.copy(), np.arange(1000, dtype=np.int32), 0.004


def _all_close():
    """500 true pairs in a cube of 5 voxels, 0.6 voxel of noise.  Every hypothesis maps three points of the cube next to their
    matches; the worst of them - a nearly collinear triple - turns the cube about the triple's own line and moves a corner by at
    most twice the cube's diagonal, 2 * 8.7 voxels = 11.5 thresholds, under the radius of 20 (and of 13).  (A cube of 10 voxels, the size first
    thought of, has no such bound: 23 thresholds, and numpy on that scene's own triples finds corners moved by 19.3.)  The noise keeps the best count under the
    number of pairs (about 450 of 500), so that without the rule a leaf sum above the best exists."""
    rng = np.random.default_rng(500)
    src = ((rng.random((500, 3)) - 0.5) * 5 * VOXEL).astype(np.float32)
    tgt = (src + rng.normal(size=(500, 3)).astype(np.float32) * np.float32(0.6 * VOXEL)).astype(np.float32)
    return src, tgt, np.arange(500, dtype=np.int32), VOXEL


def _far_out(ctx, synth):
    """100 km from the origin the rounding band is wider than the threshold: the band is off, and the bound with it"""
    src, tgt, corr, voxel = _scene(ctx, synth, 4097, 0.5)
    return (src + np.float32(1e5)).astype(np.float32), (tgt + np.float32(1e5)).astype(np.float32), corr, voxel


def _non_finite(ctx, synth):
    """40 rows of a 20,000-point scene with a NaN or an infinite source coordinate: no hypothesis has a band"""
    src, tgt, corr, voxel = _scene(ctx, synth, 20000, 0.5, seed=11)
    rng = np.random.default_rng(5)
    rows = rng.choice(len(src), 40, replace=False)
    src = src.copy()
    src[rows, rng.integers(0, 3, 40)] = np.where(np.arange(40) % 2 == 0, np.nan, np.inf).astype(np.float32)
    return src, tgt, corr, voxel


def _cases(ctx, synth):
    """name -> (inputs, iterations)"""
    return {"main": (_scene(ctx, synth, 30000, 0.5), SHORT),
            "noisy": (_noisy(4097), FIRST + BATCH + 1025),
            "odd_classes": (_classes(1001, 502, 2500), SHORT),
            "same_cloud": (_same_cloud(), SHORT),
            "no_best": (_noisy(2), FIRST + BATCH + 1),
            "all_close": (_all_close(), SHORT),
            "far_out": (_far_out(ctx, synth), SHORT),
            "non_finite": (_non_finite(ctx, synth), SHORT)}


def _run(ctx, src, tgt, corr, voxel, iters, confidence=2.0, exact=True):
    """the fast pass as the environment sets it: result, scored share, counters - and the exact kernel's result"""
    got = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence)
    scored, bound = ctx.last_ransac_scored(), list(ctx.last_ransac_bound())
    ex = None
    if exact:
        try:
            ctx.set_ransac_score("exact")
            ex = _result(ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=confidence))
        finally:
            ctx.set_ransac_score("fast")
    return {"got": _result(got), "scored": scored, "bound": bound, "exact": ex}


def _check(ctx, orc, inputs, iters, ref=None):
    """the call against the oracle and the exact kernel; returns the run"""
    run = _run(ctx, *inputs, iters)
    if ref is None:
        ref = _oracle(orc, *inputs, iters)[0]
    print("iters %d scored share %.6f bounded, close, fine, live %s result %s" % (iters, run["scored"], run["bound"], run["got"][:4]))
    assert run["got"] == ref, (run["got"][:4], ref[:4])
    assert run["got"] == run["exact"], (run["got"][:4], run["exact"][:4])
    bounded, close, fine, live = run["bound"]
    assert bounded == max(0, iters - FIRST) and 0 <= close <= live <= bounded and 0 <= fine <= bounded - close, run["bound"]
    return run


@pytest.fixture(scope="module")
def cases(ctx, synth):
    return _cases(ctx, synth)


@pytest.fixture(scope="module")
def main_ref(orc, cases):
    return _oracle(orc, *cases["main"][0], SHORT)[0]


@pytest.fixture(scope="module")
def main_run(ctx, orc, cases, main_ref):
    return _check(ctx, orc, *cases["main"], ref=main_ref)


@pytest.fixture(scope="module")
def child(tdv):
    """CHILD_RUNS from one process on the study library: "case/config" -> {got, scored, bound}"""
    assert not tdv.STUDY_BUILD, "this process must run the PRODUCT library"
    assert os.path.exists(os.path.join(ROOT, "3dvision_amd", "lib3dvision_hip_study.so")), "run __graft_entry__.build()"
    env = dict(os.environ, TDV_LIB_VARIANT="study")
    for cfg in CONFIGS.values():
        for name in cfg:
            env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


@pytest.mark.gpu
def test_main_shorter_fine_list_same_result(main_run, main_ref, child):
    """half of the correspondences true: the result is everyone's, some hypotheses are close, and the fine level's list is strictly
    shorter than without the rule in the natural order - whose result is the same - and shorter again with class-major leaves"""
    off, cls = child["main/off"], child["main/classes"]
    print("bounded, close, fine, live: on %s, rule off and natural order %s, class-major leaves %s" % (main_run["bound"], off["bound"], cls["bound"]))
    assert off["got"] == main_ref and cls["got"] == main_ref, (off["got"][:4], cls["got"][:4], main_ref[:4])
    assert off["bound"][1] == 0, off["bound"]
    assert main_run["bound"][1] > 0, main_run["bound"]
    assert main_run["bound"][2] < off["bound"][2], (main_run["bound"], off["bound"])
    assert cls["bound"][1] == main_run["bound"][1] and cls["bound"][2] < main_run["bound"][2], (cls["bound"], main_run["bound"])


@pytest.mark.gpu
def test_class_boundary_inside_leaves_on_both_buffer_sets(ctx, orc, cases, child):
    """4,097 noisy pairs: 129 fine leaves, the last of one pair, 33 coarse leaves, the last partial; the classes' sizes are whatever
    the first batch's best makes them, so the boundary falls inside a fine and a coarse leaf.  FIRST + BATCH + 1,025 iterations:
    both buffer sets run a bounded batch on the leaves built behind the first batch - the Morton leaves here, the class-major
    ones in the child"""
    run = _check(ctx, orc, *cases["noisy"])
    assert child["noisy/classes"]["got"] == run["got"], (child["noisy/classes"]["got"][:4], run["got"][:4])


@pytest.mark.gpu
def test_odd_class_sizes(ctx, orc, cases, child):
    """|F| = 1,001, |M| = 502, |I| = 2,500 under the identity: the outliers end at pair 1,503, no multiple of 32 or 128"""
    run = _check(ctx, orc, *cases["odd_classes"])
    assert child["odd_classes/classes"]["got"] == run["got"], (child["odd_classes/classes"]["got"][:4], run["got"][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["same_cloud", "no_best"])
def test_one_class_is_the_morton_order(ctx, orc, cases, child, name):
    """every pair an inlier of the best, and no best at all (two points: no valid triple): one class, the class bit is the same in
    every key - with class-major leaves result, scored share and counters are those of the Morton leaves, in the two-way order
    and in the natural one"""
    run = _check(ctx, orc, *cases[name])
    for config in ("classes", "natural"):
        off = child[name + "/" + config]
        assert off["got"] == run["got"], (config, off["got"][:4], run["got"][:4])
        assert run["scored"] == off["scored"], (config, run["scored"], off["scored"])
        assert run["bound"] == off["bound"], (config, run["bound"], off["bound"])


@pytest.mark.gpu
def test_everything_close(ctx, orc, cases, child):
    """a cloud so small that every bounded hypothesis lies within the radius of the best: all of them go live unwalked, the fine
    list is empty - and is not with the rule off"""
    run = _check(ctx, orc, *cases["all_close"])
    off = child["all_close/radius0"]
    print("bounded, close, fine, live: on %s, rule off %s" % (run["bound"], off["bound"]))
    assert off["got"] == run["got"]
    assert run["bound"][2] == 0, run["bound"]
    assert off["bound"][1] == 0 and off["bound"][2] > 0, off["bound"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["far_out", "non_finite"])
def test_nothing_close(ctx, orc, cases, child, name):
    """the scene 100 km out, and NaN / infinite source coordinates: no band, so nothing is close - result and scored share are the
    rule-off run's"""
    run = _check(ctx, orc, *cases[name])
    off = child[name + "/radius0"]
    assert run["bound"][1] == 0, run["bound"]
    assert off["got"] == run["got"], (off["got"][:4], run["got"][:4])
    assert run["scored"] == off["scored"], (run["scored"], off["scored"])


@pytest.mark.gpu
def test_best_found_in_the_bounded_batch_by_a_close_hypothesis(ctx, orc, synth):
    """a scene whose best lies in the bounded batch (the oracle says so): the winner is a near-copy of the first batch's best, goes
    live by the rule (close > 0) and is scored exactly - count and record are the oracle's"""
    inputs = _scene(ctx, synth, 9999, 0.5, seed=ODD_SEED)
    ref, _ = _oracle(orc, *inputs, SHORT)
    assert ref[0] >= FIRST, "the scene's best lies in the first batch (iteration %d): pick another seed" % ref[0]
    run = _check(ctx, orc, inputs, SHORT, ref=ref)
    assert run["bound"][1] > 0, run["bound"]


@pytest.mark.gpu
def test_one_level_and_two_levels_agree_with_the_rule_on(main_run, child):
    """the one-level walk with the rule (the study library's TDV_RANSAC_BOUND_LEVELS=1): the same result, scored share and counters,
    but for the fine list, which it does not have"""
    one = child["main/one_level"]
    assert one["got"] == main_run["got"], (one["got"][:4], main_run["got"][:4])
    assert one["scored"] == main_run["scored"], (one["scored"], main_run["scored"])
    assert one["bound"][2] == 0 and one["bound"][:2] + one["bound"][3:] == main_run["bound"][:2] + main_run["bound"][3:], (one["bound"], main_run["bound"])


@pytest.mark.gpu
def test_determinism(ctx, orc, cases, main_ref, main_run):
    """the lists' lengths do not depend on the order the workgroups append in: a second call gives the same counters and scored share"""
    again = _check(ctx, orc, *cases["main"], ref=main_ref)
    assert again["bound"] == main_run["bound"], (again["bound"], main_run["bound"])
    assert again["scored"] == main_run["scored"], (again["scored"], main_run["scored"])


def _main():
    import importlib
    sys.path.insert(0, ROOT)
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    assert tdv.STUDY_BUILD
    ctx = tdv.Context(0)
    cases = _cases(ctx, synth)
    out = {}
    for name, config in CHILD_RUNS:
        os.environ.update(CONFIGS[config])
        try:
            inputs, iters = cases[name]
            run = _run(ctx, *inputs, iters, exact=False)
        finally:
            for var in CONFIGS[config]:
                os.environ.pop(var, None)
        out[name + "/" + config] = {"got": run["got"], "scored": run["scored"], "bound": run["bound"]}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    _main()
