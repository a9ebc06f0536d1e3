"""The one-launch ICP iteration (csrc/icp.hip: k_icp_iterate, tdv_ctx_set_icp_launches) against the two launches it replaces, byte for
byte, and against what holds the two launches: the exact-sum oracle (tests/test_gpu_tree_sums_exact.py) and the loss restatement
(tests/test_gpu_icp_loss.py).  Every case runs on a Context of its own with the hash-grid search asked for, so that small problems do
not take k_icp_small.

The sizes are the kernel's own edges, not the workload's: a lone lane, a wave edge (63, 64), an accumulate-lane group with fewer than
four points (255 .. 1,023), a slab edge (1,024, 1,025: a last workgroup with one point), several slabs for the fold (2,047 .. 4,100)."""
import numpy as np
import pytest
import torch

import icp_loss_restatement as R
from state_cases import DEV, Env, StreamEnv
from test_gpu_nonfinite import _icp_problem, _poison_icp
from test_gpu_tree_sums_exact import _oracle, _problem, _same, _thresholds, _up

pytestmark = pytest.mark.gpu
F = np.float32
THR = 0.004
SIZES = [1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4100]
LOSSES = {"l2": 0.0, "huber": 0.004}
RUNS = [(1, True), (2, True), (5, True), (40, False)]          # (iterations, fixed)


@pytest.fixture
def octx(tdv):
    c = tdv.Context(0)
    c.set_icp_search("grid")
    yield c
    c.close()


def _key(r):
    """A result as bytes (NaNs of T as one pattern: a NaN's payload is the hardware's)."""
    T = np.where(np.isnan(r.transformation), F(np.nan), r.transformation).astype(F)
    return (T.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), r.iterations, r.n_corr)


def _run(ctx, form, ps, ns, pt, pn, nt, T0, thr, iters, p2plane, fixed, expect=None):
    ctx.set_icp_launches(form)
    r = ctx.icp_dev(ps, ns, pt, pn if p2plane else None, nt, T0, thr, iters, p2plane, fixed_iterations=fixed)
    assert ctx.last_icp_launches() == (expect or form), (form, ctx.last_icp_launches(), ctx.last_icp_search())
    return r


def _both(ctx, src, tgt, nrm, T0, thr, iters, p2plane, fixed, what, expect_one="one"):
    """ONE and TWO on the same device buffers: equal bytes.  Returns TWO's result."""
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    two = _run(ctx, "two", ps, len(src), pt, pn, len(tgt), T0, thr, iters, p2plane, fixed)
    one = _run(ctx, "one", ps, len(src), pt, pn, len(tgt), T0, thr, iters, p2plane, fixed, expect_one)
    assert _key(one) == _key(two), (what, one.transformation, two.transformation, one.rmse, two.rmse, one.n_corr, two.n_corr)
    return two


# ---------------------------------------------------------------- ONE against TWO
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("p2plane", [True, False])
def test_one_equals_two(octx, synth, p2plane, loss):
    octx.set_icp_loss(loss, LOSSES[loss])
    applied = 0
    for ns in SIZES:
        src, tgt, nrm, T0 = _problem(synth, ns, 3000 + 250 * (ns % 13), seed=ns + 100)
        for iters, fixed in RUNS:
            two = _both(octx, src, tgt, nrm, T0, THR, iters, p2plane, fixed, (ns, iters, fixed))
            applied += two.iterations
        assert octx.last_icp_search() == "grid"
    assert applied > 100          # the runs did iterate


# ---------------------------------------------------------------- ONE against the exact-sum oracle and the loss restatement
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns", [1025, 4100])
def test_one_against_the_exact_sum_oracle(octx, orc, synth, ns, p2plane):
    octx.set_icp_launches("one")
    src, tgt, nrm, T0 = _problem(synth, ns, 3500, seed=ns + 5)
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    for iters, fixed in ((1, True), (1, False), (40, False)):
        ref = _oracle(orc, src, tgt, nrm, T0, THR, iters, p2plane, "ns %d iters %d" % (ns, iters))
        got = _run(octx, "one", ps, ns, pt, pn, len(tgt), T0, THR, iters, p2plane, fixed)
        _same(got, ref, "ns %d iters %d fixed %s" % (ns, iters, fixed))


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("ns", [1025, 4100])
def test_one_against_the_loss_restatement(octx, orc, synth, ns, p2plane):
    src, tgt, nrm, T0 = _problem(synth, ns, 3500, seed=ns + 5)
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    held = 0
    for loss, scale in (("huber", 0.004), ("tukey", 0.008), ("cauchy", 0.004)):
        octx.set_icp_loss(loss, scale)
        for iters, fixed in ((1, True), (8, False)):
            ref = R.icp(orc, src, tgt, nrm, T0, THR, iters, p2plane, loss, scale, fixed)
            if ref["ambiguous"]:
                continue
            got = _run(octx, "one", ps, ns, pt, pn, len(tgt), T0, THR, iters, p2plane, fixed)
            what = (ns, loss, iters, fixed)
            assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), what
            assert got.transformation.tobytes() == ref["T"].tobytes(), (what, got.transformation, ref["T"])
            assert np.float32(got.rmse).tobytes() == np.float32(ref["rmse"]).tobytes() and np.float32(got.fitness).tobytes() == np.float32(ref["fitness"]).tobytes(), what
            held += 1
    assert held >= 4, "too many restated sums are ambiguous: pick another input"


# ---------------------------------------------------------------- acceptance counts
@pytest.mark.parametrize("p2plane", [True, False])
def test_none_three_and_all_accepted(octx, orc, synth, p2plane):
    src, tgt, nrm, T0 = _problem(synth, 1100, 3000, seed=9, angle=4.0, trans=0.01)
    ths = _thresholds(orc, src, tgt, T0)
    assert {"two", "three"} <= set(ths), ths
    nearest = np.sqrt(orc.icp_correspondences(src, tgt, None, T0, 1e9, False)["d2"].astype(np.float64)).min()
    assert nearest > 1e-5
    # nothing within reach: the loop ends with n_corr < 3
    two = _both(octx, src, tgt, nrm, T0, np.float32(0.5 * nearest), 5, p2plane, False, "none")
    assert (two.iterations, two.n_corr) == (0, 0)
    two = _both(octx, src, tgt, nrm, T0, ths["two"], 5, p2plane, False, "two accepted")
    assert two.iterations == 0
    two = _both(octx, src, tgt, nrm, T0, ths["three"], 1, p2plane, True, "three accepted")
    assert (two.iterations, two.n_corr) == (1, 3)
    # every source on a target: the source is the target's own points
    pose = np.eye(4, dtype=F)
    two = _both(octx, tgt[:1100].copy(), tgt, nrm, pose, THR, 1, p2plane, True, "all accepted")
    assert two.n_corr == 1100 and np.float32(two.fitness) == 1.0
    assert octx.last_icp_search() == "grid"


# ---------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("kind", ["src_nan", "src_inf", "src_far", "nrm_nan", "nrm_inf", "nrm_huge", "tgt_nan", "tgt_inf", "T0_nan", "T0_inf"])
def test_non_finite_rows_and_poses(octx, synth, kind, p2plane):
    src, tgt, nrm, T0 = _icp_problem(synth, 1100, 3000, 9)
    rng = np.random.default_rng(1)
    T0 = np.asarray(T0, F).copy()
    if kind == "src_far":                            # beyond the grid's 2^17 cells, and beyond the squares' range
        src = src.copy(); src[[0, 300, 1023, 1024, 1099], [0, 1, 2, 0, 1]] = F([3e7, -3e7, 1e19, -1e19, 3e7])
    elif kind == "T0_nan":
        T0[1, 3] = np.nan
    elif kind == "T0_inf":
        T0[0, 0] = np.inf
    else:
        src, tgt, nrm = _poison_icp(src, tgt, nrm, kind, rng)
    on_grid = not kind.startswith("tgt")              # a flagged target hands the search to the box walk: two launches
    for loss in LOSSES:
        octx.set_icp_loss(loss, LOSSES[loss])
        for iters, fixed in ((1, True), (5, True), (8, False)):
            _both(octx, src, tgt, nrm, T0, THR, iters, p2plane, fixed, (kind, loss, iters, fixed), "one" if on_grid else "two")
    assert octx.last_icp_search() == ("grid" if on_grid else "pruned")


# ---------------------------------------------------------------- state
@pytest.fixture(scope="module")
def case(tdv, synth):
    """A four-slab problem and its results on a fresh context, two launches (computed once, never modified)."""
    src, tgt, nrm, T0 = _problem(synth, 4100, 3500, seed=77, angle=3.0, trans=0.005)
    for a in (src, tgt, nrm):
        a.setflags(write=False)
    ctx = tdv.Context(0)
    try:
        ctx.set_icp_search("grid"); ctx.set_icp_launches("two")
        env = Env(ctx)
        ps, pt, pn = env.up(src), env.up(tgt), env.up(nrm)
        ref = {}
        for p2plane in (True, False):
            for iters, fixed in ((40, False), (6, True), (33, True)):
                ref[p2plane, iters, fixed] = _key(ctx.icp_dev(ps, 4100, pt, pn if p2plane else None, 3500, T0, THR, iters, p2plane, fixed_iterations=fixed))
        assert ctx.last_icp_launches() == "two"
    finally:
        ctx.close()
    return dict(src=src, tgt=tgt, nrm=nrm, T0=T0, ref=ref)


def held(ctx, case, what, env=None):
    """Every run of the case with one launch per iteration, in a row on one context: the non-fixed run stops in the middle of a burst
    (the launches after it return at st->done and must leave the ticket alone), and each call after it needs the ticket back at 0."""
    env = env or Env(ctx)
    ctx.set_icp_search("grid"); ctx.set_icp_launches("one")
    ps, pt, pn = env.up(case["src"]), env.up(case["tgt"]), env.up(case["nrm"])
    for rep in range(2):
        for (p2plane, iters, fixed), ref in case["ref"].items():
            got = ctx.icp_dev(ps, 4100, pt, pn if p2plane else None, 3500, case["T0"], THR, iters, p2plane, fixed_iterations=fixed)
            assert ctx.last_icp_launches() == "one"
            assert _key(got) == ref, (what, rep, p2plane, iters, fixed)


def test_calls_in_a_row_and_after_a_run_that_ended_mid_burst(tdv, case):
    ctx = tdv.Context(0)
    try:
        assert case["ref"][True, 40, False][3] not in (0, 4, 12, 20, 28, 36, 40)      # ended inside a burst (4 launches, then 8 at a time)
        held(ctx, case, "calls in a row")
    finally:
        ctx.close()


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_workspace(tdv, case, byte):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        ctx.workspace_fill(byte)
        before = ctx.workspace_high_water()
        held(ctx, case, "workspace filled with 0x%02X" % byte)
        assert ctx.workspace_high_water() == before, "the calls grew the workspace: part of what they used was not poisoned"
    finally:
        ctx.close()


def test_after_a_larger_call_has_grown_the_arena(tdv, synth, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        small = ctx.workspace_high_water()
        big = np.random.default_rng(5).random((1500000, 3)).astype(F)
        ctx.set_icp_search("pruned")
        ctx.icp(big, big, big, np.eye(4, dtype=F), THR, 1, False)
        assert ctx.workspace_high_water() > max(small, 64 << 20)      # past the first block
        held(ctx, case, "after the larger call")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["null", "torch"])
def test_callers_stream(tdv, case, kind):
    torch.cuda.synchronize()
    ts = torch.cuda.default_stream(DEV) if kind == "null" else torch.cuda.Stream(DEV)
    handle = int(ts.cuda_stream)
    ctx = tdv.Context(0, stream=handle)
    try:
        held(ctx, case, "a caller's stream (%s)" % kind, StreamEnv(ctx, ts))
    finally:
        ctx.close()
        torch.cuda.synchronize()


# ---------------------------------------------------------------- what ran
def test_last_icp_launches(octx, tdv, synth):
    ns, nt = 4100, 3500
    src, tgt, nrm, T0 = _problem(synth, ns, nt, seed=3)
    rng = np.random.default_rng(3)
    snrm = synth.sample_object(ns, 8)[1]
    rgb_s, rgb_t = rng.random((ns, 3)).astype(F), rng.random((nt, 3)).astype(F)
    assert octx.last_icp_launches() == "auto"                       # before any call
    octx.set_icp_launches("one")
    r = octx.icp(src, tgt, nrm, T0, THR, 3, True)
    assert octx.last_icp_launches() == "one" and octx.last_icp_search() == "grid" and r.iterations > 0
    octx.icp(src, tgt, nrm, T0, THR, 3, False)
    assert octx.last_icp_launches() == "one"
    octx.gicp(src, snrm, tgt, nrm, T0, THR, 3)
    assert octx.last_icp_launches() == "two" and octx.last_icp_search() == "grid"
    octx.colored_icp(src, rgb_s, tgt, nrm, octx.color_gradients(tgt, rgb_t, nrm), T0, THR, 3)
    assert octx.last_icp_launches() == "two" and octx.last_icp_search() == "grid"
    octx.set_icp_search("pruned")
    octx.icp(src, tgt, nrm, T0, THR, 3, True)
    assert octx.last_icp_launches() == "two" and octx.last_icp_search() == "pruned"
    octx.set_icp_search("grid")
    octx.set_icp_accumulation("reference")
    octx.icp(src, tgt, nrm, T0, THR, 3, True)
    assert octx.last_icp_launches() == "two" and octx.last_icp_search() == "grid"
    octx.set_icp_accumulation("tree")
    octx.set_icp_launches("two")
    octx.icp(src, tgt, nrm, T0, THR, 3, True)
    assert octx.last_icp_launches() == "two"
    # AUTO follows the size rule of csrc/icp.hip (ONE_LAUNCH_MIN_SOURCES .. ONE_LAUNCH_MAX_SOURCES)
    octx.set_icp_launches("auto")
    octx.icp(src, tgt, nrm, T0, THR, 3, True)
    assert octx.last_icp_launches() == AUTO_AT_4100
    assert tdv.lib().tdv_ctx_set_icp_launches(octx._h, 3) == -2 and tdv.lib().tdv_ctx_set_icp_launches(octx._h, -1) == -2
    octx.icp(src, tgt, nrm, T0, THR, 3, True)
    assert octx.last_icp_launches() == AUTO_AT_4100                # a refused mode left the setting


AUTO_AT_4100 = "two"          # 4,100 sources lie below ONE_LAUNCH_MIN_SOURCES
