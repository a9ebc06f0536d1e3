"""The probe cache of the hash-grid ICP search (csrc/icp.hip: grid_nearest<1>, tdv_ctx_set_icp_probe_cache) against the same call
without it, byte for byte: transformation, fitness, rmse, iterations and n_corr (tdv_icp_dev returns no correspondences; every one of
them enters those sums).  Every case asks for the hash-grid search, so that small problems do not take k_icp_small, and picks the launch
form where the form matters.

The cache keeps, per source point, the key of its cell and neighbour signs and the eight list heads the probes found, and takes them in
a later iteration of the same call when that iteration's key is the stored one.  What can go wrong is a head taken that the probes would
not have found: a stale one (another table, call, arena, stream, search), a key that does not tell two cells or two sides apart
(boundaries), a point the key cannot hold (non-finite, far out).  Sizes are wave and slab edges."""
import numpy as np
import pytest
import torch

from state_cases import DEV, Env, StreamEnv
from test_gpu_icp_one_launch import _key
from test_gpu_tree_sums_exact import _problem

pytestmark = pytest.mark.gpu
F = np.float32
THR = 0.004
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
LOSSES = {"l2": 0.0, "huber": 0.004}
FORMS = ["one", "two"]
RUNS = [(1, True), (2, True), (6, True), (40, False)]          # (iterations, fixed)


@pytest.fixture
def gctx(tdv):
    c = tdv.Context(0)
    c.set_icp_search("grid")
    yield c
    c.close()


def _call(ctx, cache, form, ps, ns, pt, pn, nt, T0, iters, p2plane, fixed, thr=THR):
    """One call: (result as bytes, last_icp_probe_misses)."""
    ctx.set_icp_probe_cache(cache); ctx.set_icp_launches(form)
    r = ctx.icp_dev(ps, ns, pt, pn if p2plane else None, nt, T0, thr, iters, p2plane, fixed_iterations=fixed)
    assert ctx.last_icp_search() == "grid" and ctx.last_icp_launches() == form, (ctx.last_icp_search(), ctx.last_icp_launches())
    return _key(r), ctx.last_icp_probe_misses()


def _off_on(ctx, env, src, tgt, nrm, T0, iters, p2plane, fixed, what, forms=FORMS, thr=THR):
    """OFF and ON on the same device buffers in every form: equal bytes.  Returns [(OFF's result, ON's misses)] per form."""
    ps, pt, pn = env.up(src), env.up(tgt), env.up(nrm)
    ns, nt = len(src), len(tgt)
    out = []
    for form in forms:
        off, m_off = _call(ctx, "off", form, ps, ns, pt, pn, nt, T0, iters, p2plane, fixed, thr)
        on, m_on = _call(ctx, "on", form, ps, ns, pt, pn, nt, T0, iters, p2plane, fixed, thr)
        assert m_off == -1, (what, form, m_off)
        assert on == off, (what, form, on, off)
        if iters >= 2:
            assert m_on >= 0, (what, form, m_on)          # the cache ran (a call of one iteration leaves it out: nothing could use it)
        else:
            assert m_on == -1, (what, form, m_on)
        out.append((off, m_on))
    return out


# ---------------------------------------------------------------- ON against OFF
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("p2plane", [True, False])
def test_on_equals_off(gctx, synth, p2plane, loss):
    gctx.set_icp_loss(loss, LOSSES[loss])
    env = Env(gctx)
    applied = 0
    for ns in SIZES:
        src, tgt, nrm, T0 = _problem(synth, ns, 500 + 250 * (ns % 11), seed=ns + 100)
        for iters, fixed in RUNS:
            for off, misses in _off_on(gctx, env, src, tgt, nrm, T0, iters, p2plane, fixed, (ns, iters, fixed)):
                applied += off[3]
                if iters >= 2:
                    assert misses >= ns, (ns, iters, fixed, misses)       # the first iteration finds every key invalid
    assert applied > 100          # the runs did iterate


def test_auto_takes_the_cache_with_one_launch_from_four_iterations_on(gctx, tdv, synth):
    src, tgt, nrm, T0 = _problem(synth, 1025, 2000, seed=4)
    env = Env(gctx)
    ps, pt, pn = env.up(src), env.up(tgt), env.up(nrm)
    assert gctx.last_icp_probe_misses() == -1          # before any call
    for form in FORMS:
        for iters in (1, 2, 3, 4, 6):
            auto, misses = _call(gctx, "auto", form, ps, 1025, pt, pn, 2000, T0, iters, True, True)
            off, _ = _call(gctx, "off", form, ps, 1025, pt, pn, 2000, T0, iters, True, True)
            cached = form == "one" and iters >= 4          # csrc/icp.hip: PROBE_CACHE_MIN_ITERATIONS
            assert auto == off and (misses >= 1025 if cached else misses == -1), (form, iters, misses)
    lib = tdv.lib()
    assert lib.tdv_ctx_set_icp_probe_cache(gctx._h, 3) == -2 and lib.tdv_ctx_set_icp_probe_cache(gctx._h, -1) == -2
    assert lib.tdv_ctx_set_icp_probe_cache(None, 0) == -2 and lib.tdv_ctx_last_icp_probe_misses(None) == -2


# ---------------------------------------------------------------- mixed waves: cells change for some iterations, then settle
@pytest.mark.parametrize("form", FORMS)
def test_cache_is_written_and_then_used(gctx, synth, form):
    ns, iters = 2049, 20
    src, tgt, nrm, T0 = _problem(synth, ns, 3000, seed=77, angle=3.0, trans=0.005)       # starts more than half a cell (0.0044) off
    (off, misses), = _off_on(gctx, Env(gctx), src, tgt, nrm, T0, iters, True, True, "mixed waves", [form])
    assert off[3] == iters
    print("probe misses", form, misses, "of", iters * ns)
    assert ns <= misses < iters * ns, (misses, ns, iters)


# ---------------------------------------------------------------- stale heads: equal keys, another table
@pytest.fixture(scope="module")
def two_targets(tdv, synth):
    """One source cloud and pose against two targets (the second a shifted, differently sampled cloud), and the OFF results on a fresh
    context (computed once, never modified)."""
    src, tgt_a, nrm_a, T0 = _problem(synth, 2049, 3000, seed=21)
    tgt_b, nrm_b = synth.sample_object(2500, 22)
    tgt_b = (tgt_b + F([0.0013, -0.0009, 0.0011])).astype(F)
    for a in (src, tgt_a, nrm_a, tgt_b, nrm_b):
        a.setflags(write=False)
    ctx = tdv.Context(0)
    try:
        ctx.set_icp_search("grid"); ctx.set_icp_probe_cache("off")
        env = Env(ctx)
        ps = env.up(src)
        ref = {}
        for name, (t, n) in (("a", (tgt_a, nrm_a)), ("b", (tgt_b, nrm_b))):
            pt, pn = env.up(t), env.up(n)
            for form in FORMS:
                ctx.set_icp_launches(form)
                ref[name, form] = _key(ctx.icp_dev(ps, len(src), pt, pn, len(t), T0, THR, 8, True, fixed_iterations=True))
                assert ctx.last_icp_probe_misses() == -1
    finally:
        ctx.close()
    assert ref["a", "one"] != ref["b", "one"]          # the targets do give different results
    return dict(src=src, T0=T0, tgt=dict(a=(tgt_a, nrm_a), b=(tgt_b, nrm_b)), ref=ref)


def _held(ctx, tt, what, env=None, order="ab"):
    """ON, the two targets in turn and again, same sources and pose: every call as its OFF reference."""
    env = env or Env(ctx)
    ctx.set_icp_search("grid")
    ps = env.up(tt["src"])
    up = {k: (env.up(t), env.up(n), len(t)) for k, (t, n) in tt["tgt"].items()}
    for form in FORMS:
        for name in order * 2:
            pt, pn, nt = up[name]
            got, misses = _call(ctx, "on", form, ps, len(tt["src"]), pt, pn, nt, tt["T0"], 8, True, True)
            assert got == tt["ref"][name, form], (what, form, name)
            assert misses >= len(tt["src"]), (what, form, name, misses)      # no key of the call before was taken


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_two_targets_on_one_context(tdv, two_targets, order):
    ctx = tdv.Context(0)
    try:
        _held(ctx, two_targets, "two targets " + order, order=order)
    finally:
        ctx.close()


def test_after_a_larger_call_has_grown_the_arena(tdv, two_targets):
    ctx = tdv.Context(0)
    try:
        _held(ctx, two_targets, "first calls")
        small = ctx.workspace_high_water()
        big = np.random.default_rng(5).random((1500000, 3)).astype(F)
        ctx.set_icp_search("pruned")
        ctx.icp(big, big, big, np.eye(4, dtype=F), THR, 1, False)
        assert ctx.workspace_high_water() > max(small, 64 << 20)      # past the first block
        _held(ctx, two_targets, "after the larger call", order="ba")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["null", "torch"])
def test_callers_stream(tdv, two_targets, kind):
    torch.cuda.synchronize()
    ts = torch.cuda.default_stream(DEV) if kind == "null" else torch.cuda.Stream(DEV)
    ctx = tdv.Context(0, stream=int(ts.cuda_stream))
    try:
        _held(ctx, two_targets, "a caller's stream (%s)" % kind, StreamEnv(ctx, ts))
    finally:
        ctx.close()
        torch.cuda.synchronize()


def test_after_the_search_went_to_brute_and_back(tdv, two_targets):
    ctx = tdv.Context(0)
    try:
        _held(ctx, two_targets, "first calls")
        ctx.set_icp_search("brute"); ctx.set_icp_probe_cache("on")
        tgt, nrm = two_targets["tgt"]["b"]
        ctx.icp(two_targets["src"], tgt, nrm, two_targets["T0"], THR, 3, True)
        assert ctx.last_icp_search() == "brute" and ctx.last_icp_probe_misses() == -1
        _held(ctx, two_targets, "after brute", order="ba")
    finally:
        ctx.close()


# ---------------------------------------------------------------- boundaries of the key
def _snapped(x, inv_cell, frac, step):
    """A float32 near x whose product with inv_cell is exactly a cell's lower edge + frac (0 or 0.5), moved by `step` ulps."""
    k = np.floor(F(x) * inv_cell)
    for dk in (0, 1, -1, 2, -2, 3, -3):
        g = F(k + dk + frac)
        c = F(g / inv_cell)
        for _ in range(8):
            c = np.nextafter(c, F(-np.inf))
        for _ in range(17):
            if F(c * inv_cell) == g:
                for _ in range(abs(step)):
                    c = np.nextafter(c, F(np.inf) if step > 0 else F(-np.inf))
                return c
            c = np.nextafter(c, F(np.inf))
    raise AssertionError("no float32 lands on the edge near %r" % x)


def test_cell_and_half_cell_boundaries(gctx, synth):
    """Sources whose grid coordinate gx = x * inv_cell under the identity pose is exactly a cell edge (gx - kx = 0), exactly the middle
    (0.5), and one ulp either side of both, per axis: where cx resp. the neighbour sign flips."""
    tgt, nrm = synth.sample_object(3000, 31)
    inv_cell = F(1.0) / (F(2.2) * F(THR))          # cell_grid_build's expression
    src = []
    for axis in range(3):
        for frac in (0.0, 0.5):
            for step in (-1, 0, 1):
                for p in tgt[(7 * axis + 3)::97][:10]:
                    q = p.copy(); q[axis] = _snapped(p[axis], inv_cell, F(frac), step)
                    if step == 0:
                        g = F(q[axis] * inv_cell)
                        assert g - np.floor(g) == F(frac)
                    src.append(q)
    src = np.asarray(src, F)
    assert len(src) == 180
    src = np.concatenate([src, tgt[:1025 - 180] + F(0.0005)]).astype(F)      # one slab and a point
    eye = np.eye(4, dtype=F)
    for p2plane in (True, False):
        for iters, fixed in ((2, True), (5, True), (12, False)):
            for off, misses in _off_on(gctx, Env(gctx), src, tgt, nrm, eye, iters, p2plane, fixed, ("boundaries", p2plane, iters, fixed)):
                assert off[4] >= 180 and misses >= len(src)


# ---------------------------------------------------------------- points the key cannot hold
def test_non_finite_and_far_out_sources_in_a_wave(gctx, synth):
    src, tgt, nrm, T0 = _problem(synth, 1025, 2500, seed=9)
    src = src.copy()
    rows = [0, 5, 17, 62, 63, 64, 100, 640, 1023, 1024]
    vals = [np.nan, np.inf, -np.inf, 3e7, -3e7, 1e19, -1e19, np.nan, np.inf, 2e3]      # 2e3 / 0.0088 > 2^17 cells; 3e7, 1e19 beyond the squares' range too
    for k, (r, v) in enumerate(zip(rows, vals)):
        src[r, k % 3] = F(v)
    for p2plane in (True, False):
        for iters, fixed in ((2, True), (6, True), (12, False)):
            for off, misses in _off_on(gctx, Env(gctx), src, tgt, nrm, T0, iters, p2plane, fixed, ("non-finite", p2plane, iters, fixed)):
                assert misses >= len(src)
                assert off[4] > 100          # the finite rest did find neighbours


# ---------------------------------------------------------------- the convergence stop
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("p2plane", [True, False])
def test_convergence_stop_lands_on_the_same_iteration(gctx, synth, p2plane, form):
    src, tgt, nrm, T0 = _problem(synth, 2049, 3000, seed=77, angle=3.0, trans=0.005)
    (off, misses), = _off_on(gctx, Env(gctx), src, tgt, nrm, T0, 60, p2plane, False, "convergence", [form])
    assert 2 <= off[3] < 60, off[3]          # it did stop by the rule, after iterating
    assert misses >= 2049
