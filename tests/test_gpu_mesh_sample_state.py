"""tdv_mesh_sample_points and its _dev form under the conditions tests/test_gpu_ctx_state.py sets for the other entry points: their outputs
are a function of the arguments only, never of what the ctx did before or of the stream it runs on.  Both are held to the restatement
(tests/mesh_sample_restatement.py) byte for byte on a workspace poisoned with 0x00 and 0xFF, after other entry points and after a
bad-argument return, across arena growth (a small call, the 65,540-triangle mesh with enough samples to leave the first block, the small
call again) and on a caller's stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import mesh_sample_restatement as R
from state_cases import DEV, Env, StreamEnv
from mesh_sample_cases import grid_mesh
from test_gpu_mesh_sample import run_dev, same, untouched_beyond
from test_mesh_sample_abi import Outputs, sample_call

pytestmark = pytest.mark.gpu
F = np.float32
NT, N, WIDTH, SEED, FIRST = 1000, 3000, 4, 6, 77


@pytest.fixture(scope="module")
def case():
    """A mesh with a bad, a NaN and a zero-area triangle, its companion rows, and the restatement (computed once, never modified)."""
    v, t = grid_mesh(NT, seed=12)
    v[5] = np.nan
    t[400] = (1, 1, 2); t[999] = (0, len(v), 1)
    attr = np.random.default_rng(13).random((len(v), WIDTH)).astype(F)
    ref = R.sample(v, t, N, attr, SEED, FIRST)
    assert ref["n_sampled"] == N and ref["n_bad"] > 1 and ref["n_degenerate"] == 1
    for a in (v, t, attr):
        a.setflags(write=False)
    return dict(v=v, t=t, attr=attr, ref=ref)


def held(ctx, case, what, env=None):
    """Host and device entry points against the restatement."""
    ref = case["ref"]
    same(ref, ctx.mesh_sample(case["v"], case["t"], N, case["attr"], SEED, FIRST), (what, "host"))
    got, whole, spec = run_dev(ctx, case["v"], case["t"], N, case["attr"], SEED, FIRST, env=env or Env(ctx))
    same(ref, got, (what, "dev"))
    untouched_beyond(whole, spec, N, what)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_workspace(tdv, case, byte):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")                                   # ... and the arena and staging now cover the calls
        ctx.workspace_fill(byte)
        before = ctx.workspace_high_water()
        held(ctx, case, "workspace filled with 0x%02X" % byte)
        assert ctx.workspace_high_water() == before, "the calls grew the workspace: part of what they used was not poisoned"
    finally:
        ctx.close()


def test_across_arena_growth(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        small = ctx.workspace_high_water()
        v, t = grid_mesh(65537 + 3, seed=3)
        n = 1500000                                                      # 48 bytes of device rows per sample: past the first block of 64 MiB
        r = ctx.mesh_sample(v, t, n, np.zeros((len(v), 3), F), seed=1)
        assert r["n_sampled"] == n and r["n_usable"] == len(t) and ctx.workspace_high_water() > max(small, 64 << 20)
        head = R.sample(v, t, 2000, seed=1)
        assert r["xyz"][:2000].tobytes() == head["xyz"].tobytes() and r["triangle"][:2000].tobytes() == head["triangle"].tobytes()
        held(ctx, case, "after the larger call")                         # the call that coalesces the blocks, and those after it
        held(ctx, case, "and again")
    finally:
        ctx.close()


def test_after_other_entry_points_and_a_bad_argument_return(tdv, case, synth):
    ctx = tdv.Context(0)
    try:
        pts = synth.sample_object(4000, 5)[0]
        ctx.fps(pts, 200)
        held(ctx, case, "after farthest point sampling")
        ctx.estimate_normals(pts, 20)
        held(ctx, case, "after normals")
        for dev in (False, True):
            o = Outputs(tdv)
            assert sample_call(tdv, dev, ctx._h, o, n_samples=-1) == -2 and o.untouched()
            held(ctx, case, "right after a bad-argument return of the %s entry point" % ("device" if dev else "host"))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["null", "torch"])
def test_callers_stream(tdv, case, kind):
    torch.cuda.synchronize()
    ts = torch.cuda.default_stream(DEV) if kind == "null" else torch.cuda.Stream(DEV)
    handle = int(ts.cuda_stream)
    ctx = tdv.Context(0, stream=handle)
    try:
        assert int(ctx.stream or 0) == handle
        held(ctx, case, "a caller's stream (%s)" % kind, StreamEnv(ctx, ts))
    finally:
        ctx.close()
        torch.cuda.synchronize()
