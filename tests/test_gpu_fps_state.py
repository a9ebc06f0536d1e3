"""tdv_farthest_point_down_sample, its _dev form and tdv_farthest_point_down_sample_batch_dev under the conditions
tests/test_gpu_ctx_state.py sets for the other entry points: their outputs are a function of the arguments and the path switch only, never
of what the ctx did before or of the stream it runs on.  All three are held to the restatement (tests/fps_restatement.py) byte for byte, on
both kernel families, on a workspace poisoned with 0x00 and 0xFF, after a larger call has grown the arena, right after a bad-argument
return, and on a caller's stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import fps_restatement as R
from state_cases import DEV, Env, StreamEnv
from test_fps_abi import Outputs, fps_batch_call, fps_call
from test_gpu_fps import MODE, PATHS, same

pytestmark = pytest.mark.gpu
F = np.float32
N, WIDTH, K = 5000, 4, 300
OFF = np.array([0, 700, 700, 2300, 5000], np.int32)          # the batch: the same rows as four clouds, one empty
KB = 120


@pytest.fixture(scope="module")
def case(synth):
    """The cloud, its attr rows, and the restatements (computed once, never modified)."""
    pts = synth.sample_object(N, 21)[0].astype(np.float64)
    pts = (pts + np.random.default_rng(21).normal(0, 2e-4, pts.shape) + [0.1, -0.2, 0.6]).astype(F)
    pts[17] = np.nan; pts[4000, 1] = np.inf; pts[700] = np.nan
    attr = np.random.default_rng(22).random((N, WIDTH)).astype(F)
    ref = R.fps(pts, K, 11, attr)
    assert ref["n_selected"] == K and ref["n_usable"] == N - 3
    batch, batch_off = R.fps_batch(pts, OFF, KB, attr)
    for a in (pts, attr):
        a.setflags(write=False)
    return dict(pts=pts, attr=attr, ref=ref, batch=batch, batch_off=batch_off)


def _dev(ctx, env, case):
    oi, od, ox, oa = env.out(K, np.int32), env.out(K, F), env.out(3 * K, F), env.out(WIDTH * K, F)
    res = ctx.fps_dev(env.up(case["pts"]), N, K, 11, env.up(case["attr"]), WIDTH, oi.data_ptr(), od.data_ptr(), ox.data_ptr(), oa.data_ptr())
    m = res["n_selected"]
    return dict(res, index=env.get(oi, m, np.int32), d2=env.get(od, m, F), xyz=env.get(ox, 3 * m, F).reshape(-1, 3),
                attr=env.get(oa, WIDTH * m, F).reshape(m, WIDTH))


def _batch(ctx, env, case):
    cap = int(np.minimum(np.diff(OFF), KB).sum())
    oi, od, ox, oa = env.out(cap, np.int32), env.out(cap, F), env.out(3 * cap, F), env.out(WIDTH * cap, F)
    res, out_off = ctx.fps_batch_dev(env.up(case["pts"]), OFF, KB, env.up(case["attr"]), WIDTH, oi.data_ptr(), od.data_ptr(), ox.data_ptr(),
                                     oa.data_ptr())
    index, d2, xyz, attr = env.get(oi, cap, np.int32), env.get(od, cap, F), env.get(ox, 3 * cap, F).reshape(-1, 3), env.get(oa, WIDTH * cap, F).reshape(-1, WIDTH)
    return [dict(r, index=index[a:e], d2=d2[a:e], xyz=xyz[a:e], attr=attr[a:e]) for r, a, e in zip(res, out_off[:-1], out_off[1:])], out_off


def held(ctx, case, what, env=None):
    """Host, device and batch entry points on both paths against the restatement."""
    env = env or Env(ctx)
    for path in PATHS:
        ctx.set_fps_path(path)
        ref = dict(case["ref"], path=MODE[path])
        same(ref, ctx.fps(case["pts"], K, 11, case["attr"]), (what, path, "host"))
        same(ref, _dev(ctx, env, case), (what, path, "dev"))
        got, out_off = _batch(ctx, env, case)
        assert np.array_equal(out_off, case["batch_off"]), (what, path, out_off)
        for b, (r, g) in enumerate(zip(case["batch"], got)):
            same(dict(r, path=MODE[path]), g, (what, path, "batch", b))
    ctx.set_fps_path("auto")


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


def test_after_a_larger_call_has_grown_the_arena(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        small = ctx.workspace_high_water()
        big = np.random.default_rng(3).random((500000, 3)).astype(F)
        r = ctx.fps(big, 8, 0, np.zeros((len(big), 33), F))
        assert r["n_usable"] == len(big) and r["path"] == R.GRID and ctx.workspace_high_water() > max(small, 64 << 20)      # past the first block
        held(ctx, case, "after the larger call")                         # the call that coalesces the blocks, and those after it
    finally:
        ctx.close()


def test_after_a_bad_argument_return(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        for dev in (False, True):
            o = Outputs(tdv, K, WIDTH)
            assert fps_call(tdv.lib(), dev, ctx._h, case["pts"], case["attr"], o, n=N, num_samples=K, start_index=N, attr_width=WIDTH) == -2
            assert o.untouched()
            held(ctx, case, "right after a bad-argument return of the %s entry point" % ("device" if dev else "host"))
        o = Outputs(tdv, K, WIDTH, clouds=4)
        assert fps_batch_call(tdv.lib(), ctx._h, case["pts"], case["attr"], OFF[::-1].copy(), o, num_samples=KB, attr_width=WIDTH) == -2
        assert o.untouched()
        held(ctx, case, "right after a bad-argument return of the batch entry point")
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
