"""tdv_ppf_match_batch_dev under the conditions tests/test_gpu_ppf_state.py sets for the single call: the eight-instance batch
(tests/ppf_batch_cases.py) returns the bytes a fresh context gave - poses with their scores, n_poses, peaks and peak offsets - on a workspace
poisoned with 0x00 and 0xFF without growing it, after a larger call has grown the arena, right after a bad-argument return, and on a
caller's stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import ppf_batch_cases as B
import ppf_scene as S
from state_cases import DEV, Env, StreamEnv
from test_gpu_ppf import dense_model, device_buffers, same_peaks
from test_ppf_abi import TDV_ERR_BAD_ARG
from test_ppf_batch_abi import BatchOutputs, batch_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(tdv, synth):
    """The eight instances and what a fresh context returns for them (computed once, never modified)."""
    sc = B.scene(synth, 1)
    clouds = B.clouds_of(synth, B.EIGHT)
    ctx = tdv.Context(0)
    try:
        got, peak_off = B.Setup(ctx, Env(ctx), clouds, sc["model"], sc["model_normals"]).batch()
    finally:
        ctx.close()
    same_peaks(S.restated(synth)["peaks"], got[B.EIGHT.index(1)][1], "a fresh context")
    assert all(len(bl) > 0 for bl, _ in got)
    return dict(sc=sc, clouds=clouds, batch=got, peak_off=peak_off)


def held(ctx, case, what, env=None):
    got, peak_off = B.Setup(ctx, env or Env(ctx), case["clouds"], case["sc"]["model"], case["sc"]["model_normals"]).batch()
    assert (peak_off == case["peak_off"]).all(), what
    B.same(case["batch"], got, what)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_workspace(tdv, case, byte):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first call")                                    # ... and the arena and staging now cover the call
        ctx.workspace_fill(byte)
        before = ctx.workspace_high_water()
        held(ctx, case, "workspace filled with 0x%02X" % byte)
        assert ctx.workspace_high_water() == before, "the call grew the workspace: part of what it used was not poisoned"
    finally:
        ctx.close()


def test_after_a_larger_call_has_grown_the_arena(tdv, synth, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first call")
        small = ctx.workspace_high_water()
        m, n = dense_model(synth, 1340)                                  # 1.8 M pairs: table, keys and sort scratch pass the first block; slabs
        res, _ = ctx.ppf_match(case["sc"]["scene"], case["sc"]["scene_normals"], m, n, S.THR, ref_stride=100)
        assert len(res) > 0 and ctx.workspace_high_water() > max(small, 64 << 20)
        held(ctx, case, "after the larger call")                         # the call that coalesces the blocks, and those after it
        held(ctx, case, "the call after that")
    finally:
        ctx.close()


def test_after_a_bad_argument_return(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first call")
        dev = device_buffers(tdv)
        for kw in (dict(angle_bins=0), dict(off=(0, 3, 2, 4)), dict(n=-1)):
            o = BatchOutputs(tdv)
            assert batch_call(tdv, ctx._h, o, dev=dev, **kw) == TDV_ERR_BAD_ARG
            assert o.untouched()
            held(ctx, case, "right after a bad-argument return (%r)" % (kw,))
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
