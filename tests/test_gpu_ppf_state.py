"""tdv_ppf_match, tdv_ppf_model_dev and tdv_ppf_match_dev under the conditions tests/test_gpu_ctx_state.py sets for the other entry points:
their outputs are a function of the arguments only, never of what the ctx did before or of the stream it runs on.  The peaks and the table
are held to the restatement (tests/ppf_restatement.py) byte for byte and the poses, with their scores, to the bytes a fresh context gave -
on a workspace poisoned with 0x00 and 0xFF, after a larger call has grown the arena, right after a bad-argument return, and on a caller's
stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import ppf_scene as S
from state_cases import DEV, Env, StreamEnv
from test_gpu_ppf import dense_model, dev_call, pose_blob, same_peaks
from test_ppf_abi import Outputs, TDV_ERR_BAD_ARG, ppf_call

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def case(tdv, synth):
    """The scene, the restatement on it, and the poses of a fresh context (computed once, never modified)."""
    sc, ref = S.build(synth), S.restated(synth)
    ctx = tdv.Context(0)
    try:
        res, more, pk = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, want_peaks=True)
    finally:
        ctx.close()
    same_peaks(ref["peaks"], pk, "a fresh context")
    assert len(res) == 8
    return dict(sc=sc, ref=ref, poses=pose_blob(res, more))


def held(ctx, case, what, env=None):
    """Host and device entry points against the restatement's peaks and table and the fresh context's poses."""
    env = env or Env(ctx)
    sc, ref = case["sc"], case["ref"]
    res, more, pk = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, want_peaks=True)
    same_peaks(ref["peaks"], pk, (what, "host"))
    assert pose_blob(res, more) == case["poses"], (what, "host")
    info, words, res, more, pk = dev_call(ctx, sc, env.up, env.out, env.get)
    m = ref["model"]
    assert (info["n_pairs"], info["n_keys"], F(info["diameter"]), F(info["distance_step"])) == (m["n_pairs"], m["n_keys"], m["diameter"], m["distance_step"])
    w = words.view(np.uint32)
    base, cap = (m["n_keys"] + 1 + 3) // 4 * 4, m["nt"] * (m["nt"] - 1)
    assert w[:m["n_keys"] + 1].tobytes() == m["offsets"].tobytes(), (what, "offsets")
    for k, name in enumerate(("pair", "alpha_bits")):
        assert w[base + k * cap:base + k * cap + m["n_pairs"]].tobytes() == m[name].tobytes(), (what, name)
    same_peaks(ref["peaks"], pk, (what, "dev"))
    assert pose_blob(res, more) == case["poses"], (what, "dev")


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


def test_after_a_larger_call_has_grown_the_arena(tdv, synth, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        small = ctx.workspace_high_water()
        m, n = dense_model(synth, 1340)                                  # 1.8 M pairs: table, keys and sort scratch pass the first block; slabs
        res, _ = ctx.ppf_match(case["sc"]["scene"], case["sc"]["scene_normals"], m, n, S.THR, ref_stride=100)
        assert len(res) > 0 and ctx.workspace_high_water() > max(small, 64 << 20)
        held(ctx, case, "after the larger call")                         # the call that coalesces the blocks, and those after it
    finally:
        ctx.close()


def test_after_a_bad_argument_return(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        for which in ("match", "match_dev", "model"):
            o = Outputs(tdv)
            assert ppf_call(tdv, which, ctx._h, o, angle_bins=0) == TDV_ERR_BAD_ARG
            assert o.untouched()
            held(ctx, case, "right after a bad-argument return of " + which)
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
