"""The coloured TSDF calls (include/tdv_hip.h: tdv_tsdf_integrate_color_dev) under the conditions tests/test_gpu_ctx_state.py sets for the other
entry points: their outputs are a function of the arguments only, never of what the ctx did before or of the stream it runs on.  Held to
the restatement (tests/tsdf_color_restatement.py) byte for byte on a workspace poisoned with 0x00 and 0xFF, after a larger call has grown
the arena, after other entry points and right after a bad-argument return, and on a caller's stream.  Device buffers go through
state_cases.Env and StreamEnv; tests/test_gpu_tsdf_state.py is the pattern."""
import numpy as np
import pytest
import torch

import tsdf_color_restatement as K
from state_cases import DEV, Env, StreamEnv
from test_gpu_tsdf_color import MAPS, ZMAX, cast_both, cscene, device, live_buffers, restated, same
from test_tsdf_abi import PLANE_INTR, PLANE_RAW
from test_tsdf_color_abi import Outputs, color_call

pytestmark = pytest.mark.gpu
F = np.float32
PARAMS = dict(max_weight=2.0)
SPLITS, KINDS = (1, 2), "cc"
SIZE = (37, 29)
CAM = (85.0, 89.25, 18.0, 14.25)


@pytest.fixture(scope="module")
def case():
    """Three frames into 65 x 33 x 17 voxels, in two coloured calls, a ray cast of the result, and the restatement of both (computed once,
    never modified)."""
    s = cscene((65, 33, 17), 3)
    ref = restated(s, SPLITS, KINDS, **PARAMS)
    cast = K.raycast(s["vol"], ref["volume"], ref["color"], s["poses"][2], SIZE, CAM, zmax=ZMAX)
    assert ref["n"] > 500 and ref["nt"] > 500 and ref["color"][..., 3].max() == 2 and cast["n_hit"] > 100 and cast["rgb_map"].any()
    return dict(s=s, ref=ref, cast=cast)


def held(tdv, ctx, case, what, env=None):
    """The device entry points - integrate, extract, mesh, ray cast - and the host form against the restatement."""
    s, ref, cast = case["s"], case["ref"], case["cast"]
    env = env or Env(ctx)
    same(ref, device(tdv, ctx, env, s, SPLITS, KINDS, **PARAMS), (what, "dev"))
    got, _ = cast_both(tdv, ctx, env, s["vol"], env.up(ref["volume"]), env.up(ref["color"]), s["poses"][2], SIZE, CAM, zmax=ZMAX)
    assert got["n_hit"] == cast["n_hit"] and all(got[m].tobytes() == cast[m].tobytes() for m in MAPS), (what, "ray cast")
    xyz, nrm, tri, rgb = ctx.tsdf_fuse_color(s["frames"], s["images"], s["poses"], s["intr"], s["vol"].args(), triangles=True, **PARAMS)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes() and rgb.tobytes() == ref["rgb"].tobytes(), (what, "host")
    assert tri.tobytes() == ref["triangles"].tobytes(), (what, "host")


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_workspace(tdv, case, byte):
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")                              # ... and the arena and staging now cover the calls
        ctx.workspace_fill(byte)
        before = ctx.workspace_high_water()
        held(tdv, ctx, case, "workspace filled with 0x%02X" % byte)
        assert ctx.workspace_high_water() == before, "the calls grew the workspace: part of what they used was not poisoned"
    finally:
        ctx.close()


def test_across_arena_growth(tdv, case):
    """A host-form call whose volumes (400 x 300 x 100 voxels, 288 MB) do not fit the first block: a plane of one colour between two
    layers, whose crossings are known without the restatement - one per column, normals (0, 0, -1), the colour that of every pixel."""
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")
        small = ctx.workspace_high_water()
        dims = (400, 300, 100)
        frames = np.full((1, 480, 640), PLANE_RAW, np.uint16)
        images = np.broadcast_to(np.array([0, 255, 51], np.uint8), (1, 480, 640, 3))
        intr = (PLANE_INTR[0], 500.0, 500.0, 319.5, 239.5)
        xyz, nrm, rgb = ctx.tsdf_fuse_color(frames, images, np.eye(4, dtype=F)[None], intr, ((-0.1, -0.075, 0.375), 0.0005, dims))
        assert ctx.workspace_high_water() > max(small, 256 << 20)
        assert len(xyz) == dims[0] * dims[1] and (nrm == np.array([0, 0, -1], F)).all() and np.abs(xyz[:, 2] - 0.4).max() < 1e-6
        assert np.abs(rgb - K.unit_colour([51, 255, 0])[None, :]).max() <= 5 * 2.0 ** -24      # T23 between two equal colours: five roundings
        held(tdv, ctx, case, "after the larger call")                    # the call that coalesces the blocks, and those after it
        held(tdv, ctx, case, "and again")
    finally:
        ctx.close()


def test_after_other_entry_points_and_a_bad_argument_return(tdv, case, synth):
    ctx = tdv.Context(0)
    try:
        rng = np.random.default_rng(5)
        pts = synth.sample_object(4000, 5)[0]
        calls = [lambda: ctx.fps(pts, 200), lambda: ctx.estimate_normals(pts, 20), lambda: ctx.voxel_downsample(pts, None, 0.004)]
        for k in rng.permutation(len(calls)):
            calls[k]()
            held(tdv, ctx, case, "after call %d of the history" % k)
        env = Env(ctx)
        buffers = live_buffers(env)[0]
        for which, kw in (("reset", dict(nx=0)), ("integrate", dict(n_frames=-1)), ("extract", dict(capacity=-1)), ("mesh", dict(triangle_capacity=-1)),
                          ("raycast", dict(zmin=0.0)), ("fuse", dict(trunc=-1.0))):
            o = Outputs()
            assert color_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == -2 and o.untouched()
            held(tdv, ctx, case, "right after a bad-argument return of " + which)
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
        held(tdv, ctx, case, "a caller's stream (%s)" % kind, StreamEnv(ctx, ts))
    finally:
        ctx.close()
        torch.cuda.synchronize()
