"""tdv_verify_poses_mesh, tdv_verify_poses_mesh_dev, tdv_render_depth_mesh and tdv_render_depth_mesh_dev under the conditions
tests/test_gpu_verify_state.py sets for the splat's entry points: their outputs are a function of the arguments only, never of what the ctx
did before or of the stream it runs on.  All four are held to the restatement (tests/verify_mesh_restatement.py) byte for byte on a
workspace poisoned with 0x00 and 0xFF, after other entry points (the splat verification among them: the two share their stage, plan and
read-back), after a larger call has grown the arena, right after a bad-argument return, and on a caller's stream.  Device buffers go
through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import mesh_cases
import verify_mesh_restatement as M
from state_cases import DEV, Env, StreamEnv
from test_gpu_verify_mesh import M2C, cam_of, frame_for, nudged, sheet, soup
from test_verify_abi import Outputs
from test_verify_mesh_abi import render_call, verify_call

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SCALE = 150, 140, 1000.0                               # a box of 2 x 2 tiles
PRM = dict(cull=M.CULL_NONE, tau=0.003, zmax=1.28, **M2C)


@pytest.fixture(scope="module")
def case():
    """The mesh (a sheet of small faces over the frame, 40 large triangles on top, a NaN vertex, an index past the end), the poses, the
    frame and the restatement's answer (computed once, never modified)."""
    cam = cam_of(W, H)
    sv, st = sheet(W, H, cam, 5.0, 31)
    bv, bt = soup(40, 32, W, H, cam, size=25.0, z=(0.7, 1.0))
    verts, tris = np.r_[sv, bv], np.r_[st, bt + len(sv)]
    verts[17] = np.nan; verts[700, 1] = np.inf
    tris[5, 1] = len(verts); tris[9, 0] = -1
    poses = np.stack([nudged(np.eye(4, dtype=F), 70 + i, 0.03) for i in range(9)])
    poses[4] = np.nan; poses[8] = poses[1]
    raw = frame_for(verts, tris, poses[0], W, H, cam, SCALE, 5, **PRM)
    ref, order, depths = M.verify(verts, tris, poses, raw, SCALE, **cam, **PRM)
    assert ref[4] == dict.fromkeys(M.RESULT, 0) and ref[8] == ref[1] and all(ref[0][k] > 0 for k in M.RESULT)
    for a in (verts, tris, poses, raw):
        a.setflags(write=False)
    return dict(cam=cam, verts=verts, tris=tris, poses=poses, raw=raw, ref=ref, order=order, depths=depths)


def held(ctx, case, what, env=None):
    """The four entry points against the restatement."""
    env = env or Env(ctx)
    cam, verts, tris, poses, raw = case["cam"], case["verts"], case["tris"], case["poses"], case["raw"]
    k = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    nv, nt = len(verts), len(tris)
    rprm = {a: b for a, b in PRM.items() if a != "tau"}
    got, order = ctx.verify_poses_mesh(verts, tris, poses, raw, SCALE, **cam, **PRM)
    assert got == case["ref"] and np.array_equal(order, case["order"]), (what, "host")
    got, order = ctx.verify_poses_mesh_dev(env.up(verts), nv, env.up(tris), nt, poses, env.up(raw), W, H, SCALE, *k, **PRM)
    assert got == case["ref"] and np.array_equal(order, case["order"]), (what, "dev")
    for i in (0, 3):
        assert ctx.render_depth_mesh(verts, tris, poses[i], W, H, **cam, **rprm).tobytes() == case["depths"][i].tobytes(), (what, "render", i)
        out = env.out(W * H, F)
        n = ctx.render_depth_mesh_dev(env.up(verts), nv, env.up(tris), nt, poses[i], W, H, *k, out.data_ptr(), **rprm)
        assert n == case["ref"][i]["n_rendered"], (what, "render dev", i)
        assert env.get(out, W * H, F).tobytes() == case["depths"][i].tobytes(), (what, "render dev", i)


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


def test_after_other_entry_points(tdv, case):
    ctx = tdv.Context(0)
    try:
        pts = np.random.default_rng(1).random((4000, 3)).astype(F)
        ctx.voxel_downsample(pts, None, 0.05)
        ctx.fps(pts, 64)
        held(ctx, case, "after voxel_downsample and fps")
        ctx.verify_poses(pts, case["poses"], case["raw"], SCALE, **case["cam"], splat=2, **M2C)
        held(ctx, case, "after the splat verification")
        ctx.estimate_normals(pts, 10)
        held(ctx, case, "after estimate_normals")
    finally:
        ctx.close()


def test_after_a_larger_call_has_grown_the_arena(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        small = ctx.workspace_high_water()
        w = h = 4200                                                     # a 67 MiB depth image: past the arena's first block
        cam = cam_of(w, h)
        verts, tris = mesh_cases.box((0.5, 0.4, 0.1), (0.0, 0.0, 1.0))
        img = ctx.render_depth_mesh(verts, tris, np.eye(4, dtype=F), w, h, **cam, **M2C)
        assert (img != 0).sum() > 200000 and ctx.workspace_high_water() > max(small, 64 << 20)
        held(ctx, case, "after the larger call")                         # the call that coalesces the blocks, and those after it
    finally:
        ctx.close()


def test_after_a_bad_argument_return(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        for dev in (False, True):
            o = Outputs(tdv)
            assert verify_call(tdv, dev, ctx._h, o, tau=0.0) == -2 and render_call(tdv, dev, ctx._h, o, cull=2) == -2
            assert o.untouched()
            held(ctx, case, "right after a bad-argument return of the %s entry points" % ("device" if dev else "host"))
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
