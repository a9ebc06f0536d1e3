"""tdv_tsdf_extract_mesh_dev and tdv_tsdf_fuse_mesh under the conditions tests/test_gpu_tsdf_state.py sets for the other TSDF entry points:
their outputs are a function of the arguments only, never of what the ctx did before or of the stream it runs on.  Held to the restatement
(tests/tsdf_mesh_restatement.py) byte for byte on a workspace poisoned with 0x00 and 0xFF, after a larger call has grown the arena, after
other entry points and right after a bad-argument return, and on a caller's stream.  Device buffers go through state_cases.Env and
StreamEnv."""
import numpy as np
import pytest
import torch

from state_cases import DEV, Env, StreamEnv
from test_gpu_tsdf import scene
from test_gpu_tsdf_mesh import device, live_buffers, restated, same
from test_tsdf_abi import PLANE_INTR, PLANE_RAW
from test_tsdf_mesh_abi import MeshOutputs, mesh_call

pytestmark = pytest.mark.gpu
F = np.float32
PARAMS = dict(max_weight=2.0)


@pytest.fixture(scope="module")
def case():
    """Three frames into 65 x 33 x 17 voxels and the restated mesh (computed once, never modified)."""
    s = scene((65, 33, 17), 3)
    ref = restated(s, **PARAMS)
    assert ref["nv"] > 500 and ref["nt"] > 500
    return dict(s=s, ref=ref)


def held(tdv, ctx, case, what, env=None):
    """The device entry point and the host form against the restatement."""
    s, ref = case["s"], case["ref"]
    same(ref, device(tdv, ctx, env or Env(ctx), s, **PARAMS), (what, "dev"))
    xyz, nrm, tri = ctx.tsdf_fuse_mesh(s["frames"], s["poses"], s["intr"], s["vol"].args(), **PARAMS)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes(), (what, "host")
    assert tri.tobytes() == ref["triangles"].tobytes(), (what, "host triangles")


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
    """A host-form call whose volume (400 x 300 x 100 voxels, 96 MB) does not fit the first block: a plane between two layers, whose mesh
    is known without the restatement - one vertex per column, two triangles per cell of the layer, all facing the camera."""
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")
        small = ctx.workspace_high_water()
        dims = (400, 300, 100)
        frames = np.full((1, 480, 640), PLANE_RAW, np.uint16)
        intr = (PLANE_INTR[0], 500.0, 500.0, 319.5, 239.5)
        xyz, nrm, tri = ctx.tsdf_fuse_mesh(frames, np.eye(4, dtype=F)[None], intr, ((-0.1, -0.075, 0.375), 0.0005, dims))
        assert ctx.workspace_high_water() > max(small, 64 << 20)
        assert len(xyz) == dims[0] * dims[1] and (nrm == np.array([0, 0, -1], F)).all() and np.abs(xyz[:, 2] - 0.4).max() < 1e-6
        assert len(tri) == 2 * (dims[0] - 1) * (dims[1] - 1) and tri.min() == 0 and tri.max() == len(xyz) - 1
        p = xyz.astype(np.float64)[tri]
        fz = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert (fz[:, 2] < 0).all() and (fz[:, :2] == 0).all()
        held(tdv, ctx, case, "after the larger call")                    # the call that coalesces the blocks, and those after it
        held(tdv, ctx, case, "and again")
    finally:
        ctx.close()


def test_after_other_entry_points_and_a_bad_argument_return(tdv, case, synth):
    ctx = tdv.Context(0)
    try:
        rng = np.random.default_rng(5)
        pts = synth.sample_object(4000, 5)[0]
        s = case["s"]
        calls = [lambda: ctx.fps(pts, 200), lambda: ctx.estimate_normals(pts, 20), lambda: ctx.voxel_downsample(pts, None, 0.004),
                 lambda: ctx.tsdf_fuse(s["frames"], s["poses"], s["intr"], s["vol"].args())]
        for k in rng.permutation(len(calls)):
            calls[k]()
            held(tdv, ctx, case, "after call %d of the history" % k)
        env = Env(ctx)
        buffers = live_buffers(env)
        for which, kw in (("extract_mesh", dict(triangle_capacity=-1)), ("extract_mesh", dict(nx=0)), ("fuse_mesh", dict(trunc=-1.0)),
                          ("fuse_mesh", dict(capacity=-1))):
            o = MeshOutputs()
            assert mesh_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == -2 and o.untouched()
            held(tdv, ctx, case, "right after a bad-argument return of %s %r" % (which, kw))
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
