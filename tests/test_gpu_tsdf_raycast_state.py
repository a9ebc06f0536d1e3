"""tdv_tsdf_raycast_dev, tdv_tsdf_raycast, tdv_depth_odometry_to_depth_dev, tdv_tsdf_track_dev and tdv_tsdf_track_sequence_dev under the
conditions tests/test_gpu_tsdf_state.py sets for the TSDF entry points: their outputs are a function of the arguments only, never of what
the ctx did before or of the stream it runs on.  Held to the restatement (tests/tsdf_raycast_restatement.py) byte for byte on a workspace
poisoned with 0x00 and 0xFF, after a larger call has grown the arena, after other entry points and right after a bad-argument return,
and on a caller's stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import odometry_cases as K
import tsdf_cases as Cs
import tsdf_raycast_restatement as R
import tsdf_restatement as Ts
from state_cases import DEV, Env, StreamEnv
from test_gpu_tsdf_raycast import OD_KW, ZMAX, device_cast, live_buffers, same_maps, same_track
from test_tsdf_abi import PLANE_INTR, PLANE_RAW
from test_tsdf_raycast_abi import Outputs, ray_call

pytestmark = pytest.mark.gpu
F = np.float32
N_FRAMES = 3
TRACK_KW = dict(tsdf=dict(zmax=ZMAX), odom=OD_KW)
SIZE = (96, 72)


@pytest.fixture(scope="module")
def case(orc):
    """Three views a degree apart into 48 x 40 x 32 voxels, and the restatement (computed once, never modified): the ray cast of the
    volume of frames 0 and 1 from frame 1's pose, frame 2 tracked against it, and the three frames tracked and fused as a sequence."""
    s = K.sequence(SIZE, N_FRAMES)
    poses = np.stack([np.linalg.inv(P.astype(np.float64)) for P in s["poses"]]).astype(F)
    vol = Cs.small_scene((48, 40, 32), 0)["vol"]
    buf, _ = Ts.integrate(vol, Ts.reset(vol), s["frames"][:2], poses[:2], s["intr"], pose_direction=Ts.SOURCE_ONTO_TARGET)
    cast = R.raycast(vol, buf, poses[1], SIZE, s["intr"][1:], zmax=ZMAX, pose_direction=Ts.SOURCE_ONTO_TARGET)
    one = R.track(orc, vol, buf, s["frames"][2], poses[1], s["intr"], **TRACK_KW)
    seq = R.track_sequence(orc, vol, Ts.reset(vol), s["frames"], s["intr"], poses[0], **TRACK_KW)
    assert cast["n_hit"] > 500 and one["odom"]["n_corr"] > 500
    return dict(s=s, poses=poses, vol=vol, buf=buf, cast=cast, one=one, seq=seq)


def held(tdv, ctx, case, what, env=None):
    """The device entry points and the host form against the restatement."""
    env = env or Env(ctx)
    s, vol, poses, intr = case["s"], case["vol"], case["poses"], case["s"]["intr"]
    cvol = tdv.tsdf_volume_struct(*vol.args())
    d_volume = env.up(case["buf"])
    kw = dict(zmax=ZMAX, pose_direction=Ts.SOURCE_ONTO_TARGET)
    same_maps(device_cast(tdv, ctx, env, vol, d_volume, poses[1], SIZE, intr[1:], **kw), case["cast"], (what, "raycast_dev"))
    same_maps(ctx.tsdf_raycast((cvol, case["buf"]), poses[1], *SIZE, *intr[1:], **kw), case["cast"], (what, "raycast"))
    d_raw = env.up(s["frames"][2])
    odom = ctx.depth_odometry_to_depth_dev(d_raw, env.up(case["cast"]["depth"]), *SIZE, *intr, **OD_KW)
    same_track(dict(pose=R.product(poses[1], odom["T"]), odom=odom, n_hit=case["cast"]["n_hit"]), case["one"], (what, "to_depth_dev"))
    same_track(ctx.tsdf_track_dev(cvol, d_volume, d_raw, poses[1], *SIZE, *intr, **TRACK_KW), case["one"], (what, "track_dev"))
    d_fresh = env.up(Ts.reset(vol))
    fresh = env.keep[-1]
    got_poses, res = ctx.tsdf_track_sequence_dev(cvol, d_fresh, env.up(s["frames"]), N_FRAMES, *SIZE, *intr, pose0=poses[0], **TRACK_KW)
    ref_poses, ref_res, ref_buf = case["seq"]
    assert got_poses.tobytes() == ref_poses.tobytes(), (what, "sequence poses")
    for k in range(N_FRAMES):
        same_track(res[k], ref_res[k], (what, "sequence", k))
    assert env.get(fresh, vol.voxels * 2, F).tobytes() == ref_buf.tobytes(), (what, "sequence volume")


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
    """tests/test_gpu_tsdf_state.py's larger call in between: a host-form fuse whose volume (96 MB) does not fit the first block."""
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")
        small = ctx.workspace_high_water()
        dims = (400, 300, 100)
        frames = np.full((1, 480, 640), PLANE_RAW, np.uint16)
        intr = (PLANE_INTR[0], 500.0, 500.0, 319.5, 239.5)
        xyz, _ = ctx.tsdf_fuse(frames, np.eye(4, dtype=F)[None], intr, ((-0.1, -0.075, 0.375), 0.0005, dims))
        assert ctx.workspace_high_water() > max(small, 64 << 20) and len(xyz) == dims[0] * dims[1]
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
        buffers = live_buffers(env)
        for which, kw in (("raycast_dev", dict(max_steps=0)), ("raycast", dict(zmin=-1.0)), ("to_depth_dev", dict(n_levels=0)),
                          ("track", dict(pose_direction=Ts.MODEL_TO_CAMERA)), ("sequence", dict(n_frames=-1))):
            o = Outputs()
            assert ray_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == -2 and o.untouched()
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
