"""tdv_depth_maps_dev, tdv_depth_odometry_terms_dev, tdv_depth_odometry_dev, tdv_depth_odometry and tdv_depth_odometry_sequence_dev under
the conditions tests/test_gpu_ctx_state.py sets for the other entry points: their outputs are a function of the arguments only, never of
what the ctx did before or of the stream it runs on.  Held to the restatement (tests/odometry_restatement.py) byte for byte on a workspace
poisoned with 0x00 and 0xFF, after a larger call has grown the arena, right after a bad-argument return, after an unrelated ICP call with
every switch set off-default, and on a caller's stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import odometry_restatement as R
from state_cases import DEV, Env, StreamEnv
from test_gpu_odometry import device_maps, frame, intrinsics, live_buffers, same_result, small_pose
from test_odometry_abi import Outputs, odom_call

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 65, 47
PARAMS = dict(n_levels=3, max_iterations=(5, 3, 2))


@pytest.fixture(scope="module")
def case(orc):
    """Four frames of 65 x 47, and the restatement of every call (computed once, never modified)."""
    frames = np.stack([frame(W, H, k) for k in (0, 1, 2, 4)])
    intr = intrinsics(W, H)
    T0 = small_pose(5)
    p = R.params(**PARAMS)
    ps, pt = R.pyramid(frames[1], intr, p), R.pyramid(frames[0], intr, p)
    ref = dict(maps=R.maps(frames[0], intr), sums=[R.sums(ps[l], pt[l], T0, p) for l in range(3)], n_valid=[ps[l]["n_valid"] for l in range(3)],
               pair=R.odometry(orc, frames[1], frames[0], intr, T0, **PARAMS), sequence=R.sequence(orc, frames, intr, **PARAMS))
    assert ref["pair"]["n_corr"] > 100 and all(r["n_corr"] > 100 for r in ref["sequence"][1][1:])
    return dict(frames=frames, intr=intr, T0=T0, ref=ref)


def held(tdv, ctx, case, what, env=None):
    """Every entry point against the restatement."""
    env = env or Env(ctx)
    frames, intr, T0, ref = case["frames"], case["intr"], case["T0"], case["ref"]
    got = device_maps(ctx, env, frames[0], intr)
    for k in ("vertex_map", "normal_map", "xyz", "normals"):
        assert got[k].tobytes() == ref["maps"][k].tobytes(), (what, k)
    d_src, d_tgt = env.up(frames[1]), env.up(frames[0])
    for l in range(3):
        s, n = ctx.depth_odometry_terms_dev(d_src, d_tgt, W, H, *intr, T0, l, **PARAMS)
        assert s.tobytes() == ref["sums"][l].tobytes() and n == ref["n_valid"][l], (what, "terms", l)
    same_result(ctx.depth_odometry_dev(d_src, d_tgt, W, H, *intr, T0, **PARAMS), ref["pair"], (what, "pair"))
    same_result(ctx.depth_odometry(frames[1], frames[0], intr, T0, **PARAMS), ref["pair"], (what, "host pair"))
    poses, pairs = ctx.depth_odometry_sequence_dev(env.up(frames), 4, W, H, *intr, **PARAMS)
    assert poses.tobytes() == ref["sequence"][0].tobytes(), (what, "sequence")
    for k in range(4):
        same_result(pairs[k], ref["sequence"][1][k], (what, "sequence", k))


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
    """A sequence of sixteen 640 x 480 planes (about 105 MB of pyramids) does not fit the first block of 64 MB; every pair of a plane seen
    twice has the identity as its answer to within the solver's rounding, and every interior pixel a partner."""
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")
        small = ctx.workspace_high_water()
        frames = np.full((16, 480, 640), 4000, np.uint16)
        poses, pairs = ctx.depth_odometry_sequence(frames, (10000.0, 500.0, 500.0, 319.5, 239.5), max_iterations=(2, 1, 1))
        assert ctx.workspace_high_water() > max(small, 64 << 20)
        assert all(p["n_corr"] == 639 * 479 for p in pairs[1:]) and np.abs(poses - np.eye(4, dtype=F)).max() < 1e-4
        held(tdv, ctx, case, "after the larger call")                    # the call that coalesces the blocks, and those after it
        held(tdv, ctx, case, "and again")
    finally:
        ctx.close()


def test_after_icp_with_every_switch_off_default_and_a_bad_argument_return(tdv, case, synth):
    ctx = tdv.Context(0)
    try:
        tgt, nrm = synth.sample_object(3000, 5)
        src, T_gt = synth.make_scene(3000, 5)
        ctx.set_icp_search("pruned"); ctx.set_icp_accumulation("tree"); ctx.set_icp_loss("tukey", 0.003); ctx.set_icp_launches("two")
        ctx.set_icp_probe_cache("off")
        ctx.icp(src, tgt, nrm, synth.perturb(T_gt), 0.004, 10, True)
        held(tdv, ctx, case, "after ICP with pruned search, a Tukey loss, two launches, no probe cache")
        ctx.set_icp_accumulation("reference"); ctx.set_icp_loss("l2"); ctx.set_icp_search("brute")
        ctx.icp(src, tgt, nrm, synth.perturb(T_gt), 0.004, 5, True)
        held(tdv, ctx, case, "after ICP with reference-order sums (and the switches still set)")
        env = Env(ctx)
        buffers = live_buffers(env)
        for which, kw in (("maps_dev", dict(capacity=-1)), ("terms", dict(level=2)), ("pair_dev", dict(n_levels=4)), ("sequence", dict(n_frames=-1))):
            o = Outputs()
            assert odom_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == -2 and o.untouched()
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
