"""TSDF ray casting, odometry against an f32 depth target and frame-to-model tracking on the device (include/tdv_hip.h:
tdv_tsdf_raycast_dev, csrc/tsdf_raycast.hip) against the restatement (tests/tsdf_raycast_restatement.py), byte for byte: the depth image,
the vertex map, the normal map and the hit count; the odometry's whole result; the tracked poses, results and the volume a tracked
sequence leaves.  Volumes: tests/tsdf_cases.py's small scene in 48 x 40 x 32 voxels, 65 x 33 x 17 (nx one above a run of 64) and sides of
1.  Images: 96 x 72, 67 x 35 (no multiple of the 8 x 8 tile or of 64), 1 x 1 and 0 x 0.  Both pose directions; a camera outside the
volume, inside it, looking away and behind the surface; NaN and infinite poses; a min_weight above every weight; max_steps 1 and a march
that cannot advance (bounded by the cap); every combination of NULL outputs; every bad argument on a live context.  Tracking is also held
to the composition of the public calls on the same context.  The accuracy condition is the restatement's (tests/test_tsdf_raycast_abi.py);
the device inherits it through byte equality and is given no tolerance of its own."""
import itertools

import numpy as np
import pytest

import odometry_cases as K
import odometry_restatement as Od
import tsdf_cases as Cs
import tsdf_raycast_restatement as R
import tsdf_restatement as Ts
from state_cases import Env
from test_gpu_odometry import frame, intrinsics, same_result
from test_gpu_tsdf import scene
from test_tsdf_raycast_abi import BAD, NULLS, Outputs, flipped, ray_call

pytestmark = pytest.mark.gpu
F = np.float32
NAN, INF = float("nan"), float("inf")
ZMAX = 0.5                                                                          # the scenes sit at 0.3 m: a miss ends after 113 samples
_FUSED = {}


def fused(dims, n_frames=3):
    """The small scene fused by the restatement (tests/test_gpu_tsdf.py holds the device's volume to it byte for byte), never modified."""
    key = (tuple(dims), n_frames)
    if key not in _FUSED:
        s = scene(dims, n_frames)
        buf, _ = Ts.integrate(s["vol"], Ts.reset(s["vol"]), s["frames"], s["poses"], s["intr"])
        buf.setflags(write=False)
        _FUSED[key] = dict(s, buf=buf)
    return _FUSED[key]


def camera_pose(view, direction):
    """A MODEL_TO_CAMERA view pose as the pose of `direction`."""
    return np.asarray(view, F) if direction == Ts.MODEL_TO_CAMERA else np.linalg.inv(np.asarray(view, np.float64)).astype(F)


def same_maps(got, ref, what, keys=("depth", "vertex_map", "normal_map")):
    for k in keys:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k)
        if got[k].tobytes() != ref[k].tobytes():
            bad = np.argwhere(got[k].view(np.uint32) != ref[k].view(np.uint32))
            first = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: %r, restated %r" % (what, k, len(bad), first, got[k][first], ref[k][first]))
    assert got["n_hit"] == ref["n_hit"] == int((ref["depth"] != 0).sum()), (what, got["n_hit"], ref["n_hit"])


def device_cast(tdv, ctx, env, vol, d_volume, pose, size, cam, **params):
    w, h = size
    npx = w * h
    dd, vm, nm = env.out(npx, F), env.out(3 * npx, F), env.out(3 * npx, F)
    n = ctx.tsdf_raycast_dev(tdv.tsdf_volume_struct(*vol.args()), d_volume, pose, w, h, *cam, dd.data_ptr(), vm.data_ptr(), nm.data_ptr(), **params)
    return dict(depth=env.get(dd, npx, F).reshape(h, w), vertex_map=env.get(vm, 3 * npx, F).reshape(h, w, 3),
                normal_map=env.get(nm, 3 * npx, F).reshape(h, w, 3), n_hit=n)


def held(tdv, ctx, vol, buf, pose, size, cam, what, **params):
    ref = R.raycast(vol, buf, pose, size, cam, **params)
    env = Env(ctx)
    same_maps(device_cast(tdv, ctx, env, vol, env.up(buf), pose, size, cam, **params), ref, what)
    return ref


# ---------------------------------------------------------------- volumes, images, directions
VOLUMES = [(48, 40, 32), (65, 33, 17)]
IMAGES = {(96, 72): 230.0, (67, 35): 150.0}


@pytest.mark.parametrize("dims", VOLUMES, ids=["%dx%dx%d" % d for d in VOLUMES])
@pytest.mark.parametrize("size", sorted(IMAGES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("direction", [Ts.MODEL_TO_CAMERA, Ts.SOURCE_ONTO_TARGET], ids=["model_to_camera", "source_onto_target"])
def test_views_of_the_small_scene(tdv, ctx, dims, size, direction):
    """The scan pose and a tilted view, in the frames' own camera and in one of another size."""
    s = fused(dims)
    f = IMAGES[size]
    cam = (f, 1.05 * f, (size[0] - 1) / 2.0, (size[1] - 1) / 2.0 + 0.25)
    for k in (0, 2):
        ref = held(tdv, ctx, s["vol"], s["buf"], camera_pose(s["poses"][k], direction), size, cam, (dims, size, direction, k), zmax=ZMAX,
                   pose_direction=direction)
        assert ref["n_hit"] > 150 and ((ref["normal_map"] != 0).any(-1).sum() > 100), (ref["n_hit"], k)
        assert (ref["normal_map"][..., 2][ref["depth"] > 0] <= 0).all()              # towards the camera: O3's sign


def test_sides_of_one_and_tiny_images(tdv, ctx):
    """A side of 1 has no known sample; 1 x 1 and 0 x 0 images are valid."""
    for dims in ((1, 33, 17), (33, 1, 17), (33, 17, 1), (1, 1, 1)):
        s = fused(dims, 2)
        ref = held(tdv, ctx, s["vol"], s["buf"], s["poses"][0], (67, 35), (150.0, 150.0, 33.0, 17.0), dims, zmax=ZMAX)
        assert ref["n_hit"] == 0 and not ref["depth"].any()
    s = fused((48, 40, 32))
    centre = held(tdv, ctx, s["vol"], s["buf"], s["poses"][0], (1, 1), (230.0, 230.0, 0.0, 0.0), "1x1", zmax=ZMAX)
    assert centre["n_hit"] == 1
    env = Env(ctx)
    guard = env.out(4, F)
    n = ctx.tsdf_raycast_dev(tdv.tsdf_volume_struct(*s["vol"].args()), env.up(s["buf"]), s["poses"][0], 0, 0, 230.0, 230.0, 0.0, 0.0, guard.data_ptr(),
                             guard.data_ptr(), guard.data_ptr(), zmax=ZMAX)
    assert n == 0 and env.get(guard, 4, np.uint32).tolist() == [0xA5A5A5A5] * 4
    for size in ((0, 5), (5, 0)):
        assert ctx.tsdf_raycast_dev(tdv.tsdf_volume_struct(*s["vol"].args()), env.up(s["buf"]), s["poses"][0], *size, 230.0, 230.0, 0.0, 0.0,
                                    guard.data_ptr(), None, None, zmax=ZMAX) == 0
    assert env.get(guard, 4, np.uint32).tolist() == [0xA5A5A5A5] * 4


def test_cameras(tdv, ctx):
    """Outside the volume (the views above), inside it, looking away, and behind the surface."""
    s = fused((48, 40, 32))
    vol, buf, intr = s["vol"], s["buf"], s["intr"]
    size, cam = (96, 72), intr[1:]
    near = flipped(0.02)                                                           # 20 mm above the plate, looking down: under the grid's top at 22.4 mm
    ref = held(tdv, ctx, vol, buf, near, size, cam, "inside the volume", zmax=ZMAX, zmin=0.001)
    assert ref["n_hit"] > 500
    away = np.eye(4, dtype=F); away[2, 3] = -0.3                                   # where the scan pose stands, looking up and away
    ref = held(tdv, ctx, vol, buf, away, size, cam, "looking away", zmax=ZMAX)
    assert ref["n_hit"] == 0
    behind = np.eye(4, dtype=F); behind[2, 3] = 0.3                                # 0.3 m below the plate, looking up at its back
    ref = held(tdv, ctx, vol, buf, behind, size, cam, "a back face", zmax=ZMAX)
    assert ref["n_hit"] == 0
    assert (ref["samples"] < 100).sum() > 500, "no ray of the back view reached known, negative field: the case shows nothing"
    inside = np.eye(4, dtype=F); inside[2, 3] = 0.002                              # the camera 2 mm under the plate's base plane, looking up
    ref = held(tdv, ctx, vol, buf, inside, size, cam, "inside the surface", zmax=ZMAX, zmin=0.0005)
    assert ref["n_hit"] == 0 and (ref["samples"] == 1).sum() > 500


def test_unusable_poses_and_weights(tdv, ctx):
    s = fused((48, 40, 32))
    vol, buf, cam = s["vol"], s["buf"], s["intr"][1:]
    view = s["poses"][0]
    cases = {"a pose of NaNs": np.full((4, 4), NAN, F), "a NaN in the rotation": view * np.array([1, NAN, 1, 1], F),
             "an infinite translation": view + np.array([[0, 0, 0, INF]] * 3 + [[0, 0, 0, 0]], F),
             "an infinite rotation entry": view + np.array([[0, INF, 0, 0]] + [[0, 0, 0, 0]] * 3, F)}
    for what, pose in cases.items():
        for direction in (Ts.MODEL_TO_CAMERA, Ts.SOURCE_ONTO_TARGET):
            ref = held(tdv, ctx, vol, buf, pose, (67, 35), cam, (what, direction), zmax=ZMAX, pose_direction=direction)
            assert ref["n_hit"] == 0, (what, direction)
    assert buf[..., 1].max() == 3
    ref = held(tdv, ctx, vol, buf, view, (96, 72), cam, "min_weight above every weight", zmax=ZMAX, min_weight=4.0)
    assert ref["n_hit"] == 0
    seen = held(tdv, ctx, vol, buf, view, (96, 72), cam, "min_weight 3", zmax=ZMAX, min_weight=3.0)
    assert 0 < seen["n_hit"] < held(tdv, ctx, vol, buf, view, (96, 72), cam, "min_weight 1", zmax=ZMAX)["n_hit"]
    held(tdv, ctx, vol, buf, view, (96, 72), cam, "a trunc of its own, zmax inside the scene", zmax=0.3, trunc=0.0025)
    poisoned = buf.copy()                                                          # NaN and infinite voxels: no sample there, no fault
    poisoned[10:14, 10:30, 10:40, 0] = NAN
    poisoned[16:18, 10:30, 10:40, 1] = NAN
    poisoned[4:6, 5:9, 5:9, 0] = INF
    ref = held(tdv, ctx, vol, poisoned, view, (96, 72), cam, "NaN and infinite voxels", zmax=ZMAX)
    assert np.isfinite(ref["depth"]).all() and np.isfinite(ref["normal_map"]).all()


def test_the_step_cap(tdv, ctx):
    s = fused((48, 40, 32))
    ref = held(tdv, ctx, s["vol"], s["buf"], s["poses"][0], (67, 35), s["intr"][1:], "max_steps 1", zmax=ZMAX, max_steps=1)
    assert ref["n_hit"] == 0
    few = held(tdv, ctx, s["vol"], s["buf"], s["poses"][0], (96, 72), s["intr"][1:], "max_steps 64", zmax=ZMAX, max_steps=64)      # the hits take 62 to 66 samples
    assert 0 < few["n_hit"] < held(tdv, ctx, s["vol"], s["buf"], s["poses"][0], (96, 72), s["intr"][1:], "max_steps 4096", zmax=ZMAX)["n_hit"]
    tiny = Ts.Volume((0.0, 0.0, 0.0), 1e-10, (4, 4, 4))                            # z + stride == z: 16,384 samples per ray, then the cap
    ref = held(tdv, ctx, tiny, Ts.reset(tiny), np.eye(4, dtype=F), (4, 4), (10.0, 10.0, 1.5, 1.5), "a march that cannot advance",
               max_steps=R.MAX_STEPS_CAP)
    assert ref["n_hit"] == 0 and ref["capped"].all()


def test_every_combination_of_outputs(tdv, ctx):
    s = fused((48, 40, 32))
    vol, size, cam, pose = s["vol"], (67, 35), s["intr"][1:], s["poses"][2]
    ref = R.raycast(vol, s["buf"], pose, size, cam, zmax=ZMAX)
    cvol = tdv.tsdf_volume_struct(*vol.args())
    env = Env(ctx)
    d_volume = env.up(s["buf"])
    npx = size[0] * size[1]
    pattern = np.full(1, 0xA5A5A5A5, np.uint32).view(F)[0].tobytes()
    for want in itertools.product((False, True), repeat=4):
        bufs = [env.out(npx, F), env.out(3 * npx, F), env.out(3 * npx, F)]
        n = ctx.tsdf_raycast_dev(cvol, d_volume, pose, *size, *cam, *[b.data_ptr() if w else None for b, w in zip(bufs, want)], want_count=want[3],
                                 zmax=ZMAX)
        assert n == (ref["n_hit"] if want[3] else None), want
        for b, w, k, m in zip(bufs, want, ("depth", "vertex_map", "normal_map"), (1, 3, 3)):
            got = env.get(b, m * npx, F).tobytes()
            assert got == (ref[k].tobytes() if w else pattern * (m * npx)), (want, k)
    host = ctx.tsdf_raycast((vol.args(), s["buf"]), pose, *size, *cam, zmax=ZMAX)
    same_maps(host, ref, "host form")
    only = ctx.tsdf_raycast((cvol, s["buf"]), pose, *size, *cam, maps=False, zmax=ZMAX)
    assert only["depth"].tobytes() == ref["depth"].tobytes() and only["n_hit"] == ref["n_hit"] and "vertex_map" not in only


# ---------------------------------------------------------------- odometry against an f32 target
OD_KW = dict(depth_diff=K.ACCURACY_DEPTH_DIFF, max_iterations=(6, 4, 3))


def check_to_depth(ctx, orc, src, depth, intr, what, T0=None, host=True, **kw):
    h, w = src.shape
    ref = R.odometry_to_depth(orc, src, depth, intr, T0, **kw)
    env = Env(ctx)
    same_result(ctx.depth_odometry_to_depth_dev(env.up(src), env.up(depth), w, h, *intr, T0, **kw), ref, (what, "dev"))
    if host:
        same_result(ctx.depth_odometry_to_depth(src, depth, intr, T0, **kw), ref, (what, "host"))
    return ref


def test_odometry_to_depth(tdv, ctx, orc):
    c = K.pair((96, 72), 2.0)
    src, tgt, intr = c["src"], c["tgt"], c["intr"]
    z = Od.depth0(tgt, intr[0], 10.0)
    ref = check_to_depth(ctx, orc, src, z, intr, "O1's depth of the raw target", **OD_KW)
    assert ref["n_corr"] > 500 and sum(ref["iterations"]) > 3
    env = Env(ctx)
    same_result(ctx.depth_odometry_dev(env.up(src), env.up(tgt), 96, 72, *intr, **OD_KW), ref, "the raw-frame entry point on the same pair")
    bad = z.copy()                                                                 # O10: NaN, negative, infinite and above-zmax pixels
    rng = np.random.default_rng(11)
    valid = np.argwhere(z > 0)
    pick = valid[rng.choice(len(valid), 240, replace=False)]
    for k, v in enumerate((NAN, -0.3, INF, -INF, 0.3004, 11.0)):
        rows = pick[40 * k:40 * (k + 1)]
        bad[rows[:, 0], rows[:, 1]] = v
    cut = check_to_depth(ctx, orc, src, bad, intr, "unusable pixels", zmax=0.3003, **OD_KW)
    cleaned = R.depth0_f32(bad, 0.3003)
    assert (cleaned[pick[:, 0], pick[:, 1]] == 0).all() and cut["n_corr"] > 100
    same_result(ctx.depth_odometry_to_depth(src, cleaned, intr, zmax=0.3003, **OD_KW), cut, "the same image cleaned by hand")
    check_to_depth(ctx, orc, src, z, intr, "a start pose, one level", c["T_gt"].astype(F), host=False, n_levels=1, max_iterations=(3,), depth_diff=0.004)
    for shape in ((33, 17), (65, 47), (1, 1)):
        w, h = shape
        s, t, i = frame(w, h, 1), frame(w, h, 0), intrinsics(w, h)
        levels = 3 if min(shape) > 8 else 1
        check_to_depth(ctx, orc, s, Od.depth0(t, i[0], 10.0), i, shape, n_levels=levels, max_iterations=(4, 3, 2))
    none = ctx.depth_odometry_to_depth_dev(None, None, 0, 0, *intr)
    assert none["T"].tobytes() == np.eye(4, dtype=F).tobytes() and none["n_corr"] == 0


# ---------------------------------------------------------------- tracking
TRACK_DIMS, TRACK_FRAMES = (48, 40, 32), 5
TRACK_KW = dict(tsdf=dict(zmax=ZMAX), odom=OD_KW)


@pytest.fixture(scope="module")
def tracked(orc):
    """Five views, a degree apart, and the restatement of everything the tracking tests compare with (computed once, never modified)."""
    s = K.sequence((96, 72), TRACK_FRAMES)
    poses = np.stack([np.linalg.inv(P.astype(np.float64)) for P in s["poses"]]).astype(F)
    vol = Cs.small_scene(TRACK_DIMS, 0)["vol"]
    n = TRACK_FRAMES
    buf, _ = Ts.integrate(vol, Ts.reset(vol), s["frames"][:n - 1], poses[:n - 1], s["intr"], pose_direction=Ts.SOURCE_ONTO_TARGET)
    one = R.track(orc, vol, buf, s["frames"][n - 1], poses[n - 2], s["intr"], **TRACK_KW)
    seq = R.track_sequence(orc, vol, Ts.reset(vol), s["frames"], s["intr"], poses[0], **TRACK_KW)
    return dict(s=s, poses=poses, vol=vol, buf=buf, one=one, seq=seq)


def same_track(got, ref, what):
    assert got["pose"].tobytes() == np.asarray(ref["pose"], F).tobytes(), (what, got["pose"], ref["pose"])
    assert got["n_hit"] == ref["n_hit"], (what, got["n_hit"], ref["n_hit"])
    same_result(got["odom"], ref["odom"], what)


def test_track(tdv, ctx, tracked):
    t, n = tracked, TRACK_FRAMES
    s, vol, intr = t["s"], t["vol"], t["s"]["intr"]
    cvol = tdv.tsdf_volume_struct(*vol.args())
    env = Env(ctx)
    d_volume, d_raw, guess = env.up(t["buf"]), env.up(s["frames"][n - 1]), t["poses"][n - 2]
    got = ctx.tsdf_track_dev(cvol, d_volume, d_raw, guess, 96, 72, *intr, **TRACK_KW)
    same_track(got, t["one"], "against the restatement")
    assert got["n_hit"] > 500 and got["odom"]["n_corr"] > 500
    # K1 to K3 by the public calls on the same context
    dd = env.out(96 * 72, F)
    n_hit = ctx.tsdf_raycast_dev(cvol, d_volume, guess, 96, 72, *intr[1:], dd.data_ptr(), zmax=ZMAX, pose_direction=Ts.SOURCE_ONTO_TARGET)
    odom = ctx.depth_odometry_to_depth_dev(d_raw, dd.data_ptr(), 96, 72, *intr, **OD_KW)
    same_track(got, dict(pose=R.product(guess, odom["T"]), odom=odom, n_hit=n_hit), "against the public calls")
    assert env.get(dd, 96 * 72, F).tobytes() == t["one"]["depth"].tobytes()
    empty = ctx.tsdf_track_dev(cvol, d_volume, None, guess, 0, 0, *intr, **TRACK_KW)
    assert empty["pose"].tobytes() == R.product(guess, np.eye(4, dtype=F)).tobytes() and empty["n_hit"] == 0 and empty["odom"]["n_corr"] == 0
    nothing = ctx.tsdf_track_dev(cvol, env.up(Ts.reset(vol)), d_raw, guess, 96, 72, *intr, **TRACK_KW)          # an empty volume: the guess
    assert nothing["pose"].tobytes() == R.product(guess, np.eye(4, dtype=F)).tobytes() and nothing["n_hit"] == 0


@pytest.mark.parametrize("n_frames", [0, 1, TRACK_FRAMES])
def test_track_sequence(tdv, ctx, orc, tracked, n_frames):
    t = tracked
    s, vol, intr = t["s"], t["vol"], t["s"]["intr"]
    cvol = tdv.tsdf_volume_struct(*vol.args())
    frames = s["frames"][:n_frames]
    if n_frames == TRACK_FRAMES:
        ref_poses, ref_res, ref_buf = t["seq"]
    else:
        ref_poses, ref_res, ref_buf = R.track_sequence(orc, vol, Ts.reset(vol), frames, intr, t["poses"][0], **TRACK_KW)
    env = Env(ctx)
    d_volume, d_raw = env.up(Ts.reset(vol)), env.up(frames)
    poses, res = ctx.tsdf_track_sequence_dev(cvol, d_volume, d_raw, n_frames, 96, 72, *intr, pose0=t["poses"][0], **TRACK_KW)
    assert poses.tobytes() == ref_poses.tobytes() and len(res) == n_frames
    for k in range(n_frames):
        same_track(res[k], ref_res[k], ("frame", k))
    volume = env.get(env.keep[-2], vol.voxels * 2, F)
    assert volume.tobytes() == ref_buf.tobytes()
    if n_frames < 2:
        return
    assert all(r["odom"]["n_corr"] > 500 for r in res[1:])
    # ... and the loop over the public calls on the same context
    d_loop = env.up(Ts.reset(vol))
    P = [t["poses"][0]]
    tsdf_kw = dict(TRACK_KW["tsdf"], pose_direction=Ts.SOURCE_ONTO_TARGET)
    for k in range(n_frames):
        d_frame = env.up(frames[k])
        if k:
            one = ctx.tsdf_track_dev(cvol, d_loop, d_frame, P[-1], 96, 72, *intr, **TRACK_KW)
            same_track(res[k], one, ("single call", k))
            P.append(one["pose"])
        ctx.tsdf_integrate_dev(cvol, d_loop, d_frame, P[-1][None], 96, 72, *intr, want_counts=False, **tsdf_kw)
    assert env.get(env.keep[-1 - n_frames], vol.voxels * 2, F).tobytes() == volume.tobytes()
    host_vol = ctx.tsdf_volume(*vol.args())
    host_poses, _ = ctx.tsdf_track_sequence(host_vol, frames, intr, pose0=t["poses"][0], **TRACK_KW)
    assert host_poses.tobytes() == ref_poses.tobytes()
    identity_start, _ = ctx.tsdf_track_sequence(ctx.tsdf_volume(*vol.args()), frames[:1], intr, **TRACK_KW)
    assert identity_start.tobytes() == np.eye(4, dtype=F)[None].tobytes()


# ---------------------------------------------------------------- arguments
def live_buffers(env):
    return dict(volume=env.out(4 * 3 * 2 * 2, F).data_ptr(), frames=env.up(np.full(65 * 8 * 6, 3000, np.uint16)), target=env.up(np.full(48, 0.3, F)),
                depth=env.out(48, F).data_ptr(), vm=env.out(144, F).data_ptr(), nm=env.out(144, F).data_ptr())


def test_bad_arguments_on_a_live_context(tdv, ctx):
    env = Env(ctx)
    buffers = live_buffers(env)
    ctx.tsdf_reset_dev(tdv.tsdf_volume_struct((0.0, 0.0, 0.3), 0.001, (4, 3, 2)), buffers["volume"])
    o = Outputs()
    for what, kw, where in BAD[1:]:
        for which in where:
            assert ray_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == -2, (what, which)
    for name, where in NULLS.items():
        for which in where:
            assert ray_call(tdv, which, ctx._h, o, null=(name,), buffers=buffers) == -2, (name, which)
    assert o.untouched()
    # ... and the same arguments unspoilt are accepted, with width * height == 0 and with no frame too
    for which in ("raycast_dev", "raycast", "to_depth_dev", "to_depth", "track", "sequence"):
        host = Outputs()
        host.volume[:] = np.tile(np.array([1, 0], F), 24)
        assert ray_call(tdv, which, ctx._h, host, buffers=buffers) == 0, which
        assert ray_call(tdv, which, ctx._h, host, buffers=buffers, width=0) == 0, which
    assert ray_call(tdv, "sequence", ctx._h, Outputs(), buffers=buffers, n_frames=0) == 0
