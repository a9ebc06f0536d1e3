"""CPU suite: TSDF ray casting, odometry against an f32 depth target and frame-to-model tracking (include/tdv_hip.h: tdv_tsdf_raycast_dev).
The ABI exports the entry points, lists them in ABI_SYMBOLS, has the documented struct layouts, constants and defaults, states rules T13
to T18, O10 and K1 to K3, no longer lists ray casting or frame-to-model tracking as not provided, and refuses every bad argument before
it writes anything.  Then the restatement (tests/tsdf_raycast_restatement.py) is held to what the rules promise: a front-on plane is hit
where it is with normals (0, 0, -1), a camera behind the surface hits nothing, the step cap ends a march that cannot advance, O10 drops
what it names, and tracking the last frame of a sequence against the volume fused from the frames before meets the odometry's accuracy
condition.  No compute entry point of the library runs here; tests/test_gpu_tsdf_raycast.py holds the device to this restatement byte
for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import odometry_cases as K
import odometry_restatement as Od
import tsdf_cases as Cs
import tsdf_raycast_restatement as R
import tsdf_restatement as Ts

TDV_ERR_BAD_ARG = -2
F = np.float32
NAN, INF = float("nan"), float("inf")
SYMBOLS = ("tdv_tsdf_raycast_default_params", "tdv_tsdf_raycast_dev", "tdv_tsdf_raycast", "tdv_depth_odometry_to_depth_dev",
           "tdv_depth_odometry_to_depth", "tdv_tsdf_track_dev", "tdv_tsdf_track_sequence_dev")
MAX_SIDE, MAX_FRAMES = 8192, 64


def test_symbols_constants_structs_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.TsdfRaycastParamsC) == 8
    assert [(k, getattr(tdv.TsdfRaycastParamsC, k).offset) for k, _ in tdv.TsdfRaycastParamsC._fields_] == [("zmin", 0), ("max_steps", 4)]
    assert C.sizeof(tdv.TsdfTrackResultC) == 184
    assert [(k, getattr(tdv.TsdfTrackResultC, k).offset) for k, _ in tdv.TsdfTrackResultC._fields_] == [("pose", 0), ("odom", 64), ("n_hit", 176)]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdv_hip.h")).read()
    text = header.split("#define TDV_TSDF_RAYCAST_MAX_STEPS ")[1].split("/*")[0].split("\n")[0].strip()
    assert eval(text) == tdv.TDV_TSDF_RAYCAST_MAX_STEPS == R.MAX_STEPS_CAP == 16384
    for rule in ("T13.", "T14.", "T15.", "T16.", "T17.", "T18.", "O10.", "K1.", "K2.", "K3."):
        assert " %s " % rule in header, rule
    for s in SYMBOLS:
        assert s + "(" in header, s
    for section in ("/* TSDF fusion", "/* Depth odometry"):                       # neither list names them as missing any more
        missing = header.split(section)[1].split("Not provided:")[1].split("*/")[0].split(".")[0]
        assert "ray casting" not in missing and "frame-to-model" not in missing, (section, missing)
    p = tdv.raycast_params()
    assert (p.zmin, p.max_steps) == (F(0.05), 4096) == (F(R.DEFAULTS["zmin"]), R.DEFAULTS["max_steps"])
    lib.tdv_tsdf_raycast_default_params(None)                                      # a NULL is ignored
    q = tdv.raycast_params(zmin=0.2, max_steps=7)
    assert (q.zmin, q.max_steps) == (F(0.2), 7) and tdv.Context.raycast_params(max_steps=3).max_steps == 3
    with pytest.raises(TypeError):
        tdv.raycast_params(steps=1)
    for name in ("tsdf_raycast", "tsdf_raycast_dev", "depth_odometry_to_depth", "depth_odometry_to_depth_dev", "tsdf_track", "tsdf_track_dev",
                 "tsdf_track_sequence", "tsdf_track_sequence_dev"):
        assert callable(getattr(tdv.Context, name)), name


# ---------------------------------------------------------------- arguments
GOOD = dict(voxel_length=0.001, nx=4, ny=3, nz=2, width=8, height=6, scale=1000.0, fx=10.0, fy=10.0, trunc=0.0, max_weight=255.0, zmax=10.0,
            min_weight=1.0, pose_direction=Ts.SOURCE_ONTO_TARGET, zmin=0.05, max_steps=64, depth_diff=0.03, odom_zmax=10.0, n_levels=2,
            max_iterations=(2, 2, 0, 0), n_frames=3)
CAST, TO_DEPTH, TRACK, SEQ = ("raycast_dev", "raycast"), ("to_depth_dev", "to_depth"), ("track", "sequence"), ("sequence",)
VOLUME, ODOM, ALL = CAST + TRACK, TO_DEPTH + TRACK, CAST + TO_DEPTH + TRACK
BAD = [("null ctx", {}, ALL)]
BAD += [("%s %r" % (k, v), {k: v}, VOLUME) for k in ("nx", "ny", "nz") for v in (0, -1, Ts.MAX_SIDE + 1)]
BAD += [("voxels above the cap", dict(nx=1024, ny=1024, nz=129), VOLUME), ("voxels above the host cap", dict(nx=1024, ny=1024, nz=33), ("raycast",))]
BAD += [("voxel_length %r" % v, dict(voxel_length=v), VOLUME) for v in (0.0, -0.001, NAN, INF)]
BAD += [("%s %r" % (k, v), {k: v}, ALL) for k in ("width", "height") for v in (-1, MAX_SIDE + 1)]
BAD += [("%s %r" % (k, v), {k: v}, ALL) for k in ("fx", "fy") for v in (0.0, -1.0, NAN, INF)]
BAD += [("scale %r" % v, dict(scale=v), ODOM) for v in (0.0, -1.0, NAN, INF)]
BAD += [("trunc %r" % v, dict(trunc=v), VOLUME) for v in (-0.001, NAN, INF)]
BAD += [("max_weight %r" % v, dict(max_weight=v), VOLUME) for v in (0.5, 0.0, NAN, INF)]
BAD += [("min_weight %r" % v, dict(min_weight=v), VOLUME) for v in (0.0, -1.0, NAN, INF)]
BAD += [("pose_direction %r" % v, dict(pose_direction=v), VOLUME) for v in (2, -1)]
BAD += [("tracking with model-to-camera poses", dict(pose_direction=Ts.MODEL_TO_CAMERA), TRACK)]
BAD += [("zmin %r" % v, dict(zmin=v), VOLUME) for v in (0.0, -0.05, NAN, INF, -INF)]
BAD += [("max_steps %r" % v, dict(max_steps=v), VOLUME) for v in (0, -1, R.MAX_STEPS_CAP + 1)]
BAD += [("%s %r" % (k, v), {k: v}, ODOM) for k in ("depth_diff", "odom_zmax") for v in (0.0, -1.0, NAN, INF)]
BAD += [("n_levels %r" % v, dict(n_levels=v), ODOM) for v in (0, -1, 5)]
BAD += [("a level with a side of 0", dict(n_levels=4), ODOM)]
BAD += [("max_iterations %r" % (v,), dict(max_iterations=v), ODOM) for v in ((-1, 0, 0, 0), (1, 1, 1, -5))]
BAD += [("n_frames %r" % v, dict(n_frames=v), SEQ) for v in (-1, MAX_FRAMES + 1)]
NULLS = {"vol": VOLUME, "volume": VOLUME, "tsdf_params": VOLUME, "ray_params": VOLUME, "odom_params": ODOM, "pose": CAST + ("track",),
         "frames": ODOM, "target": TO_DEPTH, "result": TO_DEPTH + ("track",), "poses": SEQ}


class Outputs:
    """Host arrays in every slot a call writes (a refused call must not look at them), filled with a pattern; untouched() compares."""

    def __init__(self):
        self.depth = np.full(48, -7, F); self.vm = np.full((48, 3), -7, F); self.nm = np.full((48, 3), -7, F)
        self.n_hit = np.full(1, -7, np.int64); self.volume = np.full(4 * 3 * 2 * 2, -7, F)
        self.result = np.full(46 * (MAX_FRAMES + 2), -7, np.int32); self.poses = np.full(16 * (MAX_FRAMES + 2), -7, F)
        self.before = self.snapshot()

    def arrays(self):
        return self.depth, self.vm, self.nm, self.n_hit, self.volume, self.result, self.poses

    def snapshot(self):
        return tuple(a.tobytes() for a in self.arrays())

    def untouched(self):
        return self.snapshot() == self.before


def P(x):
    return None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))


def ray_call(tdv, which, ctx, o, null=(), buffers=None, **kw):
    """One entry point on GOOD's arguments with kw replaced and the pointers named in `null` NULL.  buffers (the GPU suite): device
    pointers for volume, frames, target, depth, vm, nm in place of the host arrays (the device forms)."""
    g = dict(GOOD, **kw)
    lib = tdv.lib()
    dev = which != "raycast" and which != "to_depth"
    b = (buffers or {}) if dev else {}
    vol = tdv.TsdfVolumeC((C.c_float * 3)(0.0, 0.0, 0.3), g["voxel_length"], g["nx"], g["ny"], g["nz"])
    tp = tdv.TsdfParamsC(g["trunc"], g["max_weight"], g["zmax"], g["min_weight"], g["pose_direction"])
    rp = tdv.TsdfRaycastParamsC(g["zmin"], g["max_steps"])
    op = tdv.OdometryParamsC(g["depth_diff"], g["odom_zmax"], g["n_levels"], (C.c_int * 4)(*g["max_iterations"]))
    raw = np.full((MAX_FRAMES + 1) * 8 * 6, 3000, np.uint16)
    target = np.full(8 * 6, 0.3, F)
    pose = np.eye(4, dtype=F).reshape(-1)
    pv, ptp, prp, pop = (None if n in null else C.byref(s) for n, s in (("vol", vol), ("tsdf_params", tp), ("ray_params", rp), ("odom_params", op)))
    volume = None if "volume" in null else P(b.get("volume", o.volume))
    frames = None if "frames" in null else P(b.get("frames", raw))
    hp = None if "pose" in null else P(pose)
    res = None if "result" in null else P(o.result)
    wh = (g["width"], g["height"])
    f4 = (C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(3.5), C.c_float(2.5))
    if which in CAST:
        fn = lib.tdv_tsdf_raycast_dev if dev else lib.tdv_tsdf_raycast
        return fn(ctx, pv, volume, *wh, *f4, hp, ptp, prp, P(b.get("depth", o.depth)), P(b.get("vm", o.vm)), P(b.get("nm", o.nm)), P(o.n_hit))
    if which in TO_DEPTH:
        fn = lib.tdv_depth_odometry_to_depth_dev if dev else lib.tdv_depth_odometry_to_depth
        return fn(ctx, frames, None if "target" in null else P(b.get("target", target)), *wh, C.c_float(g["scale"]), *f4, P(pose), pop, res)
    if which == "track":
        return lib.tdv_tsdf_track_dev(ctx, pv, volume, frames, *wh, C.c_float(g["scale"]), *f4, hp, ptp, prp, pop, res)
    return lib.tdv_tsdf_track_sequence_dev(ctx, pv, volume, frames, g["n_frames"], *wh, C.c_float(g["scale"]), *f4, None, ptp, prp, pop,
                                           None if "poses" in null else P(o.poses), P(o.result))


@pytest.mark.parametrize("case", range(len(BAD)), ids=[b[0] for b in BAD])
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_tsdf_raycast.py refuses each bad argument on one."""
    o = Outputs()
    what, kw, where = BAD[case]
    for which in where:
        assert ray_call(tdv, which, None, o, **kw) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


def test_null_pointers_leave_outputs_untouched(tdv):
    o = Outputs()
    for name, where in NULLS.items():
        for which in where:
            assert ray_call(tdv, which, None, o, null=(name,)) == TDV_ERR_BAD_ARG, (name, which)
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against what the rules promise
PLANE_VOL = Ts.Volume((-0.009, -0.007, 0.39), 0.002, (9, 7, 12))
PLANE_D = 0.40625                                                                 # 13 / 32 m: exactly representable, between the layers at 0.405 and 0.407
PLANE_INTR = (8192.0, 500.0, 500.0, 31.5, 23.5)                                    # scale 2^13: raw 3328 is 0.40625 m exactly
PLANE_SIZE = (64, 48)


@pytest.fixture(scope="module")
def plane():
    frames = np.full((1, PLANE_SIZE[1], PLANE_SIZE[0]), 3328, np.uint16)
    buf, _ = Ts.integrate(PLANE_VOL, Ts.reset(PLANE_VOL), frames, np.eye(4, dtype=F)[None], PLANE_INTR)
    return buf


def test_front_on_plane(plane):
    """(a) One frame of a plane at d = 13/32 m under the identity, ray cast from the identity with zmax 0.5.  The projective sdf of one
    front-on view is linear in z and constant in x and y, so the trilinear sample is the field itself and T16's one interpolation lands on
    d up to f32 rounding - about 1e-7 of d, a few 1e-8 m; the bound voxel_length / 1024 = 2e-6 m is some fifty times that.  The gradient
    has only a z component, so the normal is (0, 0, -1)."""
    vol = PLANE_VOL
    assert F(3328) * F(1.0 / 8192.0) == F(PLANE_D) and float(F(PLANE_D)) == PLANE_D
    for direction in (Ts.MODEL_TO_CAMERA, Ts.SOURCE_ONTO_TARGET):
        c = R.raycast(vol, plane, np.eye(4, dtype=F), PLANE_SIZE, PLANE_INTR[1:], zmax=0.5, pose_direction=direction)
        hit = c["depth"] > 0
        assert c["n_hit"] == hit.sum() > 200
        err = np.abs(c["depth"][hit].astype(np.float64) - PLANE_D).max()
        nm = c["normal_map"][hit]
        has = (nm != 0).any(-1)
        nerr = np.abs(nm[has].astype(np.float64) - np.array([0.0, 0.0, -1.0])).max()
        print("plane (direction %d): %d hits, largest |z - d| = %.3e m (bound %.3e), %d normals, largest deviation %.1e" %
              (direction, c["n_hit"], err, float(vol.L) / 1024, has.sum(), nerr))
        assert err <= float(vol.L) / 1024
        assert has.sum() > 100 and nerr <= 1e-5
        vm = c["vertex_map"]
        assert vm[..., 2].tobytes() == c["depth"].tobytes() and not vm[~hit].any() and not c["normal_map"][~hit].any()
        # a ray that hits stays inside the volume's known region from its first known sample: no hit outside the frustum of the grid
        u0 = np.nonzero(hit.any(0))[0]
        assert 0 < u0.min() and u0.max() < PLANE_SIZE[0] - 1


def flipped(z):
    """A camera at depth z on the optical axis looking back along -z (turned about y by pi): model-to-camera."""
    T = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(F)
    T[2, 3] = z
    return T


def test_back_face_gives_no_hit(plane):
    """(b) From behind the plane the field goes from unknown (never seen) or negative to positive: T15 ends such a ray without a hit."""
    c = R.raycast(PLANE_VOL, plane, flipped(0.8), PLANE_SIZE, PLANE_INTR[1:], zmax=0.5)
    assert c["n_hit"] == 0 and not c["depth"].any() and not c["vertex_map"].any() and not c["normal_map"].any()
    known = R.sample(PLANE_VOL, plane, 1.0, tuple(np.array([x], F) for x in (0.0, 0.0, 0.408)))
    assert known[0][0] and known[1][0] < 0                                         # ... and the rays did cross known, negative field
    inside = np.eye(4, dtype=F); inside[2, 3] = -0.409                             # a camera inside the surface, looking on: negative at once
    c = R.raycast(PLANE_VOL, plane, inside, PLANE_SIZE, PLANE_INTR[1:], zmax=0.5, zmin=0.001)
    assert c["n_hit"] == 0


def test_the_step_cap_ends_a_march(plane):
    """(c) max_steps 1: one sample, never a hit (a hit needs sample k-1).  A voxel_length below an ulp of z under a trunc of the same size:
    z + stride == z, the march cannot advance and ends at the cap."""
    c = R.raycast(PLANE_VOL, plane, np.eye(4, dtype=F), PLANE_SIZE, PLANE_INTR[1:], zmax=0.5, max_steps=1)
    assert c["n_hit"] == 0 and (c["samples"] == 1).all() and c["capped"].all()
    tiny = Ts.Volume((0.0, 0.0, 0.0), 1e-10, (4, 4, 4))
    assert F(0.05) + F(4.0) * tiny.L == F(0.05)
    c = R.raycast(tiny, Ts.reset(tiny), np.eye(4, dtype=F), (4, 4), (10.0, 10.0, 1.5, 1.5), max_steps=R.MAX_STEPS_CAP)
    assert c["n_hit"] == 0 and c["capped"].all() and (c["samples"] == R.MAX_STEPS_CAP).all() and not c["far"].any()


def test_o10():
    d = np.array([[0.3, NAN, -0.2, INF], [0.0, -0.0, 10.0, 10.000001], [-INF, 1e-30, 0.56, 0.5600001]], F)
    z = R.depth0_f32(d, 10.0)
    assert z.tobytes() == np.array([[0.3, 0, 0, 0], [0, 0, 10.0, 0], [0, 1e-30, 0.56, 0.5600001]], F).tobytes()
    assert R.depth0_f32(d, 0.56).tobytes() == np.array([[0.3, 0, 0, 0], [0, 0, 0, 0], [0, 1e-30, 0.56, 0]], F).tobytes()
    raw = np.array([[3000, 0, 65535, 1]], np.uint16)                              # O1's own depth passes O10 unchanged
    z1 = Od.depth0(raw, 1000.0, 10.0)
    assert R.depth0_f32(z1, 10.0).tobytes() == z1.tobytes()


TRACK_FRAMES, TRACK_DIMS = 4, (48, 40, 32)


def test_tracking_accuracy(orc):
    """(d) The odometry's accuracy condition (tests/test_odometry_abi.py: 1/10), frame to model.  The volume - 48 x 40 x 32 voxels of 1 mm,
    tests/tsdf_cases.py's small volume - is fused by the restatement from the true poses of frames 0 .. n-2 of odometry_cases.sequence at
    96 x 72 (each view turned by one degree more); the last frame is tracked from the guess "true pose of frame n-2".  Its rotation and
    translation errors must be at most a tenth of the guess's own."""
    n = TRACK_FRAMES
    s = K.sequence((96, 72), n)
    cam_in_vol = np.stack([np.linalg.inv(P.astype(np.float64)) for P in s["poses"]])
    poses = cam_in_vol.astype(F)
    vol = Cs.small_scene(TRACK_DIMS, 0)["vol"]
    buf, counts = Ts.integrate(vol, Ts.reset(vol), s["frames"][:n - 1], poses[:n - 1], s["intr"], pose_direction=Ts.SOURCE_ONTO_TARGET)
    assert (counts > 2000).all()
    r = R.track(orc, vol, buf, s["frames"][n - 1], poses[n - 2], s["intr"], tsdf=dict(zmax=0.5), odom=dict(depth_diff=K.ACCURACY_DEPTH_DIFF))
    est, guess = K.errors(r["pose"], cam_in_vol[n - 1]), K.errors(poses[n - 2], cam_in_vol[n - 1])
    ratios = (est[0] / guess[0], est[1] / guess[1])
    print("tracking frame %d against the volume of frames 0..%d: %d hits, %d partners, iterations %s; error %.4f deg, %.3e m; the guess's %.4f "
          "deg, %.3e m; ratios %.4f and %.4f (worst %.4f)" % (n - 1, n - 2, r["n_hit"], r["odom"]["n_corr"], r["odom"]["iterations"], est[0],
                                                               est[1], guess[0], guess[1], ratios[0], ratios[1], max(ratios)))
    assert r["n_hit"] > 500 and r["odom"]["n_corr"] > 500
    assert guess[0] > 0.9 and guess[1] > 0.004
    assert max(ratios) <= 0.1
