"""CPU suite: depth odometry (include/tdv_hip.h: tdv_depth_odometry_dev).  The ABI exports the entry points, lists them in ABI_SYMBOLS, has
the documented struct layout, constants and defaults, states rules O1 to O9, and refuses every bad argument before it writes anything.
Then the restatement (tests/odometry_restatement.py) is held to what the rules promise: a front-on plane has normals exactly (0, 0, -1)
and none in the last row and column, a depth step above depth_diff has no normal across it and is not averaged in the pyramid, at the
true pose of a noise-free render the update is small, and the accuracy condition on the six pairs of tests/odometry_cases.py.  No compute
entry point of the library runs here; tests/test_gpu_odometry.py holds the device to this restatement byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import odometry_cases as K
import odometry_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
NAN, INF = float("nan"), float("inf")
SYMBOLS = ("tdv_odometry_default_params", "tdv_depth_maps_dev", "tdv_depth_maps", "tdv_depth_odometry_terms_dev", "tdv_depth_odometry_dev",
           "tdv_depth_odometry", "tdv_depth_odometry_sequence_dev")
MAX_SIDE, MAX_FRAMES = 8192, 64


def test_symbols_constants_structs_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.OdometryParamsC) == 28
    assert [(k, getattr(tdv.OdometryParamsC, k).offset) for k, _ in tdv.OdometryParamsC._fields_] == [
        ("depth_diff", 0), ("zmax", 4), ("n_levels", 8), ("max_iterations", 12)]
    assert C.sizeof(tdv.OdometryResultC) == 108
    assert [(k, getattr(tdv.OdometryResultC, k).offset) for k, _ in tdv.OdometryResultC._fields_] == [
        ("T", 0), ("fitness", 64), ("rmse", 68), ("n_corr", 72), ("iterations", 76), ("n_corr_level", 92)]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdv_hip.h")).read()
    text = header.split("#define TDV_ODOM_MAX_LEVELS ")[1].split("/*")[0].split("\n")[0].strip()
    assert eval(text) == tdv.TDV_ODOM_MAX_LEVELS == R.MAX_LEVELS
    assert (tdv.TDV_VERIFY_MAX_SIDE, tdv.TDV_TSDF_MAX_FRAMES, tdv.ODOM_TERMS) == (MAX_SIDE, MAX_FRAMES, 29)
    for rule in ("O1.", "O2.", "O3.", "O4.", "O5.", "O6.", "O7.", "O8.", "O9."):
        assert " %s " % rule in header, rule
    for s in SYMBOLS:
        assert s + "(" in header, s
    p = tdv.odometry_params()
    assert (p.depth_diff, p.zmax, p.n_levels, tuple(p.max_iterations)) == (F(0.03), 10.0, 3, (20, 10, 5, 0))
    d = R.params()
    assert (d["depth_diff"], d["zmax"], d["n_levels"], d["max_iterations"]) == (F(0.03), F(10.0), 3, (20, 10, 5, 0))
    lib.tdv_odometry_default_params(None)                                          # a NULL is ignored
    q = tdv.odometry_params(depth_diff=0.004, n_levels=2, max_iterations=(7, 3))
    assert (q.depth_diff, q.n_levels, tuple(q.max_iterations)) == (F(0.004), 2, (7, 3, 0, 0))
    assert tdv.Context.odometry_params(zmax=2).zmax == 2.0
    with pytest.raises(TypeError):
        tdv.odometry_params(depth_difference=1)


# ---------------------------------------------------------------- arguments
GOOD = dict(width=8, height=6, scale=1000.0, fx=10.0, fy=10.0, depth_diff=0.03, zmax=10.0, n_levels=2, max_iterations=(2, 2, 0, 0), level=0,
            n_frames=3, capacity=48)
ALL, PAIR, TERMS, SEQ, MAPS = ("maps_dev", "maps", "terms", "pair_dev", "pair", "sequence"), ("terms", "pair_dev", "pair", "sequence"), ("terms",), \
    ("sequence",), ("maps_dev", "maps")
BAD = [("null ctx", {}, ALL)]
BAD += [("%s %r" % (k, v), {k: v}, ALL) for k in ("width", "height") for v in (-1, MAX_SIDE + 1)]
BAD += [("%s %r" % (k, v), {k: v}, ALL) for k in ("scale", "fx", "fy", "depth_diff", "zmax") for v in (0.0, -1.0, NAN, INF)]
BAD += [("n_levels %r" % v, dict(n_levels=v), ALL) for v in (0, -1, 5)]
BAD += [("a level with a side of 0", dict(n_levels=4), PAIR), ("a level with a side of 0 (width)", dict(width=3, height=64, n_levels=3), PAIR)]
BAD += [("max_iterations %r" % (v,), dict(max_iterations=v), ALL) for v in ((-1, 0, 0, 0), (1, 1, 1, -5))]
BAD += [("level %r" % v, dict(level=v), TERMS) for v in (-1, 2)]
BAD += [("n_frames %r" % v, dict(n_frames=v), SEQ) for v in (-1, MAX_FRAMES + 1)]
BAD += [("capacity -1", dict(capacity=-1), MAPS)]
NULLS = {"params": ALL, "frames": ALL, "result": ("pair_dev", "pair"), "pose": TERMS, "sums": TERMS, "poses": SEQ, "n_out": MAPS, "rows": MAPS}


class Outputs:
    """Host arrays in every slot a call writes (a refused call must not look at them), filled with a pattern; untouched() compares."""

    def __init__(self):
        self.vm = np.full((48, 3), -7, F); self.nm = np.full((48, 3), -7, F)
        self.xyz = np.full((48, 3), -7, F); self.normals = np.full((48, 3), -7, F); self.n_out = np.full(1, -7, np.int32)
        self.sums = np.full(29, -7.0); self.n_valid = np.full(1, -7, np.int32)
        self.result = np.full(27 * (MAX_FRAMES + 2), -7, np.int32); self.poses = np.full(16 * (MAX_FRAMES + 2), -7, F)
        self.before = self.snapshot()

    def arrays(self):
        return self.vm, self.nm, self.xyz, self.normals, self.n_out, self.sums, self.n_valid, self.result, self.poses

    def snapshot(self):
        return tuple(a.tobytes() for a in self.arrays())

    def untouched(self):
        return self.snapshot() == self.before


def P(x):
    return None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))


def odom_call(tdv, which, ctx, o, null=(), buffers=None, **kw):
    """One entry point on GOOD's arguments with kw replaced and the pointers named in `null` NULL.  buffers (the GPU suite): device
    pointers for frames, vm, nm, xyz, normals in place of the host arrays."""
    g = dict(GOOD, **kw)
    lib = tdv.lib()
    b = buffers or {}
    prm = tdv.OdometryParamsC(g["depth_diff"], g["zmax"], g["n_levels"], (C.c_int * 4)(*g["max_iterations"]))
    raw = np.full((MAX_FRAMES + 1) * 8 * 6, 3000, np.uint16)
    pp = None if "params" in null else C.byref(prm)
    dev = which in ("maps_dev", "terms", "pair_dev", "sequence")
    frames = None if "frames" in null else P(b.get("frames", raw) if dev else raw)
    T = np.eye(4, dtype=F).reshape(-1)
    cam = (g["width"], g["height"], C.c_float(g["scale"]), C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(3.5), C.c_float(2.5))
    if which in MAPS:
        d = dev and bool(b)
        rows = "rows" in null
        return getattr(lib, "tdv_depth_" + which)(ctx, frames, *cam, pp, P(b["vm"] if d else o.vm), P(b["nm"] if d else o.nm),
                                                  None if rows else P(b["xyz"] if d else o.xyz), None if rows else P(b["normals"] if d else o.normals),
                                                  g["capacity"], None if "n_out" in null else P(o.n_out))
    if which == "terms":
        return lib.tdv_depth_odometry_terms_dev(ctx, frames, frames, *cam, None if "pose" in null else P(T), g["level"], pp,
                                                None if "sums" in null else P(o.sums), P(o.n_valid))
    if which in ("pair_dev", "pair"):
        fn = lib.tdv_depth_odometry_dev if dev else lib.tdv_depth_odometry
        return fn(ctx, frames, frames, *cam, P(T), pp, None if "result" in null else P(o.result))
    return lib.tdv_depth_odometry_sequence_dev(ctx, frames, g["n_frames"], *cam, None, pp, None if "poses" in null else P(o.poses), P(o.result))


@pytest.mark.parametrize("case", range(len(BAD)), ids=[b[0] for b in BAD])
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_odometry.py refuses each bad argument on one."""
    o = Outputs()
    what, kw, where = BAD[case]
    for which in where:
        assert odom_call(tdv, which, None, o, **kw) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


def test_null_pointers_leave_outputs_untouched(tdv):
    o = Outputs()
    for name, where in NULLS.items():
        for which in where:
            assert odom_call(tdv, which, None, o, null=(name,)) == TDV_ERR_BAD_ARG, (name, which)
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against what the rules promise
PLANE_INTR = (1000.0, 60.0, 55.0, 7.5, 5.0)


def test_front_on_plane():
    """O3: normals exactly (0, 0, -1), and none in the last row and column; O4 keeps the plane's depth."""
    raw = np.full((11, 16), 400, np.uint16)
    m = R.maps(raw, PLANE_INTR)
    assert (m["normal_map"][:-1, :-1] == np.array([0, 0, -1], F)).all()
    assert not m["normal_map"][-1].any() and not m["normal_map"][:, -1].any()
    assert len(m["xyz"]) == 10 * 15 and (m["xyz"][:, 2] == F(400) * F(1.0 / 1000.0)).all()
    assert m["xyz"].tobytes() == m["vertex_map"][:-1, :-1].reshape(-1, 3).tobytes()
    levels = R.pyramid(raw, PLANE_INTR, R.params(n_levels=3))
    assert [l["z"].shape for l in levels] == [(11, 16), (5, 8), (2, 4)]
    z = levels[0]["z"][0, 0]
    for l in (1, 2):
        z = (((z + z) + z) + z) / F(4)                                             # O4's sum, in its order
        assert (levels[l]["z"] == z).all() and (levels[l]["normals"][:-1, :-1] == np.array([0, 0, -1], F)).all()
    assert levels[1]["cam"] == (F(30.0), F(27.5), F(3.5), F(2.25))


def test_depth_step_and_invalid_pixels():
    """A step above depth_diff: no normal across it, and a block that straddles it averages only the pixels near its first valid one.
    Pixels at 0 or beyond zmax are invalid: no vertex, no normal through them, not averaged."""
    raw = np.full((8, 9), 400, np.uint16)
    raw[:, 5:] = 500                                                               # a step of 0.1 m at column 5; blocks (2, .) straddle it
    raw[2, 1] = 0
    raw[6, 2] = 20000                                                              # 20 m: beyond zmax
    m = R.maps(raw, PLANE_INTR)
    has = (m["normal_map"] != 0).any(-1)
    assert not has[:, 4].any() and has[:-1, 5].all() and has[0, 3]
    assert not has[2, 1] and not has[2, 0] and not has[1, 1] and not has[6, 2] and not has[6, 1] and not has[5, 2]
    assert not m["vertex_map"][2, 1].any() and not m["vertex_map"][6, 2].any() and m["vertex_map"][2, 2].any()
    z1 = R.downsample(R.depth0(raw, 1000.0, 10.0), 0.03)
    z4, z5 = F(400) * F(1.0 / 1000.0), F(500) * F(1.0 / 1000.0)
    assert z1.shape == (4, 4)
    assert np.allclose(z1[:, :2], z4, rtol=0, atol=1e-7) and np.allclose(z1[:, 3], z5, rtol=0, atol=1e-7)      # (three members at the two holes)
    assert (z1[:, 2] == (z4 + z4) / F(2)).all(), "the blocks of columns 4 and 5: first valid 0.4, the 0.5 pixels are no members"
    wide = R.downsample(R.depth0(raw, 1000.0, 10.0), 0.2)
    assert (wide[:, 2] == (((z4 + z5) + z4) + z5) / F(4)).all()
    none = R.downsample(np.zeros((4, 4), F), 0.03)
    assert not none.any()


def test_update_at_the_true_pose_is_small(orc):
    """A noise-free render: started at the ground truth, one iteration on the finest level moves the pose by less than the frame can
    resolve - half a pixel's footprint (0.3 m / 420 = 0.71 mm) in translation, and that over the part's half length (30 mm) in rotation.
    The partners are a pixel's own vertex, so the rmse stays below the footprint, and most valid pixels of a 2 degree turn have one."""
    c = K.pair((160, 120), 2.0)
    r = R.odometry(orc, c["src"], c["tgt"], c["intr"], T0=c["T_gt"].astype(F), n_levels=1, max_iterations=(1,), depth_diff=K.ACCURACY_DEPTH_DIFF)
    rot, tr = K.errors(r["T"], c["T_gt"])
    foot = K.DISTANCE / K.SIZES[(160, 120)]
    assert r["iterations"] == [1, 0, 0, 0] and r["n_corr"] == r["n_corr_level"][0] and r["fitness"] > 0.8
    assert tr < 0.5 * foot and rot < np.degrees(0.5 * foot / 0.03), (rot, tr)
    assert r["rmse"] < foot


# Measured with this restatement (f32), identity -> result, rotation in degrees / translation in mm:
#   96 x 72:   1 deg: 1.000 / 5.14 -> 0.0407 / 0.096   2 deg: 2.000 / 10.28 -> 0.0393 / 0.172   4 deg: 4.000 / 20.57 -> 0.0754 / 0.334
#   160 x 120: 1 deg: 1.000 / 5.14 -> 0.0149 / 0.091   2 deg: 2.000 / 10.28 -> 0.0345 / 0.127   4 deg: 4.000 / 20.57 -> 0.0549 / 0.262
# The worst ratio is 1 / 24.6 (rotation, 96 x 72 at 1 degree).
@pytest.mark.parametrize("size", sorted(K.SIZES))
@pytest.mark.parametrize("angle", K.ANGLES)
def test_accuracy_condition(orc, size, angle):
    """From the identity with the default params at depth_diff = 0.004, the rotation error and the translation error against the render's
    ground truth are both below one tenth of the identity's.  The device inherits the condition through byte equality."""
    c = K.pair(size, angle)
    r = R.odometry(orc, c["src"], c["tgt"], c["intr"], depth_diff=K.ACCURACY_DEPTH_DIFF)
    rot0, tr0 = K.errors(np.eye(4), c["T_gt"])
    rot, tr = K.errors(r["T"], c["T_gt"])
    print("%s %g deg: rotation %.4f -> %.4f deg, translation %.3f -> %.3f mm" % (size, angle, rot0, rot, tr0 * 1e3, tr * 1e3))
    assert abs(rot0 - angle) < 1e-3
    assert rot < rot0 / 10 and tr < tr0 / 10, (rot0, rot, tr0, tr)


def test_chain_and_sequence(orc):
    """O9: the chain of the pairs' motions is the camera's pose in camera 0's frame - against the render's own poses."""
    s = K.sequence((96, 72), 4)
    poses, pairs = R.sequence(orc, s["frames"], s["intr"], depth_diff=K.ACCURACY_DEPTH_DIFF)
    assert poses[0].tobytes() == np.eye(4, dtype=F).tobytes() and pairs[0]["n_corr"] == 0 and not pairs[0]["T"].any()
    assert poses[1].tobytes() == pairs[1]["T"].tobytes()
    for k in range(1, 4):
        gt = K.truth(s["poses"][k], s["poses"][0])                                # camera k in camera 0's frame
        rot, tr = K.errors(poses[k], gt)
        assert rot < 0.1 * k and tr < 0.000514 * k, (k, rot, tr)                  # a tenth of each pair's own motion (1 degree, 5.14 mm); errors add
    one = R.sequence(orc, s["frames"][:1], s["intr"])
    assert one[0].shape == (1, 4, 4) and len(one[1]) == 1
    assert R.sequence(orc, s["frames"][:0], s["intr"])[0].shape == (0, 4, 4)
