"""CPU suite: TSDF fusion (include/tdv_hip.h: tdv_tsdf_integrate_dev).  The ABI exports the entry points, lists them in ABI_SYMBOLS, has the
documented struct layout, constants and defaults, sizes a volume (0 for one the checks refuse) and refuses every bad argument before it
writes anything.  Then the restatement (tests/tsdf_restatement.py) is held to what rules T1 to T8 promise: a front-on plane comes out where
it is with normals (0, 0, -1), repeated frames are a running mean, a call's frames apply in order, the relief scene's crossings lie on
the true height field, min_weight drops what it should, and unusable frames update nothing.  No compute entry point of the library runs
here; tests/test_gpu_tsdf.py holds the device to this restatement byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import tsdf_cases as Cs
import tsdf_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
U = 2.0 ** -24                                                                   # half an ulp of 1: the relative error of one f32 rounding
NAN, INF = float("nan"), float("inf")
SYMBOLS = ("tdv_tsdf_default_params", "tdv_tsdf_volume_bytes", "tdv_tsdf_reset_dev", "tdv_tsdf_integrate_dev", "tdv_tsdf_extract_dev",
           "tdv_tsdf_fuse")


def test_symbols_constants_structs_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.TsdfVolumeC) == 28
    assert [(k, getattr(tdv.TsdfVolumeC, k).offset) for k, _ in tdv.TsdfVolumeC._fields_] == [
        ("origin", 0), ("voxel_length", 12), ("nx", 16), ("ny", 20), ("nz", 24)]
    assert C.sizeof(tdv.TsdfParamsC) == 20
    assert [(k, getattr(tdv.TsdfParamsC, k).offset) for k, _ in tdv.TsdfParamsC._fields_] == [
        ("trunc", 0), ("max_weight", 4), ("zmax", 8), ("min_weight", 12), ("pose_direction", 16)]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdv_hip.h")).read()
    for name, mine in (("MAX_SIDE", R.MAX_SIDE), ("MAX_VOXELS", R.MAX_VOXELS), ("HOST_MAX_VOXELS", R.HOST_MAX_VOXELS), ("MAX_FRAMES", R.MAX_FRAMES),
                       ("TILE_X", R.TILE[0]), ("TILE_Y", R.TILE[1]), ("TILE_Z", R.TILE[2])):
        text = header.split("#define TDV_TSDF_%s " % name)[1].split("/*")[0].split("\n")[0].strip()
        assert eval(text) == getattr(tdv, "TDV_TSDF_" + name) == mine, (name, text)
    assert tdv.TDV_VERIFY_MAX_SIDE == R.FRAME_MAX_SIDE
    assert (tdv.TDV_POSE_SOURCE_ONTO_TARGET, tdv.TDV_POSE_MODEL_TO_CAMERA) == (R.SOURCE_ONTO_TARGET, R.MODEL_TO_CAMERA)
    for rule in ("T1.", "T2.", "T3.", "T4.", "T5.", "T6.", "T7.", "T8."):
        assert " %s " % rule in header, rule
    p = tdv.tsdf_params()
    assert {k: getattr(p, k) for k, _ in tdv.TsdfParamsC._fields_} == R.DEFAULTS
    lib.tdv_tsdf_default_params(None)                                              # a NULL is ignored
    q = tdv.tsdf_params(trunc=0.004, max_weight=2, pose_direction="source_onto_target")
    assert (q.trunc, q.max_weight, q.pose_direction) == (F(0.004), 2.0, R.SOURCE_ONTO_TARGET)
    assert tdv.Context.tsdf_params(min_weight=2).min_weight == 2.0
    with pytest.raises(TypeError):
        tdv.tsdf_params(truncation=1)


def test_volume_bytes(tdv):
    lib = tdv.lib()

    def nbytes(origin=(0, 0, 0), L=0.001, dims=(4, 3, 2)):
        return int(lib.tdv_tsdf_volume_bytes(C.byref(tdv.tsdf_volume_struct(origin, L, dims))))

    assert nbytes() == 4 * 3 * 2 * 8 and nbytes(dims=(1, 1, 1)) == 8
    assert nbytes(dims=(1024, 1024, 128)) == 1 << 30 and nbytes(dims=(1024, 1, 1024)) == 1 << 23
    assert nbytes(dims=(1024, 1024, 129)) == 0 and nbytes(dims=(1025, 1, 1)) == 0 and nbytes(dims=(1, 1025, 1)) == 0
    assert nbytes(dims=(1, 1, 1025)) == 0
    for d in ((0, 3, 2), (4, 0, 2), (4, 3, 0), (-1, 3, 2), (4, 3, -5)):
        assert nbytes(dims=d) == 0, d
    for L in (0.0, -0.001, NAN, INF, -INF):
        assert nbytes(L=L) == 0, L
    assert int(lib.tdv_tsdf_volume_bytes(None)) == 0


# ---------------------------------------------------------------- arguments
GOOD = dict(voxel_length=0.001, nx=4, ny=3, nz=2, n_frames=2, width=8, height=6, scale=1000.0, fx=10.0, fy=10.0, trunc=0.0, max_weight=255.0,
            zmax=10.0, min_weight=1.0, pose_direction=R.MODEL_TO_CAMERA, capacity=8)
VOLUME, PARAMS, FRAMES, OUTPUT = ("reset", "integrate", "extract", "fuse"), ("integrate", "extract", "fuse"), ("integrate", "fuse"), ("extract", "fuse")
BAD = [("null ctx", {}, VOLUME)]
BAD += [("%s %r" % (k, v), {k: v}, VOLUME) for k in ("nx", "ny", "nz") for v in (0, -1, R.MAX_SIDE + 1)]
BAD += [("voxels above the cap", dict(nx=1024, ny=1024, nz=129), VOLUME), ("voxels above the host cap", dict(nx=1024, ny=1024, nz=33), ("fuse",))]
BAD += [("voxel_length %r" % v, dict(voxel_length=v), VOLUME) for v in (0.0, -0.001, NAN, INF)]
BAD += [("%s %r" % (k, v), {k: v}, FRAMES) for k in ("scale", "fx", "fy") for v in (0.0, -1.0, NAN, INF)]
BAD += [("trunc %r" % v, dict(trunc=v), PARAMS) for v in (-0.001, NAN, INF)]
BAD += [("max_weight %r" % v, dict(max_weight=v), PARAMS) for v in (0.5, 0.0, NAN, INF)]
BAD += [("min_weight %r" % v, dict(min_weight=v), PARAMS) for v in (0.0, -1.0, NAN, INF)]
BAD += [("n_frames %r" % v, dict(n_frames=v), FRAMES) for v in (-1, R.MAX_FRAMES + 1)]
BAD += [("%s %r" % (k, v), {k: v}, FRAMES) for k in ("width", "height") for v in (-1, R.FRAME_MAX_SIDE + 1)]
BAD += [("pose_direction %r" % v, dict(pose_direction=v), PARAMS) for v in (2, -1)]
BAD += [("capacity -1", dict(capacity=-1), OUTPUT)]
NULLS = {"vol": VOLUME, "volume": ("reset", "integrate", "extract"), "params": PARAMS, "frames": FRAMES, "poses": FRAMES, "n_out": OUTPUT,
         "out_xyz": OUTPUT}


class Outputs:
    """Host arrays in every slot a call writes (a refused call must not look at them), filled with a pattern; untouched() compares."""

    def __init__(self):
        self.volume = np.full(4 * 3 * 2 * 2, -7, F); self.counts = np.full(R.MAX_FRAMES + 1, -7, np.int64)
        self.xyz = np.full((8, 3), -7, F); self.normals = np.full((8, 3), -7, F); self.n_out = np.full(1, -7, np.int32)
        self.before = self.snapshot()

    def arrays(self):
        return self.volume, self.counts, self.xyz, self.normals, self.n_out

    def snapshot(self):
        return tuple(a.tobytes() for a in self.arrays())

    def untouched(self):
        return self.snapshot() == self.before


def P(x):
    return None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))


def tsdf_call(tdv, which, ctx, o, null=(), buffers=None, **kw):
    """One entry point on GOOD's arguments with kw replaced and the pointers named in `null` NULL.  buffers (the GPU suite): device
    pointers for volume, frames, xyz, normals in place of the host arrays."""
    g = dict(GOOD, **kw)
    lib = tdv.lib()
    b = buffers or {}
    vol = tdv.TsdfVolumeC((C.c_float * 3)(0.0, 0.0, 0.3), g["voxel_length"], g["nx"], g["ny"], g["nz"])
    prm = tdv.TsdfParamsC(g["trunc"], g["max_weight"], g["zmax"], g["min_weight"], g["pose_direction"])
    raw = np.full((R.MAX_FRAMES + 1) * 8 * 6, 3000, np.uint16)
    poses = np.tile(np.eye(4, dtype=F).reshape(-1), R.MAX_FRAMES + 1)
    pv = None if "vol" in null else C.byref(vol)
    pp = None if "params" in null else C.byref(prm)
    volume = None if "volume" in null else P(b.get("volume", o.volume))
    frames = None if "frames" in null else P(b.get("frames", raw))
    xyz = None if "out_xyz" in null else P(b.get("xyz", o.xyz))
    nrm = P(b.get("normals", o.normals))
    n_out = None if "n_out" in null else P(o.n_out)
    cam = (g["width"], g["height"], C.c_float(g["scale"]), C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(3.5), C.c_float(2.5))
    hp = None if "poses" in null else P(poses)
    if which == "reset":
        return lib.tdv_tsdf_reset_dev(ctx, pv, volume)
    if which == "integrate":
        return lib.tdv_tsdf_integrate_dev(ctx, pv, volume, frames, g["n_frames"], *cam, hp, pp, P(o.counts))
    if which == "extract":
        return lib.tdv_tsdf_extract_dev(ctx, pv, volume, pp, xyz, nrm, g["capacity"], n_out)
    return lib.tdv_tsdf_fuse(ctx, pv, None if "frames" in null else P(raw), g["n_frames"], *cam, hp, pp,
                             None if "out_xyz" in null else P(o.xyz), P(o.normals), g["capacity"], n_out)


@pytest.mark.parametrize("case", range(len(BAD)), ids=[b[0] for b in BAD])
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_tsdf.py refuses each bad argument on one."""
    o = Outputs()
    what, kw, where = BAD[case]
    for which in where:
        assert tsdf_call(tdv, which, None, o, **kw) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


def test_null_pointers(tdv):
    o = Outputs()
    for what, where in NULLS.items():
        for which in where:
            assert tsdf_call(tdv, which, None, o, null=(what,)) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against what the rules promise
PLANE_VOL = R.Volume((-0.009, -0.007, 0.39), 0.002, (9, 7, 12))
PLANE_D, PLANE_RAW = 0.4, 4000                                                    # 0.4 m = 4000 / 10000, between the layers at 0.399 and 0.401
PLANE_INTR = (10000.0, 500.0, 500.0, 31.5, 23.5)


def plane():
    frames = np.full((1, 48, 64), PLANE_RAW, np.uint16)
    return R.integrate(PLANE_VOL, R.reset(PLANE_VOL), frames, np.eye(4, dtype=F)[None], PLANE_INTR)


def test_front_on_plane():
    """One frame of constant depth d = 0.4 m under the identity pose.  zc is the centre's z exactly (a sum with zeros), zo and a centre
    lie within a factor of two of each other, so sdf = zo - zc is exact; trunc = 4 L is exact; t = sdf / trunc carries one rounding and the
    first update (1*0 + t) / (0 + 1) none.  With exact weights T7's expression is zo itself; the two roundings in r_a, r_b move the
    interpolation weight by at most 2u of itself, the point by less than L u / 2.  Its evaluation has only positive terms: two products,
    two sums and a division, 5u of z.  zo = float(raw) * float(1 / scale) is within 2u of d.  Together below 8 u d = 1.9e-7 m, a hundredth
    of L / 100."""
    vol = PLANE_VOL
    buf, counts = plane()
    _, _, zw = vol.centres()
    tr = R.trunc_of(vol, 0.0)
    assert tr == F(4.0) * vol.L and 0.3989 < zw[4] < PLANE_D < zw[5] < 0.4011
    touched = zw <= F(PLANE_D) + tr                                                # sdf >= -trunc
    assert touched.sum() == 9 and counts[0] == 9 * vol.nx * vol.ny
    assert (buf[touched][..., 1] == 1).all() and (buf[~touched] == (1, 0)).all()
    assert (buf[:1][..., 0] == 1).all()                                            # 9 mm in front: min(1, sdf / trunc)
    xyz, nrm, key = R.extract(vol, buf)
    assert len(key) == vol.nx * vol.ny and (key % 3 == 2).all() and (key // 3 // (vol.nx * vol.ny) == 4).all()
    bound = 8 * U * PLANE_D
    err = np.abs(xyz[:, 2].astype(np.float64) - PLANE_D).max()
    print("plane: largest |z - d| = %.3e m (bound %.3e, L / 100 = %.1e)" % (err, bound, float(vol.L) / 100))
    assert err <= bound < float(vol.L) / 100 / 100
    xw, yw, _ = vol.centres()
    assert xyz[:, 0].tobytes() == np.tile(xw, vol.ny).tobytes() and xyz[:, 1].tobytes() == np.repeat(yw, vol.nx).tobytes()
    assert (nrm == np.array([0, 0, -1], F)).all()                                  # positive in front, the camera looks along +z


def test_running_mean():
    """The same frame n times in one call: every update is the mean of the stored value and an equal t, three roundings - (f*w, + t,
    / (w + 1)) - of values of magnitude at most that of t (w + 1): within 3 n u |t| of t; w = min(n, max_weight)."""
    s = Cs.small_scene((33, 17, 21), 1)
    vol = s["vol"]
    one, c1 = R.integrate(vol, R.reset(vol), s["frames"], s["poses"], s["intr"])
    seen = one[..., 1] == 1
    assert c1[0] == seen.sum() > 2000 and ((one[..., 0] < 1) & seen).sum() > 500
    t = one[..., 0].astype(np.float64)
    for n, max_weight in ((2, 255.0), (5, 255.0), (5, 3.0), (7, 1.0)):
        buf, c = R.integrate(vol, R.reset(vol), np.repeat(s["frames"], n, 0), np.repeat(s["poses"], n, 0), s["intr"], max_weight=max_weight)
        assert (c == c1[0]).all() and len(c) == n
        assert (buf[..., 1] == np.where(seen, min(n, max_weight), 0)).all()
        err = np.abs(buf[..., 0].astype(np.float64) - t)
        assert (err <= 3 * n * U * np.abs(t)).all(), (n, max_weight, err.max())
        assert (buf[~seen] == (1, 0)).all()


def test_frame_order():
    s = Cs.small_scene((33, 17, 21), 3)
    vol, fr, po = s["vol"], s["frames"], s["poses"]
    whole, c = R.integrate(vol, R.reset(vol), fr, po, s["intr"], max_weight=1.5)
    a, ca = R.integrate(vol, R.reset(vol), fr[:1], po[:1], s["intr"], max_weight=1.5)
    ab, cb = R.integrate(vol, a, fr[1:2], po[1:2], s["intr"], max_weight=1.5)
    abc, cc = R.integrate(vol, ab, fr[2:], po[2:], s["intr"], max_weight=1.5)
    assert whole.tobytes() == abc.tobytes() and (c == [ca[0], cb[0], cc[0]]).all()
    a_bc, _ = R.integrate(vol, a, fr[1:], po[1:], s["intr"], max_weight=1.5)
    assert a_bc.tobytes() == whole.tobytes()
    acb, _ = R.integrate(vol, R.reset(vol), fr[[0, 2, 1]], po[[0, 2, 1]], s["intr"], max_weight=1.5)
    assert acb.tobytes() != whole.tobytes()                                        # with the weight capped at 1.5 the order shows
    assert a.tobytes() != R.reset(vol).tobytes()


@pytest.fixture(scope="module")
def relief():
    s = Cs.relief_scene()
    buf, counts = R.integrate(s["vol"], R.reset(s["vol"]), s["frames"], s["poses"], s["intr"], trunc=0.004)
    first, _ = R.integrate(s["vol"], R.reset(s["vol"]), s["frames"][:1], s["poses"][:1], s["intr"], trunc=0.004)
    return dict(s, buf=buf, counts=counts, first=first)


def test_relief_scene(relief):
    """Inside a 2 mm margin of the plate every crossing is within one voxel_length of the true height field, measured along z (no less
    than the distance to the surface); no normal is more than 90 degrees from the true one, none is zero; four views give more crossings
    than the first alone, which has a hole wherever no surface sample fell on a pixel."""
    vol, part = relief["vol"], relief["part"]
    xyz, nrm, key = R.extract(vol, relief["buf"])
    one = R.extract(vol, relief["first"])[0]
    inside = (np.abs(xyz[:, 0]) < part.L / 2 - 0.002) & (np.abs(xyz[:, 1]) < part.W / 2 - 0.002)
    h, n = Cs.true_surface(part, xyz)
    dz = np.abs(xyz[:, 2] - h)[inside]
    cos = (nrm.astype(np.float64) * n).sum(1)
    ang = np.degrees(np.arccos(np.clip(cos[inside], -1, 1)))
    print("relief: %d crossings from four views, %d from the first; inside the margin %d: |z - h| max %.3f, median %.3f, p99 %.3f mm; normals "
          "median %.2f, p95 %.2f, max %.1f degrees" % (len(xyz), len(one), inside.sum(), dz.max() * 1e3, np.median(dz) * 1e3,
                                                       np.percentile(dz, 99) * 1e3, np.median(ang), np.percentile(ang, 95), ang.max()))
    assert inside.sum() > 12000 and (dz <= float(vol.L)).all()
    assert (cos > 0).all() and (np.abs(nrm).sum(1) > 0).all()
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() <= 4 * U
    assert len(xyz) > len(one) > 10000
    assert (np.diff(key) > 0).all() and (relief["counts"] > 200000).all()


def test_min_weight(relief):
    """min_weight = 2 keeps exactly the crossings whose two ends were both seen twice, at the points they had."""
    vol, buf = relief["vol"], relief["buf"]
    xyz1, _, key1 = R.extract(vol, buf, min_weight=1.0)
    xyz2, _, key2 = R.extract(vol, buf, min_weight=2.0)
    w = buf[..., 1].reshape(-1)
    a, step = key1 // 3, np.array([1, vol.nx, vol.nx * vol.ny])[key1 % 3]
    keep = (w[a] >= 2) & (w[a + step] >= 2)
    assert 0 < keep.sum() < len(key1) and (w[a][~keep] == 1).any()
    assert np.array_equal(key2, key1[keep]) and xyz2.tobytes() == xyz1[keep].tobytes()


def test_unusable_frames_update_nothing():
    s = Cs.small_scene((33, 17, 21), 2)
    vol = s["vol"]
    start, _ = R.integrate(vol, R.reset(vol), s["frames"][:1], s["poses"][:1], s["intr"])
    behind = s["poses"][1].copy(); behind[2, 3] = -0.3                             # the volume at negative camera z
    cases = {"a pose of NaNs": (s["frames"][1], np.full((4, 4), NAN, F)), "a NaN in the rotation": (s["frames"][1], s["poses"][1] * np.array([1, NAN, 1, 1], F)),
             "a frame of zeros": (np.zeros_like(s["frames"][1]), s["poses"][1]), "a camera behind the volume": (s["frames"][1], behind),
             "an infinite translation": (s["frames"][1], s["poses"][1] + np.array([[0, 0, 0, INF]] * 3 + [[0, 0, 0, 0]], F))}
    for what, (frame, pose) in cases.items():
        for direction in (R.MODEL_TO_CAMERA, R.SOURCE_ONTO_TARGET):
            buf, c = R.integrate(vol, start, frame[None], pose[None], s["intr"], pose_direction=direction)
            assert c[0] == 0 and buf.tobytes() == start.tobytes(), (what, direction)
    buf, c = R.integrate(vol, start, s["frames"][1:], s["poses"][1:], s["intr"], zmax=0.2)      # zmax in front of everything
    assert c[0] == 0 and buf.tobytes() == start.tobytes()
    buf, c = R.integrate(vol, start, s["frames"][1:], s["poses"][1:], s["intr"])
    assert c[0] > 2000 and buf.tobytes() != start.tobytes()
