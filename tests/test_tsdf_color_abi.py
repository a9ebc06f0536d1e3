"""CPU suite: coloured TSDF fusion (include/tdv_hip.h: tdv_tsdf_integrate_color_dev).  The ABI exports the entry points and lists them in
ABI_SYMBOLS, sizes a colour volume at 16 bytes a voxel (0 for one the checks refuse) and refuses every bad argument before it writes
anything.  Then the restatement (tests/tsdf_color_restatement.py) is held to what rules T19 to T24 promise: constant-colour frames on a
front-on plane give the running mean worked out by hand, a call's frames apply in order, a split call is the one call, every stored
channel stays in [0, 1], wc is the colour's own weight, and on a part painted with a linear ramp the fused colour of every crossing is
the texture at that point within the bound the geometry gives.  No compute entry point of the library runs here;
tests/test_gpu_tsdf_color.py holds the device to this restatement byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import tsdf_cases as Cs
import tsdf_color_cases as Cc
import tsdf_color_restatement as K
import tsdf_restatement as R
from test_tsdf_abi import PLANE_INTR, PLANE_RAW, PLANE_VOL

TDV_ERR_BAD_ARG = -2
F = np.float32
U = 2.0 ** -24
NAN, INF = float("nan"), float("inf")
SYMBOLS = ("tdv_tsdf_color_bytes", "tdv_tsdf_color_reset_dev", "tdv_tsdf_integrate_color_dev", "tdv_tsdf_extract_color_dev",
           "tdv_tsdf_extract_mesh_color_dev", "tdv_tsdf_raycast_color_dev", "tdv_tsdf_fuse_color")


def test_symbols_and_rules(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdv_hip.h")).read()
    for rule in ("T19.", "T20.", "T21.", "T22.", "T23.", "T24."):
        assert " %s " % rule in header, rule
    for s in SYMBOLS:
        assert s + "(" in header, s
    assert "Not provided: colour," not in header                                   # the two TSDF lists it led
    for name in ("tsdf_color_volume", "tsdf_color_reset_dev", "tsdf_integrate_color_dev", "tsdf_integrate_color", "tsdf_extract_color_dev",
                 "tsdf_extract_color", "tsdf_extract_mesh_color_dev", "tsdf_extract_mesh_color", "tsdf_raycast_color_dev", "tsdf_raycast_color",
                 "tsdf_fuse_color"):
        assert callable(getattr(tdv.Context, name)), name


def test_color_bytes(tdv):
    lib = tdv.lib()

    def nbytes(origin=(0, 0, 0), L=0.001, dims=(4, 3, 2)):
        return int(lib.tdv_tsdf_color_bytes(C.byref(tdv.tsdf_volume_struct(origin, L, dims))))

    assert nbytes() == 4 * 3 * 2 * 16 and nbytes(dims=(1, 1, 1)) == 16
    assert nbytes(dims=(1024, 1024, 128)) == 1 << 31 and nbytes(dims=(1024, 1, 1024)) == 1 << 24
    assert nbytes(dims=(1024, 1024, 129)) == 0 and nbytes(dims=(1025, 1, 1)) == 0 and nbytes(dims=(1, 1025, 1)) == 0
    assert nbytes(dims=(1, 1, 1025)) == 0
    for d in ((0, 3, 2), (4, 0, 2), (4, 3, 0), (-1, 3, 2), (4, 3, -5)):
        assert nbytes(dims=d) == 0, d
    for L in (0.0, -0.001, NAN, INF, -INF):
        assert nbytes(L=L) == 0, L
    assert int(lib.tdv_tsdf_color_bytes(None)) == 0
    for dims in ((4, 3, 2), (65, 33, 17)):                                         # two pair volumes' worth, whatever the volume
        vol = tdv.tsdf_volume_struct((0, 0, 0), 0.001, dims)
        assert int(lib.tdv_tsdf_color_bytes(C.byref(vol))) == 2 * int(lib.tdv_tsdf_volume_bytes(C.byref(vol)))


# ---------------------------------------------------------------- arguments
GOOD = dict(voxel_length=0.001, nx=4, ny=3, nz=2, n_frames=2, width=8, height=6, scale=1000.0, fx=10.0, fy=10.0, trunc=0.0, max_weight=255.0,
            zmax=10.0, min_weight=1.0, pose_direction=R.MODEL_TO_CAMERA, capacity=8, triangle_capacity=8, zmin=0.05, max_steps=64, color_offset=0)
ALL = ("reset", "integrate", "extract", "mesh", "raycast", "fuse", "fuse_mesh")
PARAMS, FRAMES, OUTPUT, MESH, CAST = ALL[1:], ("integrate", "fuse", "fuse_mesh"), ("extract", "mesh", "fuse", "fuse_mesh"), ("mesh", "fuse_mesh"), ("raycast",)
COLOR = ALL[:5]                                                                    # the calls that take a colour volume from the caller
BAD = [("null ctx", {}, ALL)]
BAD += [("%s %r" % (k, v), {k: v}, ALL) for k in ("nx", "ny", "nz") for v in (0, -1, R.MAX_SIDE + 1)]
BAD += [("voxels above the cap", dict(nx=1024, ny=1024, nz=129), ALL), ("voxels above the host cap", dict(nx=1024, ny=1024, nz=33), ("fuse", "fuse_mesh"))]
BAD += [("voxel_length %r" % v, dict(voxel_length=v), ALL) for v in (0.0, -0.001, NAN, INF)]
BAD += [("scale %r" % v, dict(scale=v), FRAMES) for v in (0.0, -1.0, NAN, INF)]
BAD += [("%s %r" % (k, v), {k: v}, FRAMES + CAST) for k in ("fx", "fy") for v in (0.0, -1.0, NAN, INF)]
BAD += [("trunc %r" % v, dict(trunc=v), PARAMS) for v in (-0.001, NAN, INF)]
BAD += [("max_weight %r" % v, dict(max_weight=v), PARAMS) for v in (0.5, 0.0, NAN, INF)]
BAD += [("min_weight %r" % v, dict(min_weight=v), PARAMS) for v in (0.0, -1.0, NAN, INF)]
BAD += [("n_frames %r" % v, dict(n_frames=v), FRAMES) for v in (-1, R.MAX_FRAMES + 1)]
BAD += [("%s %r" % (k, v), {k: v}, FRAMES + CAST) for k in ("width", "height") for v in (-1, R.FRAME_MAX_SIDE + 1)]
BAD += [("pose_direction %r" % v, dict(pose_direction=v), PARAMS) for v in (2, -1)]
BAD += [("capacity -1", dict(capacity=-1), OUTPUT), ("triangle_capacity -1", dict(triangle_capacity=-1), MESH)]
BAD += [("zmin %r" % v, dict(zmin=v), CAST) for v in (0.0, -0.05, NAN, INF)]
BAD += [("max_steps %r" % v, dict(max_steps=v), CAST) for v in (0, -1, 16384 + 1)]
BAD += [("a colour volume off its 16-byte alignment by %d" % v, dict(color_offset=v), COLOR) for v in (4, 8)]
BAD += [("the cloud's host form with a triangle capacity", dict(triangle_capacity=1), ("fuse",))]
NULLS = {"vol": ALL, "volume": ALL[1:5], "color": COLOR, "params": PARAMS, "frames": FRAMES, "bgr": FRAMES, "poses": FRAMES, "pose": CAST,
         "ray_params": CAST, "n_out": OUTPUT, "out_xyz": OUTPUT, "out_rgb": OUTPUT, "n_triangles": ("mesh",), "out_triangles": MESH}


class Outputs:
    """Host arrays in every slot a call writes (a refused call must not look at them), filled with a pattern; untouched() compares."""

    def __init__(self):
        self.volume = np.full(4 * 3 * 2 * 2, -7, F); self.color = np.full(4 * 3 * 2 * 4 + 4, -7, F); self.counts = np.full(R.MAX_FRAMES + 1, -7, np.int64)
        self.xyz = np.full((8, 3), -7, F); self.normals = np.full((8, 3), -7, F); self.rgb = np.full((8, 3), -7, F)
        self.n_out = np.full(1, -7, np.int32); self.tri = np.full((8, 3), -7, np.int32); self.n_tri = np.full(1, -7, np.int32)
        self.depth = np.full(48, -7, F); self.vm = np.full((48, 3), -7, F); self.nm = np.full((48, 3), -7, F); self.rgb_map = np.full((48, 3), -7, F)
        self.n_hit = np.full(1, -7, np.int64)
        self.before = self.snapshot()

    def arrays(self):
        return (self.volume, self.color, self.counts, self.xyz, self.normals, self.rgb, self.n_out, self.tri, self.n_tri, self.depth, self.vm, self.nm,
                self.rgb_map, self.n_hit)

    def snapshot(self):
        return tuple(a.tobytes() for a in self.arrays())

    def untouched(self):
        return self.snapshot() == self.before


def address(x):
    return x if isinstance(x, int) else x.ctypes.data


def color_call(tdv, which, ctx, o, null=(), buffers=None, **kw):
    """One entry point on GOOD's arguments with kw replaced and the pointers named in `null` NULL.  buffers (the GPU suite): device
    pointers for volume, color, frames, bgr, out_xyz, normals, out_rgb, out_triangles, depth, vm, nm, rgb_map in place of the host arrays (the
    device forms only)."""
    g = dict(GOOD, **kw)
    lib = tdv.lib()
    host = which in ("fuse", "fuse_mesh")
    b = {} if host else (buffers or {})
    vol = tdv.TsdfVolumeC((C.c_float * 3)(0.0, 0.0, 0.3), g["voxel_length"], g["nx"], g["ny"], g["nz"])
    prm = tdv.TsdfParamsC(g["trunc"], g["max_weight"], g["zmax"], g["min_weight"], g["pose_direction"])
    rp = tdv.TsdfRaycastParamsC(g["zmin"], g["max_steps"])
    raw = np.full((R.MAX_FRAMES + 1) * 8 * 6, 3000, np.uint16)
    img = np.full((R.MAX_FRAMES + 1) * 8 * 6 * 3, 100, np.uint8)
    poses = np.tile(np.eye(4, dtype=F).reshape(-1), R.MAX_FRAMES + 1)

    def ptr(name, default):
        return None if name in null else C.c_void_p(address(b.get(name, default)))

    pv = None if "vol" in null else C.byref(vol)
    pp = None if "params" in null else C.byref(prm)
    prp = None if "ray_params" in null else C.byref(rp)
    volume, frames, bgr = ptr("volume", o.volume), ptr("frames", raw), ptr("bgr", img)
    color = None if "color" in null else C.c_void_p(address(b.get("color", o.color)) + g["color_offset"])
    xyz, nrm, rgb, tri = ptr("out_xyz", o.xyz), ptr("normals", o.normals), ptr("out_rgb", o.rgb), ptr("out_triangles", o.tri)
    n_out = None if "n_out" in null else C.c_void_p(address(o.n_out))
    n_tri = None if "n_triangles" in null else C.c_void_p(address(o.n_tri))
    hp = None if "poses" in null else C.c_void_p(address(poses))
    cam = (g["width"], g["height"], C.c_float(g["scale"]), C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(3.5), C.c_float(2.5))
    if which == "reset":
        return lib.tdv_tsdf_color_reset_dev(ctx, pv, color)
    if which == "integrate":
        return lib.tdv_tsdf_integrate_color_dev(ctx, pv, volume, color, frames, bgr, g["n_frames"], *cam, hp, pp, C.c_void_p(address(o.counts)))
    if which == "extract":
        return lib.tdv_tsdf_extract_color_dev(ctx, pv, volume, color, pp, xyz, nrm, rgb, g["capacity"], n_out)
    if which == "mesh":
        return lib.tdv_tsdf_extract_mesh_color_dev(ctx, pv, volume, color, pp, xyz, nrm, rgb, g["capacity"], n_out, tri, g["triangle_capacity"], n_tri)
    if which == "raycast":
        pose = None if "pose" in null else C.c_void_p(address(poses))
        return lib.tdv_tsdf_raycast_color_dev(ctx, pv, volume, color, g["width"], g["height"], *cam[3:], pose, pp, prp,
                                              C.c_void_p(address(b.get("depth", o.depth))), C.c_void_p(address(b.get("vm", o.vm))),
                                              C.c_void_p(address(b.get("nm", o.nm))), C.c_void_p(address(b.get("rgb_map", o.rgb_map))),
                                              C.c_void_p(address(o.n_hit)))
    if which == "fuse":                                                            # the cloud: no triangle output at all
        return lib.tdv_tsdf_fuse_color(ctx, pv, frames, bgr, g["n_frames"], *cam, hp, pp, xyz, nrm, rgb, g["capacity"], n_out, None,
                                       g["triangle_capacity"] if "triangle_capacity" in kw else 0, None)
    return lib.tdv_tsdf_fuse_color(ctx, pv, frames, bgr, g["n_frames"], *cam, hp, pp, xyz, nrm, rgb, g["capacity"], n_out, tri, g["triangle_capacity"],
                                   C.c_void_p(address(o.n_tri)))


@pytest.mark.parametrize("case", range(len(BAD)), ids=[b[0] for b in BAD])
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_tsdf_color.py refuses each bad argument on one."""
    o = Outputs()
    what, kw, where = BAD[case]
    for which in where:
        assert color_call(tdv, which, None, o, **kw) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


def test_null_pointers(tdv):
    o = Outputs()
    for what, where in NULLS.items():
        for which in where:
            assert color_call(tdv, which, None, o, null=(what,)) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against what the rules promise
def plane(bytes_bgr, max_weight=255.0):
    """len(bytes_bgr) frames of the front-on plane of tests/test_tsdf_abi.py, frame k painted (B, G, R) = bytes_bgr[k] throughout."""
    n = len(bytes_bgr)
    frames = np.full((n, 48, 64), PLANE_RAW, np.uint16)
    images = np.broadcast_to(np.asarray(bytes_bgr, np.uint8)[:, None, None, :], (n, 48, 64, 3))
    return K.integrate(PLANE_VOL, R.reset(PLANE_VOL), K.reset(PLANE_VOL), frames, images, np.tile(np.eye(4, dtype=F), (n, 1, 1)), PLANE_INTR,
                       max_weight=max_weight)


def test_running_mean_of_constant_colours_by_hand():
    """Frames of one colour each on the front-on plane.  By T21, from (0, 0):
      R bytes 255, 255, 255, 255: 1, (1*1 + 1) / 2 = 1, (1*2 + 1) / 3 = 1, (1*3 + 1) / 4 = 1 - every step exact.
      G bytes 0, 0, 0, 0: 0 throughout.
      B bytes 255, 0, 0, 255: 1; (1*1 + 0) / 2 = 0.5; (0.5*2 + 0) / 3 = fl(1/3) = 0x3EAAAAAB, above 1/3 by 9.9e-9; fl(1/3)*3 = 1 + 3e-8, which
        rounds to 1 (half an ulp of 1 is 6e-8), so (1 + 1) / 4 = 0.5.
    wc = 1, 2, 3, 4, and where the pair volume was not updated the quad stays (0, 0, 0, 0).  With max_weight = 2 the third frame finds wc = 2:
    B = (0.5*2 + 0) / 3 = fl(1/3), wc = min(3, 2) = 2, and the fourth gives (fl(1/3)*2 + 1) / 3 with wc = 2."""
    bgr = [(255, 0, 255), (0, 0, 255), (0, 0, 255), (255, 0, 255)]
    third = F(1.0) / F(3.0)
    assert third.view(np.uint32) == 0x3EAAAAAB and F(third * F(3.0)) == F(1.0)
    expect = {1: (1.0, 0.0, 1.0), 2: (1.0, 0.0, 0.5), 3: (1.0, 0.0, third), 4: (1.0, 0.0, 0.5)}
    for n in (1, 2, 3, 4):
        buf, col, counts = plane(bgr[:n])
        seen = buf[..., 1] > 0
        assert seen.sum() == 9 * PLANE_VOL.nx * PLANE_VOL.ny and (counts == seen.sum()).all()
        assert (col[seen] == np.array(expect[n] + (n,), F)).all(), (n, col[seen][0])
        assert (col[~seen] == 0).all() and (col[..., 3] == buf[..., 1]).all()
    buf, col, _ = plane(bgr, max_weight=2.0)
    seen = buf[..., 1] > 0
    last = F(F(third * F(2.0)) + F(1.0)) / F(3.0)
    assert (col[seen] == np.array([1.0, 0.0, last, 2.0], F)).all(), col[seen][0]
    # any byte: the mean of n equal samples c stays within 3 n u c of c, as the pair volume's does of t (tests/test_tsdf_abi.py)
    for byte in (1, 51, 128, 254):
        c = float(K.unit_colour(byte))
        buf, col, _ = plane([(byte, byte, byte)] * 7)
        seen = col[..., 3] > 0
        assert (col[seen][:, 3] == 7).all() and np.abs(col[seen][:, :3].astype(np.float64) - c).max() <= 3 * 7 * U * c, byte
    xyz, _, key, rgb = K.extract(PLANE_VOL, buf, col)
    assert len(key) == PLANE_VOL.nx * PLANE_VOL.ny and (K.crossing_classes(PLANE_VOL, buf, col) == 2).all()
    assert np.abs(rgb.astype(np.float64) - c).max() <= (3 * 7 + 5) * U * c         # T23 between two equal colours: five more roundings


@pytest.fixture(scope="module")
def small():
    s = Cs.small_scene((33, 17, 21), 3)
    return dict(s, images=Cc.random_images(s["frames"]))


def test_frame_order_and_split_calls(small):
    vol, fr, im, po, intr = small["vol"], small["frames"], small["images"], small["poses"], small["intr"]
    start = (R.reset(vol), K.reset(vol))
    whole = K.integrate(vol, *start, fr, im, po, intr, max_weight=1.5)
    a = K.integrate(vol, *start, fr[:1], im[:1], po[:1], intr, max_weight=1.5)
    ab = K.integrate(vol, a[0], a[1], fr[1:2], im[1:2], po[1:2], intr, max_weight=1.5)
    abc = K.integrate(vol, ab[0], ab[1], fr[2:], im[2:], po[2:], intr, max_weight=1.5)
    assert whole[0].tobytes() == abc[0].tobytes() and whole[1].tobytes() == abc[1].tobytes()
    assert (whole[2] == [a[2][0], ab[2][0], abc[2][0]]).all()
    a_bc = K.integrate(vol, a[0], a[1], fr[1:], im[1:], po[1:], intr, max_weight=1.5)
    assert a_bc[1].tobytes() == whole[1].tobytes()
    acb = K.integrate(vol, *start, fr[[0, 2, 1]], im[[0, 2, 1]], po[[0, 2, 1]], intr, max_weight=1.5)
    assert acb[1].tobytes() != whole[1].tobytes()                                  # with the weight capped at 1.5 the order shows
    same_depth_other_colours = K.integrate(vol, *start, fr, im[[1, 2, 0]], po, intr, max_weight=1.5)
    assert same_depth_other_colours[0].tobytes() == whole[0].tobytes() and same_depth_other_colours[1].tobytes() != whole[1].tobytes()
    assert a[1].tobytes() != K.reset(vol).tobytes()


def test_channels_stay_in_the_unit_interval(small):
    """T21's claim, on random bytes that include 0 and 255, with integer and non-integer weight caps."""
    vol = small["vol"]
    assert small["images"].min() == 0 and small["images"].max() == 255
    for max_weight in (255.0, 2.0, 1.5, 1.0):
        buf, col = R.reset(vol), K.reset(vol)
        for _ in range(3):                                                         # nine updates of the voxels every frame sees
            buf, col, _ = K.integrate(vol, buf, col, small["frames"], small["images"], small["poses"], small["intr"], max_weight=max_weight)
        seen = col[..., 3] > 0
        assert seen.sum() > 2000 and col[..., 3].max() == min(9.0, max_weight)
        assert col[..., :3].min() >= 0.0 and col[..., :3].max() <= 1.0, (max_weight, col[..., :3].min(), col[..., :3].max())
        rgb = K.extract(vol, buf, col)[3]
        assert len(rgb) > 100 and rgb.min() >= 0.0 and rgb.max() <= 1.0


def test_colour_weight_is_its_own(small):
    """Plain and coloured calls on one volume: w counts every frame, wc the coloured ones."""
    vol, fr, im, po, intr = small["vol"], small["frames"], small["images"], small["poses"], small["intr"]
    buf, _ = R.integrate(vol, R.reset(vol), fr[:1], po[:1], intr)
    buf, col, _ = K.integrate(vol, buf, K.reset(vol), fr[1:2], im[1:2], po[1:2], intr)
    buf, _ = R.integrate(vol, buf, fr[2:], po[2:], intr)
    all_three, _ = R.integrate(vol, R.reset(vol), fr, po, intr)
    assert buf.tobytes() == all_three.tobytes()
    w, wc = buf[..., 1], col[..., 3]
    assert w.max() == 3 and wc.max() == 1 and (wc <= w).all() and ((w == 3) & (wc == 1)).sum() > 1000 and ((w > 0) & (wc == 0)).sum() > 0
    classes = K.crossing_classes(vol, buf, col)
    assert (classes == 2).sum() > 100                                              # ... and the crossings take what colour there is
    alone = K.integrate(vol, R.reset(vol), K.reset(vol), fr[1:2], im[1:2], po[1:2], intr)[1]
    assert col.tobytes() == alone.tobytes()                                        # the colour volume does not know of the plain calls


def test_ramp_accuracy():
    """The part painted with Cc.ramp, four views, 65 x 33 x 17 voxels of 1 mm.  A crossing lies between two voxel centres one voxel_length
    apart; each voxel's colour is a mean of pixels whose surface points lie, seen from the camera, within half a pixel of the voxel's
    centre, and the voxel's centre is within the cell's diagonal, sqrt(3) voxel_length, of the crossing: a colour at the crossing comes
    from surface points within sqrt(3) voxel_length + one pixel's footprint, distance / f, of it, over which a linear texture changes by at
    most |gradient| times that; the byte costs at most 1/255 (half of it by rounding, the rest covers the f32 roundings)."""
    s = Cs.small_scene((65, 33, 17), 4)
    vol, intr = s["vol"], s["intr"]
    images = Cc.ramp_images(s["frames"], s["poses"], intr)
    xyz, _, rgb = K.fuse(vol, s["frames"], images, s["poses"], intr)
    buf, col, _ = K.integrate(vol, R.reset(vol), K.reset(vol), s["frames"], images, s["poses"], intr)
    assert (K.crossing_classes(vol, buf, col) == 2).all()                          # every observed voxel was coloured with its depth
    footprint = 0.3 / intr[1]                                                      # the scene's distance over f: 1.3 mm
    reach = np.sqrt(3.0) * float(vol.L) + footprint
    truth = Cc.ramp(xyz[:, :2].astype(np.float64))
    err = np.abs(rgb.astype(np.float64) - truth)
    bound = np.linalg.norm(Cc.RAMP_GRADIENT, axis=1) * reach + 1.0 / 255.0
    print("ramp: %d crossings; largest |fused - texture| per channel %s, bound %s; median %s" % (len(xyz), err.max(0), bound, np.median(err, 0)))
    assert len(xyz) > 2000 and (err <= bound[None, :]).all(), (err.max(0), bound)
