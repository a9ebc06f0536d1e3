"""Coloured TSDF fusion on the device (include/tdv_hip.h: tdv_tsdf_integrate_color_dev; csrc/tsdf.hip, csrc/tsdf_raycast.hip) against the
restatement (tests/tsdf_color_restatement.py), byte for byte: the colour volume and the pair volume after the integrate calls, h_n_updated,
the counts, the points, normals, colours and triangles, and the ray cast's depth, vertex map, normal map, colour map and hit count.  The
pair volume, points, normals, triangles and maps are also held to the plain calls on the same context.  Volume sides stand on the edges of
a wave's run of 64 voxels and of the tile; the frame counts on 0, 1, a split and TDV_TSDF_MAX_FRAMES; both pose directions, a max_weight
that is reached, plain and coloured calls interleaved, a hand-seeded colour volume with uncoloured patches across the surface (every class
of T23), the output forms, ray casts of images that are no multiple of the 8 x 8 tile from a view that reaches the rim of the coloured
region, the host form with and without triangles, every bad argument on a live context, and the fused cloud handed to Colored ICP.
Scenes are tests/tsdf_cases.py's small renders with tests/tsdf_color_cases.py's random images, 64 x 48 to 160 x 120 pixels."""
import numpy as np
import pytest

import tsdf_color_cases as Cc
import tsdf_color_restatement as K
import tsdf_mesh_restatement as M
import tsdf_restatement as R
from state_cases import Env
from test_gpu_tsdf import chunks, scene
from test_tsdf_color_abi import BAD, NULLS, TDV_ERR_BAD_ARG, Outputs, color_call

pytestmark = pytest.mark.gpu
F = np.float32
TX, TY, TZ = R.TILE
PATTERN = 0xA5A5A5A5
_IMAGES, _SEEDED = {}, []


def cscene(dims, n_frames=2, size=(96, 72), f=230.0):
    """tests/test_gpu_tsdf.py's scene with random images for its frames, made once per shape and never modified."""
    s = scene(dims, n_frames, size, f)
    key = (n_frames, size, f)
    if key not in _IMAGES:
        _IMAGES[key] = Cc.random_images(s["frames"])
        _IMAGES[key].setflags(write=False)
    return dict(s, images=_IMAGES[key])


def kinds_of(n_calls, kinds):
    return "c" * n_calls if kinds is None else kinds


def restated(s, splits=None, kinds=None, start=None, **params):
    """The restatement's volumes after the calls (kinds: 'c' a coloured call, 'p' a plain one), its cloud with colours and its mesh."""
    vol = s["vol"]
    buf, col = (R.reset(vol), K.reset(vol)) if start is None else start
    counts, calls = [], chunks(len(s["frames"]), splits)
    for (a, e), kind in zip(calls, kinds_of(len(calls), kinds)):
        if kind == "c":
            buf, col, c = K.integrate(vol, buf, col, s["frames"][a:e], s["images"][a:e], s["poses"][a:e], s["intr"], **params)
        else:
            buf, c = R.integrate(vol, buf, s["frames"][a:e], s["poses"][a:e], s["intr"], **params)
        counts.append(c)
    xyz, nrm, _, rgb = K.extract(vol, buf, col, params.get("min_weight", 1.0))
    tri = M.mesh(vol, buf, params.get("min_weight", 1.0))[3]
    return dict(volume=buf, color=col, counts=np.concatenate(counts) if counts else np.zeros(0, np.int64), n=len(xyz), xyz=xyz, normals=nrm, rgb=rgb,
                nt=len(tri), triangles=tri)


def device_volumes(tdv, ctx, env, s, splits=None, kinds=None, start=None, **params):
    """(the struct, the pair volume's tensor, the colour volume's tensor, the counts) after the calls."""
    vol = s["vol"]
    cvol = tdv.tsdf_volume_struct(*vol.args())
    if start is None:
        d_vol, d_col = env.out(vol.voxels * 2, F), env.out(vol.voxels * 4, F)
        ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
        ctx.tsdf_color_reset_dev(cvol, d_col.data_ptr())
    else:
        env.up(start[0]); env.up(start[1])
        d_vol, d_col = env.keep[-2:]
    h, w = s["frames"].shape[1:]
    counts, calls = [], chunks(len(s["frames"]), splits)
    for (a, e), kind in zip(calls, kinds_of(len(calls), kinds)):
        if kind == "c":
            counts.append(ctx.tsdf_integrate_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), env.up(s["frames"][a:e]), env.up(s["images"][a:e]),
                                                       s["poses"][a:e], w, h, *s["intr"], **params))
        else:
            counts.append(ctx.tsdf_integrate_dev(cvol, d_vol.data_ptr(), env.up(s["frames"][a:e]), s["poses"][a:e], w, h, *s["intr"], **params))
    return cvol, d_vol, d_col, (np.concatenate(counts) if counts else np.zeros(0, np.int64))


def device(tdv, ctx, env, s, splits=None, kinds=None, start=None, normals=True, **params):
    """The coloured calls' outputs; on the way the plain calls on the same context, whose bytes the coloured ones must give."""
    vol = s["vol"]
    cvol, d_vol, d_col, counts = device_volumes(tdv, ctx, env, s, splits, kinds, start, **params)
    pv, pc = d_vol.data_ptr(), d_col.data_ptr()
    n, fits = ctx.tsdf_extract_color_dev(cvol, pv, pc, None, None, None, 0, **params)                      # the query
    assert fits == (n == 0)
    ox, on, oc = env.out(3 * n, F), env.out(3 * n, F), env.out(3 * n, F)
    assert ctx.tsdf_extract_color_dev(cvol, pv, pc, ox.data_ptr(), on.data_ptr() if normals else None, oc.data_ptr(), n, **params) == (n, True)
    px, pn = env.out(3 * n, F), env.out(3 * n, F)
    assert ctx.tsdf_extract_dev(cvol, pv, px.data_ptr(), pn.data_ptr() if normals else None, n, **params) == (n, True)
    got = dict(n=n, counts=counts, xyz=env.get(ox, 3 * n, F).reshape(-1, 3), normals=env.get(on, 3 * n, F).reshape(-1, 3) if normals else None,
               rgb=env.get(oc, 3 * n, F).reshape(-1, 3))
    assert got["xyz"].tobytes() == env.get(px, 3 * n, F).tobytes(), "the coloured call's points are not the plain call's"
    if normals:
        assert got["normals"].tobytes() == env.get(pn, 3 * n, F).tobytes(), "the coloured call's normals are not the plain call's"
    else:
        assert (env.get(on, 3 * n, np.uint32) == PATTERN).all()
    # the mesh
    nv, nt, fits = ctx.tsdf_extract_mesh_color_dev(cvol, pv, pc, None, None, None, 0, None, 0, **params)
    assert nv == n and fits == (nv == 0)
    mx, mn, mc, mt = env.out(3 * nv, F), env.out(3 * nv, F), env.out(3 * nv, F), env.out(3 * nt, np.int32)
    assert ctx.tsdf_extract_mesh_color_dev(cvol, pv, pc, mx.data_ptr(), mn.data_ptr() if normals else None, mc.data_ptr(), nv, mt.data_ptr(), nt,
                                           **params) == (nv, nt, True)
    pt = env.out(3 * nt, np.int32)
    assert ctx.tsdf_extract_mesh_dev(cvol, pv, px.data_ptr(), pn.data_ptr() if normals else None, nv, pt.data_ptr(), nt, **params) == (nv, nt, True)
    got.update(nt=nt, triangles=env.get(mt, 3 * nt, np.int32).reshape(-1, 3))
    assert got["triangles"].tobytes() == env.get(pt, 3 * nt, np.int32).tobytes(), "the coloured mesh's triangles are not the plain call's"
    assert env.get(mx, 3 * nv, F).tobytes() == got["xyz"].tobytes() and env.get(mc, 3 * nv, F).tobytes() == got["rgb"].tobytes()
    if normals:
        assert env.get(mn, 3 * nv, F).tobytes() == got["normals"].tobytes()
    got.update(volume=env.get(d_vol, vol.voxels * 2, F).reshape(vol.nz, vol.ny, vol.nx, 2),
               color=env.get(d_col, vol.voxels * 4, F).reshape(vol.nz, vol.ny, vol.nx, 4))
    return got


def same(ref, got, what):
    assert (got["n"], got["nt"]) == (ref["n"], ref["nt"]), (what, got["n"], got["nt"], ref["n"], ref["nt"])
    assert np.array_equal(got["counts"], ref["counts"]), (what, got["counts"], ref["counts"])
    for k in ("volume", "color", "xyz", "normals", "rgb", "triangles"):
        if got[k] is None:
            continue
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].shape, ref[k].shape)
        if got[k].tobytes() != ref[k].tobytes():
            bad = np.argwhere(got[k].view(np.uint32) != ref[k].view(np.uint32))
            first = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: %r, restated %r" % (what, k, len(bad), first, got[k][first], ref[k][first]))


def held(tdv, ctx, s, what, env=None, splits=None, kinds=None, start=None, normals=True, **params):
    ref = restated(s, splits, kinds, start, **params)
    same(ref, device(tdv, ctx, env or Env(ctx), s, splits, kinds, start, normals, **params), what)
    return ref


# ---------------------------------------------------------------- sides and tiles, frames
SIDES = [(1, 33, 17), (63, 9, 7), (64, 8, 8), (65, 7, 9), (33, TY + 1, TZ), (1, 1, 1), (65, 33, 17)]


@pytest.mark.parametrize("dims", SIDES, ids=["%dx%dx%d" % d for d in SIDES])
def test_sides_and_tiles(tdv, ctx, dims):
    ref = held(tdv, ctx, cscene(dims), dims)
    if min(dims) > 1:
        assert ref["n"] > 20 and (ref["counts"] > 0).all() and (ref["color"][..., 3] > 0).sum() > 100, (ref["n"], ref["counts"])


def test_the_large_frames(tdv, ctx):
    s = cscene((65, 33, 17), 3, size=(160, 120), f=420.0)
    ref = held(tdv, ctx, s, "65x33x17, 160x120")
    key = R.extract(s["vol"], ref["volume"])[2]
    assert ref["n"] > 1000 and ref["nt"] > 1000 and set((key % 3).tolist()) == {0, 1, 2}
    assert ref["color"][..., :3].min() >= 0.0 and ref["color"][..., :3].max() <= 1.0 and ref["rgb"].min() >= 0.0 and ref["rgb"].max() <= 1.0


@pytest.mark.parametrize("n,splits", [(0, None), (1, None), (5, None), (5, (2, 3)), (R.MAX_FRAMES, None)])
def test_frame_counts(tdv, ctx, n, splits):
    s = cscene((65, 33, 17), n, size=(64, 48), f=150.0)
    ref = held(tdv, ctx, s, (n, splits), splits=splits)
    assert len(ref["counts"]) == n and (n == 0) == (ref["n"] == 0)
    if splits:                                                                     # ... and the split is the one call, by the rules alone
        whole = restated(s)
        assert whole["color"].tobytes() == ref["color"].tobytes() and whole["volume"].tobytes() == ref["volume"].tobytes()
    if n:
        assert ref["color"][..., 3].max() == n and (ref["color"][..., 3] == ref["volume"][..., 1]).all()
    else:
        assert not ref["color"].any()


def test_both_pose_directions(tdv, ctx):
    s = cscene((65, 33, 17), 3)
    a = held(tdv, ctx, s, "model to camera", pose_direction=R.MODEL_TO_CAMERA)
    inv = dict(s, poses=np.linalg.inv(s["poses"].astype(np.float64)).astype(F))
    b = held(tdv, ctx, inv, "camera poses", pose_direction=R.SOURCE_ONTO_TARGET)
    assert abs(a["n"] - b["n"]) < 0.05 * a["n"]                                    # the same fusion, other roundings


def test_max_weight_reached(tdv, ctx):
    s = cscene((65, 33, 17), 5)
    ref = held(tdv, ctx, s, "max_weight 2", max_weight=2.0)
    assert ref["color"][..., 3].max() == 2 and restated(s)["color"][..., 3].max() == 5
    assert ref["color"].tobytes() != restated(s)["color"].tobytes()
    held(tdv, ctx, s, "max_weight 2.5, trunc 2 mm, min_weight 2", max_weight=2.5, trunc=0.002, min_weight=2.0)


def test_plain_and_coloured_calls_interleaved(tdv, ctx):
    s = cscene((65, 33, 17), 5)
    ref = held(tdv, ctx, s, "coloured, plain, coloured", splits=(2, 1, 2), kinds="cpc")
    w, wc = ref["volume"][..., 1], ref["color"][..., 3]
    assert w.max() == 5 and wc.max() == 4 and (wc <= w).all() and (wc < w).any()
    assert ref["volume"].tobytes() == restated(s, kinds="p")["volume"].tobytes()   # the pair volume does not know which calls had colour
    ref = held(tdv, ctx, s, "plain first", splits=(3, 2), kinds="pc")
    assert ref["color"][..., 3].max() == 2


# ---------------------------------------------------------------- a hand-seeded colour volume: every class of T23
def seeded():
    """The five-frame fusion's volumes with the colour taken away (wc = 0) in slabs across the surface along each axis and in a sprinkling
    of single voxels, and the channels replaced by seeded random values in [0, 1] - 0 and 1 among them.  Made once, never modified."""
    if _SEEDED:
        return _SEEDED[0]
    s = cscene((65, 33, 17), 5)
    ref = restated(s)
    rng = np.random.default_rng(23)
    col = ref["color"].copy()
    col[..., :3] = rng.choice(np.concatenate([np.array([0.0, 1.0], F), rng.random(61).astype(F)]), col[..., :3].shape)
    col[:, :, 10:14, 3] = 0
    col[:, 20:23, :, 3] = 0
    col[5, :, 40:52, 3] = 0
    col[..., 3] = np.where(rng.random(col[..., 3].shape) < 0.15, F(0), col[..., 3])
    col.setflags(write=False); ref["volume"].setflags(write=False)
    _SEEDED.append((s, ref["volume"], col))
    return _SEEDED[0]


def test_seeded_colour_volume_has_every_class(tdv, ctx):
    s, buf, col = seeded()
    classes = K.crossing_classes(s["vol"], buf, col)
    counts = [int((classes == k).sum()) for k in (0, 1, 2)]
    assert min(counts) > 50, counts                                                # neither end, one end, both ends coloured
    ref = held(tdv, ctx, dict(s, frames=s["frames"][:0], images=s["images"][:0], poses=s["poses"][:0]), "seeded", start=(buf, col))
    assert (ref["rgb"][classes == 0] == 0).all() and ref["rgb"].min() >= 0.0 and ref["rgb"].max() <= 1.0
    a, b = K.crossing_ends(s["vol"], R.extract(s["vol"], buf)[2])
    q = col.reshape(-1, 4)
    one = classes == 1
    end = np.where((q[a, 3] > 0)[:, None], q[a, :3], q[b, :3])
    assert ref["rgb"][one].tobytes() == end[one].tobytes()                         # the coloured end's colour, untouched
    held(tdv, ctx, s, "frames onto the seeded volumes", start=(buf, col), max_weight=3.0)


# ---------------------------------------------------------------- output forms
def test_output_forms(tdv, ctx):
    s = cscene((65, 33, 17), 2)
    ref = held(tdv, ctx, s, "no normals", normals=False)
    n, nt = ref["n"], ref["nt"]
    env = Env(ctx)
    cvol = tdv.tsdf_volume_struct(*s["vol"].args())
    env.up(ref["volume"]); env.up(ref["color"])
    d_vol, d_col = env.keep[-2:]
    for capacity in (n - 1, 0):
        ox, on, oc, ot = env.out(3 * n, F), env.out(3 * n, F), env.out(3 * n, F), env.out(3 * nt, np.int32)
        assert ctx.tsdf_extract_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), ox.data_ptr(), on.data_ptr(), oc.data_ptr(), capacity) == (n, False)
        assert ctx.tsdf_extract_mesh_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), ox.data_ptr(), on.data_ptr(), oc.data_ptr(), capacity,
                                               ot.data_ptr(), nt) == (n, nt, False)
        assert ctx.tsdf_extract_mesh_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), ox.data_ptr(), on.data_ptr(), oc.data_ptr(), n,
                                               ot.data_ptr(), nt - 1) == (n, nt, False)
        for t in (ox, on, oc):
            assert (env.get(t, 3 * n, np.uint32) == PATTERN).all()                 # no row written
        assert (env.get(ot, 3 * nt, np.uint32) == PATTERN).all()
    ox, on, oc = env.out(3 * (n + 2), F), env.out(3 * (n + 2), F), env.out(3 * (n + 2), F)
    assert ctx.tsdf_extract_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), ox.data_ptr(), on.data_ptr(), oc.data_ptr(), n + 2) == (n, True)
    for t, k in ((ox, "xyz"), (on, "normals"), (oc, "rgb")):
        x = env.get(t, 3 * (n + 2), F)
        assert x[:3 * n].tobytes() == ref[k].tobytes() and (x[3 * n:].view(np.uint32) == PATTERN).all()      # nothing beyond
    assert env.get(d_vol, s["vol"].voxels * 2, F).tobytes() == ref["volume"].tobytes()                      # extraction reads only
    assert env.get(d_col, s["vol"].voxels * 4, F).tobytes() == ref["color"].tobytes()


# ---------------------------------------------------------------- the ray cast
ZMAX = 0.5
MAPS = ("depth", "vertex_map", "normal_map", "rgb_map")


def cast_both(tdv, ctx, env, vol, d_vol, d_col, pose, size, cam, **params):
    """(the coloured call's maps and count, the plain call's) on the same context."""
    w, h = size
    npx = w * h
    cvol = tdv.tsdf_volume_struct(*vol.args())
    out = {k: env.out(npx * (1 if k == "depth" else 3), F) for k in MAPS}
    n = ctx.tsdf_raycast_color_dev(cvol, d_vol, d_col, pose, w, h, *cam, out["depth"].data_ptr(), out["vertex_map"].data_ptr(),
                                   out["normal_map"].data_ptr(), out["rgb_map"].data_ptr(), **params)
    got = {k: env.get(out[k], npx * (1 if k == "depth" else 3), F).reshape((h, w) if k == "depth" else (h, w, 3)) for k in MAPS}
    plain = {k: env.out(npx * (1 if k == "depth" else 3), F) for k in MAPS[:3]}
    m = ctx.tsdf_raycast_dev(cvol, d_vol, pose, w, h, *cam, plain["depth"].data_ptr(), plain["vertex_map"].data_ptr(), plain["normal_map"].data_ptr(),
                             **params)
    return dict(got, n_hit=n), dict({k: env.get(plain[k], npx * (1 if k == "depth" else 3), F) for k in MAPS[:3]}, n_hit=m)


@pytest.mark.parametrize("size,f", [((64, 48), 150.0), ((37, 29), 85.0)], ids=["64x48", "37x29"])
@pytest.mark.parametrize("direction", [R.MODEL_TO_CAMERA, R.SOURCE_ONTO_TARGET], ids=["model_to_camera", "source_onto_target"])
def test_ray_cast(tdv, ctx, size, f, direction):
    """The scan pose and a tilted view of the seeded volumes: the view crosses the uncoloured slabs, so rays hit on both sides of the rim."""
    s, buf, col = seeded()
    vol = s["vol"]
    cam = (f, 1.05 * f, (size[0] - 1) / 2.0, (size[1] - 1) / 2.0 + 0.25)
    env = Env(ctx)
    d_vol, d_col = env.up(buf), env.up(col)
    for k in (0, 2):
        view = s["poses"][k]
        pose = np.asarray(view, F) if direction == R.MODEL_TO_CAMERA else np.linalg.inv(np.asarray(view, np.float64)).astype(F)
        ref = K.raycast(vol, buf, col, pose, size, cam, zmax=ZMAX, pose_direction=direction)
        hit = ref["depth"] != 0
        coloured = (ref["rgb_map"] != 0).any(-1)
        assert ref["n_hit"] > 100 and (hit & coloured).sum() >= 1 and (hit & ~coloured).sum() >= 1 and not (coloured & ~hit).any(), \
            (ref["n_hit"], (hit & coloured).sum(), (hit & ~coloured).sum())
        got, plain = cast_both(tdv, ctx, env, vol, d_vol, d_col, pose, size, cam, zmax=ZMAX, pose_direction=direction)
        for m in MAPS:
            assert got[m].shape == ref[m].shape and got[m].dtype == ref[m].dtype, (k, m)
            if got[m].tobytes() != ref[m].tobytes():
                bad = np.argwhere(got[m].view(np.uint32) != ref[m].view(np.uint32))
                raise AssertionError("view %d: %s differs in %d places, first at %s: %r, restated %r" % (k, m, len(bad), tuple(bad[0]),
                                                                                                        got[m][tuple(bad[0])], ref[m][tuple(bad[0])]))
        assert got["n_hit"] == ref["n_hit"] == plain["n_hit"]
        for m in MAPS[:3]:
            assert got[m].tobytes() == plain[m].tobytes(), (k, m, "the coloured call's map is not the plain call's")
    # the optional outputs: the colour map alone, and no colour map at all
    w, h = size
    cvol = tdv.tsdf_volume_struct(*vol.args())
    only = env.out(3 * w * h, F)
    assert ctx.tsdf_raycast_color_dev(cvol, d_vol, d_col, pose, w, h, *cam, None, None, None, only.data_ptr(), want_count=False, zmax=ZMAX,
                                      pose_direction=direction) is None
    assert env.get(only, 3 * w * h, F).tobytes() == ref["rgb_map"].tobytes()
    dd = env.out(w * h, F)
    assert ctx.tsdf_raycast_color_dev(cvol, d_vol, d_col, pose, w, h, *cam, dd.data_ptr(), None, None, None, zmax=ZMAX,
                                      pose_direction=direction) == ref["n_hit"]
    assert env.get(dd, w * h, F).tobytes() == ref["depth"].tobytes()
    guard = env.out(4, F)
    assert ctx.tsdf_raycast_color_dev(cvol, d_vol, d_col, pose, 0, 0, *cam, guard.data_ptr(), guard.data_ptr(), guard.data_ptr(), guard.data_ptr(),
                                      zmax=ZMAX, pose_direction=direction) == 0
    assert env.get(guard, 4, np.uint32).tolist() == [PATTERN] * 4


# ---------------------------------------------------------------- the host form and the conveniences
def test_host_form_and_conveniences(tdv, ctx):
    s = cscene((65, 33, 17), 3)
    ref = restated(s, max_weight=2.0)
    args = (s["frames"], s["images"], s["poses"], s["intr"], s["vol"].args())
    xyz, nrm, rgb = ctx.tsdf_fuse_color(*args, max_weight=2.0)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes() and rgb.tobytes() == ref["rgb"].tobytes()
    xyz, nrm, rgb = ctx.tsdf_fuse_color(*args, normals=False, max_weight=2.0)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm is None and rgb.tobytes() == ref["rgb"].tobytes()
    xyz, nrm, tri, rgb = ctx.tsdf_fuse_color(*args, triangles=True, max_weight=2.0)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes() and rgb.tobytes() == ref["rgb"].tobytes()
    assert tri.tobytes() == ref["triangles"].tobytes() and len(tri) > 500
    cx, cn, ct, cc = ctx.tsdf_fuse_color(*args, triangles=True, compact=True, max_weight=2.0)
    used = np.zeros(ref["n"], bool); used[ref["triangles"].reshape(-1)] = True
    assert 0 < used.sum() <= ref["n"] and cx.tobytes() == ref["xyz"][used].tobytes() and cc.tobytes() == ref["rgb"][used].tobytes()
    assert np.array_equal(cx[ct], ref["xyz"][ref["triangles"]]) and cn.tobytes() == ref["normals"][used].tobytes()
    empty = ctx.tsdf_fuse_color(s["frames"][:0], s["images"][:0], s["poses"][:0], s["intr"], s["vol"].args(), triangles=True)
    assert [e.shape for e in empty] == [(0, 3)] * 4
    volume = ctx.tsdf_volume(*s["vol"].args())
    color = ctx.tsdf_color_volume(volume[0])
    assert tuple(color.shape) == (s["vol"].voxels, 4) and not color.cpu().numpy().any()
    counts = ctx.tsdf_integrate_color(volume, color, s["frames"], s["images"], s["poses"], s["intr"], max_weight=2.0)
    assert np.array_equal(counts, ref["counts"]) and volume[1].cpu().numpy().tobytes() == ref["volume"].tobytes()
    assert color.cpu().numpy().tobytes() == ref["color"].tobytes()
    xyz, nrm, rgb = ctx.tsdf_extract_color(volume, color)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes() and rgb.tobytes() == ref["rgb"].tobytes()
    xyz, nrm, tri, rgb = ctx.tsdf_extract_mesh_color(volume, color)
    assert xyz.tobytes() == ref["xyz"].tobytes() and tri.tobytes() == ref["triangles"].tobytes() and rgb.tobytes() == ref["rgb"].tobytes()
    cam = s["intr"][1:]
    view = ctx.tsdf_raycast_color(volume, color, s["poses"][0], 96, 72, *cam, zmax=ZMAX)
    cast = K.raycast(s["vol"], ref["volume"], ref["color"], s["poses"][0], (96, 72), cam, zmax=ZMAX)
    assert view["n_hit"] == cast["n_hit"] > 500 and all(view[m].tobytes() == cast[m].tobytes() for m in MAPS)
    ctx.tsdf_color_reset_dev(volume[0], color.data_ptr())
    ctx.synchronize()
    assert not color.cpu().numpy().any()


# ---------------------------------------------------------------- arguments
def live_buffers(env):
    """Device buffers for color_call on a live context, of the size GOOD's arguments need (the frames: of the largest n_frames tried),
    0xA5 throughout, by color_call's names."""
    sizes = dict(volume=(48, F), color=(96 + 4, F), frames=((R.MAX_FRAMES + 1) * 48, np.uint16), bgr=((R.MAX_FRAMES + 1) * 48 * 3, np.uint8),
                 out_xyz=(24, F), normals=(24, F), out_rgb=(24, F), out_triangles=(24, np.int32), depth=(48, F), vm=(144, F), nm=(144, F),
                 rgb_map=(144, F))
    tensors = {k: env.out(n, t) for k, (n, t) in sizes.items()}
    return {k: t.data_ptr() for k, t in tensors.items()}, tensors, sizes


def test_bad_arguments_on_a_live_context(tdv, ctx):
    """Every refusal of tests/test_tsdf_color_abi.py's tables with a real ctx: TDV_ERR_BAD_ARG, the host outputs and the device buffers as
    they were.  Then the same calls with nothing wrong go through."""
    env = Env(ctx)
    buffers, tensors, sizes = live_buffers(env)
    o = Outputs()
    for what, kw, where in BAD[1:]:
        for which in where:
            assert color_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == TDV_ERR_BAD_ARG, (what, which)
    for what, where in NULLS.items():
        for which in where:
            assert color_call(tdv, which, ctx._h, o, null=(what,), buffers=buffers) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()
    for k, (n, t) in sizes.items():
        assert (env.get(tensors[k], n, t).view(np.uint8) == 0xA5).all(), k
    assert color_call(tdv, "reset", ctx._h, o, buffers=buffers) == 0
    ctx.tsdf_reset_dev(tdv.tsdf_volume_struct((0.0, 0.0, 0.3), 0.001, (4, 3, 2)), buffers["volume"])
    assert color_call(tdv, "integrate", ctx._h, o, buffers=buffers) == 0 and (o.counts[:2] >= 0).all()
    assert color_call(tdv, "extract", ctx._h, o, buffers=buffers) in (0, TDV_ERR_BAD_ARG) and o.n_out[0] >= 0
    assert color_call(tdv, "mesh", ctx._h, o, buffers=buffers) in (0, TDV_ERR_BAD_ARG) and o.n_out[0] >= 0 and o.n_tri[0] >= 0
    assert color_call(tdv, "raycast", ctx._h, o, buffers=buffers) == 0 and o.n_hit[0] >= 0
    assert color_call(tdv, "fuse", ctx._h, o, capacity=0, null=("out_xyz", "out_rgb")) in (0, TDV_ERR_BAD_ARG) and o.n_out[0] >= 0
    assert color_call(tdv, "fuse_mesh", ctx._h, o, capacity=0, triangle_capacity=0, null=("out_xyz", "out_rgb", "out_triangles")) in (0, TDV_ERR_BAD_ARG)
    assert o.n_out[0] >= 0 and o.n_tri[0] >= 0
    # a NULL colour image is fine where no frame has a pixel, and with no frame at all
    assert color_call(tdv, "integrate", ctx._h, o, buffers=buffers, null=("bgr",), width=0) == 0
    assert color_call(tdv, "integrate", ctx._h, o, buffers=buffers, null=("bgr", "frames", "poses"), n_frames=0) == 0


# ---------------------------------------------------------------- the fused cloud as Colored ICP's target
def test_fused_cloud_goes_through_colored_icp(tdv, ctx):
    """The link this stage exists for: the fused rows and colours, still on the device, through color_gradients_dev and colored_icp_dev from
    the identity, the cloud against itself.  No accuracy is asserted - none has been measured."""
    s = cscene((65, 33, 17), 3)
    env = Env(ctx)
    cvol, d_vol, d_col, _ = device_volumes(tdv, ctx, env, s)
    n, _ = ctx.tsdf_extract_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), None, None, None, 0)
    ox, on, oc, og = env.out(3 * n, F), env.out(3 * n, F), env.out(3 * n, F), env.out(4 * n, F)
    assert ctx.tsdf_extract_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), ox.data_ptr(), on.data_ptr(), oc.data_ptr(), n) == (n, True)
    ctx.color_gradients_dev(ox.data_ptr(), oc.data_ptr(), on.data_ptr(), n, 20, og.data_ptr())
    res = ctx.colored_icp_dev(ox.data_ptr(), oc.data_ptr(), n, ox.data_ptr(), on.data_ptr(), og.data_ptr(), n, np.eye(4, dtype=F), 0.003, 5)
    assert n > 1000 and res.n_corr > 0 and np.isfinite(res.transformation).all()
