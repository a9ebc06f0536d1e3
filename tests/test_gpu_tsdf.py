"""TSDF fusion on the device (include/tdv_hip.h: tdv_tsdf_integrate_dev, csrc/tsdf.hip) against the restatement (tests/tsdf_restatement.py),
byte for byte: the volume buffer after the integrate calls, h_n_updated, n_out, the points and the normals.  Volume sides stand on the
edges of a wave's run of 64 voxels and of the LDS tile (TDV_TSDF_TILE_X/Y/Z minus one, exact, plus one; sides of 1), the frame counts on
0, 1 and TDV_TSDF_MAX_FRAMES and on the same frames split over calls; both pose directions, a frustum that covers part of the volume, a
view from behind, zmax inside the scene, a max_weight that is reached, a hand-seeded volume with zeros and negative zeros on one side of
a crossing, NaN poses, the output forms (no normals; capacity exact, one short, zero), the host form, and every bad argument on a live
context.  Scenes are small renders of a ReliefPart (tests/tsdf_cases.py), 64 x 48 to 160 x 120 pixels."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as Cs
import tsdf_restatement as R
from state_cases import Env
from test_tsdf_abi import BAD, NULLS, TDV_ERR_BAD_ARG, Outputs, tsdf_call

pytestmark = pytest.mark.gpu
F = np.float32
TX, TY, TZ = R.TILE
_SCENES = {}


def scene(dims, n_frames=2, size=(96, 72), f=230.0, **kw):
    """Cs.small_scene, rendered once per shape and never modified."""
    key = (tuple(dims), n_frames, size, f, tuple(sorted(kw.items())))
    if key not in _SCENES:
        s = Cs.small_scene(dims, n_frames, size, f, **kw)
        for a in (s["frames"], s["poses"]):
            a.setflags(write=False)
        _SCENES[key] = s
    return _SCENES[key]


def chunks(n, splits):
    """The frames of each call: splits = the calls' frame counts (None: one call with all of them)."""
    edges = np.concatenate([[0], np.cumsum([n] if splits is None else splits)])
    assert edges[-1] == n
    return list(zip(edges[:-1], edges[1:]))


def restated(s, splits=None, start=None, **params):
    vol = s["vol"]
    buf, counts = (R.reset(vol) if start is None else start), []
    for a, e in chunks(len(s["frames"]), splits):
        buf, c = R.integrate(vol, buf, s["frames"][a:e], s["poses"][a:e], s["intr"], **params)
        counts.append(c)
    xyz, nrm, _ = R.extract(vol, buf, params.get("min_weight", 1.0))
    return dict(volume=buf, counts=np.concatenate(counts) if counts else np.zeros(0, np.int64), n=len(xyz), xyz=xyz, normals=nrm)


def device(tdv, ctx, env, s, splits=None, start=None, normals=True, **params):
    vol = s["vol"]
    cvol = tdv.tsdf_volume_struct(*vol.args())
    if start is None:
        d_vol = env.out(vol.voxels * 2, F)
        ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
    else:
        env.up(start)
        d_vol = env.keep[-1]
    h, w = s["frames"].shape[1:]
    counts = []
    for a, e in chunks(len(s["frames"]), splits):
        counts.append(ctx.tsdf_integrate_dev(cvol, d_vol.data_ptr(), env.up(s["frames"][a:e]), s["poses"][a:e], w, h, *s["intr"], **params))
    n, fits = ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), None, None, 0, **params)
    assert fits == (n == 0)
    ox, on = env.out(3 * n, F), env.out(3 * n, F)
    m, fits = ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), ox.data_ptr(), on.data_ptr() if normals else None, n, **params)
    assert fits and m == n
    return dict(volume=env.get(d_vol, vol.voxels * 2, F).reshape(vol.nz, vol.ny, vol.nx, 2), counts=np.concatenate(counts) if counts else np.zeros(0, np.int64),
                n=n, xyz=env.get(ox, 3 * n, F).reshape(-1, 3), normals=env.get(on, 3 * n, F).reshape(-1, 3) if normals else None)


def same(ref, got, what):
    assert got["n"] == ref["n"], (what, got["n"], ref["n"])
    assert np.array_equal(got["counts"], ref["counts"]), (what, got["counts"], ref["counts"])
    for k in ("volume", "xyz", "normals"):
        if got[k] is None:
            continue
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k)
        if got[k].tobytes() != ref[k].tobytes():
            bad = np.argwhere(got[k].view(np.uint32) != ref[k].view(np.uint32))
            first = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: %r, restated %r" % (what, k, len(bad), first, got[k][first], ref[k][first]))


def held(tdv, ctx, s, what, env=None, splits=None, start=None, normals=True, **params):
    ref = restated(s, splits, start, **params)
    same(ref, device(tdv, ctx, env or Env(ctx), s, splits, start, normals, **params), what)
    return ref


# ---------------------------------------------------------------- sides and tiles
SIDES = [(1, 33, 17), (63, 9, 7), (64, 8, 8), (65, 7, 9), (129, 9, 5), (33, TY - 1, 17), (33, TY, TZ + 1), (33, TY + 1, TZ), (17, 33, TZ - 1),
         (33, 1, 17), (33, 17, 1), (1, 1, 1), (65, 33, 17)]


@pytest.mark.parametrize("dims", SIDES, ids=["%dx%dx%d" % d for d in SIDES])
def test_sides_and_tiles(tdv, ctx, dims):
    ref = held(tdv, ctx, scene(dims), dims)
    if min(dims) > 1:
        assert ref["n"] > 20 and (ref["counts"] > 0).all(), (ref["n"], ref["counts"])


def test_the_large_scene_has_every_axis(tdv, ctx):
    s = scene((65, 33, 17), 3, size=(160, 120), f=420.0)
    ref = held(tdv, ctx, s, "65x33x17, 160x120")
    key = R.extract(s["vol"], ref["volume"])[2]
    assert ref["n"] > 1000 and set((key % 3).tolist()) == {0, 1, 2}
    assert (np.abs(np.linalg.norm(ref["normals"].astype(np.float64), axis=1) - 1) < 1e-6).all()


# ---------------------------------------------------------------- frame counts
@pytest.mark.parametrize("n,splits", [(0, None), (1, None), (2, None), (5, None), (5, (2, 3)), (5, (1, 0, 4)), (R.MAX_FRAMES, None),
                                      (R.MAX_FRAMES, (1, R.MAX_FRAMES - 1))])
def test_frame_counts(tdv, ctx, n, splits):
    s = scene((65, 33, 17), n, size=(64, 48), f=150.0)
    ref = held(tdv, ctx, s, (n, splits), splits=splits)
    assert len(ref["counts"]) == n and (n == 0) == (ref["n"] == 0)
    if splits:                                                                     # ... and the split is the one call, by the rules alone
        assert restated(s)["volume"].tobytes() == ref["volume"].tobytes()
    if n:
        assert ref["volume"][..., 1].max() == n                                    # some voxel was seen in every frame


# ---------------------------------------------------------------- poses, depths, weights
def test_both_pose_directions(tdv, ctx):
    s = scene((65, 33, 17), 3)
    a = held(tdv, ctx, s, "model to camera", pose_direction=R.MODEL_TO_CAMERA)
    inv = dict(s, poses=np.linalg.inv(s["poses"].astype(np.float64)).astype(F))
    b = held(tdv, ctx, inv, "camera poses", pose_direction=R.SOURCE_ONTO_TARGET)
    assert abs(a["n"] - b["n"]) < 0.05 * a["n"] and np.abs(a["counts"] - b["counts"]).max() < 0.05 * a["counts"].min()      # the same fusion, other roundings


def test_partial_frustum_behind_and_zmax(tdv, ctx):
    s = scene((65, 33, 17), 3, f=700.0)                                            # 96 x 72 pixels at f = 700: 41 x 31 mm of the 65 x 33 mm volume
    ref = held(tdv, ctx, s, "partial frustum")
    seen = ref["volume"][..., 1] > 0
    assert seen[:, :, 32].any() and not seen[:, :, 0].any() and not seen[:, :, -1].any()
    behind = dict(s, poses=(s["poses"].astype(np.float64) @ Cs.synth.make_transform([1.0, 0.0, 0.0], 180.0, (0, 0, 0))).astype(F))
    assert held(tdv, ctx, behind, "from behind")["counts"].min() > 0
    s = scene((65, 33, 17), 3)
    cut = held(tdv, ctx, s, "zmax inside the scene", zmax=0.2995)
    full = restated(s)
    assert 0 < cut["counts"].sum() < full["counts"].sum()
    assert held(tdv, ctx, s, "zmax in front of everything", zmax=0.1)["counts"].sum() == 0


def test_max_weight_reached_and_min_weight(tdv, ctx):
    s = scene((65, 33, 17), 5)
    ref = held(tdv, ctx, s, "max_weight 2", max_weight=2.0)
    assert ref["volume"][..., 1].max() == 2 and restated(s)["volume"][..., 1].max() == 5
    held(tdv, ctx, s, "max_weight 2.5, trunc 2 mm", max_weight=2.5, trunc=0.002)
    a = held(tdv, ctx, s, "min_weight 3", min_weight=3.0)
    assert 0 < a["n"] < restated(s)["n"]
    held(tdv, ctx, s, "min_weight 0.5", min_weight=0.5, max_weight=1.0)


# ---------------------------------------------------------------- degenerate values
def test_seeded_volume_with_zeros_on_a_crossing(tdv, ctx):
    """A hand-made volume: tsdf from {-0.5, -0.0, 0.0, 0.25, 1.0, -1.0}, weights from {0, 1, 3}: crossings with f == 0 on one side (zero
    counts as non-negative, so (0, -0.5) brackets and (0, 0.25) does not), gradients with one and both neighbours replaced."""
    rng = np.random.default_rng(11)
    dims = (TX + 3, TY + 2, TZ + 1)
    s = dict(scene(dims, 0), vol=R.Volume((0.01, -0.02, 0.3), 0.0015, dims))
    start = np.stack([rng.choice(np.array([-0.5, -0.0, 0.0, 0.25, 1.0, -1.0], F), dims[::-1]), rng.choice(np.array([0, 1, 3], F), dims[::-1])], -1)
    ref = held(tdv, ctx, s, "seeded", start=start)
    f, w = start[..., 0].reshape(-1), start[..., 1].reshape(-1)
    key = R.extract(s["vol"], start)[2]
    a, b = key // 3, key // 3 + np.array([1, dims[0], dims[0] * dims[1]])[key % 3]
    assert ref["n"] > 500 and ((f[a] == 0) | (f[b] == 0)).sum() > 100 and (w[a] > 0).all() and (w[b] > 0).all()
    assert not np.isnan(ref["normals"]).any() and not np.isnan(ref["xyz"]).any()
    held(tdv, ctx, s, "seeded, min_weight 2", start=start, min_weight=2.0)


def test_nan_poses(tdv, ctx):
    s = scene((65, 33, 17), 5)
    poses = s["poses"].copy()
    poses[1] = np.nan; poses[3, 0, 1] = np.nan; poses[4, 2, 3] = np.inf
    for direction in (R.MODEL_TO_CAMERA, R.SOURCE_ONTO_TARGET):
        ref = held(tdv, ctx, dict(s, poses=poses), "NaN poses", pose_direction=direction)
        assert ref["counts"][0] > 0 and (ref["counts"][[1, 3, 4]] == 0).all()
        assert not np.isnan(ref["volume"]).any()


# ---------------------------------------------------------------- output forms, host form, arguments
def test_output_forms(tdv, ctx):
    s = scene((65, 33, 17), 2)
    ref = held(tdv, ctx, s, "no normals", normals=False)
    n = ref["n"]
    env = Env(ctx)
    cvol = tdv.tsdf_volume_struct(*s["vol"].args())
    env.up(ref["volume"])
    d_vol = env.keep[-1]
    for capacity in (n - 1, 0):
        ox, on = env.out(3 * n, F), env.out(3 * n, F)
        assert ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), ox.data_ptr(), on.data_ptr(), capacity) == (n, False)
        assert (env.get(ox, 3 * n, np.uint32) == 0xA5A5A5A5).all() and (env.get(on, 3 * n, np.uint32) == 0xA5A5A5A5).all()      # no row written
    ox, on = env.out(3 * (n + 2), F), env.out(3 * (n + 2), F)
    assert ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), ox.data_ptr(), on.data_ptr(), n + 2) == (n, True)
    x, nr = env.get(ox, 3 * (n + 2), F), env.get(on, 3 * (n + 2), F)
    assert x[:3 * n].tobytes() == ref["xyz"].tobytes() and nr[:3 * n].tobytes() == ref["normals"].tobytes()
    assert (x[3 * n:].view(np.uint32) == 0xA5A5A5A5).all() and (nr[3 * n:].view(np.uint32) == 0xA5A5A5A5).all()                # nothing beyond
    assert env.get(d_vol, s["vol"].voxels * 2, F).tobytes() == ref["volume"].tobytes()                                          # extraction reads only


def test_host_form_and_conveniences(tdv, ctx):
    s = scene((65, 33, 17), 3)
    ref = restated(s, max_weight=2.0)
    xyz, nrm = ctx.tsdf_fuse(s["frames"], s["poses"], s["intr"], s["vol"].args(), max_weight=2.0)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes()
    xyz, nrm = ctx.tsdf_fuse(s["frames"], s["poses"], s["intr"], s["vol"].args(), normals=False, max_weight=2.0)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm is None
    empty = ctx.tsdf_fuse(s["frames"][:0], s["poses"][:0], s["intr"], s["vol"].args())
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)
    volume = ctx.tsdf_volume(*s["vol"].args())
    assert volume[1].cpu().numpy().tobytes() == R.reset(s["vol"]).tobytes()
    counts = ctx.tsdf_integrate(volume, s["frames"], s["poses"], s["intr"], max_weight=2.0)
    xyz, nrm = ctx.tsdf_extract(volume)
    assert np.array_equal(counts, ref["counts"]) and volume[1].cpu().numpy().tobytes() == ref["volume"].tobytes()
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes()


def live_buffers(env):
    """Device buffers for tsdf_call on a live context, of the size GOOD's arguments need (the frames: of the largest n_frames tried), 0xA5
    throughout: env.keep[-4:] are the volume, the frames, the points and the normals."""
    d_vol, d_raw = env.out(4 * 3 * 2 * 2, F), env.out((R.MAX_FRAMES + 1) * 8 * 6, np.uint16)
    d_xyz, d_nrm = env.out(8 * 3, F), env.out(8 * 3, F)
    return dict(volume=d_vol.data_ptr(), frames=d_raw.data_ptr(), xyz=d_xyz.data_ptr(), normals=d_nrm.data_ptr())


def test_bad_arguments_on_a_live_context(tdv, ctx):
    """Every refusal of tests/test_tsdf_abi.py's table with a real ctx: TDV_ERR_BAD_ARG, the host outputs and the device buffers as they
    were.  The device buffers have the size GOOD's arguments need, with room for the frames of the largest n_frames tried."""
    env = Env(ctx)
    buffers = live_buffers(env)
    d_vol, d_raw, d_xyz, d_nrm = env.keep[-4:]
    o = Outputs()
    for what, kw, where in BAD[1:]:
        for which in where:
            assert tsdf_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == TDV_ERR_BAD_ARG, (what, which)
    for what, where in NULLS.items():
        for which in where:
            assert tsdf_call(tdv, which, ctx._h, o, null=(what,), buffers=buffers) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()
    for t, count, dtype in ((d_vol, 48, F), (d_raw, (R.MAX_FRAMES + 1) * 48, np.uint16), (d_xyz, 24, F), (d_nrm, 24, F)):
        assert (env.get(t, count, dtype).view(np.uint8) == 0xA5).all()
    # and the same calls with nothing wrong go through
    assert tsdf_call(tdv, "reset", ctx._h, o, buffers=buffers) == 0
    assert tsdf_call(tdv, "integrate", ctx._h, o, buffers=buffers) == 0 and (o.counts[:2] >= 0).all()
    assert tsdf_call(tdv, "extract", ctx._h, o, buffers=buffers, capacity=8) in (0, TDV_ERR_BAD_ARG) and o.n_out[0] >= 0
    assert tsdf_call(tdv, "fuse", ctx._h, o, buffers=buffers, capacity=0, null=("out_xyz",)) in (0, TDV_ERR_BAD_ARG) and o.n_out[0] >= 0
