"""Pose verification on the device (include/tdv_hip.h: tdv_verify_poses) against the restatement of tests/verify_restatement.py, byte
for byte: the result structs and the order from the host and the device entry points, the depth image from tdv_render_depth and
tdv_render_depth_dev, each test on a Context of its own.  The shapes are the smallest at which each mechanism can go wrong: the wave (63,
64, 65) and the workgroup (L - 1, L, L + 1 with L = TDV_VERIFY_LANES: where a lane takes its second point) in the model size; frames of one
tile less, exactly and one more than a tile in each direction, covered entirely, so that a pose's box spans 1, 2 and 4 tiles and cover squares
straddle the tile edges; pose counts 0, 1, 2, 257 and 1,025 (the tile scan carries over blocks of 1,024 poses)."""
import numpy as np
import pytest
import torch

import verify_restatement as R
from test_verify_abi import BAD, Outputs, exact_pose, null_refusals, refusals, small_frame

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
L = R.LANES
M2C = dict(pose_direction=R.MODEL_TO_CAMERA)
EYE = np.eye(4, dtype=F)
PAD = 5                                                      # floats past the depth image of a device render: never written


@pytest.fixture
def vctx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def cam_of(w, h, f=None):
    f = float(f or max(w, h))
    return dict(fx=f, fy=f * 0.96875, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0)


def _up(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(16, np.uint8)).to(DEV)
    return t


def dev_verify(ctx, model, poses, raw, scale, cam, **prm):
    model = np.ascontiguousarray(model, F).reshape(-1, 3)
    mt, rt = _up(model), _up(np.ascontiguousarray(raw, np.uint16))
    torch.cuda.synchronize()                                 # the uploads are torch's; the ctx runs on a stream of its own
    h, w = raw.shape
    return ctx.verify_poses_dev(mt.data_ptr(), len(model), poses, rt.data_ptr(), w, h, scale, cam["fx"], cam["fy"], cam["cx"], cam["cy"], **prm)


def dev_render(ctx, model, pose, w, h, cam, **prm):
    model = np.ascontiguousarray(model, F).reshape(-1, 3)
    mt = _up(model)
    out = torch.full((w * h + PAD,), -9.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    n = ctx.render_depth_dev(mt.data_ptr(), len(model), pose, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"], out.data_ptr(), **prm)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[w * h:] == -9).all(), "written beyond the image"
    return got[:w * h].reshape(h, w), n


def check(ctx, model, poses, raw, scale, cam, what, render=(0,), **prm):
    """Host and device entry points against the restatement: results, order, and the depth image of the poses listed in `render`."""
    raw = np.ascontiguousarray(raw, np.uint16)
    h, w = raw.shape
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    ref, order, depths = R.verify(model, poses, raw, scale, **cam, **dict(R.DEFAULTS, **prm))
    for r in ref:
        assert r["n_rendered"] == r["n_consistent"] + r["n_occluded"] + r["n_violating"] + r["n_unknown"]
    for name, (got, got_order) in (("host", ctx.verify_poses(model, poses, raw, scale, **cam, **prm)),
                                   ("dev", dev_verify(ctx, model, poses, raw, scale, cam, **prm))):
        assert got == ref, (what, name, [(i, g, r) for i, (g, r) in enumerate(zip(got, ref)) if g != r][:3])
        assert got_order.dtype == np.int32 and np.array_equal(got_order, order), (what, name, got_order, order)
    rprm = {k: v for k, v in prm.items() if k != "tau"}
    for i in render:
        if 0 <= i < len(poses):
            n_rendered = int((depths[i] != 0).sum())
            assert n_rendered == ref[i]["n_rendered"]
            img = ctx.render_depth(model, poses[i], w, h, **cam, **rprm)
            assert img.dtype == F and img.shape == (h, w) and img.tobytes() == depths[i].tobytes(), (what, "render_depth", i)
            img, n = dev_render(ctx, model, poses[i], w, h, cam, **rprm)
            assert img.tobytes() == depths[i].tobytes() and n == n_rendered, (what, "render_depth_dev", i, n, n_rendered)
    return ref, order, depths


def slab(n, seed, w=37, h=29, cam=None, z=(0.7, 1.3), spill=1.15):
    """n points in camera coordinates whose images spread over the frame and a little beyond it."""
    cam = cam or cam_of(w, h)
    rng = np.random.default_rng(seed)
    zc = rng.uniform(*z, n)
    u, v = rng.uniform(-0.5, w - 0.5, n), rng.uniform(-0.5, h - 0.5, n)
    u, v = (u - cam["cx"]) * spill + cam["cx"], (v - cam["cy"]) * spill + cam["cy"]
    return np.c_[(u - cam["cx"]) * zc / cam["fx"], (v - cam["cy"]) * zc / cam["fy"], zc].astype(F)


def cover(w, h, cam, seed):
    """One point per pixel, inside it: a model that covers the whole frame at every splat."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    zc = rng.uniform(0.8, 1.2, (h, w))
    uu, vv = u + rng.uniform(-0.3, 0.3, (h, w)), v + rng.uniform(-0.3, 0.3, (h, w))
    pts = np.stack([(uu - cam["cx"]) * zc / cam["fx"], (vv - cam["cy"]) * zc / cam["fy"], zc], -1).reshape(-1, 3).astype(F)
    return pts[rng.permutation(len(pts))]


def frame_for(model, pose, w, h, cam, scale, seed, **prm):
    """An observed frame around the model's own rendered depth (test_verify_abi.small_frame): every class occurs."""
    prm = {k: v for k, v in dict(R.DEFAULTS, **prm).items() if k != "tau"}
    return small_frame(R.depth_of(R.render_keys(model, pose, w, h, **cam, **prm)[0]), scale, seed)


def nudged(T, seed, trans=0.01):
    rng = np.random.default_rng(seed)
    T = np.array(T, F)
    T[:3, 3] += rng.uniform(-trans, trans, 3).astype(F)
    return T


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, L - 1, L, L + 1, 5000])
def test_model_sizes(vctx, n):
    w, h = 37, 29
    cam = cam_of(w, h)
    model = slab(n, 300 + n, w, h)
    full = slab(400, 1, w, h)
    raw = frame_for(full, EYE, w, h, cam, 1000.0, n, **M2C)
    for splat in (0, 1):
        ref, _, _ = check(vctx, model, [EYE, nudged(EYE, n)], raw, 1000.0, cam, ("model size", n, splat), render=(0, 1), splat=splat, **M2C)
        assert ref[0]["n_projected"] == n and (n == 0 or ref[0]["n_rendered"] > 0)


FRAMES = [(1, 1), (37, 29)] + [(w, h) for w in (R.TILE_W - 1, R.TILE_W, R.TILE_W + 1) for h in (R.TILE_H - 1, R.TILE_H, R.TILE_H + 1)]


@pytest.mark.parametrize("w, h", FRAMES)
def test_frame_sizes_around_the_tile(vctx, w, h):
    cam = cam_of(w, h)
    model = cover(w, h, cam, w * 1000 + h)
    for splat in (0, 1, 3):
        raw = frame_for(model, EYE, w, h, cam, 1000.0, splat, splat=splat, **M2C)
        ref, _, depths = check(vctx, model, [EYE, nudged(EYE, w + h, 0.004)], raw, 1000.0, cam, ("frame", w, h, splat), render=(0, 1), splat=splat,
                               **M2C)
        assert ref[0]["n_rendered"] == w * h and (depths[0] != 0).all()            # the box is the frame: 1, 2 or 4 tiles
        assert ref[0]["n_projected"] == w * h


def test_a_box_that_starts_past_the_first_tile(vctx):
    """A small model in the far corner of a 300 x 260 frame: its box begins in tile (1, 1) and ends in the frame's last, partial tiles."""
    w, h = 300, 260
    cam = cam_of(w, h)
    rng = np.random.default_rng(5)
    n = 600
    zc = rng.uniform(0.8, 1.2, n)
    u, v = rng.uniform(250, 299.4, n), rng.uniform(251, 259.4, n)
    model = np.c_[(u - cam["cx"]) * zc / cam["fx"], (v - cam["cy"]) * zc / cam["fy"], zc].astype(F)
    raw = frame_for(model, EYE, w, h, cam, 1000.0, 3, **M2C)
    ref, _, depths = check(vctx, model, [EYE], raw, 1000.0, cam, "corner", **M2C)
    ys, xs = np.nonzero(depths[0])
    assert xs.min() >= 2 * R.TILE_W - 7 and ys.min() >= 250 and xs.max() == w - 1 and ys.max() == h - 1
    mid = np.c_[(rng.uniform(100, 160, n) - cam["cx"]) * zc / cam["fx"], (rng.uniform(120, 135, n) - cam["cy"]) * zc / cam["fy"], zc].astype(F)
    both = np.r_[model, mid]                                                       # ... and a box of 3 x 2 tiles that starts inside tile (0, 0)
    check(vctx, both, [EYE, nudged(EYE, 9)], frame_for(both, EYE, w, h, cam, 1000.0, 4, **M2C), 1000.0, cam, "two by two", render=(0, 1), **M2C)


# ---------------------------------------------------------------- pose counts
@pytest.mark.parametrize("n_poses", [0, 1, 2, 257, 1025])
def test_pose_counts(vctx, n_poses):
    w, h = 37, 29
    cam = cam_of(w, h)
    model = slab(300, 8, w, h)
    raw = frame_for(model, EYE, w, h, cam, 1000.0, 2, **M2C)
    poses = np.stack([nudged(EYE, 50 + i, 0.02) for i in range(n_poses)]) if n_poses else np.zeros((0, 4, 4), F)
    if n_poses >= 2:
        poses[-1] = poses[0]                                                       # the same pose twice
    if n_poses > 2:
        poses[100] = np.nan; poses[200][:3, 3] = (9, 9, 1)                         # poses without a tile inside the list
    ref, order, _ = check(vctx, model, poses, raw, 1000.0, cam, ("poses", n_poses), render=(0, n_poses - 1), **M2C)
    assert len(ref) == n_poses == len(order)
    if n_poses >= 2:
        assert ref[0] == ref[-1] and list(order).index(0) < list(order).index(n_poses - 1)
    if n_poses >= 257:
        assert len({r["n_consistent"] - r["n_violating"] for r in ref}) > 20


def test_both_directions(vctx):
    """A general pose under source_onto_target (the default, what every registration here returns) and under model_to_camera."""
    w, h = 64, 48
    cam = cam_of(w, h)
    pts = slab(2000, 4, w, h)
    c, s = np.cos(0.3), np.sin(0.3)
    T = np.array([[c, -s, 0, 0.02], [s, c, 0, -0.01], [0, 0, 1, 0.05], [0, 0, 0, 1]], F)    # model -> camera
    model = ((pts.astype(np.float64) - T[:3, 3]) @ T[:3, :3].astype(np.float64)).astype(F)
    raw = frame_for(model, T, w, h, cam, 1000.0, 1, **M2C)
    a, _, _ = check(vctx, model, [T, nudged(T, 1)], raw, 1000.0, cam, "model_to_camera", render=(0, 1), **M2C)
    Ti = np.linalg.inv(T.astype(np.float64)).astype(F)
    b, _, _ = check(vctx, model, [Ti, nudged(Ti, 2)], raw, 1000.0, cam, "source_onto_target", render=(0, 1))
    assert a[0]["n_consistent"] > 100 and b[0]["n_consistent"] > 100
    E = exact_pose((1, 0, 2), (1, -1, 1), (0.25, -0.125, 0.0625))
    check(vctx, model, [E], raw, 1000.0, cam, "exact", pose_direction=R.SOURCE_ONTO_TARGET)


# ---------------------------------------------------------------- the usable test
def test_usable(vctx):
    w, h, splat = 37, 29, 2
    cam = cam_of(w, h)
    inside = slab(200, 2, w, h, spill=0.9)
    raw = frame_for(inside, EYE, w, h, cam, 1000.0, 6, splat=splat, **M2C)
    zeros = dict.fromkeys(R.RESULT, 0)

    def run(model, poses, what, **prm):
        return check(vctx, model, poses, raw, 1000.0, cam, what, render=(0,), **dict(dict(splat=splat, **M2C), **prm))[0]

    behind = inside * F([1, 1, -1])
    assert run(behind, [EYE], "behind the camera") == [zeros]
    off = inside + F([5.0, 0, 0])                                                  # images far to the right of the frame
    r = run(off, [EYE], "off the frame")[0]
    assert r["n_projected"] == len(off) and r["n_rendered"] == 0
    # centres outside the frame by at most splat pixels, all around it: only clipped covers land
    rng = np.random.default_rng(3)
    n = 120
    zc = rng.uniform(0.8, 1.2, n)
    side = np.arange(n) % 4                                                        # left, right, above, below; the corners included
    out = rng.integers(1, splat + 1, n) + rng.uniform(-0.3, 0.3, n)
    along_u, along_v = rng.uniform(-splat - 0.3, w - 0.7 + splat, n), rng.uniform(-splat - 0.3, h - 0.7 + splat, n)
    u = np.where(side == 0, -out, np.where(side == 1, w - 1 + out, along_u))
    v = np.where(side == 2, -out, np.where(side == 3, h - 1 + out, along_v))
    rim = np.c_[(u - cam["cx"]) * zc / cam["fx"], (v - cam["cy"]) * zc / cam["fy"], zc].astype(F)
    ok, pu, pv, _ = R.project(rim, EYE, **cam, pose_direction=R.MODEL_TO_CAMERA, zmax=10.0)
    assert ok.all() and (((pu < 0) | (pu >= w)) | ((pv < 0) | (pv >= h))).all()     # no centre inside
    r = run(rim, [EYE], "clipped covers only")[0]
    assert 0 < r["n_rendered"] < 2 * splat * (w + h + 2 * splat)
    bad = inside.copy()
    bad[::3] = np.nan; bad[1::7, 2] = np.inf; bad[2::11, 0] = -np.inf
    r = run(bad, [EYE], "NaN and infinite rows")[0]
    assert 0 < r["n_projected"] == int(np.isfinite(bad).all(1).sum())
    nan_pose, inf_pose, one_nan = np.full((4, 4), np.nan, F), np.full((4, 4), np.inf, F), EYE.copy()
    one_nan[0, 3] = np.nan
    for direction in (R.MODEL_TO_CAMERA, R.SOURCE_ONTO_TARGET):
        res = run(inside, [nan_pose, EYE, inf_pose, one_nan], "non-finite poses", pose_direction=direction)
        assert res[0] == zeros and res[2] == zeros and res[3] == zeros and res[1]["n_rendered"] > 0
    zmax = F(1.0)
    edge = np.array([[0, 0, zmax], [0.05, 0, np.nextafter(zmax, F(2))], [-0.05, 0, np.nextafter(zmax, F(0))]], F)
    r = run(edge, [EYE], "zc at zmax", zmax=float(zmax), splat=0)[0]
    assert r["n_projected"] == 2 and r["n_rendered"] == 2
    huge = np.array([[1e30, 0, 1e-3], [0, 3e4, 1.0], [0, 0, 1.0]], F)               # |uf| and |vf| at or above 2^20
    assert run(huge, [EYE], "pixel magnitude")[0]["n_projected"] == 1


# ---------------------------------------------------------------- the z-buffer
def test_z_buffer(vctx):
    w, h = 37, 29
    cam = cam_of(w, h)

    def at(u, v, z):
        return [(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z]

    raw = np.full((h, w), 1000, np.uint16)
    two = np.array([at(10, 12, 1.25), at(10, 12, 0.75), at(20, 5, 0.5), at(20, 5, 0.5)], F)     # different depths; equal depths
    _, _, depths = check(vctx, two, [EYE], raw, 1000.0, cam, "two on a pixel", splat=0, **M2C)
    assert depths[0][12, 10] == F(0.75) and depths[0][5, 20] == F(0.5) and (depths[0] != 0).sum() == 2
    rng = np.random.default_rng(1)
    z = rng.uniform(0.6, 1.4, 20000)
    many = np.array([at(18 + rng.uniform(-0.2, 0.2), 14 + rng.uniform(-0.2, 0.2), zz) for zz in z], F)   # one LDS word, 20,000 contenders
    for splat in (0, 2):
        ref, _, depths = check(vctx, many, [EYE], raw, 1000.0, cam, "many on a pixel", splat=splat, **M2C)
        assert ref[0]["n_rendered"] == (2 * splat + 1) ** 2 and depths[0][14, 18] == many[:, 2].min()


# ---------------------------------------------------------------- classification edges
def test_classification_edges(vctx):
    """The observed frame is the rendered depth itself (scale and tau powers of two: zo == zr is reachable), then single pixels are moved
    onto and just past each boundary."""
    w, h, scale, tau, zmax, steps = 40, 30, 1024.0, 2.0 ** -8, 1.5, 4            # tau = 4 raw steps
    cam = cam_of(w, h)
    rng = np.random.default_rng(2)
    v, u = np.mgrid[0:h, 0:w]
    zc = rng.integers(820, 1230, (h, w)) / 1024.0                                 # exact raw values
    model = np.stack([(u - cam["cx"]) * zc / cam["fx"], (v - cam["cy"]) * zc / cam["fy"], zc], -1).reshape(-1, 3).astype(F)
    prm = dict(splat=0, tau=tau, zmax=zmax, **M2C)
    keys = R.render_keys(model, EYE, w, h, **cam, pose_direction=R.MODEL_TO_CAMERA, splat=0, zmax=zmax)[0]
    zr = R.depth_of(keys)
    assert (zr != 0).all() and (zr * F(scale) == np.rint(zr * F(scale))).all()
    raw = (zr * F(scale)).astype(np.uint16)
    exact = R.verify(model, [EYE], raw, scale, **cam, **dict(R.DEFAULTS, **prm))[0][0]
    assert exact["n_consistent"] == w * h and exact["err_q20"] == 0                # zo == zr everywhere
    moved = raw.copy().reshape(-1)
    plan = [(+steps, "n_consistent"), (-steps, "n_consistent"), (+steps + 1, "n_violating"), (-steps - 1, "n_occluded"), (None, "n_unknown"),
            ("over", "n_unknown"), ("at", "n_violating")]
    want = dict(n_consistent=w * h, n_violating=0, n_occluded=0, n_unknown=0)
    err = 0
    for k, (move, cls) in enumerate(plan):
        for px in range(40 * k, 40 * k + 25):                                      # 25 pixels per move
            moved[px] = 0 if move is None else int(zmax * scale) + 1 if move == "over" else int(zmax * scale) if move == "at" else int(moved[px]) + move
            want["n_consistent"] -= 1
            want[cls] += 1
            err += steps * (1 << 20) // 1024 if cls == "n_consistent" else 0
    moved = moved.reshape(h, w)
    ref = R.verify(model, [EYE], moved, scale, **cam, **dict(R.DEFAULTS, **prm))[0][0]
    assert {k: ref[k] for k in want} == want and ref["err_q20"] == err and min(want.values()) >= 25       # every class, both sides of each edge
    check(vctx, model, [EYE], moved, scale, cam, "classification edges", **prm)
    check(vctx, model, [EYE], raw, scale, cam, "zo == zr", **prm)


# ---------------------------------------------------------------- arguments on a real context
def test_bad_arguments_on_a_context(vctx, tdv):
    o = Outputs(tdv)
    for case in range(len(BAD)):
        for status in refusals(tdv, vctx._h, o, case):
            assert status == TDV_ERR_BAD_ARG, BAD[case][0]
    for what, status in null_refusals(tdv, vctx._h, o):
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()
    w, h = 37, 29
    cam = cam_of(w, h)
    model = slab(100, 1, w, h)
    check(vctx, model, [EYE], frame_for(model, EYE, w, h, cam, 1000.0, 1, **M2C), 1000.0, cam, "after the refusals", **M2C)
    empty = np.zeros((0, w), np.uint16)                                            # an empty frame is valid: the points still project
    res, order = vctx.verify_poses(model, [EYE], empty, 1000.0, **cam, **M2C)
    assert res == [dict(dict.fromkeys(R.RESULT, 0), n_projected=100)] and order.tolist() == [0]


# ---------------------------------------------------------------- behaviour
def test_true_pose_against_a_pose_in_free_space(vctx, synth):
    """A relief part over a fronto-parallel background, the frame rendered by the restatement at the true pose and rounded to u16: the
    true pose is consistent everywhere (the only error is the quantisation, at most 0.5 mm plus rounding, inside tau); the same pose moved
    towards the camera by more than the part's depth extent plus tau is seen through everywhere."""
    w, h, scale, tau, f = 160, 120, 1000.0, 0.002, 150.0
    cam = dict(fx=f, fy=f, cx=80.0, cy=60.0)
    part = synth.ReliefPart(seed=3).surface_points(0.001).astype(F)
    true = synth.scan_pose(0.5).astype(F)                                          # model -> camera
    prm = dict(splat=1, tau=tau, **M2C)
    depth = R.depth_of(R.render_keys(part, true, w, h, **cam, pose_direction=R.MODEL_TO_CAMERA, splat=1)[0])
    on_part = depth != 0
    extent = float(depth[on_part].max() - depth[on_part].min())
    assert on_part.sum() > 800 and extent < 0.03
    raw = np.rint(np.where(on_part, depth, F(0.6)).astype(np.float64) * scale).astype(np.uint16)
    free = true.copy()
    free[2, 3] -= 0.05                                                             # > extent + tau
    assert 0.05 > extent + tau
    ref, order, _ = check(vctx, part, [free, true], raw, scale, cam, "behaviour", render=(0, 1), **prm)
    assert ref[1]["n_violating"] == 0 and ref[1]["n_occluded"] == 0 and ref[1]["n_consistent"] == ref[1]["n_rendered"] == int(on_part.sum())
    assert ref[0]["n_violating"] == ref[0]["n_rendered"] > 800
    assert order.tolist() == [1, 0]
