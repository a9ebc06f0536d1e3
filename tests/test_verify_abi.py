"""CPU suite: pose verification (include/tdv_hip.h: tdv_verify_poses).  The ABI exports the entry points, lists them in ABI_SYMBOLS, has
the documented struct layouts, constants and defaults, and refuses every bad argument before it writes anything; the restatement
(tests/verify_restatement.py) is held to an independent definition (a per-pixel loop that takes the minimum over the explicit list of the
points covering the pixel, the projection in scalar f32), to n_rendered == the sum of the four classes, and to the equivalence of the two
pose directions on exactly invertible poses.  No compute entry point of the library runs here; tests/test_gpu_verify.py holds the device to
this restatement byte for byte."""
import ctypes as C

import numpy as np
import pytest

import verify_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_verify_default_params", "tdv_verify_poses", "tdv_verify_poses_dev", "tdv_render_depth", "tdv_render_depth_dev")
NAN, INF = float("nan"), float("inf")


def test_symbols_constants_structs_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.VerifyParamsC) == 16
    assert [(k, getattr(tdv.VerifyParamsC, k).offset) for k, _ in tdv.VerifyParamsC._fields_] == [("pose_direction", 0), ("splat", 4), ("tau", 8),
                                                                                                 ("zmax", 12)]
    assert C.sizeof(tdv.VerifyResultC) == 32
    assert tuple(k for k, _ in tdv.VerifyResultC._fields_) == R.RESULT
    assert [getattr(tdv.VerifyResultC, k).offset for k in R.RESULT] == [0, 4, 8, 12, 16, 20, 24]
    assert (tdv.TDV_POSE_SOURCE_ONTO_TARGET, tdv.TDV_POSE_MODEL_TO_CAMERA) == (0, 1) == (R.SOURCE_ONTO_TARGET, R.MODEL_TO_CAMERA)
    assert tdv.TDV_VERIFY_MAX_SPLAT == R.MAX_SPLAT == 3 and tdv.TDV_VERIFY_MAX_MODEL == R.MAX_MODEL == 1 << 22
    assert tdv.TDV_VERIFY_MAX_POSES == R.MAX_POSES == 65536 and tdv.TDV_VERIFY_MAX_SIDE == R.MAX_SIDE == 8192
    assert (tdv.TDV_VERIFY_TILE_W, tdv.TDV_VERIFY_TILE_H, tdv.TDV_VERIFY_LANES) == (R.TILE_W, R.TILE_H, R.LANES)
    assert 2 * R.TILE_W * R.TILE_H * 4 <= 160 * 1024                              # two workgroups' tiles in a CU's LDS
    p = tdv.verify_params()
    assert (p.pose_direction, p.splat) == (R.DEFAULTS["pose_direction"], R.DEFAULTS["splat"])
    assert F(p.tau).tobytes() == F(R.DEFAULTS["tau"]).tobytes() and F(p.zmax).tobytes() == F(R.DEFAULTS["zmax"]).tobytes()
    lib.tdv_verify_default_params(None)                                            # a NULL is ignored
    assert tdv.verify_params(pose_direction="model_to_camera", splat=3).pose_direction == 1
    with pytest.raises(TypeError):
        tdv.verify_params(nope=1)


# ---------------------------------------------------------------- arguments
GOOD = dict(n_model=4, n_poses=2, width=4, height=3, scale=1000.0, fx=50.0, fy=50.0, cx=2.0, cy=1.5, pose_direction=0, splat=1, tau=0.002,
            zmax=10.0)
# (what, the arguments replaced, whether the render entry points take the argument too)
BAD = [("n_model < 0", dict(n_model=-1), True), ("n_model > 2^22", dict(n_model=R.MAX_MODEL + 1), True),
       ("n_poses < 0", dict(n_poses=-1), False), ("n_poses > 65536", dict(n_poses=R.MAX_POSES + 1), False),
       ("width < 0", dict(width=-1), True), ("height < 0", dict(height=-1), True),
       ("width > 8192", dict(width=R.MAX_SIDE + 1), True), ("height > 8192", dict(height=R.MAX_SIDE + 1), True),
       ("splat < 0", dict(splat=-1), True), ("splat > 3", dict(splat=R.MAX_SPLAT + 1), True),
       ("tau == 0", dict(tau=0.0), True), ("tau < 0", dict(tau=-0.002), True), ("tau NaN", dict(tau=NAN), True), ("tau inf", dict(tau=INF), True),
       ("scale == 0", dict(scale=0.0), False), ("scale < 0", dict(scale=-1000.0), False), ("scale NaN", dict(scale=NAN), False),
       ("scale inf", dict(scale=INF), False),
       ("fx == 0", dict(fx=0.0), True), ("fx < 0", dict(fx=-50.0), True), ("fx NaN", dict(fx=NAN), True), ("fx inf", dict(fx=INF), True),
       ("fy == 0", dict(fy=0.0), True), ("fy < 0", dict(fy=-50.0), True), ("fy NaN", dict(fy=NAN), True), ("fy inf", dict(fy=INF), True),
       ("pose_direction 2", dict(pose_direction=2), True), ("pose_direction -1", dict(pose_direction=-1), True)]
NULLS = ("model", "poses", "frame", "params", "results")


class Outputs:
    """Every output of a call, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n_poses=2, pixels=12, fill=0x5A):
        self.res = (tdv.VerifyResultC * n_poses)(); C.memset(C.byref(self.res), fill, C.sizeof(self.res))
        self.order = np.full(n_poses, -7, np.int32); self.depth = np.full(pixels, -7, F); self.n_rendered = C.c_int(-7)
        self.before = self.snapshot()

    def snapshot(self):
        return bytes(self.res), self.order.tobytes(), self.depth.tobytes(), self.n_rendered.value

    def untouched(self):
        return self.snapshot() == self.before


def P(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def inputs():
    return np.ones((4, 3), F), np.tile(np.eye(4, dtype=F).reshape(-1), 2), np.full((3, 4), 1000, np.uint16)


def _params(tdv, g, null):
    p = tdv.VerifyParamsC(g["pose_direction"], g["splat"], g["tau"], g["zmax"])
    return None if "params" in null else C.byref(p)


def verify_call(tdv, dev, ctx, o, null=(), **kw):
    """Host arrays in every slot: a refused call must not look at them (the device entry point included)."""
    g = dict(GOOD, **kw)
    model, poses, raw = inputs()
    fn = tdv.lib().tdv_verify_poses_dev if dev else tdv.lib().tdv_verify_poses
    return fn(ctx, None if "model" in null else P(model), g["n_model"], None if "poses" in null else P(poses), g["n_poses"],
              None if "frame" in null else P(raw), g["width"], g["height"], C.c_float(g["scale"]), C.c_float(g["fx"]), C.c_float(g["fy"]),
              C.c_float(g["cx"]), C.c_float(g["cy"]), _params(tdv, g, null), None if "results" in null else C.byref(o.res), P(o.order))


def render_call(tdv, dev, ctx, o, null=(), **kw):
    g = dict(GOOD, **kw)
    model, poses, _ = inputs()
    fn = tdv.lib().tdv_render_depth_dev if dev else tdv.lib().tdv_render_depth
    return fn(ctx, None if "model" in null else P(model), g["n_model"], None if "poses" in null else P(poses), g["width"], g["height"],
              C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(g["cx"]), C.c_float(g["cy"]), _params(tdv, g, null),
              None if "frame" in null else P(o.depth), C.byref(o.n_rendered))


def refusals(tdv, ctx, o, case):
    """The statuses of the entry points that take BAD[case]'s argument, host and device form."""
    _, kw, render = BAD[case]
    for dev in (False, True):
        yield verify_call(tdv, dev, ctx, o, **kw)
        if render:
            yield render_call(tdv, dev, ctx, o, **kw)


def null_refusals(tdv, ctx, o):
    for dev in (False, True):
        for what in NULLS:
            yield what, verify_call(tdv, dev, ctx, o, null=(what,))
            if what != "results":
                yield what, render_call(tdv, dev, ctx, o, null=(what,))


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_verify.py refuses each bad argument on one."""
    o = Outputs(tdv)
    for dev in (False, True):
        assert verify_call(tdv, dev, None, o) == TDV_ERR_BAD_ARG and render_call(tdv, dev, None, o) == TDV_ERR_BAD_ARG
    for status in refusals(tdv, None, o, case):
        assert status == TDV_ERR_BAD_ARG, BAD[case][0]
    assert o.untouched()


def test_null_pointers(tdv):
    o = Outputs(tdv, fill=0x33)
    for what, status in null_refusals(tdv, None, o):
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against an independent definition
CAM = dict(fx=14.0, fy=13.0, cx=7.5, cy=5.5)


def exact_pose(perm, signs, t):
    """A rotation that is an axis permutation with signs and a translation: exact in f32, and so is its inverse."""
    T = np.eye(4, dtype=F)
    T[:3, :3] = 0
    for r, (c, s) in enumerate(zip(perm, signs)):
        T[r, c] = s
    T[:3, 3] = t
    return T


def inverse_exact(T):
    Ti = np.eye(4, dtype=F)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def small_model(seed, n=70):
    """Points of a slab in front of a camera at the origin looking down +z (model_to_camera with the identity), some off the frame, some
    behind the camera, one NaN and one infinite row."""
    rng = np.random.default_rng(seed)
    m = np.c_[rng.uniform(-0.6, 0.6, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.7, 1.3, n)].astype(F)
    m[3, 2] = -0.5; m[11] = np.nan; m[19, 0] = np.inf; m[23, 2] = 0.0
    return m


def small_frame(depth, scale, seed):
    """An observed frame around a rendered depth: exact, a few raw steps off either way, holes and far readings."""
    rng = np.random.default_rng(seed)
    raw = np.rint(depth.astype(np.float64) * scale) + rng.integers(-4, 5, depth.shape)
    raw[depth == 0] = rng.integers(0, 3000, int((depth == 0).sum()))
    raw[rng.random(depth.shape) < 0.15] = 0
    raw[rng.random(depth.shape) < 0.1] = 60000
    return np.clip(raw, 0, 65535).astype(np.uint16)


def scalar_project(m, t, cam, direction, zmax):
    """Rules 1 to 3 for one point, every operation a scalar f32: (u, v, zc) or None."""
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        if direction == R.SOURCE_ONTO_TARGET:
            d = [F(m[k] - t[12 + k]) for k in range(3)]
            c = [F(F(F(t[4 * r] * d[0]) + F(t[4 * r + 1] * d[1])) + F(t[4 * r + 2] * d[2])) for r in range(3)]
        else:
            c = [F(F(F(F(t[r] * m[0]) + F(t[4 + r] * m[1])) + F(t[8 + r] * m[2])) + t[12 + r]) for r in range(3)]
        if not (all(np.isfinite(x) for x in c) and c[2] > 0 and c[2] <= F(zmax)):
            return None
        uf, vf = F(F(F(c[0] * fx) / c[2]) + cx), F(F(F(c[1] * fy) / c[2]) + cy)
        if not (np.isfinite(uf) and np.isfinite(vf) and abs(uf) < 2 ** 20 and abs(vf) < 2 ** 20):
            return None
        return int(np.floor(F(uf + F(0.5)))), int(np.floor(F(vf + F(0.5)))), c[2]


def per_pixel(model, T, raw, scale, cam, direction, splat, tau, zmax):
    """The definition, pixel by pixel: the covering points listed, their minimum, the class."""
    t = [F(x) for x in np.asarray(T, F).T.reshape(16)]
    pts = [p for p in (scalar_project([F(x) for x in m], t, cam, direction, zmax) for m in model) if p is not None]
    h, w = raw.shape
    inv = F(1.0 / float(F(scale)))
    out = dict(n_projected=len(pts), n_rendered=0, n_consistent=0, n_occluded=0, n_violating=0, n_unknown=0, err_q20=0)
    depth = np.zeros((h, w), F)
    for y in range(h):
        for x in range(w):
            cover = [zc for (u, v, zc) in pts if abs(u - x) <= splat and abs(v - y) <= splat]
            if not cover:
                continue
            zr = min(cover)
            depth[y, x] = zr
            out["n_rendered"] += 1
            zo = F(F(raw[y, x]) * inv)
            if raw[y, x] == 0 or not zo <= F(zmax):
                out["n_unknown"] += 1
                continue
            diff = F(zo - zr)
            if abs(diff) <= F(tau):
                out["n_consistent"] += 1
                out["err_q20"] += int(F(abs(diff) * F(1048576.0)))
            elif diff < -F(tau):
                out["n_occluded"] += 1
            else:
                assert diff > F(tau)
                out["n_violating"] += 1
    return out, depth


@pytest.mark.parametrize("direction", [R.SOURCE_ONTO_TARGET, R.MODEL_TO_CAMERA])
@pytest.mark.parametrize("splat", [0, 1, 2, 3])
def test_against_the_per_pixel_definition(direction, splat):
    w, h, scale, tau, zmax = 16, 12, 1000.0, 0.002, 1.25
    model = small_model(splat)
    cam_pose = np.eye(4, dtype=F)                                                  # the slab is already in front of the camera
    tilt = exact_pose((1, 0, 2), (-1, 1, 1), (0.125, -0.0625, 0.03125))
    poses = np.stack([cam_pose, tilt, np.full((4, 4), np.nan, F)])
    first = R.render_keys(model, poses[0], w, h, **CAM, pose_direction=direction, splat=splat, zmax=zmax)[0]
    raw = small_frame(R.depth_of(first), scale, 7 + splat)
    res, order, depths = R.verify(model, poses, raw, scale, **CAM, pose_direction=direction, splat=splat, tau=tau, zmax=zmax)
    seen = set()
    for T, r, d in zip(poses, res, depths):
        ref, ref_depth = per_pixel(model, T, raw, scale, CAM, direction, splat, tau, zmax)
        assert r == ref, (direction, splat, r, ref)
        assert d.tobytes() == ref_depth.tobytes()
        assert r["n_rendered"] == r["n_consistent"] + r["n_occluded"] + r["n_violating"] + r["n_unknown"]
        seen |= {k for k in R.RESULT if r[k] > 0}
    assert seen == set(R.RESULT), seen                                             # every class occurred
    assert res[2] == dict.fromkeys(R.RESULT, 0) and 0 < res[0]["n_projected"] < len(model) - 4       # zmax cuts the slab
    score = [r["n_consistent"] - r["n_violating"] for r in res]
    assert order.tolist() == sorted(range(3), key=lambda i: (-score[i], i))


def test_order_ties_go_to_the_lower_index():
    res = [dict(n_consistent=c, n_violating=v) for c, v in ((5, 1), (9, 0), (4, 0), (9, 0), (0, 7))]
    assert R.order_of(res).tolist() == [1, 3, 0, 2, 4]


@pytest.mark.parametrize("perm, signs", [((0, 1, 2), (1, 1, 1)), ((1, 0, 2), (1, -1, 1)), ((2, 0, 1), (-1, 1, -1)), ((0, 2, 1), (-1, -1, -1))])
def test_both_directions_agree_on_exactly_invertible_poses(perm, signs):
    """T under one direction and its exact inverse under the other: the same bytes."""
    w, h, scale = 16, 12, 1024.0
    rng = np.random.default_rng(20 + sum(perm) + 3 * sum(signs))
    cam = small_model(5, 90)                                                       # the points in camera coordinates
    for t in ((0.25, -0.5, 0.125), (-1.0, 0.0, 2.0 ** -6)):
        T = exact_pose(perm, signs, t)                                             # model -> camera
        Ti = inverse_exact(T)
        assert (inverse_exact(Ti) == T).all() and np.isin(np.abs(T[:3, :3]), (0, 1)).all()
        with np.errstate(invalid="ignore"):
            model = ((cam.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)    # R^T (p - t): the model whose image is `cam`, rounded
        model[11] = np.nan; model[19] = (np.inf, 0, 1)
        raw = small_frame(R.depth_of(R.render_keys(model, T, w, h, **CAM, pose_direction=R.MODEL_TO_CAMERA)[0]), scale, int(rng.integers(99)))
        a = R.verify(model, [T], raw, scale, **CAM, pose_direction=R.MODEL_TO_CAMERA, splat=1, tau=2.0 ** -9, zmax=2.0)
        b = R.verify(model, [Ti], raw, scale, **CAM, pose_direction=R.SOURCE_ONTO_TARGET, splat=1, tau=2.0 ** -9, zmax=2.0)
        assert a[0] == b[0] and a[0][0]["n_rendered"] > 20 and a[0][0]["n_consistent"] > 0
        assert a[2][0].tobytes() == b[2][0].tobytes() and np.array_equal(a[1], b[1])
