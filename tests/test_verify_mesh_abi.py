"""CPU suite: pose verification from a triangle mesh (include/tdv_hip.h: tdv_verify_poses_mesh).  The ABI exports the entry points, lists
them in ABI_SYMBOLS, has the documented struct layout, constants and defaults, and refuses every bad argument before it writes anything.
The restatement (tests/verify_mesh_restatement.py) is held to an independent definition: point-in-triangle decided in fractions.Fraction on
the snapped positions with the top-left rule stated geometrically, the depth in Python floats, the minimum over the explicit list of the
covering triangles, the projection in scalar f32.  Then the properties the rules promise: a centre on a shared edge belongs to one triangle,
winding and culling, the rendered depth against the analytic ray-plane depth, n_rendered == the sum of the classes, the two pose directions
on exactly invertible poses - and what a mesh buys over the splat: no rim.  No compute entry point of the library runs here;
tests/test_gpu_verify_mesh.py holds the device to this restatement byte for byte."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import mesh_cases
import verify_mesh_restatement as M
import verify_restatement as R
from test_verify_abi import Outputs, P, exact_pose, inverse_exact, small_frame

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_mesh_verify_default_params", "tdv_verify_poses_mesh", "tdv_verify_poses_mesh_dev", "tdv_render_depth_mesh",
           "tdv_render_depth_mesh_dev")
NAN, INF = float("nan"), float("inf")
EYE = np.eye(4, dtype=F)
M2C = dict(pose_direction=M.MODEL_TO_CAMERA)


def test_symbols_constants_structs_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.MeshVerifyParamsC) == 16
    assert [(k, getattr(tdv.MeshVerifyParamsC, k).offset) for k, _ in tdv.MeshVerifyParamsC._fields_] == [("pose_direction", 0), ("cull", 4),
                                                                                                         ("tau", 8), ("zmax", 12)]
    assert (tdv.TDV_MESH_CULL_NONE, tdv.TDV_MESH_CULL_BACK) == (0, 1) == (M.CULL_NONE, M.CULL_BACK)
    assert tdv.TDV_MESH_MAX_VERTICES == M.MAX_VERTICES == 1 << 22 and tdv.TDV_MESH_MAX_TRIANGLES == M.MAX_TRIANGLES == 1 << 22
    assert tdv.TDV_MESH_SUBPIXEL == M.SUBPIXEL == 16
    assert tdv.TDV_MESH_COOP_PIXELS == M.COOP_PIXELS and tdv.TDV_MESH_QUEUE == M.QUEUE
    assert 1 <= M.COOP_PIXELS < R.TILE_W * R.TILE_H and M.QUEUE >= 1
    assert R.TILE_W * R.TILE_H * 4 + M.QUEUE * 64 <= 80 * 1024                     # the tile and the queue's 64-byte records: two per CU
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdv_hip.h")).read()
    for name in ("CULL_NONE", "CULL_BACK", "MAX_VERTICES", "MAX_TRIANGLES", "SUBPIXEL", "COOP_PIXELS", "QUEUE"):
        value = getattr(tdv, "TDV_MESH_" + name)
        text = header.split("#define TDV_MESH_%s " % name)[1].split("/*")[0].split("\n")[0].strip()
        assert eval(text) == value, (name, text, value)
    p = tdv.mesh_verify_params()
    assert (p.pose_direction, p.cull) == (M.DEFAULTS["pose_direction"], M.DEFAULTS["cull"]) == (0, 0)
    assert F(p.tau).tobytes() == F(M.DEFAULTS["tau"]).tobytes() and F(p.zmax).tobytes() == F(M.DEFAULTS["zmax"]).tobytes()
    lib.tdv_mesh_verify_default_params(None)                                       # a NULL is ignored
    q = tdv.mesh_verify_params(pose_direction="model_to_camera", cull="back")
    assert (q.pose_direction, q.cull) == (1, 1)
    with pytest.raises(TypeError):
        tdv.mesh_verify_params(splat=1)


# ---------------------------------------------------------------- arguments
GOOD = dict(n_vertices=4, n_triangles=2, n_poses=2, width=4, height=3, scale=1000.0, fx=50.0, fy=50.0, cx=2.0, cy=1.5, pose_direction=0, cull=0,
            tau=0.002, zmax=10.0)
# (what, the arguments replaced, whether the render entry points take the argument too)
BAD = [("n_vertices < 0", dict(n_vertices=-1), True), ("n_vertices > 2^22", dict(n_vertices=M.MAX_VERTICES + 1), True),
       ("n_triangles < 0", dict(n_triangles=-1), True), ("n_triangles > 2^22", dict(n_triangles=M.MAX_TRIANGLES + 1), True),
       ("n_poses < 0", dict(n_poses=-1), False), ("n_poses > 65536", dict(n_poses=R.MAX_POSES + 1), False),
       ("width < 0", dict(width=-1), True), ("height < 0", dict(height=-1), True),
       ("width > 8192", dict(width=R.MAX_SIDE + 1), True), ("height > 8192", dict(height=R.MAX_SIDE + 1), True),
       ("cull 2", dict(cull=2), True), ("cull -1", dict(cull=-1), True),
       ("tau == 0", dict(tau=0.0), True), ("tau < 0", dict(tau=-0.002), True), ("tau NaN", dict(tau=NAN), True), ("tau inf", dict(tau=INF), True),
       ("scale == 0", dict(scale=0.0), False), ("scale < 0", dict(scale=-1000.0), False), ("scale NaN", dict(scale=NAN), False),
       ("scale inf", dict(scale=INF), False),
       ("fx == 0", dict(fx=0.0), True), ("fx < 0", dict(fx=-50.0), True), ("fx NaN", dict(fx=NAN), True), ("fx inf", dict(fx=INF), True),
       ("fy == 0", dict(fy=0.0), True), ("fy < 0", dict(fy=-50.0), True), ("fy NaN", dict(fy=NAN), True), ("fy inf", dict(fy=INF), True),
       ("pose_direction 2", dict(pose_direction=2), True), ("pose_direction -1", dict(pose_direction=-1), True)]
NULLS = ("vertices", "triangles", "poses", "frame", "params", "results")


def inputs():
    return (np.ones((4, 3), F), np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.tile(np.eye(4, dtype=F).reshape(-1), 2),
            np.full((3, 4), 1000, np.uint16))


def _params(tdv, g, null):
    p = tdv.MeshVerifyParamsC(g["pose_direction"], g["cull"], g["tau"], g["zmax"])
    return None if "params" in null else C.byref(p)


def verify_call(tdv, dev, ctx, o, null=(), **kw):
    """Host arrays in every slot: a refused call must not look at them (the device entry point included)."""
    g = dict(GOOD, **kw)
    vtx, tri, poses, raw = inputs()
    fn = tdv.lib().tdv_verify_poses_mesh_dev if dev else tdv.lib().tdv_verify_poses_mesh
    return fn(ctx, None if "vertices" in null else P(vtx), g["n_vertices"], None if "triangles" in null else P(tri), g["n_triangles"],
              None if "poses" in null else P(poses), g["n_poses"], None if "frame" in null else P(raw), g["width"], g["height"],
              C.c_float(g["scale"]), C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(g["cx"]), C.c_float(g["cy"]), _params(tdv, g, null),
              None if "results" in null else C.byref(o.res), P(o.order))


def render_call(tdv, dev, ctx, o, null=(), **kw):
    g = dict(GOOD, **kw)
    vtx, tri, poses, _ = inputs()
    fn = tdv.lib().tdv_render_depth_mesh_dev if dev else tdv.lib().tdv_render_depth_mesh
    return fn(ctx, None if "vertices" in null else P(vtx), g["n_vertices"], None if "triangles" in null else P(tri), g["n_triangles"],
              None if "poses" in null else P(poses), g["width"], g["height"], C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(g["cx"]),
              C.c_float(g["cy"]), _params(tdv, g, null), None if "frame" in null else P(o.depth), C.byref(o.n_rendered))


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
    tests/test_gpu_verify_mesh.py refuses each bad argument on one."""
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
W, H = 40, 30
CAM = dict(fx=16.0, fy=16.0, cx=20.0, cy=15.0)             # powers of two: a vertex made by at() at z = 1 or 2 lands exactly on its (u, v)


def at(u, v, z, cam=CAM):
    """The camera-frame point whose image is (u, v) at depth z."""
    return [(u - cam["cx"]) * z / cam["fx"], (v - cam["cy"]) * z / cam["fy"], z]


def scalar_vertex(m, t, cam, direction, zmax):
    """Rule M1 for one vertex, every operation a scalar f32: (X, Y, zc) or None."""
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        if direction == M.SOURCE_ONTO_TARGET:
            d = [F(m[k] - t[12 + k]) for k in range(3)]
            c = [F(F(F(t[4 * r] * d[0]) + F(t[4 * r + 1] * d[1])) + F(t[4 * r + 2] * d[2])) for r in range(3)]
        else:
            c = [F(F(F(F(t[r] * m[0]) + F(t[4 + r] * m[1])) + F(t[8 + r] * m[2])) + t[12 + r]) for r in range(3)]
        if not (all(np.isfinite(x) for x in c) and c[2] > 0 and c[2] <= F(zmax)):
            return None
        uf, vf = F(F(F(c[0] * fx) / c[2]) + cx), F(F(F(c[1] * fy) / c[2]) + cy)
        if not (np.isfinite(uf) and np.isfinite(vf) and abs(uf) < 2 ** 20 and abs(vf) < 2 ** 20):
            return None
        return int(np.floor(F(F(uf * F(16.0)) + F(0.5)))), int(np.floor(F(F(vf * F(16.0)) + F(0.5)))), c[2]


def cross(o, p, q):
    return (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])


def owns(i, j, k):
    """Whether the edge i - j of a triangle whose third corner is k keeps the points on it: the top-left rule in words.  A horizontal edge
    keeps them when the triangle lies below it (y grows downwards), any other edge when the triangle lies to its right."""
    if i[1] == j[1]:
        return k[1] > i[1]
    x_on_edge = i[0] + (j[0] - i[0]) * (k[1] - i[1]) / (j[1] - i[1])              # the edge's line at k's height
    return k[0] > x_on_edge


def independent(vertices, triangles, T, raw, scale, cam, direction, cull, tau, zmax):
    """The definition, pixel by pixel: (result dict, depth image, the number of (pixel, triangle) pairs with the centre exactly on an edge)."""
    t = [F(x) for x in np.asarray(T, F).T.reshape(16)]
    verts = [scalar_vertex([F(x) for x in m], t, cam, direction, zmax) for m in np.asarray(vertices, F).reshape(-1, 3)]
    tris = []
    for a, b, c in np.asarray(triangles).reshape(-1, 3).tolist():
        if not all(0 <= i < len(verts) for i in (a, b, c)) or any(verts[i] is None for i in (a, b, c)):
            continue
        pa, pb, pc = ((Fraction(verts[i][0], 16), Fraction(verts[i][1], 16)) for i in (a, b, c))      # in pixels
        area2 = cross(pa, pb, pc)
        if area2 == 0 or (area2 > 0 and cull == M.CULL_BACK):                      # > 0 in an image whose y grows downwards: the back
            continue
        if area2 < 0:
            b, c, pb, pc, area2 = c, b, pc, pb, -area2
        tris.append((pa, pb, pc, area2, [1.0 / float(verts[i][2]) for i in (a, b, c)]))
    h, w = raw.shape
    inv = F(1.0 / float(F(scale)))
    out = dict(n_projected=len(tris), n_rendered=0, n_consistent=0, n_occluded=0, n_violating=0, n_unknown=0, err_q20=0)
    depth = np.zeros((h, w), F)
    on_edge = 0
    for y in range(h):
        for x in range(w):
            p = (Fraction(x), Fraction(y))
            cover = []
            for pa, pb, pc, area2, iz in tris:
                l = [cross(p, pb, pc) / area2, cross(p, pc, pa) / area2, cross(p, pa, pb) / area2]     # barycentric: they sum to 1
                assert sum(l) == 1
                if min(l) < 0:
                    continue
                edges = [(pb, pc, pa), (pc, pa, pb), (pa, pb, pc)]
                on_edge += any(v == 0 for v in l)
                if any(v == 0 and not owns(*e) for v, e in zip(l, edges)):
                    continue
                A = area2 * 256                                                    # in (1/16 px)^2, an integer, as are the weights
                wts = [v * A for v in l]
                assert A.denominator == 1 and all(v.denominator == 1 for v in wts)
                s = (float(int(wts[0])) * iz[0] + float(int(wts[1])) * iz[1]) + float(int(wts[2])) * iz[2]
                cover.append(F(float(int(A)) / s))
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
    return out, depth, on_edge


def small_mesh(seed):
    """30 triangles for a 40 x 30 frame: twelve on lattice vertices (a quad strip and a fan: shared edges through pixel centres, horizontal
    and vertical edges), fourteen random ones (some reaching off the frame, some facing away), and four unusable ones: an index of -1, an
    index of n, a vertex behind the camera, a NaN vertex; plus a repeated index (zero area)."""
    rng = np.random.default_rng(seed)
    lattice = [at(u, v, z) for u, v, z in [(4, 3, 1), (12, 3, 1), (20, 3, 2), (4, 11, 1), (12, 11, 2), (20, 11, 1),      # 0..5: a 2 x 1 strip
                                           (30, 20, 1), (36, 20, 1), (36, 26, 2), (30, 26, 1), (24, 26, 1), (24, 20, 2), (24, 14, 1),
                                           (30, 14, 1), (36, 14, 2)]]                                                    # 6: the fan's hub
    strip = [(0, 4, 1), (0, 3, 4), (1, 5, 2), (1, 4, 5)]                           # all looking at the camera: CULL_BACK keeps them
    rim = [7, 8, 9, 10, 11, 12, 13, 14]
    fan = [(6, rim[(k + 1) % 8], rim[k]) for k in range(8)]
    n0 = len(lattice)
    free = np.c_[rng.uniform(-0.4, 0.4, 30) * 2.5, rng.uniform(-0.3, 0.3, 30) * 2.5, rng.uniform(0.7, 2.2, 30)]
    rand = [tuple(int(i) + n0 for i in rng.choice(30, 3, replace=False)) for _ in range(14)]
    verts = np.array(lattice + free.tolist() + [[0.1, 0.1, -0.5], [NAN, 0.0, 1.0]], F)
    behind, nan = len(verts) - 2, len(verts) - 1
    bad = [(-1, 0, 1), (0, len(verts), 1), (behind, n0, n0 + 1), (n0 + 2, nan, n0 + 3)]
    tris = strip + fan + rand[:13] + [(n0, n0, n0 + 1)] + bad
    assert len(tris) == 30
    return verts, np.array(tris, np.int32)


@pytest.mark.parametrize("direction", [M.SOURCE_ONTO_TARGET, M.MODEL_TO_CAMERA])
@pytest.mark.parametrize("cull", [M.CULL_NONE, M.CULL_BACK])
def test_against_the_independent_definition(direction, cull):
    scale, tau, zmax = 1000.0, 0.004, 2.0                                          # the lattice reaches z = 2 = zmax exactly
    verts, tris = small_mesh(3 + cull)
    tilt = exact_pose((1, 0, 2), (-1, 1, 1), (0.125, -0.0625, 0.03125))
    poses = np.stack([EYE, tilt, np.full((4, 4), np.nan, F)])
    first = M.render_keys(verts, tris, poses[0], W, H, **CAM, pose_direction=direction, cull=cull, zmax=zmax)[0]
    raw = small_frame(M.depth_of(first), scale, 11 + cull)
    res, order, depths = M.verify(verts, tris, poses, raw, scale, **CAM, pose_direction=direction, cull=cull, tau=tau, zmax=zmax)
    seen, edge_hits = set(), 0
    for T, r, d in zip(poses, res, depths):
        ref, ref_depth, on_edge = independent(verts, tris, T, raw, scale, CAM, direction, cull, tau, zmax)
        assert r == ref, (direction, cull, r, ref)
        assert d.tobytes() == ref_depth.tobytes()
        assert r["n_rendered"] == r["n_consistent"] + r["n_occluded"] + r["n_violating"] + r["n_unknown"]
        seen |= {k for k in M.RESULT if r[k] > 0}
        edge_hits += on_edge
    assert seen == set(M.RESULT), seen                                             # every class occurred
    assert edge_hits >= 20                                                         # ... and the tie rule decided many centres
    assert res[2] == dict.fromkeys(M.RESULT, 0)
    assert 12 < res[0]["n_projected"] < 25                                         # the lattice's 12; zmax, the facing or both cut random ones
    score = [r["n_consistent"] - r["n_violating"] for r in res]
    assert order.tolist() == sorted(range(3), key=lambda i: (-score[i], i))


# ---------------------------------------------------------------- the properties
CAM2 = dict(fx=256.0, fy=256.0, cx=64.0, cy=48.0)           # at(u, v, 1.0, CAM2) is exact for integer u, v


def covered(verts, tris, w=150, h=140, cam=CAM2, pose=EYE, **prm):
    keys, n = M.render_keys(np.asarray(verts, F), np.asarray(tris, np.int32).reshape(-1, 3), pose, w, h, **cam, **dict(M2C, **prm))
    return keys != M.EMPTY, n


def test_a_shared_edge_belongs_to_one_triangle():
    """A 30 x 30 pixel square with its corners on pixel centres, cut along the diagonal that passes through 31 centres: 900 pixels (the top
    and the left edge are the square's, the other two are not), 465 + 435, none twice.  Both windings of the pair, both diagonals."""
    sq = [at(u, v, 1.0, CAM2) for u, v in [(10, 10), (40, 10), (40, 40), (10, 40)]]
    for tris in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 3, 2)], [(0, 1, 3), (1, 2, 3)], [(3, 1, 0), (3, 2, 1)]):
        both, n = covered(sq, tris)
        one, two = covered(sq, [tris[0]])[0], covered(sq, [tris[1]])[0]
        assert n == 2 and both.sum() == 900 and sorted([one.sum(), two.sum()]) == [435, 465]
        assert not (one & two).any() and ((one | two) == both).all()
        ys, xs = np.nonzero(both)
        assert (xs.min(), xs.max(), ys.min(), ys.max()) == (10, 39, 10, 39)        # the top-left rule


def test_a_fan_covers_every_pixel_once():
    """Eight triangles around a hub on a pixel centre, the spokes horizontal, vertical and diagonal through pixel centres; the hub itself
    lies on every triangle and belongs to exactly one."""
    hub = (60, 50)
    rim = [(80, 50), (80, 70), (60, 70), (40, 70), (40, 50), (40, 30), (60, 30), (80, 30)]
    verts = [at(*hub, 1.0, CAM2)] + [at(u, v, 1.0 + 0.03125 * k, CAM2) for k, (u, v) in enumerate(rim)]
    tris = [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)]
    whole, n = covered(verts, tris)
    each = [covered(verts, [t])[0] for t in tris]
    assert n == 8 and whole.sum() == 40 * 40 == sum(e.sum() for e in each)
    assert (np.sum(each, axis=0) == whole).all() and whole[50, 60] and sum(e[50, 60] for e in each) == 1
    flipped = [(a, c, b) for a, b, c in tris]                                      # the other facing: the same, once each
    assert (covered(verts, flipped)[0] == whole).all()


def test_winding_and_cull():
    """(b - a) x (c - a) towards the camera (-z): the front.  CULL_BACK renders it and drops the other winding; CULL_NONE renders both alike."""
    a, b, c = at(20, 20, 1.0, CAM2), at(90.3, 31.7, 1.25, CAM2), at(48.6, 88.1, 1.5, CAM2)
    va, vb, vc = (np.array(p) for p in (a, b, c))
    assert np.cross(vc - va, vb - va)[2] < 0                                       # (a, c, b) looks at the camera
    front, back = [(0, 2, 1)], [(0, 1, 2)]
    f_none, _ = covered([a, b, c], front)
    b_none, _ = covered([a, b, c], back)
    f_cull, nf = covered([a, b, c], front, cull=M.CULL_BACK)
    b_cull, nb = covered([a, b, c], back, cull=M.CULL_BACK)
    assert f_none.sum() > 1500 and (f_none == b_none).all() and (f_cull == f_none).all() and nf == 1
    assert not b_cull.any() and nb == 0
    kf = M.render_keys(np.array([a, b, c], F), np.array(front, np.int32), EYE, 150, 140, **CAM2, **M2C)[0]
    kb = M.render_keys(np.array([a, b, c], F), np.array(back, np.int32), EYE, 150, 140, **CAM2, **M2C)[0]
    assert kf.tobytes() == kb.tobytes()                                            # the depths too
    # a closed box seen from outside: with culling exactly its front faces, and the same image (the back faces are behind them)
    verts, tris = mesh_cases.box((0.2, 0.12, 0.06), (0.01, -0.02, 0.0))
    c_, s_ = np.cos(0.5), np.sin(0.5)
    pose = np.array([[c_, 0, s_, 0.0], [0.3 * s_, 0.954, -0.3 * c_, 0.0], [-0.954 * s_, 0.3, 0.954 * c_, 0.6], [0, 0, 0, 1]], F)
    cam = dict(fx=150.0, fy=150.0, cx=75.0, cy=70.0)
    k_none, n_none = M.render_keys(verts, tris, pose, 150, 140, **cam, **M2C)
    k_back, n_back = M.render_keys(verts, tris, pose, 150, 140, **cam, cull=M.CULL_BACK, **M2C)
    assert n_none == 12 and n_back == 6 and k_none.tobytes() == k_back.tobytes() and (k_none != M.EMPTY).sum() > 800


def test_rendered_depth_against_the_ray_plane_depth():
    """A tilted planar quad (two triangles) at the identity pose, against the plane's depth along each pixel's ray.  With the true inverse
    depth iz(u, v) = A u + B v + C, the rendered 1 / zr is the affine function through the vertices' own 1 / zc, placed at the snapped
    positions: the difference of two affine functions is bounded over a triangle by its corner values, and a corner's is (A, B) . (the
    corner's displacement), at most (|A| + |B|) * d per axis-displacement d.  d <= 1/32 px from the snap (half of 1/16), plus the f32
    error of uf and vf themselves, which is MEASURED here against a float64 projection of the same f32 vertices and held to 4 ulps of the
    largest |uf| (measured on the CPU: 0.61 ulp for these vertices).  Beyond the displacement: the fourth vertex is off the plane of the
    first three by at most half an f32 ulp of its depth, and zr itself is rounded to f32 once - 2^-24 of iz each.  The prototype reached 0.40 of
    (|A| + |B|) / 32."""
    w, h = 150, 140
    cam = dict(fx=300.0, fy=300.0, cx=64.3, cy=47.7)
    V = np.array([[-.2, -.15, 1.0], [.25, -.12, 1.3], [.22, .2, 1.1], [-.18, .17, 0.8]], F)
    Vd = V.astype(np.float64)
    n = np.cross(Vd[1] - Vd[0], Vd[2] - Vd[0])
    d = n @ Vd[0]
    V[3, 2] = F((d - n[0] * Vd[3, 0] - n[1] * Vd[3, 1]) / n[2])                    # onto the plane of the first three, rounded to f32
    Vd = V.astype(np.float64)
    tris = np.array([(0, 1, 2), (0, 2, 3)], np.int32)
    usable, _, _, zc, uf, vf = M.project(V, EYE, **cam, pose_direction=M.MODEL_TO_CAMERA, zmax=10.0)
    assert usable.all() and (zc == V[:, 2]).all()
    uf64, vf64 = Vd[:, 0] * cam["fx"] / Vd[:, 2] + cam["cx"], Vd[:, 1] * cam["fy"] / Vd[:, 2] + cam["cy"]
    ulp = float(np.spacing(F(max(np.abs(uf).max(), np.abs(vf).max()))))
    measured = max(np.abs(uf - uf64).max(), np.abs(vf - vf64).max()) / ulp
    print("f32 error of uf, vf: %.3f ulp of %.1f px" % (measured, max(np.abs(uf).max(), np.abs(vf).max())))
    assert measured <= 4.0
    keys, used = M.render_keys(V, tris, EYE, w, h, **cam, **M2C)
    on = keys != M.EMPTY
    assert used == 2 and on.sum() > 8000
    A, B = n[0] / cam["fx"] / d, n[1] / cam["fy"] / d
    yy, xx = np.mgrid[0:h, 0:w]
    iz_true = (n[0] * (xx - cam["cx"]) / cam["fx"] + n[1] * (yy - cam["cy"]) / cam["fy"] + n[2]) / d
    err = np.abs(1.0 / keys.view(F)[on].astype(np.float64) - iz_true[on])
    bound = (abs(A) + abs(B)) * (1.0 / 32 + 4.0 * ulp) + 2.0 ** -23 * iz_true[on].max()
    print("max |1/zr - iz| = %.3e, bound %.3e (%.2f of it)" % (err.max(), bound, err.max() / bound))
    assert err.max() <= bound
    # ... and the silhouette is the quad's: a pixel is rendered iff its centre is inside the quad of the snapped corners (boundary aside)
    _, X, Y, _, _, _ = M.project(V, EYE, **cam, pose_direction=M.MODEL_TO_CAMERA, zmax=10.0)
    q = np.stack([X, Y], 1) / 16.0
    e = [(q[(k + 1) % 4, 0] - q[k, 0]) * (yy - q[k, 1]) - (q[(k + 1) % 4, 1] - q[k, 1]) * (xx - q[k, 0]) for k in range(4)]
    strictly_in, strictly_out = np.all([v > 0 for v in e], 0), np.any([v < 0 for v in e], 0)
    assert on[strictly_in].all() and not on[strictly_out].any()


# ---------------------------------------------------------------- what it buys
@pytest.fixture(scope="module")
def part_over_a_floor(synth):
    """The relief part as a mesh over a floor, the frame rendered from the mesh itself at the true pose and rounded to u16."""
    w, h, scale, f = 160, 120, 1000.0, 150.0
    cam = dict(fx=f, fy=f, cx=80.0, cy=60.0)
    part = synth.ReliefPart(seed=3)
    verts, tris = mesh_cases.relief(part, 0.002)
    true = synth.scan_pose(0.5).astype(F)                                          # model -> camera
    depth = M.depth_of(M.render_keys(verts, tris, true, w, h, **cam, **M2C)[0])
    on = depth != 0
    assert on.sum() > 800
    raw = np.rint(np.where(on, depth, F(0.6)).astype(np.float64) * scale).astype(np.uint16)
    return dict(w=w, h=h, scale=scale, cam=cam, part=part, verts=verts, tris=tris, true=true, raw=raw, on=on, depth=depth)


def test_the_true_pose_has_no_rim(part_over_a_floor, synth):
    """tau just above half a raw step (the frame's rounding, 0.5 / scale; the f32 roundings of zo and of the difference are below 1e-7 m
    and the 0.002 / scale on top is 2e-6 m): every rendered pixel of the mesh is consistent - the silhouette is exact and the depth is the
    frame's own.  The splat of a dense sampling of the same part at splat 1 reaches a pixel past the silhouette onto the floor: violating."""
    c = part_over_a_floor
    tau = 0.502 / c["scale"]
    res, order, _ = M.verify(c["verts"], c["tris"], [c["true"]], c["raw"], c["scale"], **c["cam"], tau=tau, **M2C)
    r = res[0]
    assert r["n_violating"] == 0 and r["n_occluded"] == 0 and r["n_unknown"] == 0
    assert r["n_consistent"] == r["n_rendered"] == int(c["on"].sum()) and r["n_projected"] == len(c["tris"])
    dense = c["part"].surface_points(0.001).astype(F)
    s = R.verify(dense, [c["true"]], c["raw"], c["scale"], **c["cam"], pose_direction=R.MODEL_TO_CAMERA, splat=1, tau=tau)[0][0]
    assert s["n_violating"] > 0 and s["n_rendered"] > r["n_rendered"]
    print("mesh: %d rendered, all consistent; splat 1: %d rendered, %d violating" % (r["n_rendered"], s["n_rendered"], s["n_violating"]))


def test_a_pose_in_free_space_scores_negative(part_over_a_floor):
    c = part_over_a_floor
    extent = float(c["depth"][c["on"]].max() - c["depth"][c["on"]].min())
    free = c["true"].copy()
    free[2, 3] -= 0.05                                                             # towards the camera by more than the part's depth extent
    assert 0.05 > extent + 0.002
    res, order, _ = M.verify(c["verts"], c["tris"], [free, c["true"]], c["raw"], c["scale"], **c["cam"], tau=0.002, **M2C)
    assert res[0]["n_violating"] == res[0]["n_rendered"] > 800 and res[0]["n_consistent"] - res[0]["n_violating"] < 0
    assert res[1]["n_consistent"] == res[1]["n_rendered"] and order.tolist() == [1, 0]


# ---------------------------------------------------------------- sums and directions
@pytest.mark.parametrize("perm, signs", [((0, 1, 2), (1, 1, 1)), ((1, 0, 2), (1, -1, 1)), ((2, 0, 1), (-1, 1, -1)), ((0, 2, 1), (-1, -1, -1))])
def test_both_directions_agree_on_exactly_invertible_poses(perm, signs):
    """T under one direction and its exact inverse under the other: the same bytes; n_rendered is the sum of the four classes."""
    w, h, scale = 40, 30, 1024.0
    verts_cam, tris = small_mesh(9)                                                # the vertices in camera coordinates
    for t in ((0.25, -0.5, 0.125), (-1.0, 0.0, 2.0 ** -6)):
        T = exact_pose(perm, signs, t)                                             # model -> camera
        Ti = inverse_exact(T)
        with np.errstate(invalid="ignore"):
            verts = ((verts_cam.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)          # R^T (p - t): the model whose image it is
        raw = small_frame(M.depth_of(M.render_keys(verts, tris, T, w, h, **CAM, **M2C)[0]), scale, sum(perm) + 5)
        for cull in (M.CULL_NONE, M.CULL_BACK):
            a = M.verify(verts, tris, [T], raw, scale, **CAM, pose_direction=M.MODEL_TO_CAMERA, cull=cull, tau=2.0 ** -8, zmax=2.0)
            b = M.verify(verts, tris, [Ti], raw, scale, **CAM, pose_direction=M.SOURCE_ONTO_TARGET, cull=cull, tau=2.0 ** -8, zmax=2.0)
            r = a[0][0]
            assert a[0] == b[0] and r["n_rendered"] > 100 and r["n_consistent"] > 0
            assert r["n_rendered"] == r["n_consistent"] + r["n_occluded"] + r["n_violating"] + r["n_unknown"]
            assert a[2][0].tobytes() == b[2][0].tobytes() and np.array_equal(a[1], b[1])
