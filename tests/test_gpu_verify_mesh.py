"""Pose verification from a mesh on the device (include/tdv_hip.h: tdv_verify_poses_mesh) against the restatement of
tests/verify_mesh_restatement.py, byte for byte: the result structs and the order from the host and the device entry points, the depth
image from tdv_render_depth_mesh and tdv_render_depth_mesh_dev, each test on a Context of its own.  The shapes are the smallest at which
each mechanism can go wrong: the wave (63, 64, 65), the workgroup's block of triangles (L - 1, L, L + 1, 2 L + 1 with L = TDV_VERIFY_LANES)
in the triangle count; frames of one tile less, exactly and one more than a tile; a triangle's pixel box inside a tile one below, at and
one above TDV_MESH_COOP_PIXELS (where a lane hands its triangle to the workgroup); one below, at, one above and past twice
TDV_MESH_QUEUE large triangles in one tile (where the queue drains in rounds); pose counts across the plan's scan block of 1,024."""
import numpy as np
import pytest
import torch

import mesh_cases
import verify_mesh_restatement as M
import verify_restatement as R
from test_verify_abi import Outputs, exact_pose, small_frame
from test_verify_mesh_abi import BAD, CAM2, at, null_refusals, refusals

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
L = R.LANES
COOP, QUEUE = M.COOP_PIXELS, M.QUEUE
M2C = dict(pose_direction=M.MODEL_TO_CAMERA)
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
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(16, np.uint8)).to(DEV)


def _mesh(verts, tris):
    return np.ascontiguousarray(verts, F).reshape(-1, 3), np.ascontiguousarray(tris, np.int32).reshape(-1, 3)


def dev_verify(ctx, verts, tris, poses, raw, scale, cam, **prm):
    verts, tris = _mesh(verts, tris)
    vt, tt, rt = _up(verts), _up(tris), _up(np.ascontiguousarray(raw, np.uint16))
    torch.cuda.synchronize()                                 # the uploads are torch's; the ctx runs on a stream of its own
    h, w = raw.shape
    return ctx.verify_poses_mesh_dev(vt.data_ptr(), len(verts), tt.data_ptr(), len(tris), poses, rt.data_ptr(), w, h, scale, cam["fx"], cam["fy"],
                                     cam["cx"], cam["cy"], **prm)


def dev_render(ctx, verts, tris, pose, w, h, cam, **prm):
    verts, tris = _mesh(verts, tris)
    vt, tt = _up(verts), _up(tris)
    out = torch.full((w * h + PAD,), -9.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    n = ctx.render_depth_mesh_dev(vt.data_ptr(), len(verts), tt.data_ptr(), len(tris), pose, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                  out.data_ptr(), **prm)
    ctx.synchronize()
    got = out.cpu().numpy()
    assert (got[w * h:] == -9).all(), "written beyond the image"
    return got[:w * h].reshape(h, w), n


def check(ctx, verts, tris, poses, raw, scale, cam, what, render=(0,), **prm):
    """Host and device entry points against the restatement: results, order, and the depth image of the poses listed in `render`."""
    verts, tris = _mesh(verts, tris)
    raw = np.ascontiguousarray(raw, np.uint16)
    h, w = raw.shape
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    ref, order, depths = M.verify(verts, tris, poses, raw, scale, **cam, **dict(M.DEFAULTS, **prm))
    for r in ref:
        assert r["n_rendered"] == r["n_consistent"] + r["n_occluded"] + r["n_violating"] + r["n_unknown"]
    for name, (got, got_order) in (("host", ctx.verify_poses_mesh(verts, tris, poses, raw, scale, **cam, **prm)),
                                   ("dev", dev_verify(ctx, verts, tris, poses, raw, scale, cam, **prm))):
        assert got == ref, (what, name, [(i, g, r) for i, (g, r) in enumerate(zip(got, ref)) if g != r][:3])
        assert got_order.dtype == np.int32 and np.array_equal(got_order, order), (what, name, got_order, order)
    rprm = {k: v for k, v in prm.items() if k != "tau"}
    for i in render:
        if 0 <= i < len(poses):
            n_rendered = int((depths[i] != 0).sum())
            assert n_rendered == ref[i]["n_rendered"]
            img = ctx.render_depth_mesh(verts, tris, poses[i], w, h, **cam, **rprm)
            assert img.dtype == F and img.shape == (h, w)
            assert img.tobytes() == depths[i].tobytes(), (what, "render_depth_mesh", i, int((img != depths[i]).sum()))
            img, n = dev_render(ctx, verts, tris, poses[i], w, h, cam, **rprm)
            assert img.tobytes() == depths[i].tobytes() and n == n_rendered, (what, "render_depth_mesh_dev", i, n, n_rendered)
    return ref, order, depths


def soup(n, seed, w, h, cam, size=3.0, spill=1.1, z=(0.7, 1.3)):
    """n triangles of their own three vertices each, centred anywhere on the frame and a little beyond it, corners within `size` pixels of
    the centre, either facing, every corner at its own depth."""
    rng = np.random.default_rng(seed)
    cu, cv = rng.uniform(-0.5, w - 0.5, n), rng.uniform(-0.5, h - 0.5, n)
    cu, cv = (cu - cam["cx"]) * spill + cam["cx"], (cv - cam["cy"]) * spill + cam["cy"]
    u = cu[:, None] + rng.uniform(-size, size, (n, 3))
    v = cv[:, None] + rng.uniform(-size, size, (n, 3))
    zc = rng.uniform(*z, n)[:, None] * rng.uniform(0.97, 1.03, (n, 3))
    verts = np.stack([(u - cam["cx"]) * zc / cam["fx"], (v - cam["cy"]) * zc / cam["fy"], zc], -1).reshape(-1, 3).astype(F)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def sheet(w, h, cam, step, seed, margin=4.0):
    """A jittered grid of vertices over the whole frame and `margin` pixels beyond it, two triangles per cell, each vertex at its own
    depth: every pixel of the frame is covered."""
    rng = np.random.default_rng(seed)
    us, vs = np.arange(-margin, w - 1 + margin + step, step), np.arange(-margin, h - 1 + margin + step, step)
    U, V = np.meshgrid(us, vs)
    inner = np.zeros_like(U, bool)
    inner[1:-1, 1:-1] = True
    U = U + inner * rng.uniform(-0.3, 0.3, U.shape) * step
    V = V + inner * rng.uniform(-0.3, 0.3, V.shape) * step
    zc = rng.uniform(0.8, 1.2, U.shape)
    verts = np.stack([(U - cam["cx"]) * zc / cam["fx"], (V - cam["cy"]) * zc / cam["fy"], zc], -1).reshape(-1, 3).astype(F)
    nx, ny = len(us), len(vs)
    j, i = (a.ravel() for a in np.mgrid[0:ny - 1, 0:nx - 1])
    v00, v10, v01, v11 = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
    tris = np.concatenate([np.stack([v00, v11, v10], 1), np.stack([v00, v01, v11], 1)]).astype(np.int32)
    return verts, tris[rng.permutation(len(tris))]


def frame_for(verts, tris, pose, w, h, cam, scale, seed, **prm):
    """An observed frame around the mesh's own rendered depth (test_verify_abi.small_frame): every class occurs."""
    prm = {k: v for k, v in dict(M.DEFAULTS, **prm).items() if k != "tau"}
    return small_frame(M.depth_of(M.render_keys(verts, tris, pose, w, h, **cam, **prm)[0]), scale, seed)


def nudged(T, seed, trans=0.01):
    rng = np.random.default_rng(seed)
    T = np.array(T, F)
    T[:3, 3] += rng.uniform(-trans, trans, 3).astype(F)
    return T


def pixel_boxes(verts, tris, pose, w, h, cam, x0=0, y0=0, x1=None, y1=None, **prm):
    """The number of pixel centres in each usable triangle's box inside [x0, x1] x [y0, y1] (default: the frame; a frame of one tile: the
    tile), from the restatement's snapped positions."""
    s = M.setup(verts, tris, pose, **cam, **{k: v for k, v in dict(M.DEFAULTS, **prm).items() if k != "tau"})
    x1, y1 = (w - 1 if x1 is None else x1), (h - 1 if y1 is None else y1)
    a0, a1 = np.maximum(-(-s["X"].min(1) // 16), x0), np.minimum(s["X"].max(1) // 16, x1)
    b0, b1 = np.maximum(-(-s["Y"].min(1) // 16), y0), np.minimum(s["Y"].max(1) // 16, y1)
    return np.where((a0 <= a1) & (b0 <= b1), (a1 - a0 + 1) * (b1 - b0 + 1), 0)


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1])
def test_triangle_counts(vctx, n):
    w, h = 37, 29
    cam = cam_of(w, h)
    verts, tris = soup(n, 300 + n, w, h, cam)
    raw = frame_for(*soup(300, 1, w, h, cam), EYE, w, h, cam, 1000.0, n, **M2C)
    for cull in (M.CULL_NONE, M.CULL_BACK):
        ref, _, _ = check(vctx, verts, tris, [EYE, nudged(EYE, n)], raw, 1000.0, cam, ("triangles", n, cull), render=(0, 1), cull=cull, **M2C)
        # (a random triangle of a few pixels now and then has a snapped area of zero)
        assert n - 3 <= ref[0]["n_projected"] <= n if cull == M.CULL_NONE else (n < 4 or n / 4 < ref[0]["n_projected"] < 3 * n / 4)
        assert n < 63 or ref[0]["n_rendered"] > 0


FRAMES = [(1, 1), (R.TILE_W - 1, R.TILE_H + 1), (R.TILE_W, R.TILE_H), (R.TILE_W + 1, R.TILE_H - 1), (150, 140)]


@pytest.mark.parametrize("w, h", FRAMES)
def test_frame_sizes_around_the_tile(vctx, w, h):
    cam = cam_of(w, h)
    verts, tris = sheet(w, h, cam, 9.0, w * 1000 + h)
    raw = frame_for(verts, tris, EYE, w, h, cam, 1000.0, w + h, **M2C)
    ref, _, depths = check(vctx, verts, tris, [EYE, nudged(EYE, w + h, 0.004)], raw, 1000.0, cam, ("frame", w, h), render=(0, 1), **M2C)
    assert ref[0]["n_rendered"] == w * h and (depths[0] != 0).all()                # the box is the frame: 1, 2 or 4 tiles
    assert ref[0]["n_projected"] == len(tris)


def test_a_box_that_starts_past_the_first_tile(vctx):
    """A small mesh in the far corner of a 300 x 260 frame: its box begins in tile (1, 1) and ends in the frame's last, partial tiles; then
    with a second patch that makes the box 3 x 2 tiles starting inside tile (0, 0)."""
    w, h = 300, 260
    cam = cam_of(w, h)
    corner = soup(300, 5, 46, 8, dict(cam, cx=cam["cx"] - 253, cy=cam["cy"] - 251), size=2.5, spill=1.0)      # images in [252.5, 298.5] x [250.5, 258.5] + 2.5
    raw = frame_for(*corner, EYE, w, h, cam, 1000.0, 3, **M2C)
    ref, _, depths = check(vctx, *corner, [EYE], raw, 1000.0, cam, "corner", **M2C)
    ys, xs = np.nonzero(depths[0])
    assert xs.min() >= 2 * R.TILE_W - 7 and ys.min() >= 2 * R.TILE_H - 9 and xs.max() == w - 1 and ys.max() == h - 1
    mid = soup(300, 6, 60, 15, dict(cam, cx=cam["cx"] - 100, cy=cam["cy"] - 120), size=2.5, spill=1.0)
    verts, tris = np.r_[corner[0], mid[0]], np.r_[corner[1], mid[1] + len(corner[0])]
    check(vctx, verts, tris, [EYE, nudged(EYE, 9)], frame_for(verts, tris, EYE, w, h, cam, 1000.0, 4, **M2C), 1000.0, cam, "two by two",
          render=(0, 1), **M2C)


# ---------------------------------------------------------------- single triangles and the frame
def test_triangles_across_tiles_and_off_the_frame(vctx):
    w, h = 150, 140
    cam = dict(CAM2, cx=70.0, cy=60.0)
    raw = np.full((h, w), 1000, np.uint16)

    def tri(*uvz):
        return np.array([at(u, v, z, cam) for u, v, z in uvz], F), np.array([[0, 2, 1]], np.int32)

    four = tri((100, 90, 0.9), (149, 133.3, 1.1), (110.2, 139, 1.0))               # around the corner (128, 128) where four tiles meet
    ref, _, depths = check(vctx, *four, [EYE], raw, 1000.0, cam, "four tiles", **M2C)
    on = depths[0] != 0
    assert on[:128, :128].any() and on[:128, 128:].any() and on[128:, :128].any() and on[128:, 128:].any()
    whole = tri((-40, -30, 0.8), (400, -20, 1.2), (60, 500, 1.0))                  # the frame lies inside it
    ref, _, _ = check(vctx, *whole, [EYE], raw, 1000.0, cam, "the frame inside a triangle", **M2C)
    assert ref[0]["n_rendered"] == w * h
    outside = tri((160, 20, 1.0), (300, 40, 1.0), (170, 130, 1.0))
    ref, _, _ = check(vctx, *outside, [EYE], raw, 1000.0, cam, "wholly outside", **M2C)
    assert ref[0]["n_projected"] == 1 and ref[0]["n_rendered"] == 0
    beside = tri((-300, 200, 1.0), (-20, 30, 1.0), (-10, 400, 1.0))                # its box overlaps the frame's rows and columns, it does not
    check(vctx, *beside, [EYE], raw, 1000.0, cam, "outside, box across", **M2C)
    far = tri((20, 30, 0.9), (5000, 70, 1.4), (40, -7000, 1.1))                    # vertices thousands of pixels away
    ref, _, _ = check(vctx, *far, [EYE], raw, 1000.0, cam, "a far vertex", **M2C)
    assert 500 < ref[0]["n_rendered"] < w * h
    edge = tri((1000000, 10, 1.0), (-1000000, 20, 1.0), (30, 1000000, 1.0))        # |uf| just inside 2^20
    ref, _, _ = check(vctx, *edge, [EYE], raw, 1000.0, cam, "at the pixel limit", **M2C)
    assert ref[0]["n_projected"] == 1 and ref[0]["n_rendered"] > 5000
    together = np.r_[four[0], whole[0], outside[0], far[0]], np.array([[0, 2, 1], [3, 5, 4], [6, 8, 7], [9, 11, 10], [9, 10, 11]], np.int32)
    check(vctx, *together, [EYE, nudged(EYE, 1)], frame_for(*together, EYE, w, h, cam, 1000.0, 2, **M2C), 1000.0, cam, "together",
          render=(0, 1), **M2C)


def _dims(p):
    """bw x bh = p, as square as it goes."""
    bw = next(d for d in range(int(p ** 0.5), 0, -1) if p % d == 0)
    return p // bw, bw


@pytest.mark.parametrize("pixels", [COOP - 1, COOP, COOP + 1])
def test_pixel_box_at_the_cooperative_threshold(vctx, pixels):
    """A right triangle on lattice corners whose pixel box holds exactly `pixels` centres; the same cut by a tile's edge so that the part
    inside the first tile holds them; and both among small triangles."""
    w, h = 150, 140
    cam = dict(CAM2, cx=70.0, cy=60.0)
    bw, bh = _dims(pixels)
    raw = np.full((h, w), 1000, np.uint16)
    whole = np.array([at(10, 10, 1.0, cam), at(10 + bw - 1, 10, 1.25, cam), at(10, 10 + bh - 1, 0.75, cam)], F)
    front = np.array([[0, 2, 1]], np.int32)
    assert pixel_boxes(whole, front, EYE, w, h, cam, **M2C).tolist() == [pixels]
    check(vctx, whole, front, [EYE], raw, 1000.0, cam, ("box", pixels), **M2C)
    x0 = R.TILE_W - bw                                                             # columns x0 .. 127 in the first tile, 128 .. beyond
    cut = np.array([at(x0, 20, 1.0, cam), at(x0 + bw + 14, 20, 1.25, cam), at(x0, 20 + bh - 1, 0.75, cam)], F)
    assert pixel_boxes(cut, front, EYE, w, h, cam, x1=R.TILE_W - 1, **M2C).tolist() == [pixels]
    assert pixel_boxes(cut, front, EYE, w, h, cam, x0=R.TILE_W, **M2C)[0] not in (0, pixels)
    check(vctx, cut, front, [EYE], raw, 1000.0, cam, ("box cut by a tile", pixels), **M2C)
    sv, st = soup(200, pixels, w, h, cam)
    verts, tris = np.r_[whole, cut, sv], np.r_[front, front + 3, st + 6]
    check(vctx, verts, tris, [EYE, nudged(EYE, 2, 0.002)], frame_for(verts, tris, EYE, w, h, cam, 1000.0, 1, **M2C), 1000.0, cam,
          ("boxes among small ones", pixels), render=(0, 1), **M2C)


@pytest.mark.parametrize("n", [QUEUE - 1, QUEUE, QUEUE + 1, 2 * QUEUE + 1])
def test_large_triangles_in_one_tile(vctx, n):
    """n triangles of more than TDV_MESH_COOP_PIXELS pixels each in a frame of one tile: the queue takes them in one, two or three rounds;
    then the same among 1,500 small ones, spread over two blocks of the workgroup's triangle loop."""
    w, h = 100, 90
    cam = cam_of(w, h)
    inner = dict(cam, cx=cam["cx"] - 15, cy=cam["cy"] - 15)                        # centres 15 pixels inside the frame
    verts, tris = soup(2 * n, 40 + n, w - 30, h - 30, inner, size=12.0, spill=1.0)
    large = np.nonzero(pixel_boxes(verts, tris, EYE, w, h, cam, **M2C) > COOP)[0][:n]
    verts, tris = verts.reshape(-1, 3, 3)[large].reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    boxes = pixel_boxes(verts, tris, EYE, w, h, cam, **M2C)
    assert len(boxes) == n and (boxes > COOP).all()                                # n usable triangles, every one a large one
    raw = frame_for(verts, tris, EYE, w, h, cam, 1000.0, n, **M2C)
    check(vctx, verts, tris, [EYE, nudged(EYE, n, 0.003)], raw, 1000.0, cam, ("large triangles", n), render=(0, 1), **M2C)
    sv, st = soup(1500, n, w, h, cam, size=2.0)
    rng = np.random.default_rng(n)
    mv, mt = np.r_[verts, sv], np.r_[tris, st + len(verts)]
    mt = mt[rng.permutation(len(mt))]
    check(vctx, mv, mt, [EYE], raw, 1000.0, cam, ("large among small", n), **M2C)


def test_large_and_small_mixed_over_four_tiles(vctx):
    w, h = 150, 140
    cam = cam_of(w, h)
    sv, st = soup(2000, 11, w, h, cam, size=2.5)
    bv, bt = soup(60, 12, w, h, cam, size=40.0)
    verts, tris = np.r_[sv, bv], np.r_[st, bt + len(sv)]
    tris = tris[np.random.default_rng(3).permutation(len(tris))]
    raw = frame_for(verts, tris, EYE, w, h, cam, 1000.0, 5, **M2C)
    for cull in (M.CULL_NONE, M.CULL_BACK):
        check(vctx, verts, tris, [EYE, nudged(EYE, 4), nudged(EYE, 5, 0.05)], raw, 1000.0, cam, ("mixed", cull), render=(0, 2), cull=cull, **M2C)


def test_duplicates_and_intersections(vctx):
    w, h = 100, 90
    cam = dict(CAM2, cx=50.0, cy=45.0)
    a = [at(10, 10, 0.8, cam), at(90, 20, 1.2, cam), at(30, 80, 1.0, cam)]
    b = [at(15, 70, 0.8, cam), at(85, 75, 0.85, cam), at(50, 5, 1.3, cam)]         # crosses a in depth
    verts = np.array(a + b + a, F)                                                 # the last three: a again, as vertices of its own
    tris = np.array([[0, 2, 1], [3, 5, 4], [0, 2, 1], [0, 1, 2], [6, 8, 7], [2, 0, 1]], np.int32)
    raw = frame_for(verts, tris, EYE, w, h, cam, 1000.0, 2, **M2C)
    ref, _, depths = check(vctx, verts, tris, [EYE, nudged(EYE, 3)], raw, 1000.0, cam, "duplicates", render=(0, 1), **M2C)
    one = M.depth_of(M.render_keys(verts, tris[:2], EYE, w, h, **cam, **M2C)[0])
    assert ref[0]["n_projected"] == 6 and depths[0].tobytes() == one.tobytes()     # the copies change nothing
    ka = M.render_keys(verts, tris[:1], EYE, w, h, **cam, **M2C)[0]
    kb = M.render_keys(verts, tris[1:2], EYE, w, h, **cam, **M2C)[0]
    both = (ka != M.EMPTY) & (kb != M.EMPTY)
    assert (ka[both] < kb[both]).any() and (kb[both] < ka[both]).any()             # each is in front somewhere
    check(vctx, verts, tris, [EYE], raw, 1000.0, cam, "duplicates, culled", cull=M.CULL_BACK, **M2C)


def test_unusable_triangles(vctx):
    """Zero area, repeated indices, indices of -1 and n_vertices (and far beyond), NaN and infinite vertices, a vertex behind the camera and
    at zc == 0, one just beyond zmax and one on it, a pose of NaNs: dropped, without a fault and without a trace in the result."""
    w, h = 64, 48
    cam = cam_of(w, h)
    zmax = F(1.25)
    good, gt = soup(40, 3, w, h, cam, size=6.0, z=(0.9, 1.1))
    n0 = len(good)
    odd = np.array([at(10, 10, 1.0, cam), at(20, 20, 1.0, cam), at(30, 30, 1.0, cam),          # n0 + 0..2: collinear
                    [np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [0.1, 0.1, -0.5], [0.1, 0.0, 0.0],   # + 3..7
                    at(40, 10, float(np.nextafter(zmax, F(2))), cam), at(44, 30, float(zmax), cam), at(20, 40, 1.0, cam)], F)      # + 8..10
    verts = np.r_[good, odd]
    nv = len(verts)
    bad = [(n0, n0 + 1, n0 + 2), (0, 0, 1), (5, 5, 5), (-1, 0, 1), (0, nv, 1), (0, 1, 2 ** 31 - 1), (-2 ** 31, 1, 2), (0, n0 + 3, 1), (n0 + 4, 1, 2),
           (0, 1, n0 + 5), (0, n0 + 6, 2), (n0 + 7, 1, 2), (n0 + 8, n0 + 10, 0)]
    ok = [(n0 + 9, n0 + 10, 0), (n0 + 9, 0, n0 + 10)]                              # a vertex exactly on zmax is usable
    tris = np.r_[gt, np.array(bad + ok, np.int64).astype(np.int32)]
    tris = tris[np.random.default_rng(8).permutation(len(tris))]
    raw = frame_for(verts, tris, EYE, w, h, cam, 1000.0, 6, zmax=float(zmax), **M2C)
    nan_pose, inf_pose, one_nan = np.full((4, 4), np.nan, F), np.full((4, 4), np.inf, F), EYE.copy()
    one_nan[0, 3] = np.nan
    zeros = dict.fromkeys(M.RESULT, 0)
    for direction in (M.MODEL_TO_CAMERA, M.SOURCE_ONTO_TARGET):
        ref, _, _ = check(vctx, verts, tris, [nan_pose, EYE, inf_pose, one_nan], raw, 1000.0, cam, ("unusable", direction), render=(0, 1),
                          zmax=float(zmax), pose_direction=direction)
        assert ref[0] == zeros and ref[2] == zeros and ref[3] == zeros
        assert ref[1]["n_projected"] == len(gt) + len(ok) and ref[1]["n_rendered"] > 0
    only_bad = np.array(bad, np.int64).astype(np.int32)
    ref, _, _ = check(vctx, verts, only_bad, [EYE], raw, 1000.0, cam, "nothing usable", zmax=float(zmax), **M2C)
    assert ref == [zeros]
    ref, _, _ = check(vctx, np.zeros((0, 3), F), np.array([[0, 1, 2], [-1, 0, 0]], np.int32), [EYE], raw, 1000.0, cam, "no vertices", **M2C)
    assert ref == [zeros]


# ---------------------------------------------------------------- pose counts, culling, directions
@pytest.mark.parametrize("n_poses", [0, 1, 2, 9, 1025])
def test_pose_counts(vctx, n_poses):
    w, h = 37, 29
    cam = cam_of(w, h)
    sv, st = soup(30, 8, w, h, cam, size=2.5)
    bv, bt = soup(2, 9, w, h, cam, size=14.0)
    verts, tris = np.r_[sv, bv], np.r_[st, bt + len(sv)]
    raw = frame_for(verts, tris, EYE, w, h, cam, 1000.0, 2, **M2C)
    poses = np.stack([nudged(EYE, 50 + i, 0.02) for i in range(n_poses)]) if n_poses else np.zeros((0, 4, 4), F)
    if n_poses >= 2:
        poses[-1] = poses[0]                                                       # the same pose twice
    if n_poses > 9:
        poses[100] = np.nan; poses[200][:3, 3] = (9, 9, 1)                         # poses without a tile inside the list
    ref, order, _ = check(vctx, verts, tris, poses, raw, 1000.0, cam, ("poses", n_poses), render=(0, n_poses - 1), **M2C)
    assert len(ref) == n_poses == len(order)
    if n_poses >= 2:
        assert ref[0] == ref[-1] and list(order).index(0) < list(order).index(n_poses - 1)
    if n_poses > 9:
        assert ref[100] == dict.fromkeys(M.RESULT, 0) and ref[200]["n_rendered"] == 0 < ref[200]["n_projected"]
        assert len({r["n_consistent"] - r["n_violating"] for r in ref}) > 20


def test_cull_modes_and_directions(vctx, synth):
    """The closed object of synth._faces() at a general pose, under model_to_camera and, inverted, under source_onto_target (the default, what
    every registration here returns); with CULL_BACK the faces that look away are gone and the image is the same."""
    w, h = 160, 120
    cam = dict(fx=300.0, fy=295.0, cx=79.5, cy=59.5)
    verts, tris = mesh_cases.faces_object(synth)
    T = synth.make_transform([0.3, 1.0, 0.2], 35.0, (0.02, -0.01, 0.62))           # model -> camera
    raw = frame_for(verts, tris, T, w, h, cam, 1000.0, 1, **M2C)
    a, _, da = check(vctx, verts, tris, [T, nudged(T, 1)], raw, 1000.0, cam, "model_to_camera", render=(0, 1), **M2C)
    c, _, dc = check(vctx, verts, tris, [T, nudged(T, 1)], raw, 1000.0, cam, "model_to_camera, culled", render=(0, 1), cull=M.CULL_BACK, **M2C)
    assert a[0]["n_projected"] == 22 and 0 < c[0]["n_projected"] < 22 and da[0].tobytes() == dc[0].tobytes() and a[0]["n_rendered"] > 2000
    Ti = np.linalg.inv(T.astype(np.float64)).astype(F)
    for cull in (M.CULL_NONE, M.CULL_BACK):
        b, _, _ = check(vctx, verts, tris, [Ti, nudged(Ti, 2)], raw, 1000.0, cam, ("source_onto_target", cull), render=(0, 1), cull=cull)
        assert b[0]["n_consistent"] > 1000
    E = exact_pose((1, 0, 2), (1, -1, 1), (0.25, -0.125, -0.5625))
    check(vctx, verts, tris, [E], raw, 1000.0, cam, "exact", pose_direction=M.SOURCE_ONTO_TARGET)


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
    verts, tris = soup(100, 1, w, h, cam)
    check(vctx, verts, tris, [EYE], frame_for(verts, tris, EYE, w, h, cam, 1000.0, 1, **M2C), 1000.0, cam, "after the refusals", **M2C)
    empty = np.zeros((0, w), np.uint16)                                            # an empty frame is valid: the triangles still count
    res, order = vctx.verify_poses_mesh(verts, tris, [EYE], empty, 1000.0, **cam, **M2C)
    assert res == [dict(dict.fromkeys(M.RESULT, 0), n_projected=100)] and order.tolist() == [0]
    none = np.zeros((0, 3), np.int32)                                              # ... and so is a mesh without triangles
    res, order = vctx.verify_poses_mesh(verts, none, [EYE, EYE], np.full((h, w), 1000, np.uint16), 1000.0, **cam, **M2C)
    assert res == [dict.fromkeys(M.RESULT, 0)] * 2 and order.tolist() == [0, 1]


# ---------------------------------------------------------------- the three kinds of mesh at a realistic pose
@pytest.mark.parametrize("kind", ["box", "faces", "relief"])
def test_meshes_at_a_realistic_pose(vctx, synth, kind):
    """The box (12 faces of thousands of pixels: the queue), the object of synth._faces() (22) and the relief part's height grid at 2 mm
    (4,800 faces of about a pixel: the lanes' own path) in a 300 x 260 frame, against a frame rendered from the mesh itself over a floor:
    at the true pose every rendered pixel is consistent, a pose in free space is seen through."""
    w, h, scale = 300, 260, 1000.0
    cam = dict(fx=420.0, fy=420.0, cx=150.0, cy=130.0)
    if kind == "relief":
        verts, tris = mesh_cases.relief(synth.ReliefPart(seed=3), 0.002)
        true = synth.instance_pose(2, 0.45, 25.0).astype(F)
    else:
        verts, tris = mesh_cases.box() if kind == "box" else mesh_cases.faces_object(synth)
        true = synth.make_transform([1.0, 0.4, 0.1], 140.0, (0.01, 0.0, 0.55)).astype(F)
    depth = M.depth_of(M.render_keys(verts, tris, true, w, h, **cam, **M2C)[0])
    on = depth != 0
    raw = np.rint(np.where(on, depth, F(0.75)).astype(np.float64) * scale).astype(np.uint16)
    free = true.copy()
    free[2, 3] -= 0.2
    ref, order, _ = check(vctx, verts, tris, [free, true, nudged(true, 3, 0.004)], raw, scale, cam, kind, render=(0, 1), tau=0.502 / scale, **M2C)
    assert ref[1]["n_consistent"] == ref[1]["n_rendered"] == int(on.sum()) > 5000 and ref[1]["n_projected"] == len(tris)
    assert ref[0]["n_violating"] == ref[0]["n_rendered"] > 5000 and order[0] == 1 and order[-1] == 0
    check(vctx, verts, tris, [true], raw, scale, cam, (kind, "culled"), cull=M.CULL_BACK, tau=0.502 / scale, **M2C)
