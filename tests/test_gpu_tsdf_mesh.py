"""The mesh of a fused volume on the device (include/tdv_hip.h: tdv_tsdf_extract_mesh_dev, csrc/tsdf.hip) against the restatement
(tests/tsdf_mesh_restatement.py), byte for byte: n_vertices, n_triangles, the vertices, the normals and the triangles.  Volume sides stand
where a cell's vertices sit in the next run of 64 voxels along x and in the next LDS tile along y and z, and on sides of 1 and 2; seeded
volumes bring all 256 cases with their ambiguous faces, unobserved voxels, exact zeros and negative zeros.  Then: the vertices are
tdv_tsdf_extract_dev's rows, the output forms (no normals, a query, each capacity one short), the host form and compact=True, the device
mesh's pointers into the mesh renderer and the mesh sampler, and every bad argument on a live context.  Scenes are tsdf_cases.small_scene's,
frames of 96 x 72."""
import numpy as np
import pytest
import torch

import mesh_sample_restatement as MS
import tsdf_mesh_restatement as M
import tsdf_restatement as R
import verify_mesh_restatement as VM
from state_cases import Env
from test_gpu_tsdf import scene
from test_tsdf_abi import TDV_ERR_BAD_ARG
from test_tsdf_mesh_abi import MESH_BAD, MESH_NULLS, MeshOutputs, mesh_call, random_signs, seeded

pytestmark = pytest.mark.gpu
F = np.float32
TX, TY, TZ = R.TILE
PATTERN = 0xA5A5A5A5


def restated(s, start=None, **params):
    """The restatement's mesh of the scene's frames fused in one call (or of the volume `start`)."""
    vol = s["vol"]
    buf = start
    if buf is None:
        buf, _ = R.integrate(vol, R.reset(vol), s["frames"], s["poses"], s["intr"], **params)
    xyz, nrm, _, tri = M.mesh(vol, buf, params.get("min_weight", 1.0))
    return dict(volume=buf, nv=len(xyz), nt=len(tri), xyz=xyz, normals=nrm, triangles=tri)


def device_volume(tdv, ctx, env, s, start=None, **params):
    """(the volume struct, the device tensor of the fused volume)."""
    vol = s["vol"]
    cvol = tdv.tsdf_volume_struct(*vol.args())
    if start is not None:
        env.up(start)
        return cvol, env.keep[-1]
    d_vol = env.out(vol.voxels * 2, F)
    ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
    h, w = s["frames"].shape[1:]
    ctx.tsdf_integrate_dev(cvol, d_vol.data_ptr(), env.up(s["frames"]), s["poses"], w, h, *s["intr"], want_counts=False, **params)
    return cvol, d_vol


def device(tdv, ctx, env, s, start=None, normals=True, **params):
    cvol, d_vol = device_volume(tdv, ctx, env, s, start, **params)
    nv, nt, fits = ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), None, None, 0, None, 0, **params)      # the query
    assert fits == (nv == 0) and (nt == 0 or nv > 0)
    ox, on, ot = env.out(3 * nv, F), env.out(3 * nv, F), env.out(3 * nt, np.int32)
    got = ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), ox.data_ptr(), on.data_ptr() if normals else None, nv, ot.data_ptr(), nt, **params)
    assert got == (nv, nt, True)                                                   # each capacity exact
    return dict(nv=nv, nt=nt, xyz=env.get(ox, 3 * nv, F).reshape(-1, 3), normals=env.get(on, 3 * nv, F).reshape(-1, 3) if normals else None,
                triangles=env.get(ot, 3 * nt, np.int32).reshape(-1, 3), cvol=cvol, d_vol=d_vol, buffers=(ox, on, ot))


def same(ref, got, what):
    assert (got["nv"], got["nt"]) == (ref["nv"], ref["nt"]), (what, got["nv"], got["nt"], ref["nv"], ref["nt"])
    for k in ("xyz", "normals", "triangles"):
        if got[k] is None:
            continue
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].dtype, ref[k].dtype)
        if got[k].tobytes() != ref[k].tobytes():
            bad = np.argwhere(got[k].view(np.uint32) != ref[k].view(np.uint32))
            first = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: %r, restated %r" % (what, k, len(bad), first, got[k][first], ref[k][first]))


def held(tdv, ctx, s, what, env=None, start=None, normals=True, **params):
    ref = restated(s, start, **params)
    got = device(tdv, ctx, env or Env(ctx), s, start, normals, **params)
    same(ref, got, what)
    return ref, got


# ---------------------------------------------------------------- sides, runs and tiles
SIDES = [(2, 2, 2), (1, 33, 17), (33, 1, 17), (33, 17, 1), (63, 9, 7), (64, 8, 8), (65, 9, 9), (66, 9, 9), (129, 9, 5), (33, TY - 1, 17),
         (33, TY, TZ + 1), (33, TY + 1, TZ), (17, 33, TZ - 1), (65, 33, 17)]


@pytest.mark.parametrize("dims", SIDES, ids=["%dx%dx%d" % d for d in SIDES])
def test_sides_runs_and_tiles(tdv, ctx, dims):
    ref, _ = held(tdv, ctx, scene(dims), dims)
    if min(dims) == 1:
        assert ref["nv"] > 20 and ref["nt"] == 0                                   # vertices, no cell
    elif dims != (2, 2, 2):
        assert ref["nv"] > 20 and ref["nt"] > 20, (ref["nv"], ref["nt"])
    if dims == (129, 9, 5):                                                        # some cell's vertices sit in the next run along x
        _, cell = M.triangle_keys(scene(dims)["vol"], ref["volume"])
        assert ((cell % dims[0]) % TX == TX - 1).any()


def test_one_cell(tdv, ctx):
    """(2, 2, 2): the one cell in a few cases - a corner cut off, a plane, an ambiguous face, every face ambiguous, five triangles - and
    their complements; with one corner unobserved there are crossings and no triangle."""
    s = dict(scene((2, 2, 2), 0))
    count = []
    for case in (0x00, 0x01, 0x0F, 0x09, 0x69, 0x1E, 0x3D, 0xFF):
        for c in (case, case ^ 0xFF):
            f = np.where((c >> np.arange(8)) & 1, -0.25, 0.5).astype(F)
            vol, start = seeded((2, 2, 2), f)
            ref, _ = held(tdv, ctx, dict(s, vol=vol), hex(c), start=start)
            assert ref["nt"] == M.TABLE[c, 0]
            count.append(ref["nt"])
            w = np.ones(8, F); w[6] = 0
            ref, _ = held(tdv, ctx, dict(s, vol=vol), (hex(c), "corner 6 unobserved"), start=seeded((2, 2, 2), f, w)[1])
            assert ref["nt"] == 0
    assert max(count) == 5 and min(count) == 0


# ---------------------------------------------------------------- seeded volumes
def test_all_cases_fully_observed(tdv, ctx):
    vol, start = random_signs()
    ref, _ = held(tdv, ctx, dict(scene((2, 2, 2), 0), vol=vol), "random signs", start=start)
    assert (np.bincount(M.cells(vol, start)[1], minlength=256) > 0).all() and ref["nt"] > 20000
    assert np.isfinite(ref["xyz"]).all() and np.isfinite(ref["normals"]).all()


def test_unobserved_voxels(tdv, ctx):
    vol, start = random_signs(0.85)
    ref, _ = held(tdv, ctx, dict(scene((2, 2, 2), 0), vol=vol), "random signs, 15 % unobserved", start=start)
    assert 2000 < ref["nt"] and len(np.unique(ref["triangles"])) < ref["nv"]       # crossings no triangle uses stay in the vertex array


def test_zeros_and_negative_zeros(tdv, ctx):
    """tsdf from {-0.5, -0.0, 0.0, 0.25, 1.0, -1.0}: zero and negative zero count as non-negative, and a triangle whose three crossings
    coincide at a corner of value 0 is emitted like any other.  One voxel in ten unobserved; then min_weight 2 over weights of 1 and 3."""
    rng = np.random.default_rng(11)
    dims = (TX + 3, TY + 2, TZ + 1)
    f = rng.choice(np.array([-0.5, -0.0, 0.0, 0.25, 1.0, -1.0], F), dims[::-1])
    w = rng.choice(np.array([0, 1, 3], F), dims[::-1], p=[0.1, 0.45, 0.45])
    vol, start = seeded(dims, f, w)
    s = dict(scene((2, 2, 2), 0), vol=vol)
    ref, _ = held(tdv, ctx, s, "zeros", start=start)
    flat = (M.face_vectors(ref["xyz"], ref["triangles"]) == 0).all(1)
    assert ref["nt"] > 2000 and flat.sum() > 20 and np.isfinite(ref["xyz"]).all() and np.isfinite(ref["normals"]).all()
    two, _ = held(tdv, ctx, s, "zeros, min_weight 2", start=start, min_weight=2.0)
    assert 0 < two["nt"] < ref["nt"]


# ---------------------------------------------------------------- identity with the cloud, output forms
def test_vertices_are_the_clouds_rows_and_output_forms(tdv, ctx):
    s = scene((65, 33, 17), 2)
    env = Env(ctx)
    ref, got = held(tdv, ctx, s, "65x33x17", env)
    nv, nt, cvol, d_vol = ref["nv"], ref["nt"], got["cvol"], got["d_vol"]
    assert nv > 500 and nt > 500
    # identity: tdv_tsdf_extract_dev on the same volume
    ox, on = env.out(3 * nv, F), env.out(3 * nv, F)
    assert ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), ox.data_ptr(), on.data_ptr(), nv) == (nv, True)
    assert env.get(ox, 3 * nv, F).tobytes() == got["xyz"].tobytes() and env.get(on, 3 * nv, F).tobytes() == got["normals"].tobytes()
    # no normals
    plain = device(tdv, ctx, env, s, normals=False)
    same(ref, plain, "no normals")
    assert (env.get(plain["buffers"][1], 3 * nv, np.uint32) == PATTERN).all()
    # a capacity one short, or zero: both counts, nothing written
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (nv - 1, nt - 1), (0, nt), (nv, 0)):
        bx, bn, bt = env.out(3 * nv, F), env.out(3 * nv, F), env.out(3 * nt, np.int32)
        assert ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), bx.data_ptr(), bn.data_ptr(), vcap, bt.data_ptr(), tcap) == (nv, nt, False)
        for b, n in ((bx, 3 * nv), (bn, 3 * nv), (bt, 3 * nt)):
            assert (env.get(b, n, np.uint32) == PATTERN).all(), (vcap, tcap)
    # room to spare: nothing beyond the rows
    bx, bn, bt = env.out(3 * (nv + 2), F), env.out(3 * (nv + 2), F), env.out(3 * (nt + 2), np.int32)
    assert ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), bx.data_ptr(), bn.data_ptr(), nv + 2, bt.data_ptr(), nt + 2) == (nv, nt, True)
    for b, n, want in ((bx, 3 * nv, ref["xyz"]), (bn, 3 * nv, ref["normals"]), (bt, 3 * nt, ref["triangles"])):
        a = env.get(b, n + 6, np.uint32)
        assert a[:n].tobytes() == want.tobytes() and (a[n:] == PATTERN).all()
    assert env.get(d_vol, s["vol"].voxels * 2, F).tobytes() == ref["volume"].astype(F).tobytes()        # extraction reads only


def test_host_form_and_compact(tdv, ctx):
    s = scene((65, 33, 17), 3)
    ref = restated(s, max_weight=2.0)
    xyz, nrm, tri = ctx.tsdf_fuse_mesh(s["frames"], s["poses"], s["intr"], s["vol"].args(), max_weight=2.0)
    assert tri.dtype == np.int32 and tri.shape == (ref["nt"], 3)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes() and tri.tobytes() == ref["triangles"].tobytes()
    xyz, nrm, tri = ctx.tsdf_fuse_mesh(s["frames"], s["poses"], s["intr"], s["vol"].args(), normals=False, max_weight=2.0)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm is None and tri.tobytes() == ref["triangles"].tobytes()
    empty = ctx.tsdf_fuse_mesh(s["frames"][:0], s["poses"][:0], s["intr"], s["vol"].args())
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0, 3) and empty[2].dtype == np.int32
    # compact=True against the numpy compaction of the ABI's result
    cx, cn, ct = M.compact(ref["xyz"], ref["normals"], ref["triangles"])
    assert cx[ct].tobytes() == ref["xyz"][ref["triangles"]].tobytes()
    gx, gn, gt = ctx.tsdf_fuse_mesh(s["frames"], s["poses"], s["intr"], s["vol"].args(), compact=True, max_weight=2.0)
    assert gx.tobytes() == cx.tobytes() and gn.tobytes() == cn.tobytes() and gt.tobytes() == ct.tobytes() and gt.dtype == np.int32
    volume = ctx.tsdf_volume(*s["vol"].args())
    ctx.tsdf_integrate(volume, s["frames"], s["poses"], s["intr"], max_weight=2.0)
    xyz, nrm, tri = ctx.tsdf_extract_mesh(volume)
    assert xyz.tobytes() == ref["xyz"].tobytes() and nrm.tobytes() == ref["normals"].tobytes() and tri.tobytes() == ref["triangles"].tobytes()
    gx, gn, gt = ctx.tsdf_extract_mesh(volume, normals=False, compact=True)
    assert gx.tobytes() == cx.tobytes() and gn is None and gt.tobytes() == ct.tobytes()
    # ... and where it drops something: the seeded volume with unobserved voxels, whose rim crossings are in no triangle
    vol, start = random_signs(0.85)
    volume = (tdv.tsdf_volume_struct(*vol.args()), torch.from_numpy(start.reshape(-1, 2).copy()).to(volume[1].device))
    torch.cuda.synchronize()
    xyz, nrm, tri = ctx.tsdf_extract_mesh(volume)
    cx, cn, ct = M.compact(xyz, nrm, tri)
    assert 0 < len(cx) < len(xyz) and (np.diff(np.unique(ct)) == 1).all() and ct.max() == len(cx) - 1
    gx, gn, gt = ctx.tsdf_extract_mesh(volume, compact=True)
    assert gx.tobytes() == cx.tobytes() and gn.tobytes() == cn.tobytes() and gt.tobytes() == ct.tobytes() and gt.dtype == np.int32
    assert gx[gt].tobytes() == xyz[tri].tobytes()


# ---------------------------------------------------------------- downstream
def test_device_mesh_into_the_renderer_and_the_sampler(tdv, ctx):
    """The device mesh's pointers as they are into tdv_render_depth_mesh_dev (back faces culled, at the first frame's pose) and
    tdv_mesh_sample_points_dev; the results equal those entry points' restatements run on the restated mesh."""
    s = scene((65, 33, 17), 3)
    env = Env(ctx)
    ref, got = held(tdv, ctx, s, "65x33x17", env)
    ox, _, ot = got["buffers"]
    h, w = s["frames"].shape[1:]
    _, fx, fy, cx, cy = s["intr"]
    depth = env.out(w * h, F)
    n = ctx.render_depth_mesh_dev(ox.data_ptr(), ref["nv"], ot.data_ptr(), ref["nt"], s["poses"][0], w, h, fx, fy, cx, cy, depth.data_ptr(),
                                  pose_direction="model_to_camera", cull="back")
    keys, _ = VM.render_keys(ref["xyz"], ref["triangles"], s["poses"][0], w, h, fx, fy, cx, cy, VM.MODEL_TO_CAMERA, VM.CULL_BACK)
    want = VM.depth_of(keys)
    assert n == (keys != VM.EMPTY).sum() > 500 and env.get(depth, w * h, F).tobytes() == want.tobytes()
    k = 1000
    sx, sn = env.out(3 * k, F), env.out(3 * k, F)
    res = ctx.mesh_sample_dev(ox.data_ptr(), ref["nv"], ot.data_ptr(), ref["nt"], k, seed=5, d_out_xyz=sx.data_ptr(), d_out_normals=sn.data_ptr())
    want = MS.sample(ref["xyz"], ref["triangles"], k, seed=5)
    assert res["n_sampled"] == k and res["n_usable"] > 500
    for f in MS.RESULT + ("surface_area",):
        assert (np.float32(res[f]).tobytes() == np.float32(want[f]).tobytes()) if f == "area_max" else (res[f] == want[f]), f
    assert env.get(sx, 3 * k, F).tobytes() == want["xyz"].tobytes() and env.get(sn, 3 * k, F).tobytes() == want["normals"].tobytes()
    near = ref["normals"][ref["triangles"][want["triangle"], 0]].astype(np.float64)
    assert ((want["normals"].astype(np.float64) * near).sum(1) > 0).all()            # the sampler's outward normal is T8's side


# ---------------------------------------------------------------- arguments
def live_buffers(env):
    """Device buffers for mesh_call on a live context, 0xA5 throughout: env.keep[-4:] are the volume, the points, the normals, the triangles."""
    d_vol, d_xyz, d_nrm, d_tri = env.out(4 * 3 * 2 * 2, F), env.out(8 * 3, F), env.out(8 * 3, F), env.out(8 * 3, np.int32)
    return dict(volume=d_vol.data_ptr(), xyz=d_xyz.data_ptr(), normals=d_nrm.data_ptr(), triangles=d_tri.data_ptr())


def test_bad_arguments_on_a_live_context(tdv, ctx):
    env = Env(ctx)
    buffers = live_buffers(env)
    o = MeshOutputs()
    for what, kw, where in MESH_BAD[1:]:
        for which in where:
            assert mesh_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == TDV_ERR_BAD_ARG, (what, which)
    for what, where in MESH_NULLS.items():
        for which in where:
            assert mesh_call(tdv, which, ctx._h, o, null=(what,), buffers=buffers) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()
    for t in env.keep[-4:]:
        assert (env.get(t, t.numel(), np.uint8) == 0xA5).all()
    # and the same calls with nothing wrong go through: a reset volume has no crossing, the host form may find some
    ctx.tsdf_reset_dev(tdv.tsdf_volume_struct((0.0, 0.0, 0.3), 0.001, (4, 3, 2)), buffers["volume"])
    assert mesh_call(tdv, "extract_mesh", ctx._h, o, buffers=buffers) == 0 and (o.n_out[0], o.n_triangles[0]) == (0, 0)
    assert mesh_call(tdv, "fuse_mesh", ctx._h, o, capacity=0, triangle_capacity=0, null=("out_xyz", "out_triangles")) in (0, TDV_ERR_BAD_ARG)
    assert o.n_out[0] >= 0 and o.n_triangles[0] >= 0
