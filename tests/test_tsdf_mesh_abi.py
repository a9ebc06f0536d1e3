"""CPU suite: the mesh of a fused volume (include/tdv_hip.h: tdv_tsdf_extract_mesh_dev, rules T9 to T12).  The ABI exports the two entry
points and the constant and refuses every bad argument before it writes anything (tests/test_tsdf_abi.py's table and pattern, by import).
The committed case table equals what the generator (tools/gen_tsdf_mc_table.py) makes from rule T11, has the counts the rule's statement
lists, and is watertight case by case.  Then the restatement (tests/tsdf_mesh_restatement.py) is held to what the rules promise: a closed
sphere that faces outwards, random signs with every one of the 256 cases and no edge drawn twice, unobserved voxels, a plane, the relief
scene and min_weight.  No compute entry point of the library runs here; tests/test_gpu_tsdf_mesh.py holds the device to the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import tsdf_mesh_restatement as M
import tsdf_restatement as R
from test_tsdf_abi import BAD, GOOD, NULLS, PLANE_VOL, TDV_ERR_BAD_ARG, U, Outputs, P, plane, relief  # noqa: F401 (relief: a fixture)

F = np.float32
G = M.G
SYMBOLS = ("tdv_tsdf_extract_mesh_dev", "tdv_tsdf_fuse_mesh")
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- ABI
def test_symbols_constant_and_rules(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    header = open(os.path.join(HERE, "..", "include", "tdv_hip.h")).read()
    text = header.split("#define TDV_TSDF_MC_MAX_TRIANGLES ")[1].split("/*")[0].split("\n")[0].strip()
    assert eval(text) == tdv.TDV_TSDF_MC_MAX_TRIANGLES == M.MAX_TRIANGLES == 5
    for rule in ("T9.", "T10.", "T11.", "T12."):
        assert " %s " % rule in header, rule
    tsdf_block = header.split("/* TSDF fusion")[1].split("*/")[0]
    assert "Not provided" in tsdf_block and "mesh extraction" not in tsdf_block.split("Not provided")[1]


MESH_GOOD = dict(GOOD, triangle_capacity=8)
WHICH = {"extract": "extract_mesh", "fuse": "fuse_mesh"}
MESH_BAD = [(what, kw, tuple(WHICH[w] for w in where if w in WHICH)) for what, kw, where in BAD if any(w in WHICH for w in where)]
MESH_BAD += [("triangle_capacity -1", dict(triangle_capacity=-1), tuple(WHICH.values())),
             ("both capacities -1", dict(capacity=-1, triangle_capacity=-1), tuple(WHICH.values()))]
MESH_NULLS = {what: tuple(WHICH[w] for w in where if w in WHICH) for what, where in NULLS.items() if any(w in WHICH for w in where)}
MESH_NULLS.update(n_triangles=tuple(WHICH.values()), out_triangles=tuple(WHICH.values()))


class MeshOutputs(Outputs):
    """test_tsdf_abi.Outputs with the triangle rows and their count."""

    def __init__(self):
        self.triangles = np.full((8, 3), -7, np.int32); self.n_triangles = np.full(1, -7, np.int32)
        Outputs.__init__(self)

    def arrays(self):
        return Outputs.arrays(self) + (self.triangles, self.n_triangles)


def mesh_call(tdv, which, ctx, o, null=(), buffers=None, **kw):
    """tdv_tsdf_extract_mesh_dev or tdv_tsdf_fuse_mesh on MESH_GOOD's arguments with kw replaced and the pointers named in `null` NULL;
    buffers (the GPU suite): device pointers for volume, xyz, normals and triangles in place of the host arrays."""
    g = dict(MESH_GOOD, **kw)
    lib = tdv.lib()
    b = buffers or {}
    vol = tdv.TsdfVolumeC((C.c_float * 3)(0.0, 0.0, 0.3), g["voxel_length"], g["nx"], g["ny"], g["nz"])
    prm = tdv.TsdfParamsC(g["trunc"], g["max_weight"], g["zmax"], g["min_weight"], g["pose_direction"])
    raw = np.full((R.MAX_FRAMES + 1) * 8 * 6, 3000, np.uint16)
    poses = np.tile(np.eye(4, dtype=F).reshape(-1), R.MAX_FRAMES + 1)
    pv = None if "vol" in null else C.byref(vol)
    pp = None if "params" in null else C.byref(prm)
    n_out = None if "n_out" in null else P(o.n_out)
    n_tri = None if "n_triangles" in null else P(o.n_triangles)
    if which == "extract_mesh":
        volume = None if "volume" in null else P(b.get("volume", o.volume))
        xyz = None if "out_xyz" in null else P(b.get("xyz", o.xyz))
        tri = None if "out_triangles" in null else P(b.get("triangles", o.triangles))
        return lib.tdv_tsdf_extract_mesh_dev(ctx, pv, volume, pp, xyz, P(b.get("normals", o.normals)), g["capacity"], n_out, tri,
                                             g["triangle_capacity"], n_tri)
    assert which == "fuse_mesh"
    cam = (g["width"], g["height"], C.c_float(g["scale"]), C.c_float(g["fx"]), C.c_float(g["fy"]), C.c_float(3.5), C.c_float(2.5))
    return lib.tdv_tsdf_fuse_mesh(ctx, pv, None if "frames" in null else P(raw), g["n_frames"], *cam, None if "poses" in null else P(poses), pp,
                                  None if "out_xyz" in null else P(o.xyz), P(o.normals), g["capacity"], n_out,
                                  None if "out_triangles" in null else P(o.triangles), g["triangle_capacity"], n_tri)


@pytest.mark.parametrize("case", range(len(MESH_BAD)), ids=[b[0] for b in MESH_BAD])
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  On a live context:
    tests/test_gpu_tsdf_mesh.py."""
    o = MeshOutputs()
    what, kw, where = MESH_BAD[case]
    assert where
    for which in where:
        assert mesh_call(tdv, which, None, o, **kw) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


def test_null_pointers(tdv):
    o = MeshOutputs()
    assert set(MESH_NULLS) == {"vol", "volume", "params", "frames", "poses", "n_out", "out_xyz", "n_triangles", "out_triangles"}
    for what, where in MESH_NULLS.items():
        for which in where:
            assert mesh_call(tdv, which, None, o, null=(what,)) == TDV_ERR_BAD_ARG, (what, which)
    assert o.untouched()


# ---------------------------------------------------------------- the table
def test_committed_table_equals_the_generator():
    text = open(G.HEADER).read()
    assert G.parse_header(text) == G.packed()
    assert text == G.header_text()


def test_table_counts():
    s = G.stats()
    assert s["triangles"] == 820 and s["most"] == 5 == M.MAX_TRIANGLES
    assert s["histogram"] == [2, 16, 50, 80, 76, 32]
    assert s["rotated"] == [9, 9]                                                  # 18 loops need the rotation: 9 by one place, 9 by two
    assert M.TABLE.shape == (256, 16) and (M.TABLE[:, 0] <= 5).all()
    for case in range(256):
        n = M.TABLE[case, 0]
        assert (M.TABLE[case, 1:1 + 3 * n] < 12).all() and (M.TABLE[case, 1 + 3 * n:] == G.FILL).all()


@pytest.mark.parametrize("case", range(256))
def test_table_case_is_watertight(case):
    """Every crossing edge is used; each face segment occurs once as a directed triangle side; every other side (an inner diagonal)
    occurs once in each direction; no diagonal lies in a face of the cube."""
    tris = G.table()[case]
    crossing = {e for e in range(12) if G.crossing(case, e)}
    assert {e for t in tris for e in t} == crossing
    sides = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(sides)) == len(sides)
    segs = [frozenset(s) for s in G.segments(case)]
    assert len(set(segs)) == len(segs)
    for s in segs:
        a, b = tuple(s)
        assert ((a, b) in sides) + ((b, a) in sides) == 1, s
    for a, b in sides:
        if frozenset((a, b)) in segs:
            continue
        assert (b, a) in sides and not G.on_common_face(a, b), (a, b)


# ---------------------------------------------------------------- the restatement against what the rules promise
def seeded(dims, f, w=None):
    vol = R.Volume((0.01, -0.02, 0.3), 0.0015, dims)
    f = np.asarray(f, F).reshape(dims[::-1])
    w = np.ones(dims[::-1], F) if w is None else np.asarray(w, F).reshape(dims[::-1])
    return vol, np.stack([f, w], -1)


def key_voxel(vol, key):
    """(i, j, k, axis) of T7 keys."""
    v = key // 3
    return v % vol.nx, (v // vol.nx) % vol.ny, v // (vol.nx * vol.ny), key % 3


def on_rim(vol, key):
    """The crossing's voxel edge lies in a boundary face of the volume."""
    i, j, k, ax = key_voxel(vol, key)
    out = np.zeros(len(key), bool)
    for d, (c, n) in enumerate(((i, vol.nx), (j, vol.ny), (k, vol.nz))):
        out |= (ax != d) & ((c == 0) | (c == n - 1))
    return out


def test_sphere_is_closed_and_faces_outwards():
    n = 20
    centre = np.array([10.2, 9.9, 10.1])
    z, y, x = np.meshgrid(*([np.arange(n) + 0.5] * 3), indexing="ij")
    f = (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - 6.5) / 8.0        # in voxels, negative inside
    vol, buf = seeded((n, n, n), f)
    xyz, nrm, key, tri = M.mesh(vol, buf)
    once, open_edges = M.unmatched_edges(tri, len(xyz))
    assert once and len(open_edges) == 0
    assert len(tri) > 1000 and np.array_equal(np.unique(tri), np.arange(len(xyz)))  # all observed: every crossing is a vertex of some triangle
    assert len(xyz) - 3 * len(tri) // 2 + len(tri) == 2                            # V - E + F
    c = vol.origin.astype(np.float64) + centre * float(vol.L)
    mid = xyz.astype(np.float64)[tri].mean(1)
    fv = M.face_vectors(xyz, tri)
    assert ((fv * (mid - c)).sum(1) > 0).all()
    assert ((fv * nrm.astype(np.float64)[tri[:, 0]]).sum(1) > 0).all()             # T8's side


RANDOM_DIMS = (65, 17, 9)


def random_signs(observed=1.0):
    rng = np.random.default_rng(7)
    f = rng.standard_normal(RANDOM_DIMS[::-1])
    w = (rng.random(RANDOM_DIMS[::-1]) < observed).astype(F)
    return seeded(RANDOM_DIMS, f, w)


def test_random_signs_fully_observed():
    vol, buf = random_signs()
    cell, case = M.cells(vol, buf)
    assert len(cell) == 64 * 16 * 8
    hist = np.bincount(case, minlength=256)
    print("random signs: the rarest case occurs %d times" % hist.min())
    assert hist.min() == 19                                                        # all 256 cases, the ambiguous faces among them
    xyz, _, key, tri = M.mesh(vol, buf)
    once, open_edges = M.unmatched_edges(tri, len(xyz))
    assert once and len(open_edges) > 0
    assert on_rim(vol, key[open_edges[:, 0]]).all() and on_rim(vol, key[open_edges[:, 1]]).all()
    assert len(tri) == M.TABLE[case, 0].sum() > 20000


def usable_cells(vol, buf, min_weight=1.0):
    """bool [nz-1, ny-1, nx-1], by T9 and nothing else."""
    obs = buf[..., 1] >= F(min_weight)
    u = np.ones((vol.nz - 1, vol.ny - 1, vol.nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                u &= obs[dz:vol.nz - 1 + dz, dy:vol.ny - 1 + dy, dx:vol.nx - 1 + dx]
    return u


def test_random_signs_partly_observed():
    vol, buf = random_signs(0.85)
    assert 0.1 < (buf[..., 1] == 0).mean() < 0.2
    usable = usable_cells(vol, buf)
    xyz, _, key, tri = M.mesh(vol, buf)
    tk, cell = M.triangle_keys(vol, buf)
    assert len(tri) == len(tk) > 2000 and np.array_equal(key[tri], tk)
    ci, cj, ck = cell % vol.nx, (cell // vol.nx) % vol.ny, cell // (vol.nx * vol.ny)
    assert usable[ck, cj, ci].all() and (np.diff(cell) >= 0).all()
    # every corner of a triangle is an edge of the triangle's cell
    i, j, k, ax = key_voxel(vol, tk)
    d = np.stack([i - ci[:, None], j - cj[:, None], k - ck[:, None]], -1)
    assert ((d >= 0) & (d <= 1)).all() and (np.take_along_axis(d, ax[..., None], -1)[..., 0] == 0).all()
    # an unmatched side lies in a face of its cell beyond which there is no usable cell
    once, open_edges = M.unmatched_edges(tri, len(xyz))
    assert once and len(open_edges) > 100
    sides = M.directed_edges(tri)
    side_cell = np.tile(cell, 3)
    lookup = {(a, b): c for (a, b), c in zip(map(tuple, sides), side_cell)}
    dims = np.array(vol.dims)
    for a, b in open_edges:
        c = lookup[(a, b)]
        cc = np.array([c % vol.nx, (c // vol.nx) % vol.ny, c // (vol.nx * vol.ny)])
        ends = []
        for kk in (key[a], key[b]):                                               # both ends of both voxel edges, relative to the cell
            v = np.array([(kk // 3) % vol.nx, (kk // 3 // vol.nx) % vol.ny, kk // 3 // (vol.nx * vol.ny)]) - cc
            far = v.copy(); far[kk % 3] += 1
            ends += [v, far]
        ends = np.array(ends)
        border = False
        for axis in range(3):
            for side in (0, 1):
                if (ends[:, axis] == side).all():                                  # the side lies in this face of the cell
                    nb = cc.copy(); nb[axis] += 1 if side else -1
                    border |= bool((nb < 0).any() or (nb > dims - 2).any() or not usable[nb[2], nb[1], nb[0]])
        assert border, (a, b, cc)


def test_plane():
    """test_tsdf_abi's front-on plane: the layer of cells between z layers 4 and 5 is cut into two triangles per cell, all facing the
    camera.  Every crossing has the same z bit for bit (one expression on equal inputs), so the face vectors are exactly along z.  The two
    triangles of a cell tile its rectangle, so the total area is (x_last - x_first)(y_last - y_first) of the f32 centres.  A centre
    origin + (i + 0.5) L carries two roundings, of the product and of the sum: it is within e = 2 u (|origin| + n L) of its exact value,
    so each extent is within 2 e of (n - 1) L and the area within 2 e_x Y + 2 e_y X + 4 e_x e_y of X Y, X = (nx - 1) L, Y = (ny - 1) L with
    L the f32 voxel length; the f64 sums add a relative 1e-12 at most."""
    vol = PLANE_VOL
    buf, _ = plane()
    xyz, nrm, key, tri = M.mesh(vol, buf)
    ncell = (vol.nx - 1) * (vol.ny - 1)
    assert len(tri) == 2 * ncell
    tk, cell = M.triangle_keys(vol, buf)
    layer = ((4 * vol.ny + np.arange(vol.ny - 1)[:, None]) * vol.nx + np.arange(vol.nx - 1)[None, :]).reshape(-1)
    assert np.array_equal(cell, np.repeat(layer, 2))                               # two triangles per cell of the layer
    fv = M.face_vectors(xyz, tri)
    area = np.linalg.norm(fv, axis=1) / 2
    assert (area > 0).all() and np.array_equal(fv / (2 * area[:, None]), np.tile([0.0, 0.0, -1.0], (len(tri), 1)))
    L = float(vol.L)
    X, Y = (vol.nx - 1) * L, (vol.ny - 1) * L
    ex, ey = (2 * U * (abs(float(vol.origin[d])) + n * L) for d, n in ((0, vol.nx), (1, vol.ny)))
    bound = 2 * ex * Y + 2 * ey * X + 4 * ex * ey + 1e-12 * X * Y
    print("plane: area %.9e, (nx-1)(ny-1)L^2 = %.9e, difference %.3e (bound %.3e)" % (area.sum(), X * Y, abs(area.sum() - X * Y), bound))
    assert abs(area.sum() - X * Y) <= bound < 1e-5 * X * Y


def test_relief_scene_faces_agree_with_vertex_normals(relief):
    vol = relief["vol"]
    xyz, nrm, key, tri = M.mesh(vol, relief["buf"])
    fv = M.face_vectors(xyz, tri)
    flat = (fv == 0).all(1)
    dots = (fv[:, None, :] * nrm.astype(np.float64)[tri]).sum(-1)
    print("relief: %d vertices, %d triangles (%d of zero area), %d vertices unreferenced; smallest cosine %.3f" % (
        len(xyz), len(tri), flat.sum(), len(xyz) - len(np.unique(tri)),
        (dots[~flat] / np.linalg.norm(fv[~flat], axis=1)[:, None]).min()))
    assert len(tri) > 20000 and flat.sum() < len(tri) // 100
    assert (dots[~flat] > 0).all()
    once, _ = M.unmatched_edges(tri, len(xyz))
    assert once


def test_min_weight(relief):
    """min_weight = 2 keeps exactly the triangles of cells whose eight corners were seen twice."""
    vol, buf = relief["vol"], relief["buf"]
    tk1, cell1 = M.triangle_keys(vol, buf, 1.0)
    tk2, cell2 = M.triangle_keys(vol, buf, 2.0)
    twice = usable_cells(vol, buf, 2.0)
    keep = twice[cell1 // (vol.nx * vol.ny), (cell1 // vol.nx) % vol.ny, cell1 % vol.nx]
    assert 0 < keep.sum() < len(cell1)
    assert np.array_equal(cell2, cell1[keep]) and np.array_equal(tk2, tk1[keep])
    xyz1, _, key1, tri1 = M.mesh(vol, buf, 1.0)
    xyz2, _, key2, tri2 = M.mesh(vol, buf, 2.0)
    assert xyz2[tri2].tobytes() == xyz1[tri1[keep]].tobytes()
