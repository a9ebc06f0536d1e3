"""The mesh of a fused volume as include/tdv_hip.h (tdv_tsdf_extract_mesh_dev) states it, rules T9 to T12, in numpy: the vertices, normals
and keys are tsdf_restatement.extract's own, the triangles are int32 rows over them.  The case table is built by the generator
(tools/gen_tsdf_mc_table.py) from rule T11, not read from the committed header.  Vectorised over the cells; it knows nothing of tiles or
runs.  tests/test_tsdf_mesh_abi.py holds it to what the rules promise; tests/test_gpu_tsdf_mesh.py holds the device to it byte for byte."""
import os
import sys

import numpy as np

import tsdf_restatement as R

_TOOLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import gen_tsdf_mc_table as G  # noqa: E402

F = R.F
MAX_TRIANGLES = G.MAX_TRIANGLES
TABLE = np.frombuffer(G.packed(), np.uint8).reshape(256, 16)                       # count, 15 edge numbers
EDGE_AXIS = np.array([e >> 2 for e in range(12)], np.int64)
EDGE_OWNER = np.array([G.edge_owner(e) for e in range(12)], np.int64)              # (dx, dy, dz)
CORNER = np.array([G.corner(q) for q in range(8)], np.int64)


def cells(vol, buf, min_weight=1.0):
    """T9: (the voxel index of every usable cell's corner 0, ascending; its case)."""
    f, wt = buf[..., 0], buf[..., 1]
    if min(vol.dims) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    obs = wt >= F(min_weight)
    neg = f < 0
    usable = np.ones((vol.nz - 1, vol.ny - 1, vol.nx - 1), bool)
    case = np.zeros(usable.shape, np.int64)
    for q, (dx, dy, dz) in enumerate(CORNER):
        sl = (slice(dz, vol.nz - 1 + dz), slice(dy, vol.ny - 1 + dy), slice(dx, vol.nx - 1 + dx))
        usable &= obs[sl]
        case |= neg[sl].astype(np.int64) << q
    k, j, i = np.nonzero(usable)
    return (k * vol.ny + j) * vol.nx + i, case[usable]


def triangle_keys(vol, buf, min_weight=1.0):
    """T10 to T12: (int64[m, 3] the T7 key of every triangle corner, int64[m] the cell of every triangle), rows in T12's order."""
    cell, case = cells(vol, buf, min_weight)
    count = TABLE[case, 0].astype(np.int64)
    rep = np.repeat(np.arange(len(cell)), count)
    t = np.arange(len(rep)) - np.repeat(np.cumsum(count) - count, count)           # the triangle's number within its cell
    e = TABLE[case[rep][:, None], 1 + 3 * t[:, None] + np.arange(3)[None, :]].astype(np.int64)
    assert (e < 12).all()
    own = EDGE_OWNER[e]
    voxel = cell[rep][:, None] + own[..., 0] + own[..., 1] * vol.nx + own[..., 2] * vol.nx * vol.ny
    return 3 * voxel + EDGE_AXIS[e], cell[rep]


def mesh(vol, buf, min_weight=1.0, **_):
    """(xyz f32[n, 3], normals f32[n, 3], key int64[n], triangles int32[m, 3])."""
    xyz, nrm, key = R.extract(vol, buf, min_weight)
    tk, _ = triangle_keys(vol, buf, min_weight)
    tri = np.searchsorted(key, tk)
    assert tk.size == 0 or (tri < len(key)).all() and (key[tri] == tk).all(), "a crossing edge of a usable cell that is none of T7's"
    return xyz, nrm, key, tri.astype(np.int32).reshape(-1, 3)


def compact(xyz, nrm, tri):
    """The vertices some triangle refers to, in their order, and the triangles renumbered."""
    used = np.zeros(len(xyz), bool)
    used[tri.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return xyz[used], (None if nrm is None else nrm[used]), new[tri].astype(np.int32).reshape(-1, 3)


def fuse_mesh(vol, frames, poses, intrinsics, **params):
    buf, _ = R.integrate(vol, R.reset(vol), frames, poses, intrinsics, **params)
    xyz, nrm, _, tri = mesh(vol, buf, params.get("min_weight", 1.0))
    return xyz, nrm, tri


# ---------------------------------------------------------------- what a mesh is made of (for the tests)
def directed_edges(tri):
    """int64[3m, 2]: (from, to) of every triangle side."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def unmatched_edges(tri, n):
    """(no directed edge occurs twice, the directed edges whose reverse is missing)."""
    d = directed_edges(tri)
    code = d[:, 0] * n + d[:, 1]
    once = len(np.unique(code)) == len(code)
    return once, d[~np.isin(d[:, 1] * n + d[:, 0], code)]


def face_vectors(xyz, tri):
    """(vb - va) x (vc - va) in f64."""
    p = xyz.astype(np.float64)[np.asarray(tri, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
