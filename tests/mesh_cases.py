"""Triangle meshes for the mesh verification's tests and its bench (tests/test_verify_mesh_abi.py, tests/test_gpu_verify_mesh.py,
tools/bench_verify_mesh.py): (vertices float32 [n, 3], triangles int32 [m, 3]).  Every face is wound so that (b - a) x (c - a) points out of
the solid (for the relief: up, +z, the side its scan sees), which is what TDV_MESH_CULL_BACK takes for the front."""
import numpy as np

F = np.float32


def _quad(o, eu, ev, normal):
    """The rectangle o, o + eu, o + eu + ev, o + ev as two triangles whose normal is `normal`'s side."""
    o, eu, ev = (np.asarray(a, np.float64) for a in (o, eu, ev))
    v = [o, o + eu, o + eu + ev, o + ev]
    t = [(0, 1, 2), (0, 2, 3)] if np.dot(np.cross(eu, ev), normal) > 0 else [(0, 2, 1), (0, 3, 2)]
    return v, t


def from_rectangles(rects):
    """(origin, edge_u, edge_v, outward normal) rectangles -> a mesh of two triangles each; corners shared between rectangles are merged,
    so neighbouring faces share their edge's vertices."""
    verts, index, tris = [], {}, []
    for o, eu, ev, n in rects:
        v, t = _quad(o, eu, ev, n)
        ids = []
        for p in v:
            key = tuple(np.round(p, 9))
            if key not in index:
                index[key] = len(verts)
                verts.append(p)
            ids.append(index[key])
        tris += [tuple(ids[k] for k in tri) for tri in t]
    return np.array(verts, F), np.array(tris, np.int32)


def box(size=(0.2, 0.12, 0.06), centre=(0.0, 0.0, 0.0)):
    """A box of 8 vertices and 12 triangles: faces of thousands of pixels at a bin-picking camera."""
    s, c = np.asarray(size, np.float64), np.asarray(centre, np.float64)
    o = c - s / 2
    ex, ey, ez = np.diag(s)
    rects = [(o, ex, ey, (0, 0, -1)), (o + ez, ex, ey, (0, 0, 1)), (o, ex, ez, (0, -1, 0)), (o + ey, ex, ez, (0, 1, 0)),
             (o, ey, ez, (-1, 0, 0)), (o + ex, ey, ez, (1, 0, 0))]
    v, t = from_rectangles(rects)
    assert len(v) == 8 and len(t) == 12
    return v, t


def faces_object(synth):
    """The rectangles of synth._faces() (a box with a boss on its top: 11 rectangles) as 22 triangles."""
    v, t = from_rectangles(synth._faces())
    assert len(t) == 22
    return v, t


def relief(part, step, keep=None, transform=None):
    """part.height_grid(step) triangulated, two triangles per cell, normals up (+z): many small faces.  keep(x, y) -> bool per vertex: only
    cells with all four corners kept (a disc part); transform: a 4 x 4 applied to the vertices (part frame -> the model's frame)."""
    xs, ys, Z = part.height_grid(step)
    nx, ny = len(xs), len(ys)
    X, Y = np.meshgrid(xs, ys)
    v = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    j, i = (a.ravel() for a in np.mgrid[0:ny - 1, 0:nx - 1])
    v00, v10, v01, v11 = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
    t = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)])
    if keep is not None:
        ok = keep(v[:, 0], v[:, 1])
        t = t[ok[t].all(1)]
        used = np.unique(t)
        remap = np.full(len(v), -1, np.int64)
        remap[used] = np.arange(len(used))
        v, t = v[used], remap[t]
    if transform is not None:
        M = np.asarray(transform, np.float64)
        v = v @ M[:3, :3].T + M[:3, 3]
    return v.astype(F), t.astype(np.int32)
