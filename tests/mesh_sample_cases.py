"""Meshes for the mesh sampling's tests and its bench (tests/test_gpu_mesh_sample.py, tests/test_gpu_mesh_sample_state.py,
tools/bench_mesh_sample.py), beside tests/mesh_cases.py: (vertices float32 [n, 3], triangles int32 [m, 3]) from a size and a seed."""
import numpy as np

F = np.float32


def grid_mesh(nt, seed=0, step=0.01):
    """nt small triangles: a jittered grid, two per cell, normals +z (up to the jitter)."""
    cells = (nt + 1) // 2
    nx = max(1, int(np.ceil(np.sqrt(cells))))
    ny = (cells + nx - 1) // nx
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1) * step + rng.uniform(-0.3, 0.3, (X.size, 3)) * step
    j, i = (a.ravel() for a in np.mgrid[0:ny, 0:nx])
    v00, v10, v01, v11 = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i, (j + 1) * (nx + 1) + i + 1
    t = np.stack([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)], 1).reshape(-1, 3)[:nt]
    assert len(t) == nt
    return v.astype(F), t.astype(np.int32)


def binades_mesh(m=300, seed=4):
    """Separate triangles whose areas spread over 30 binades: the small ones fall below 2^-32 of the largest only where they should."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.uniform(-8, 7, m)                                           # edge lengths: areas over 2^-16 .. 2^14
    v = (rng.random((3 * m, 3)) * np.repeat(scale, 3)[:, None]).astype(F)
    return v, np.arange(3 * m, dtype=np.int32).reshape(m, 3)
