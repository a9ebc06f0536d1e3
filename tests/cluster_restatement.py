"""A restatement of Euclidean clustering (include/tdv_hip.h: tdv_cluster_dbscan) in numpy and scipy, rule by rule as the header states it.

It shares nothing with the device's search structure.  `cluster` takes its candidate pairs from scipy's cKDTree at a slightly enlarged
f64 radius, applies the header's f32 test to them, takes the components of the core points from scipy.sparse.csgraph and applies the
numbering, border and size rules.  `cluster_brute` is the definition read literally for small clouds: the dense n x n matrix of f32
distances, components by an ascending scan that grows each cluster to its end (Open3D's loop), the border rule by an arg-min over each
row.  Every output is an integer (or a row of the input): the device is held to them byte for byte.
"""
import numpy as np

F = np.float32
DEFAULTS = dict(min_cluster_size=1)
# The f32 d2 differs from the exact distance by a few roundings (each difference, three squares, two sums: below 4 * 2^-24 relative
# on d2); the tree's radius is enlarged by far more than that, and the f32 test decides.
RADIUS_SLACK = 1e-5


def d2_f32(a, b):
    """(dx*dx + dy*dy) + dz*dz in f32, every step rounded (numpy's f32 arithmetic does not contract)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = np.asarray(a, F) - np.asarray(b, F)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def eps2_f32(eps):
    with np.errstate(over="ignore"):
        return min(F(eps) * F(eps), np.finfo(F).max)        # finite: an infinite d2 never passes


def neighbour_pairs(xyz, eps):
    """(i, j, d2) of every pair i < j with d2 <= eps2, and the rows that neighbour themselves (d2(i, i) = 0 <= eps2: the finite rows)."""
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    self_nb = d2_f32(xyz, xyz) <= eps2_f32(eps)
    idx = np.nonzero(np.isfinite(xyz).all(1))[0]
    if len(idx) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F), self_nb
    tree = cKDTree(xyz[idx].astype(np.float64))
    r = float(F(eps)) * (1.0 + RADIUS_SLACK) + 1e-300
    pairs = tree.query_pairs(r, output_type="ndarray")
    i, j = idx[pairs[:, 0]], idx[pairs[:, 1]]
    i, j = np.minimum(i, j), np.maximum(i, j)
    d2 = d2_f32(xyz[i], xyz[j])
    ok = d2 <= eps2_f32(eps)
    return i[ok], j[ok], d2[ok], self_nb


def _finish(xyz, core, root_of_core, border_from, min_cluster_size):
    """Rules 5-8 from: the core flags, the lowest core index of every core point's component, the core neighbour each non-core point
    joins (-1: none)."""
    n = len(xyz)
    roots = np.unique(root_of_core[core])                     # ascending lowest core index: the numbering
    cid = np.full(n, -1, np.int64)
    cid[roots] = np.arange(len(roots))
    raw = np.full(n, -1, np.int64)
    raw[core] = cid[root_of_core[core]]
    is_border = ~core & (border_from >= 0)
    raw[is_border] = cid[root_of_core[border_from[is_border]]]
    size = np.bincount(raw[raw >= 0], minlength=len(roots))
    keep = size >= min_cluster_size
    newid = np.cumsum(keep) - 1
    labels = np.full(n, -1, np.int32)
    if len(roots):
        labels = np.where((raw >= 0) & keep[np.maximum(raw, 0)], newid[np.maximum(raw, 0)], -1).astype(np.int32)
    kept = size[keep]
    n_clusters = int(keep.sum())
    order = np.lexsort((np.arange(n), np.where(labels < 0, n_clusters, labels))).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.int32)
    result = dict(n_clusters=n_clusters, n_core=int(core.sum()), n_border=int(is_border.sum()), n_noise=int((labels < 0).sum()),
                  n_dropped=int(len(roots) - n_clusters), largest=int(kept.max()) if n_clusters else 0, n_labelled=int(kept.sum()))
    return dict(result=result, labels=labels, order=order, offsets=offsets, grouped=xyz[order], core=core, border=is_border)


def cluster(xyz, eps, min_points, min_cluster_size=1):
    """dict(result, labels int32[n], order int32[n], offsets int32[n_clusters + 1], grouped float32[n, 3], core, border)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return _finish(xyz, np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, np.int64), min_cluster_size)
    i, j, d2, self_nb = neighbour_pairs(xyz, eps)
    count = self_nb.astype(np.int64) + np.bincount(i, minlength=n) + np.bincount(j, minlength=n)
    core = count >= min_points
    cc = core[i] & core[j]
    g = coo_matrix((np.ones(int(cc.sum()), np.int8), (i[cc], j[cc])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    low = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(low, comp[core], np.nonzero(core)[0])
    root_of_core = np.where(core, low[comp], -1)
    # border: for every non-core end of a pair whose other end is core, the smallest (d2 bits, index of the core end)
    bits = d2.view(np.uint32).astype(np.uint64) << np.uint64(32)
    p = np.concatenate([i[~core[i] & core[j]], j[~core[j] & core[i]]])
    q = np.concatenate([j[~core[i] & core[j]], i[~core[j] & core[i]]])
    key = np.concatenate([bits[~core[i] & core[j]], bits[~core[j] & core[i]]]) | q.astype(np.uint64)
    border_from = np.full(n, -1, np.int64)
    if len(p):
        o = np.lexsort((key, p))
        first = np.concatenate([[True], p[o][1:] != p[o][:-1]])
        border_from[p[o][first]] = q[o][first]
    return _finish(xyz, core, root_of_core, border_from, min_cluster_size)


def cluster_brute(xyz, eps, min_points, min_cluster_size=1):
    """The same outputs from the dense matrix, O(n^2): for small clouds."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    d2 = d2_f32(xyz[:, None, :], xyz[None, :, :]) if n else np.zeros((0, 0), F)
    nb = d2 <= eps2_f32(eps)
    core = nb.sum(1) >= min_points
    root_of_core = np.full(n, -1, np.int64)
    for s in range(n):                                        # ascending scan: s is the lowest core index of the cluster it opens
        if not core[s] or root_of_core[s] >= 0:
            continue
        root_of_core[s] = s
        stack = [s]
        while stack:
            a = stack.pop()
            for b in np.nonzero(nb[a] & core & (root_of_core < 0))[0]:
                root_of_core[b] = s
                stack.append(int(b))
    border_from = np.full(n, -1, np.int64)
    for a in np.nonzero(~core)[0]:
        cand = np.nonzero(nb[a] & core)[0]
        if len(cand):
            key = (d2[a, cand].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64)
            border_from[a] = cand[int(np.argmin(key))]
    return _finish(xyz, core, root_of_core, border_from, min_cluster_size)


# ---------------------------------------------------------------- the scene of the tests and of tools/bench_cluster.py
FLOOR_Z = 0.8
SCENE = dict(n_floor=30000, n_parts=6, n_part=4000, n_stray=60, noise=0.0005, gap=0.004, pitch=(0.30, 0.60))


def scene(synth, seed=5, stray_value=None):
    """A bin floor seen from above (camera frame, z forward): 30,000 points over +-0.5 x +-0.35 m at z = 0.8; six
    synth.sample_object(4000, 100 + b) parts, each turned about z by a random angle, on a grid of 0.30 m x 0.60 m pitch with the part's
    far side 4 mm above the floor; 60 stray points above the floor; 0.5 mm Gaussian noise; rows permuted.  Returns (points float32,
    part int: b for part b, -1 floor, -2 stray).  stray_value (NaN, inf): the stray rows are poisoned with it instead, in turn the
    whole row or one coordinate, with alternating sign."""
    S = SCENE
    rng = np.random.default_rng(seed)
    floor = np.c_[rng.uniform(-0.5, 0.5, S["n_floor"]), rng.uniform(-0.35, 0.35, S["n_floor"]), np.full(S["n_floor"], FLOOR_Z)]
    rows, part = [floor], [np.full(S["n_floor"], -1)]
    for b in range(S["n_parts"]):
        p = synth.sample_object(S["n_part"], 100 + b)[0].astype(np.float64)
        a = rng.uniform(0, 2 * np.pi)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        p = (p - p.mean(0)) @ Rz.T
        p += [(b % 3 - 1) * S["pitch"][0], (b // 3 - 0.5) * S["pitch"][1], 0]
        p[:, 2] += FLOOR_Z - S["gap"] - p[:, 2].max()
        rows.append(p); part.append(np.full(len(p), b))
    stray = np.c_[rng.uniform(-0.5, 0.5, S["n_stray"]), rng.uniform(-0.35, 0.35, S["n_stray"]), rng.uniform(FLOOR_Z - 0.3, FLOOR_Z - 0.15, S["n_stray"])]
    rows.append(stray); part.append(np.full(S["n_stray"], -2))
    pts = np.concatenate(rows)
    pts = pts + rng.normal(0, S["noise"], pts.shape)
    part = np.concatenate(part)
    if stray_value is not None:
        for k, r in enumerate(np.nonzero(part == -2)[0]):
            v = stray_value if k % 2 == 0 else -stray_value
            if k % 4 == 3:
                pts[r] = v
            else:
                pts[r, k % 4] = v
    perm = rng.permutation(len(pts))
    return pts[perm].astype(F), part[perm]


PLANE = dict(max_planes=1, distance_threshold=0.002, num_iterations=500)
PARAMS = [(0.010, 10), (0.012, 10), (0.008, 5)]
