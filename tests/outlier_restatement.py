"""A restatement of outlier removal (include/tdv_hip.h: tdv_remove_statistical_outlier, tdv_remove_radius_outlier) in numpy and scipy,
rule by rule as the header states it.  It shares nothing with the device's search structure.

`statistical_brute` is the definition read literally, O(n^2): per query every f32 d2, the (d2 bits, index) order, the first k.
`statistical` takes its candidates from scipy's cKDTree: k nearest in f64 bound the k-th f32 d2 from above, a ball of a slightly larger
radius holds every row that can reach the list, and the f32 expression and the (d2 bits, index) order decide among them.  Rows that are
not clean (NaN, infinite, or so large that d2 could overflow) are done as in the brute variant.  The statistics come twice: summed with
math.fsum (exact), and - under the key "tree" - in the header's own order (rule 4, tests/fixed_tree_restatement.py).  The device is held to
the second byte for byte, and both the device and the second to the first within a bound derived below.
"""
import math

import numpy as np

import cluster_restatement as CR
import fixed_tree_restatement as FT

F = np.float32
NAN = np.float64(np.nan)
RADIUS_SLACK = 1e-5             # as cluster_restatement: far above the few f32 roundings of d2
CLEAN_LIMIT = 1e18              # |coordinate| below it: d2 between two such rows stays finite, and below the d2 to any row beyond


def d2_knn_f32(a, b):
    """dx*dx + (dy*dy + dz*dz) in f32, every step rounded: the kNN lists' tree (tdv_estimate_normals)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = np.asarray(a, F) - np.asarray(b, F)
        return d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def _keys(d2, idx):
    return (np.ascontiguousarray(d2, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def _mean_of_list(d2_sorted):
    """Rule 2 for one list (f32 d2 in list order): sequential f64 sum of correctly rounded square roots over the count."""
    if len(d2_sorted) == 0:
        return NAN
    with np.errstate(over="ignore", invalid="ignore"):
        return np.add.accumulate(np.sqrt(d2_sorted.astype(np.float64)))[-1] / np.float64(len(d2_sorted))


def _mean_brute_row(xyz, i, k):
    d2 = d2_knn_f32(xyz, xyz[i])
    ok = np.nonzero(~np.isnan(d2))[0]
    key = np.sort(_keys(d2[ok], ok))[:k]
    return _mean_of_list((key >> np.uint64(32)).astype(np.uint32).view(F))


def means_brute(xyz, nb_neighbors):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    k = min(nb_neighbors, len(xyz))
    return np.array([_mean_brute_row(xyz, i, k) for i in range(len(xyz))], np.float64).reshape(-1)


def means_tree(xyz, nb_neighbors):
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    k = min(nb_neighbors, n)
    with np.errstate(invalid="ignore"):
        clean = np.isfinite(xyz).all(1) & (np.abs(xyz) < CLEAN_LIMIT).all(1)
    ci = np.nonzero(clean)[0]
    if len(ci) < k:                                          # a clean query's list reaches beyond the clean rows
        return means_brute(xyz, nb_neighbors)
    mean = np.full(n, NAN)
    for i in np.nonzero(~clean)[0]:
        mean[i] = _mean_brute_row(xyz, i, k)
    if len(ci) == 0:
        return mean
    P = xyz[ci].astype(np.float64)
    tree = cKDTree(P)
    _, nn = tree.query(P, k, workers=8)
    nn = nn.reshape(len(ci), k)
    bound = d2_knn_f32(xyz[ci][nn], xyz[ci][:, None, :]).max(1)       # k real rows: the k-th f32 d2 is at most this
    r = np.sqrt(bound.astype(np.float64)) * (1.0 + RADIUS_SLACK) + 1e-300
    balls = tree.query_ball_point(P, r, workers=8)
    lens = np.array([len(b) for b in balls], np.int64)
    q = np.repeat(np.arange(len(ci)), lens)
    t = np.concatenate([np.asarray(b, np.int64) for b in balls]) if len(q) else np.zeros(0, np.int64)
    d2 = d2_knn_f32(xyz[ci[t]], xyz[ci[q]])
    keep = d2 <= bound[q]
    q, key = q[keep], _keys(d2[keep], ci[t[keep]])                       # the tie-break is the ORIGINAL index
    o = np.lexsort((key, q))
    q, key = q[o], key[o]
    start = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=len(ci)))[:-1]])
    assert (np.bincount(q, minlength=len(ci)) >= k).all()
    rows = key[start[:, None] + np.arange(k)[None, :]]                   # the first k of every query
    d2k = (rows >> np.uint64(32)).astype(np.uint32).view(F).reshape(len(ci), k)
    mean[ci] = np.add.accumulate(np.sqrt(d2k.astype(np.float64)), axis=1)[:, -1] / np.float64(k)    # accumulate: sequential
    return mean


def _kept_rows(xyz, rgb, mask):
    index = np.nonzero(mask)[0].astype(np.int32)
    return index, xyz[index], None if rgb is None else np.asarray(rgb, F).reshape(-1, 3)[index]


def _statistics(mean, std_ratio):
    """Rules 3-5 with exact sums."""
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(mean) & (mean > 0)
    nv = int(valid.sum())
    mv = mean[valid]
    cloud_mean = np.float64(math.fsum(mv)) / np.float64(nv) if nv > 0 else NAN
    std_dev = NAN
    if nv > 1:
        dev = mv - cloud_mean
        std_dev = np.sqrt(np.float64(math.fsum(dev * dev)) / np.float64(nv - 1))
    with np.errstate(invalid="ignore"):
        threshold = cloud_mean + np.float64(std_ratio) * std_dev
        mask = valid & (mean < threshold)
    return valid, nv, cloud_mean, std_dev, threshold, mask


def _statistics_tree(mean, std_ratio):
    """Rules 3-5 with rule 4's sums in the header's fixed order: the term of point i is its mean (pass 2: its squared deviation from the
    restated cloud_mean) where it is valid and +0.0 elsewhere; division, square root, product and sum are single f64 operations."""
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(mean) & (mean > 0)
    nv = int(valid.sum())
    safe = np.where(valid, mean, 0.0)
    cloud_mean = FT.tree_sum(safe) / np.float64(nv) if nv > 0 else NAN
    std_dev = NAN
    if nv > 1:
        dev = safe - cloud_mean
        std_dev = np.sqrt(FT.tree_sum(np.where(valid, dev * dev, 0.0)) / np.float64(nv - 1))
    with np.errstate(invalid="ignore"):
        threshold = cloud_mean + np.float64(std_ratio) * std_dev
        mask = valid & (mean < threshold)
    return valid, nv, np.float64(cloud_mean), np.float64(std_dev), np.float64(threshold), mask


def _statistical(xyz, nb_neighbors, std_ratio, rgb, means):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    mean = means(xyz, nb_neighbors) if len(xyz) else np.zeros(0)
    out = []
    for statistics in (_statistics, _statistics_tree):
        valid, nv, cloud_mean, std_dev, threshold, mask = statistics(mean, std_ratio)
        index, rows, cols = _kept_rows(xyz, rgb, mask)
        out.append(dict(n_valid=nv, n_kept=int(mask.sum()), cloud_mean=cloud_mean, std_dev=std_dev, threshold=threshold,
                        mask=mask.astype(np.uint8), mean=mean, index=index, xyz=rows, rgb=cols, valid=valid))
    out[0]["tree"] = out[1]                                  # the exact-sum form, and the header's order under "tree"
    return out[0]


def statistical(xyz, nb_neighbors, std_ratio, rgb=None):
    """dict(n_valid, n_kept, cloud_mean, std_dev, threshold, mask uint8[n], mean float64[n], index int32[n_kept], xyz, rgb, valid) with
    exact sums, and under "tree" the same dict with rule 4's sums in the header's fixed order."""
    return _statistical(xyz, nb_neighbors, std_ratio, rgb, means_tree)


def statistical_brute(xyz, nb_neighbors, std_ratio, rgb=None):
    return _statistical(xyz, nb_neighbors, std_ratio, rgb, means_brute)


def _radius(xyz, nb_points, rgb, full_count, self_nb):
    cap = nb_points + 1
    mask = full_count > nb_points
    index, rows, cols = _kept_rows(xyz, rgb, mask)
    return dict(n_valid=int(self_nb.sum()), n_kept=int(mask.sum()), cloud_mean=0.0, std_dev=0.0, threshold=0.0, mask=mask.astype(np.uint8),
                count=np.minimum(full_count, cap).astype(np.int32), index=index, xyz=rows, rgb=cols)


def radius(xyz, nb_points, radius, rgb=None):
    """dict(n_valid, n_kept, the three doubles 0, mask, count int32[n] saturated at nb_points + 1, index, xyz, rgb): candidates from
    cluster_restatement's tree at an enlarged f64 radius, the f32 test of tdv_cluster_dbscan's rule 1 decides."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return _radius(xyz, nb_points, rgb, np.zeros(0, np.int64), np.zeros(0, bool))
    i, j, _, self_nb = CR.neighbour_pairs(xyz, radius)
    return _radius(xyz, nb_points, rgb, self_nb.astype(np.int64) + np.bincount(i, minlength=n) + np.bincount(j, minlength=n), self_nb)


def radius_brute(xyz, nb_points, radius, rgb=None):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    d2 = CR.d2_f32(xyz[:, None, :], xyz[None, :, :]) if n else np.zeros((0, 0), F)
    nb = d2 <= CR.eps2_f32(radius)
    return _radius(xyz, nb_points, rgb, nb.sum(1).astype(np.int64), np.diagonal(nb).copy() if n else np.zeros(0, bool))


# ---------------------------------------------------------------- the bound on the device's statistics, and the gap condition
U = 2.0 ** -53


def tree_depth(n):
    """Additions on the longest path of the header's fixed tree (rule 4) over n terms: 6 shuffle steps and 2 wave additions in a workgroup,
    ceil(nb / 256) serial additions per thread of the last workgroup (nb = ceil(n / 256) partials), then 6 + 2 again."""
    nb = -(-n // 256)
    return 8 + -(-nb // 256) + 8


def statistics_bounds(ref, n, std_ratio):
    """Absolute bounds (b_mean, b_std, b_thr) on |device - restatement| for cloud_mean, std_dev and threshold, from the tree alone.

    Every term is >= 0, so a tree sum of depth D has relative error below (1 + u)^D - 1 <= (D + 1) u, u = 2^-53; with the division,
    cloud_mean' = c (1 + d), |d| <= E = (D + 8) u (the margin of 7 u covers what follows).  The deviation sum S' runs over
    (m_i - c')^2: as sum (m_i - c) = 0 for the exact c, sum (m_i - c')^2 = S + n_valid c^2 d^2 exactly, and the roundings of each term
    (one subtraction, one square: 3 u) and of the tree (D u) are relative to it.  Hence std_dev' <= sqrt(S (1 + (D + 4) u) / (n_valid - 1))
    + |c| |d| sqrt(n_valid / (n_valid - 1)), i.e. |std_dev' - std_dev| <= E (std_dev + 2 |c|) - the absolute error of the mean enters the
    deviations once, which matters only where the means barely differ.  threshold' = c' + std_ratio * std_dev' adds one product and one
    sum.  With at most two valid points every sum is a single correctly rounded addition (+0.0 terms are exact): the device's doubles
    are then the restatement's bit for bit and the bounds are 0."""
    if ref["n_valid"] <= 2:
        return 0.0, 0.0, 0.0
    E = (tree_depth(n) + 8) * U
    assert E < 1e-12
    c, sd = abs(float(ref["cloud_mean"])), float(ref["std_dev"])
    b_mean = E * c
    b_std = E * (sd + 2 * c)
    b_thr = b_mean + abs(std_ratio) * b_std + 2 * U * (c + abs(std_ratio) * sd)
    return b_mean, b_std, b_thr


def gap_ok(ref, n, std_ratio):
    """The gap condition: no valid mean within the threshold's bound of the restated threshold (so that the strict test of rule 5 cannot
    fall differently on the device).  With a bound of 0 the thresholds are the same bits and there is nothing to exclude."""
    b_thr = statistics_bounds(ref, n, std_ratio)[2]
    if b_thr == 0.0 or not np.isfinite(ref["threshold"]):
        return True
    mv = ref["mean"][ref["valid"]]
    return not (np.abs(mv - ref["threshold"]) <= b_thr).any()
