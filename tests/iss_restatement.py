"""A restatement of ISS keypoints (include/tdv_hip.h: tdv_iss_keypoints) in numpy and scipy, rule by rule as the header states it, op by op
where the header fixes the order.  It shares nothing with the device's search structure: the candidate pairs come from scipy's cKDTree at
a slightly enlarged f64 radius (cluster_restatement.neighbour_pairs) and the header's f32 test decides; the moments are int64 sums
(np.add.reduceat: exact whatever the order); the covariance, the Jacobi schedule and the saliency test are f64 expressions in the stated
order, vectorised over points (numpy neither contracts nor reorders them).  Every output is then fixed bit for bit and the device is held to
it byte for byte.

Rule 8 (the default radii): the kNN list at k = 2 by the library's (d2 bits, index) key, as outlier_restatement builds its lists.  The
resolution comes twice: `resolution_in_tree_order` sums in the header's fixed order (the statistical filter's rule 4,
tests/fixed_tree_restatement.py) and the device is held to its bytes; `resolution` sums with math.fsum (exact), and `resolution_bound`
bounds the fixed tree - the device's and the restated one - against it from the tree's depth alone.
"""
import math

import numpy as np

import cluster_restatement as CR
import fixed_tree_restatement as FT
import outlier_restatement as OR

F = np.float32
SWEEPS = 6                                   # TDV_ISS_JACOBI_SWEEPS
MAX_POINTS = 1 << 22                         # TDV_ISS_MAX_POINTS
DEFAULTS = dict(salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)
FLT_MAX = np.finfo(F).max
U_LO, U_HI = F(-2147483648.0), F(2147483520.0)     # rule 3's saturation: what an int holds


# ---------------------------------------------------------------- rules 1-3: neighbours and integer moments
def r2_f32(r):
    """r * r in f32, FLT_MAX where that overflows; a NaN radius stays NaN (nothing passes)."""
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = F(r) * F(r)
    return FLT_MAX if r2 > FLT_MAX else r2


def shift(r):
    """sh = 20 - E with r = m * 2^E, m in [0.5, 1) (frexp; E = 0 for r = 0)."""
    r = F(r)
    return 20 - int(np.frexp(r)[1]) if np.isfinite(r) else 20


def directed_pairs(xyz, r):
    """(a, b): every ordered pair with d2(a, b) <= r2, self pairs included, sorted by a."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    if len(xyz) == 0 or not np.isfinite(F(r)):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    i, j, _, self_nb = CR.neighbour_pairs(xyz, r)
    s = np.nonzero(self_nb)[0]
    a, b = np.concatenate([i, j, s]).astype(np.int64), np.concatenate([j, i, s]).astype(np.int64)
    o = np.argsort(a, kind="stable")
    return a[o], b[o]


def _group_starts(a):
    """rows that have entries, and where each one's run starts in the sorted a."""
    first = np.concatenate([[True], a[1:] != a[:-1]]) if len(a) else np.zeros(0, bool)
    return a[first], np.nonzero(first)[0]


def moments(xyz, r):
    """support int64[n], S int64[n, 9]: S_x, S_y, S_z, S_xx, S_xy, S_xz, S_yy, S_yz, S_zz of rule 3 (0 where there is no neighbour)."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    a, b = directed_pairs(xyz, r)
    support = np.bincount(a, minlength=n).astype(np.int64)
    S = np.zeros((n, 9), np.int64)
    if len(a):
        d = xyz[b] - xyz[a]                                            # p_j - p_i, one f32 rounding
        with np.errstate(over="ignore", under="ignore"):
            u = np.clip(np.rint(np.ldexp(d, shift(r))), U_LO, U_HI).astype(np.int64)     # rint: round half even
        rows, starts = _group_starts(a)
        cols = [u[:, 0], u[:, 1], u[:, 2], u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2],
                u[:, 2] * u[:, 2]]
        for k, v in enumerate(cols):
            S[rows, k] = np.add.reduceat(v, starts)
    return support, S


# ---------------------------------------------------------------- rules 4-6
def covariance(support, S):
    """Rule 4: the six entries (a00, a01, a02, a11, a12, a22), f64, in the stated order."""
    c = support.astype(np.float64)
    D = S.astype(np.float64)
    pair = {(0, 0): 3, (0, 1): 4, (0, 2): 5, (1, 1): 6, (1, 2): 7, (2, 2): 8}
    with np.errstate(invalid="ignore", divide="ignore"):
        return [(D[:, k] - (D[:, p] * D[:, q]) / c) / c for (p, q), k in pair.items()]


def _rotate(app, aqq, apq, arp, arq):
    """Rule 5, one pair; a pair whose off-diagonal entry is exactly 0 is skipped."""
    with np.errstate(all="ignore"):
        on = apq != 0.0
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        rp, rq = c * arp - s * arq, s * arp + c * arq
    return (np.where(on, app - h, app), np.where(on, aqq + h, aqq), np.where(on, 0.0, apq), np.where(on, rp, arp), np.where(on, rq, arq))


def _order(a, b):
    swap = a < b
    return np.where(swap, b, a), np.where(swap, a, b)


def jacobi_eigenvalues(a00, a01, a02, a11, a12, a22, sweeps=SWEEPS):
    """(l1, l2, l3), l1 >= l2 >= l3: the header's fixed schedule, vectorised; also the off-diagonal left (for the tests)."""
    a00, a01, a02, a11, a12, a22 = (np.array(x, np.float64) for x in (a00, a01, a02, a11, a12, a22))
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)
    l0, l1, l2 = a00, a11, a22
    l0, l1 = _order(l0, l1); l1, l2 = _order(l1, l2); l0, l1 = _order(l0, l1)
    return (l0, l1, l2), np.maximum(np.abs(a01), np.maximum(np.abs(a02), np.abs(a12)))


def saliency(support, S, sh, gamma_21, gamma_32, min_neighbors):
    """eigenvalues float64[n, 3] (reported scale; +0.0 below min_neighbors) and saliency float64[n] of rules 2 and 4-6."""
    n = len(support)
    eig = np.zeros((n, 3), np.float64)
    sal = np.zeros(n, np.float64)
    ok = np.nonzero(support >= min_neighbors)[0]
    if len(ok):
        (l0, l1, l2), _ = jacobi_eigenvalues(*covariance(support[ok], S[ok]))
        l0, l1, l2 = (np.ldexp(x, -2 * sh) for x in (l0, l1, l2))
        eig[ok] = np.stack([l0, l1, l2], 1)
        with np.errstate(all="ignore"):
            salient = (l1 / l0 < np.float64(gamma_21)) & (l2 / l1 < np.float64(gamma_32)) & (l2 > 0.0)
        sal[ok] = np.where(salient, l2, 0.0)
    return eig, sal


# ---------------------------------------------------------------- rule 7
def non_max(xyz, sal, r, min_neighbors):
    n = len(sal)
    a, b = directed_pairs(xyz, r)
    cnt = np.bincount(a, minlength=n)
    best = np.full(n, -np.inf)
    if len(a):
        rows, starts = _group_starts(a)
        best[rows] = np.maximum.reduceat(sal[b], starts)
    return (sal > 0.0) & (cnt >= min_neighbors) & ~(best > sal)


# ---------------------------------------------------------------- rule 8
def _nn_of_keys(key):
    return np.sqrt(np.float64((key[1] >> np.uint64(32)).astype(np.uint32).view(F))) if len(key) >= 2 else OR.NAN


def _nn_brute_row(xyz, i):
    d2 = OR.d2_knn_f32(xyz, xyz[i])
    ok = np.nonzero(~np.isnan(d2))[0]
    with np.errstate(invalid="ignore"):
        return _nn_of_keys(np.sort(OR._keys(d2[ok], ok))[:2])


def nearest_brute(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.array([_nn_brute_row(xyz, i) for i in range(len(xyz))], np.float64).reshape(-1)


def nearest(xyz):
    """nn float64[n]: sqrt((double)d2) of entry 1 of the kNN list at k = 2 (NaN where the list is shorter); candidates from cKDTree as
    outlier_restatement.means_tree takes them, the f32 d2 and the (d2 bits, index) order decide."""
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    with np.errstate(invalid="ignore"):
        clean = np.isfinite(xyz).all(1) & (np.abs(xyz) < OR.CLEAN_LIMIT).all(1)
    ci = np.nonzero(clean)[0]
    if len(ci) < 2:
        return nearest_brute(xyz)
    nn = np.full(n, OR.NAN)
    for i in np.nonzero(~clean)[0]:
        nn[i] = _nn_brute_row(xyz, i)
    P = xyz[ci].astype(np.float64)
    tree = cKDTree(P)
    _, near = tree.query(P, 2, workers=8)
    bound = OR.d2_knn_f32(xyz[ci][near], xyz[ci][:, None, :]).max(1)            # two real rows: the second f32 d2 is at most this
    r = np.sqrt(bound.astype(np.float64)) * (1.0 + OR.RADIUS_SLACK) + 1e-300
    balls = tree.query_ball_point(P, r, workers=8)
    lens = np.array([len(b) for b in balls], np.int64)
    q = np.repeat(np.arange(len(ci)), lens)
    t = np.concatenate([np.asarray(b, np.int64) for b in balls])
    d2 = OR.d2_knn_f32(xyz[ci[t]], xyz[ci[q]])
    keep = d2 <= bound[q]
    q, key = q[keep], OR._keys(d2[keep], ci[t[keep]])                          # the tie-break is the ORIGINAL index
    o = np.lexsort((key, q))
    q, key = q[o], key[o]
    count = np.bincount(q, minlength=len(ci))
    assert (count >= 2).all()
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    second = (key[start + 1] >> np.uint64(32)).astype(np.uint32).view(F)
    nn[ci] = np.sqrt(second.astype(np.float64))
    return nn


def resolution(xyz, nn_of=nearest):
    """(resolution with the exact sum, n_valid, nn): rule 8 with math.fsum in the tree's place."""
    nn = nn_of(xyz) if len(np.asarray(xyz).reshape(-1, 3)) else np.zeros(0)
    valid = np.isfinite(nn)
    nv = int(valid.sum())
    return (np.float64(math.fsum(nn[valid])) / np.float64(nv) if nv else OR.NAN), nv, nn


def resolution_in_tree_order(xyz, nn_of=nearest):
    """(resolution, n_valid, nn): rule 8 as the header states it - the term of point i is nn_i where it is valid and +0.0 elsewhere, summed
    in the fixed f64 tree of the statistical filter's rule 4, then one division."""
    nn = nn_of(xyz) if len(np.asarray(xyz).reshape(-1, 3)) else np.zeros(0)
    valid = np.isfinite(nn)
    nv = int(valid.sum())
    return (np.float64(FT.tree_sum(np.where(valid, nn, 0.0)) / np.float64(nv)) if nv else OR.NAN), nv, nn


def default_radii(res):
    with np.errstate(invalid="ignore"):
        return F(np.float64(6.0) * np.float64(res)), F(np.float64(4.0) * np.float64(res))


def resolution_bound(res, n):
    """Absolute bound on |device - exact-sum resolution| from the header's fixed tree alone: every term is >= 0, so a tree sum of depth D
    (outlier_restatement.tree_depth) has relative error below (1 + u)^D - 1 <= (D + 1) u, u = 2^-53; the device's division adds one
    rounding, and the exact-sum value carries two of its own (the rounded fsum, its division): (D + 4) u in all.  The margin of
    outlier_restatement.statistics_bounds, (D + 8) u, is kept.  Nothing here is measured on a device."""
    if not np.isfinite(res):
        return 0.0
    return (OR.tree_depth(n) + 8) * OR.U * abs(float(res))


# ---------------------------------------------------------------- the whole call
def iss(xyz, attr=None, nn_of=nearest, **params):
    """dict(n_finite, n_supported, n_salient, n_keypoints, salient_radius, non_max_radius, resolution (exact sum; NaN when the radii were
    given), mask uint8[n], saliency float64[n], eigenvalues float64[n, 3], support int32[n], index int32[m], xyz float32[m, 3], attr)."""
    p = dict(DEFAULTS, **params)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    rs, rn, res = F(p["salient_radius"]), F(p["non_max_radius"]), OR.NAN
    if rs == 0 and rn == 0:
        res = resolution(xyz, nn_of)[0]
        rs, rn = default_radii(res)
    support, S = moments(xyz, rs)
    eig, sal = saliency(support, S, shift(rs), p["gamma_21"], p["gamma_32"], p["min_neighbors"])
    key = non_max(xyz, sal, rn, p["min_neighbors"]) if n else np.zeros(0, bool)
    index = np.nonzero(key)[0].astype(np.int32)
    return dict(n_finite=int((support >= 1).sum()), n_supported=int((support >= p["min_neighbors"]).sum()), n_salient=int((sal > 0).sum()),
                n_keypoints=len(index), salient_radius=rs, non_max_radius=rn, resolution=res, mask=key.astype(np.uint8), saliency=sal,
                eigenvalues=eig, support=support.astype(np.int32), index=index, xyz=xyz[index],
                attr=None if attr is None else np.asarray(attr, F).reshape(n, -1)[index])


COUNTS = ("n_finite", "n_supported", "n_salient", "n_keypoints")
ARRAYS = ("mask", "support", "saliency", "eigenvalues", "index", "xyz", "attr")
