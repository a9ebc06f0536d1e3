"""A restatement of Fast Global Registration (include/tdv_hip.h: tdv_fgr) in numpy, step by step as the header states it.

It implements the header's definition, not the kernels: Philox4x32-10, the mutual filter, the tuple test (trial order, the device's chunk
schedule for trials_run), the normalisation, the Geman-McClure Gauss-Newton loop with the graduated mu schedule, the f64 LDL^T step, the
Rz Ry Rx update, the return to the original scale and the score of tdv_ransac's winner.  The descriptor matches come from the caller:
pyoracle.feature_match in both directions at test sizes, or the device's tdv_feature_match_dev outputs at large sizes (those are held to
the oracle elsewhere).  The discrete sets (mutual pairs, tuple pairs, counts) are exact; the pose agrees with the device's to the last
places of f64 sin / cos and sum order, not to the bit.
"""
import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
CHUNK = 1 << 17            # TDV_FGR_TRIAL_CHUNK: trials of the first chunk; each later chunk doubles, up to CHUNK << 5
CHUNK_MAX_SHIFT = 5

DEFAULTS = dict(division_factor=1.4, maximum_correspondence_distance=0.025, tuple_scale=0.95, iteration_number=64,
                maximum_tuple_count=1000, use_absolute_scale=0, decrease_mu=1, tuple_test=1, seed=42)


def philox4x32(ctr, key):
    """Philox4x32-10 (Salmon et al., Random123).  ctr: (4, n) or 4 ints; key: 2 ints.  Returns (4, n) uint32-valued uint64 words."""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & M32 for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        p0 = PHILOX_M[0] * c[0]
        p1 = PHILOX_M[1] * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        if r < 9:
            k0 = (k0 + PHILOX_W[0]) & 0xFFFFFFFF
            k1 = (k1 + PHILOX_W[1]) & 0xFFFFFFFF
    return np.stack(c)


def trial_indices(t, n_mutual, seed):
    """Indices (3, len(t)) into the mutual list of trials t (uint64): words x0..x2 of Philox(counter (lo32 t, hi32 t, 0, 0), key
    (seed, 0)), index (x * n_mutual) >> 32."""
    t = np.asarray(t, np.uint64)
    z = np.zeros_like(t)
    x = philox4x32((t & M32, t >> np.uint64(32), z, z), (seed, 0))
    return (x[:3] * np.uint64(n_mutual)) >> np.uint64(32)


def mutual(cst, cts):
    """(k, 2) int64 pairs (i, cst[i]) with cts[cst[i]] == i, ascending i."""
    cst = np.asarray(cst, np.int64); cts = np.asarray(cts, np.int64)
    i = np.nonzero(cts[cst] == np.arange(len(cst)))[0]
    return np.stack([i, cst[i]], 1)


def _edges(x, a, b, c):
    """|x_a - x_b|, |x_b - x_c|, |x_c - x_a| per trial: component differences in f64 from f32, (dx*dx + dy*dy) + dz*dz, sqrt."""
    x = np.asarray(x, F).astype(np.float64)

    def n(u, v):
        d = x[u] - x[v]
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return n(a, b), n(b, c), n(c, a)


def chunk_bounds(total):
    """The device's chunks over trials [0, total): chunk k holds CHUNK << min(k, CHUNK_MAX_SHIFT) trials."""
    start, k = 0, 0
    while start < total:
        size = CHUNK << min(k, CHUNK_MAX_SHIFT)
        yield start, min(start + size, total)
        start += size; k += 1


def tuple_test(src, tgt, pairs, scale, max_count, seed):
    """(tuple pairs (3 m, 2), trials_run): the pairs of the first max_count passing trials, three per trial, and the trials evaluated
    (whole chunks, up to the chunk in which the count was reached, at most 100 n_mutual)."""
    n = len(pairs)
    total = 100 * n
    s = np.float64(F(scale))
    kept = []; run = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for lo, hi in chunk_bounds(total):
            t = np.arange(lo, hi, dtype=np.uint64)
            idx = trial_indices(t, n, seed).astype(np.int64)
            P = pairs[idx]                                    # (3, m, 2)
            la = _edges(src, P[0, :, 0], P[1, :, 0], P[2, :, 0])
            lb = _edges(tgt, P[0, :, 1], P[1, :, 1], P[2, :, 1])
            ok = np.ones(len(t), bool)
            for a, b in zip(la, lb):
                ok &= (a * s < b) & (b < a / s)
            for m in np.nonzero(ok)[0]:
                if len(kept) < max_count:
                    kept.append(P[:, m, :])
            run = hi
            if len(kept) >= max_count:
                break
    out = np.concatenate(kept, 0) if kept else np.zeros((0, 2), np.int64)
    return out, run


def correspondences(src, tgt, cst, cts, params=None):
    """dict(mutual, tuples, n_mutual, n_tuple, trials_run, corr): corr is the pair list the optimisation uses."""
    p = dict(DEFAULTS, **(params or {}))
    mu = mutual(cst, cts)
    if p["tuple_test"] and len(mu):
        tup, run = tuple_test(src, tgt, mu, p["tuple_scale"], p["maximum_tuple_count"], p["seed"])
    else:
        tup, run = np.zeros((0, 2), np.int64), 0
    corr = tup if p["tuple_test"] else mu
    return dict(mutual=mu, tuples=tup, n_mutual=len(mu), n_tuple=len(tup), trials_run=run, corr=corr)


def normalisation(src, tgt, use_absolute_scale):
    """(mu_s, mu_t, sigma, mu0): f64 means of all points of each cloud; scale = the largest |x - mu| over both clouds (a NaN never
    wins; 0 when no value is > 0); sigma = scale and mu0 = 1, or with use_absolute_scale sigma = 1 and mu0 = scale (Open3D's
    scale_global and scale_start)."""
    xs = np.asarray(src, F).astype(np.float64); xt = np.asarray(tgt, F).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mu_s = xs.sum(0) / len(xs); mu_t = xt.sum(0) / len(xt)
        ds = xs - mu_s; dt = xt - mu_t
        r = np.r_[np.sqrt((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2]),
                  np.sqrt((dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]) + dt[:, 2] * dt[:, 2])]
    r = r[~np.isnan(r)]
    scale = float(r.max()) if len(r) and r.max() > 0 else 0.0
    return (mu_s, mu_t, 1.0, scale) if use_absolute_scale else (mu_s, mu_t, scale, 1.0)


def ldlt6(A, b):
    """x with A x = b by unpivoted LDL^T in the header's order; None when a pivot is not > 0 or not finite."""
    L = np.zeros((6, 6)); d = np.zeros(6)
    for j in range(6):
        for i in range(j, 6):
            s = A[i, j]
            for k in range(j):
                s = s - (L[i, k] * d[k]) * L[j, k]
            if i == j:
                if not (s > 0.0 and np.isfinite(s)):
                    return None
                d[j] = s
            else:
                L[i, j] = s / d[j]
    y = np.zeros(6)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s
    x = np.zeros(6)
    for i in range(5, -1, -1):
        s = y[i] / d[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * x[k]
        x[i] = s
    return x


def rz_ry_rx(x0, x1, x2):
    c0, s0, c1, s1, c2, s2 = np.cos(x0), np.sin(x0), np.cos(x1), np.sin(x1), np.cos(x2), np.sin(x2)
    return np.array([[c2 * c1, (c2 * s1) * s0 - s2 * c0, (c2 * s1) * c0 + s2 * s0],
                     [s2 * c1, (s2 * s1) * s0 + c2 * c0, (s2 * s1) * c0 - c2 * s0],
                     [-s1, c1 * s0, c1 * c0]])


def optimise(src, tgt, corr, params=None, norm=None):
    """(T (4x4 f64, target onto source in normalised units), mu_s, mu_t, sigma) after iteration_number iterations."""
    p = dict(DEFAULTS, **(params or {}))
    mu_s, mu_t, sigma, mu0 = norm if norm is not None else normalisation(src, tgt, p["use_absolute_scale"])
    xs = np.asarray(src, F).astype(np.float64); xt = np.asarray(tgt, F).astype(np.float64)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    T = np.eye(4)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        P = (xs[corr[:, 0]] - mu_s) / sigma
        Q = (xt[corr[:, 1]] - mu_t) / sigma
        mu = float(mu0)
        div = np.float64(F(p["division_factor"])); mcd = np.float64(F(p["maximum_correspondence_distance"]))
        for itr in range(p["iteration_number"]):
            if p["decrease_mu"] and itr % 4 == 0 and mu > mcd:
                mu = mu / div
            q = [((T[a, 0] * Q[:, 0] + T[a, 1] * Q[:, 1]) + T[a, 2] * Q[:, 2]) + T[a, 3] for a in range(3)]
            r = [P[:, a] - q[a] for a in range(3)]
            rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
            w = mu / (rr + mu); w = w * w
            zero = np.zeros(len(P)); one = np.ones(len(P))
            rows = [((zero, -q[2], q[1], -one, zero, zero), r[0]),
                    ((q[2], zero, -q[0], zero, -one, zero), r[1]),
                    ((-q[1], q[0], zero, zero, zero, -one), r[2])]
            JtJ = np.zeros((6, 6)); Jtr = np.zeros(6)
            for a in range(6):
                for b in range(a, 6):
                    v = (w * (rows[0][0][a] * rows[0][0][b]) + w * (rows[1][0][a] * rows[1][0][b])) + w * (rows[2][0][a] * rows[2][0][b])
                    JtJ[a, b] = JtJ[b, a] = v.sum()
                Jtr[a] = ((w * (rows[0][0][a] * rows[0][1]) + w * (rows[1][0][a] * rows[1][1])) + w * (rows[2][0][a] * rows[2][1])).sum()
            y = ldlt6(JtJ, Jtr)
            x = np.zeros(6) if y is None else -y
            D = np.eye(4); D[:3, :3] = rz_ry_rx(x[0], x[1], x[2]); D[:3, 3] = x[3:]
            T = D @ T
    return T, mu_s, mu_t, sigma


def original_scale(T, mu_s, mu_t, sigma):
    """The source-to-target pose in f32: R' = R^T, t' = -R^T (mu_s + sigma t - R mu_t)."""
    R = T[:3, :3]; t = T[:3, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (mu_s + sigma * t) - R @ mu_t
        out = np.eye(4)
        out[:3, :3] = R.T
        out[:3, 3] = -(R.T @ u)
    return out.astype(F)


def score(src, tgt, cst, T, voxel):
    """(inliers, error terms) of tdv_ransac's winner scoring for the f32 pose T over the one-way matches cst: threshold 1.5 voxel,
    inlier iff sqrtf(d2) < thr with d2 from the row form of the transform in f32; term (double)(err * err), err = sqrtf(d2)."""
    s = np.asarray(src, F); q = np.asarray(tgt, F)[np.asarray(cst, np.int64)]
    T = np.asarray(T, F)
    thr = F(F(voxel) * F(1.5))
    with np.errstate(invalid="ignore", over="ignore"):
        x = [F(F(T[a, 0] * s[:, 0]) + F(F(T[a, 1] * s[:, 1]) + F(T[a, 2] * s[:, 2]))) + T[a, 3] for a in range(3)]
        d = [(x[a] - q[:, a]).astype(F) for a in range(3)]
        d2 = (d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])).astype(F)
        err = np.sqrt(d2).astype(F)
        inl = err < thr
    return int(inl.sum()), (err[inl] * err[inl]).astype(F).astype(np.float64)


def fgr(src, tgt, cst, cts, voxel, params=None):
    """The whole definition: dict(T (f32 4x4, source onto target), degenerate, inliers, terms, fitness and the correspondences)."""
    p = dict(DEFAULTS, **(params or {}))
    c = correspondences(src, tgt, cst, cts, p)
    if len(c["corr"]) < 10:
        T = np.eye(4, dtype=F); deg = True
    else:
        T64, mu_s, mu_t, sigma = optimise(src, tgt, c["corr"], p)
        T = original_scale(T64, mu_s, mu_t, sigma); deg = False
    inl, terms = score(src, tgt, cst, T, voxel)
    return dict(c, T=T, degenerate=deg, inliers=inl, terms=terms, fitness=F(F(inl) / F(len(src))))
