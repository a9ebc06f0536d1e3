"""A restatement of plane segmentation by RANSAC (include/tdv_hip.h: tdv_segment_planes) in numpy, step by step as the header states it.

It implements the header's definition, not the kernels: the Philox draw of each hypothesis (fgr_restatement.philox4x32 with key
(seed, 1)), the f64 plane of the three candidates, the strict inlier test, the chunked arg-max with the lowest t on ties and the early
stop after each chunk, the acceptance rule, the rounds over the shrinking candidate set, the reported hypothesis and the least-squares
refit.  The discrete results (labels, counts, winners, iterations run, the hypothesis' bits, the rest cloud) are exact; the refit plane
and rmse agree with the device's to the last places of the sum order and the eigen solver (numpy's eigh here, a Jacobi sweep there).
"""
import numpy as np

from fgr_restatement import philox4x32

F = np.float32
CHUNK = 1024               # TDV_PLANE_CHUNK
PLANE_MAX = 16             # TDV_PLANE_MAX
DEFAULTS = dict(probability=0.99999999, distance_threshold=0.01, num_iterations=100, max_planes=1, min_inliers=3, refit=1, seed=42)
SCORE_BLOCK = 8            # hypotheses scored at once (memory only: the counts do not depend on it)


def draw(t, k, m, seed):
    """Candidate indices (3, len(t)) of hypotheses t of round k over m candidates: words x0..x2 of Philox(counter (t, k, 0, 0), key
    (seed, 1)), index (x * m) >> 32."""
    t = np.asarray(t, np.uint64)
    z = np.zeros_like(t)
    x = philox4x32((t, z + np.uint64(k), z, z), (seed, 1))
    return ((x[:3] * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def planes(cand, idx):
    """(a, b, c, d) f64 arrays and the validity of the hypotheses whose candidate indices are idx (3, h).  An invalid hypothesis gets
    (0, 0, 0, NaN): it scores nothing."""
    P = np.asarray(cand, F).astype(np.float64)
    i0, i1, i2 = idx
    p0, p1, p2 = P[i0], P[i1], P[i2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = p1 - p0
        v = p2 - p0
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        s = (nx * nx + ny * ny) + nz * nz
        valid = (i0 != i1) & (i0 != i2) & (i1 != i2) & (s > 0) & np.isfinite(s)
        r = np.sqrt(s)
        a, b, c = nx / r, ny / r, nz / r
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
    zero = np.zeros_like(a)
    a, b, c = np.where(valid, a, zero), np.where(valid, b, zero), np.where(valid, c, zero)
    d = np.where(valid, d, np.nan)
    return np.stack([a, b, c, d], 1), valid


def distances(cand, pl):
    """|((a x + b y) + c z) + d| in f64 for every candidate against one plane pl (4 f64)."""
    P = np.asarray(cand, F).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(((pl[0] * P[:, 0] + pl[1] * P[:, 1]) + pl[2] * P[:, 2]) + pl[3])


def counts(cand, pls, thr):
    """Inlier counts of the planes pls (h, 4) over the candidates (strict <; a NaN distance is no inlier)."""
    P = np.asarray(cand, F).astype(np.float64)
    out = np.zeros(len(pls), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, len(pls), SCORE_BLOCK):
            q = pls[lo:lo + SCORE_BLOCK]
            dist = np.abs(((q[:, 0:1] * P[None, :, 0] + q[:, 1:2] * P[None, :, 1]) + q[:, 2:3] * P[None, :, 2]) + q[:, 3:4])
            out[lo:lo + SCORE_BLOCK] = (dist < thr).sum(1)
    return out


def stops(best, m, run, probability):
    """The early-stop rule after a chunk: best count b, m candidates, run hypotheses so far."""
    if not (probability < 1.0 and best > 0):
        return False
    f = float(best) / float(m)
    if f >= 1.0:
        return True
    with np.errstate(divide="ignore"):
        L = np.log(1.0 - (f * f) * f)
        return bool(L < 0.0 and float(run) >= np.log(1.0 - probability) / L)


def search(cand, k, p):
    """One round's search: dict(best_count, best_t, run)."""
    m = len(cand)
    thr = np.float64(F(p["distance_threshold"]))
    best_c, best_t, run = -1, 0, 0
    n_it = p["num_iterations"]
    for t0 in range(0, n_it, CHUNK):
        h = min(CHUNK, n_it - t0)
        pls, _ = planes(cand, draw(np.arange(t0, t0 + h), k, m, p["seed"]))
        c = counts(cand, pls, thr)
        i = int(np.argmax(c))                      # the first maximum: the lowest t
        if c[i] > best_c:
            best_c, best_t = int(c[i]), t0 + i
        run += h
        if t0 + h >= n_it or stops(best_c, m, run, p["probability"]):
            break
    return dict(best_count=best_c, best_t=best_t, run=run)


def refit_plane(inl, hyp_normal):
    """Least-squares plane of the inliers (f64): the unit eigenvector of the smallest eigenvalue of the centred scatter, turned towards
    hyp_normal, and d = -n . mean; None when it is not finite."""
    P = np.asarray(inl, F).astype(np.float64)
    mu = P.sum(0) / len(P)
    D = P - mu
    w, V = np.linalg.eigh(D.T @ D)
    e = V[:, int(np.argmin(w))]
    e = e / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    if (e[0] * hyp_normal[0] + e[1] * hyp_normal[1]) + e[2] * hyp_normal[2] < 0:
        e = -e
    d = -((e[0] * mu[0] + e[1] * mu[1]) + e[2] * mu[2])
    out = np.array([e[0], e[1], e[2], d])
    return out if np.isfinite(out).all() else None


def segment_planes(xyz, params=None):
    """The whole definition: dict(planes = list of result dicts as the ABI reports them (plus plane64: the refit in f64), labels
    int32[n], rest (the unlabelled points in ascending index), n_planes)."""
    p = dict(DEFAULTS, **(params or {}))
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    labels = np.full(n, -1, np.int32)
    cand_idx = np.arange(n)
    thr = np.float64(F(p["distance_threshold"]))
    out = []
    for k in range(p["max_planes"]):
        cand = xyz[cand_idx]
        m = len(cand)
        if m < 3:
            break
        s = search(cand, k, p)
        pl, valid = planes(cand, draw(np.array([s["best_t"]]), k, m, p["seed"]))
        if not valid[0] or s["best_count"] < p["min_inliers"]:
            break
        pl = pl[0]
        dist = distances(cand, pl)
        inl = dist < thr
        assert int(inl.sum()) == s["best_count"]
        labels[cand_idx[inl]] = k
        flip = pl[3] < 0
        hyp = pl.astype(F)
        if flip:
            hyp = -hyp
        plane, plane64 = hyp.copy(), None
        if p["refit"]:
            plane64 = refit_plane(cand[inl], -pl[:3] if flip else pl[:3])
            if plane64 is not None:
                plane = plane64.astype(F)
        cnt = s["best_count"]
        out.append(dict(plane=plane, hypothesis=hyp, fitness=F(cnt / m), rmse=F(np.sqrt((dist[inl] ** 2).sum() / cnt)), inliers=cnt,
                        candidates=m, best_iteration=s["best_t"], iterations_run=s["run"], plane64=plane64))
        cand_idx = cand_idx[~inl]
    return dict(planes=out, labels=labels, rest=xyz[labels == -1], n_planes=len(out))
