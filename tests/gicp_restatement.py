"""A restatement of generalized ICP (include/tdv_hip.h: tdv_gicp), iteration by iteration, from the oracle's pieces.

It implements the header's definition, not the kernel: correspondences from the oracle (pyoracle.icp_correspondences: nearest target,
its d2, accepted = sqrt(d2) <= thr), a = R ns, C, its cofactors, M = C^-1, g = M e and the 27 terms in np.float32 in the header's order,
each widened to f64 (and scaled by the robust weight of the Mahalanobis residual, as tests/icp_loss_restatement.py scales
point-to-plane's); every sum is pyoracle.exact_sum's, which the device's f64 tree gives rounded to the same f32 unless exact_sum reports
the sum ambiguous.  The step is pyoracle.ldlt6_solve, euler_xyz_matrix and the f32 4x4 product of icp_loss_restatement.mul44.
"""
import numpy as np

import icp_loss_restatement as L

F = np.float32
EPSILON = 1e-3


def rotate(T, v):
    """a = R v per row, r0*vx + (r1*vy + r2*vz) in f32: transform without the translation."""
    T = np.asarray(T, F); v = np.asarray(v, F)
    return np.stack([T[r, 0] * v[:, 0] + (T[r, 1] * v[:, 1] + T[r, 2] * v[:, 2]) for r in range(3)], 1).astype(F)


def covariance(a, n, c):
    """C = 2 I - c (a a^T + n n^T) per correspondence, f32, as the 6 entries (C00, C11, C22, C01, C02, C12)."""
    a = np.asarray(a, F); n = np.asarray(n, F); c = F(c)
    s = lambda i, j: (a[:, i] * a[:, j] + n[:, i] * n[:, j]).astype(F)   # noqa: E731
    two = F(2)
    return dict(C00=two - c * s(0, 0), C11=two - c * s(1, 1), C22=two - c * s(2, 2),
                C01=-(c * s(0, 1)), C02=-(c * s(0, 2)), C12=-(c * s(1, 2)))


def inverse(C):
    """M = C^-1: the cofactors, the determinant and s = 1 / det in f64 from the f32 entries, M_ij = f32(A_ij * s), in the header's
    order: dict M00, M11, M22, M01, M02, M12 (f32)."""
    C00, C11, C22, C01, C02, C12 = (np.asarray(C[k], np.float64) for k in ("C00", "C11", "C22", "C01", "C02", "C12"))
    A00 = C11 * C22 - C12 * C12; A11 = C00 * C22 - C02 * C02; A22 = C00 * C11 - C01 * C01
    A01 = C02 * C12 - C01 * C22; A02 = C01 * C12 - C02 * C11; A12 = C01 * C02 - C00 * C12
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = 1.0 / (C00 * A00 + (C01 * A01 + C02 * A02))
    return dict(M00=(A00 * s).astype(F), M11=(A11 * s).astype(F), M22=(A22 * s).astype(F),
                M01=(A01 * s).astype(F), M02=(A02 * s).astype(F), M12=(A12 * s).astype(F))


def full(S, name):
    """The 3x3 symmetric matrices (k, 3, 3) of the 6-entry dict S with entries name00 .. name12."""
    g = lambda i, j: S["%s%d%d" % (name, min(i, j), max(i, j))]   # noqa: E731
    return np.stack([np.stack([g(i, j) for j in range(3)], -1) for i in range(3)], -2)


def terms(p, q, nt, a, c):
    """The 27 f32 terms (k, 27) - H's 21 upper-triangular entries in row order, then v's 6 - and the Mahalanobis e.g (k,)."""
    p = np.asarray(p, F); q = np.asarray(q, F)
    M = inverse(covariance(a, nt, c))
    M00, M11, M22, M01, M02, M12 = (M[k] for k in ("M00", "M11", "M22", "M01", "M02", "M12"))
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    ex, ey, ez = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
    gx = M00 * ex + (M01 * ey + M02 * ez); gy = M01 * ex + (M11 * ey + M12 * ez); gz = M02 * ex + (M12 * ey + M22 * ez)
    eg = ex * gx + (ey * gy + ez * gz)

    def cross(x0, x1, x2):
        return py * x2 - pz * x1, pz * x0 - px * x2, px * x1 - py * x0
    P0 = cross(M00, M01, M02); P1 = cross(M01, M11, M12); P2 = cross(M02, M12, M22)
    K = [(P0[b], P1[b], P2[b]) for b in range(3)]
    H = {}
    for b in range(3):
        kb = cross(*K[b])
        for a_ in range(b + 1):
            H[a_, b] = kb[a_]
    P = (P0, P1, P2)
    for a_ in range(3):
        for j in range(3):
            H[a_, 3 + j] = P[j][a_]
    Mf = {(0, 0): M00, (1, 1): M11, (2, 2): M22, (0, 1): M01, (0, 2): M02, (1, 2): M12}
    for i in range(3):
        for j in range(i, 3):
            H[3 + i, 3 + j] = Mf[i, j]
    v = list(cross(gx, gy, gz)) + [gx, gy, gz]
    cols = [H[a_, b] for a_ in range(6) for b in range(a_, 6)] + v
    return np.stack(cols, 1).astype(F), eg.astype(F)


def iteration_sums(orc, src, src_normals, tgt, tgt_normals, T, thr, epsilon=EPSILON, kind="l2", scale=0.0):
    """One iteration: n_corr, n_eff, te (f32 error sum), ATA (6x6 f32), ATb (6 f32), ambiguous."""
    c = orc.icp_correspondences(src, tgt, None, T, thr, False)
    acc = c["accepted"]
    idx = c["corr"][acc]
    d2 = c["d2"][acc].astype(F)
    T = np.asarray(T, F)
    p = L.transform(T, src)[acc]
    a = rotate(T, np.asarray(src_normals, F)[acc])
    q = np.asarray(tgt, F)[idx]
    nt = np.asarray(tgt_normals, F)[idx]
    depth = L.tree_depth(len(src))
    amb = []
    out = dict(n_corr=int(acc.sum()), te=L._sum(orc, d2.astype(np.float64), depth, amb))
    t, eg = terms(p, q, nt, a, F(F(1) - F(epsilon)))
    w = L.weight(kind, scale, np.sqrt(np.maximum(F(0), eg)).astype(F))
    wd = w.astype(np.float64)
    sums = [L._sum(orc, wd * t[:, k].astype(np.float64), depth, amb) for k in range(27)]
    ATA = np.zeros((6, 6), F); ATb = np.zeros(6, F)
    k = 0
    for a_ in range(6):
        for b in range(a_, 6):
            ATA[a_, b] = ATA[b, a_] = sums[k]; k += 1
    ATb[:] = sums[21:]
    out.update(ATA=ATA, ATb=ATb, n_eff=int((w > 0).sum()), ambiguous=any(amb))
    return out


def gicp(orc, src, src_normals, tgt, tgt_normals, T0, thr, max_iterations, epsilon=EPSILON, kind="l2", scale=0.0, fixed=False,
         relative_fitness=np.inf, relative_rmse=1e-6):
    """The device loop: a dict T, rmse, fitness, iterations, n_corr as a tdv_icp_result reads, ambiguous (some sum of an applied
    iteration could round the other way on the device) and per-iteration (n_corr, n_eff) in counts.
    relative_fitness, relative_rmse (as f32): the convergence criteria of icp_update, the defaults being the reference's rule;
    history: (rmse, fitness) after every applied iteration."""
    T = np.asarray(T0, F).copy()
    ns = len(src)
    res = dict(T=T.copy(), rmse=F(0), fitness=F(0), iterations=0, n_corr=0, ambiguous=False, counts=[], history=[])
    for it in range(max_iterations):
        s = iteration_sums(orc, src, src_normals, tgt, tgt_normals, T, thr, epsilon, kind, scale)
        res["counts"].append((s["n_corr"], s["n_eff"]))
        if s["n_corr"] < 3 or s["n_eff"] < 3:
            if fixed:
                continue
            break
        res["ambiguous"] |= s["ambiguous"]
        T = L.mul44(L.delta_transform(orc, s, True, True), T)
        prev, prev_fit = res["rmse"], res["fitness"]
        rmse = F(np.sqrt(F(s["te"] / F(s["n_corr"]))))
        fit = F(F(s["n_corr"]) / F(ns))
        res.update(T=T.copy(), rmse=rmse, fitness=fit, iterations=it + 1, n_corr=s["n_corr"])
        res["history"].append((rmse, fit))
        if not fixed and it > 0 and abs(F(prev_fit - fit)) < F(relative_fitness) and abs(F(prev - rmse)) < F(relative_rmse):
            break
    return res
