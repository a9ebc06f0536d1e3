"""A restatement of colored ICP (include/tdv_hip.h: tdv_color_gradients, tdv_colored_icp), iteration by iteration, from the oracle's pieces.

It implements the header's definition, not the kernels.  Gradients: the intensity I = ((r + g) + b) / 3 in f32, the oracle's exact kNN
lists (pyoracle.estimate_normals, want_knn), u_j and b_j in f32, the normal equations summed in f64 in list order, the cofactor solve in
f64, rounded once.  ICP: correspondences from the oracle (pyoracle.icp_correspondences: nearest target, its d2, accepted = sqrt(d2) <=
thr), the geometric row (point-to-plane's, scaled by lg) and the photometric row in np.float32 in the header's order, each product
widened to f64, scaled by its own row's robust weight and the two rows added in f64; every sum is pyoracle.exact_sum's, which the
device's f64 tree gives rounded to the same f32 unless exact_sum reports the sum ambiguous.  The step is pyoracle.ldlt6_solve,
euler_xyz_matrix and the f32 4x4 product of icp_loss_restatement.mul44.

It also holds the textured scene of the tests: a lid with a sinusoidal texture whose flat top leaves point-to-plane's in-plane slide
and spin about the normal to the narrow rim.
"""
import numpy as np

import icp_loss_restatement as L

F = np.float32
LAMBDA = 0.968          # Open3D's default lambda_geometric
K = 30                  # neighbours of the gradients (and of the normals they go with)


def intensity(rgb):
    """I = ((r + g) + b) / 3.0f per point, f32."""
    c = np.asarray(rgb, F).reshape(-1, 3)
    return (((c[:, 0] + c[:, 1]) + c[:, 2]) / F(3)).astype(F)


def gradients(xyz, rgb, normals, knn):
    """(n, 4) f32: (I, d) per point from the kNN lists knn (n, k) int, -1 padded, as tdv_color_gradients defines them."""
    x = np.asarray(xyz, F).reshape(-1, 3); nrm = np.asarray(normals, F).reshape(-1, 3)
    knn = np.asarray(knn, np.int64).reshape(len(x), -1)
    n = len(x)
    I = intensity(rgb)
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    S = {k: np.zeros(n) for k in ("00", "01", "02", "11", "12", "22")}
    c = [np.zeros(n) for _ in range(3)]
    m = np.zeros(n, np.int64)
    own = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(knn.shape[1]):
            j = knn[:, r]
            valid = (j >= 0) & (j != own)
            jj = np.where(valid, j, 0)
            d = (x[jj] - x).astype(F)
            t = (d[:, 0] * nx + (d[:, 1] * ny + d[:, 2] * nz)).astype(F)
            u = [(d[:, a] - t * nrm[:, a]).astype(F).astype(np.float64) for a in range(3)]
            b = (I[jj] - I).astype(F).astype(np.float64)
            for key in S:
                S[key] = S[key] + np.where(valid, u[int(key[0])] * u[int(key[1])], 0.0)
            for a in range(3):
                c[a] = c[a] + np.where(valid, u[a] * b, 0.0)
            m += valid
        mm = m.astype(np.float64) * m.astype(np.float64)
        N = [nrm[:, a].astype(np.float64) for a in range(3)]
        A = {key: S[key] + (mm * N[int(key[0])]) * N[int(key[1])] for key in S}
        A00, A01, A02, A11, A12, A22 = (A[k] for k in ("00", "01", "02", "11", "12", "22"))
        C00 = A11 * A22 - A12 * A12; C11 = A00 * A22 - A02 * A02; C22 = A00 * A11 - A01 * A01
        C01 = A02 * A12 - A01 * A22; C02 = A01 * A12 - A02 * A11; C12 = A01 * A02 - A00 * A12
        det = A00 * C00 + (A01 * C01 + A02 * C02)
        ok = (m >= 3) & (det > 0) & (det < np.inf)
        sdet = np.where(ok, det, 1.0)
        d0 = (C00 * c[0] + (C01 * c[1] + C02 * c[2])) / sdet
        d1 = (C01 * c[0] + (C11 * c[1] + C12 * c[2])) / sdet
        d2 = (C02 * c[0] + (C12 * c[1] + C22 * c[2])) / sdet
    out = np.zeros((n, 4), F)
    out[:, 0] = I
    out[:, 1] = np.where(ok, d0, 0.0).astype(F)
    out[:, 2] = np.where(ok, d1, 0.0).astype(F)
    out[:, 3] = np.where(ok, d2, 0.0).astype(F)
    return out


def gradients_of(orc, xyz, rgb, normals, k=K):
    """gradients() on the oracle's exact kNN lists for k (the lists tdv_estimate_normals returns)."""
    _, knn = orc.estimate_normals(np.asarray(xyz, F), k, want_knn=True)
    return gradients(xyz, rgb, normals, knn)


def weights_of_lambda(lam):
    """lg = sqrtf(lambda), lc = sqrtf(1 - lambda) in f32."""
    lam = F(lam)
    return F(np.sqrt(lam)), F(np.sqrt(F(F(1) - lam)))


def rows(p, q, n, tc, Is, lg, lc):
    """The two rows of each correspondence in the header's order: JG (k, 6), rG (k,), JC (k, 6), rC (k,), all f32."""
    p = np.asarray(p, F); q = np.asarray(q, F); n = np.asarray(n, F); tc = np.asarray(tc, F).reshape(-1, 4); Is = np.asarray(Is, F)
    lg = F(lg); lc = F(lc)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        J = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
        ex, ey, ez = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
        en = ex * nx + (ey * ny + ez * nz)
        etx, ety, etz = ex - en * nx, ey - en * ny, ez - en * nz
        Iq, dx, dy, dz = tc[:, 0], tc[:, 1], tc[:, 2], tc[:, 3]
        dn = dx * nx + (dy * ny + dz * nz)
        gx, gy, gz = dn * nx - dx, dn * ny - dy, dn * nz - dz
        de = dx * etx + (dy * ety + dz * etz)
        rG = lg * en
        rC = lc * (Is - (Iq + de))
        JG = np.stack([lg * Ja for Ja in J], 1).astype(F)
        JC = np.stack([lc * (py * gz - pz * gy), lc * (pz * gx - px * gz), lc * (px * gy - py * gx), lc * gx, lc * gy, lc * gz], 1).astype(F)
    return JG, rG.astype(F), JC, rC.astype(F)


def terms(JG, rG, JC, rC, wG=None, wC=None):
    """The 27 f64 terms (k, 27) - H's 21 upper-triangular entries in row order, then v's 6: per slot (double)wG * (JG product) +
    (double)wC * (JC product), each product formed in f32; wG = wC = None: the L2 terms (double)(JG product) + (double)(JC product)."""
    cols = []
    with np.errstate(invalid="ignore", over="ignore"):
        def slot(g, c):
            g = np.asarray(g, F).astype(np.float64); c = np.asarray(c, F).astype(np.float64)
            if wG is None:
                return g + c
            return np.asarray(wG, F).astype(np.float64) * g + np.asarray(wC, F).astype(np.float64) * c
        for a in range(6):
            for b in range(a, 6):
                cols.append(slot(JG[:, a] * JG[:, b], JC[:, a] * JC[:, b]))
        for a in range(6):
            cols.append(slot(JG[:, a] * rG, JC[:, a] * rC))
    return np.stack(cols, 1)


def iteration_sums(orc, src, src_rgb, tgt, tgt_normals, tgt_color, T, thr, lam=LAMBDA, kind="l2", scale=0.0):
    """One iteration: n_corr, n_eff, te (f32 error sum), ATA (6x6 f32), ATb (6 f32), ambiguous."""
    c = orc.icp_correspondences(src, tgt, None, T, thr, False)
    acc = c["accepted"]
    idx = c["corr"][acc]
    d2 = c["d2"][acc].astype(F)
    T = np.asarray(T, F)
    p = L.transform(T, src)[acc]
    q = np.asarray(tgt, F)[idx]
    n = np.asarray(tgt_normals, F)[idx]
    tc = np.asarray(tgt_color, F).reshape(-1, 4)[idx]
    Is = intensity(src_rgb)[acc]
    lg, lc = weights_of_lambda(lam)
    JG, rG, JC, rC = rows(p, q, n, tc, Is, lg, lc)
    depth = L.tree_depth(len(src))
    amb = []
    out = dict(n_corr=int(acc.sum()), te=L._sum(orc, d2.astype(np.float64), depth, amb))
    if kind == "l2":
        t = terms(JG, rG, JC, rC)
        n_eff = int(acc.sum())
    else:
        wG = L.weight(kind, scale, rG); wC = L.weight(kind, scale, rC)
        t = terms(JG, rG, JC, rC, wG, wC)
        n_eff = int(((wG > 0) | (wC > 0)).sum())
    sums = [L._sum(orc, t[:, k], depth, amb) for k in range(27)]
    ATA = np.zeros((6, 6), F); ATb = np.zeros(6, F)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            ATA[a, b] = ATA[b, a] = sums[k]; k += 1
    ATb[:] = sums[21:]
    out.update(ATA=ATA, ATb=ATb, n_eff=n_eff, ambiguous=any(amb))
    return out


def colored_icp(orc, src, src_rgb, tgt, tgt_normals, tgt_color, T0, thr, max_iterations, lam=LAMBDA, kind="l2", scale=0.0, fixed=False,
                relative_fitness=np.inf, relative_rmse=1e-6):
    """The device loop: a dict T, rmse, fitness, iterations, n_corr as a tdv_icp_result reads, ambiguous (some sum of an applied
    iteration could round the other way on the device) and per-iteration (n_corr, n_eff) in counts.
    relative_fitness, relative_rmse (as f32): the convergence criteria of icp_update, the defaults being the reference's rule;
    history: (rmse, fitness) after every applied iteration."""
    T = np.asarray(T0, F).copy()
    ns = len(src)
    res = dict(T=T.copy(), rmse=F(0), fitness=F(0), iterations=0, n_corr=0, ambiguous=False, counts=[], history=[])
    for it in range(max_iterations):
        s = iteration_sums(orc, src, src_rgb, tgt, tgt_normals, tgt_color, T, thr, lam, kind, scale)
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


# ---------------------------------------------------------------- the textured scene
# A cuboid lid 100 x 100 mm with a 4 mm rim, textured I = 0.5 + 0.25 sin(2 pi x / WAVE) sin(2 pi y / WAVE) (grey, r = g = b).  The model
# is a 2.5 mm grid with analytic normals, rim walls included; the scan sees the top only, as a sensor above the lid does, sampled at its
# own random positions (not the model's points), and starts off by an in-plane slide and a spin about the top's normal.  Geometry then
# holds the slide and the spin only where the scan's border meets the model's edge.
WAVE = 0.03
SCENE = dict(half=0.05, rim=0.004, step=0.0025, n_scan=3000, slide=(0.002, -0.0015), spin_deg=3.0, thr=0.01, iterations=30, walls=False,
             seed=1)


def texture(xyz):
    x = np.asarray(xyz, np.float64)
    I = 0.5 + 0.25 * np.sin(2 * np.pi * x[:, 0] / WAVE) * np.sin(2 * np.pi * x[:, 1] / WAVE)
    return np.repeat(I[:, None], 3, 1).astype(F)


def _lid_surface(u, v, face, half, rim):
    """Points of the lid's faces from parameters u, v in [0, 1): face 0 the top (z = 0), 1..4 the rim walls (z in [-rim, 0])."""
    a = (2 * u - 1) * half
    h = -v * rim
    if face == 0:
        return np.stack([a, (2 * v - 1) * half, np.zeros_like(u)], 1), np.array([0.0, 0.0, 1.0])
    s = 1.0 if face in (1, 3) else -1.0
    if face in (1, 2):
        return np.stack([np.full_like(u, s * half), a, h], 1), np.array([s, 0.0, 0.0])
    return np.stack([a, np.full_like(u, s * half), h], 1), np.array([0.0, s, 0.0])


def lid_model(half=SCENE["half"], rim=SCENE["rim"], step=SCENE["step"]):
    """(points, normals, rgb) of the model: a grid of pitch step on the top and on the walls."""
    m = int(round(2 * half / step))
    g = (np.arange(m) + 0.5) / m
    U, V = np.meshgrid(g, g, indexing="ij")
    pts, nrm = [], []
    p, n = _lid_surface(U.ravel(), V.ravel(), 0, half, rim)
    pts.append(p); nrm.append(np.broadcast_to(n, p.shape))
    mr = max(2, int(round(rim / step)) + 1)
    gr = np.arange(mr) / (mr - 1)
    U, V = np.meshgrid(g, gr, indexing="ij")
    for face in (1, 2, 3, 4):
        p, n = _lid_surface(U.ravel(), V.ravel(), face, half, rim)
        pts.append(p); nrm.append(np.broadcast_to(n, p.shape))
    P = np.concatenate(pts).astype(F)
    return P, np.concatenate(nrm).astype(F), texture(P)


def lid_scene(seed, n_scan=SCENE["n_scan"], slide=SCENE["slide"], spin_deg=SCENE["spin_deg"], walls=SCENE["walls"]):
    """(src, src_rgb, tgt, tgt_normals, T0, T_gt): the scan in the sensor frame, T_gt maps it onto the model, T0 = the start.
    walls: the scan sees the rim walls too (else the top only, as a sensor above the lid does)."""
    rng = np.random.default_rng(seed)
    half, rim = SCENE["half"], SCENE["rim"]
    top_area, wall_area = (2 * half) ** 2, 2 * half * rim
    p_face = np.array([top_area] + [wall_area if walls else 0.0] * 4); p_face /= p_face.sum()
    face = rng.choice(5, size=n_scan, p=p_face)
    pts = np.zeros((n_scan, 3))
    for f in range(5):
        sel = face == f
        p, _ = _lid_surface(rng.random(sel.sum()), rng.random(sel.sum()), f, half, rim)
        pts[sel] = p
    rgb = texture(pts)
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    ang = np.deg2rad(rng.uniform(10, 30))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    T_gt = np.eye(4); T_gt[:3, :3] = R; T_gt[:3, 3] = rng.uniform(-0.02, 0.02, 3) + np.array([0, 0, 0.5])
    T_gt = np.linalg.inv(T_gt)                     # sensor -> model
    Ti = np.linalg.inv(T_gt)
    src = (pts @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    c, s = np.cos(np.deg2rad(spin_deg)), np.sin(np.deg2rad(spin_deg))
    D = np.eye(4); D[:2, :2] = [[c, -s], [s, c]]; D[0, 3], D[1, 3] = slide
    T0 = (D @ T_gt).astype(F)
    tgt, nrm, _ = lid_model()
    return src, rgb, tgt, nrm, T0, T_gt.astype(F)


def lid_target_color(orc):
    """The model's colour table (gradients on its analytic normals, k = K)."""
    tgt, nrm, rgb = lid_model()
    return gradients_of(orc, tgt, rgb, nrm)
