"""A restatement of ICP with a robust loss (include/tdv_hip.h: tdv_ctx_set_icp_loss), iteration by iteration, from the oracle's pieces.

Correspondences come from the oracle (pyoracle.icp_correspondences: nearest target, its d2, accepted = sqrt(d2) <= thr).  The terms are
formed in f32 the way csrc/icp.hip forms them (transform_point, corr_terms, loss_weight), widened to f64 and scaled by the weight as
acc_terms does; each sum is pyoracle.exact_sum's, which the device's f64 tree gives rounded to the same f32 unless exact_sum reports
the sum ambiguous.  Solve and update use pyoracle.ldlt6_solve, euler_xyz_matrix and kabsch_rotation; the 4x4 product and the
translation steps are written out in np.float32 scalars in dl::mul44's / dl::mulv3's order.

Point-to-point: the device divides f64 tree sums (sm = sum w p / W, H = f32(sum w p q^T - (W sm) tm)).  Here the same expressions are
evaluated on the exactly rounded sums, so a weighted point-to-point iteration agrees with the device to the tree's rounding of W and
of the centring, not necessarily to the bit (with L2 the weights are 1 and W = n_corr exactly).
"""
import numpy as np

F = np.float32
KINDS = {"l2": 0, "huber": 1, "tukey": 2, "cauchy": 3}


def tree_depth(ns):
    """Most additions a term passes through in the device's tree for ns points (oracle.cpp: icp_tree_depth)."""
    return 20 + 4 * ((((ns + 255) // 256) + 127) // 128)


def weight(kind, scale, e):
    """loss_weight: the IRLS weight of residuals e (f32 array), f32 arithmetic without contraction."""
    e = np.asarray(e, F)
    if kind == "l2":
        return np.ones_like(e)
    a = np.abs(e)
    k = F(scale)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "huber":
            return np.where(a <= k, F(1), k / a).astype(F)
        u = (a / k).astype(F)
        if kind == "tukey":
            t = (F(1) - u * u).astype(F)
            return np.where(a <= k, t * t, F(0)).astype(F)
        if kind == "cauchy":
            return (F(1) / (F(1) + u * u)).astype(F)
    raise ValueError(kind)


def transform(T, src):
    """transform_point: p = r0*sx + (r1*sy + r2*sz), then + t, per row, in f32."""
    T = np.asarray(T, F); s = np.asarray(src, F)
    return np.stack([(T[r, 0] * s[:, 0] + (T[r, 1] * s[:, 1] + T[r, 2] * s[:, 2])) + T[r, 3] for r in range(3)], 1).astype(F)


def mul44(A, B):
    """dl::mul44: C(i, j) = A(i,0) B(0,j), then + A(i,k) B(k,j) for k = 1 .. 3, in f32."""
    C = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            acc = F(A[i, 0] * B[0, j])
            for k in range(1, 4):
                acc = F(F(A[i, k] * B[k, j]) + acc)
            C[i, j] = acc
    return C


def _sum(orc, terms, depth, amb):
    _, f32, a = orc.exact_sum(np.asarray(terms, np.float64), depth)
    amb.append(a)
    return F(f32)


def iteration_sums(orc, src, tgt, nrm, T, thr, p2plane, kind, scale):
    """One iteration's correspondences and terms.  Returns a dict: n_corr, n_eff, te (f32 error sum), and point-to-plane ATA (6x6 f32),
    ATb (6 f32) or point-to-point the exactly rounded f64 sums W, SP, SQ, SPQ; ambiguous: some f32 sum within the tree's bound of a
    rounding midpoint."""
    c = orc.icp_correspondences(src, tgt, None, T, thr, False)
    acc = c["accepted"]
    idx = c["corr"][acc]
    d2 = c["d2"][acc].astype(F)
    p = transform(T, src)[acc]
    q = np.asarray(tgt, F)[idx]
    depth = tree_depth(len(src))
    amb = []
    out = dict(n_corr=int(acc.sum()), te=_sum(orc, d2.astype(np.float64), depth, amb))
    if p2plane:
        n = np.asarray(nrm, F)[idx]
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        J = np.stack([py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz], 1).astype(F)
        ex, ey, ez = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
        r = (ex * nx + (ey * ny + ez * nz)).astype(F)
        w = weight(kind, scale, r)
        wd = w.astype(np.float64)
        ATA = np.zeros((6, 6), F); ATb = np.zeros(6, F)
        for a in range(6):
            for b in range(a, 6):
                ATA[a, b] = ATA[b, a] = _sum(orc, wd * (J[:, a] * J[:, b]).astype(np.float64), depth, amb)
            ATb[a] = _sum(orc, wd * (J[:, a] * r).astype(np.float64), depth, amb)
        out.update(ATA=ATA, ATb=ATb)
    else:
        w = weight(kind, scale, np.sqrt(d2).astype(F))
        wd = w.astype(np.float64)
        P = p.astype(np.float64); Q = q.astype(np.float64)
        fs = lambda t: orc.exact_sum(t, depth)[0]   # noqa: E731  (the exact sum rounded to f64)
        out.update(W=fs(wd), SP=np.array([fs(wd * P[:, a]) for a in range(3)]), SQ=np.array([fs(wd * Q[:, a]) for a in range(3)]),
                   SPQ=np.array([[fs(wd * (P[:, a] * Q[:, b])) for b in range(3)] for a in range(3)]))
    out["n_eff"] = int((w > 0).sum())
    out["ambiguous"] = any(amb)
    return out


def delta_transform(orc, s, p2plane, l2):
    """The update of icp_update from the sums (4x4 f32)."""
    D = np.eye(4, dtype=F)
    if p2plane:
        x = orc.ldlt6_solve(s["ATA"].reshape(36), -s["ATb"])
        D[:3, :3] = orc.euler_xyz_matrix(x[0], x[1], x[2])
        D[:3, 3] = x[3:6]
        return D
    n = float(s["n_corr"]) if l2 else s["W"]
    sm = s["SP"] / n; tm = s["SQ"] / n
    H = np.array([[F(s["SPQ"][a, b] - n * sm[a] * tm[b]) for b in range(3)] for a in range(3)], F)
    R = orc.kabsch_rotation(H)
    smf = sm.astype(F); tmf = tm.astype(F)
    D[:3, :3] = R
    for r in range(3):
        D[r, 3] = F(tmf[r] - F(F(R[r, 0] * smf[0]) + F(F(R[r, 1] * smf[1]) + F(R[r, 2] * smf[2]))))
    return D


def icp(orc, src, tgt, nrm, T0, thr, max_iterations, p2plane=True, kind="l2", scale=0.0, fixed=False,
        relative_fitness=np.inf, relative_rmse=1e-6):
    """The device loop (icp_update + the host's bursts): a dict T, rmse, fitness, iterations, n_corr as a tdv_icp_result reads, plus
    ambiguous (some sum of an applied iteration could round the other way on the device) and per-iteration (n_corr, n_eff) in counts.
    relative_fitness, relative_rmse (as f32): the convergence criteria of icp_update, the defaults being the reference's rule;
    history: (rmse, fitness) after every applied iteration."""
    T = np.asarray(T0, F).copy()
    ns = len(src)
    res = dict(T=T.copy(), rmse=F(0), fitness=F(0), iterations=0, n_corr=0, ambiguous=False, counts=[], history=[])
    for it in range(max_iterations):
        s = iteration_sums(orc, src, tgt, nrm, T, thr, p2plane, kind, scale)
        res["counts"].append((s["n_corr"], s["n_eff"]))
        if s["n_corr"] < 3 or s["n_eff"] < 3:
            if fixed:
                continue
            break
        res["ambiguous"] |= s["ambiguous"]
        T = mul44(delta_transform(orc, s, p2plane, kind == "l2"), T)
        prev, prev_fit = res["rmse"], res["fitness"]
        rmse = F(np.sqrt(F(s["te"] / F(s["n_corr"]))))
        fit = F(F(s["n_corr"]) / F(ns))
        res.update(T=T.copy(), rmse=rmse, fitness=fit, iterations=it + 1, n_corr=s["n_corr"])
        res["history"].append((rmse, fit))
        if not fixed and it > 0 and abs(F(prev_fit - fit)) < F(relative_fitness) and abs(F(prev - rmse)) < F(relative_rmse):
            break
    return res


# ---------------------------------------------------------------- the clutter scenario
# A synthetic scan of the part (synth.make_scene: 10 % uniform outliers already) plus a bin floor: a plane 4 mm under the part's bottom
# face, dense enough that a third of the accepted correspondences lie on it.  A threshold of 10 mm (wider than the pipeline's 0.4
# voxel, so that a start 2 deg / 3 mm off converges) accepts the floor; point-to-plane L2 is pulled towards it, Tukey at 2.5 mm is not.
SCENE = dict(n_scan=3000, n_model=3000, n_floor=1500, floor_gap=0.004, thr=0.010, angle=2.0, trans=0.003, seed=11,
             tukey_scale=0.0025, gate_rad=2e-3, gate_m=5e-4, iterations=60)


def clutter_scene(synth, n_scan=None, n_model=None, n_floor=None, floor_gap=None, seed=None):
    """(src, tgt, nrm, T0, T_gt): the scan with the floor in the scan's frame, the model, a start pose off by SCENE's angle and trans."""
    c = dict(SCENE)
    for k, v in (("n_scan", n_scan), ("n_model", n_model), ("n_floor", n_floor), ("floor_gap", floor_gap), ("seed", seed)):
        if v is not None:
            c[k] = v
    tgt, nrm = synth.sample_object(c["n_model"], c["seed"])
    scan, T_gt = synth.make_scene(c["n_scan"], c["seed"] + 1)
    rng = np.random.default_rng(c["seed"] + 2)
    floor = np.stack([rng.uniform(-0.13, 0.13, c["n_floor"]), rng.uniform(-0.08, 0.08, c["n_floor"]),
                      np.full(c["n_floor"], -0.03 - c["floor_gap"])], 1)          # the part's bottom face is z = -0.03 in its frame
    Ti = np.linalg.inv(T_gt.astype(np.float64))
    floor_scan = floor @ Ti[:3, :3].T + Ti[:3, 3]
    src = np.concatenate([scan, floor_scan.astype(np.float32)], 0)
    src = src[np.random.default_rng(c["seed"] + 3).permutation(len(src))].astype(np.float32)
    T0 = synth.perturb(T_gt, seed=c["seed"] + 4, angle_deg=c["angle"], trans=c["trans"]).astype(np.float32)
    return src, tgt, nrm, T0, T_gt


def within_gate(synth, T, T_gt):
    ang, tr = synth.pose_error(T, T_gt)
    return ang <= SCENE["gate_rad"] and tr <= SCENE["gate_m"], (ang, tr)
