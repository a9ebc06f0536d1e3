"""Depth odometry's rules O1 to O9 (include/tdv_hip.h: tdv_depth_odometry_dev) restated in numpy from the header's text: float32 with one
rounding per operation in the order written, the 29 sums of O7 over tests/fixed_tree_restatement.py, the step of O8 through
oracle.pyoracle.ldlt6_solve and euler_xyz_matrix (the device's versions are held to those by tests/test_gpu_solver_probe.py) and a
restated 4x4 product.  It shares nothing with csrc/odometry.hip.  Poses are row-major [4, 4] here, intrinsics (scale, fx, fy, cx, cy).

numpy keeps float32 where every operand is float32 and neither contracts nor reorders; every scalar below is made float32 first."""
import numpy as np

import fixed_tree_restatement as tree

F = np.float32
MAX_LEVELS = 4
DEFAULTS = dict(depth_diff=0.03, zmax=10.0, n_levels=3, max_iterations=(20, 10, 5, 0))
QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in p:
            raise TypeError(k)
    p.update(kw)
    its = [int(x) for x in p["max_iterations"]]
    p["max_iterations"] = tuple(its + [0] * (MAX_LEVELS - len(its)))
    p["depth_diff"], p["zmax"] = F(p["depth_diff"]), F(p["zmax"])
    return p


# ------------------------------------------------------------------------------------------------ O1 to O4
def depth0(raw, scale, zmax):
    """O1: float32 [h, w], 0 where invalid."""
    raw = np.asarray(raw, np.uint16)
    inv = F(1.0 / float(F(scale)))
    z = raw.astype(F) * inv
    return np.where((raw != 0) & (z <= F(zmax)), z, F(0)).astype(F)


def level_intrinsics(fx, fy, cx, cy, level):
    """O4: the intrinsics `level` halvings down."""
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    for _ in range(level):
        fx, fy, cx, cy = fx * F(0.5), fy * F(0.5), (cx - F(0.5)) * F(0.5), (cy - F(0.5)) * F(0.5)
    return fx, fy, cx, cy


def vertex(u, v, z, cam):
    """O2 for arrays u, v (ints) and z (float32): three float32 arrays."""
    fx, fy, cx, cy = cam
    with np.errstate(**QUIET):
        x = ((u.astype(F) - cx) * z) / fx
        y = ((v.astype(F) - cy) * z) / fy
    return x.astype(F), y.astype(F), z.astype(F)


def vertex_map(z, cam):
    """float32 [h, w, 3]: O2 at the valid pixels, zeros elsewhere."""
    h, w = z.shape
    v, u = np.mgrid[0:h, 0:w]
    x, y, zz = vertex(u, v, z, cam)
    valid = z > 0
    return np.where(valid[..., None], np.stack([x, y, zz], -1), F(0)).astype(F)


def normal_map(z, cam, depth_diff):
    """O3: float32 [h, w, 3], zeros where the normal is absent."""
    h, w = z.shape
    dd = F(depth_diff)
    V = vertex_map(z, cam)
    out = np.zeros((h, w, 3), F)
    if h < 2 or w < 2:
        return out
    z0, zu, zv = z[:-1, :-1], z[:-1, 1:], z[1:, :-1]
    with np.errstate(**QUIET):
        ok = (z0 > 0) & (zu > 0) & (zv > 0) & (np.abs(zu - z0) <= dd) & (np.abs(zv - z0) <= dd)
        a = V[:-1, 1:] - V[:-1, :-1]
        b = V[1:, :-1] - V[:-1, :-1]
        n0 = b[..., 1] * a[..., 2] - b[..., 2] * a[..., 1]
        n1 = b[..., 2] * a[..., 0] - b[..., 0] * a[..., 2]
        n2 = b[..., 0] * a[..., 1] - b[..., 1] * a[..., 0]
        L = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        ok &= (L > 0) & np.isfinite(L)
        n = np.stack([n0 / L, n1 / L, n2 / L], -1)
    out[:-1, :-1] = np.where(ok[..., None], n, F(0))
    return out


def downsample(z, depth_diff):
    """O4: the next level's depth."""
    h, w = z.shape
    h2, w2 = h // 2, w // 2
    dd = F(depth_diff)
    blk = [z[0:2 * h2:2, 0:2 * w2:2], z[0:2 * h2:2, 1:2 * w2:2], z[1:2 * h2:2, 0:2 * w2:2], z[1:2 * h2:2, 1:2 * w2:2]]
    z0 = np.zeros((h2, w2), F)
    have = np.zeros((h2, w2), bool)
    for b in blk:
        take = (b > 0) & ~have
        z0 = np.where(take, b, z0)
        have |= b > 0
    s = np.zeros((h2, w2), F)
    cnt = np.zeros((h2, w2), np.int32)
    for b in blk:
        m = (b > 0) & (np.abs(b - z0) <= dd)
        s = np.where(m, np.where(cnt > 0, s + b, b), s).astype(F)
        cnt += m
    with np.errstate(**QUIET):
        return np.where(cnt > 0, s / cnt.astype(F), F(0)).astype(F)


def pyramid(raw, intr, p):
    """A frame's levels: a list of dict(z, normals, cam, n_valid)."""
    scale, fx, fy, cx, cy = intr
    z = depth0(raw, scale, p["zmax"])
    out = []
    for l in range(p["n_levels"]):
        if l:
            z = downsample(z, p["depth_diff"])
        cam = level_intrinsics(fx, fy, cx, cy, l)
        out.append(dict(z=z, normals=normal_map(z, cam, p["depth_diff"]), cam=cam, n_valid=int((z > 0).sum())))
    return out


def maps(raw, intr, **kw):
    """tdv_depth_maps: dict(vertex_map, normal_map, xyz, normals)."""
    p = params(**kw)
    scale, fx, fy, cx, cy = intr
    z = depth0(raw, scale, p["zmax"])
    cam = level_intrinsics(fx, fy, cx, cy, 0)
    vm, nm = vertex_map(z, cam), normal_map(z, cam, p["depth_diff"])
    has = (nm != 0).any(-1)
    return dict(vertex_map=vm, normal_map=nm, xyz=vm[has], normals=nm[has])


# ------------------------------------------------------------------------------------------------ O5 to O7
def terms(src, tgt, T, p):
    """O5 + O6 for one level (src, tgt: that level of pyramid()): float64 [w*h, 29], zeros for a pixel without a partner."""
    T = np.asarray(T, F)
    cam = src["cam"]
    fx, fy, cx, cy = cam
    zs = src["z"]
    h, w = zs.shape
    v, u = np.mgrid[0:h, 0:w]
    px, py, pz = vertex(u, v, zs, cam)
    out = np.zeros((h * w, 29), np.float64)
    with np.errstate(**QUIET):
        qx = ((T[0, 0] * px + T[0, 1] * py) + T[0, 2] * pz) + T[0, 3]
        qy = ((T[1, 0] * px + T[1, 1] * py) + T[1, 2] * pz) + T[1, 3]
        qz = ((T[2, 0] * px + T[2, 1] * py) + T[2, 2] * pz) + T[2, 3]
        ok = (zs > 0) & np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz) & (qz > 0) & (qz <= p["zmax"])
        uf = (qx * fx) / qz + cx
        vf = (qy * fy) / qz + cy
        ok &= (np.abs(uf) < F(1048576.0)) & (np.abs(vf) < F(1048576.0))
        ut = np.floor(np.where(ok, uf, F(0)) + F(0.5)).astype(np.int64)
        vt = np.floor(np.where(ok, vf, F(0)) + F(0.5)).astype(np.int64)
        ok &= (ut >= 0) & (ut < w) & (vt >= 0) & (vt < h)
        ut, vt = np.where(ok, ut, 0), np.where(ok, vt, 0)
        n = tgt["normals"][vt, ut]
        zt = tgt["z"][vt, ut]
        ok &= (n != 0).any(-1) & (np.abs(zt - qz) <= p["depth_diff"])
        tx, ty, tz = vertex(ut, vt, zt, cam)
        n0, n1, n2 = n[..., 0], n[..., 1], n[..., 2]
        J = [qy * n2 - qz * n1, qz * n0 - qx * n2, qx * n1 - qy * n0, n0, n1, n2]
        ex, ey, ez = qx - tx, qy - ty, qz - tz
        r = ex * n0 + (ey * n1 + ez * n2)
        d2 = ex * ex + (ey * ey + ez * ez)
        cols = [np.ones_like(d2, dtype=np.float64), d2.astype(np.float64)]
        for a in range(6):
            for b in range(a, 6):
                cols.append((J[a] * J[b]).astype(F).astype(np.float64))
        for a in range(6):
            cols.append((J[a] * r).astype(F).astype(np.float64))
    m = ok.reshape(-1)
    allc = np.stack([c.reshape(-1) for c in cols], 1)
    out[m] = allc[m]
    return out


def sums(src, tgt, T, p):
    """O7: float64 [29]."""
    return tree.tree_sum(terms(src, tgt, T, p))


# ------------------------------------------------------------------------------------------------ O8, O9
def mul44(A, B):
    """C(i, j) = A(i,0) B(0,j), then A(i,k) B(k,j) + the sum so far for k = 1 .. 3, in float32."""
    C = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            acc = F(A[i, 0] * B[0, j])
            for k in range(1, 4):
                acc = F(F(A[i, k] * B[k, j]) + acc)
            C[i, j] = acc
    return C


def step(orc, s, T):
    """The update of O8 from the sums: the new pose."""
    A = np.zeros((6, 6), F)
    k = 2
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = F(s[k]); k += 1
    nb = np.array([-F(s[k + a]) for a in range(6)], F)
    x = orc.ldlt6_solve(A.reshape(36), nb)
    D = np.eye(4, dtype=F)
    D[:3, :3] = orc.euler_xyz_matrix(x[0], x[1], x[2])
    D[:3, 3] = x[3:6]
    return mul44(D, np.asarray(T, F))


def odometry(orc, raw_src, raw_tgt, intr, T0=None, **kw):
    """tdv_depth_odometry: dict(T, fitness, rmse, n_corr, iterations, n_corr_level)."""
    p = params(**kw)
    T = np.eye(4, dtype=F) if T0 is None else np.array(T0, F)
    res = dict(T=T, fitness=F(0), rmse=F(0), n_corr=0, iterations=[0] * MAX_LEVELS, n_corr_level=[0] * MAX_LEVELS)
    raw_src, raw_tgt = np.asarray(raw_src, np.uint16), np.asarray(raw_tgt, np.uint16)
    if raw_src.size == 0:
        return res
    ps, pt = pyramid(raw_src, intr, p), pyramid(raw_tgt, intr, p)
    for l in range(p["n_levels"] - 1, -1, -1):
        prev_rmse = F(0)
        for it in range(p["max_iterations"][l]):
            s = sums(ps[l], pt[l], T, p)
            n_corr = int(s[0] + 0.5)
            if n_corr < 3:
                break
            T = step(orc, s, T)
            with np.errstate(**QUIET):
                rmse = np.sqrt(F(s[1]) / F(n_corr))
                fitness = F(n_corr) / F(ps[l]["n_valid"])
                converged = bool(np.abs(prev_rmse - rmse) < F(1e-6))
            prev_rmse = rmse
            res.update(fitness=fitness, rmse=rmse, n_corr=n_corr)
            res["iterations"][l] = it + 1
            res["n_corr_level"][l] = n_corr
            if it > 0 and converged:
                break
    res["T"] = T
    return res


def chain(Ts):
    """O9: P_0 = I, P_k = P_(k-1) T_k, each entry the float64 sum of four float64 products in index order, rounded once."""
    P = [np.eye(4, dtype=F)]
    for T in Ts:
        A, B = P[-1].astype(np.float64), np.asarray(T, F).astype(np.float64)
        C = np.zeros((4, 4), F)
        for i in range(4):
            for j in range(4):
                acc = A[i, 0] * B[0, j]
                for k in range(1, 4):
                    acc = acc + A[i, k] * B[k, j]
                C[i, j] = F(acc)
        P.append(C)
    return np.stack(P)


def sequence(orc, frames, intr, init=None, **kw):
    """tdv_depth_odometry_sequence_dev: (poses [n, 4, 4], the pairs' results with entry 0 zeros)."""
    frames = np.asarray(frames, np.uint16)
    n = len(frames)
    zero = dict(T=np.zeros((4, 4), F), fitness=F(0), rmse=F(0), n_corr=0, iterations=[0] * MAX_LEVELS, n_corr_level=[0] * MAX_LEVELS)
    if n == 0:
        return np.zeros((0, 4, 4), F), []
    pairs = [zero] + [odometry(orc, frames[k], frames[k - 1], intr, None if init is None else init[k], **kw) for k in range(1, n)]
    return chain([r["T"] for r in pairs[1:]]), pairs
