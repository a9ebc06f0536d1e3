"""TSDF ray casting and frame-to-model tracking as include/tdv_hip.h (tdv_tsdf_raycast_dev) states them - rules T13 to T18, O10, K1 to K3 -
in numpy f32 with one rounding per operation in the order written.  The rules are vectorised over the pixels with a loop over a ray's
samples; a volume is tests/tsdf_restatement.py's array [nz, ny, nx, 2], poses are row-major [4, 4], a camera is (fx, fy, cx, cy) and
intrinsics are (scale, fx, fy, cx, cy).  Tracking is composed from tests/odometry_restatement.py's downsample / normal_map / sums / step
(the target's level 0 by O10) and tests/tsdf_restatement.py's integrate.  It knows nothing of tiles, waves or csrc/tsdf_raycast.hip.

One shortcut, stated because it is not in the rules: a ray whose z does not advance (z + stride == z) repeats its sample for ever, so it
can only end at the step cap without a hit, and the loop drops it at once instead of walking to the cap."""
import numpy as np

import odometry_restatement as Od
import tsdf_restatement as Ts

F = np.float32
MAX_STEPS_CAP = 16384
DEFAULTS = dict(zmin=0.05, max_steps=4096)
QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def colmajor(T):
    return np.ascontiguousarray(np.asarray(T, F).reshape(4, 4).T).reshape(16)


def point(u, v, z, cam, t, direction):
    """T13: the volume-frame point of the pixels (u, v) at the depths z under the column-major pose t."""
    c0, c1, c2 = Od.vertex(u, v, z, tuple(F(x) for x in cam))
    if direction == Ts.SOURCE_ONTO_TARGET:
        p0 = ((t[0] * c0 + t[4] * c1) + t[8] * c2) + t[12]
        p1 = ((t[1] * c0 + t[5] * c1) + t[9] * c2) + t[13]
        p2 = ((t[2] * c0 + t[6] * c1) + t[10] * c2) + t[14]
    else:
        d0, d1, d2 = c0 - t[12], c1 - t[13], c2 - t[14]
        p0 = (t[0] * d0 + t[1] * d1) + t[2] * d2
        p1 = (t[4] * d0 + t[5] * d1) + t[6] * d2
        p2 = (t[8] * d0 + t[9] * d1) + t[10] * d2
    assert p0.dtype == F and p1.dtype == F and p2.dtype == F
    return p0, p1, p2


def lerp(a, b, t):
    return a + t * (b - a)


def sample(vol, buf, min_weight, p):
    """T14: (known bool[n], F f32[n]) at the points p = (p0, p1, p2); F is 0 where unknown."""
    n = len(p[0])
    dims = vol.dims
    g = [(p[a] - vol.origin[a]) / vol.L - F(0.5) for a in range(3)]
    ok = np.ones(n, bool)
    for a in range(3):
        ok &= np.isfinite(g[a]) & (g[a] >= 0) & (g[a] < F(dims[a] - 1))
    fl = [np.floor(np.where(ok, g[a], F(0))).astype(F) for a in range(3)]
    t = [np.where(ok, g[a], F(0)) - fl[a] for a in range(3)]
    i, j, k = (x.astype(np.int64) for x in fl)
    f = {}
    obs = ok.copy()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                kk, jj, ii = np.where(ok, k + dz, 0), np.where(ok, j + dy, 0), np.where(ok, i + dx, 0)
                f[dx, dy, dz] = buf[kk, jj, ii, 0]
                obs &= buf[kk, jj, ii, 1] >= F(min_weight)                                                   # T6 (false for NaN)
    x = {(dy, dz): lerp(f[0, dy, dz], f[1, dy, dz], t[0]) for dy in (0, 1) for dz in (0, 1)}
    y = {dz: lerp(x[0, dz], x[1, dz], t[1]) for dz in (0, 1)}
    s = lerp(y[0], y[1], t[2])
    assert s.dtype == F
    known = obs & ~np.isnan(s)
    return known, np.where(known, s, F(0))


def raycast(vol, buf, pose, size, cam, trunc=0.0, zmax=10.0, min_weight=1.0, pose_direction=Ts.MODEL_TO_CAMERA, zmin=0.05, max_steps=4096,
            max_weight=255.0, normals=True):
    """tdv_tsdf_raycast_dev: dict(depth f32[h, w], vertex_map f32[h, w, 3], normal_map f32[h, w, 3], n_hit, samples int64[h, w] - the
    samples every ray took, capped bool[h, w] - it ended at the step cap, far bool[h, w] - it ended beyond zmax)."""
    w, h = size
    n = w * h
    t = colmajor(pose)
    cam = tuple(F(x) for x in cam)
    tr, zmax, L, zmin = Ts.trunc_of(vol, trunc), F(zmax), vol.L, F(zmin)
    vv, uu = np.mgrid[0:h, 0:w]
    uu, vv = uu.reshape(-1), vv.reshape(-1)
    z = np.full(n, zmin, F)
    zp, sp = np.zeros(n, F), np.zeros(n, F)
    prev = np.zeros(n, bool)
    active = np.ones(n, bool)
    depth = np.zeros(n, F)
    samples = np.zeros(n, np.int64)
    far, capped = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(**QUIET):
        for _ in range(int(max_steps)):                                                                      # T15
            beyond = active & ~(z <= zmax)
            far |= beyond
            active &= ~beyond
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                break
            samples[idx] += 1
            zi = z[idx]
            known, s = sample(vol, buf, min_weight, point(uu[idx], vv[idx], zi, cam, t, pose_direction))
            end = known & (s < 0)
            hit = end & prev[idx]
            zh = np.fmin(zp[idx] + ((zi - zp[idx]) * sp[idx]) / (sp[idx] - s), zi)                           # T16
            assert zh.dtype == F
            depth[idx[hit]] = zh[hit]
            active[idx[end]] = False
            go = ~end
            ii = idx[go]
            zp[ii], sp[ii], prev[ii] = zi[go], s[go], known[go]
            nz = zi[go] + np.where(known[go], np.fmax(s[go] * tr, L), tr)
            assert nz.dtype == F
            stalled = nz == zi[go]                                                                           # the module docstring's shortcut
            samples[ii[stalled]] = max_steps
            capped[ii[stalled]] = True
            active[ii[stalled]] = False
            z[ii] = nz
    with np.errstate(**QUIET):
        far |= active & ~(z <= zmax)
    capped |= active & ~far                                                                                  # k == max_steps
    hitm = depth != 0
    hi = np.nonzero(hitm)[0]
    vm, nm = np.zeros((n, 3), F), np.zeros((n, 3), F)
    with np.errstate(**QUIET):
        x, y, zz = Od.vertex(uu[hi], vv[hi], depth[hi], cam)                                                 # T17
        vm[hi] = np.stack([x, y, zz], -1)
        if normals and len(hi):                                                                              # T18
            p = point(uu[hi], vv[hi], depth[hi], cam, t, pose_direction)
            G, all_known = [], np.ones(len(hi), bool)
            for a in range(3):
                q = list(p)
                q[a] = p[a] + L
                kf, sf = sample(vol, buf, min_weight, q)
                q[a] = p[a] - L
                kb, sb = sample(vol, buf, min_weight, q)
                all_known &= kf & kb
                G.append(sf - sb)
            if pose_direction == Ts.SOURCE_ONTO_TARGET:
                n0 = (t[0] * G[0] + t[1] * G[1]) + t[2] * G[2]
                n1 = (t[4] * G[0] + t[5] * G[1]) + t[6] * G[2]
                n2 = (t[8] * G[0] + t[9] * G[1]) + t[10] * G[2]
            else:
                n0 = (t[0] * G[0] + t[4] * G[1]) + t[8] * G[2]
                n1 = (t[1] * G[0] + t[5] * G[1]) + t[9] * G[2]
                n2 = (t[2] * G[0] + t[6] * G[1]) + t[10] * G[2]
            length = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            assert length.dtype == F
            good = all_known & (length > 0) & np.isfinite(length)
            nm[hi] = np.where(good[:, None], np.stack([n0 / length, n1 / length, n2 / length], -1), F(0))
    return dict(depth=depth.reshape(h, w), vertex_map=vm.reshape(h, w, 3), normal_map=nm.reshape(h, w, 3), n_hit=int(hitm.sum()),
                samples=samples.reshape(h, w), capped=capped.reshape(h, w), far=far.reshape(h, w))


# ------------------------------------------------------------------------------------------------ O10 and the odometry against it
def depth0_f32(d, zmax):
    """O10: the target's level 0 from an f32 depth image."""
    d = np.asarray(d, F)
    with np.errstate(**QUIET):
        return np.where(~np.isnan(d) & (d > 0) & (d <= F(zmax)), d, F(0)).astype(F)


def pyramid_f32(d, intr, p):
    """Od.pyramid with level 0 by O10."""
    _, fx, fy, cx, cy = intr
    z = depth0_f32(d, p["zmax"])
    out = []
    for l in range(p["n_levels"]):
        if l:
            z = Od.downsample(z, p["depth_diff"])
        cam = Od.level_intrinsics(fx, fy, cx, cy, l)
        out.append(dict(z=z, normals=Od.normal_map(z, cam, p["depth_diff"]), cam=cam, n_valid=int((z > 0).sum())))
    return out


def odometry_to_depth(orc, raw_src, depth_tgt, intr, T0=None, **kw):
    """tdv_depth_odometry_to_depth: Od.odometry's loop (O8) with the target's pyramid from the f32 image."""
    p = Od.params(**kw)
    T = np.eye(4, dtype=F) if T0 is None else np.array(T0, F)
    res = dict(T=T, fitness=F(0), rmse=F(0), n_corr=0, iterations=[0] * Od.MAX_LEVELS, n_corr_level=[0] * Od.MAX_LEVELS)
    raw_src = np.asarray(raw_src, np.uint16)
    if raw_src.size == 0:
        return res
    ps, pt = Od.pyramid(raw_src, intr, p), pyramid_f32(depth_tgt, intr, p)
    for l in range(p["n_levels"] - 1, -1, -1):
        prev_rmse = F(0)
        for it in range(p["max_iterations"][l]):
            s = Od.sums(ps[l], pt[l], T, p)
            n_corr = int(s[0] + 0.5)
            if n_corr < 3:
                break
            T = Od.step(orc, s, T)
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


# ------------------------------------------------------------------------------------------------ K1 to K3
def product(A, B):
    """O9's product of two poses: each entry the float64 sum of four float64 products in index order, rounded once."""
    A, B = np.asarray(A, F).astype(np.float64), np.asarray(B, F).astype(np.float64)
    C = np.zeros((4, 4), F)
    for i in range(4):
        for j in range(4):
            acc = A[i, 0] * B[0, j]
            for k in range(1, 4):
                acc = acc + A[i, k] * B[k, j]
            C[i, j] = F(acc)
    return C


def _tsdf(tsdf):
    return dict(dict(pose_direction=Ts.SOURCE_ONTO_TARGET), **(tsdf or {}))


def track(orc, vol, buf, raw, guess, intr, tsdf=None, ray=None, odom=None):
    """tdv_tsdf_track_dev: dict(pose, odom, n_hit, depth - K1's image)."""
    tsdf = _tsdf(tsdf)
    assert tsdf["pose_direction"] == Ts.SOURCE_ONTO_TARGET
    raw = np.asarray(raw, np.uint16)
    h, w = raw.shape
    guess = np.asarray(guess, F).reshape(4, 4)
    if raw.size == 0:
        o = odometry_to_depth(orc, raw, np.zeros((h, w), F), intr, **(odom or {}))
        return dict(pose=product(guess, o["T"]), odom=o, n_hit=0, depth=np.zeros((h, w), F))
    cast = raycast(vol, buf, guess, (w, h), intr[1:], normals=False, **dict(tsdf, **(ray or {})))                 # K1
    o = odometry_to_depth(orc, raw, cast["depth"], intr, **(odom or {}))                                       # K2
    return dict(pose=product(guess, o["T"]), odom=o, n_hit=cast["n_hit"], depth=cast["depth"])                 # K3


def track_sequence(orc, vol, buf, frames, intr, pose0=None, tsdf=None, ray=None, odom=None):
    """tdv_tsdf_track_sequence_dev: (poses [n, 4, 4], the frames' results, the volume at the end).  buf is not modified."""
    frames = np.asarray(frames, np.uint16)
    n = len(frames)
    if n == 0:
        return np.zeros((0, 4, 4), F), [], buf
    P = [np.eye(4, dtype=F) if pose0 is None else np.array(pose0, F).reshape(4, 4)]
    zero = dict(T=np.zeros((4, 4), F), fitness=F(0), rmse=F(0), n_corr=0, iterations=[0] * Od.MAX_LEVELS, n_corr_level=[0] * Od.MAX_LEVELS)
    results = [dict(pose=P[0], odom=zero, n_hit=0)]
    for k in range(n):
        if k:
            r = track(orc, vol, buf, frames[k], P[-1], intr, tsdf, ray, odom)
            P.append(r["pose"])
            results.append(r)
        buf, _ = Ts.integrate(vol, buf, frames[k:k + 1], P[-1][None], intr, **_tsdf(tsdf))
    return np.stack(P), results, buf
