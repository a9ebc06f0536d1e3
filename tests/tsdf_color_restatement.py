"""Coloured TSDF fusion as include/tdv_hip.h (tdv_tsdf_integrate_color_dev) states it, rules T19 to T24, in numpy f32 with one rounding per
operation in the order written, on top of tests/tsdf_restatement.py (T1 to T8) and tests/tsdf_raycast_restatement.py (T13 to T18), which
stay as they are.  A colour volume is an array [nz, ny, nx, 4] of (r, g, b, wc) - the buffer's public layout, voxel (i, j, k) at quad
(k*ny + j)*nx + i; images are uint8 [n, h, w, 3], B, G, R.  integrate() walks T1 to T5 itself, because it needs the pixel a voxel was
updated from, and asserts that the pair volume and the counts it gets are tsdf_restatement.integrate's.  It knows nothing of tiles, runs or
waves.  tests/test_tsdf_color_abi.py holds it to what the rules promise; tests/test_gpu_tsdf_color.py holds the device to it byte for byte."""
import numpy as np

import tsdf_raycast_restatement as Rc
import tsdf_restatement as R

F = np.float32
QUIET = Rc.QUIET


def reset(vol):
    """T19: every quad (0, 0, 0, 0)."""
    return np.zeros((vol.nz, vol.ny, vol.nx, 4), F)


def unit_colour(byte):
    """T20: a channel from its byte."""
    c = np.asarray(byte, np.uint8).astype(F) / F(255.0)
    assert c.dtype == F
    return c


def integrate(vol, buf, col, frames, images, poses, intrinsics, trunc=0.0, max_weight=255.0, zmax=10.0, min_weight=1.0,
              pose_direction=R.MODEL_TO_CAMERA):
    """T1 to T5 and T19 to T21: (the new pair volume, the new colour volume, int64[n] voxels updated per frame).  buf and col are not
    modified."""
    frames = np.asarray(frames, np.uint16)
    frames = frames.reshape((-1,) + frames.shape[-2:])
    images = np.asarray(images, np.uint8).reshape(frames.shape + (3,))
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    assert len(poses) == len(frames)
    scale, fx, fy, cx, cy = (F(x) for x in intrinsics)
    inv_scale = F(1.0 / float(scale))
    tr, max_weight, zmax = R.trunc_of(vol, trunc), F(max_weight), F(zmax)
    h, w = frames.shape[1:]
    xw, yw, zw = vol.centres()
    m0, m1, m2 = np.broadcast_arrays(xw[None, None, :], yw[None, :, None], zw[:, None, None])
    f, wt = buf[..., 0].copy(), buf[..., 1].copy()
    c, wc = [col[..., k].copy() for k in range(3)], col[..., 3].copy()
    counts = np.zeros(len(frames), np.int64)
    with np.errstate(all="ignore"):
        for n, (raw, bgr, T) in enumerate(zip(frames, images, poses)):
            xc, yc, zc = R.camera(T, pose_direction, m0, m1, m2)                                            # T2
            ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > 0) & (zc <= zmax)              # T3
            uf = (xc * fx) / zc + cx
            vf = (yc * fy) / zc + cy
            ok &= np.isfinite(uf) & np.isfinite(vf) & (np.abs(uf) < F(1 << 20)) & (np.abs(vf) < F(1 << 20))
            u = np.floor(np.where(ok, uf, F(0)) + F(0.5)).astype(np.int64)
            v = np.floor(np.where(ok, vf, F(0)) + F(0.5)).astype(np.int64)
            ok &= (u >= 0) & (u < w) & (v >= 0) & (v < h)
            u, v = np.where(ok, u, 0), np.where(ok, v, 0)
            r = raw[v, u] if h * w else np.zeros(u.shape, np.uint16)
            zo = r.astype(F) * inv_scale                                                                    # T4
            ok &= (r != 0) & (zo <= zmax)
            sdf = zo - zc                                                                                   # T5
            ok &= ~(sdf < -tr)
            t = np.minimum(F(1.0), sdf / tr)
            nf = (f * wt + t) / (wt + F(1.0))
            nw = np.minimum(wt + F(1.0), max_weight)
            f, wt = np.where(ok, nf, f), np.where(ok, nw, wt)
            px = bgr[v, u] if h * w else np.zeros(u.shape + (3,), np.uint8)                                 # T20: B, G, R
            for k in range(3):                                                                              # T21
                nc = (c[k] * wc + unit_colour(px[..., 2 - k])) / (wc + F(1.0))
                assert nc.dtype == F
                c[k] = np.where(ok, nc, c[k])
            wc = np.where(ok, np.minimum(wc + F(1.0), max_weight), wc)
            counts[n] = int(ok.sum())
    pair = np.stack([f, wt], -1)
    ref, ref_counts = R.integrate(vol, buf, frames, poses, intrinsics, trunc=trunc, max_weight=max_weight, zmax=zmax, min_weight=min_weight,
                                  pose_direction=pose_direction)
    assert pair.tobytes() == ref.tobytes() and np.array_equal(counts, ref_counts), "T21: the pair volume and the counts are the plain call's"
    return pair, np.stack(c + [wc], -1).astype(F), counts


def crossing_ends(vol, key):
    """The voxel indices (a, b) of the crossings with T7's keys."""
    a = key // 3
    return a, a + np.array([1, vol.nx, vol.nx * vol.ny], np.int64)[key % 3]


def crossing_classes(vol, buf, col, min_weight=1.0):
    """T23's class of every crossing: 2 both ends coloured, 1 exactly one, 0 neither."""
    key = R.extract(vol, buf, min_weight)[2]
    a, b = crossing_ends(vol, key)
    wc = col[..., 3].reshape(-1)
    return (wc[a] > 0).astype(np.int64) + (wc[b] > 0).astype(np.int64)


def extract(vol, buf, col, min_weight=1.0, **_):
    """T6 to T8 and T22, T23: (xyz, normals, key - tsdf_restatement.extract's own -, rgb f32[n, 3])."""
    xyz, nrm, key = R.extract(vol, buf, min_weight)
    a, b = crossing_ends(vol, key)
    f, q = buf[..., 0].reshape(-1), col.reshape(-1, 4)
    with np.errstate(**QUIET):
        ra, rb = np.abs(f[a]), np.abs(f[b])
        ca, cb = q[a, 3] > 0, q[b, 3] > 0                                                                   # T22
        rgb = np.zeros((len(key), 3), F)
        for k in range(3):
            both = (q[a, k] * rb + q[b, k] * ra) / (ra + rb)
            assert both.dtype == F
            rgb[:, k] = np.where(ca & cb, both, np.where(ca, q[a, k], np.where(cb, q[b, k], F(0))))
    return xyz, nrm, key, rgb


def colour_sample(vol, col, p):
    """T24 at the points p = (p0, p1, p2): f32[n, 3], zeros where T14's conditions on the grid coordinates fail or a voxel has no colour."""
    n = len(p[0])
    dims = vol.dims
    with np.errstate(**QUIET):
        g = [(p[a] - vol.origin[a]) / vol.L - F(0.5) for a in range(3)]
        ok = np.ones(n, bool)
        for a in range(3):
            ok &= np.isfinite(g[a]) & (g[a] >= 0) & (g[a] < F(dims[a] - 1))
        fl = [np.floor(np.where(ok, g[a], F(0))).astype(F) for a in range(3)]
        t = [np.where(ok, g[a], F(0)) - fl[a] for a in range(3)]
        i, j, k = (x.astype(np.int64) for x in fl)
        q, coloured = {}, ok.copy()
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    kk, jj, ii = np.where(ok, k + dz, 0), np.where(ok, j + dy, 0), np.where(ok, i + dx, 0)
                    q[dx, dy, dz] = col[kk, jj, ii]
                    coloured &= q[dx, dy, dz][:, 3] > 0                                                     # T22
        out = np.zeros((n, 3), F)
        for ch in range(3):
            x = {(dy, dz): Rc.lerp(q[0, dy, dz][:, ch], q[1, dy, dz][:, ch], t[0]) for dy in (0, 1) for dz in (0, 1)}
            y = {dz: Rc.lerp(x[0, dz], x[1, dz], t[1]) for dz in (0, 1)}
            s = Rc.lerp(y[0], y[1], t[2])
            assert s.dtype == F
            out[:, ch] = np.where(coloured, s, F(0))
    return out


def raycast(vol, buf, col, pose, size, cam, **params):
    """tdv_tsdf_raycast_color_dev: tsdf_raycast_restatement.raycast's dict with rgb_map f32[h, w, 3]."""
    out = Rc.raycast(vol, buf, pose, size, cam, **params)
    w, h = size
    depth = out["depth"].reshape(-1)
    hi = np.nonzero(depth != 0)[0]
    rgb = np.zeros((w * h, 3), F)
    if len(hi):
        with np.errstate(**QUIET):
            p = Rc.point(hi % w, hi // w, depth[hi], tuple(F(x) for x in cam), Rc.colmajor(pose), params.get("pose_direction", R.MODEL_TO_CAMERA))
        rgb[hi] = colour_sample(vol, col, p)
    out["rgb_map"] = rgb.reshape(h, w, 3)
    return out


def fuse(vol, frames, images, poses, intrinsics, **params):
    """reset, integrate, extract: (xyz, normals, rgb)."""
    buf, col, _ = integrate(vol, R.reset(vol), reset(vol), frames, images, poses, intrinsics, **params)
    xyz, nrm, _, rgb = extract(vol, buf, col, params.get("min_weight", 1.0))
    return xyz, nrm, rgb
