"""TSDF fusion as include/tdv_hip.h (tdv_tsdf_integrate_dev) states it, rules T1 to T8, in numpy f32 with one rounding per operation.
A volume is an array [nz, ny, nx, 2] of (tsdf, weight) - the buffer's public layout, voxel (i, j, k) at pair (k*ny + j)*nx + i.  The
frames of a call are applied one after the other over the whole grid, which is each voxel's ascending frame order; the crossings come
out of np.nonzero over [nz, ny, nx, 3], which is ascending 3*voxel_index + axis.  It knows nothing of tiles, runs or waves.
tests/test_tsdf_abi.py holds it to what the rules promise; tests/test_gpu_tsdf.py holds the device to it byte for byte."""
import numpy as np

F = np.float32
SOURCE_ONTO_TARGET, MODEL_TO_CAMERA = 0, 1
MAX_SIDE = 1024
MAX_VOXELS = 1 << 27
HOST_MAX_VOXELS = 1 << 25
MAX_FRAMES = 64
FRAME_MAX_SIDE = 8192                      # TDV_VERIFY_MAX_SIDE
TILE = (64, 8, 8)
DEFAULTS = dict(trunc=0.0, max_weight=255.0, zmax=10.0, min_weight=1.0, pose_direction=MODEL_TO_CAMERA)


class Volume:
    """origin (the grid's corner), voxel_length, dims = (nx, ny, nz)."""

    def __init__(self, origin, voxel_length, dims):
        self.origin = np.asarray(origin, F).reshape(3)
        self.L = F(voxel_length)
        self.nx, self.ny, self.nz = (int(d) for d in dims)

    @property
    def dims(self):
        return self.nx, self.ny, self.nz

    @property
    def voxels(self):
        return self.nx * self.ny * self.nz

    def centres(self):
        """T1: (xw[nx], yw[ny], zw[nz])."""
        out = tuple(self.origin[a] + (np.arange(n).astype(F) + F(0.5)) * self.L for a, n in enumerate(self.dims))
        assert all(c.dtype == F for c in out)
        return out

    def args(self):
        """What Context.tsdf_volume and tsdf_volume_struct take."""
        return self.origin, self.L, self.dims


def reset(vol):
    buf = np.zeros((vol.nz, vol.ny, vol.nx, 2), F)
    buf[..., 0] = 1
    return buf


def trunc_of(vol, trunc):
    return F(4.0) * vol.L if F(trunc) == 0 else F(trunc)


def camera(T, pose_direction, m0, m1, m2):
    """T2 = rule 1 of tdv_verify_poses.  T: [4, 4] row-major."""
    t = np.ascontiguousarray(np.asarray(T, F).reshape(4, 4).T).reshape(16)          # column-major, as the ABI takes it
    if pose_direction == SOURCE_ONTO_TARGET:
        d0, d1, d2 = m0 - t[12], m1 - t[13], m2 - t[14]
        xc = (t[0] * d0 + t[1] * d1) + t[2] * d2
        yc = (t[4] * d0 + t[5] * d1) + t[6] * d2
        zc = (t[8] * d0 + t[9] * d1) + t[10] * d2
    else:
        xc = ((t[0] * m0 + t[4] * m1) + t[8] * m2) + t[12]
        yc = ((t[1] * m0 + t[5] * m1) + t[9] * m2) + t[13]
        zc = ((t[2] * m0 + t[6] * m1) + t[10] * m2) + t[14]
    assert xc.dtype == F and yc.dtype == F and zc.dtype == F
    return xc, yc, zc


def integrate(vol, buf, frames, poses, intrinsics, trunc=0.0, max_weight=255.0, zmax=10.0, min_weight=1.0, pose_direction=MODEL_TO_CAMERA):
    """T1 to T5 for the frames (uint16 [n, h, w]) at poses ([n, 4, 4] row-major), intrinsics = (scale, fx, fy, cx, cy): (the new volume,
    int64[n] voxels updated per frame).  buf is not modified."""
    frames = np.asarray(frames, np.uint16)
    frames = frames.reshape((-1,) + frames.shape[-2:])
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    assert len(poses) == len(frames)
    scale, fx, fy, cx, cy = (F(x) for x in intrinsics)
    inv_scale = F(1.0 / float(scale))
    tr, max_weight, zmax = trunc_of(vol, trunc), F(max_weight), F(zmax)
    h, w = frames.shape[1:]
    xw, yw, zw = vol.centres()
    m0, m1, m2 = np.broadcast_arrays(xw[None, None, :], yw[None, :, None], zw[:, None, None])
    f, wt = buf[..., 0].copy(), buf[..., 1].copy()
    counts = np.zeros(len(frames), np.int64)
    with np.errstate(all="ignore"):
        for n, (raw, T) in enumerate(zip(frames, poses)):
            xc, yc, zc = camera(T, pose_direction, m0, m1, m2)
            ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > 0) & (zc <= zmax)              # T3
            uf = (xc * fx) / zc + cx
            vf = (yc * fy) / zc + cy
            assert uf.dtype == F and vf.dtype == F
            ok &= np.isfinite(uf) & np.isfinite(vf) & (np.abs(uf) < F(1 << 20)) & (np.abs(vf) < F(1 << 20))
            u = np.floor(np.where(ok, uf, F(0)) + F(0.5)).astype(np.int64)
            v = np.floor(np.where(ok, vf, F(0)) + F(0.5)).astype(np.int64)
            ok &= (u >= 0) & (u < w) & (v >= 0) & (v < h)
            r = raw[np.where(ok, v, 0), np.where(ok, u, 0)] if h * w else np.zeros(u.shape, np.uint16)
            zo = r.astype(F) * inv_scale                                                                    # T4
            ok &= (r != 0) & (zo <= zmax)
            sdf = zo - zc                                                                                   # T5
            ok &= ~(sdf < -tr)
            t = np.minimum(F(1.0), sdf / tr)
            nf = (f * wt + t) / (wt + F(1.0))
            nw = np.minimum(wt + F(1.0), max_weight)
            assert nf.dtype == F and nw.dtype == F
            f, wt = np.where(ok, nf, f), np.where(ok, nw, wt)
            counts[n] = int(ok.sum())
    return np.stack([f, wt], -1), counts


def _shift(a, axis, by, fill):
    """a moved so that out[.., i, ..] = a[.., i + by, ..] along `axis`, `fill` where that leaves the array."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(by) < n:
        src = [slice(None)] * a.ndim
        dst = [slice(None)] * a.ndim
        src[axis] = slice(max(by, 0), n + min(by, 0))
        dst[axis] = slice(max(-by, 0), n - max(by, 0))
        out[tuple(dst)] = a[tuple(src)]
    return out


AXIS_OF = (2, 1, 0)                        # the array axis of x, y, z


def gradient(f, obs):
    """T8's gradient of every voxel: [nz, ny, nx, 3]."""
    g = []
    for ax in range(3):
        A = AXIS_OF[ax]
        of, ob = _shift(obs, A, 1, False), _shift(obs, A, -1, False)
        d = np.where(of, _shift(f, A, 1, F(0)), f) - np.where(ob, _shift(f, A, -1, F(0)), f)
        d = np.where(of != ob, d * F(2.0), d)
        g.append(np.where(of | ob, d, F(0)).astype(F))
    return np.stack(g, -1)


def extract(vol, buf, min_weight=1.0, **_):
    """T6 to T8: (xyz f32[n, 3], normals f32[n, 3], key int64[n] = 3*voxel_index + axis, ascending)."""
    f, wt = buf[..., 0], buf[..., 1]
    centre = vol.centres()
    with np.errstate(all="ignore"):
        obs = wt >= F(min_weight)                                                                           # T6
        G = gradient(f, obs)
        keys, points, normals = [], [], []
        step = (1, vol.nx, vol.nx * vol.ny)                                                                  # voxel index of the +axis neighbour
        ff, Gf = f.reshape(-1), G.reshape(-1, 3)
        for ax in range(3):
            A = AXIS_OF[ax]
            has = obs & _shift(obs, A, 1, False) & ((f < 0) != (_shift(f, A, 1, F(0)) < 0))                  # T7
            a = np.nonzero(has.reshape(-1))[0].astype(np.int64)
            b = a + step[ax]
            ijk = [a % vol.nx, (a // vol.nx) % vol.ny, a // (vol.nx * vol.ny)]
            ra, rb = np.abs(ff[a]), np.abs(ff[b])
            ca = centre[ax][ijk[ax]]
            cb = vol.origin[ax] + ((ijk[ax] + 1).astype(F) + F(0.5)) * vol.L
            p = np.stack([centre[d][ijk[d]] for d in range(3)], -1)
            p[:, ax] = (ca * rb + cb * ra) / (ra + rb)
            n = Gf[a] * rb[:, None] + Gf[b] * ra[:, None]                                                    # T8
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            assert p.dtype == F and n.dtype == F and length.dtype == F
            good = (length > 0) & np.isfinite(length)
            keys.append(3 * a + ax); points.append(p); normals.append(np.where(good[:, None], n / length[:, None], F(0)).astype(F))
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    return np.concatenate(points)[order], np.concatenate(normals)[order], key[order]


def fuse(vol, frames, poses, intrinsics, **params):
    """reset, integrate, extract: (xyz, normals)."""
    buf, _ = integrate(vol, reset(vol), frames, poses, intrinsics, **params)
    xyz, nrm, _ = extract(vol, buf, params.get("min_weight", 1.0))
    return xyz, nrm
