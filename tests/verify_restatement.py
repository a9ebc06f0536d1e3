"""Pose verification as include/tdv_hip.h (tdv_verify_poses) states it, in numpy f32 with one rounding per operation: the whole frame's
z-buffer by np.minimum.at on the u32 keys, then the classification.  It knows nothing of tiles or boxes.  tests/test_verify_abi.py holds
it to an independent per-pixel definition; tests/test_gpu_verify.py holds the device to it byte for byte."""
import numpy as np

F = np.float32
SOURCE_ONTO_TARGET, MODEL_TO_CAMERA = 0, 1
MAX_SPLAT = 3
MAX_MODEL = 1 << 22
MAX_POSES = 65536
MAX_SIDE = 8192
TILE_W, TILE_H = 128, 128
LANES = 1024
EMPTY = np.uint32(0xFFFFFFFF)
DEFAULTS = dict(pose_direction=SOURCE_ONTO_TARGET, splat=1, tau=0.002, zmax=10.0)
RESULT = ("n_projected", "n_rendered", "n_consistent", "n_occluded", "n_violating", "n_unknown", "err_q20")


def project(model, T, fx, fy, cx, cy, pose_direction, zmax):
    """Rules 1 to 3: (usable bool[n], u int64[n], v int64[n], zc f32[n]); u, v are 0 where the point is unusable.  T: [4, 4] row-major."""
    m = np.ascontiguousarray(model, F).reshape(-1, 3)
    t = np.ascontiguousarray(np.asarray(T, F).reshape(4, 4).T).reshape(16)          # column-major, as the ABI takes it
    m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
    fx, fy, cx, cy, zmax = F(fx), F(fy), F(cx), F(cy), F(zmax)
    with np.errstate(all="ignore"):
        if pose_direction == SOURCE_ONTO_TARGET:
            d0, d1, d2 = m0 - t[12], m1 - t[13], m2 - t[14]
            xc = (t[0] * d0 + t[1] * d1) + t[2] * d2
            yc = (t[4] * d0 + t[5] * d1) + t[6] * d2
            zc = (t[8] * d0 + t[9] * d1) + t[10] * d2
        else:
            xc = ((t[0] * m0 + t[4] * m1) + t[8] * m2) + t[12]
            yc = ((t[1] * m0 + t[5] * m1) + t[9] * m2) + t[13]
            zc = ((t[2] * m0 + t[6] * m1) + t[10] * m2) + t[14]
        assert xc.dtype == F and zc.dtype == F
        usable = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > 0) & (zc <= zmax)
        uf = (xc * fx) / zc + cx
        vf = (yc * fy) / zc + cy
        assert uf.dtype == F
        usable &= np.isfinite(uf) & np.isfinite(vf) & (np.abs(uf) < F(1 << 20)) & (np.abs(vf) < F(1 << 20))
        u = np.floor(np.where(usable, uf, F(0)) + F(0.5)).astype(np.int64)
        v = np.floor(np.where(usable, vf, F(0)) + F(0.5)).astype(np.int64)
    return usable, u, v, zc


def render_keys(model, T, w, h, fx, fy, cx, cy, pose_direction=SOURCE_ONTO_TARGET, splat=1, zmax=10.0):
    """Rule 4: (the u32 keys of the frame [h, w], EMPTY where nothing rendered; n_projected)."""
    usable, u, v, zc = project(model, T, fx, fy, cx, cy, pose_direction, zmax)
    keys = np.full(h * w, EMPTY, np.uint32)
    bits = zc.view(np.uint32)
    for dy in range(-splat, splat + 1):
        for dx in range(-splat, splat + 1):
            x, y = u + dx, v + dy
            hit = usable & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            np.minimum.at(keys, (y * w + x)[hit], bits[hit])
    return keys.reshape(h, w), int(usable.sum())


def depth_of(keys):
    return np.where(keys != EMPTY, keys.view(F), F(0)).astype(F)


def observed(raw, scale, zmax):
    """Rule 5: (zo f32, valid)."""
    raw = np.asarray(raw, np.uint16)
    zo = raw.astype(F) * F(1.0 / float(F(scale)))
    assert zo.dtype == F
    return zo, (raw != 0) & (zo <= F(zmax))


def classify(keys, raw, scale, tau, zmax):
    """Rules 6 and 7 on a frame's keys: the six counts after n_projected and err_q20."""
    tau = F(tau)
    zo, valid = observed(raw, scale, zmax)
    rendered = keys != EMPTY
    with np.errstate(all="ignore"):
        diff = zo - keys.view(F)
        ad = np.abs(diff)
        cons = rendered & valid & (ad <= tau)
        occ = rendered & valid & (diff < -tau)
        vio = rendered & valid & (diff > tau)
        q = (ad * F(1048576.0))[cons]
        assert q.dtype == F
    q32 = [0xFFFFFFFF if x >= 4294967296.0 else int(x) for x in q.astype(np.float64)]
    return dict(n_rendered=int(rendered.sum()), n_consistent=int(cons.sum()), n_occluded=int(occ.sum()), n_violating=int(vio.sum()),
                n_unknown=int((rendered & ~valid).sum()), err_q20=int(sum(q32)))


def order_of(results):
    """The pose indices by n_consistent - n_violating descending, ties to the lower index."""
    score = np.array([r["n_consistent"] - r["n_violating"] for r in results], np.int64)
    return np.argsort(-score, kind="stable").astype(np.int32)


def verify(model, poses, raw, scale, fx, fy, cx, cy, pose_direction=SOURCE_ONTO_TARGET, splat=1, tau=0.002, zmax=10.0):
    """(one result dict per pose, order, the f32 depth image of every pose).  poses: [n, 4, 4] row-major."""
    raw = np.asarray(raw, np.uint16)
    h, w = raw.shape
    results, depths = [], []
    for T in np.asarray(poses, F).reshape(-1, 4, 4):
        keys, n_projected = render_keys(model, T, w, h, fx, fy, cx, cy, pose_direction, splat, zmax)
        results.append(dict(n_projected=n_projected, **classify(keys, raw, scale, tau, zmax)))
        depths.append(depth_of(keys))
    return results, order_of(results), depths
