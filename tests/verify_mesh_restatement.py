"""Pose verification from a triangle mesh as include/tdv_hip.h (tdv_verify_poses_mesh) states it, in numpy: rules M1 to M6 over the whole
frame - int64 edge functions, the f64 depth with one rounding per operation, the z-buffer by np.minimum.at on the u32 keys - then the
classification of tests/verify_restatement.py (rule M7: one statement of rules 5 to 7).  It knows nothing of tiles, queues or which
triangles are large.  tests/test_verify_mesh_abi.py holds it to an independent definition (point-in-triangle in fractions.Fraction, the
minimum over an explicit list); tests/test_gpu_verify_mesh.py holds the device to it byte for byte."""
import numpy as np

import verify_restatement as R

F = np.float32
SOURCE_ONTO_TARGET, MODEL_TO_CAMERA = R.SOURCE_ONTO_TARGET, R.MODEL_TO_CAMERA
CULL_NONE, CULL_BACK = 0, 1
MAX_VERTICES = 1 << 22
MAX_TRIANGLES = 1 << 22
SUBPIXEL = 16
COOP_PIXELS = 64
QUEUE = 128
EMPTY = R.EMPTY
DEFAULTS = dict(pose_direction=SOURCE_ONTO_TARGET, cull=CULL_NONE, tau=0.002, zmax=10.0)
RESULT = R.RESULT


def project(vertices, T, fx, fy, cx, cy, pose_direction, zmax):
    """Rule M1: (usable bool[n], X int64[n], Y int64[n], zc f32[n], uf f32[n], vf f32[n]); X, Y are 0 where the vertex is unusable."""
    m = np.ascontiguousarray(vertices, F).reshape(-1, 3)
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
        sx = np.where(usable, uf, F(0)) * F(SUBPIXEL) + F(0.5)
        sy = np.where(usable, vf, F(0)) * F(SUBPIXEL) + F(0.5)
        assert sx.dtype == F
    return usable, np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64), zc, uf, vf


def setup(vertices, triangles, T, fx, fy, cx, cy, pose_direction, cull, zmax):
    """Rules M2 and M3: the usable triangles after the swap, as a dict of arrays (X, Y int64 [n, 3], iz f64 [n, 3], A int64 [n] > 0, index:
    their rows in `triangles`)."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    usable, X, Y, zc, _, _ = project(vertices, T, fx, fy, cx, cy, pose_direction, zmax)
    nv = len(usable)
    ok = ((tri >= 0) & (tri < nv)).all(1)
    idx = np.where(ok[:, None], tri, 0)
    ok &= usable[idx].all(1) if nv else False
    Xt, Yt, zt = (X[idx], Y[idx], zc[idx]) if nv else (np.zeros((len(tri), 3), np.int64),) * 2 + (np.ones((len(tri), 3), F),)
    A = (Xt[:, 1] - Xt[:, 0]) * (Yt[:, 2] - Yt[:, 0]) - (Yt[:, 1] - Yt[:, 0]) * (Xt[:, 2] - Xt[:, 0])
    ok &= A != 0
    if cull == CULL_BACK:
        ok &= A < 0                                                                # A > 0: the normal points away from the camera
    swap = A < 0
    order = np.where(swap[:, None], [0, 2, 1], [0, 1, 2])
    Xt, Yt, zt = (np.take_along_axis(a, order, 1) for a in (Xt, Yt, zt))
    A = np.abs(A)
    keep = np.nonzero(ok)[0]
    with np.errstate(all="ignore"):
        iz = 1.0 / zt[keep].astype(np.float64)
    return dict(X=Xt[keep], Y=Yt[keep], iz=iz, A=A[keep], index=keep)


def _owns(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def raster(X, Y, iz, px, py):
    """Rules M4 and M5 at the pixel centres (px, py) (1/16 px; broadcast against the triangles' leading axes): (covered, zr f32)."""
    def edge(i, j):
        dx, dy = X[..., j] - X[..., i], Y[..., j] - Y[..., i]
        E = dx * (py - Y[..., i]) - dy * (px - X[..., i])
        return E, (E > 0) | ((E == 0) & _owns(dx, dy))
    (w0, c0), (w1, c1), (w2, c2) = edge(1, 2), edge(2, 0), edge(0, 1)
    A = w0 + w1 + w2
    with np.errstate(all="ignore"):
        s = (w0.astype(np.float64) * iz[..., 0] + w1.astype(np.float64) * iz[..., 1]) + w2.astype(np.float64) * iz[..., 2]
        zr = (A.astype(np.float64) / s).astype(F)
    return c0 & c1 & c2, zr


def render_keys(vertices, triangles, T, w, h, fx, fy, cx, cy, pose_direction=SOURCE_ONTO_TARGET, cull=CULL_NONE, zmax=10.0):
    """Rule M6: (the u32 keys of the frame [h, w], EMPTY where nothing rendered; n_projected = the usable triangles)."""
    s = setup(vertices, triangles, T, fx, fy, cx, cy, pose_direction, cull, zmax)
    keys = np.full(h * w, EMPTY, np.uint32)
    X, Y, iz = s["X"], s["Y"], s["iz"]
    n = len(X)
    if n and w > 0 and h > 0:
        # the pixel centres that can lie inside: ceil(min / 16) .. floor(max / 16), inside the frame (a speed-up, not a rule)
        x0, x1 = np.maximum(-(-X.min(1) // SUBPIXEL), 0), np.minimum(X.max(1) // SUBPIXEL, w - 1)
        y0, y1 = np.maximum(-(-Y.min(1) // SUBPIXEL), 0), np.minimum(Y.max(1) // SUBPIXEL, h - 1)
        some = (x0 <= x1) & (y0 <= y1)
        small = some & (x1 - x0 < 8) & (y1 - y0 < 8)
        k = np.nonzero(small)[0]                                                   # all small ones together, one pixel of each at a time
        if len(k):
            for dy in range(int((y1 - y0)[k].max()) + 1):
                for dx in range(int((x1 - x0)[k].max()) + 1):
                    x, y = x0[k] + dx, y0[k] + dy
                    cov, zr = raster(X[k], Y[k], iz[k], x * SUBPIXEL, y * SUBPIXEL)
                    hit = cov & (x <= x1[k]) & (y <= y1[k])
                    np.minimum.at(keys, (y * w + x)[hit], zr.view(np.uint32)[hit])
        for t in np.nonzero(some & ~small)[0]:                                     # a large one: all of its pixels at once
            y, x = np.mgrid[y0[t]:y1[t] + 1, x0[t]:x1[t] + 1]
            cov, zr = raster(X[t], Y[t], iz[t], x * SUBPIXEL, y * SUBPIXEL)
            np.minimum.at(keys, (y * w + x)[cov], zr.view(np.uint32)[cov])
    return keys.reshape(h, w), n


depth_of = R.depth_of
order_of = R.order_of


def verify(vertices, triangles, poses, raw, scale, fx, fy, cx, cy, pose_direction=SOURCE_ONTO_TARGET, cull=CULL_NONE, tau=0.002, zmax=10.0):
    """(one result dict per pose, order, the f32 depth image of every pose).  poses: [n, 4, 4] row-major."""
    raw = np.asarray(raw, np.uint16)
    h, w = raw.shape
    results, depths = [], []
    for T in np.asarray(poses, F).reshape(-1, 4, 4):
        keys, n_projected = render_keys(vertices, triangles, T, w, h, fx, fy, cx, cy, pose_direction, cull, zmax)
        results.append(dict(n_projected=n_projected, **R.classify(keys, raw, scale, tau, zmax)))
        depths.append(depth_of(keys))
    return results, order_of(results), depths
