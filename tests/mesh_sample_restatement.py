"""Mesh sampling as include/tdv_hip.h (tdv_mesh_sample_points, rules S1 to S7) states it, in numpy: f32 arrays so that every operation
rounds once, the weights and prefix sums in uint64, the high product of S4 in Python integers.  tests/test_mesh_sample_abi.py holds it to
independent definitions; tests/test_gpu_mesh_sample.py holds the device to it byte for byte."""
import math

import numpy as np

from fgr_restatement import philox4x32

F = np.float32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
MAX_VERTICES = 1 << 22
MAX_TRIANGLES = 1 << 22
SAMPLE_MAX = 1 << 24
KEY_TAG = 2                                                                        # S4: Philox key word 1
ONE = 1 << 24                                                                      # S5
DEFAULTS = dict(seed=0, first_sample=0)
RESULT = ("n_usable", "n_degenerate", "n_bad", "n_sampled", "weight_exponent", "area_max", "total_weight")
OUTPUTS = ("xyz", "normals", "triangle", "bary", "attr")


def faces(vertices, triangles):
    """S1 and S2 per triangle: dict(bad bool[m], area f32[m] (0 where bad), n f32[m, 3], L f32[m], va, vb, vc f32[m, 3], tri int64[m, 3])."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    in_range = ((t >= 0) & (t < len(v))).all(1)
    ts = np.where(in_range[:, None], t, 0)
    vv = v if len(v) else np.zeros((1, 3), F)                                      # (no vertex: every triangle is out of range)
    va, vb, vc = vv[ts[:, 0]], vv[ts[:, 1]], vv[ts[:, 2]]
    finite = np.isfinite(va).all(1) & np.isfinite(vb).all(1) & np.isfinite(vc).all(1)
    with np.errstate(all="ignore"):
        e1, e2 = vb - va, vc - va
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        area = F(0.5) * L
    assert n.dtype == F and L.dtype == F and area.dtype == F
    bad = ~in_range | ~finite | ~np.isfinite(area)
    return dict(bad=bad, area=np.where(bad, F(0), area), n=n, L=L, va=va, vb=vb, vc=vc, tri=ts)


def weights(area, bad):
    """S3: (w uint64[m], e, area_max f32)."""
    ok = ~bad
    area_max = F(area[ok].max()) if ok.any() else F(0)
    if area_max == 0:
        return np.zeros(len(area), U64), 0, F(0)
    e = int((np.float64(area_max).view(U64) >> U64(52)) & U64(0x7FF)) - 1023
    w = np.where(ok, np.ldexp(area.astype(np.float64), 31 - e), 0.0)              # a power of two: exact
    assert w.max() < 2.0 ** 32 and w.max() >= 2.0 ** 31
    return np.floor(w).astype(U64), e, area_max


def draws(g, seed):
    """S4, S5 for global indices g (uint64 array): (r = (x0 << 32) | x1 as Python integers, i1, i2 int64 after the reflection)."""
    g = np.asarray(g, U64)
    z = np.zeros_like(g)
    x = philox4x32((g & M32, g >> U64(32), z, z), (seed, KEY_TAG))
    r = [(int(a) << 32) | int(b) for a, b in zip(x[0], x[1])]
    return (r,) + reflect((x[2] >> U64(8)).astype(np.int64), (x[3] >> U64(8)).astype(np.int64))


def reflect(i1, i2):
    """S5: the 24-bit integers, both mirrored where their sum exceeds 2^24."""
    i1, i2 = np.asarray(i1, np.int64), np.asarray(i2, np.int64)
    over = i1 + i2 > ONE
    return np.where(over, ONE - i1, i1), np.where(over, ONE - i2, i2)


def bary(i1, i2):
    """S5: (u, v, w) in f32 from the integers."""
    s = F(2.0 ** -24)
    return i1.astype(F) * s, i2.astype(F) * s, (ONE - i1 - i2).astype(F) * s


def mix(w, u, v, a, b, c):
    """S6: (w*a + u*b) + v*c per column, f32."""
    with np.errstate(all="ignore"):
        out = (w[:, None] * a + u[:, None] * b) + v[:, None] * c
    assert out.dtype == F
    return out


def surface_area(total_weight, e):
    return math.ldexp(float(total_weight), e - 31)


def sample(vertices, triangles, n_samples, attr=None, seed=0, first_sample=0):
    """Every output of tdv_mesh_sample_points: the result's fields, surface_area, C (the prefix sums), and the rows."""
    f = faces(vertices, triangles)
    m = len(f["bad"])
    if m == 0:
        res = dict.fromkeys(RESULT, 0)
        res["area_max"] = F(0)
        w, C = np.zeros(0, U64), np.zeros(0, U64)
    else:
        w, e, area_max = weights(f["area"], f["bad"])
        C = np.cumsum(w, dtype=U64)
        res = dict(n_usable=int((w > 0).sum()), n_degenerate=int((~f["bad"] & (w == 0)).sum()), n_bad=int(f["bad"].sum()), n_sampled=0,
                   weight_exponent=e, area_max=area_max, total_weight=int(C[-1]))
    W = res["total_weight"]
    k = int(n_samples) if W > 0 else 0
    res["n_sampled"] = k
    width = 0 if attr is None else np.asarray(attr).shape[1]
    out = dict(res, surface_area=surface_area(W, res["weight_exponent"]), C=C, w=w)
    if k == 0:
        return dict(out, xyz=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), triangle=np.zeros(0, np.int32), bary=np.zeros((0, 2), F),
                    attr=None if attr is None else np.zeros((0, width), F))
    g = (np.arange(k, dtype=U64) + U64(first_sample & 0xFFFFFFFFFFFFFFFF))
    r, i1, i2 = draws(g, seed)
    target = np.array([(x * W) >> 64 for x in r], U64)
    t = np.searchsorted(C, target, side="right")                                   # the smallest t with C_t > target
    u, v, ww = bary(i1, i2)
    A = None
    if attr is not None:
        a = np.ascontiguousarray(attr, F)
        A = mix(ww, u, v, a[f["tri"][t, 0]], a[f["tri"][t, 1]], a[f["tri"][t, 2]])
    with np.errstate(all="ignore"):
        normals = f["n"][t] / f["L"][t][:, None]
    return dict(out, xyz=mix(ww, u, v, f["va"][t], f["vb"][t], f["vc"][t]), normals=normals, triangle=t.astype(np.int32),
                bary=np.stack([u, v], 1), attr=A)


def mesh_model(vertices, triangles, n_points, oversample=8, seed=0):
    """Context.mesh_model: oversample * n_points samples thinned by farthest point sampling from row 0, the normals beside."""
    import fps_restatement
    s = sample(vertices, triangles, oversample * n_points, seed=seed)
    r = fps_restatement.fps(s["xyz"], n_points, 0, s["normals"])
    return r["xyz"], r["attr"], r
