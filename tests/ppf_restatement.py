"""The rules of tdv_ppf_match (include/tdv_hip.h) in numpy - written from the header's text, not from the kernels.  f32 rules run on
float32 arrays (numpy rounds every operation once and never contracts), rule 7 in float64.  atan2f is the running libm's
(oracle.pyoracle.libm_f32_batch; tests/test_libm_restatement.py ties it to the device's restatement).  Everything is vectorised over
pairs; nothing here is shaped like the device code (no tiles, no scans, no atomics: a bincount per reference point)."""
import numpy as np

from oracle import pyoracle

F = np.float32
PI, TWO_PI = F(3.14159274), F(6.28318548)
PEAK = np.dtype([("ref", np.int32), ("model_index", np.int32), ("bin", np.int32), ("votes", np.int32)])
DEFAULTS = dict(distance_step_relative=0.05, angle_bins=30, rotation_bins=30, ref_stride=5, max_poses=8, cluster_translation_relative=0.1,
                cluster_rotation=float(F(2.0 * np.pi / 30.0)), flip_model_normals=0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def atan2f(y, x):
    y = np.asarray(y, F); x = np.asarray(x, F)
    return pyoracle.libm_f32_batch("atan2f", y, x).reshape(y.shape)


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def ang(u, v):
    c = cross(u, v)
    return atan2f(np.sqrt(dot(c, c)), dot(u, v))


def usable(p, n):
    """Rule 0."""
    with np.errstate(all="ignore"):
        nn = dot(n, n)
        return np.isfinite(p).all(1) & np.isfinite(n).all(1) & (nn > 0) & np.isfinite(nn)


def key_space(p):
    """Rule 1: (n_dist, n_keys)."""
    n_dist = int(np.floor(F(1.0) / F(p["distance_step_relative"]))) + 1
    return n_dist, n_dist * p["angle_bins"] ** 3


def diameter(tgt, p):
    """Rule 1: (diameter, distance_step), f32."""
    fin = tgt[np.isfinite(tgt).all(1)]
    if len(fin) == 0:
        return F(0), F(p["distance_step_relative"]) * F(0)
    e = fin.max(0) - fin.min(0)
    d = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return F(d), F(p["distance_step_relative"]) * F(d)


def pairs(pa, na, pb, nb, step, p):
    """Rules 2 and 3 for the ordered pairs (a, b) of usable points, row by row: (has a key, key, alpha)."""
    A = p["angle_bins"]
    n_dist, _ = key_space(p)
    with np.errstate(all="ignore"):
        d = pb - pa
        ln = np.sqrt(dot(d, d))
        ok = (ln > 0) & np.isfinite(ln)
        q0f = np.floor(ln / F(step))
        ok &= q0f < F(n_dist)
        f1, f2, f3 = ang(na, d), ang(nb, d), ang(na, nb)
        ok &= ~(np.isnan(f1) | np.isnan(f2) | np.isnan(f3))
        norm = np.sqrt(dot(na, na))
        u = na / norm[:, None]
        neg = na[:, 0] < 0
        w = np.where(neg[:, None], -u, u)
        k = F(1.0) + w[:, 0]
        ca, cb = w[:, 1] / k, w[:, 2] / k
        t = w[:, 1] * d[:, 1] + w[:, 2] * d[:, 2]
        y = (d[:, 1] - ca * t) - w[:, 1] * d[:, 0]
        z = (d[:, 2] - cb * t) - w[:, 2] * d[:, 0]
        z = np.where(neg, -z, z)
        alpha = atan2f(-z, y)
        ok &= ~np.isnan(alpha)
        astep = PI / F(A)
        q = [np.minimum(np.floor(np.where(ok, f, F(0)) / astep).astype(np.int64), A - 1) for f in (f1, f2, f3)]
        q0 = np.where(ok, q0f, F(0)).astype(np.int64)
    key = ((q0 * A + q[0]) * A + q[1]) * A + q[2]
    return ok, key, alpha


def model_table(tgt, tgt_normals, **kw):
    """Rules 1 and 4: dict(diameter, distance_step, n_pairs, n_keys, nt, offsets, pair, alpha_bits, key)."""
    p = params(**kw)
    tgt = np.asarray(tgt, F).reshape(-1, 3); tn = np.asarray(tgt_normals, F).reshape(-1, 3)
    if p["flip_model_normals"]:
        tn = -tn
    nt = len(tgt)
    _, n_keys = key_space(p)
    diam, step = diameter(tgt, p) if nt >= 2 else (F(0), F(0))
    pair = np.zeros(0, np.int64); key = np.zeros(0, np.int64); alpha = np.zeros(0, F)
    if nt >= 2:
        good = np.flatnonzero(usable(tgt, tn))
        I, J = np.meshgrid(good, good, indexing="ij")
        I, J = I.ravel(), J.ravel()
        I, J = I[I != J], J[I != J]
        ok, k, al = pairs(tgt[I], tn[I], tgt[J], tn[J], step, p)
        pair, key, alpha = (I * nt + J)[ok], k[ok], al[ok]
        o = np.lexsort((pair, key))
        pair, key, alpha = pair[o], key[o], alpha[o]
    offsets = np.searchsorted(key, np.arange(n_keys + 1), "left").astype(np.int32)
    return dict(diameter=F(diam), distance_step=F(step), n_pairs=len(pair), n_keys=n_keys, nt=nt, offsets=offsets, pair=pair.astype(np.uint32),
                alpha_bits=np.ascontiguousarray(alpha, F).view(np.uint32).copy(), key=key.astype(np.uint32), tn=tn, tgt=tgt, params=p)


def rotation_bin(am, as_, p):
    R = p["rotation_bins"]
    with np.errstate(all="ignore"):
        x = am - as_
        x = np.where(x < -PI, x + TWO_PI, np.where(x >= PI, x - TWO_PI, x))
        return np.clip(np.floor((x + PI) / (TWO_PI / F(R))).astype(np.int64), 0, R - 1)


def peaks(src, src_normals, model):
    """Rules 5 and 6: one PEAK record per reference point."""
    p = model["params"]
    src = np.asarray(src, F).reshape(-1, 3); sn = np.asarray(src_normals, F).reshape(-1, 3)
    ns, nt, R, stride = len(src), model["nt"], p["rotation_bins"], p["ref_stride"]
    n_ref = (ns + stride - 1) // stride
    out = np.zeros(n_ref, PEAK)
    out["ref"] = np.arange(n_ref) * stride
    good = usable(src, sn)
    off = model["offsets"].astype(np.int64)
    alpha_m = model["alpha_bits"].view(F)
    im_of = model["pair"].astype(np.int64) // max(nt, 1)
    for q in range(n_ref):
        r = q * stride
        if not good[r]:
            continue
        others = np.flatnonzero(good & (np.arange(ns) != r))
        if len(others) == 0:
            continue
        m = len(others)
        ok, key, al = pairs(np.broadcast_to(src[r], (m, 3)), np.broadcast_to(sn[r], (m, 3)), src[others], sn[others], model["distance_step"], p)
        key, al = key[ok], al[ok]
        start, cnt = off[key], off[key + 1] - off[key]
        total = int(cnt.sum())
        if total == 0:
            continue
        idx = np.repeat(start, cnt) + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        cell = im_of[idx] * R + rotation_bin(alpha_m[idx], np.repeat(al, cnt), p)
        acc = np.bincount(cell, minlength=nt * R)
        c = int(np.argmax(acc))                                   # the first maximum: lowest model point, then lowest bin
        out[q] = (r, c // R, c % R, acc[c])
    return out


# ---------------------------------------------------------------- rule 7, float64
def frame64(n):
    nx, ny, nz = (np.float64(v) for v in n)
    norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
    neg = nx < 0
    u = np.array([nx / norm, ny / norm, nz / norm])
    w = -u if neg else u
    k = 1.0 + w[0]
    ca, cb = w[1] / k, w[2] / k
    Rm = np.array([[w[0], w[1], w[2]], [-w[1], 1.0 - w[1] * ca, -w[1] * cb], [-w[2], -w[2] * ca, 1.0 - w[2] * cb]])
    if neg:
        Rm[0] = -Rm[0]; Rm[2] = -Rm[2]
    return Rm


def pose64(ps, ns_, pm, nm, b, R):
    """(Rot, t) of a peak."""
    alpha_c = F(-np.pi + (b + 0.5) * ((2.0 * np.pi) / R))
    c, sn = np.cos(np.float64(alpha_c)), np.sin(np.float64(alpha_c))
    Rs, Rm = frame64(ns_), frame64(nm)
    M = np.stack([Rs[0], c * Rs[1] + sn * Rs[2], c * Rs[2] - sn * Rs[1]])
    Rot = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Rot[i, j] = (Rm[0, i] * M[0, j] + Rm[1, i] * M[1, j]) + Rm[2, i] * M[2, j]
    ps = np.asarray(ps, np.float64); pm = np.asarray(pm, np.float64)
    t = np.array([pm[i] - ((Rot[i, 0] * ps[0] + Rot[i, 1] * ps[1]) + Rot[i, 2] * ps[2]) for i in range(3)])
    return Rot, t


def within(a, b, max_t, min_c):
    d = a[1] - b[1]
    if not np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= max_t:
        return False
    tr = 0.0
    for i in range(3):
        for j in range(3):
            tr += a[0][i, j] * b[0][i, j]
    return (tr - 1.0) / 2.0 >= min_c


def poses(src, src_normals, model, pk):
    """Rule 7 without the score: a list of dict(T (4, 4) f32, votes, members, ref, model_index, bin), ranked."""
    p = model["params"]
    src = np.asarray(src, F).reshape(-1, 3); sn = np.asarray(src_normals, F).reshape(-1, 3)
    order = [int(i) for i in np.argsort(-pk["votes"].astype(np.int64), kind="stable") if pk["votes"][i] > 0]
    P = {i: pose64(src[pk["ref"][i]], sn[pk["ref"][i]], model["tgt"][pk["model_index"][i]], model["tn"][pk["model_index"][i]],
                   int(pk["bin"][i]), p["rotation_bins"]) for i in order}
    max_t = np.float64(F(p["cluster_translation_relative"])) * np.float64(model["diameter"])
    min_c = np.cos(np.float64(F(p["cluster_rotation"])))
    clusters = []
    for i in order:
        for c in clusters:
            if within(P[i], P[c["founder"]], max_t, min_c):
                break
        else:
            c = dict(founder=i, votes=0, members=0)
            clusters.append(c)
        c["votes"] += int(pk["votes"][i]); c["members"] += 1
    top = sorted(range(len(clusters)), key=lambda c: -clusters[c]["votes"])[:p["max_poses"]]      # sorted() is stable: founding order among equals
    out = []
    for c in (clusters[t] for t in top):
        i = c["founder"]
        T = np.eye(4, dtype=F)
        T[:3, :3] = P[i][0].astype(F); T[:3, 3] = P[i][1].astype(F)
        out.append(dict(T=T, votes=c["votes"], members=c["members"], ref=int(pk["ref"][i]), model_index=int(pk["model_index"][i]),
                        bin=int(pk["bin"][i])))
    return out


def score(corr):
    """Rule 7's score from a tdv_icp_correspondences result (dict with d2, accepted, n_corr) over ns points: (n_corr, fitness, rmse)."""
    n, ns = int(corr["n_corr"]), len(corr["d2"])
    S = 0.0
    for v in corr["d2"][corr["accepted"]].astype(np.float64):
        S += v
    return n, F(n) / F(ns), (F(np.sqrt(S / n)) if n > 0 else F(0))


def match(src, src_normals, tgt, tgt_normals, **kw):
    """Table, peaks and ranked poses (unscored): (model, peaks, poses)."""
    model = model_table(tgt, tgt_normals, **kw)
    src = np.asarray(src, F).reshape(-1, 3)
    if len(src) == 0 or model["nt"] < 2 or model["n_pairs"] == 0:
        return model, np.zeros(0, PEAK), []
    pk = peaks(src, src_normals, model)
    return model, pk, poses(src, src_normals, model, pk)
