"""RansacFarBound (csrc/ransac.hip): a pair of F that rf_near's threshold T leaves uncounted is no inlier of the hypothesis in the
reference arithmetic, and the count table's lookup is never below the true count.  The kernel's f32 operations are emulated here one
for one (fused multiply-adds through float64, where a product of two floats is exact): the displacement bound Delta over the 8 corners
of the sources' box, the two bands, T; pairs are placed on the shell d_B = s + Delta + m (E_h + E_B) for m around the kernel's margin
of 3, their sources at the corner where the displacement is largest and their matches in the displacement's direction - the worst
case of the triangle inequality - at the origin and 250 m from it (and 100 km, where the bands, and with them the skipping, are off)."""
import numpy as np
import pytest

U = 2.0 ** -24
RF_SHIFT, RF_BINS = 20, 2048


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    return _f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))


def _tau_lt(thr):
    """smallest float f with sqrtf(f) >= thr (csrc/ctx.hip tau_lt): d2 < tau <=> sqrtf(d2) < thr"""
    thr = np.float32(thr)
    f = np.float32(thr * thr)
    while np.sqrt(f) >= thr:
        f = np.nextafter(f, np.float32(0))
    while np.sqrt(f) < thr:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def _reach(R, t, P):
    """ransac_band_reach in f32: max over rows of (|r0| + |r1| + |r2|) P + |t|"""
    return np.max(_f32(_f32(_f32(_f32(np.abs(R[:, :, 0]) + np.abs(R[:, :, 1])) + np.abs(R[:, :, 2])) * P) + np.abs(t)), axis=1)


def _d2_ref(R, t, p, q):
    """the reference arithmetic per pair (k_ransac_score / the oracle): mul, mul, mul, add, add, add; squared norm in its order"""
    def row(c):
        a = _f32(R[:, None, c, 0] * p[:, :, 0]); b = _f32(R[:, None, c, 1] * p[:, :, 1]); cc = _f32(R[:, None, c, 2] * p[:, :, 2])
        return _f32(_f32(a + _f32(b + cc)) + t[:, None, c])
    dr = [_f32(row(c) - q[:, :, c]) for c in range(3)]
    return _f32(_f32(dr[0] * dr[0]) + _f32(_f32(dr[1] * dr[1]) + _f32(dr[2] * dr[2])))


def _bin(t):
    return (np.asarray(t, np.float32).view(np.uint32) >> RF_SHIFT).astype(np.int64)


@pytest.mark.parametrize("offset", [0.0, 250.0, 1e5])
def test_ransac_far_bound_margin_covers_both_arithmetics(offset):
    rng = np.random.default_rng(31 + int(offset) % 1000)
    L, K = 4000, 32                      # (hypothesis, ordering pose) couples, pairs per couple
    thr = np.float32(0.003 * 1.5)
    tau = _tau_lt(thr)
    s = np.nextafter(np.float32(np.sqrt(np.float64(tau))), np.float32(np.inf))     # sqrt_tau of ransac_run_dev
    band_u = np.float32(16.0 * U)

    # the ordering pose B and a hypothesis h that differs from it by a rotation of up to 0.1 rad and a shift of up to 30 thresholds
    qr, _ = np.linalg.qr(rng.normal(size=(L, 3, 3)))
    RB = _f32(qr)
    tB = _f32(rng.normal(size=(L, 3)) * 0.3 - (RB.astype(np.float64) @ np.full(3, offset)) + offset)
    w = rng.normal(size=(L, 3)) * rng.choice([0.0, 1e-6, 1e-4, 1e-2, 1e-1], (L, 1))
    Wx = np.zeros((L, 3, 3)); Wx[:, 0, 1] = -w[:, 2]; Wx[:, 0, 2] = w[:, 1]; Wx[:, 1, 0] = w[:, 2]; Wx[:, 1, 2] = -w[:, 0]; Wx[:, 2, 0] = -w[:, 1]; Wx[:, 2, 1] = w[:, 0]
    Rh = _f32((np.eye(3) + Wx) @ RB.astype(np.float64))
    lo = _f32(np.full((L, 3), offset) - 0.3 * rng.random((L, 3))); hi = _f32(np.full((L, 3), offset) + 0.3 * rng.random((L, 3)))
    mid = 0.5 * (lo.astype(np.float64) + hi)
    # (the shift is taken at the box's middle, so that rotation and shift both show in Delta)
    th = _f32(tB.astype(np.float64) + ((RB.astype(np.float64) - Rh) @ mid[:, :, None])[:, :, 0] + rng.normal(size=(L, 3)) * thr * rng.choice([0.0, 0.1, 1.0, 30.0], (L, 1)))

    # rf_near, operation for operation
    P = np.float32(max(np.abs(lo).max(), np.abs(hi).max()))
    AB, Ah = _reach(RB, tB, P), _reach(Rh, th, P)
    EB = _f32(_f32(_f32(band_u * AB) + _f32(band_u * s)) * np.float32(1.0001))
    Eh = _f32(_f32(_f32(band_u * Ah) + _f32(band_u * s)) * np.float32(1.0001))
    bounded = (Eh < np.float32(0.25) * s) & (EB < np.float32(0.25) * s)
    dR, dt = _f32(Rh - RB), _f32(th - tB)
    m2 = np.zeros(L, np.float32)
    D2 = np.zeros(L); arg = np.zeros(L, np.int64)         # the real squared displacement's largest corner (float64)
    dRr, dtr = Rh.astype(np.float64) - RB, th.astype(np.float64) - tB
    for k in range(8):
        c = np.stack([hi[:, a] if (k >> a) & 1 else lo[:, a] for a in range(3)], axis=1)
        n2 = np.zeros(L, np.float32)
        for a in range(3):
            v = _fma(dR[:, a, 0], c[:, 0], _fma(dR[:, a, 1], c[:, 1], _fma(dR[:, a, 2], c[:, 2], dt[:, a])))
            n2 = _fma(v, v, n2)
        m2 = np.maximum(m2, n2)
        r2 = (((dRr @ c.astype(np.float64)[:, :, None])[:, :, 0] + dtr) ** 2).sum(1)
        arg = np.where(r2 > D2, k, arg); D2 = np.maximum(D2, r2)
    delta_f = np.sqrt(m2)                                  # f32, correctly rounded as the build's sqrtf
    sb = _f32(_f32(_f32(s + delta_f) + _f32(np.float32(3.0) * _f32(Eh + EB))) * np.float32(1.0 + 4e-6))
    T = _f32(_f32(sb * sb) * np.float32(1.0 + 1e-6))
    delta = np.sqrt(D2)
    # (1) the f32 corner maximum against the real one
    assert (delta[bounded] <= (1 + 3 * U) * delta_f[bounded].astype(np.float64) + 9 * U * (Ah + AB)[bounded].astype(np.float64)).all()

    # sources: half of them at the corner of the largest displacement, the rest anywhere in the box; matches in the displacement's
    # direction from the point under B, at s + Delta + m (E_h + E_B)
    corner = np.stack([np.where((arg >> a) & 1, hi[:, a], lo[:, a]) for a in range(3)], axis=1)
    p = _f32(lo[:, None, :] + rng.random((L, K, 3)) * (hi - lo)[:, None, :])
    p[:, : K // 2] = corner[:, None, :]
    xB = np.einsum("lij,lkj->lki", RB.astype(np.float64), p.astype(np.float64)) + tB[:, None, :].astype(np.float64)
    xh = np.einsum("lij,lkj->lki", Rh.astype(np.float64), p.astype(np.float64)) + th[:, None, :].astype(np.float64)
    disp = xh - xB
    nd = np.linalg.norm(disp, axis=2, keepdims=True)
    rnd = rng.normal(size=(L, K, 3)); rnd /= np.linalg.norm(rnd, axis=2, keepdims=True)
    dirs = np.where(nd > 0, disp / np.where(nd > 0, nd, 1.0), rnd)
    m = rng.choice([-1.0, 0.0, 1.0, 2.0, 2.9, 3.0, 3.05, 3.2, 4.0, 8.0], (L, 1)) + rng.normal(size=(L, K)) * 0.01
    dist = s.astype(np.float64) + delta[:, None] + m * (Eh + EB)[:, None].astype(np.float64)
    q = _f32(xB + dirs * dist[:, :, None])

    d2_B = _d2_ref(RB, tB, p, q)
    inlier_h = _d2_ref(Rh, th, p, q) < tau
    excluded = bounded[:, None] & (d2_B >= T[:, None])     # what the lookup at T may leave uncounted (it counts every d2_B < T)
    # (2) the reference's distance under B against the real one, from above
    DB = np.linalg.norm(xB - q.astype(np.float64), axis=2)
    assert (np.sqrt(d2_B.astype(np.float64)) <= (1 + 3 * U) * DB + 7 * U * AB[:, None]).all()
    # end to end: no excluded pair is an inlier of h
    assert not (inlier_h & excluded).any()
    if offset < 1e4:
        Dh = np.linalg.norm(xh - q.astype(np.float64), axis=2)
        shell = excluded & (Dh < s + 4 * (Eh + EB)[:, None])
        assert shell.sum() > 50, shell.sum()               # the test reaches the shell
        assert inlier_h.any() and excluded.sum() > L * K // 10
    else:
        assert not bounded.any()                           # 100 km from the origin the bands are off: no skipping

    # the count table: bins over the leading bits of d2_B, running sums; a lookup at t counts at least the pairs with d2_B < t
    pool = d2_B[np.isfinite(d2_B)].ravel()
    hist = np.bincount(_bin(pool), minlength=RF_BINS)
    cum = np.cumsum(hist)
    ts = np.concatenate([T, pool[:: 97], np.nextafter(pool[:: 89], np.float32(np.inf)), np.float32([0.0, 1e-30, 3e38, np.inf])]).astype(np.float32)
    srt = np.sort(pool)
    true = np.searchsorted(srt, ts, side="left")           # pairs strictly below t
    assert (cum[_bin(ts)] >= true).all()
