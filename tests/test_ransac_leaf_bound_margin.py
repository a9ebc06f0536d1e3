"""RansacLeafBound (csrc/ransac.hip): a leaf that k_ransac_bound fails holds no pair the reference arithmetic counts as an
inlier.  The kernel's leaf summary and its f32 bound are emulated here operation for operation (fused multiply-adds through
float64, where a product of two floats is exact), on leaves whose boxes touch the threshold shell: pairs placed at s + m E
from their transformed points for m around the kernel's 3 E margin, leaf boxes from a single point to a tenth of the
threshold, clouds at the origin and 250 m from it (and 100 km, where the band, and with it the bound, is off)."""
import numpy as np
import pytest

U = 2.0 ** -24


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


@pytest.mark.parametrize("offset", [0.0, 250.0, 1e5])
def test_ransac_leaf_bound_margin_covers_both_arithmetics(offset):
    rng = np.random.default_rng(29 + int(offset) % 1000)
    L, K = 4000, 32                      # leaves, pairs per leaf (RL_LEAF)
    thr = np.float32(0.003 * 1.5)
    tau = _tau_lt(thr)
    s = np.nextafter(np.float32(np.sqrt(np.float64(tau))), np.float32(np.inf))     # sqrt_tau of ransac_run_dev
    band_u = np.float32(16.0 * U)

    # one hypothesis per leaf: rotations with and without noise, translations that bring the object back near the offset
    qr, _ = np.linalg.qr(rng.normal(size=(L, 3, 3)))
    R = _f32(qr + rng.normal(size=(L, 3, 3)) * rng.choice([0.0, 1e-7, 1e-3], (L, 1, 1)))
    t = _f32(rng.normal(size=(L, 3)) * 0.3 - (R.astype(np.float64) @ np.full(3, offset)) + offset)
    # leaves: K source points in a box of half-size `spread` (a single point up to a tenth of the threshold)
    spread = thr * rng.choice([0.0, 1e-7, 1e-5, 1e-3, 1e-1], L)
    centre = (rng.random((L, 3)) - 0.5) * 0.6 + offset
    p = _f32(centre[:, None, :] + (rng.random((L, K, 3)) - 0.5) * 2 * spread[:, None, None])
    xr = np.einsum("lij,lkj->lki", R.astype(np.float64), p.astype(np.float64)) + t[:, None, :].astype(np.float64)
    # matches at distance s + m E from the transformed point, E the kernel's band; m around the 3 E margin and below it
    P = np.float32(np.abs(p).max())
    A = np.max(_f32(_f32(_f32(_f32(np.abs(R[:, :, 0]) + np.abs(R[:, :, 1])) + np.abs(R[:, :, 2])) * P) + np.abs(t)), axis=1)   # the kernel's f32 A
    E = _f32(_f32(_f32(band_u * A) + _f32(band_u * s)) * np.float32(1.0001))
    bounded = E < np.float32(0.25) * s
    m = rng.choice([-1.0, 0.0, 1.0, 2.0, 2.9, 3.0, 3.05, 3.2, 4.0, 8.0], (L, 1)) + rng.normal(size=(L, K)) * 0.01
    dirs = rng.normal(size=(L, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dist = s.astype(np.float64) + m * E[:, None].astype(np.float64)
    q = _f32(xr + dirs[:, None, :] * dist[:, :, None])

    # the reference arithmetic per pair (k_ransac_score / the oracle): mul, mul, mul, add, add, add; squared norm in its order
    Rr = R.astype(np.float32)
    def row_ref(c):
        a = _f32(Rr[:, None, c, 0] * p[:, :, 0]); b = _f32(Rr[:, None, c, 1] * p[:, :, 1]); cc = _f32(Rr[:, None, c, 2] * p[:, :, 2])
        return _f32(_f32(a + _f32(b + cc)) + t[:, None, c])
    dr = [_f32(row_ref(c) - q[:, :, c]) for c in range(3)]
    d2_ref = _f32(_f32(dr[0] * dr[0]) + _f32(_f32(dr[1] * dr[1]) + _f32(dr[2] * dr[2])))
    inlier = d2_ref < tau

    # k_leaf_build: p centre and half-extent (rounded up past the exact one), q lo / hi
    lo, hi = p.min(1), p.max(1)
    pc = _f32(_f32(np.float32(0.5) * lo) + _f32(np.float32(0.5) * hi))
    d = np.maximum(hi.astype(np.float64) - pc, pc.astype(np.float64) - lo)
    pe = np.nextafter(_f32(d), np.float32(np.inf))
    qlo, qhi = q.min(1), q.max(1)
    assert (np.abs(p - pc[:, None, :]).astype(np.float64) <= pe[:, None, :]).all()

    # k_ransac_bound, one leaf per hypothesis
    sb = _f32(s + _f32(np.float32(3.0) * E))
    tb = _f32(_f32(sb * sb) * np.float32(1.0 + 1e-6))
    g2 = np.zeros(L, np.float32)
    G2 = np.zeros(L)                      # the real gap length squared (float64)
    for c in range(3):
        xc = _fma(R[:, c, 0], pc[:, 0], _fma(R[:, c, 1], pc[:, 1], _fma(R[:, c, 2], pc[:, 2], t[:, c])))
        xe = _fma(np.abs(R[:, c, 0]), pe[:, 0], _fma(np.abs(R[:, c, 1]), pe[:, 1], _f32(np.abs(R[:, c, 2]) * pe[:, 2])))
        lo_gap = _f32(_f32(xc - xe) - qhi[:, c]); hi_gap = _f32(qlo[:, c] - _f32(xc + xe))
        gp = np.maximum(np.maximum(lo_gap, hi_gap), np.float32(0))
        g2 = _fma(gp, gp, g2)
        xcr = (R[:, c, :].astype(np.float64) * pc).sum(1) + t[:, c]
        xer = (np.abs(R[:, c, :]).astype(np.float64) * pe).sum(1)
        G2 += np.maximum(np.maximum(xcr - xer - qhi[:, c], qlo[:, c] - xcr - xer), 0.0) ** 2
    fails = bounded & (g2 > tb)

    # (1) the f32 bound against the real gap length: sqrt(g2) <= (1 + 3 u) G + 14.2 u A
    G = np.sqrt(G2)
    b1 = (1 + 3 * U) * G + 14.2 * U * A
    assert (np.sqrt(g2[bounded].astype(np.float64)) <= b1[bounded]).all()
    # (2) the reference's distance against the real one: sqrt(d2_ref) >= D (1 - 3 u) - 7 u A
    D = np.linalg.norm(xr - q.astype(np.float64), axis=2)
    assert (np.sqrt(d2_ref.astype(np.float64)) >= D * (1 - 3 * U) - 7 * U * A[:, None]).all()
    # the leaf box bounds every pair's real distance from below (up to float64's own rounding at these magnitudes)
    assert (D.min(1) >= G - 1e-12 * max(1.0, offset)).all()
    # end to end: a failed leaf holds no inlier
    assert not (inlier & fails[:, None]).any()
    if offset < 1e4:
        # the test reaches the shell: failed leaves whose closest pair sits within 4 E of the threshold
        near = fails & (D.min(1) < s + 4 * E)
        assert near.sum() > 50, near.sum()
        assert inlier.any() and fails.sum() > L // 10
    else:
        assert not bounded.any()          # 100 km from the origin the band is off, and so is the bound: nothing is pruned
