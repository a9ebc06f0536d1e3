"""RansacLeafBound's two levels (csrc/ransac.hip, k_ransac_bound): a coarse leaf is the union of 4 consecutive fine leaves, and
the coarse pass fails a leaf only on g2 > (s + 5 E)^2 where the fine pass uses (s + 3 E)^2.  Emulated operation for operation in
f32 (as tests/test_ransac_leaf_bound_margin.py does for the fine leaves), on coarse leaves whose boxes touch the threshold shell:
  * a coarse leaf that fails holds no pair the reference arithmetic counts as an inlier;
  * a coarse leaf that fails has four children that all fail the fine test, so the coarse sum bounds the fine sum and a
    hypothesis the coarse level proves dead is one the fine walk proves dead too (the live list does not change).
Clouds at the origin and 250 m from it, and 100 km out, where the band and with it both levels are off."""
import numpy as np
import pytest

U = 2.0 ** -24


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    return _f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))


def _tau_lt(thr):
    thr = np.float32(thr)
    f = np.float32(thr * thr)
    while np.sqrt(f) >= thr:
        f = np.nextafter(f, np.float32(0))
    while np.sqrt(f) < thr:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def _box(lo, hi):
    """k_leaf_build's summary of a leaf from its per-axis min / max (rl_leaf_store): p centre, half-extent rounded up"""
    pc = _f32(_f32(np.float32(0.5) * lo) + _f32(np.float32(0.5) * hi))
    d = np.maximum(hi.astype(np.float64) - pc, pc.astype(np.float64) - lo)
    return pc, np.nextafter(_f32(d), np.float32(np.inf))


def _g2(R, t, pc, pe, qlo, qhi):
    """k_ransac_bound's f32 gap length squared of one leaf per row of R / t"""
    g2 = np.zeros(len(R), np.float32)
    for c in range(3):
        xc = _fma(R[:, c, 0], pc[:, 0], _fma(R[:, c, 1], pc[:, 1], _fma(R[:, c, 2], pc[:, 2], t[:, c])))
        xe = _fma(np.abs(R[:, c, 0]), pe[:, 0], _fma(np.abs(R[:, c, 1]), pe[:, 1], _f32(np.abs(R[:, c, 2]) * pe[:, 2])))
        lo_gap = _f32(_f32(xc - xe) - qhi[:, c]); hi_gap = _f32(qlo[:, c] - _f32(xc + xe))
        gp = np.maximum(np.maximum(lo_gap, hi_gap), np.float32(0))
        g2 = _fma(gp, gp, g2)
    return g2


@pytest.mark.parametrize("offset", [0.0, 250.0, 1e5])
def test_coarse_leaf_failure_implies_fine_failure_and_no_inlier(offset):
    rng = np.random.default_rng(61 + int(offset) % 1000)
    L, F, K = 3000, 4, 32                 # coarse leaves, fine leaves per coarse leaf (RL_COARSE / RL_LEAF), pairs per fine leaf
    thr = np.float32(0.003 * 1.5)
    tau = _tau_lt(thr)
    s = np.nextafter(np.float32(np.sqrt(np.float64(tau))), np.float32(np.inf))
    band_u = np.float32(16.0 * U)

    qr, _ = np.linalg.qr(rng.normal(size=(L, 3, 3)))
    R = _f32(qr + rng.normal(size=(L, 3, 3)) * rng.choice([0.0, 1e-7, 1e-3], (L, 1, 1)))
    t = _f32(rng.normal(size=(L, 3)) * 0.3 - (R.astype(np.float64) @ np.full(3, offset)) + offset)
    # four fine leaves per coarse leaf: each its own centre near the coarse one and its own spread (a point up to a hundredth of thr)
    spread = thr * rng.choice([0.0, 1e-7, 1e-5, 1e-3, 1e-2], (L, 1)) * (0.5 + 0.5 * rng.random((L, F)))
    centre = (rng.random((L, 3)) - 0.5) * 0.6 + offset
    sub = centre[:, None, :] + rng.normal(size=(L, F, 3)) * (thr * rng.choice([0.0, 1e-6, 1e-3, 1e-2], (L, 1, 1)))
    p = _f32(sub[:, :, None, :] + (rng.random((L, F, K, 3)) - 0.5) * 2 * spread[:, :, None, None])
    xr = np.einsum("lij,lfkj->lfki", R.astype(np.float64), p.astype(np.float64)) + t[:, None, None, :].astype(np.float64)
    P = np.float32(np.abs(p).max())
    A = np.max(_f32(_f32(_f32(_f32(np.abs(R[:, :, 0]) + np.abs(R[:, :, 1])) + np.abs(R[:, :, 2])) * P) + np.abs(t)), axis=1)
    E = _f32(_f32(_f32(band_u * A) + _f32(band_u * s)) * np.float32(1.0001))
    bounded = E < np.float32(0.25) * s
    # matches at s + m E from the transformed point: m around both margins (3 E fine, 5 E coarse) and below them
    m = rng.choice([-1.0, 0.0, 2.0, 2.9, 3.0, 3.1, 4.0, 4.9, 5.0, 5.05, 5.2, 6.0, 10.0], (L, 1, 1)) + rng.normal(size=(L, F, K)) * 0.01
    dirs = rng.normal(size=(L, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dist = s.astype(np.float64) + m * E[:, None, None].astype(np.float64)
    q = _f32(xr + dirs[:, None, None, :] * dist[..., None])

    # the reference arithmetic per pair
    def row_ref(c):
        a = _f32(R[:, None, None, c, 0] * p[..., 0]); b = _f32(R[:, None, None, c, 1] * p[..., 1]); cc = _f32(R[:, None, None, c, 2] * p[..., 2])
        return _f32(_f32(a + _f32(b + cc)) + t[:, None, None, c])
    dr = [_f32(row_ref(c) - q[..., c]) for c in range(3)]
    d2_ref = _f32(_f32(dr[0] * dr[0]) + _f32(_f32(dr[1] * dr[1]) + _f32(dr[2] * dr[2])))
    inlier = d2_ref < tau

    def tb(margin):
        sb = _f32(s + _f32(np.float32(margin) * E))
        return _f32(_f32(sb * sb) * np.float32(1.0 + 1e-6))

    # fine leaves (k_leaf_build's shuffles) and their coarse parents (the min / max of the fine ones)
    flo, fhi = p.min(2), p.max(2)
    fqlo, fqhi = q.min(2), q.max(2)
    fine_fail = np.zeros((L, F), bool)
    for f in range(F):
        pc, pe = _box(flo[:, f], fhi[:, f])
        fine_fail[:, f] = bounded & (_g2(R, t, pc, pe, fqlo[:, f], fqhi[:, f]) > tb(3.0))
    pc, pe = _box(flo.min(1), fhi.max(1))
    assert (np.abs(p - pc[:, None, None, :]).astype(np.float64) <= pe[:, None, None, :]).all()
    coarse_fail = bounded & (_g2(R, t, pc, pe, fqlo.min(1), fqhi.max(1)) > tb(5.0))

    assert not (inlier.reshape(L, -1) & coarse_fail[:, None]).any()          # a failed coarse leaf holds no inlier
    assert fine_fail[coarse_fail].all()                                        # ... and all four of its children fail as well
    if offset < 1e4:
        D = np.linalg.norm(xr - q.astype(np.float64), axis=3).reshape(L, -1).min(1)
        near = coarse_fail & (D < s + 6 * E)                                   # failures right at the coarse margin
        assert near.sum() > 15, near.sum()
        assert coarse_fail.sum() > L // 20 and (fine_fail.all(1) & ~coarse_fail).any()
    else:
        assert not bounded.any()
