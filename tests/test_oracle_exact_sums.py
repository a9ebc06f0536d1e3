"""The oracle's exact-sum mode (oracle.cpp: XSum, icp_impl / ransac_impl with exact != 0), on the CPU.

The device's default ICP accumulation and its RANSAC rmse add f32 terms in f64 along a fixed tree; the f32 it takes from such a sum
is the exact sum rounded once, unless the exact sum lies within the tree's error bound of an f32 rounding midpoint.  The exact-sum
mode computes exactly that, and flags the ambiguous case, so tests/test_gpu_tree_sums_exact.py can hold the device to it bit for
bit.  Here the mode itself is pinned: its accumulator against math.fsum, its rounding and flag on constructed sums, and the whole
ICP / RANSAC against the float oracle where both must agree."""
import math

import numpy as np
import pytest

ROT_TOL, TRANS_TOL = 1e-4, 1e-6          # tests/test_gpu_icp.py (BASELINE.json): tree sums against the float oracle


def _f32_of_fraction(x):
    """A Python Fraction rounded to float32 (round half to even), by exact comparison with the two float32 neighbours."""
    f = np.float32(float(x))                                          # within an f64 ulp of x: f or one of its neighbours
    from fractions import Fraction
    for _ in range(3):
        up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
        hi, lo = (Fraction(float(f)) + Fraction(float(up))) / 2, (Fraction(float(f)) + Fraction(float(dn))) / 2
        if x > hi:
            f = up
        elif x < lo:
            f = dn
        else:
            if x == hi and int(f.view(np.uint32)) & 1:
                f = up
            if x == lo and int(f.view(np.uint32)) & 1:
                f = dn
            return f
    raise AssertionError("no float32 rounding found")


# ---------------------------------------------------------------- the accumulator
@pytest.mark.parametrize("seed", range(6))
def test_exact_sum_equals_fsum_on_f32_products(orc, seed):
    """Sets of f32 products (as the device forms J[a] * J[b], J[a] * r, err * err) and exact f64 products of f32 values (P_a * Q_b),
    with cancelling signs and spread exponents: the correctly rounded f64 is math.fsum's, the f32 is the exact sum rounded once."""
    from fractions import Fraction
    rng = np.random.default_rng(seed)
    n = [1, 7, 300, 5000, 40000, 3][seed]
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 4, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 4, n)).astype(np.float32)
    sets = {
        "f32 products": (a * b).astype(np.float64),
        "f64 products": a.astype(np.float64) * b.astype(np.float64),
        "cancelling": np.concatenate([(a * b).astype(np.float64), -(a * b).astype(np.float64)[::-1], [np.float64(np.float32(1e-7))]]),
        "mostly cancelling": np.concatenate([a.astype(np.float64) * 1e3, -a.astype(np.float64) * 1e3, b.astype(np.float64) * 1e-9]),
    }
    for name, t in sets.items():
        rng.shuffle(t)
        f64, f32, _ = orc.exact_sum(t, 30)
        assert f64 == math.fsum(t.tolist()), name
        exact = sum((Fraction(float(v)) for v in t), Fraction(0))
        assert f32.tobytes() == _f32_of_fraction(exact).tobytes(), (name, f32, float(exact))


def test_exact_sum_rounds_once_where_f64_would_round_twice(orc):
    """1 + 2^-24 + 2^-60: the f64 sum is 1 + 2^-24, an f32 midpoint that ties to 1; the exact sum is above it and rounds up."""
    t = np.array([1.0, 2.0 ** -24, 2.0 ** -60])
    f64, f32, amb = orc.exact_sum(t, 1)
    assert f64 == 1.0 + 2.0 ** -24
    assert f32 == np.float32(1.0 + 2.0 ** -23)
    assert np.float32(f64) == np.float32(1.0)                         # what rounding twice would give
    # ... and its exact distance from the midpoint, 2^-60, is inside a one-level tree's bound (2^-53 * 1.01): ambiguous
    assert amb
    # ties: the exact midpoint rounds to even, both ways
    assert orc.exact_sum([1.0, 2.0 ** -24], 0)[1] == np.float32(1.0)
    assert orc.exact_sum([1.0, 3 * 2.0 ** -24], 0)[1] == np.float32(1.0 + 2 * 2.0 ** -23)


def test_near_midpoint_sum_raises_the_flag(orc):
    """A sum whose exact value lies 2^-45 from an f32 rounding midpoint, from terms whose magnitudes sum to ~2^10: a 20-level f64
    tree may be off by 20 * 2^-53 * 2^10 = 2^-38.7 and round either way, so the sum is flagged; 2^-30 away it is not."""
    mid = 1.0 + 2.0 ** -24                                            # between the f32s 1 and 1 + 2^-23
    for off, flagged in ((2.0 ** -45, True), (-(2.0 ** -45), True), (2.0 ** -30, False), (-(2.0 ** -30), False)):
        t = np.array([512.0, mid + off, -512.0, 256.0, -256.0])
        f64, f32, amb = orc.exact_sum(t, 20)
        assert amb == flagged, (off, f64)
        assert f32 == np.float32(1.0 + 2.0 ** -23 if off > 0 else 1.0), off
    # terms on a grid whose every partial sum is exact in f64: the device's tree gives the exact midpoint too, and ties to even
    assert orc.exact_sum([1.0, 2.0 ** -24, 0.5, -0.5], 20)[1:] == (np.float32(1.0), False)
    # no terms, or terms that are all zero: nothing to round
    assert orc.exact_sum([], 20) == (0.0, np.float32(0.0), False)
    assert orc.exact_sum([0.0, 0.0], 20)[2] is False


# ---------------------------------------------------------------- ICP
def _grid_problem(p2plane, n=8, seed=0):
    """Source and target on a 2^-4 m grid, n accepted points (a power of two: the float oracle's means are exact), identity start:
    every sum either oracle forms is exact in f32, so both modes must give the same bits."""
    rng = np.random.default_rng(seed)
    src = rng.integers(-8, 8, (n, 3)).astype(np.float32) / 16.0
    src = np.unique(src, axis=0)[:n]
    assert len(src) == n
    tgt = src + np.array([1.0, -2.0, 1.0], np.float32) / 64.0        # every source's nearest target is its own shifted copy
    axes = np.eye(3, dtype=np.float32)
    nrm = axes[rng.integers(0, 3, n)]                                 # axis-aligned normals: J = p x n exact in f32
    return src, tgt, nrm if p2plane else None


@pytest.mark.parametrize("p2plane", [True, False])
def test_exact_mode_equals_the_float_oracle_where_sums_are_exact(orc, p2plane):
    src, tgt, nrm = _grid_problem(p2plane)
    for iters in (1, 2):   # one update from grid points (exact); the second from the updated pose must still agree within tolerance
        a = orc.icp(src, tgt, nrm, np.eye(4), 0.1, iters, p2plane, trace=True)
        b = orc.icp(src, tgt, nrm, np.eye(4), 0.1, iters, p2plane, trace=True, exact=True)
        if iters == 1:
            assert a["T"].tobytes() == b["T"].tobytes()
            assert a["trace"].tobytes() == b["trace"].tobytes()      # column 19 included: no sum is ambiguous
            assert (a["rmse"], a["fitness"], a["iterations"]) == (b["rmse"], b["fitness"], b["iterations"])
            assert not b["ambiguous"]
            assert b["trace"][0, 18] == 8
        else:
            assert np.abs(a["T"] - b["T"]).max() < TRANS_TOL


def _scene(synth, ns, nt, seed, offset=(0.0, 0.0, 0.0)):
    tgt, nrm = synth.sample_object(nt, seed)
    src, T_gt = synth.make_scene(ns, seed)
    T0 = synth.perturb(T_gt, seed=seed + 1, angle_deg=2.0, trans=0.003)
    S = np.eye(4, dtype=np.float32); S[:3, 3] = offset
    return src, tgt + np.float32(offset), nrm, (S @ T0).astype(np.float32)


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("seed,offset", [(3, 0.0), (4, 0.8), (5, 3.0)])
def test_exact_mode_agrees_with_the_float_oracle_on_scenes(orc, synth, p2plane, seed, offset):
    """Random scenes (object at the origin, 0.8 m and 3 m): within the tolerances that hold tree sums to the float oracle."""
    src, tgt, nrm, T0 = _scene(synth, 600, 500, seed, (0.0, 0.0, offset))
    a = orc.icp(src, tgt, nrm, T0, 0.004, 30, p2plane)
    b = orc.icp(src, tgt, nrm, T0, 0.004, 30, p2plane, exact=True)
    assert synth.rotation_angle(a["T"][:3, :3], b["T"][:3, :3]) <= ROT_TOL
    assert np.abs(a["T"][:3, 3] - b["T"][:3, 3]).max() <= TRANS_TOL * max(1.0, offset)
    assert abs(float(a["fitness"]) - float(b["fitness"])) <= 2.0 / len(src)
    if p2plane:   # point-to-point drifts past the float oracle's stopping point; its stopping iteration is its own
        assert abs(a["iterations"] - b["iterations"]) <= 1
    # one-iteration runs: the two sums differ by rounding only
    a1 = orc.icp(src, tgt, nrm, T0, 0.004, 1, p2plane, trace=True)
    b1 = orc.icp(src, tgt, nrm, T0, 0.004, 1, p2plane, trace=True, exact=True)
    assert a1["trace"][0, 18] == b1["trace"][0, 18]
    assert abs(float(a1["rmse"]) - float(b1["rmse"])) <= 1e-7


def test_exact_mode_sums_are_the_exact_sums(orc, synth):
    """The one-iteration point-to-plane update from sums computed here: the accepted set and the f32 products from
    icp_correspondences, math.fsum of them rounded to f32, then the oracle's own solve; the rmse from the fsum of d2."""
    from fractions import Fraction
    src, tgt, nrm, T0 = _scene(synth, 700, 400, 6)
    c = orc.icp_correspondences(src, tgt, nrm, T0, 0.004, True)
    acc = c["accepted"]
    te = _f32_of_fraction(sum((Fraction(float(v)) for v in c["d2"][acc]), Fraction(0)))
    r = orc.icp(src, tgt, nrm, T0, 0.004, 1, True, trace=True, exact=True)
    assert r["trace"][0, 18] == c["n_corr"] and not r["ambiguous"]
    assert r["rmse"] == np.sqrt(np.float32(te / np.float32(c["n_corr"])))


# ---------------------------------------------------------------- RANSAC
@pytest.mark.parametrize("ns", [255, 257, 2048])
def test_ransac_exact_rmse_is_the_exact_sum(orc, synth, ns):
    """The winner's rmse in exact mode is sqrt(f32(exact sum of err * err) / inliers), err recomputed here in the oracle's float
    arithmetic; transform, fitness and iterations are the float oracle's."""
    from fractions import Fraction
    src, T_gt = synth.make_scene(ns, 11)
    tgt = (src.astype(np.float64) @ T_gt[:3, :3].T.astype(np.float64) + T_gt[:3, 3]).astype(np.float32)
    tgt += np.random.default_rng(ns).normal(0, 0.0006, tgt.shape).astype(np.float32)
    corr = np.arange(ns, dtype=np.int32)
    a = orc.ransac(src, tgt, corr=corr, voxel=0.001, max_iterations=200)
    b = orc.ransac(src, tgt, corr=corr, voxel=0.001, max_iterations=200, exact=True)
    assert a["T"].tobytes() == b["T"].tobytes() and a["fitness"] == b["fitness"] and a["best_iter"] == b["best_iter"]
    assert abs(float(a["rmse"]) - float(b["rmse"])) <= 1e-7 and not b["rmse_ambiguous"]
    R, t = b["T"][:3, :3], b["T"][:3, 3]
    p = np.empty_like(src)
    for r in range(3):     # sum3(a, b, c) = a + (b + c), then + t: the oracle's mulv
        p[:, r] = R[r, 0] * src[:, 0] + (R[r, 1] * src[:, 1] + R[r, 2] * src[:, 2])
    p = p + t
    d = p - tgt
    err = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    inl = err < np.float32(0.001) * np.float32(1.5)
    e2 = (err[inl] * err[inl]).astype(np.float32)
    te = _f32_of_fraction(sum((Fraction(float(v)) for v in e2), Fraction(0)))
    assert int(inl.sum()) == round(float(b["fitness"]) * ns)
    assert b["rmse"] == np.sqrt(np.float32(te / np.float32(inl.sum())))


# ---------------------------------------------------------------- non-finite terms
@pytest.mark.parametrize("terms,expect", [
    ([1.0, np.inf, 2.0], np.inf),
    ([np.inf], np.inf),
    ([-3.0, -np.inf, 1e300, -np.inf], -np.inf),
    ([np.inf, 5.0, -np.inf], np.nan),
    ([1.0, np.nan, 2.0], np.nan),
    ([np.nan, np.inf], np.nan),
    ([-np.nan, -np.inf, -1.0], np.nan),
])
def test_exact_sum_of_non_finite_terms(orc, terms, expect):
    """What the device's f64 tree gives in any order (oracle.cpp, XSum): a NaN term or both infinities make NaN, else an infinite
    term makes that infinity; the f32 is the same value and nothing is ambiguous."""
    for order in (terms, terms[::-1], terms[1:] + terms[:1]):
        for reps in (1, 1000):
            t = np.array(order * reps, np.float64)
            f64, f32, amb = orc.exact_sum(t, 30)
            if np.isnan(expect):
                assert np.isnan(f64) and np.isnan(f32), (order, reps, f64, f32)
            else:
                assert f64 == expect and f32 == np.float32(expect), (order, reps, f64, f32)
            assert not amb
            if reps == 1:
                with np.errstate(invalid="ignore"):
                    assert np.array_equal(np.float64(np.sum(t)), f64, equal_nan=True)   # one more order, numpy's pairwise sum


def test_exact_sum_finite_terms_unchanged_next_to_overflowing_f32_products(orc):
    """An f32 product that overflows to +inf in one term set leaves another set of finite terms exact (the infinities are per sum)."""
    big = np.float32(1e20)
    with np.errstate(over="ignore"):
        sq = np.float32(big * big)
    assert np.isinf(sq)
    f64, f32, _ = orc.exact_sum(np.array([sq, 1.0], np.float64), 30)
    assert f64 == np.inf and f32 == np.inf
    t = np.array([1e38, 1.0, -1e38, 2.0 ** -60], np.float64)
    assert orc.exact_sum(t, 30)[0] == math.fsum(t.tolist())


def test_oracle_svd_ends_on_non_finite_entries(orc):
    """The oracle's Jacobi SVD loop has no iteration count: a NaN or an infinite entry must end it (every comparison with NaN is
    false; an infinite scale turns the other entries into 0 or NaN)."""
    for v in (np.inf, -np.inf, np.nan, 1e38):
        H = np.eye(3, dtype=np.float32) * 0.3 + 0.01
        H[1, 2] = v
        R = orc.kabsch_rotation(H)
        assert R.shape == (3, 3)
