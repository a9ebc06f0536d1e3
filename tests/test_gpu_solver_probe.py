"""The device's per-lane solvers (csrc/device_linalg.hpp), its libm restatement (csrc/libm_f32.hpp) and RANSAC's hypothesis lane, each
called directly through the study library's probe (csrc/probe.hip: one problem per lane, the product kernels' own inline functions) on
the adversarial families of tests/solver_inputs.py, and held to the CPU oracle BYTE FOR BYTE - zero signs included; where the oracle
has a NaN the device must have one (payload and sign free).  No tolerances, except sinf / cosf from |x| = 120 on (see there).

Every batch runs twice on the device, grouped by family and in a fixed pseudo-random order - lanes of one wave then take different
sweep counts, iteration counts and early exits - and both runs must give the same bytes per problem.  Every family asserts that it
still reaches the branch it aims at, from the oracle's outputs or the inputs.

The tests named test_probed_* need the study library: tests/test_gpu_study_build.py runs them in its study process."""
import ctypes as C

import numpy as np
import pytest

import solver_inputs as si

pytestmark = pytest.mark.gpu
SEED = 20240


def same(got, ref, what, where=None):
    """Equal as bytes; a NaN of the oracle needs a NaN of the device in its place."""
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = (gn != rn) | (~gn & ~rn & (got.view(np.uint32) != ref.view(np.uint32)))
    if bad.any():
        rows = np.unique(np.argwhere(bad.reshape(len(bad), -1))[:, 0])
        fams = {} if where is None else {n: int(((rows >= s.start) & (rows < s.stop)).sum()) for n, s in where.items()}
        i = rows[0]
        raise AssertionError("%s: %d of %d problems differ %s; first: problem %d device %s oracle %s" % (
            what, len(rows), len(got), {n: c for n, c in fams.items() if c}, i, got[i].tolist(), ref[i].tolist()))


def both_orders(probe, op, x, what):
    """The device's results for x, after holding them equal - as bytes - to a second run in a fixed pseudo-random order."""
    out = probe(op, x)
    perm = si.permutation(len(x))
    out2 = probe(op, np.ascontiguousarray(x[perm]))
    assert out2.tobytes() == out[perm].tobytes(), what + ": a problem's result depends on its neighbours in the wave"
    return out


def reach(count, least, what):
    print("reach: %s: %d (at least %d)" % (what, count, least))
    assert count >= least, "the inputs no longer reach '%s': %d < %d" % (what, count, least)


# ------------------------------------------------------------------------------------------------ the checks (probe: (op, array) -> array)
def check_svd3(probe, orc, synth):
    (M,), where = si.concat(si.mat3_families(SEED, synth, orc))
    A = si.colmajor9(M)
    U, S, V, sweeps = orc.jacobi_svd3_batch(A)
    print("svd3: %d problems, oracle sweeps max %d" % (len(A), sweeps.max()))
    assert sweeps.max() < 64, "an input needs the device's 64-sweep guard: change the family (problem %d)" % int(sweeps.argmax())
    reach(int((sweeps >= 3).sum()), 20000, "sweeps >= 3")
    with np.errstate(invalid="ignore"):
        reach(int((((S[:, 0] == S[:, 1]) | (S[:, 1] == S[:, 2])) & (S[:, 0] > 0)).sum()), 1500, "repeated non-zero singular values")
        reach(int((S[:, 2] == 0).sum()), 3000, "a singular value exactly zero")
    reach(int(np.isnan(S).any(1).sum()), 300, "NaN singular values")
    got = both_orders(probe, "svd3", A, "svd3")
    same(got, np.concatenate([U, V, S], 1), "svd3 (U, V, s)", where)
    return int(sweeps.max())


def check_kabsch(probe, orc, synth):
    (M,), where = si.concat(si.mat3_families(SEED, synth, orc))
    A = si.colmajor9(M)
    U, S, V, _ = orc.jacobi_svd3_batch(A)
    Um = U.reshape(-1, 3, 3).transpose(0, 2, 1).astype(np.float64); Vm = V.reshape(-1, 3, 3).transpose(0, 2, 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        det = np.linalg.det(np.nan_to_num(Vm @ Um.transpose(0, 2, 1)))
        reach(int((det < -0.5).sum()), 5000, "det(V U^T) < 0 before the flip")
        reach(int(((det < -0.5) & (S[:, 2] == 0)).sum()), 500, "a reflection of a rank-deficient H")
    same(both_orders(probe, "kabsch_rotation", A, "kabsch_rotation"), orc.kabsch_rotation_batch(A), "kabsch_rotation", where)


def check_eigvec(probe, orc, synth):
    (M,), where = si.concat(si.sym3_families(SEED, synth, orc))
    w, V, rc, iters = orc.self_adjoint_eig3_batch(si.colmajor9(M))
    print("smallest_eigvec3: %d problems, QR steps max %d among the converged, %d not converged" % (len(M), iters[rc == 0].max(), int((rc != 0).sum())))
    reach(int((rc != 0).sum()), 100, "ok == false (the QR iteration gave up)")
    reach(int((rc == 0).sum()), 100000, "ok == true")
    assert iters[rc != 0].min() == 91 and iters[rc == 0].max() <= 90
    reach(int(((rc == 0) & (iters == 0)).sum()), 2000, "nothing to iterate (diagonal after the cut-offs)")
    with np.errstate(invalid="ignore"):
        reach(int(((rc == 0) & ((w[:, 0] == w[:, 1]) | (w[:, 1] == w[:, 2]))).sum()), 1500, "equal eigenvalues")
    reach(int(si.reaches_e2_underflow(M).sum()), 200, "e * e == 0 in the Wilkinson shift")
    ref = np.concatenate([V[:, :3], (rc == 0).astype(np.float32)[:, None]], 1)       # column 0 of V: the smallest eigenvalue's vector
    same(both_orders(probe, "smallest_eigvec3", si.lower6(M), "smallest_eigvec3"), ref, "smallest_eigvec3 (vector, ok)", where)
    return int(iters[rc == 0].max())


def check_ldlt(probe, orc):
    (A, b), where = si.concat(si.ldlt_families(SEED, orc))
    reach(int(si.has_zero_row(A).sum()), 4000, "an exactly zero pivot after step 0")
    d = A.reshape(-1, 6, 6)[:, np.arange(6), np.arange(6)]
    reach(int(((d == 0).all(1) & (A != 0).any(1)).sum()), 1500, "a zero diagonal at step 0 under non-zero off-diagonals (the early-out)")
    reach(int((np.abs(d) == np.abs(d[:, :1])).all(1).sum()), 4000, "pivot ties at step 0")
    reach(int(np.isnan(A).any(1).sum() + np.isinf(A).any(1).sum()), 200, "non-finite entries")
    ref = orc.ldlt6_solve_batch(A, b)
    same(both_orders(probe, "ldlt6_solve", np.concatenate([A, b], 1), "ldlt6_solve"), ref, "ldlt6_solve", where)


def libm_agreement(probe, orc, x):
    """Per argument: whether the device's sinf and cosf both equal the running libm's."""
    ok = np.ones(len(x), bool)
    for name in ("sinf", "cosf"):
        got = probe(name, x[:, None])[:, 0]; ref = orc.libm_f32_batch(name, x)
        ok &= (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    return ok


def check_euler(probe, orc):
    (abg,), where = si.concat(si.euler_families(SEED))
    ref = orc.euler_xyz_matrix_batch(abg)
    got = both_orders(probe, "euler_xyz", abg, "euler_xyz")
    # From |half angle| = 120 on the header claims one ulp for sinf / cosf, not equality (check_sinf_cosf).  The rotation built from
    # them is the oracle's exactly where the device's six sines and cosines are libm's.  Where one of them is the neighbouring float, the
    # same composition is held to a bound: each of the six values is at most d = 2^-23 off (an ulp of a value in [-1, 1]); a quaternion
    # component is a sum of two products of three of them, at most 6 d off to first order; a matrix entry is 1 or 0 plus or minus twice
    # a sum of two products of two components of modulus <= 1, at most 2 * 2 * 2 * 6 d = 48 d off; the roundings of either evaluation
    # (about ten operations on values <= 2) add less than 16 d.  So |device - oracle| <= 64 * 2^-23 per entry.
    with np.errstate(invalid="ignore", over="ignore"):
        half = (np.float32(0.5) * abg).astype(np.float32)
        large = np.isfinite(half) & (np.abs(half) >= 120)
    exact = np.ones(len(abg), bool)
    rows = np.flatnonzero(large.any(1))
    agree = libm_agreement(probe, orc, half[rows].reshape(-1)).reshape(-1, 3).all(1)
    exact[rows[~agree]] = False
    reach(int(agree.sum()), len(rows) // 2, "rotations from half angles >= 120 whose sines and cosines are libm's")
    reach(int(np.isnan(ref).any(1).sum()), 12, "non-finite angles")
    same(got[exact], ref[exact], "euler_xyz")
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    off = np.abs(got[~exact].astype(np.float64) - ref[~exact])
    print("euler_xyz: %d rotations from a sine or cosine one ulp from libm's, largest entry difference %.3g" % (len(off), off.max() if len(off) else 0.0))
    assert np.isfinite(got[~exact]).all() and (off <= 64 * 2.0 ** -23).all()


def check_sinf_cosf(probe, orc):
    """Returns how many of the arguments from 120 on differ (by one ulp) in sinf resp. cosf."""
    lo = si.angles_below_120(); hi = si.angles_from_120(SEED); nf = si.angles_nonfinite()
    differ = {}
    for name in ("sinf", "cosf"):
        ref = orc.libm_f32_batch(name, lo)
        same(both_orders(probe, name, lo[:, None], name)[:, 0], ref, name + " below 120")
        got = both_orders(probe, name, nf[:, None], name)[:, 0]
        assert np.isnan(got).all() and np.isnan(orc.libm_f32_batch(name, nf)).all()
        # |x| >= 120: the device rounds the double function once (error <= 0.5 ulp + 2^-29), glibc's sinf / cosf document < 1 ulp:
        # the two are at most one float apart.  Distance in floats through the ordered integer image of the bit patterns.
        got = both_orders(probe, name, hi[:, None], name)[:, 0]; ref = orc.libm_f32_batch(name, hi)
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        key = lambda f: np.where(f.view(np.int32) < 0, np.int64(-1) - (f.view(np.int32).astype(np.int64) & 0x7fffffff), f.view(np.int32).astype(np.int64))
        dist = np.abs(key(got) - key(ref))
        dist[(got == 0) & (ref == 0)] = 0
        differ[name] = int((dist != 0).sum())
        print("%s: %d of %d arguments from 120 on differ from libm, all by %d ulp at most" % (name, differ[name], len(hi), dist.max()))
        assert dist.max() <= 1, (name, hi[dist.argmax()], got[dist.argmax()], ref[dist.argmax()])
    return differ


def check_atanf(probe, orc):
    x = si.atanf_set()
    same(both_orders(probe, "atanf", x[:, None], "atanf")[:, 0], orc.libm_f32_batch("atanf", x), "atanf")


def check_atan2f(probe, orc, n=20000000):
    yx = si.atan2f_pairs(n, SEED)
    same(both_orders(probe, "atan2f", yx, "atan2f")[:, 0], orc.libm_f32_batch("atan2f", yx[:, 0], yx[:, 1]), "atan2f")


def check_mul44(probe, orc):
    (A, B), where = si.concat(si.mul44_families(SEED))
    ref = orc.mul44_batch(A, B)
    reach(int(np.isnan(ref).any(1).sum()), 500, "NaN products")
    same(both_orders(probe, "mul44", np.concatenate([A, B], 1), "mul44"), ref, "mul44", where)


def check_hypothesis(probe, orc):
    (s, t), where = si.concat(si.triple_families(SEED + 1))
    T = orc.hypothesis_from_pairs_batch(s, t).reshape(-1, 4, 4)                        # column-major: T[:, c, r]
    ref = np.ascontiguousarray(np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, 3, :3]], 1))
    reach(int(np.isnan(ref).any(1).sum()), 300, "NaN hypotheses")
    U, S, V, sweeps = orc.jacobi_svd3_batch(si.colmajor9(si.hyp_H(s, t)))
    assert sweeps.max() < 64
    with np.errstate(invalid="ignore"):
        reach(int((S[:, 1] <= 1e-4 * S[:, 0]).sum()), 12000, "H of rank <= 1 to 1e-4 (collinear or coincident points)")
        reach(int((S[:, 0] == 0).sum()), 500, "H exactly zero")
        Um = U.reshape(-1, 3, 3).transpose(0, 2, 1).astype(np.float64); Vm = V.reshape(-1, 3, 3).transpose(0, 2, 1).astype(np.float64)
        reach(int((np.linalg.det(np.nan_to_num(Vm @ Um.transpose(0, 2, 1))) < -0.5).sum()), 3000, "det(V U^T) < 0 before the flip")
    same(both_orders(probe, "ransac_hypothesis", si.pq24(s, t), "ransac_hypothesis_lane"), ref, "ransac_hypothesis_lane (R | t)", where)


# ------------------------------------------------------------------------------------------------ on the device
@pytest.fixture(scope="module")
def probe(ctx):
    return lambda op, x: ctx.study_probe(op, x)


@pytest.mark.study
def test_probed_svd3(probe, orc, synth):
    check_svd3(probe, orc, synth)


@pytest.mark.study
def test_probed_kabsch_rotation(probe, orc, synth):
    check_kabsch(probe, orc, synth)


@pytest.mark.study
def test_probed_smallest_eigvec3(probe, orc, synth):
    check_eigvec(probe, orc, synth)


@pytest.mark.study
def test_probed_ldlt6_solve(probe, orc):
    check_ldlt(probe, orc)


@pytest.mark.study
def test_probed_euler_xyz(probe, orc):
    check_euler(probe, orc)


@pytest.mark.study
def test_probed_mul44(probe, orc):
    check_mul44(probe, orc)


@pytest.mark.study
def test_probed_sinf_cosf(probe, orc):
    check_sinf_cosf(probe, orc)


@pytest.mark.study
def test_probed_atanf(probe, orc):
    check_atanf(probe, orc)


@pytest.mark.study
def test_probed_atan2f(probe, orc):
    check_atan2f(probe, orc)


@pytest.mark.study
def test_probed_ransac_hypothesis_lane(probe, orc):
    check_hypothesis(probe, orc)


@pytest.mark.study
def test_probed_entry_point_arguments(ctx, tdv):
    """TDV_ERR_BAD_ARG (-2, include/tdv_hip.h) for an unknown op, n < 0 or a NULL pointer with n > 0, before anything is launched or
    allocated; n == 0 does nothing, whatever the pointers."""
    import torch
    BAD_ARG = -2
    f = tdv.lib().tdv_study_probe
    buf = torch.zeros(64, dtype=torch.float32, device=torch.device("cuda", ctx.device))
    p = C.c_void_p(buf.data_ptr())
    for op, n in ((-1, 1), (11, 1), (99, 1), (0, -1), (10, -5), (3, -(1 << 40))):
        assert f(ctx._h, op, C.c_longlong(n), p, p) == BAD_ARG, (op, n)
    for op in range(11):
        assert f(ctx._h, op, C.c_longlong(1), None, p) == BAD_ARG, op
        assert f(ctx._h, op, C.c_longlong(1), p, None) == BAD_ARG, op
        assert f(ctx._h, op, C.c_longlong(0), None, None) == 0
    assert f(None, 0, C.c_longlong(1), p, p) == BAD_ARG
    assert ctx.study_probe("svd3", np.zeros((0, 9), np.float32)).shape == (0, 21)
    assert not buf.cpu().numpy().any()


def test_product_library_has_no_probe(ctx, tdv):
    assert not tdv.STUDY_BUILD, "this process must run the PRODUCT library"
    assert not hasattr(tdv.lib(), "tdv_study_probe")
    with pytest.raises(tdv.TdvError):
        ctx.study_probe("svd3", np.zeros((1, 9), np.float32))
