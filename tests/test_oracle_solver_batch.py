"""The oracle's batch solver exports (oracle.cpp: orc_*_batch) give the single-call exports' bytes, problem by problem, on a sample of
every family of tests/solver_inputs.py; and the conditions tests/test_gpu_solver_probe.py places on those families hold on the oracle
alone: its unbounded Jacobi sweep loop stays below the device's 64-sweep guard on EVERY input (so the guard never decides a
comparison), and the QR iteration both converges and gives up within them."""
import numpy as np

import solver_inputs as si

SEED = 20240          # tests/test_gpu_solver_probe.py's


def _sample(arrays, count, seed=1):
    idx = np.sort(np.random.default_rng(seed).choice(len(arrays[0]), min(count, len(arrays[0])), replace=False))
    return [a[idx] for a in arrays]


def _cm(a9):
    return a9.reshape(3, 3).T              # the single calls take ordinary matrices


def test_batch_exports_equal_the_single_calls(orc, synth):
    (M,), _ = si.concat(si.mat3_families(SEED, synth, orc))
    (A,) = _sample([si.colmajor9(M)], 4000)
    U, S, V, sweeps = orc.jacobi_svd3_batch(A)
    R = orc.kabsch_rotation_batch(A)
    assert sweeps.min() >= 1
    for i, a in enumerate(A):
        u, s, v = orc.jacobi_svd3(_cm(a))
        assert (u.T.tobytes(), s.tobytes(), v.T.tobytes()) == (U[i].tobytes(), S[i].tobytes(), V[i].tobytes()), i
        assert orc.kabsch_rotation(_cm(a)).T.tobytes() == R[i].tobytes(), i
    (M,), _ = si.concat(si.sym3_families(SEED, synth, orc))
    (A,) = _sample([si.colmajor9(M)], 4000)
    w, V, rc, iters = orc.self_adjoint_eig3_batch(A)
    for i, a in enumerate(A):
        w1, v1, rc1 = orc.self_adjoint_eig3(_cm(a))
        assert (w1.tobytes(), v1.T.tobytes(), rc1) == (w[i].tobytes(), V[i].tobytes(), rc[i]), i
    assert np.array_equal(rc != 0, iters == 91)
    (A, b), _ = si.concat(si.ldlt_families(SEED, orc))
    A, b = _sample([A, b], 4000)
    x = orc.ldlt6_solve_batch(A, b)
    for i in range(len(A)):
        assert orc.ldlt6_solve(A[i], b[i]).tobytes() == x[i].tobytes(), i
    (abg,), _ = si.concat(si.euler_families(SEED))
    (abg,) = _sample([abg], 4000)
    R = orc.euler_xyz_matrix_batch(abg)
    for i, (a, b_, g) in enumerate(abg):
        assert orc.euler_xyz_matrix(a, b_, g).T.tobytes() == R[i].tobytes(), i
    (s, t), _ = si.concat(si.triple_families(SEED + 1))
    s, t = _sample([s, t], 4000)
    T = orc.hypothesis_from_pairs_batch(s, t)
    for i in range(len(s)):
        assert orc.hypothesis_from_pairs(s[i], t[i]).T.tobytes() == T[i].tobytes(), i
    (A, B), _ = si.concat(si.mul44_families(SEED))
    A, B = _sample([A, B], 3000)
    Cm = orc.mul44_batch(A, B)
    for i in range(len(A)):
        assert orc.mul44(A[i], B[i]).tobytes() == Cm[i].tobytes(), i
    # the 4x4 product is the one pose composition uses: extrinsics * I
    E = np.arange(16, dtype=np.float32).reshape(4, 4) + np.float32(0.5)
    assert orc.from_colmajor16(orc.mul44(orc.to_colmajor16(E), orc.to_colmajor16(np.eye(4)))).tobytes() == E.tobytes()


def test_libm_batch_is_the_running_libm(orc):
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    x = np.concatenate([si.angles_below_120()[::50021], si.angles_from_120(SEED)[::97], si.angles_nonfinite()])
    y = np.roll(x, 7)
    for name in ("sinf", "cosf", "atanf", "atan2f"):
        f = getattr(m, name); f.restype = ctypes.c_float; f.argtypes = [ctypes.c_float] * (2 if name == "atan2f" else 1)
        got = orc.libm_f32_batch(name, x, y if name == "atan2f" else None)
        with np.errstate(all="ignore"):
            ref = np.array([f(float(a), float(b)) if name == "atan2f" else f(float(a)) for a, b in zip(x, y)], np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and got[~np.isnan(got)].tobytes() == ref[~np.isnan(ref)].tobytes(), name
    assert orc.lib().orc_libm_f32_batch(4, ctypes.c_longlong(0), None, None, None) == 1


def test_every_input_stays_below_the_sweep_guard_and_both_qr_exits_are_reached(orc, synth):
    (M,), _ = si.concat(si.mat3_families(SEED, synth, orc))
    (s, t), _ = si.concat(si.triple_families(SEED + 1))
    sweeps = np.concatenate([orc.jacobi_svd3_batch(si.colmajor9(M))[3], orc.jacobi_svd3_batch(si.colmajor9(si.hyp_H(s, t)))[3]])
    print("Jacobi sweeps over %d inputs: max %d; histogram %s" % (len(sweeps), sweeps.max(), np.bincount(sweeps).tolist()))
    assert sweeps.max() < 64
    (M,), _ = si.concat(si.sym3_families(SEED, synth, orc))
    _, _, rc, iters = orc.self_adjoint_eig3_batch(si.colmajor9(M))
    print("QR steps over %d inputs: max %d among the converged, %d gave up" % (len(iters), iters[rc == 0].max(), int((rc != 0).sum())))
    assert (rc != 0).sum() >= 100 and (rc == 0).sum() >= 100000
    assert (~np.isfinite(M[rc != 0])).any(axis=(1, 2)).all(), "only NaN and infinite entries are known to exhaust the QR iteration"


def test_generators_are_deterministic(orc, synth):
    a = si.concat(si.ldlt_families(SEED, orc))[0]; b = si.concat(si.ldlt_families(SEED, orc))[0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert si.atan2f_pairs(1000, 3).tobytes() == si.atan2f_pairs(1000, 3).tobytes()
    assert not np.array_equal(si.permutation(1000), np.arange(1000)) and np.array_equal(si.permutation(1000), si.permutation(1000))
