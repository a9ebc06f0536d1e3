"""Adversarial inputs for the per-lane solvers (csrc/device_linalg.hpp), the libm restatement (csrc/libm_f32.hpp) and RANSAC's
hypothesis lane: the matrices, systems, triples and angles that tidy synthetic geometry never feeds them.  Everything is generated
from a seed; nothing is stored.  tests/test_gpu_solver_probe.py runs them on the device, tests/test_oracle_solver_batch.py on the
oracle alone.

A family is (name, arrays...).  3x3 matrices are [n,3,3] with M[r,c] here and cross to the libraries COLUMN-MAJOR through colmajor9;
6x6 systems are ([n,36] row-major, [n,6]); triples are ([n,9] three source points, [n,9] three target points)."""
import numpy as np

F = np.float32
FLT_MIN = np.float32(1.1754943508222875e-38)          # 2^-126
FLT_EPS = np.float32(1.1920928955078125e-07)          # 2^-23
DENORM_MIN = np.float32(1.401298464324817e-45)        # 2^-149
SPECIALS = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), DENORM_MIN]


def ulps(x, k):
    """x moved by k units in the last place (x > 0 and finite; the result may be denormal)."""
    x = np.asarray(x, F)
    return (x.view(np.int32) + np.asarray(k, np.int32)).view(F)


def colmajor9(M):
    return np.ascontiguousarray(np.asarray(M, F).transpose(0, 2, 1)).reshape(-1, 9)


def lower6(M):
    """a00 a10 a20 a11 a21 a22: what smallest_eigvec3 reads."""
    M = np.asarray(M, F)
    return np.ascontiguousarray(np.stack([M[:, 0, 0], M[:, 1, 0], M[:, 2, 0], M[:, 1, 1], M[:, 2, 1], M[:, 2, 2]], 1))


def mirror_lower(M):
    """The symmetric matrix with M's lower triangle (NaN and zero signs kept)."""
    M = np.asarray(M, F).copy()
    for r, c in ((0, 1), (0, 2), (1, 2)):
        M[:, r, c] = M[:, c, r]
    return M


def concat(families):
    """(arrays concatenated along the problems, {name: slice})."""
    where, start = {}, 0
    for f in families:
        where[f[0]] = slice(start, start + len(f[1])); start += len(f[1])
    k = len(families[0]) - 1
    return tuple(np.ascontiguousarray(np.concatenate([f[1 + j] for f in families])) for j in range(k)), where


def permutation(n, seed=12345):
    """The fixed pseudo-random order of the second device run."""
    return np.random.default_rng(seed).permutation(n)


def _orth(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def _signed_perms(rng, n):
    P = np.zeros((n, 3, 3))
    for i in range(n):
        P[i, np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
    return P


def _ints(rng, shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


def _poke(bases, positions):
    """Every base with exactly one entry (each of `positions`, flat index into the base's trailing axes) set to each special."""
    flat = bases.reshape(len(bases), -1)
    out = []
    for b in flat:
        for p in positions:
            for v in SPECIALS:
                m = b.copy(); m[p] = v; out.append(m)
    return np.array(out, F).reshape((-1,) + bases.shape[1:])


# ------------------------------------------------------------------------------------------------ 3x3
def hyp_H(s9, t9):
    """H of RANSAC's hypothesis (registration.cpp:242-254) in the solvers' arithmetic: float32, 3-term sums as c0 + (c1 + c2)."""
    with np.errstate(all="ignore"):
        s = np.asarray(s9, F).reshape(-1, 3, 3); t = np.asarray(t9, F).reshape(-1, 3, 3)          # [n, point, coordinate]
        sc = (s[:, 0] + (s[:, 1] + s[:, 2])) / F(3); tc = (t[:, 0] + (t[:, 1] + t[:, 2])) / F(3)
        S = s - sc[:, None, :]; T = t - tc[:, None, :]                                            # [n, k, r]
        H = np.empty((len(s), 3, 3), F)
        for r in range(3):
            for c in range(3):
                H[:, r, c] = S[:, 0, r] * T[:, 0, c] + (S[:, 1, r] * T[:, 1, c] + S[:, 2, r] * T[:, 2, c])
    return H


def knn_covariances(points, k=30, count=1500, seed=0):
    """Covariances of the k nearest neighbours of `count` of the points (estimateNormals' matrices, float32)."""
    p = np.asarray(points, F)
    idx = np.random.default_rng(seed).choice(len(p), min(count, len(p)), replace=False)
    d2 = ((p[idx, None, :].astype(np.float64) - p[None, :, :]) ** 2).sum(-1)
    nb = p[np.argsort(d2, axis=1, kind="stable")[:, :k]]                                          # [count, k, 3]
    c = (nb.sum(1, dtype=F) / F(k)).astype(F)
    d = nb - c[:, None, :]
    return (np.einsum("nkr,nkc->nrc", d, d).astype(F) / F(k)).astype(F)


def mat3_families(seed, synth, orc):
    """General 3x3 matrices for svd3 / kabsch_rotation; mirror_lower of each goes to smallest_eigvec3 as well."""
    rng = np.random.default_rng(seed)
    fam = []
    with np.errstate(all="ignore"):
        e = np.repeat(np.arange(-140, 126), 110)
        fam.append(("gauss_scaled", np.ldexp(rng.normal(size=(len(e), 3, 3)), e[:, None, None]).astype(F)))
        g = rng.normal(size=(6000, 3, 3))
        which = rng.integers(0, 3, 6000); sgn = rng.choice([-60, 60], 6000); row = rng.random(6000) < 0.5
        for i in range(6000):
            if row[i]:
                g[i, which[i], :] = np.ldexp(g[i, which[i], :], sgn[i])
            else:
                g[i, :, which[i]] = np.ldexp(g[i, :, which[i]], sgn[i])
        fam.append(("mixed_scale", g.astype(F)))
        z = np.zeros((8, 3, 3), F); z[1] = -0.0; z[2, 0, 0] = -0.0; z[3, 2, 1] = -0.0; z[4, 0, 2] = -0.0
        fam.append(("rank0", z))
        u, v = _ints(rng, (3000, 3, 1)), _ints(rng, (3000, 1, 3))
        sc = np.ldexp(1.0, rng.choice([0, 0, -40, 40, -100, 100], 3000))[:, None, None]
        fam.append(("rank1", (u * v * sc).astype(F)))
        u2, v2 = _ints(rng, (3000, 3, 1)), _ints(rng, (3000, 1, 3))
        fam.append(("rank2", ((u * v + u2 * v2) * sc).astype(F)))
        c = np.ldexp(rng.uniform(1, 2, 3000), rng.integers(-20, 21, 3000))[:, None, None]
        Q = _orth(rng, 3000)
        fam.append(("scaled_orthogonal", (c * Q).astype(F)))
        a, b = rng.uniform(0.1, 4, 3000), rng.uniform(0.1, 4, 3000)
        a[:600] = np.round(a[:600] * 4) / 4; b[:600] = np.round(b[:600] * 4) / 4                  # exact quarters as well
        kind = rng.integers(0, 3, 3000)
        D = np.zeros((3000, 3, 3))
        D[:, 0, 0] = a; D[:, 1, 1] = np.where(kind == 1, b, a); D[:, 2, 2] = np.where(kind == 2, a, b)   # (a,a,b) (a,b,b) (a,a,a)
        fam.append(("repeated_diag", (_signed_perms(rng, 3000) @ D @ _signed_perms(rng, 3000)).astype(F)))
        g = rng.normal(size=(2000, 3, 3)); g[np.linalg.det(g) > 0, 0, :] *= -1
        fam.append(("improper", g.astype(F)))
        fam.append(("reflections", (Q[:1500] * np.array([1, 1, -1.0])).astype(F)))
        near = (u[:2000] * v[:2000] + u2[:2000] * v2[:2000]).astype(F)                             # rank <= 2, then one entry moved by a few ulps
        pos = rng.integers(0, 9, 2000); k = rng.integers(-3, 4, 2000)
        nf = near.reshape(-1, 9)
        for i in range(2000):
            x = nf[i, pos[i]]
            nf[i, pos[i]] = ulps(abs(x), k[i]) * (F(-1) if x < 0 else F(1)) if x != 0 else F(k[i]) * FLT_EPS
        fam.append(("det_near_zero", near))
        # off-diagonal entries around the sweep's two cut-offs.  2 eps maxDiag: a diagonal of order 1, one or two off-diagonal
        # entries k ulps from 2 eps, the whole at scales 1, 2^40, 2^-40.
        cut = []
        for s in (0, 40, -40):
            for (p, q) in ((1, 0), (0, 1), (2, 0), (0, 2), (2, 1), (1, 2)):
                for k in range(-4, 5):
                    for sg in (1, -1):
                        for d in ((1.0, 0.5, 0.25), (0.5, 1.0, 1.0), (1.0, 1.0, 1.0), (-1.0, 0.75, 0.0)):
                            m = np.diag(np.array(d, F)); m[p, q] = F(sg) * ulps(F(2) * FLT_EPS * F(max(abs(x) for x in d)), k)
                            cut.append(np.ldexp(m, s).astype(F))
                            m2 = m.copy(); m2[q, p] = ulps(F(2) * FLT_EPS, -k)
                            cut.append(np.ldexp(m2, s).astype(F))
        fam.append(("cutoff_2eps_maxdiag", np.array(cut, F)))
        # FLT_MIN: the threshold is FLT_MIN only when the diagonal is below 2^-104 of the largest entry, so the diagonal is zero or
        # denormal here and an off-diagonal 1 pins the scale; the small entries come from a palette around FLT_MIN and FLT_MIN / 2
        # (jacobi_sym's 2|y| < FLT_MIN), both signs, and a few sizes between.
        pal = [F(0)] + [ulps(FLT_MIN, k) for k in range(-4, 5)] + [ulps(FLT_MIN * F(0.5), k) for k in range(-4, 5)] + \
              [F(2.0) ** -100, F(2.0) ** -110, F(2.0) ** -120, DENORM_MIN, F(2.0) ** -140]
        pal = np.array(pal + [-x for x in pal], F)
        m = pal[rng.integers(0, len(pal), (9000, 3, 3))]
        big = rng.integers(0, 6, 9000)
        offd = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
        for i in range(9000):
            m[i][offd[big[i]]] = F(1) if i % 3 else F(-1)
        m[6000:] = np.ldexp(m[6000:], np.where(np.arange(3000) % 2, 40, -20)[:, None, None]).astype(F)
        fam.append(("cutoff_flt_min", m))
        bases = np.concatenate([rng.normal(size=(12, 3, 3)), np.diag([2.0, 1.0, 0.5])[None], np.zeros((1, 3, 3)),
                                np.ones((1, 3, 3)), _orth(rng, 3)]).astype(F)
        fam.append(("one_special_entry", _poke(bases, range(9))))
        # a special value on the diagonal beside a 2x2 block whose off-diagonals lie between FLT_MIN and 2 eps maxDiag: whether the
        # block is rotated depends on how the maximum of the diagonal treats the NaN
        blk = []
        for v in SPECIALS:
            for pos in range(3):
                for e in (1e-8, 1e-10, 1e-20, 1e-30, -1e-9):
                    for d in ((1.0, 0.5, 0.25), (0.25, 0.5, 1.0), (0.5, 1.0, 0.75)):
                        m = np.diag(np.array(d, F)); m[pos, pos] = v
                        p, q = [i for i in range(3) if i != pos]
                        m[p, q] = F(e); m[q, p] = F(e) * F(0.5)
                        blk.append(m)
        fam.append(("special_diagonal_beside_a_block", np.array(blk, F)))
        s9, t9 = concat(triple_families(seed + 1))[0]
        fam.append(("hypothesis_H", hyp_H(s9, t9)))
        pts, _ = synth.sample_object(4000, 11)
        fam.append(("knn_covariance", knn_covariances(pts, 30, 1500, seed)))
        model, _ = orc.demo_model()
        fam.append(("planar_grid_covariance", knn_covariances(model, 30, 800, seed)))
    return fam


def sym3_families(seed, synth, orc):
    """Symmetric 3x3 matrices for smallest_eigvec3: the lower triangles of mat3_families, and what only a symmetric solver meets."""
    rng = np.random.default_rng(seed + 7)
    fam = [("sym_" + n, mirror_lower(M)) for n, M in mat3_families(seed, synth, orc)]
    with np.errstate(all="ignore"):
        # already tridiagonal or diagonal: a20 * a20 <= FLT_MIN (a20 zero, denormal, or k ulps around 2^-63)
        a20 = np.array([F(0), F(-0.0), DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN] +
                       [s * ulps(F(2.0) ** -63, k) for k in range(-4, 5) for s in (F(1), F(-1))], F)
        m = rng.normal(size=(len(a20) * 120, 3, 3)).astype(F)
        m[::3, 1, 0] = 0; m[1::6, 2, 1] = 0                                                     # diagonal blocks too
        m[:, 2, 0] = np.tile(a20, 120)
        m[:, 0, 0] = np.where(np.arange(len(m)) % 2, F(1), m[:, 0, 0])                           # scale 1: a20 is divided by exactly 1
        m[np.arange(len(m)) % 2 == 1] = np.clip(m[np.arange(len(m)) % 2 == 1], -1, 1)
        m[:, 2, 0] = np.tile(a20, 120)
        fam.append(("tridiagonal_a20_cutoff", mirror_lower(m)))
        a, b = rng.uniform(-3, 3, 4000), rng.uniform(-3, 3, 4000)
        D = np.zeros((4000, 3, 3)); D[:, 0, 0] = a; D[:, 1, 1] = a; D[:, 2, 2] = np.where(np.arange(4000) % 4 == 0, a, b)
        Q = _orth(rng, 4000); Q[:1500] = _signed_perms(rng, 1500)
        fam.append(("equal_eigenvalues", mirror_lower((Q @ D @ Q.transpose(0, 2, 1)).astype(F))))
        blk = np.zeros((1500, 3, 3)); c = rng.uniform(-2, 2, 1500); o = rng.uniform(-2, 2, 1500)
        blk[:, 0, 0] = c + o; blk[:, 1, 1] = c; blk[:, 2, 2] = c; blk[:, 2, 1] = o; blk[:, 1, 2] = o     # eigenvalues c+o, c+o, c-o
        P = _signed_perms(rng, 1500)
        fam.append(("equal_eigenvalues_block", mirror_lower((P @ blk @ P.transpose(0, 2, 1)).astype(F))))
        # the Wilkinson shift's e2 == 0: an off-diagonal e that survives both cut-offs (|e| >= FLT_MIN and (e / eps)^2 above the sum
        # of its two diagonal entries) while e * e underflows to zero, i.e. 2^-97 <= |e| < 2^-75 beside a zero or denormal diagonal
        # pair; the third diagonal entry, 1, pins the scale.  Both positions of the pair.
        rows = []
        for ex in (-76, -78, -80, -85, -90, -95, -97):
            for sg in (1.0, -1.0):
                for da in (2.0 ** -130, 2.0 ** -140, float(DENORM_MIN), -(2.0 ** -135), 0.0):
                    for db in (0.0, float(DENORM_MIN), -float(DENORM_MIN), 2.0 ** -145):
                        for lay in (0, 1):
                            m = np.zeros((3, 3))
                            i, j, k = (1, 2, 0) if lay == 0 else (0, 1, 2)
                            m[i, i] = da; m[j, j] = db; m[j, i] = m[i, j] = sg * 2.0 ** ex; m[k, k] = 1.0 if (ex + lay) % 2 else -1.0
                            rows.append(m)
        fam.append(("wilkinson_e2_underflow", np.array(rows).astype(F)))
    return fam


def reaches_e2_underflow(M):
    """Symmetric matrices that by their entries alone take the e2 == 0 branch of the QR step's shift at its first step: scale 1 from
    one diagonal entry, the other two rows a 2x2 block [[a, e], [e, b]] apart from it, with FLT_MIN <= |e|, (e * 2^23)^2 > |a| + |b|
    (e survives the cut-offs), a != b (td != 0) and e * e == 0 in float32."""
    M = np.asarray(M, F)
    out = np.zeros(len(M), bool)
    with np.errstate(all="ignore"):
        for (i, j, k) in ((1, 2, 0), (0, 1, 2)):
            a, b, e = M[:, i, i], M[:, j, j], M[:, j, i]
            alone = (np.abs(M[:, k, k]) == 1) & (M[:, k, i] == 0) & (M[:, k, j] == 0) & (M[:, i, k] == 0) & (M[:, j, k] == 0)
            sc = (F(2.0) ** 23 * e).astype(F)
            out |= alone & (np.abs(e) >= FLT_MIN) & ((sc * sc).astype(F) > (np.abs(a) + np.abs(b)).astype(F)) & (a != b) & ((e * e).astype(F) == 0) \
                & (np.abs(a) <= 1) & (np.abs(b) <= 1)
    return out


# ------------------------------------------------------------------------------------------------ three pairs
def triple_families(seed):
    rng = np.random.default_rng(seed)
    fam = []
    with np.errstate(all="ignore"):
        def moved(s, noise=1e-3):
            R = _orth(rng, len(s)); R[np.linalg.det(R) < 0, :, 0] *= -1
            return np.einsum("nrc,nkc->nkr", R, s) + rng.uniform(-1, 1, (len(s), 1, 3)) + rng.normal(0, noise, s.shape)
        for name, off in (("generic_0m", 0.0), ("generic_250m", 250.0), ("generic_100km", 1e5)):
            s = rng.uniform(-0.1, 0.1, (6000, 3, 3)) + off * np.array([0.6, -0.64, 0.48])
            fam.append((name, s.astype(F).reshape(-1, 9), moved(s).astype(F).reshape(-1, 9)))
        a = _ints(rng, (4000, 1, 3), -8, 8); d = _ints(rng, (4000, 1, 3), -3, 3); k = np.array([0.0, 1.0, 2.0])[None, :, None]
        k = k * rng.choice([1.0, 2.0, -1.0], (4000, 1, 1))
        s = ((a + k * d) * 0.125).astype(F)
        fam.append(("collinear_exact", s.reshape(-1, 9), moved(s, 0).astype(F).reshape(-1, 9)))
        s1 = s.copy().reshape(-1, 9); pos = rng.integers(0, 9, 4000)
        x = s1[np.arange(4000), pos]
        s1[np.arange(4000), pos] = np.where(x == 0, DENORM_MIN, np.nextafter(x, np.where(rng.random(4000) < 0.5, F(np.inf), F(-np.inf)), dtype=F))
        fam.append(("collinear_one_ulp", s1, moved(s, 0).astype(F).reshape(-1, 9)))
        s = rng.uniform(-1, 1, (3000, 3, 3)); t = moved(s)
        s[:1000, 1] = s[:1000, 0]; s[1000:2000, 2] = s[1000:2000, 0]; s[2000:, 1] = s[2000:, 0]; s[2000:, 2] = s[2000:, 0]
        fam.append(("coincident_sources", s.astype(F).reshape(-1, 9), t.astype(F).reshape(-1, 9)))
        s = rng.uniform(-1, 1, (3000, 3, 3)); t = moved(s)
        t[:1000, 1] = t[:1000, 0]; t[1000:2000, 2] = t[1000:2000, 1]; t[2000:, 1] = t[2000:, 0]; t[2000:, 2] = t[2000:, 0]
        t[2500:] = 0; s[2800:] = 0
        fam.append(("coincident_targets", s.astype(F).reshape(-1, 9), t.astype(F).reshape(-1, 9)))
        s = rng.uniform(-1, 1, (4000, 3, 3)); t = moved(s, 1e-4) * np.array([1.0, 1.0, -1.0])
        s[:1000] += rng.normal(size=(1000, 1, 3)) * 3                                            # a mirrored triple seen off its own plane
        fam.append(("mirrored_targets", s.astype(F).reshape(-1, 9), t.astype(F).reshape(-1, 9)))
        s = rng.uniform(-1, 1, (4000, 3, 3)); t = moved(s)
        es, et = rng.choice([-60, 0, 60], 4000), rng.choice([-60, 0, 60], 4000)
        fam.append(("scaled_2^60", np.ldexp(s, es[:, None, None]).astype(F).reshape(-1, 9), np.ldexp(t, et[:, None, None]).astype(F).reshape(-1, 9)))
        s = rng.uniform(-1, 1, (12, 3, 3)); t = moved(s)
        st = np.concatenate([s.reshape(12, 9), t.reshape(12, 9)], 1).astype(F)
        sp = np.array([np.nan, np.inf, -np.inf], F)
        rows = []
        for b in st:
            for p in range(18):
                for v in sp:
                    r = b.copy(); r[p] = v; rows.append(r)
        rows = np.array(rows, F)
        fam.append(("one_nonfinite_coordinate", np.ascontiguousarray(rows[:, :9]), np.ascontiguousarray(rows[:, 9:])))
    return fam


def pq24(s9, t9):
    """Three pairs as the probe's op takes them: three records px py pz qx qy qz 0 0."""
    n = len(s9)
    out = np.zeros((n, 3, 8), F)
    out[:, :, 0:3] = np.asarray(s9, F).reshape(n, 3, 3); out[:, :, 3:6] = np.asarray(t9, F).reshape(n, 3, 3)
    return out.reshape(n, 24)


# ------------------------------------------------------------------------------------------------ 6x6
def icp_planar_trace(orc):
    """Every normal system the oracle's point-to-plane ICP forms on the planar C1 model (tests/test_gpu_icp_reference_order.py:
    test_demo_model_rank3_normal_matrix): A = J^T J [k,36], b = -J^T r [k,6], one per iteration."""
    g = (np.arange(40, dtype=F) * F(0.005) - F(0.1)).astype(F)
    tgt = np.stack([np.repeat(g, 40), np.tile(g, 40), np.zeros(1600, F)], 1).astype(F)
    nrm = np.tile(np.array([0, 0, 1], F), (1600, 1))
    rng = np.random.default_rng(3)
    src = (tgt[rng.integers(0, 1600, 900)] + rng.normal(0, 2e-4, (900, 3))).astype(F)
    T0 = np.eye(4, dtype=F); T0[:3, 3] = [0.0006, -0.0004, 0.0011]
    ref = orc.icp(src, tgt, nrm, T0, 0.002, 15, True, trace=True)
    Ts = [T0] + [orc.from_colmajor16(row[:16]) for row in ref["trace"]]
    A, b = [], []
    for T in Ts[:-1]:
        c = orc.icp_correspondences(src, tgt, nrm, T, 0.002, True)
        A.append(c["ATA"].reshape(36)); b.append(-c["ATb"])
    return np.array(A, F), np.array(b, F)


def ldlt_families(seed, orc):
    rng = np.random.default_rng(seed)
    fam = []
    with np.errstate(all="ignore"):
        for r in range(6, -1, -1):
            n = 2500
            J = _ints(rng, (n, 9, 6), -3, 3) if r == 6 else _ints(rng, (n, 9, max(r, 1)), -2, 2) @ _ints(rng, (n, max(r, 1), 6), -2, 2) * (r > 0)
            res = _ints(rng, (n, 9, 1), -5, 5)
            A = J.transpose(0, 2, 1) @ J; b = (J.transpose(0, 2, 1) @ res)[:, :, 0]
            if r == 0:
                b = _ints(rng, (n, 6), -5, 5)
            fam.append(("JtJ_rank%d" % r, A.astype(F).reshape(n, 36), b.astype(F)))
        # a full-rank integer block on some of the rows and columns, exact zeros elsewhere: zero pivots past step 0 (the planar case's shape)
        n = 6000
        A = np.zeros((n, 6, 6)); b = _ints(rng, (n, 6), -5, 5)
        for i in range(n):
            r = 1 + i % 5
            idx = np.sort(rng.choice(6, r, replace=False))
            J = _ints(rng, (r + 3, r), -3, 3)
            A[i][np.ix_(idx, idx)] = J.T @ J
        fam.append(("embedded_block", A.astype(F).reshape(n, 36), b.astype(F)))
        # equal diagonals at every step: (c - o) I + o 1 1^T keeps that shape under elimination; c I; and equal diagonals over random off-diagonals
        n = 4500
        c = np.round(rng.uniform(1, 8, n) * 8) / 8; o = np.round(rng.uniform(-1, 1, n) * 8) / 8
        A = o[:, None, None] * np.ones((n, 6, 6)) + (c - o)[:, None, None] * np.eye(6)
        A[1500:3000] = c[1500:3000, None, None] * np.eye(6)
        g = rng.normal(size=(1500, 6, 6)); g = g + g.transpose(0, 2, 1)
        g[:, np.arange(6), np.arange(6)] = c[3000:, None]
        A[3000:] = g
        fam.append(("equal_diagonals", A.astype(F).reshape(n, 36), rng.normal(size=(n, 6)).astype(F)))
        g = rng.normal(size=(2000, 6, 6)); g = g + g.transpose(0, 2, 1)
        g[:, np.arange(6), np.arange(6)] = 0.0
        g[1000:] = np.round(g[1000:] * 4)
        fam.append(("zero_diagonal", g.astype(F).reshape(-1, 36), rng.normal(size=(2000, 6)).astype(F)))
        g = rng.normal(size=(5000, 6, 6)); g = g + g.transpose(0, 2, 1)
        fam.append(("indefinite", g.astype(F).reshape(-1, 36), rng.normal(size=(5000, 6)).astype(F)))
        g = rng.normal(size=(5000, 6, 6)); g = g @ g.transpose(0, 2, 1)
        g[2500:] -= np.eye(6) * 0.5
        e = rng.integers(-30, 31, (5000, 6))
        A = np.ldexp(g, e[:, :, None] + e[:, None, :])
        fam.append(("diagonals_2^60", A.astype(F).reshape(-1, 36), np.ldexp(rng.normal(size=(5000, 6)), e).astype(F)))
        # pivots k ulps around FLT_MIN (the pseudo-inverse's |d| > FLT_MIN) and around zero (denormal pivots are valid pivots)
        tiny = np.array([ulps(FLT_MIN, k) for k in range(-4, 5)] + [DENORM_MIN, F(2.0) ** -140, F(0), F(-0.0)], F)
        tiny = np.concatenate([tiny, -tiny])
        n = 4000
        d = rng.uniform(0.5, 2, (n, 6)).astype(F)
        cnt = 1 + rng.integers(0, 6, n)
        for i in range(n):
            d[i, rng.choice(6, cnt[i], replace=False)] = tiny[rng.integers(0, len(tiny), cnt[i])]
        A = np.zeros((n, 6, 6), F); A[:, np.arange(6), np.arange(6)] = d
        off = np.zeros((n, 6, 6), F)
        off[2000:, 1, 0] = off[2000:, 0, 1] = tiny[rng.integers(0, len(tiny), n - 2000)]
        off[3000:, 5, 2] = off[3000:, 2, 5] = F(0.25)
        fam.append(("flt_min_pivots", (A + off).reshape(n, 36), np.where(rng.random((n, 6)) < 0.3, tiny[rng.integers(0, len(tiny), (n, 6))], rng.normal(size=(n, 6))).astype(F)))
        g = rng.normal(size=(6, 6, 6)); g = (g @ g.transpose(0, 2, 1)).astype(F)
        g[4] = np.eye(6); g[5] = 0
        sysm = np.concatenate([g.reshape(6, 36), rng.normal(size=(6, 6)).astype(F)], 1)
        lower = [i * 6 + j for i in range(6) for j in range(i + 1)] + list(range(36, 42))
        poked = _poke(sysm, lower)
        for (i, j) in ((i, j) for i in range(6) for j in range(i)):                              # keep the matrix symmetric
            poked[:, j * 6 + i] = poked[:, i * 6 + j]
        fam.append(("one_special_entry", np.ascontiguousarray(poked[:, :36]), np.ascontiguousarray(poked[:, 36:])))
        A, b = icp_planar_trace(orc)
        fam.append(("icp_planar_trace", A, b))
    return fam


def has_zero_row(A36):
    """Systems with an all-zero row (and column) beside a non-zero entry: LDLT meets an exactly zero pivot after step 0."""
    A = np.asarray(A36).reshape(-1, 6, 6)
    return ((A == 0).all(2).any(1)) & (A[:, np.arange(6), np.arange(6)] != 0).any(1)


# ------------------------------------------------------------------------------------------------ angles, libm
def _bits(lo, hi, stride):
    return np.arange(np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32), stride, dtype=np.uint32).view(F)


def angles_below_120():
    """Every 7th float of [2^-13, 0.8), every 4,099th of the rest of [0, 120), both signs, and zeros and denormals."""
    x = np.concatenate([_bits(2.0 ** -13, 0.8, 7), _bits(0.0, 2.0 ** -13, 4099), _bits(0.8, 120.0, 4099),
                        np.array([0.0, DENORM_MIN, 1e-40, FLT_MIN, ulps(F(120.0), -1), ulps(F(0.8), -1), 0.8, 2.0 ** -13], F)])
    return np.concatenate([x, -x])


def angles_from_120(seed):
    """2^16 floats of [120, 2^127] with the exponent uniform, both signs."""
    rng = np.random.default_rng(seed)
    e = rng.integers(133, 254, 1 << 16).astype(np.uint32)                                       # 2^6 .. 2^126 as the leading power
    x = ((e << 23) | rng.integers(0, 1 << 23, 1 << 16).astype(np.uint32)).view(F)
    x = np.where(x < 120, F(120.0), x)
    x[:4] = [120.0, ulps(F(120.0), 1), 2.0 ** 127, 3.4028234663852886e38]
    return np.concatenate([x, -x]).astype(F)


def angles_nonfinite():
    return np.array([np.inf, -np.inf, np.nan, -np.nan], F)


def euler_families(seed):
    """euler_xyz halves its arguments: twice the angle sets, so that the half angles are the sets' members."""
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        x = (angles_below_120() * F(2)).astype(F)
        x = np.concatenate([x, x[: (-len(x)) % 3]])
        small = rng.permutation(x)[: 3 * (1 << 16)].reshape(-1, 3)
        big = (angles_from_120(seed) * F(2)).astype(F)
        fb = small[np.arange(len(big)) % len(small)].copy(); fb[np.arange(len(big)), np.arange(len(big)) % 3] = big
        nf = angles_nonfinite()
        fn = small[: 3 * len(nf)].copy(); fn[np.arange(len(fn)), np.arange(len(fn)) % 3] = np.repeat(nf, 3)
    return [("below_120", np.ascontiguousarray(x.reshape(-1, 3))), ("from_120", fb), ("nonfinite", fn),
            ("icp_increments", rng.normal(0, 3e-3, (20000, 3)).astype(F))]


def atanf_set():
    """Every 61st of the 2^32 bit patterns."""
    return np.arange(0, 1 << 32, 61, dtype=np.uint64).astype(np.uint32).view(F)


def atan2f_pairs(n, seed):
    """(y, x): uniform bit patterns, uniform values in (-1, 1), small exponents, x near +-1 (SPFH's shape) - a quarter each - and
    every pair from {+-0, +-denormal, +-1, +-inf, NaN}."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32); b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    y = np.empty(n, F); x = np.empty(n, F)
    q = np.arange(n) & 3
    unit = lambda u: (u.view(np.int32).astype(F) * F(4.6566e-10)).astype(F)
    small = lambda u: ((u & np.uint32(0x807fffff)) | (np.uint32(0x3e000000) + (((u >> np.uint32(23)) & np.uint32(15)) << np.uint32(23)))).view(F)
    m = q == 0; y[m] = a[m].view(F); x[m] = b[m].view(F)
    m = q == 1; y[m] = unit(a[m]); x[m] = unit(b[m])
    m = q == 2; y[m] = small(a[m]); x[m] = small(b[m])
    m = q == 3; y[m] = unit(a[m]); x[m] = ((b[m] & np.uint32(0x80000000)) | (np.uint32(0x3f800000) - (b[m] & np.uint32(0xfffff)))).view(F)
    sp = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1.0, -1.0, np.inf, -np.inf, np.nan], F)
    yy, xx = np.meshgrid(sp, sp, indexing="ij")
    return np.ascontiguousarray(np.stack([np.concatenate([y, yy.ravel()]), np.concatenate([x, xx.ravel()])], 1))


# ------------------------------------------------------------------------------------------------ 4x4
def mul44_families(seed):
    """Column-major [n,16] pairs: rigid times rigid, the same with one special entry, and with scales 2^+-60."""
    rng = np.random.default_rng(seed)

    def rigid(n):
        T = np.zeros((n, 4, 4)); R = _orth(rng, n); R[np.linalg.det(R) < 0, :, 0] *= -1
        T[:, :3, :3] = R; T[:, :3, 3] = rng.normal(size=(n, 3)); T[:, 3, 3] = 1
        return T.transpose(0, 2, 1).reshape(n, 16)
    with np.errstate(all="ignore"):
        fam = [("rigid", rigid(20000).astype(F), rigid(20000).astype(F))]
        both = np.concatenate([rigid(12), rigid(12)], 1).astype(F)
        p = _poke(both, range(32))
        fam.append(("one_special_entry", np.ascontiguousarray(p[:, :16]), np.ascontiguousarray(p[:, 16:])))
        e = rng.choice([-60, 0, 60], (6000, 2))
        fam.append(("scaled_2^60", np.ldexp(rigid(6000), e[:, :1]).astype(F), np.ldexp(rigid(6000), e[:, 1:]).astype(F)))
    return fam
