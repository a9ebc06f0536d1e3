"""CPU suite: ISS keypoints (include/tdv_hip.h: tdv_iss_keypoints).  The ABI exports the entry points, lists them in ABI_SYMBOLS, has the
documented defaults and struct layouts, and refuses every bad argument before it writes anything; the restatement
(tests/iss_restatement.py) is held to independent mathematics: its Jacobi schedule to numpy's eigvalsh, its integer-sum eigenvalues to
the plain f64 covariance of the raw coordinates within a bound derived from the two error terms, an exactly flat grid to lambda3 == 0,
and a row permutation to permuted outputs.  No compute entry point of the library runs here; tests/test_gpu_iss.py holds the device to
this restatement byte for byte."""
import ctypes as C

import numpy as np
import pytest

import cluster_restatement as CR
import iss_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_iss_default_params", "tdv_iss_keypoints", "tdv_iss_keypoints_dev")
NAN, INF = float("nan"), float("inf")


def test_symbols_defaults_and_structs(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.IssParamsC) == 32 and C.sizeof(tdv.IssResultC) == 32
    assert [k for k, _ in tdv.IssParamsC._fields_] == ["salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors"]
    assert [k for k, _ in tdv.IssResultC._fields_] == ["n_finite", "n_supported", "n_salient", "n_keypoints", "salient_radius",
                                                       "non_max_radius", "resolution"]
    assert tdv.IssParamsC.gamma_21.offset == 8 and tdv.IssParamsC.min_neighbors.offset == 24
    assert tdv.IssResultC.salient_radius.offset == 16 and tdv.IssResultC.resolution.offset == 24
    p = tdv.iss_params()
    assert (p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32, p.min_neighbors) == (0.0, 0.0, 0.975, 0.975, 5)
    assert tdv.iss_params(min_neighbors=9, gamma_32=0.5).min_neighbors == 9
    with pytest.raises(TypeError):
        tdv.iss_params(radius=1.0)
    assert R.DEFAULTS == dict(salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)


# ---------------------------------------------------------------- arguments
GOOD = dict(salient_radius=0.3, non_max_radius=0.2, gamma_21=0.975, gamma_32=0.975, min_neighbors=2, attr_width=3)
BAD = [("null ctx", {}), ("salient < 0", dict(salient_radius=-0.1)), ("salient nan", dict(salient_radius=NAN)), ("salient inf", dict(salient_radius=INF)),
       ("non-max < 0", dict(non_max_radius=-0.1)), ("non-max nan", dict(non_max_radius=NAN)), ("non-max inf", dict(non_max_radius=INF)),
       ("only salient 0", dict(salient_radius=0.0)), ("only non-max 0", dict(non_max_radius=0.0)),
       ("gamma_21 nan", dict(gamma_21=NAN)), ("gamma_21 0", dict(gamma_21=0.0)), ("gamma_21 < 0", dict(gamma_21=-1.0)),
       ("gamma_32 nan", dict(gamma_32=NAN)), ("gamma_32 0", dict(gamma_32=0.0)), ("gamma_32 < 0", dict(gamma_32=-0.5)),
       ("min_neighbors 0", dict(min_neighbors=0)), ("min_neighbors < 0", dict(min_neighbors=-3)), ("attr_width < 0", dict(attr_width=-1))]


class Outputs:
    """Every output of a call on n points, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n, width=3, fill=0x5A):
        self.res = tdv.IssResultC(); C.memset(C.byref(self.res), fill, C.sizeof(self.res))
        self.mask = np.full(n, 7, np.uint8); self.saliency = np.full(n, -7, np.float64); self.eig = np.full((n, 3), -7, np.float64)
        self.support = np.full(n, -7, np.int32); self.index = np.full(n, -7, np.int32); self.rows = np.full((n, 3), -7, F)
        self.cols = np.full((n, max(width, 1)), -7, F)
        self.before = self.snapshot()

    def arrays(self):
        return self.mask, self.saliency, self.eig, self.support, self.index, self.rows, self.cols

    def snapshot(self):
        return (bytes(self.res),) + tuple(a.tobytes() for a in self.arrays())

    def untouched(self):
        return self.snapshot() == self.before


def iss_call(lib, dev, ctx, pts, attr, n, o, res=True, prm=True, cols=True, **kw):
    """Host arrays in every slot: a refused call must not look at them (the device entry point included)."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    g = dict(GOOD, **kw)
    p = lib_params(g)
    fn = lib.tdv_iss_keypoints_dev if dev else lib.tdv_iss_keypoints
    return fn(ctx, P(pts), n, C.byref(p) if prm else None, P(attr), g["attr_width"], C.byref(o.res) if res else None, P(o.mask), P(o.saliency),
              P(o.eig), P(o.support), P(o.index), P(o.rows), P(o.cols) if cols else None)


def lib_params(g):
    import importlib
    tdv = importlib.import_module("3dvision_amd")
    return tdv.IssParamsC(g["salient_radius"], g["non_max_radius"], g["gamma_21"], g["gamma_32"], g["min_neighbors"])


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad parameter: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_iss.py refuses each bad parameter on one."""
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); attr = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4)
        assert iss_call(lib, dev, None, pts, attr, 4, o, **BAD[case][1]) == TDV_ERR_BAD_ARG
        assert o.untouched()


def null_and_size_cases(lib, dev, ctx, pts, attr, n, o):
    """The refusals that are not a parameter's: every one must return TDV_ERR_BAD_ARG."""
    yield iss_call(lib, dev, ctx, None, None, n, o, attr_width=0)                  # a NULL cloud with n > 0
    yield iss_call(lib, dev, ctx, pts, None, -1, o, attr_width=0)                  # n < 0
    yield iss_call(lib, dev, ctx, pts, None, R.MAX_POINTS + 1, o, attr_width=0)    # n > 2^22
    yield iss_call(lib, dev, ctx, pts, attr, n, o, res=False)                      # a NULL result
    yield iss_call(lib, dev, ctx, pts, attr, n, o, prm=False)                      # NULL params
    yield iss_call(lib, dev, ctx, pts, None, n, o)                                 # attr_width > 0 with a NULL attr
    yield iss_call(lib, dev, ctx, pts, None, n, o, attr_width=0)                   # out_attr without attr


def test_null_arrays_sizes_and_attr(tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); attr = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4, fill=0x33)
        for status in null_and_size_cases(lib, dev, None, pts, attr, 4, o):
            assert status == TDV_ERR_BAD_ARG
        assert o.untouched()


# ---------------------------------------------------------------- the restatement against independent mathematics
U = 2.0 ** -53


def _eigvals_desc(M):
    return np.linalg.eigvalsh(M)[..., ::-1]


def _entries(M):
    return M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]


def test_jacobi_schedule_against_eigvalsh():
    """The fixed schedule (6 sweeps over (0,1), (0,2), (1,2)) against LAPACK within 64 u of the largest |eigenvalue|, u = 2^-53: at most 18
    rotations, each a product with a matrix that is orthogonal to within the roundings of c and s and rounds every entry it updates twice -
    under 3 u of the matrix norm per rotation, 54 u in all - and eigvalsh itself is backward stable to a few u of the norm."""
    rng = np.random.default_rng(7)
    B = rng.normal(size=(4000, 3, 3))
    sym = B + B.transpose(0, 2, 1)
    Q = np.linalg.qr(rng.normal(size=(1000, 3, 3)))[0]
    psd = B[:1000] @ B[:1000].transpose(0, 2, 1) * 10.0 ** rng.integers(-12, 12, (1000, 1, 1))
    v = rng.normal(size=(500, 3))
    rank1 = v[:, :, None] * v[:, None, :]
    rep = Q[:500] @ (np.array([2.0, 2.0, 0.5]) * np.eye(3)) @ Q[:500].transpose(0, 2, 1)          # a repeated eigenvalue
    rep = (rep + rep.transpose(0, 2, 1)) / 2
    same = np.tile(3.0 * np.eye(3), (4, 1, 1))
    diag = np.zeros((300, 3, 3)); diag[:, [0, 1, 2], [0, 1, 2]] = rng.normal(size=(300, 3))
    zero = np.zeros((2, 3, 3))
    for name, M in (("symmetric", sym), ("psd", psd), ("rank 1", rank1), ("repeated", rep), ("scalar", same), ("diagonal", diag), ("zero", zero)):
        (l0, l1, l2), off = R.jacobi_eigenvalues(*_entries(M))
        got, want = np.stack([l0, l1, l2], 1), _eigvals_desc(M)
        scale = np.abs(want).max(1)
        err = np.abs(got - want).max(1)
        print(name, "max error / (u * |lambda|max): %.2f" % (err / np.maximum(scale, 1e-300) / U).max(), " off-diagonal left: %.3g" % (off / np.maximum(scale, 1e-300)).max())
        assert (err <= 64 * U * scale).all(), name
        assert (off <= 64 * U * scale).all(), name
        assert (l0 >= l1).all() and (l1 >= l2).all()
    (l0, l1, l2), _ = R.jacobi_eigenvalues(*_entries(diag))
    assert np.stack([l0, l1, l2], 1).tobytes() == np.sort(diag[:, [0, 1, 2], [0, 1, 2]], 1)[:, ::-1].tobytes()       # every pair skipped: the diagonal itself


def _plain_eigenvalues(xyz, r):
    """eigvalsh of the plain f64 covariance of every neighbourhood's RAW coordinates about its own mean (two passes); tr C with it."""
    a, b = R.directed_pairs(xyz, r)
    rows, starts = R._group_starts(a)
    P = xyz.astype(np.float64)
    cnt = np.bincount(a, minlength=len(xyz))[rows].astype(np.float64)
    mean = np.stack([np.add.reduceat(P[b, k], starts) for k in range(3)], 1) / cnt[:, None]
    d = P[b] - np.repeat(mean, np.diff(np.concatenate([starts, [len(a)]])), 0)
    Cm = np.zeros((len(rows), 3, 3))
    for p in range(3):
        for q in range(3):
            Cm[:, p, q] = np.add.reduceat(d[:, p] * d[:, q], starts) / cnt
    return rows, _eigvals_desc(Cm), Cm[:, [0, 1, 2], [0, 1, 2]].sum(1)


def _bracket(synth, n, offset=(0.0, 0.0, 0.0)):
    pts = synth.sample_object(n, 11)[0].astype(np.float64)
    pts += np.random.default_rng(n).normal(0, 2e-4, pts.shape)
    return (pts + np.asarray(offset)).astype(F)


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (0.5, -0.4, 0.48)], ids=["origin", "lever arm 0.8 m"])
def test_integer_sum_eigenvalues_against_the_plain_covariance(synth, offset):
    """The reported eigenvalues against eigvalsh of the plain f64 covariance of the raw f32 coordinates, for every supported point.

    The integer moments see each coordinate difference d_a = p_j,a - p_i,a (a covariance does not move with the query's own position)
    through two perturbations: the f32 rounding of the difference, at most 2^-24 |d_a| (relative to the DIFFERENCE whatever the cloud's
    distance from the origin: the inputs are f32 already, and the reference takes them as they are), and the rounding to the quantum, at
    most half of 2^-sh <= 2^-20 r.  With |d_a| <= r (1 + 2^-22): e = r (2^-20 + 2^-23) bounds either coordinate error, sqrt(3) e the
    error vector of a neighbour.  For x_k -> x_k + e_k the covariance moves by (1/c) sum [(x_k - xm)(e_k - em)' + (e_k - em)(x_k - xm)' +
    (e_k - em)(e_k - em)'], whose 2-norm is at most 2 sqrt(tr C) sqrt(3) e + 3 e^2 (Cauchy-Schwarz; the variance of e is at most its mean
    square), and by Weyl's inequality no eigenvalue moves by more.  The f64 steps of rules 4 and 5 and the reference's own work on values of
    at most 3 r^2 stay under 2^-40 r^2 (a few hundred roundings of 2^-53), added as slack."""
    xyz = _bracket(synth, 3000, offset)
    res = R.resolution(xyz)[0]
    rs, rn = R.default_radii(res)
    out = R.iss(xyz, salient_radius=rs, non_max_radius=rn)
    rows, want, trace = _plain_eigenvalues(xyz, rs)
    ok = out["support"][rows] >= 5
    rows, want, trace = rows[ok], want[ok], trace[ok]
    r = float(rs)
    e = r * (2.0 ** -20 + 2.0 ** -23)
    bound = 2 * np.sqrt(3.0 * trace) * e + 3 * e * e + 2.0 ** -40 * r * r
    err = np.abs(out["eigenvalues"][rows] - want).max(1)
    print("points %d  keypoints %d  max |d lambda| / lambda1 %.3g  max |d lambda| / bound %.3g  bound / lambda1 (median) %.3g"
          % (len(rows), out["n_keypoints"], (err / want[:, 0]).max(), (err / bound).max(), np.median(bound / want[:, 0])))
    assert len(rows) > 2900 and (err <= bound).all()
    assert (bound < 2e-5 * want[:, 0]).all()                              # the bound itself is parts in 10^5 of lambda1: it holds something
    assert 0 < out["n_keypoints"] < 0.1 * len(xyz)                        # a few percent of a noisy part


def test_moments_against_the_dense_definition():
    """moments() (tree candidates, reduceat) against rules 1-3 read literally over the dense n x n matrix, NaN / infinite / 1e19 rows and
    exact duplicates included."""
    rng = np.random.default_rng(3)
    pts = rng.random((400, 3)).astype(F)
    pts[5] = np.nan; pts[6, 1] = np.inf; pts[7, 0] = 1e19; pts[20:24] = pts[20]
    for r in (0.17, 0.25, 0.5, 1e-9, 3.0):
        support, S = R.moments(pts, r)
        with np.errstate(invalid="ignore", over="ignore"):
            d = pts[None, :, :] - pts[:, None, :]                        # [i, j] = p_j - p_i
            nb = CR.d2_f32(pts[None, :, :], pts[:, None, :]) <= R.r2_f32(r)
            u = np.where(nb[:, :, None], np.rint(np.ldexp(d, R.shift(r))), 0).astype(np.int64)
        assert np.array_equal(support, nb.sum(1))
        want = [u[:, :, 0], u[:, :, 1], u[:, :, 2], u[:, :, 0] * u[:, :, 0], u[:, :, 0] * u[:, :, 1], u[:, :, 0] * u[:, :, 2], u[:, :, 1] * u[:, :, 1],
                u[:, :, 1] * u[:, :, 2], u[:, :, 2] * u[:, :, 2]]
        assert np.array_equal(S, np.stack([w.sum(1) for w in want], 1)), r
        assert np.abs(u).max() <= 2 ** 20 + 1
        assert support[[5, 6]].tolist() == [0, 0] and support[7] == 1
    assert R.shift(0.5) == 20 and R.shift(np.nextafter(F(0.5), F(0))) == 21 and R.shift(1.0) == 19 and R.shift(0.0) == 20     # frexp's edges


def test_flat_grid_has_no_keypoint():
    """An exactly flat grid: u_z = 0 for every pair, so a02, a12 and a22 are exactly 0, stay 0 through every rotation, and lambda3 == 0 on
    every point: nothing is salient whatever the gammas."""
    g = np.stack(np.meshgrid(np.arange(30), np.arange(30), indexing="ij"), -1).reshape(-1, 2)
    for pitch, z in ((0.01, 0.25), (0.0078125, -3.0)):
        pts = np.c_[g * pitch, np.full(len(g), z)].astype(F)
        out = R.iss(pts, salient_radius=3.2 * pitch, non_max_radius=2.1 * pitch, gamma_21=2.0, gamma_32=2.0)
        assert out["n_supported"] == len(pts) and (out["eigenvalues"][:, 2] == 0).all() and (out["eigenvalues"][:, 1] > 0).all()
        assert out["n_salient"] == 0 and out["n_keypoints"] == 0 and not out["saliency"].any()
    line = np.zeros((50, 3), F); line[:, 1] = np.arange(50) * 0.01
    out = R.iss(line, salient_radius=0.035, non_max_radius=0.02, gamma_21=2.0, gamma_32=2.0)
    assert (out["eigenvalues"][:, 1:] == 0).all() and out["n_keypoints"] == 0


def test_row_permutation(synth):
    """Permuting the rows permutes mask, saliency, eigenvalues and support bit for bit (integer sums have no order) and leaves the set of
    keypoint coordinates as it was."""
    xyz = _bracket(synth, 1500)
    rng = np.random.default_rng(5)
    attr = rng.random((len(xyz), 4)).astype(F)
    a = R.iss(xyz, attr)                                                 # default radii: the exact-sum resolution has no order either
    perm = rng.permutation(len(xyz))
    b = R.iss(xyz[perm], attr[perm])
    assert (a["salient_radius"], a["non_max_radius"]) == (b["salient_radius"], b["non_max_radius"])
    assert a["n_keypoints"] > 5
    for k in ("mask", "saliency", "eigenvalues", "support"):
        assert a[k][perm].tobytes() == b[k].tobytes(), k
    assert [a[k] for k in R.COUNTS] == [b[k] for k in R.COUNTS]
    rows = lambda o: sorted(map(bytes, np.c_[o["xyz"], o["attr"]]))      # noqa: E731
    assert rows(a) == rows(b)


def test_resolution_variants_agree_and_default_radii():
    rng = np.random.default_rng(9)
    pts = rng.random((500, 3)).astype(F)
    pts[3] = np.nan; pts[4, 2] = -np.inf; pts[9, 0] = 1e19; pts[40:43] = pts[40]
    assert R.nearest(pts).tobytes() == R.nearest_brute(pts).tobytes()
    res, nv, nn = R.resolution(pts)
    assert nv == 498 and np.isnan(nn[3]) and np.isinf(nn[4]) and nn[9] > 9e18 and nn[40] == 0.0      # (1e19)^2 is still an f32: a distance like any other
    rs, rn = R.default_radii(res)
    assert rs == F(6.0 * res) and rn == F(4.0 * res) and R.resolution_bound(res, 500) < 1e-14 * res
    out = R.iss(pts)
    assert (out["salient_radius"], out["non_max_radius"]) == (rs, rn) and out["resolution"] == res
    one = R.iss(pts[:1])                                                  # no second neighbour: no resolution, NaN radii, nothing counted
    assert np.isnan(one["resolution"]) and np.isnan(one["salient_radius"]) and one["n_finite"] == 0
    none = R.iss(np.zeros((0, 3), F))
    assert np.isnan(none["resolution"]) and none["n_keypoints"] == 0 and len(none["mask"]) == 0
