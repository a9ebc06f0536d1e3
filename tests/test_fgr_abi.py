"""CPU suite: Fast Global Registration (include/tdv_hip.h: tdv_fgr).  The ABI exports the entry points, lists them in ABI_SYMBOLS, gives
Open3D's defaults and refuses every bad argument before it writes anything; the restatement (tests/fgr_restatement.py) produces
Random123's Philox4x32-10 known answers, and from scratch it registers the relief part of tests/chain_scene.py, where ICP from the
identity does not.  No compute entry point of the library runs here; tests/test_gpu_fgr.py holds the device to this restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import chain_scene as cs
import fgr_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_fgr_default_params", "tdv_fgr", "tdv_fgr_dev", "tdv_fgr_correspondences")


def test_symbols_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    p = tdv.fgr_params()
    assert (p.division_factor, p.maximum_correspondence_distance, p.tuple_scale) == (F(1.4), F(0.025), F(0.95))
    assert (p.iteration_number, p.maximum_tuple_count, p.use_absolute_scale, p.decrease_mu, p.tuple_test, p.seed) == (64, 1000, 0, 1, 1, 42)
    assert C.sizeof(tdv.FgrParamsC) == 36 and C.sizeof(tdv.FgrResultC) == 96
    assert R.DEFAULTS == dict(division_factor=1.4, maximum_correspondence_distance=0.025, tuple_scale=0.95, iteration_number=64,
                              maximum_tuple_count=1000, use_absolute_scale=0, decrease_mu=1, tuple_test=1, seed=42)
    assert R.CHUNK == 131072          # TDV_FGR_TRIAL_CHUNK


BAD = [("null ctx", {}), ("voxel 0", {}), ("voxel nan", {}), ("voxel inf", {}),
       ("division_factor", dict(division_factor=1.0)), ("division_factor", dict(division_factor=float("nan"))),
       ("division_factor", dict(division_factor=float("inf"))),
       ("tuple_scale", dict(tuple_scale=0.0)), ("tuple_scale", dict(tuple_scale=1.01)), ("tuple_scale", dict(tuple_scale=float("nan"))),
       ("maximum_correspondence_distance", dict(maximum_correspondence_distance=0.0)),
       ("maximum_correspondence_distance", dict(maximum_correspondence_distance=-1.0)),
       ("maximum_correspondence_distance", dict(maximum_correspondence_distance=float("inf"))),
       ("iteration_number", dict(iteration_number=-1)), ("maximum_tuple_count", dict(maximum_tuple_count=0))]


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_out_untouched(tdv, case):
    """A NULL ctx, alone and with each bad parameter: TDV_ERR_BAD_ARG, out (and the counts) byte for byte as they were.  A real ctx
    needs a device: tests/test_gpu_fgr.py refuses each bad parameter on one."""
    lib = tdv.lib()
    name, kw = BAD[case]
    pts = np.zeros((4, 3), F); fd = np.zeros((4, 33), F)
    p = tdv.fgr_params(**kw)
    voxel = {"voxel 0": 0.0, "voxel nan": float("nan"), "voxel inf": float("inf")}.get(name, 0.01)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for fn in (lib.tdv_fgr, lib.tdv_fgr_dev):
        out = tdv.FgrResultC(); C.memset(C.byref(out), 0x5A, C.sizeof(out)); before = bytes(out)
        assert fn(None, P(pts), 4, P(pts), 4, P(fd), P(fd), C.c_float(voxel), C.byref(p), C.byref(out)) == TDV_ERR_BAD_ARG
        assert bytes(out) == before
    nm = C.c_int(-7); nu = C.c_int(-7); tr = C.c_longlong(-7)
    assert lib.tdv_fgr_correspondences(None, P(pts), 4, P(pts), 4, P(fd), P(fd), C.byref(p), None, 0, None, 0, C.byref(nm), C.byref(nu),
                                       C.byref(tr)) == TDV_ERR_BAD_ARG
    assert (nm.value, nu.value, tr.value) == (-7, -7, -7)


def test_null_arrays_and_params(tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); fd = np.zeros((4, 33), F); p = tdv.fgr_params()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    out = tdv.FgrResultC(); C.memset(C.byref(out), 0x33, C.sizeof(out)); before = bytes(out)
    for args in [(None, 4, P(pts), 4, P(fd), P(fd)), (P(pts), 4, None, 4, P(fd), P(fd)), (P(pts), 4, P(pts), 4, None, P(fd)),
                 (P(pts), 4, P(pts), 4, P(fd), None), (P(pts), -1, P(pts), 4, P(fd), P(fd))]:
        assert lib.tdv_fgr(None, *args, C.c_float(0.01), C.byref(p), C.byref(out)) == TDV_ERR_BAD_ARG
    assert lib.tdv_fgr(None, P(pts), 4, P(pts), 4, P(fd), P(fd), C.c_float(0.01), None, C.byref(out)) == TDV_ERR_BAD_ARG
    assert lib.tdv_fgr(None, P(pts), 4, P(pts), 4, P(fd), P(fd), C.c_float(0.01), C.byref(p), None) == TDV_ERR_BAD_ARG
    assert bytes(out) == before
    with pytest.raises(TypeError):
        tdv.fgr_params(no_such_option=1)


# ---------------------------------------------------------------- restatement
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,expect", KAT)
def test_philox_known_answers(ctr, key, expect):
    got = tuple(int(w[0]) for w in R.philox4x32(ctr, key))
    assert got == expect, ["%08x" % g for g in got]


def test_trial_indices_are_in_range_and_spread():
    t = np.arange(200000, dtype=np.uint64)
    for n in (1, 3, 1000, 123457):
        idx = R.trial_indices(t, n, 42)
        assert idx.shape == (3, len(t)) and int(idx.max()) < n
    idx = R.trial_indices(t, 10, 7)
    counts = np.bincount(idx.ravel().astype(np.int64), minlength=10)
    assert counts.min() > 0.97 * counts.mean() and counts.max() < 1.03 * counts.mean()
    t64 = np.array([1 << 32, (1 << 32) + 1], np.uint64)              # the high word of the counter is used
    assert not np.array_equal(R.trial_indices(t64, 1000, 42), R.trial_indices(t64 - np.uint64(1 << 32), 1000, 42))


def test_tuple_test_keeps_the_first_passes_in_trial_order():
    rng = np.random.default_rng(2)
    src = rng.uniform(-1, 1, (300, 3)).astype(F)
    tgt = (src @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F).T + F(0.3)).astype(F)
    tgt[200:] = rng.uniform(-1, 1, (100, 3))                       # a third of the pairs are wrong
    pairs = np.stack([np.arange(300), np.arange(300)], 1)
    all5, run5 = R.tuple_test(src, tgt, pairs, 0.95, 5, 42)
    many, run = R.tuple_test(src, tgt, pairs, 0.95, 1000, 42)
    assert len(all5) == 15 and np.array_equal(all5, many[:15]) and run5 == 30000       # one chunk, cut at 100 n_mutual
    assert len(many) == 3000 and run == 30000
    # a kept trial passes the test on its three pairs, and a pair with a wrong target seldom survives
    for k in range(0, 3000, 3):
        a, b = src[many[k:k + 3, 0]].astype(np.float64), tgt[many[k:k + 3, 1]].astype(np.float64)
        for u, v in ((0, 1), (1, 2), (2, 0)):
            la, lb = np.linalg.norm(a[u] - a[v]), np.linalg.norm(b[u] - b[v])
            assert la * np.float64(F(0.95)) < lb < la / np.float64(F(0.95))
    assert (many[:, 0] >= 200).mean() < 0.1


def test_ldlt_and_update_match_numpy():
    rng = np.random.default_rng(5)
    J = rng.normal(size=(40, 6)); A = J.T @ J; b = rng.normal(size=6)
    assert np.allclose(R.ldlt6(A, b), np.linalg.solve(A, b), rtol=1e-12, atol=1e-12)
    assert R.ldlt6(np.zeros((6, 6)), b) is None
    x = rng.normal(size=3) * 0.3
    Rx = np.array([[1, 0, 0], [0, np.cos(x[0]), -np.sin(x[0])], [0, np.sin(x[0]), np.cos(x[0])]])
    Ry = np.array([[np.cos(x[1]), 0, np.sin(x[1])], [0, 1, 0], [-np.sin(x[1]), 0, np.cos(x[1])]])
    Rz = np.array([[np.cos(x[2]), -np.sin(x[2]), 0], [np.sin(x[2]), np.cos(x[2]), 0], [0, 0, 1]])
    assert np.allclose(R.rz_ry_rx(*x), Rz @ Ry @ Rx, atol=1e-15)


def test_optimisation_recovers_a_noiseless_pose(synth):
    """On exact correspondences the pose comes back to rounding; with a tenth of them wrong, the Geman-McClure weights of those (about
    (mu / r^2)^2 once mu has come down) leave a small bias only."""
    rng = np.random.default_rng(9)
    tgt = rng.uniform(-0.1, 0.1, (600, 3)).astype(F)
    T = synth.perturb(np.eye(4), seed=3, angle_deg=40.0, trans=0.05).astype(np.float64)
    src = ((tgt.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)        # src = T^-1 tgt: T moves the source onto the target
    corr = np.stack([np.arange(600), np.arange(600)], 1)
    for wrong, bound in ((0, (1e-6, 1e-7)), (60, (1e-3, 1e-4))):
        c = corr.copy()
        c[:wrong, 1] = (c[:wrong, 1] + 300) % 600
        est = R.original_scale(*R.optimise(src, tgt, c))
        ang, tr = synth.pose_error(est, T)
        assert ang < bound[0] and tr < bound[1], (wrong, ang, tr)


@pytest.fixture(scope="module")
def chain(orc, synth):
    sc = cs.build(synth, n_instances=3)
    model = cs.oracle_model(orc, sc)
    return sc, model


def test_restatement_registers_the_chain_scene(orc, synth, chain):
    """From scratch on the relief part: ICP from the identity fails; FGR on the oracle's FPFH lands within a few mrad / mm, and the
    oracle's ICP from there reaches the tolerance of the RANSAC + ICP chain tests (1e-2 rad, 1 mm).  Measured (instances 0, 1, 2):
    FGR 4.1 / 4.2 / 2.8 mrad and 1.8 / 1.8 / 1.2 mm, after ICP 1.8 / 1.6 / 1.4 mrad and 0.17 / 0.08 / 0.25 mm; RANSAC (4,000
    hypotheses) and the same ICP: the numbers printed beside them."""
    sc, model = chain
    for b in range(3):
        r = cs.oracle_instance(orc, sc, b, model)
        T = sc["T_gt"][b]
        src = r["src"]
        cts = orc.feature_match(model["fpfh"], r["fpfh"])
        g = R.fgr(src, model["xyz"], r["coarse"]["corr"], cts, cs.VOXEL)
        assert not g["degenerate"] and g["n_tuple"] == 3000 and g["trials_run"] == R.CHUNK
        fine = orc.icp(src, model["xyz"], model["normals"], g["T"], cs.VOXEL * 0.4, cs.ICP_ITERS, True)
        ident = orc.icp(src, model["xyz"], model["normals"], np.eye(4, dtype=F), cs.VOXEL * 0.4, cs.ICP_ITERS, True)
        e_f, e_fi, e_i = synth.pose_error(g["T"], T), synth.pose_error(fine["T"], T), synth.pose_error(ident["T"], T)
        e_r, e_ri = synth.pose_error(r["coarse"]["T"], T), synth.pose_error(r["fine"]["T"], T)
        print("instance %d: FGR %d mutual, %d tuple pairs, %.2e rad %.2e m -> ICP %.2e rad %.2e m; RANSAC %.2e rad %.2e m -> ICP %.2e rad "
              "%.2e m; ICP from I %.2f rad" % (b, g["n_mutual"], g["n_tuple"], *e_f, *e_fi, *e_r, *e_ri, e_i[0]))
        assert e_i[0] > 0.5                                          # the pose is not one ICP finds on its own
        assert e_f[0] < 1e-2 and e_f[1] < 5e-3                       # FGR alone: coarse, like RANSAC's
        assert e_fi[0] < 1e-2 and e_fi[1] < 1e-3                     # the chain tests' tolerance after ICP
        # the score is RANSAC's: counts over the one-way matches at 1.5 voxel
        assert g["inliers"] == R.score(src, model["xyz"], r["coarse"]["corr"], g["T"], cs.VOXEL)[0] > 0.3 * len(src)


def test_degenerate_and_non_finite_rules():
    rng = np.random.default_rng(1)
    src = rng.uniform(-1, 1, (50, 3)).astype(F); tgt = src.copy()
    cst = np.arange(50); cts = np.arange(50)
    few = R.fgr(src[:9], tgt[:9], cst[:9], cts[:9], 0.01, dict(tuple_test=0))
    assert few["degenerate"] and np.array_equal(few["T"], np.eye(4, dtype=F)) and few["n_mutual"] == 9
    ok = R.fgr(src, tgt, cst, cts, 0.01, dict(tuple_test=0))
    assert not ok["degenerate"] and np.abs(ok["T"] - np.eye(4)).max() < 1e-6 and ok["inliers"] == 50
    bad = src.copy(); bad[3, 1] = np.nan
    nf = R.fgr(bad, tgt, cst, cts, 0.01, dict(tuple_test=0))
    assert np.isnan(nf["T"][:3, 3]).all() and nf["inliers"] == 0       # NaN through the means: the pose is NaN, nothing scores
    t = R.correspondences(bad, tgt, cst, cts)
    assert not (t["tuples"][:, 0] == 3).any()                          # a trial with the NaN point never passes
    assert math.isclose(R.normalisation(src, tgt, 1)[2], 1.0) and R.normalisation(src, tgt, 1)[3] == R.normalisation(src, tgt, 0)[2]
