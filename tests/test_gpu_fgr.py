"""Fast Global Registration on the device (include/tdv_hip.h: tdv_fgr), against the restatement of tests/fgr_restatement.py.

The discrete stages (mutual pairs, tuple pairs, n_mutual, n_tuple, trials_run) read no sum, so they are the restatement's exactly.  The
score counts inliers of the device's own f32 pose with RANSAC's arithmetic: the count is the restatement's, and rmse is the exact sum's
rounding unless exact_sum reports it ambiguous.  The pose agrees with the restatement's to 1e-5 rad and 1e-5 sigma (f64 sin / cos and
the sum order differ in the last places).  Every test runs on a Context of its own."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import chain_scene as cs
import fgr_restatement as R
from test_fgr_abi import BAD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32


@pytest.fixture
def fctx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


@pytest.fixture(scope="module")
def chain(orc, synth):
    """Instance 0 of the chain scene against the model: (src, tgt, fs, ft, cst, cts, T_gt, normals of the model)."""
    sc = cs.build(synth, n_instances=1)
    model = cs.oracle_model(orc, sc)
    d = orc.depth_preprocess(sc["depth"][0], sc["masks"][0], cs.SCALE)
    xyz, _ = orc.unproject(d, None, cs.F, cs.F, cs.CX, cs.CY, cs.ZMAX)
    src, _, _ = orc.voxel_downsample(xyz, None, cs.VOXEL)
    fs = orc.compute_fpfh(src, orc.estimate_normals(src, 30), cs.VOXEL * 5.0)
    ft = model["fpfh"]
    return dict(src=src, tgt=model["xyz"], fs=fs, ft=ft, cst=orc.feature_match(fs, ft), cts=orc.feature_match(ft, fs), T_gt=sc["T_gt"][0],
                normals=model["normals"])


def _same_sets(got, ref):
    assert got["n_mutual"] == ref["n_mutual"] and got["n_tuple"] == ref["n_tuple"] and got["trials_run"] == ref["trials_run"], \
        ((got["n_mutual"], got["n_tuple"], got["trials_run"]), (ref["n_mutual"], ref["n_tuple"], ref["trials_run"]))
    assert np.array_equal(got["mutual"], ref["mutual"])
    assert np.array_equal(got["tuples"], ref["tuples"])


def _pose_close(T, ref, sigma, synth):
    ang = synth.rotation_angle(np.asarray(ref, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, :3])
    dt = float(np.abs(np.asarray(ref, np.float64)[:3, 3] - np.asarray(T, np.float64)[:3, 3]).max())
    assert ang <= 1e-5 and dt <= 1e-5 * sigma, (ang, dt, sigma)


def _check_score(orc, res, c, T, voxel):
    inl, terms = R.score(c["src"], c["tgt"], c["cst"], T, voxel)
    assert res.inliers == inl
    assert res.fitness == F(F(inl) / F(len(c["src"])))
    if inl == 0:
        assert res.rmse == F(999.0)
        return
    nb = (len(c["src"]) + 255) // 256
    _, s32, amb = orc.exact_sum(terms, 16 + (nb + 255) // 256)
    if not amb:
        assert np.float32(res.rmse).tobytes() == np.sqrt(F(s32) / F(inl)).astype(F).tobytes()


def test_discrete_stages_score_and_pose(fctx, orc, synth, chain):
    c = chain
    ref = R.correspondences(c["src"], c["tgt"], c["cst"], c["cts"])
    _same_sets(fctx.fgr_correspondences(c["src"], c["tgt"], c["fs"], c["ft"]), ref)
    res, info = fctx.fgr(c["src"], c["tgt"], c["fs"], c["ft"], cs.VOXEL)
    assert (info["n_mutual"], info["n_tuple"], info["trials_run"], info["degenerate"]) == (ref["n_mutual"], ref["n_tuple"], ref["trials_run"], False)
    _check_score(orc, res, c, res.transformation, cs.VOXEL)
    full = R.fgr(c["src"], c["tgt"], c["cst"], c["cts"], cs.VOXEL)
    sigma = R.normalisation(c["src"], c["tgt"], 0)[2]
    _pose_close(res.transformation, full["T"], sigma, synth)


def test_ground_truth_after_icp(fctx, synth, chain):
    """FGR's pose, then tdv_icp as the chain runs it: the tolerance of the RANSAC + ICP chain tests."""
    c = chain
    res, _ = fctx.fgr(c["src"], c["tgt"], c["fs"], c["ft"], cs.VOXEL)
    fine = fctx.icp(c["src"], c["tgt"], c["normals"], res.transformation, cs.VOXEL * 0.4, cs.ICP_ITERS, True)
    ang, tr = synth.pose_error(fine.transformation, c["T_gt"])
    assert ang < 1e-2 and tr < 1e-3, (ang, tr)


def test_repeatable_and_host_equals_device(fctx, chain):
    c = chain
    a, ia = fctx.fgr(c["src"], c["tgt"], c["fs"], c["ft"], cs.VOXEL)
    b, ib = fctx.fgr(c["src"], c["tgt"], c["fs"], c["ft"], cs.VOXEL)
    bufs = [_up(c[k]) for k in ("src", "tgt", "fs", "ft")]
    d, idd = fctx.fgr_dev(bufs[0][1], len(c["src"]), bufs[1][1], len(c["tgt"]), bufs[2][1], bufs[3][1], cs.VOXEL)
    for r, i in ((b, ib), (d, idd)):
        assert r.transformation.tobytes() == a.transformation.tobytes() and i == ia
        assert (r.inliers, np.float32(r.fitness).tobytes(), np.float32(r.rmse).tobytes()) == \
               (a.inliers, np.float32(a.fitness).tobytes(), np.float32(a.rmse).tobytes())


def test_tuple_count_seed_and_no_tuple_test(fctx, synth, chain):
    c = chain
    five = fctx.fgr_correspondences(c["src"], c["tgt"], c["fs"], c["ft"], maximum_tuple_count=5)
    ref5 = R.correspondences(c["src"], c["tgt"], c["cst"], c["cts"], dict(maximum_tuple_count=5))
    _same_sets(five, ref5)
    full = R.correspondences(c["src"], c["tgt"], c["cst"], c["cts"])
    assert five["n_tuple"] == 15 and np.array_equal(five["tuples"], full["tuples"][:15])
    other = fctx.fgr_correspondences(c["src"], c["tgt"], c["fs"], c["ft"], seed=7)
    _same_sets(other, R.correspondences(c["src"], c["tgt"], c["cst"], c["cts"], dict(seed=7)))
    assert not np.array_equal(other["tuples"], full["tuples"])
    # without the tuple test the mutual set is the pair list
    off = fctx.fgr_correspondences(c["src"], c["tgt"], c["fs"], c["ft"], tuple_test=0)
    assert off["n_tuple"] == 0 and off["trials_run"] == 0 and np.array_equal(off["mutual"], full["mutual"])
    res, info = fctx.fgr(c["src"], c["tgt"], c["fs"], c["ft"], cs.VOXEL, tuple_test=0)
    assert info["n_tuple"] == 0 and not info["degenerate"]
    r = R.fgr(c["src"], c["tgt"], c["cst"], c["cts"], cs.VOXEL, dict(tuple_test=0))
    _pose_close(res.transformation, r["T"], R.normalisation(c["src"], c["tgt"], 0)[2], synth)


def test_absolute_scale_and_options(fctx, orc, synth, chain):
    c = chain
    for kw in (dict(use_absolute_scale=1), dict(decrease_mu=0, iteration_number=10), dict(iteration_number=0)):
        res, _ = fctx.fgr(c["src"], c["tgt"], c["fs"], c["ft"], cs.VOXEL, **kw)
        r = R.fgr(c["src"], c["tgt"], c["cst"], c["cts"], cs.VOXEL, kw)
        norm = R.normalisation(c["src"], c["tgt"], 0)
        _pose_close(res.transformation, r["T"], norm[2], synth)
        _check_score(orc, res, c, res.transformation, cs.VOXEL)


def test_degenerate_and_empty(fctx, synth):
    rng = np.random.default_rng(4)
    src = rng.uniform(-1, 1, (8, 3)).astype(F); fs = synth.random_features(8, 5)
    res, info = fctx.fgr(src, src, fs, fs, 0.01, tuple_test=0)         # 8 mutual pairs: fewer than 10
    assert info["degenerate"] and res.transformation.tobytes() == np.eye(4, dtype=F).tobytes()
    assert info["n_mutual"] == 8 and res.inliers == 8                  # the identity is scored like any pose
    res, info = fctx.fgr(src, src, fs, fs, 0.01, maximum_tuple_count=3)   # 3 trials kept: 9 tuple pairs
    assert info["degenerate"] and info["n_tuple"] == 9 and res.transformation.tobytes() == np.eye(4, dtype=F).tobytes()
    z3 = np.zeros((0, 3), F); z33 = np.zeros((0, 33), F)
    for a, b, fa, fb in ((z3, src, z33, fs), (src, z3, fs, z33)):
        res, info = fctx.fgr(a, b, fa, fb, 0.01)
        assert res.transformation.tobytes() == np.eye(4, dtype=F).tobytes() and (res.inliers, res.fitness, res.rmse) == (0, 0, 0)
        assert (info["n_mutual"], info["n_tuple"], info["trials_run"], info["degenerate"]) == (0, 0, 0, True)


@pytest.mark.parametrize("case", range(1, len(BAD)))
def test_bad_parameters_on_a_ctx(tdv, fctx, case):
    name, kw = BAD[case]
    voxel = {"voxel 0": 0.0, "voxel nan": float("nan"), "voxel inf": float("inf")}.get(name, 0.01)
    pts = np.zeros((4, 3), F); fd = np.zeros((4, 33), F)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    p = tdv.fgr_params(**kw)
    out = tdv.FgrResultC(); C.memset(C.byref(out), 0x5A, C.sizeof(out)); before = bytes(out)
    assert tdv.lib().tdv_fgr(fctx._h, P(pts), 4, P(pts), 4, P(fd), P(fd), C.c_float(voxel), C.byref(p), C.byref(out)) == TDV_ERR_BAD_ARG
    assert bytes(out) == before


def test_non_finite_coordinates(fctx, chain):
    """A NaN and an infinite coordinate: they fail every trial they enter, and through the means the pose is NaN - as the restatement."""
    c = dict(chain)
    src = c["src"].copy(); src[5, 0] = np.nan; src[40, 2] = np.inf
    c["src"] = src
    ref = R.correspondences(src, c["tgt"], c["cst"], c["cts"])
    _same_sets(fctx.fgr_correspondences(src, c["tgt"], c["fs"], c["ft"]), ref)
    res, info = fctx.fgr(src, c["tgt"], c["fs"], c["ft"], cs.VOXEL)
    r = R.fgr(src, c["tgt"], c["cst"], c["cts"], cs.VOXEL)
    assert np.array_equal(np.isnan(res.transformation), np.isnan(r["T"])) and np.isnan(r["T"]).any()
    assert res.inliers == r["inliers"] == 0 and res.rmse == F(999.0)


def test_c4_size_sets(fctx, synth):
    """About 150k x 150k points with random descriptors: the call runs, and its mutual and tuple sets are the restatement's, fed with
    the device's own two matches (tdv_feature_match_dev, held to the oracle elsewhere)."""
    n = 150000
    rng = np.random.default_rng(11)
    src = rng.uniform(-0.2, 0.2, (n, 3)).astype(F); tgt = rng.uniform(-0.2, 0.2, (n + 1234, 3)).astype(F)
    fs = synth.random_features(n, 21); ft = synth.random_features(n + 1234, 22)
    (s_t, s_p), (t_t, t_p), (fs_t, fs_p), (ft_t, ft_p) = _up(src), _up(tgt), _up(fs), _up(ft)
    cst_t = torch.zeros(n, dtype=torch.int32, device=DEV); cts_t = torch.zeros(n + 1234, dtype=torch.int32, device=DEV)
    fctx.feature_match_dev(fs_p, n, ft_p, n + 1234, cst_t.data_ptr())
    fctx.feature_match_dev(ft_p, n + 1234, fs_p, n, cts_t.data_ptr())
    cst = cst_t.cpu().numpy(); cts = cts_t.cpu().numpy()
    res, info = fctx.fgr_dev(s_p, n, t_p, n + 1234, fs_p, ft_p, 0.002)
    got = fctx.fgr_correspondences(src, tgt, fs, ft)
    ref = R.correspondences(src, tgt, cst, cts)
    _same_sets(got, ref)
    assert (info["n_mutual"], info["n_tuple"], info["trials_run"]) == (ref["n_mutual"], ref["n_tuple"], ref["trials_run"])
    assert ref["n_mutual"] > 1000 and math.isfinite(float(res.transformation[0, 0]))
    print("C4 size: %d mutual, %d tuple pairs, %d trials, %d inliers" % (ref["n_mutual"], ref["n_tuple"], ref["trials_run"], res.inliers))
