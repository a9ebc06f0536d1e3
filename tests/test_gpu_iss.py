"""ISS keypoints on the device (include/tdv_hip.h: tdv_iss_keypoints) against the restatement of tests/iss_restatement.py, from the host and
the device entry points, each test on a Context of its own.

Byte for byte, with no gap condition: the four counts, mask, support, saliency and eigenvalues (f64 arrays: the integer sums and the fixed
f64 schedule fix every bit), index and the keypoints' xyz / attr rows.  With the default radii the device's resolution is the bytes of
rule 8 restated in the header's fixed order of additions (iss_restatement.resolution_in_tree_order), the radii are float32(6 * resolution)
and float32(4 * resolution) of that RESTATED resolution, and everything else is the restatement run at those radii.  The device's and the
restated resolution are also held to the exact-sum value within iss_restatement.resolution_bound (the fixed tree's depth times 2^-53,
nothing measured)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import iss_restatement as R
from state_cases import blob
from test_cluster_abi import rest_of_scene
from test_gpu_cluster import KINDS, _eps_for
from test_gpu_fuzz import _make
from test_iss_abi import BAD, Outputs, iss_call, null_and_size_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
SIZES = [1, 4, 63, 64, 65, 1000, 4096, 4097, 9001]        # below min_neighbors; around one leaf; where the second group of 64 leaves begins


@pytest.fixture
def ictx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def dev_call(ctx, pts, attr=None, **params):
    """tdv_iss_keypoints_dev with every output asked for, read back with torch."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    w = 0 if attr is None else np.asarray(attr).reshape(n, -1).shape[1] if n else np.asarray(attr).shape[-1]
    (pts_t, px), (mt, pm), (st, ps), (et, pe) = _up(pts), _up(np.full(n, 9, np.uint8), np.uint8), _up(np.full(n, -9.0), np.float64), _up(np.full(3 * n, -9.0), np.float64)
    (ut, pu), (it, pi), (xt, pxo) = _up(np.full(n, -9, np.int32), np.int32), _up(np.full(n, -9, np.int32), np.int32), _up(np.full((n, 3), -9, F))
    (attr_t, pa), (ct, pc) = (_up(attr), _up(np.full(n * w, -9, F))) if attr is not None else ((None, None), (None, None))     # (every tensor stays named:
                                                                                                                          # a dropped one is memory torch hands out again)
    torch.cuda.synchronize()                                             # the uploads are torch's; the ctx runs on a stream of its own
    res = ctx.iss_keypoints_dev(px, n, pa, w, pm, ps, pe, pu, pi, pxo, pc, **params)
    torch.cuda.synchronize()
    m = res["n_keypoints"]
    assert (it[m:n].cpu().numpy() == -9).all() and (xt[3 * m:3 * n].cpu().numpy() == -9).all()       # nothing beyond n_keypoints is written
    res.update(mask=mt[:n].cpu().numpy(), saliency=st[:n].cpu().numpy(), eigenvalues=et[:3 * n].cpu().numpy().reshape(-1, 3),
               support=ut[:n].cpu().numpy(), index=it[:m].cpu().numpy(), xyz=xt[:3 * m].cpu().numpy().reshape(-1, 3),
               attr=None if attr is None else ct[:m * w].cpu().numpy().reshape(m, w))
    return res


def same(ref, got, what):
    counts = [got[k] for k in R.COUNTS], [ref[k] for k in R.COUNTS]
    assert counts[0] == counts[1], (what, "counts", counts)
    for k in R.ARRAYS:
        if ref[k] is not None:
            assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes(), (what, k)
    for k in ("salient_radius", "non_max_radius"):
        assert F(got[k]).tobytes() == F(ref[k]).tobytes() or (np.isnan(got[k]) and np.isnan(ref[k])), (what, k, got[k], ref[k])


def check(ctx, pts, attr=None, what=None, ref=None, **params):
    """Host and device entry points at given radii against the restatement; returns the restatement's dict."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    ref = ref or R.iss(pts, attr, **params)
    for name, got in (("host", ctx.iss(pts, attr, **params)), ("dev", dev_call(ctx, pts, attr, **params))):
        same(ref, got, (what, len(pts), params, name))
        assert np.isnan(got["resolution"])                                 # the radii were given
    return ref


def check_defaults(ctx, pts, attr=None, what=None, **params):
    """Default radii: the resolution is the restated tree order's bytes (and within the tree's bound of the exact-sum value), the radii
    are made of the restated resolution, everything else is byte-equal to the restatement at those radii."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    exact = R.resolution(pts)[0]
    bound = R.resolution_bound(exact, n)
    restated = np.float64(R.resolution_in_tree_order(pts)[0])
    rs, rn = R.default_radii(restated)
    if np.isnan(exact):
        assert np.isnan(restated)
    else:
        assert abs(restated - exact) <= bound, (what, "the restated order against the exact sum", restated, exact, bound)
    ref = R.iss(pts, attr, **dict(params, salient_radius=rs, non_max_radius=rn)) if np.isfinite(rs) and rs > 0 else \
        R.iss(pts, attr, **dict(params, salient_radius=np.nan, non_max_radius=np.nan)) if np.isnan(rs) else None
    same_radius = lambda a, b: F(a).tobytes() == F(b).tobytes() or (np.isnan(a) and np.isnan(b))      # noqa: E731
    for name, got in (("host", ctx.iss(pts, attr, **params)), ("dev", dev_call(ctx, pts, attr, **params))):
        res = np.float64(got["resolution"])
        print(what, n, name, "resolution %.17g (%s) restated %.17g (%s) exact %.17g bound %.3g" % (res, res.tobytes().hex(), restated,
                                                                                              restated.tobytes().hex(), exact, bound))
        if np.isnan(exact):
            assert np.isnan(res), (what, name, res)
        else:
            assert abs(res - exact) <= bound and bound <= 1e-12 * exact, (what, name, res, exact, bound)
            assert res.tobytes() == restated.tobytes(), (what, name, "device %.17g restated order %.17g" % (res, restated))
        assert same_radius(got["salient_radius"], rs) and same_radius(got["non_max_radius"], rn), (what, name, got["salient_radius"], rs)
        if ref is not None:                                                # (a resolution of exactly 0 - every point a duplicate - has no given-radii form)
            same(ref, got, (what, n, "defaults", name))
    return ref


def _object(synth, n, seed=11, offset=(0.0, 0.0, 0.0)):
    pts = synth.sample_object(n, seed)[0].astype(np.float64)
    pts += np.random.default_rng(n + seed).normal(0, 2e-4, pts.shape)
    return (pts + np.asarray(offset)).astype(F)


# ---------------------------------------------------------------- 1. kinds and sizes
def _radii(kind, pts, rng):
    if kind == "grid":                                                     # pitch 0.01: many supports and saliencies exactly equal
        return 0.025, 0.015
    return _eps_for(pts, 25, rng), _eps_for(pts, 10, rng)


@pytest.mark.parametrize("kind", KINDS)
def test_fuzz(ictx, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 31)
    total = 0
    for s, n in enumerate(SIZES):
        pts = _make(kind, n, rng)
        rs, rn = _radii(kind, pts, rng)
        attr = rng.random((n, (1, 3, 4, 33)[s % 4])).astype(F) if s % 2 == 0 else None
        ref = check(ictx, pts, attr, what=kind, salient_radius=rs, non_max_radius=rn, min_neighbors=5 if n > 4 else (1, 5)[s % 2])
        total += ref["n_keypoints"]
        if kind in ("flat", "line"):
            assert ref["n_salient"] == 0 and (ref["eigenvalues"][:, 2] == 0).all()       # lambda3 == 0 exactly: never a keypoint
        if kind in ("nan_rows", "inf_rows"):
            bad = ~np.isfinite(pts).all(1)
            assert bad.any() and (ref["support"][bad] == 0).all() and ref["n_finite"] == n - bad.sum()
    if kind in ("uniform", "grid", "dups", "clusters", "huge", "nan_rows", "inf_rows"):
        assert total > 20, total                                           # the comparison is not of empty lists


def test_grid_ties_keep_both(ictx):
    """The exact grid: interior points share one neighbourhood shape, so whole runs of saliencies are bit-equal and rule 7 keeps every one
    of a tie.  (Powers of two as pitch: the coordinates and their differences are exact.)"""
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.0078125)
    g[:, 2] *= F(0.5); g[:, 1] *= F(0.75)                                   # three distinct extents: salient at the default gammas
    ref = check(ictx, g, what="grid ties", salient_radius=0.02, non_max_radius=0.012)
    sal = ref["saliency"][ref["mask"] == 1]
    assert ref["n_keypoints"] > 30 and len(np.unique(sal)) < len(sal) / 4


def test_empty_cloud_and_open3d_shape(ictx, synth):
    r = ictx.iss(np.zeros((0, 3), F), salient_radius=0.1, non_max_radius=0.05)
    assert [r[k] for k in R.COUNTS] == [0, 0, 0, 0] and len(r["index"]) == 0 and np.isnan(r["resolution"]) and r["salient_radius"] == F(0.1)
    r = dev_call(ictx, np.zeros((0, 3), F))
    assert [r[k] for k in R.COUNTS] == [0, 0, 0, 0] and np.isnan(r["resolution"]) and np.isnan(r["salient_radius"]) and np.isnan(r["non_max_radius"])
    pts = _object(synth, 3000)
    ref = R.iss(pts, salient_radius=0.008, non_max_radius=0.005)
    rows, ind = ictx.compute_iss_keypoints(pts, 0.008, 0.005)
    assert ind.dtype == np.int64 and ind.tobytes() == ref["index"].astype(np.int64).tobytes() and rows.tobytes() == ref["xyz"].tobytes()
    assert 10 < len(ind) < 300


def test_scene_and_lever_arm(ictx, synth):
    """The bin scene with the floor off (six parts and strays, 0.8 m from the camera), and a part moved 0.8 m from the origin."""
    rest = rest_of_scene(synth)[0]
    assert 0.6 < np.linalg.norm(rest.mean(0)) < 1.0
    ref = check(ictx, rest, what="scene", salient_radius=0.012, non_max_radius=0.008)
    assert 50 < ref["n_keypoints"] < 0.1 * len(rest)
    far = _object(synth, 4000, offset=(0.5, -0.4, 0.48))
    ref = check(ictx, far, what="lever arm", salient_radius=0.008, non_max_radius=0.005)
    assert ref["n_keypoints"] > 10


# ---------------------------------------------------------------- 2. radii and parameters
@pytest.fixture(scope="module")
def cube():
    return np.random.default_rng(17).random((3000, 3)).astype(F)


def test_one_support_is_the_whole_cloud(ictx):
    """A shell around one centre point, salient_radius just past the shell: the centre's support is every finite row (at n = 5,000 its
    second moments pass 2^50), a shell point's a quarter of the cloud."""
    rng = np.random.default_rng(23)
    v = rng.normal(size=(5000, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    pts = (v * rng.uniform(0.97, 1.0, (5000, 1))).astype(F)
    pts[0] = 0.0; pts[7] = np.nan; pts[9, 1] = np.inf
    ref = check(ictx, pts, what="whole cloud", salient_radius=1.001, non_max_radius=0.06, min_neighbors=3)
    assert ref["n_finite"] == 4998 and ref["support"][0] == ref["n_finite"] and np.median(ref["support"]) > 1000


def test_every_support_is_one(ictx, cube):
    for mn in (5, 1):
        ref = check(ictx, cube, what="support 1", salient_radius=1e-7, non_max_radius=1e-7, min_neighbors=mn)
        assert (ref["support"] == 1).all() and ref["n_supported"] == (0 if mn == 5 else len(cube)) and ref["n_salient"] == 0


@pytest.mark.parametrize("rs,rn", [(0.13, 0.09), (0.09, 0.13)])
def test_non_max_radius_smaller_and_larger(ictx, cube, rs, rn):
    ref = check(ictx, cube, np.arange(3 * len(cube), dtype=F).reshape(-1, 3), what="radii", salient_radius=rs, non_max_radius=rn)
    assert ref["n_keypoints"] > 10


@pytest.mark.parametrize("rs", [0.125, float(np.nextafter(F(0.125), F(0))), 0.25, float(np.nextafter(F(0.25), F(0)))])
def test_frexp_edges(ictx, cube, rs):
    """salient_radius exactly at a power of two (m = 0.5: the binade above) and just below it (m just under 1)."""
    assert R.shift(0.125) == 22 and R.shift(np.nextafter(F(0.125), F(0))) == 23
    ref = check(ictx, cube, what="frexp", salient_radius=rs, non_max_radius=0.08)
    assert ref["n_keypoints"] > 10


def test_min_neighbors_and_gammas(ictx, cube):
    kw = dict(salient_radius=0.13, non_max_radius=0.09)
    ref = check(ictx, cube, what="min 1", min_neighbors=1, **kw)
    assert ref["n_supported"] == len(cube)
    ref = check(ictx, cube, what="min > any support", min_neighbors=100000, **kw)
    assert ref["n_supported"] == 0 and ref["n_keypoints"] == 0 and not ref["eigenvalues"].any()
    tight = check(ictx, cube, what="gamma 0.5", gamma_21=0.5, gamma_32=0.5, **kw)
    loose = check(ictx, cube, what="gamma 2", gamma_21=2.0, gamma_32=2.0, **kw)
    assert 0 < tight["n_salient"] < loose["n_salient"]
    assert loose["n_salient"] == int(((loose["support"] >= 5) & (loose["eigenvalues"][:, 2] > 0)).sum()) == loose["n_supported"]
    mixed = check(ictx, cube, what="gammas differ", gamma_21=0.6, gamma_32=float("inf"), **kw)
    assert tight["n_salient"] < mixed["n_salient"] < loose["n_salient"]


# ---------------------------------------------------------------- 3. attr and optional outputs
@pytest.mark.parametrize("width", [1, 3, 4, 33])
def test_attr_widths(ictx, synth, width):
    pts = _object(synth, 2500)
    attr = np.random.default_rng(width).random((len(pts), width)).astype(F)
    ref = check(ictx, pts, attr, what="attr", salient_radius=0.008, non_max_radius=0.005)
    assert ref["n_keypoints"] > 10 and ref["attr"].shape == (ref["n_keypoints"], width)


def test_attr_without_out_attr_and_no_output_at_all(ictx, tdv, synth):
    pts = _object(synth, 2500)
    n = len(pts)
    attr = np.random.default_rng(2).random((n, 4)).astype(F)
    kw = dict(salient_radius=0.008, non_max_radius=0.005)
    ref = R.iss(pts, attr, **kw)
    (pts_t, px), (attr_t, pa), (it, pi) = _up(pts), _up(attr), _up(np.full(n, -9, np.int32), np.int32)
    torch.cuda.synchronize()
    got = ictx.iss_keypoints_dev(px, n, pa, 4, d_index=pi, **kw)            # attr given, out_attr not
    torch.cuda.synchronize()
    assert [got[k] for k in R.COUNTS] == [ref[k] for k in R.COUNTS] and it[:got["n_keypoints"]].cpu().numpy().tobytes() == ref["index"].tobytes()
    got = ictx.iss_keypoints_dev(px, n, **kw)                               # every optional output NULL at once
    assert [got[k] for k in R.COUNTS] == [ref[k] for k in R.COUNTS]
    lib = tdv.lib()
    o = Outputs(tdv, n, 4)
    assert iss_call(lib, False, ictx._h, pts, attr, n, o, cols=False, attr_width=4, min_neighbors=5, **kw) == 0
    assert o.index[:ref["n_keypoints"]].tobytes() == ref["index"].tobytes() and o.mask.tobytes() == ref["mask"].tobytes()
    assert o.cols.tobytes() == np.full((n, 4), -7, F).tobytes() and (o.index[ref["n_keypoints"]:] == -7).all()
    res = tdv.IssResultC()
    p = tdv.iss_params(**kw)
    assert lib.tdv_iss_keypoints(ictx._h, pts.ctypes.data_as(C.c_void_p), n, C.byref(p), None, 0, C.byref(res), *[None] * 7) == 0
    assert [getattr(res, k) for k in R.COUNTS] == [ref[k] for k in R.COUNTS]


# ---------------------------------------------------------------- 4. default radii
def _default_clouds(synth):
    rng = np.random.default_rng(41)
    yield "object 2000", _object(synth, 2000)
    yield "object 9000", _object(synth, 9000, seed=12)
    yield "uniform 1000", rng.random((1000, 3)).astype(F)
    yield "dups 1000", _make("dups", 1000, rng)
    yield "nan rows 4097", _make("nan_rows", 4097, rng)
    yield "inf rows 65", _make("inf_rows", 65, rng)
    yield "one point", rng.random((1, 3)).astype(F)
    yield "four points", rng.random((4, 3)).astype(F)
    yield "all nan", np.full((70, 3), np.nan, F)
    yield "uniform 3000, not the exact sum", np.random.default_rng(43).random((3000, 3)).astype(F)


def test_default_radii(ictx, synth):
    for what, pts in _default_clouds(synth):
        attr = np.random.default_rng(len(pts)).random((len(pts), 3)).astype(F)
        ref = check_defaults(ictx, pts, attr, what=what)
        if what.endswith("not the exact sum"):                             # the fixed order's bits are not math.fsum's here: equality asks more than the bound
            assert np.float64(R.resolution(pts)[0]).tobytes() != np.float64(R.resolution_in_tree_order(pts)[0]).tobytes()
        if what.startswith("object"):
            assert 0.01 * len(pts) < ref["n_keypoints"] < 0.1 * len(pts), (what, ref["n_keypoints"])      # a few percent


def test_default_radii_when_every_point_is_a_duplicate(ictx):
    """resolution 0: both radii 0, r2 = 0, the neighbours are the exact copies; u = 0, every eigenvalue 0, no keypoint."""
    pts = np.repeat(np.random.default_rng(5).random((100, 3)).astype(F), 3, 0)
    for got in (ictx.iss(pts), dev_call(ictx, pts)):
        assert got["resolution"] == 0.0 and got["salient_radius"] == 0.0 and got["non_max_radius"] == 0.0
        assert (got["support"] == 3).all() and got["n_finite"] == 300 and got["n_supported"] == 0 and got["n_keypoints"] == 0
    got = ictx.iss(pts, min_neighbors=2)
    assert got["n_supported"] == 300 and not got["eigenvalues"].any() and got["n_salient"] == 0


# ---------------------------------------------------------------- 5. repeat calls, the chain
def test_two_calls_give_identical_bytes(ictx, synth):
    pts = _object(synth, 6000)
    attr = np.random.default_rng(4).random((len(pts), 33)).astype(F)

    def snap(r):
        return blob({k: v for k, v in r.items()})
    a = snap(ictx.iss(pts, attr))
    ictx.statistical_outlier(rest_of_scene(synth)[0], 20, 2.0)            # another user of the workspace, of another size
    assert snap(ictx.iss(pts, attr)) == a
    assert snap(dev_call(ictx, pts, attr)) == a                          # host == device, the resolution's bits included


def test_chain_into_ransac(ictx, synth):
    """(out_xyz, out_attr = FPFH rows) of the keypoints go into ransac_dev as they stand: the result is ransac_dev's on the same rows
    gathered with numpy."""
    tgt = synth.sample_object(3000, 3)[0]
    src = synth.make_scene(3000, 3)[0]
    src, _ = ictx.voxel_downsample(src, None, 0.004); tgt, _ = ictx.voxel_downsample(tgt, None, 0.004)
    fs = ictx.compute_fpfh(src, ictx.estimate_normals(src, 30), 0.02)
    ft = ictx.compute_fpfh(tgt, ictx.estimate_normals(tgt, 30), 0.02)
    n = len(src)
    (src_t, ps), (fs_t, pf), (tgt_t, pt), (ft_t, pft) = _up(src), _up(fs), _up(tgt), _up(ft)     # named: a dropped tensor is memory torch hands out again
    (xt, pxo), (at, pao), (it, pi) = _up(np.zeros((n, 3), F)), _up(np.zeros((n, 33), F)), _up(np.zeros(n, np.int32), np.int32)
    torch.cuda.synchronize()                                             # the ctx runs on a stream of its own
    res = ictx.iss_keypoints_dev(ps, n, pf, 33, d_index=pi, d_out_xyz=pxo, d_out_attr=pao)
    m = res["n_keypoints"]
    assert 10 <= m < n / 4
    a = ictx.ransac_dev(pxo, m, pt, len(tgt), pao, pft, None, 0.004, 20000, 0.999, 42)
    torch.cuda.synchronize()
    ind = it[:m].cpu().numpy()
    assert (np.diff(ind) > 0).all() and xt[:3 * m].cpu().numpy().tobytes() == src[ind].tobytes() and at[:33 * m].cpu().numpy().tobytes() == fs[ind].tobytes()
    (gs_t, pgs), (gf_t, pgf) = _up(src[ind]), _up(fs[ind])
    b = ictx.ransac_dev(pgs, m, pt, len(tgt), pgf, pft, None, 0.004, 20000, 0.999, 42)
    assert blob(a) == blob(b)


# ---------------------------------------------------------------- 6. arguments
@pytest.mark.parametrize("case", range(1, len(BAD)))
def test_bad_parameters_on_a_real_ctx(ictx, tdv, case):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F)
    for dev in (False, True):                                            # refused before any pointer is looked at: host arrays serve both
        o = Outputs(tdv, 4)
        assert iss_call(lib, dev, ictx._h, pts, pts, 4, o, **BAD[case][1]) == TDV_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert o.untouched()


def test_null_arrays_on_a_real_ctx_then_a_good_call(ictx, tdv):
    lib = tdv.lib()
    pts = np.random.default_rng(1).random((40, 3)).astype(F)
    attr = np.random.default_rng(2).random((40, 3)).astype(F)
    for dev in (False, True):
        o = Outputs(tdv, 40)
        for status in null_and_size_cases(lib, dev, ictx._h, pts, attr, 40, o):
            assert status == TDV_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert o.untouched()
    o = Outputs(tdv, 40)
    assert iss_call(lib, False, ictx._h, pts, attr, 40, o) == 0           # the ctx goes on working
    ref = R.iss(pts, attr, salient_radius=0.3, non_max_radius=0.2, min_neighbors=2)
    m = ref["n_keypoints"]
    assert o.res.n_keypoints == m and o.mask.tobytes() == ref["mask"].tobytes() and o.saliency.tobytes() == ref["saliency"].tobytes()
    assert o.cols[:m].tobytes() == ref["attr"].tobytes() and (o.index[m:] == -7).all() and (o.cols[m:] == -7).all()
