"""Euclidean clustering on the device (include/tdv_hip.h: tdv_cluster_dbscan), against the restatement of tests/cluster_restatement.py.

Every output is an integer or a row of the input, so everything is compared byte for byte: labels, every field of the result, order,
offsets and the grouped coordinates, from the host and the device entry point.  Every test runs on a Context of its own."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import cluster_restatement as R
from test_cluster_abi import BAD, GOOD, Outputs, call, rest_of_scene
from test_gpu_fuzz import _make

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32


@pytest.fixture
def cctx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def _same(ref, res, labels, order, offsets, grouped, what):
    assert res == ref["result"], (what, res, ref["result"])
    assert labels.tobytes() == ref["labels"].tobytes(), what
    assert order.tobytes() == ref["order"].tobytes(), what
    assert np.asarray(offsets, np.int32).tobytes() == ref["offsets"].tobytes(), (what, offsets, ref["offsets"])
    assert grouped.tobytes() == ref["grouped"].tobytes(), what


def check(ctx, pts, eps, min_points, min_cluster_size=1, what=None, ref=None):
    """Host and device entry points against the restatement; returns the restatement's dict."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    what = (what, n, eps, min_points, min_cluster_size)
    ref = ref or R.cluster(pts, eps, min_points, min_cluster_size)
    res, labels, order, offsets, grouped = ctx.cluster(pts, eps, min_points, min_cluster_size, grouped=True)
    _same(ref, res, labels, order, offsets, grouped, what + ("host",))
    (_, px), (lt, pl), (ot, po), (gt, pg) = _up(pts), _up(np.full(n, -9, np.int32), np.int32), _up(np.full(n, -9, np.int32), np.int32), _up(np.zeros((n, 3), F))
    dres, doff = ctx.cluster_dbscan_dev(px, n, eps, min_points, min_cluster_size, d_labels=pl, d_order=po, d_grouped=pg)
    torch.cuda.synchronize()
    _same(ref, dres, lt[:n].cpu().numpy(), ot[:n].cpu().numpy(), doff, gt[:3 * n].cpu().numpy().reshape(-1, 3), what + ("dev",))
    return ref


# ---------------------------------------------------------------- 1. the scene
@pytest.fixture(scope="module")
def rest(synth):
    return rest_of_scene(synth)[0]


@pytest.mark.parametrize("eps,min_points", R.PARAMS)
def test_scene_equals_the_restatement(cctx, rest, eps, min_points):
    ref = check(cctx, rest, eps, min_points, what="scene")
    assert ref["result"]["n_clusters"] >= 6


def test_scene_with_min_cluster_size(cctx, rest):
    for eps, mp in R.PARAMS:
        ref = check(cctx, rest, eps, mp, 20, what="scene, min_cluster_size")
        assert ref["result"]["n_clusters"] == 6
    assert ref["result"]["n_dropped"] >= 1                              # the speck at 8 mm / 5


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_scene_with_non_finite_strays(cctx, synth, value):
    rest = rest_of_scene(synth, stray_value=value)[0]
    bad = ~np.isfinite(rest).all(1)
    assert bad.sum() == R.SCENE["n_stray"]                               # the plane leaves them in the rest cloud
    for eps, mp in R.PARAMS:
        ref = check(cctx, rest, eps, mp, what="scene, strays %r" % value)
        assert (ref["labels"][bad] == -1).all() and ref["result"]["n_clusters"] >= 6


# ---------------------------------------------------------------- 2. fuzz
KINDS = ["uniform", "flat", "line", "grid", "dups", "clusters", "offset", "tiny", "nan_rows", "inf_rows", "huge"]
SIZES = [1, 2, 63, 64, 65, 1000, 4097, 30011]
LARGE = 200003


def _eps_for(pts, k, rng):
    """A radius at which a typical clean point has about k neighbours (the median distance to the k-th of a sample): the parameters of
    the fuzz, not its expectation."""
    from scipy.spatial import cKDTree
    clean = pts[(np.abs(pts) < 1e18).all(1)].astype(np.float64)
    if len(clean) <= k:
        return 0.1
    tree = cKDTree(clean)
    d, _ = tree.query(clean[rng.integers(0, len(clean), 200)], k + 1)
    e = float(np.median(d[:, k]))
    return e if e > 0 else 1e-6


def _cases(kind, pts, rng, large):
    if kind == "grid":                                                   # pitch 0.01 in f64, rounded to f32: d2 lands on either side of eps2
        return [(0.01, 7), (0.0142, 15)] if large else [(0.01, 5), (0.01, 7), (0.0142, 12)]
    e8 = _eps_for(pts, 8, rng)
    if large:                                                            # a low and a high min_points: the count pass ends early, or not
        return [(e8, 6), (_eps_for(pts, 24, rng), 20)]
    return [(e8, 5), (e8, 12), (_eps_for(pts, 16, rng), 8), (e8, 1)]


@pytest.mark.parametrize("kind", KINDS)
def test_fuzz(cctx, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 7)
    for n in SIZES + [LARGE]:
        pts = _make(kind, n, rng)
        for k, (eps, mp) in enumerate(_cases(kind, pts, rng, n == LARGE)):
            check(cctx, pts, eps, mp, 1 if k % 2 == 0 else 3, what=kind)


def test_min_points_above_n_and_huge_eps(cctx):
    rng = np.random.default_rng(11)
    pts = rng.random((3000, 3)).astype(F)
    ref = check(cctx, pts, 0.05, 3001, what="min_points > n")
    assert ref["result"] == dict(n_clusters=0, n_core=0, n_border=0, n_noise=3000, n_dropped=0, largest=0, n_labelled=0)
    ref = check(cctx, pts, 10.0, 5, what="huge eps")
    assert ref["result"]["n_clusters"] == 1 and ref["result"]["largest"] == 3000 and (ref["labels"] == 0).all()
    ref = check(cctx, pts, 1e20, 3000, what="eps2 overflows")            # eps2 = +inf: every finite d2 passes
    assert ref["result"]["n_clusters"] == 1 and ref["result"]["n_core"] == 3000
    res, labels, order, offsets = cctx.cluster(np.zeros((0, 3), F), 0.1, 3)
    assert res == dict(n_clusters=0, n_core=0, n_border=0, n_noise=0, n_dropped=0, largest=0, n_labelled=0)
    assert len(labels) == 0 and len(order) == 0 and offsets.tolist() == [0]
    assert cctx.cluster_dbscan(pts, 10.0, 5).tobytes() == np.zeros(3000, np.int32).tobytes()       # Open3D's shape


# ---------------------------------------------------------------- 3. workspace reuse
def test_repeatable_and_after_an_unrelated_call(cctx, rest, synth):
    a = cctx.cluster(rest, 0.010, 10, grouped=True)
    b = cctx.cluster(rest, 0.010, 10, grouped=True)
    cctx.segment_planes(R.scene(synth)[0], **R.PLANE)                    # another user of the workspace, of another size
    small = cctx.cluster(rest[:5000], 0.02, 4, 2, grouped=True)
    c = cctx.cluster(rest, 0.010, 10, grouped=True)
    for other in (b, c):
        assert other[0] == a[0]
        for x, y in zip(other[1:], a[1:]):
            assert x.tobytes() == y.tobytes()
    ref = R.cluster(rest[:5000], 0.02, 4, 2)
    _same(ref, *small, "small")


# ---------------------------------------------------------------- 4. arguments
@pytest.mark.parametrize("case", range(1, len(BAD)))
def test_bad_parameters_on_a_real_ctx(cctx, tdv, case):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F)
    p = tdv.cluster_params(**dict(GOOD, **BAD[case][1]))
    o = Outputs(tdv, 4)
    assert call(lib.tdv_cluster_dbscan, cctx._h, pts, 4, C.byref(p), o) == TDV_ERR_BAD_ARG
    assert o.untouched()
    (lt, pl), (ot, po), (gt, pg), (_, px) = _up(np.full(4, -7, np.int32), np.int32), _up(np.full(4, -7, np.int32), np.int32), _up(np.full(12, -7, F)), _up(pts)
    st = lib.tdv_cluster_dbscan_dev(cctx._h, C.c_void_p(px), 4, C.byref(p), C.byref(o.res), C.c_void_p(pl), C.c_void_p(po), C.c_void_p(pg),
                                    o.offsets.ctypes.data_as(C.c_void_p), 4, C.byref(o.nl))
    torch.cuda.synchronize()
    assert st == TDV_ERR_BAD_ARG and o.untouched()
    assert lt.cpu().tolist() == [-7] * 4 and ot.cpu().tolist() == [-7] * 4 and gt.cpu().tolist() == [-7.0] * 12


def test_null_arrays_on_a_real_ctx(cctx, tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); p = tdv.cluster_params(**GOOD)
    for fn in (lib.tdv_cluster_dbscan, lib.tdv_cluster_dbscan_dev):      # refused before any pointer is looked at: host arrays serve both
        o = Outputs(tdv, 4)
        assert call(fn, cctx._h, None, 4, C.byref(p), o) == TDV_ERR_BAD_ARG
        assert call(fn, cctx._h, pts, -1, C.byref(p), o) == TDV_ERR_BAD_ARG
        assert call(fn, cctx._h, pts, 4, None, o) == TDV_ERR_BAD_ARG
        assert call(fn, cctx._h, pts, 4, C.byref(p), o, res=False) == TDV_ERR_BAD_ARG
        assert call(fn, cctx._h, pts, 4, C.byref(p), o, cap=-1) == TDV_ERR_BAD_ARG
        assert call(fn, cctx._h, pts, 4, C.byref(p), o, offsets=False, cap=2) == TDV_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert o.untouched()


def test_offsets_capacity_too_small_then_right(cctx, tdv, rest):
    lib = tdv.lib()
    n = len(rest)
    ref = R.cluster(rest, 0.008, 5)
    k = ref["result"]["n_clusters"]
    assert k >= 6
    p = tdv.cluster_params(eps=0.008, min_points=5)
    for fn, dev in ((lib.tdv_cluster_dbscan, False), (lib.tdv_cluster_dbscan_dev, True)):
        res = tdv.ClusterResultC(); nl = C.c_int(-7)
        labels = np.full(n, -7, np.int32); offsets = np.full(k + 1, -7, np.int32)
        lt, pl = _up(labels, np.int32)
        _, px = _up(rest)
        src, lab = (C.c_void_p(px), C.c_void_p(pl)) if dev else (rest.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p))
        P = offsets.ctypes.data_as(C.c_void_p)
        for cap, off in ((k - 1, P), (0, None)):                         # too small; the query
            assert fn(cctx._h, src, n, C.byref(p), C.byref(res), lab, None, None, off, cap, C.byref(nl)) == TDV_ERR_BAD_ARG
            torch.cuda.synchronize()
            got = lt[:n].cpu().numpy() if dev else labels
            assert {f: getattr(res, f) for f, _ in tdv.ClusterResultC._fields_} == {f: v for f, v in ref["result"].items() if f != "n_labelled"}
            assert nl.value == ref["result"]["n_labelled"] and got.tobytes() == ref["labels"].tobytes()
            assert (offsets == -7).all()
        assert fn(cctx._h, src, n, C.byref(p), C.byref(res), lab, None, None, P, res.n_clusters, C.byref(nl)) == 0
        assert offsets.tobytes() == ref["offsets"].tobytes()


# ---------------------------------------------------------------- 5. what it is for
def test_frame_to_planes_to_clusters_to_batch_icp(cctx, synth):
    """segment_planes_dev writes the rest cloud, cluster_dbscan_dev groups it, and (d_grouped, offsets) goes into icp_batch_dev as it
    is: per cluster the batch returns what icp_dev returns on that cluster's rows, bit for bit - with no mask from outside."""
    pts, part = R.scene(synth)
    n = len(pts)
    (_, px), (rt, pr) = _up(pts), _up(np.zeros((n, 3), F))
    planes, n_rest = cctx.segment_planes_dev(px, n, d_rest=pr, **R.PLANE)
    assert len(planes) == 1 and n_rest > 20000
    gt, pg = _up(np.zeros((n_rest, 3), F))
    res, off = cctx.cluster_dbscan_dev(pr, n_rest, 0.010, 10, min_cluster_size=20, d_grouped=pg)
    torch.cuda.synchronize()
    assert res["n_clusters"] == 6 and off[-1] == res["n_labelled"]
    ref = R.cluster(rt[:3 * n_rest].cpu().numpy().reshape(-1, 3), 0.010, 10, 20)
    grouped = gt[:3 * n_rest].cpu().numpy().reshape(-1, 3)
    assert off.tobytes() == ref["offsets"].tobytes() and grouped.tobytes() == ref["grouped"].tobytes()
    model, nrm = synth.sample_object(8000, 1)
    (_, pm), (_, pn) = _up(model), _up(nrm)
    T0s = []
    for b in range(6):
        T = np.eye(4, dtype=F)
        T[:3, 3] = model.mean(0) - grouped[off[b]:off[b + 1]].mean(0)
        T0s.append(T)
    got = cctx.icp_batch_dev(pg, off, pm, pn, len(model), T0s, 0.02, 15, True)
    assert len(got) == 6
    for b in range(6):
        one = cctx.icp_dev(pg + 12 * int(off[b]), int(off[b + 1] - off[b]), pm, pn, len(model), T0s[b], 0.02, 15, True)
        assert got[b].transformation.tobytes() == one.transformation.tobytes(), b
        assert (np.float32(got[b].fitness).tobytes(), np.float32(got[b].rmse).tobytes(), got[b].iterations, got[b].n_corr) == \
               (np.float32(one.fitness).tobytes(), np.float32(one.rmse).tobytes(), one.iterations, one.n_corr), b
        assert got[b].n_corr > 0.5 * (off[b + 1] - off[b])
