"""Outlier removal on the device (include/tdv_hip.h: tdv_remove_statistical_outlier, tdv_remove_radius_outlier) against the restatement
of tests/outlier_restatement.py, from the host and the device entry points.

Byte for byte: n_valid, n_kept, mask, index, the kept xyz / rgb rows, the radius counts and the per-point mean (an f64 array: rule 2
fixes every bit of it) - and cloud_mean, std_dev and threshold, against rule 4 restated in the header's own order of additions
(outlier_restatement's "tree" form over tests/fixed_tree_restatement.py; a NaN where the restatement has one).  The three doubles of the
device AND of that restatement are also held to the exact-sum values within the bounds of outlier_restatement.statistics_bounds, which
come from the tree's depth alone (its depth times 2^-53, plus the way the error of cloud_mean enters the deviation sum: written out in that
function's docstring; nothing in it is measured on the device, and it stays below 1e-12 relative).  With equal thresholds the mask needs
no gap condition: test_means_on_the_threshold_and_tree_edges runs the inputs on which every mean lies at the threshold.  The older cases
still assert the gap, which there makes the exact-sum mask the same mask.  Every test runs on a Context of
its own."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

import cluster_restatement as CR
import outlier_restatement as R
import plane_restatement as PR
from test_cluster_abi import rest_of_scene
from test_gpu_cluster import KINDS, SIZES, LARGE, _eps_for
from test_gpu_fuzz import _make
from test_outlier_abi import BAD_RAD, BAD_STAT, SCENE_PARAMS, Outputs, rad_call, stat_call

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
RADIUS_PARAMS = [(5, 0.008), (10, 0.010), (16, 0.012)]
NB_NEIGHBORS = [2, 20, 64, 65, 192, 193, 255]
# The k of a case is its kind's index plus its size's, through NB_NEIGHBORS.  Two kinds are shifted: without it a grid of 64 or 65 points
# met k = 2 (every mean is half the one pitch: no deviation, every mean ON the threshold; the shift puts k = 2 on the grid of 1000)
# and the huge rows at 64 points met k = n (every list holds a 1e19 row): inputs that violate the gap condition whatever their seed.
# test_means_on_the_threshold_and_tree_edges runs exactly those, against the restatement in the header's order, which needs no gap.
K_SHIFT = {"grid": 6, "huge": 1}


@pytest.fixture
def octx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def _same_doubles(ref, got, n, ratio, what):
    bounds = R.statistics_bounds(ref, n, ratio)
    for key, b in zip(("cloud_mean", "std_dev", "threshold"), bounds):
        r, g = float(ref[key]), float(got[key])
        print(what, key, "ref %.17g got %.17g bound %.3g" % (r, g, b))
        if math.isnan(r):
            assert math.isnan(g), (what, key, g)
        else:
            assert abs(g - r) <= b, (what, key, r, g, b)
            sd = float(ref["std_dev"]) if ref["n_valid"] > 1 else 0.0      # (one valid point: std_dev is NaN and the bounds are 0)
            assert b <= 1e-12 * (abs(float(ref["cloud_mean"])) + abs(ratio) * sd + abs(r)), (what, key, b)
        t = np.float64(ref["tree"][key])                                  # rule 4 in the header's own order: the same bytes
        print(what, key, "restated in the header's order %.17g (%s) got (%s)" % (t, t.tobytes().hex(), np.float64(g).tobytes().hex()))
        if np.isnan(t):
            assert math.isnan(g) and math.isnan(r), (what, key, g)
        else:
            assert np.float64(g).tobytes() == t.tobytes(), (what, key, "device %.17g restated order %.17g" % (g, t))
            assert abs(float(t) - r) <= b, (what, key, "the restated order against the exact sum", float(t), r, b)


def _same(ref, got, what, per="mean"):
    assert (got["n_valid"], got["n_kept"]) == (ref["n_valid"], ref["n_kept"]), (what, got["n_valid"], got["n_kept"], ref["n_valid"], ref["n_kept"])
    for k in ("mask", per, "index", "xyz", "rgb"):
        if ref[k] is not None:
            assert np.ascontiguousarray(got[k]).tobytes() == ref[k].tobytes(), (what, k)


def _dev_call(ctx, statistical, pts, rgb, a, b):
    n = len(pts)
    (_, px), (mt, pm), (it, pi), (xt, pxo) = _up(pts), _up(np.full(n, 9, np.uint8), np.uint8), _up(np.full(n, -9, np.int32), np.int32), _up(np.zeros((n, 3), F))
    pt, pp = _up(np.zeros(n), np.float64 if statistical else np.int32)
    (_, pr), (ct, pc) = (_up(rgb), _up(np.zeros((n, 3), F))) if rgb is not None else ((None, None), (None, None))
    fn = ctx.remove_statistical_outlier_dev if statistical else ctx.remove_radius_outlier_dev
    res = fn(px, n, a, b, pr, pm, pp, pi, pxo, pc)
    torch.cuda.synchronize()
    m = res["n_kept"]
    res.update(mask=mt[:n].cpu().numpy(), index=it[:m].cpu().numpy(), xyz=xt[:3 * m].cpu().numpy().reshape(-1, 3),
               rgb=None if rgb is None else ct[:3 * m].cpu().numpy().reshape(-1, 3))
    res["mean" if statistical else "count"] = pt[:n].cpu().numpy()
    return res


def check_stat(ctx, pts, k, ratio, rgb=None, what=None, ref=None, gap=True):
    """Both entry points against the restatement in the header's order (ref["tree"]), byte for byte.  gap: the inputs are also asserted to
    leave a gap at the threshold, and then the exact-sum form keeps the same rows."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    what = (what, len(pts), k, ratio)
    ref = ref or R.statistical(pts, k, ratio, rgb)
    if gap:
        assert R.gap_ok(ref, len(pts), ratio), ("gap condition", what)
        assert ref["mask"].tobytes() == ref["tree"]["mask"].tobytes(), ("the two restatements keep different rows across a gap", what)
    for name, got in (("host", ctx.statistical_outlier(pts, k, ratio, rgb)), ("dev", _dev_call(ctx, True, pts, rgb, k, ratio))):
        _same_doubles(ref, got, len(pts), ratio, what + (name,))
        _same(ref["tree"], got, what + (name,))
    return ref


def check_rad(ctx, pts, nb, radius, rgb=None, what=None):
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    what = (what, len(pts), nb, radius)
    ref = R.radius(pts, nb, radius, rgb)
    for name, got in (("host", ctx.radius_outlier(pts, nb, radius, rgb)), ("dev", _dev_call(ctx, False, pts, rgb, nb, radius))):
        assert (got["cloud_mean"], got["std_dev"], got["threshold"]) == (0.0, 0.0, 0.0), what
        _same(ref, got, what + (name,), per="count")
    return ref


# ---------------------------------------------------------------- 1. the scene
@pytest.fixture(scope="module")
def scene(synth):
    rest, part = rest_of_scene(synth)
    return rest, part, {p: R.statistical(rest, *p) for p in SCENE_PARAMS}


@pytest.mark.parametrize("k,ratio", SCENE_PARAMS)
def test_scene_statistical(octx, scene, k, ratio):
    rest, part, refs = scene
    ref = check_stat(octx, rest, k, ratio, what="scene", ref=refs[(k, ratio)])
    assert (ref["mask"][part == -2] == 0).all() and (ref["mask"][part >= 0] == 1).all()


@pytest.mark.parametrize("nb,radius", RADIUS_PARAMS)
def test_scene_radius(octx, scene, nb, radius):
    rest, part, _ = scene
    rgb = np.random.default_rng(3).random((len(rest), 3)).astype(F)
    ref = check_rad(octx, rest, nb, radius, rgb, what="scene")
    assert (ref["mask"][part == -2] == 0).all()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_scene_with_non_finite_strays(octx, synth, value):
    rest = rest_of_scene(synth, stray_value=value)[0]
    bad = ~np.isfinite(rest).all(1)
    assert bad.sum() == CR.SCENE["n_stray"]
    ref = check_stat(octx, rest, 20, 2.0, what="scene, strays %r" % value)
    assert (ref["mask"][bad] == 0).all() and not ref["valid"][bad].any()
    ref = check_rad(octx, rest, 10, 0.010, what="scene, strays %r" % value)
    assert (ref["count"][bad] == 0).all()


# ---------------------------------------------------------------- 2. fuzz
def fuzz_cases(kind):
    """(n, nb_neighbors, std_ratio, points): every size of the clustering fuzz, the row widths' k spread over kinds and sizes."""
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 23)
    for s, n in enumerate(SIZES):
        k = NB_NEIGHBORS[(KINDS.index(kind) + s + K_SHIFT.get(kind, 0)) % len(NB_NEIGHBORS)]
        yield n, k, (2.0, 1.0, -0.5)[s % 3], _make(kind, n, rng)
    if kind == "uniform":
        yield LARGE, 20, 2.0, _make(kind, LARGE, rng)


@pytest.mark.parametrize("kind", KINDS)
def test_fuzz(octx, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 29)
    for n, k, ratio, pts in fuzz_cases(kind):
        rgb = rng.random((n, 3)).astype(F) if n % 2 else None
        check_stat(octx, pts, k, ratio, rgb, what=kind)
        eps = 0.01 if kind == "grid" else _eps_for(pts, 8, rng)
        check_rad(octx, pts, (k // 8) if n < LARGE else 6, eps, rgb, what=kind)


def _on_threshold_cases():
    """(what, points, nb_neighbors, std_ratio): the inputs K_SHIFT steers the fuzz around, and the edges of the tree."""
    rng = np.random.default_rng(61)
    for n in (64, 65):                                                   # every mean is half a pitch: no deviation, every mean AT the threshold
        yield "grid, k = 2", _make("grid", n, rng), 2, (2.0, 0.0, -0.5)[n % 3]
    huge = _make("huge", 64, rng)
    yield "huge rows, k = n", huge, 64, 1.0                              # every list holds a 1e19 row
    a = rng.random((1, 3)).astype(F)
    b, c = (a + F(0.25)).astype(F), (a - F(0.125)).astype(F)
    yield "n_valid = 0", np.repeat(a, 10, 0), 3, 2.0                     # every list is copies of the query: mean 0, not valid
    yield "n_valid = 1", np.concatenate([np.repeat(a, 3, 0), b]), 2, 2.0
    yield "n_valid = 2", np.concatenate([np.repeat(a, 3, 0), b, c]), 2, 2.0
    for n in (255, 256, 257, 65537):                                     # one workgroup short, full, two; 257 partials: two terms in thread 0
        yield "uniform", rng.random((n, 3)).astype(F), 20 if n < 60000 else 4, 2.0


@pytest.mark.parametrize("case", range(13))
def test_means_on_the_threshold_and_tree_edges(octx, case):
    """No gap condition: cloud_mean, std_dev and threshold are the restated order's bytes, so mask, index and the kept rows are held byte
    for byte where every mean lies on the threshold, where n_valid is 0, 1 or 2, and at the sizes where the tree changes shape."""
    cases = list(_on_threshold_cases())
    assert len(cases) == 13 - 3
    if case >= len(cases):                                               # the three grid / huge cases again, with colours
        what, pts, k, ratio = cases[case - len(cases)]
        rgb = np.random.default_rng(case).random((len(pts), 3)).astype(F)
    else:
        (what, pts, k, ratio), rgb = cases[case], None
    ref = check_stat(octx, pts, k, ratio, rgb, what=what, gap=False)
    nv = ref["tree"]["n_valid"]
    print(what, len(pts), "n_valid", nv, "kept", ref["tree"]["n_kept"], "gap", R.gap_ok(ref, len(pts), ratio))
    if what.startswith("n_valid"):
        assert nv == int(what[-1]) and (nv > 1 or ref["tree"]["n_kept"] == 0)
    if what == "uniform" and len(pts) == 256:                            # the fixed order's bits are not math.fsum's here: equality asks more than the bound
        assert np.float64(ref["cloud_mean"]).tobytes() != np.float64(ref["tree"]["cloud_mean"]).tobytes()
    if what.startswith("grid"):
        mv = ref["mean"][ref["valid"]]
        assert nv == len(pts) and np.ptp(mv) <= 1e-6 * mv.max()           # the means are one value up to the f32 rounding of the pitch


def test_empty_cloud_and_open3d_shapes(octx):
    r = octx.statistical_outlier(np.zeros((0, 3), F), 20, 2.0)
    assert (r["n_valid"], r["n_kept"]) == (0, 0) and np.isnan([r["cloud_mean"], r["std_dev"], r["threshold"]]).all() and len(r["index"]) == 0
    r = octx.radius_outlier(np.zeros((0, 3), F), 3, 0.1)
    assert (r["n_valid"], r["n_kept"], r["threshold"]) == (0, 0, 0.0)
    rng = np.random.default_rng(8)
    pts = rng.random((3000, 3)).astype(F); rgb = rng.random((3000, 3)).astype(F)
    ref = R.statistical(pts, 12, 1.0, rgb)
    rows, ind = octx.remove_statistical_outlier(pts, 12, 1.0)
    assert ind.dtype == np.int64 and ind.tobytes() == ref["index"].astype(np.int64).tobytes() and rows.tobytes() == ref["xyz"].tobytes()
    rows, cols, ind = octx.remove_radius_outlier(pts, 4, 0.05, rgb)
    ref = R.radius(pts, 4, 0.05, rgb)
    assert ind.tobytes() == ref["index"].astype(np.int64).tobytes() and cols.tobytes() == ref["rgb"].tobytes() and rows.tobytes() == ref["xyz"].tobytes()


# ---------------------------------------------------------------- 3. cross-checks on the device
@pytest.mark.parametrize("n,k", [(5000, 20), (3001, 70), (700, 200)])
def test_mean_equals_the_sum_over_the_normals_knn_lists(octx, n, k):
    """Rule 1 says the lists are tdv_estimate_normals_dev's: rule 2 applied on the host to d_knn gives the device's mean byte for byte."""
    pts = np.random.default_rng(n).random((n, 3)).astype(F)
    pts[5] = pts[6]
    (_, px), (_, pn), (kt, pk), (mt, pm) = _up(pts), _up(np.zeros((n, 3), F)), _up(np.zeros((n, k), np.int32), np.int32), _up(np.zeros(n), np.float64)
    octx.estimate_normals_dev(px, n, k, pn, pk)
    octx.remove_statistical_outlier_dev(px, n, k, 2.0, d_mean=pm)
    torch.cuda.synchronize()
    knn = kt[:n * k].cpu().numpy().reshape(n, k)
    assert (knn >= 0).all()
    d2 = R.d2_knn_f32(pts[knn], pts[:, None, :])
    want = np.add.accumulate(np.sqrt(d2.astype(np.float64)), axis=1)[:, -1] / np.float64(k)
    assert mt[:n].cpu().numpy().tobytes() == want.tobytes()


def test_radius_mask_is_the_core_count_of_clustering(octx, scene):
    rest = scene[0]
    n = len(rest)
    for nb, radius in RADIUS_PARAMS:
        (_, px), (lt, pl), (mt, pm) = _up(rest), _up(np.zeros(n, np.int32), np.int32), _up(np.zeros(n, np.uint8), np.uint8)
        res, _ = octx.cluster_dbscan_dev(px, n, radius, nb + 1, d_labels=pl)
        got = octx.remove_radius_outlier_dev(px, n, nb, radius, d_mask=pm)
        torch.cuda.synchronize()
        mask, labels = mt[:n].cpu().numpy() == 1, lt[:n].cpu().numpy()
        assert got["n_kept"] == res["n_core"] == int(mask.sum())
        assert (labels[mask] >= 0).all() and int((labels >= 0).sum()) == res["n_core"] + res["n_border"]
        assert np.array_equal(mask, CR.cluster(rest, radius, nb + 1)["core"])


def test_two_calls_give_identical_bytes(octx, scene, synth):
    rest = scene[0]
    rgb = np.random.default_rng(4).random((len(rest), 3)).astype(F)

    def snap(r, per):
        return (r["n_valid"], r["n_kept"]) + tuple(np.float64(r[k]).tobytes() for k in ("cloud_mean", "std_dev", "threshold")) + \
            tuple(np.ascontiguousarray(r[k]).tobytes() for k in ("mask", per, "index", "xyz", "rgb"))
    a = snap(octx.statistical_outlier(rest, 20, 2.0, rgb), "mean")
    ra = snap(octx.radius_outlier(rest, 5, 0.008, rgb), "count")
    octx.segment_planes(CR.scene(synth)[0], **CR.PLANE)                  # another user of the workspace, of another size
    assert snap(octx.statistical_outlier(rest, 20, 2.0, rgb), "mean") == a
    assert snap(_dev_call(octx, True, rest, rgb, 20, 2.0), "mean") == a
    assert snap(octx.radius_outlier(rest, 5, 0.008, rgb), "count") == ra


# ---------------------------------------------------------------- 4. device-resident chain at frame size
W, H, FX, FY, CX, CY, SCALE, ZMAX = 1280, 720, 900.0, 900.0, 640.0, 360.0, 0.001, 2.0


def _frame():
    """A depth frame (uint16 mm) of a floor tilted 20 degrees, 1 m from the camera, the 6 cm high tops of two boxes on it, and 150
    flying pixels between 10 and 40 cm above the floor."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    rx, ry = (u - CX) / FX, (v - CY) / FY
    nrm = np.array([0.0, -math.sin(math.radians(20)), -math.cos(math.radians(20))])
    z = 1.0 / -(nrm[0] * rx + nrm[1] * ry + nrm[2])
    box = ((np.abs(u - 400) < 90) | (np.abs(u - 860) < 90)) & (np.abs(v - 400) < 70)
    z = np.where(box, z - 0.06, z)
    rng = np.random.default_rng(12)
    fu, fv = rng.integers(0, W, 150), rng.integers(0, H, 150)
    z[fv, fu] -= rng.uniform(0.10, 0.40, 150)
    return np.round(z / SCALE).astype(np.uint16)


def test_device_chain_at_frame_size(octx, orc):
    """depth_to_cloud_dev -> segment_planes_dev (rest cloud) -> the statistical filter -> cluster_dbscan_dev with no host copy of a cloud in
    between, each stage held to its restatement on the previous stage's restated output."""
    raw = _frame()
    cloud = orc.unproject(orc.depth_preprocess(raw, None, 1.0 / SCALE), None, FX, FY, CX, CY, ZMAX)[0]
    d_raw = torch.from_numpy(raw.reshape(-1).view(np.int16).copy()).to(DEV)
    d_xyz = torch.zeros(W * H * 3, dtype=torch.float32, device=DEV)
    n = octx.depth_to_cloud_dev(d_raw.data_ptr(), None, None, W, H, 1.0 / SCALE, FX, FY, CX, CY, ZMAX, d_xyz.data_ptr(), None, W * H)
    assert n == len(cloud) > 900000
    d_rest = torch.zeros(n * 3, dtype=torch.float32, device=DEV)
    params = dict(max_planes=1, distance_threshold=0.005, num_iterations=100)
    planes, n_rest = octx.segment_planes_dev(d_xyz.data_ptr(), n, d_rest=d_rest.data_ptr(), **params)
    d_kept = torch.zeros(n_rest * 3, dtype=torch.float32, device=DEV)
    d_ind = torch.zeros(n_rest, dtype=torch.int32, device=DEV)
    res = octx.remove_statistical_outlier_dev(d_rest.data_ptr(), n_rest, 20, 2.0, d_index=d_ind.data_ptr(), d_out_xyz=d_kept.data_ptr())
    m = res["n_kept"]
    d_lab = torch.zeros(m, dtype=torch.int32, device=DEV)
    cres, off = octx.cluster_dbscan_dev(d_kept.data_ptr(), m, 0.008, 10, min_cluster_size=50, d_labels=d_lab.data_ptr())
    torch.cuda.synchronize()
    assert d_xyz[:3 * n].cpu().numpy().tobytes() == cloud.tobytes()
    seg = PR.segment_planes(cloud, params)
    assert len(planes) == 1 and n_rest == len(seg["rest"]) and d_rest[:3 * n_rest].cpu().numpy().tobytes() == seg["rest"].tobytes()
    ref = R.statistical(seg["rest"], 20, 2.0)
    assert R.gap_ok(ref, n_rest, 2.0)
    _same_doubles(ref, res, n_rest, 2.0, "chain")
    assert (res["n_valid"], m) == (ref["n_valid"], ref["n_kept"]) and 0 < n_rest - m < 2000
    assert d_ind[:m].cpu().numpy().tobytes() == ref["index"].tobytes() and d_kept[:3 * m].cpu().numpy().tobytes() == ref["xyz"].tobytes()
    cref = CR.cluster(ref["xyz"], 0.008, 10, 50)
    assert cres == cref["result"] and cres["n_clusters"] == 2 and d_lab.cpu().numpy().tobytes() == cref["labels"].tobytes()
    assert off.tobytes() == cref["offsets"].tobytes()


# ---------------------------------------------------------------- 5. arguments
@pytest.mark.parametrize("case", range(1, len(BAD_STAT)))
def test_statistical_bad_parameters_on_a_real_ctx(octx, tdv, case):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F)
    for dev in (False, True):                                            # refused before any pointer is looked at: host arrays serve both
        o = Outputs(tdv, 4, True)
        assert stat_call(lib, dev, octx._h, pts, pts, 4, o, **BAD_STAT[case][1]) == TDV_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert o.untouched()


@pytest.mark.parametrize("case", range(1, len(BAD_RAD)))
def test_radius_bad_parameters_on_a_real_ctx(octx, tdv, case):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4, False)
        assert rad_call(lib, dev, octx._h, pts, pts, 4, o, **BAD_RAD[case][1]) == TDV_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert o.untouched()


def test_null_arrays_on_a_real_ctx_then_a_good_call(octx, tdv):
    lib = tdv.lib()
    pts = np.random.default_rng(1).random((40, 3)).astype(F)
    for fn, stat in ((stat_call, True), (rad_call, False)):
        for dev in (False, True):
            o = Outputs(tdv, 40, stat)
            assert fn(lib, dev, octx._h, None, None, 40, o) == TDV_ERR_BAD_ARG
            assert fn(lib, dev, octx._h, pts, None, -1, o) == TDV_ERR_BAD_ARG
            assert fn(lib, dev, octx._h, pts, None, 40, o, res=False) == TDV_ERR_BAD_ARG
            torch.cuda.synchronize()
            assert o.untouched()
    o = Outputs(tdv, 40, True)
    assert stat_call(lib, False, octx._h, pts, None, 40, o) == 0          # the ctx goes on working; no rgb: out_rgb stays as it was
    ref = R.statistical(pts, 3, 2.0)
    assert o.res.n_kept == ref["n_kept"] and o.mask.tobytes() == ref["mask"].tobytes() and o.per.tobytes() == ref["mean"].tobytes()
    assert o.cols.tobytes() == np.full((40, 3), -7, F).tobytes() and (o.index[ref["n_kept"]:] == -7).all()
