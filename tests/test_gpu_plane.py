"""Plane segmentation on the device (include/tdv_hip.h: tdv_segment_planes), against the restatement of tests/plane_restatement.py.

Labels, plane counts, winners, iterations run, inlier and candidate counts, the hypothesis' bits and the rest cloud read no sum: they
are the restatement's exactly, and so is fitness, one rounded quotient of two of those counts.  rmse agrees to 1e-6 relative, the refit normal to 1e-6 rad and its offset to 1e-7 m (the
f64 sum order and the eigen solver differ in the last places).  Every test runs on a Context of its own."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import icp_loss_restatement as IL
import plane_restatement as R
from test_plane_abi import BAD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32


@pytest.fixture
def pctx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


# ---------------------------------------------------------------- scenes
FLOOR_Z = 0.8


def tray_scene(synth, seed=3, noise=0.0005):
    """A bin seen from above (camera frame, z forward): floor z = 0.8 (0.5 x 0.36 m), four walls 0.15 m high rising towards the camera,
    four parts of synth.sample_object lying on the floor, 0.5 mm Gaussian noise.  Returns (points, list of the five true planes
    (unit n, d) with n . p + d = 0, the camera on the positive side)."""
    rng = np.random.default_rng(seed)
    hx, hy, hz = 0.25, 0.18, 0.15
    floor = np.c_[rng.uniform(-hx, hx, 20000), rng.uniform(-hy, hy, 20000), np.full(20000, FLOOR_Z)]
    long_w = [np.c_[np.full(6000, s * hx), rng.uniform(-hy, hy, 6000), rng.uniform(FLOOR_Z - hz, FLOOR_Z, 6000)] for s in (1, -1)]
    short_w = [np.c_[rng.uniform(-hx, hx, 4500), np.full(4500, s * hy), rng.uniform(FLOOR_Z - hz, FLOOR_Z, 4500)] for s in (1, -1)]
    parts = []
    for b, (x, y) in enumerate(((-0.1, -0.06), (0.08, -0.05), (-0.05, 0.07), (0.11, 0.08))):
        p, _ = synth.sample_object(1500, 100 + b)
        p = p.astype(np.float64)
        parts.append(p - p.mean(0) + [x, y, FLOOR_Z - 0.035])
    pts = np.concatenate([floor] + long_w + short_w + parts)
    pts = pts + rng.normal(0, noise, pts.shape)
    pts = pts[rng.permutation(len(pts))].astype(F)
    truth = [(np.array([0, 0, -1.0]), FLOOR_Z), (np.array([-1.0, 0, 0]), hx), (np.array([1.0, 0, 0]), hx),
             (np.array([0, -1.0, 0]), hy), (np.array([0, 1.0, 0]), hy)]
    return pts, truth


@pytest.fixture(scope="module")
def tray(synth):
    return tray_scene(synth)


def _same(got, labels, ref, rest=None):
    assert len(got) == ref["n_planes"], (len(got), ref["n_planes"])
    assert np.array_equal(labels, ref["labels"])
    for g, r in zip(got, ref["planes"]):
        for k in ("inliers", "candidates", "best_iteration", "iterations_run"):
            assert g[k] == r[k], (k, g[k], r[k])
        assert g["hypothesis"].tobytes() == r["hypothesis"].tobytes(), (g["hypothesis"], r["hypothesis"])
        assert F(g["fitness"]).tobytes() == F(r["fitness"]).tobytes(), (g["fitness"], r["fitness"])      # (float)((double)count / m_k) of exact counts
        assert abs(g["rmse"] - r["rmse"]) <= 1e-6 * r["rmse"], (g["rmse"], r["rmse"])
        if r["plane64"] is None:
            assert g["plane"].tobytes() == r["hypothesis"].tobytes()
        else:
            ref_n = r["plane64"][:3]
            ang = math.acos(min(1.0, float(np.dot(g["plane"][:3].astype(np.float64), ref_n) / np.linalg.norm(g["plane"][:3].astype(np.float64)))))
            assert ang <= 1e-6 and abs(float(g["plane"][3]) - r["plane64"][3]) <= 1e-7, (ang, g["plane"], r["plane64"])
    if rest is not None:
        assert rest.tobytes() == ref["rest"].tobytes()


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("params", [dict(max_planes=5, distance_threshold=0.003, num_iterations=2000),
                                    dict(max_planes=3, distance_threshold=0.003, num_iterations=3000, probability=1.0, seed=7),
                                    dict(max_planes=2, distance_threshold=0.01)])
def test_equals_the_restatement(pctx, tray, params):
    pts, _ = tray
    ref = R.segment_planes(pts, params)
    got, labels = pctx.segment_planes(pts, **params)
    _same(got, labels, ref)
    n = len(pts)
    (_, px), (lt, pl), (rt, pr) = _up(pts), _up(np.zeros(n, np.int32), np.int32), _up(np.zeros((n, 3), F))
    dgot, n_rest = pctx.segment_planes_dev(px, n, d_labels=pl, d_rest=pr, **params)
    torch.cuda.synchronize()
    assert n_rest == len(ref["rest"])
    _same(dgot, lt[:n].cpu().numpy(), ref, rt[:3 * n_rest].cpu().numpy().reshape(-1, 3))


# ---------------------------------------------------------------- 2. the tray
def test_tray_five_planes(pctx, tray):
    pts, truth = tray
    got, labels = pctx.segment_planes(pts, max_planes=5, distance_threshold=0.003, num_iterations=2000)
    assert len(got) == 5
    found = [False] * 5
    for g in got:
        n = g["plane"][:3].astype(np.float64)
        for i, (tn, td) in enumerate(truth):
            if float(np.dot(n, tn)) > math.cos(math.radians(1.0)):
                assert abs(float(g["plane"][3]) - td) < 2e-3, (g["plane"], tn, td)
                found[i] = True
    assert all(found), [g["plane"] for g in got]
    floor = got[0]["plane"]                                              # the largest first; its normal faces the camera
    assert float(floor[2]) < -math.cos(math.radians(1.0)) and floor[3] > 0
    assert (labels == 0).sum() >= 19000 and (labels == -1).sum() >= 5000      # the parts stay


# ---------------------------------------------------------------- 3. the switches
def test_min_inliers_probability_and_refit(pctx, tray):
    pts, _ = tray
    got, _ = pctx.segment_planes(pts, max_planes=5, distance_threshold=0.003, num_iterations=2000, min_inliers=5000)
    assert len(got) == 3 and all(g["inliers"] >= 5000 for g in got)         # the floor and the long walls; a short wall ends it
    ref = R.segment_planes(pts, dict(max_planes=5, distance_threshold=0.003, num_iterations=2000, min_inliers=5000))
    assert ref["n_planes"] == 3
    early, _ = pctx.segment_planes(pts, distance_threshold=0.003, num_iterations=5000)
    full, _ = pctx.segment_planes(pts, distance_threshold=0.003, num_iterations=5000, probability=1.0)
    assert early[0]["iterations_run"] == 1024 and full[0]["iterations_run"] == 5000
    raw, _ = pctx.segment_planes(pts, distance_threshold=0.003, refit=0)
    assert raw[0]["plane"].tobytes() == raw[0]["hypothesis"].tobytes()
    fit, _ = pctx.segment_planes(pts, distance_threshold=0.003)
    assert fit[0]["hypothesis"].tobytes() == raw[0]["hypothesis"].tobytes() and fit[0]["plane"].tobytes() != raw[0]["plane"].tobytes()


@pytest.mark.parametrize("case", range(1, len(BAD)))
def test_bad_parameters_on_a_real_ctx(pctx, tdv, case):
    _, kw = BAD[case]
    pts = np.zeros((4, 3), F)
    p = tdv.plane_params(**kw)
    out = (tdv.PlaneResultC * 16)(); C.memset(out, 0x5A, C.sizeof(out)); before = bytes(out)
    npl = C.c_int(-7)
    assert tdv.lib().tdv_segment_planes(pctx._h, pts.ctypes.data_as(C.c_void_p), 4, C.byref(p), out, C.byref(npl), None) == TDV_ERR_BAD_ARG
    assert bytes(out) == before and npl.value == -7


# ---------------------------------------------------------------- 4. edge cases
def test_tiny_and_non_finite_clouds(pctx, tray):
    for n in (0, 1, 2):
        pts = np.arange(3 * n, dtype=F).reshape(n, 3)
        got, labels = pctx.segment_planes(pts)
        assert got == [] and labels.tolist() == [-1] * n
        (_, px), (lt, pl), (rt, pr) = _up(pts), _up(np.full(max(n, 1), 5, np.int32), np.int32), _up(np.zeros((max(n, 1), 3), F))
        dgot, n_rest = pctx.segment_planes_dev(px if n else None, n, d_labels=pl, d_rest=pr, max_planes=3)
        torch.cuda.synchronize()
        assert dgot == [] and n_rest == n and lt[:n].cpu().tolist() == [-1] * n
        assert rt[:3 * n].cpu().numpy().tobytes() == pts.tobytes()
    pts, _ = tray
    bad = pts[:8000].copy()
    rng = np.random.default_rng(8)
    for v in (np.nan, np.inf, -np.inf):
        bad[rng.choice(len(bad), 300, replace=False), rng.integers(0, 3, 300)] = v
    params = dict(max_planes=3, distance_threshold=0.003, num_iterations=1500)
    ref = R.segment_planes(bad, params)
    got, labels = pctx.segment_planes(bad, **params)
    _same(got, labels, ref)
    nonfinite = ~np.isfinite(bad).all(1)
    assert nonfinite.sum() > 0 and (labels[nonfinite] == -1).all()


def test_host_equals_device_and_repeatable(pctx, tray):
    pts, _ = tray
    params = dict(max_planes=5, distance_threshold=0.003, num_iterations=2000)
    a, la = pctx.segment_planes(pts, **params)
    b, lb = pctx.segment_planes(pts, **params)
    n = len(pts)
    (_, px), (lt, pl) = _up(pts), _up(np.zeros(n, np.int32), np.int32)
    d, _ = pctx.segment_planes_dev(px, n, d_labels=pl, **params)
    torch.cuda.synchronize()
    assert la.tobytes() == lb.tobytes() == lt[:n].cpu().numpy().tobytes()
    for r in (b, d):
        assert len(r) == len(a)
        for x, y in zip(r, a):
            for k in x:
                assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def test_segment_plane_open3d_shape(pctx, tray):
    pts, _ = tray
    model, idx = pctx.segment_plane(pts, distance_threshold=0.003, ransac_n=3, num_iterations=1000)
    _, labels = pctx.segment_planes(pts, distance_threshold=0.003, num_iterations=1000)
    assert model.shape == (4,) and model.dtype == np.float32 and np.array_equal(idx, np.nonzero(labels == 0)[0])
    with pytest.raises(ValueError):
        pctx.segment_plane(pts, ransac_n=4)


# ---------------------------------------------------------------- 5. device-resident chain at frame size
W, H, FX, FY, CX, CY, SCALE, ZMAX, VOXEL = 1280, 720, 900.0, 900.0, 640.0, 360.0, 0.001, 2.0, 0.004


def _frame():
    """A depth frame (uint16 mm) of a floor tilted 20 degrees, 1 m from the camera, and the 6 cm high top of a box on it."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    rx, ry = (u - CX) / FX, (v - CY) / FY
    n = np.array([0.0, -math.sin(math.radians(20)), -math.cos(math.radians(20))])          # floor: n . p + 1 = 0
    z = 1.0 / -(n[0] * rx + n[1] * ry + n[2])
    box = (np.abs(u - 560) < 120) & (np.abs(v - 400) < 80)
    z = np.where(box, z - 0.06, z)
    return np.round(z / SCALE).astype(np.uint16)


def test_device_chain_at_frame_size(pctx, orc):
    raw = _frame()
    cloud = orc.unproject(orc.depth_preprocess(raw, None, 1.0 / SCALE), None, FX, FY, CX, CY, ZMAX)[0]
    n_ref = len(cloud)
    assert n_ref > 900000
    d_raw = torch.from_numpy(raw.reshape(-1).view(np.int16).copy()).to(DEV)
    d_xyz = torch.zeros(W * H * 3, dtype=torch.float32, device=DEV)
    n = pctx.depth_to_cloud_dev(d_raw.data_ptr(), None, None, W, H, 1.0 / SCALE, FX, FY, CX, CY, ZMAX, d_xyz.data_ptr(), None, W * H)
    assert n == n_ref
    d_lab = torch.zeros(n, dtype=torch.int32, device=DEV)
    d_rest = torch.zeros(n * 3, dtype=torch.float32, device=DEV)
    params = dict(max_planes=1, distance_threshold=0.005, num_iterations=100)
    got, n_rest = pctx.segment_planes_dev(d_xyz.data_ptr(), n, d_labels=d_lab.data_ptr(), d_rest=d_rest.data_ptr(), **params)
    d_vox = torch.zeros(max(n_rest, 1) * 3 + 3, dtype=torch.float32, device=DEV)
    m = pctx.voxel_downsample_dev(d_rest.data_ptr(), None, n_rest, VOXEL, d_vox.data_ptr(), None, max(n_rest, 1), order=1)
    torch.cuda.synchronize()
    assert d_xyz[:3 * n].cpu().numpy().tobytes() == cloud.tobytes()
    ref = R.segment_planes(cloud, params)
    _same(got, d_lab.cpu().numpy(), ref, d_rest[:3 * n_rest].cpu().numpy().reshape(-1, 3))
    assert got[0]["inliers"] > 0.8 * n and n_rest > 30000                  # the box top stays
    vox, _, _ = orc.voxel_downsample(ref["rest"], None, VOXEL)
    assert m == len(vox) and d_vox[:3 * m].cpu().numpy().tobytes() == vox.tobytes()


# ---------------------------------------------------------------- 6. what it buys
def test_floor_off_then_icp_on_the_clutter_scene(pctx, synth):
    """The robust-loss clutter scene (a bin floor 4 mm under the part): point-to-plane L2 ICP on the whole scan ends 1.9 mm / 1.6 mrad
    from the ground truth (as DESIGN.md 7 reports); with the floor taken off first (one plane at 2 mm) it ends 0.78 mm / 0.97 mrad
    away (the oracle's ICP on the restatement's rest, measured on the CPU)."""
    src, tgt, nrm, T0, T_gt = IL.clutter_scene(synth)
    S = IL.SCENE
    got, labels = pctx.segment_planes(src, distance_threshold=0.002)
    assert len(got) == 1 and got[0]["inliers"] >= S["n_floor"]
    rest = src[labels == -1]
    whole = pctx.icp(src, tgt, nrm, T0, S["thr"], S["iterations"], True)
    strip = pctx.icp(rest, tgt, nrm, T0, S["thr"], S["iterations"], True)
    e_w, e_s = synth.pose_error(whole.transformation, T_gt), synth.pose_error(strip.transformation, T_gt)
    print("L2 whole scan %.3e rad %.3e m; floor off %.3e rad %.3e m" % (*e_w, *e_s))
    assert e_w[1] > 1.5e-3
    assert e_s[1] < 1.0e-3 and e_s[1] < 0.6 * e_w[1] and e_s[0] < e_w[0]
