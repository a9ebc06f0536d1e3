"""CPU suite: plane segmentation (include/tdv_hip.h: tdv_segment_planes).  The ABI exports the entry points, lists them in ABI_SYMBOLS,
gives Open3D's defaults and refuses every bad argument before it writes anything; the restatement (tests/plane_restatement.py) follows
the header's plane, orientation, validity and stop rules on hand-made cases, and on the clutter scene of tests/icp_loss_restatement.py
it takes the bin floor off the scan and leaves the part.  No compute entry point of the library runs here; tests/test_gpu_plane.py
holds the device to this restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_loss_restatement as IL
import plane_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_plane_default_params", "tdv_segment_planes", "tdv_segment_planes_dev")


def test_symbols_defaults_and_sizes(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    p = tdv.plane_params()
    assert p.probability == 0.99999999 and p.distance_threshold == F(0.01)
    assert (p.num_iterations, p.max_planes, p.min_inliers, p.refit, p.seed) == (100, 1, 3, 1, 42)
    assert C.sizeof(tdv.PlaneParamsC) == 32 and C.sizeof(tdv.PlaneResultC) == 56
    assert (tdv.TDV_PLANE_CHUNK, tdv.TDV_PLANE_MAX) == (R.CHUNK, R.PLANE_MAX) == (1024, 16)
    assert R.DEFAULTS == dict(probability=0.99999999, distance_threshold=0.01, num_iterations=100, max_planes=1, min_inliers=3, refit=1,
                              seed=42)
    with pytest.raises(TypeError):
        tdv.plane_params(no_such_option=1)


BAD = [("null ctx", {}), ("threshold 0", dict(distance_threshold=0.0)), ("threshold < 0", dict(distance_threshold=-0.01)),
       ("threshold nan", dict(distance_threshold=float("nan"))), ("threshold inf", dict(distance_threshold=float("inf"))),
       ("probability 0", dict(probability=0.0)), ("probability > 1", dict(probability=1.0000001)),
       ("probability nan", dict(probability=float("nan"))), ("probability < 0", dict(probability=-0.5)),
       ("num_iterations 0", dict(num_iterations=0)), ("max_planes 0", dict(max_planes=0)), ("max_planes 17", dict(max_planes=17)),
       ("min_inliers 2", dict(min_inliers=2))]


def _call(tdv, fn, ctx, pts, n, p, out, npl, dev):
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if dev:
        return fn(ctx, P(pts), n, p, out, npl, None, None, None)
    return fn(ctx, P(pts), n, p, out, npl, None)


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_out_untouched(tdv, case):
    """A NULL ctx, alone and with each bad parameter: TDV_ERR_BAD_ARG, out and n_planes byte for byte as they were.  A real ctx needs a
    device: tests/test_gpu_plane.py refuses each bad parameter on one."""
    lib = tdv.lib()
    _, kw = BAD[case]
    pts = np.zeros((4, 3), F)
    p = tdv.plane_params(**kw)
    for fn, dev in ((lib.tdv_segment_planes, False), (lib.tdv_segment_planes_dev, True)):
        out = (tdv.PlaneResultC * 16)(); C.memset(out, 0x5A, C.sizeof(out)); before = bytes(out)
        npl = C.c_int(-7)
        assert _call(tdv, fn, None, pts, 4, C.byref(p), out, C.byref(npl), dev) == TDV_ERR_BAD_ARG
        assert bytes(out) == before and npl.value == -7


def test_null_arrays_and_params(tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); p = tdv.plane_params()
    out = (tdv.PlaneResultC * 16)(); C.memset(out, 0x33, C.sizeof(out)); before = bytes(out)
    npl = C.c_int(-7)
    for fn, dev in ((lib.tdv_segment_planes, False), (lib.tdv_segment_planes_dev, True)):
        assert _call(tdv, fn, None, None, 4, C.byref(p), out, C.byref(npl), dev) == TDV_ERR_BAD_ARG
        assert _call(tdv, fn, None, pts, -1, C.byref(p), out, C.byref(npl), dev) == TDV_ERR_BAD_ARG
        assert _call(tdv, fn, None, pts, 4, None, out, C.byref(npl), dev) == TDV_ERR_BAD_ARG
        assert _call(tdv, fn, None, pts, 4, C.byref(p), None, C.byref(npl), dev) == TDV_ERR_BAD_ARG
        assert _call(tdv, fn, None, pts, 4, C.byref(p), out, None, dev) == TDV_ERR_BAD_ARG
    assert bytes(out) == before and npl.value == -7


# ---------------------------------------------------------------- restatement
def test_draw_uses_its_own_stream():
    """Key (seed, 1): not FGR's (seed, 0) stream; the round enters the counter; indices stay below m."""
    import fgr_restatement as FR
    t = np.arange(5000)
    d = R.draw(t, 0, 1000, 42)
    assert d.shape == (3, 5000) and d.min() >= 0 and d.max() < 1000
    assert not np.array_equal(d, FR.trial_indices(t, 1000, 42).astype(np.int64))
    assert not np.array_equal(d, R.draw(t, 1, 1000, 42)) and not np.array_equal(d, R.draw(t, 0, 1000, 7))
    x = FR.philox4x32((np.uint64(17), np.uint64(2), 0, 0), (42, 1))
    assert [int(v) for v in R.draw([17], 2, 1 << 20, 42)[:, 0]] == [int(w[0]) * (1 << 20) >> 32 for w in x[:3]]


def test_plane_and_orientation_of_hand_made_triples():
    # a floor 1 m in front of the camera: counter-clockwise seen from the camera gives the normal +z, d = -1; reported flipped
    cand = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], F)
    pl, ok = R.planes(cand, np.array([[0], [1], [2]]))
    assert ok[0] and np.array_equal(pl[0], [0.0, 0.0, 1.0, -1.0])
    res = R.segment_planes(np.concatenate([cand, [[0.5, 0.5, 1.0]]]), dict(num_iterations=50))
    assert res["n_planes"] == 1 and np.array_equal(res["planes"][0]["hypothesis"], F([-0.0, -0.0, -1.0, 1.0]))
    assert (res["labels"] == 0).all() and len(res["rest"]) == 0
    # the plane's offset is the camera-side distance; the refit turns with the hypothesis
    assert res["planes"][0]["plane"][3] == F(1.0) and res["planes"][0]["plane"][2] == F(-1.0)
    # the order of the three points decides the sign of n only, and the f64 arithmetic is the header's
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(3, 3)).astype(F)
    a, _ = R.planes(pts, np.array([[0], [1], [2]]))
    b, _ = R.planes(pts, np.array([[0], [2], [1]]))
    assert np.allclose(a[0], -b[0], rtol=0, atol=1e-12)
    P = pts.astype(np.float64); u = P[1] - P[0]; v = P[2] - P[0]
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    r = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    abc = n / r
    assert a[0].tobytes() == np.array([*abc, -((abc[0] * P[0, 0] + abc[1] * P[0, 1]) + abc[2] * P[0, 2])]).tobytes()


def test_invalid_hypotheses():
    cand = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [2, 0, 1], [np.nan, 0, 1], [np.inf, 0, 1]], F)
    idx = np.array([[0, 0, 0, 0, 0, 1], [0, 1, 1, 1, 1, 2], [1, 0, 3, 4, 5, 5]])     # repeated, repeated, collinear, NaN, inf, inf
    pl, ok = R.planes(cand, idx)
    assert not ok.any() and np.isnan(pl[:, 3]).all()
    assert (R.counts(cand, pl, 1.0) == 0).all()                         # an invalid hypothesis scores nothing
    good, ok = R.planes(cand, np.array([[0], [1], [2]]))
    assert ok[0] and R.counts(cand, good, 0.01)[0] == 4                 # the NaN and inf points are never inliers


def test_early_stop_rule():
    assert not R.stops(0, 1000, 1024, 0.99)                             # nothing found yet
    assert R.stops(1000, 1000, 1024, 0.99)                               # f = 1
    assert not R.stops(1000, 1000, 1024, 1.0)                            # probability 1 never stops
    assert not R.stops(500, 1000, 1 << 30, 1.0)
    # f = 0.5: log(1 - 0.99999999) / log(1 - 0.125) = 137.9..., so one chunk is enough; f = 0.1 needs 18,411 hypotheses
    bound = math.log(1 - 0.99999999) / math.log(1 - 0.125)
    assert 137 < bound < 138 and R.stops(500, 1000, 1024, 0.99999999)
    assert not R.stops(100, 1000, 17 * 1024, 0.99999999) and R.stops(100, 1000, 18 * 1024, 0.99999999)
    assert not R.stops(3, 10 ** 6, 1 << 30, 0.99999999)                # f^3 below half an ulp of 1: no bound
    # a whole search: chunks stop early with probability < 1, never with 1
    rng = np.random.default_rng(4)
    floor = np.c_[rng.uniform(-1, 1, (300, 2)), np.zeros(300)]
    noise = rng.uniform(-1, 1, (700, 3))
    cloud = np.concatenate([floor, noise]).astype(F)
    a = R.search(cloud, 0, dict(R.DEFAULTS, num_iterations=20000, distance_threshold=0.005))
    b = R.search(cloud, 0, dict(R.DEFAULTS, num_iterations=20000, distance_threshold=0.005, probability=1.0))
    assert a["run"] % 1024 == 0 and a["run"] < 20000 and b["run"] == 20000
    assert b["best_count"] >= a["best_count"] >= 300


def test_rounds_and_acceptance():
    rng = np.random.default_rng(5)
    floor = np.c_[rng.uniform(-1, 1, (400, 2)), np.zeros(400)]
    wall = np.c_[np.full(200, 1.0), rng.uniform(-1, 1, (200, 2))]
    noise = rng.uniform(-0.9, 0.9, (100, 3))
    cloud = np.concatenate([floor, wall, noise]).astype(F)
    r = R.segment_planes(cloud, dict(num_iterations=500, max_planes=4, distance_threshold=0.003, min_inliers=50))
    assert r["n_planes"] == 2                                           # a third round finds fewer than 50 inliers: rejected
    assert (r["labels"][:400] == 0).all() and (r["labels"][400:600] == 1).all()
    assert r["planes"][0]["candidates"] == 700 and r["planes"][1]["candidates"] == 700 - r["planes"][0]["inliers"]
    assert len(r["rest"]) == (r["labels"] == -1).sum() and np.array_equal(r["rest"], cloud[r["labels"] == -1])
    one = R.segment_planes(cloud, dict(num_iterations=500, max_planes=1, distance_threshold=0.003))
    assert np.array_equal(one["labels"] == 0, r["labels"] == 0)       # round 0 does not depend on max_planes
    assert R.segment_planes(cloud[:2])["n_planes"] == 0


def test_clutter_scene_floor_comes_off(synth):
    """On the robust-loss clutter scene (a bin floor 4 mm under the part), one plane at 2 mm takes the floor and almost none of the
    part's scan."""
    src, _, _, _, T_gt = IL.clutter_scene(synth)
    T = np.asarray(T_gt, np.float64)
    z = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3])[:, 2]          # the floor lies at z = -0.034 in the part's frame
    is_floor = np.abs(z + 0.034) < 1e-5
    assert is_floor.sum() == IL.SCENE["n_floor"]
    r = R.segment_planes(src, dict(distance_threshold=0.002))
    assert r["n_planes"] == 1
    lab = r["labels"] == 0
    assert lab[is_floor].mean() > 0.999
    assert lab[~is_floor].mean() < 0.01, lab[~is_floor].mean()
