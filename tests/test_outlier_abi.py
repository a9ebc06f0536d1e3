"""CPU suite: outlier removal (include/tdv_hip.h: tdv_remove_statistical_outlier, tdv_remove_radius_outlier).  The ABI exports the entry
points, lists them in ABI_SYMBOLS and refuses every bad argument before it writes anything; the restatement
(tests/outlier_restatement.py) follows the header's rules on hand-made cases, its tree and brute-force variants agree byte for byte, the
radius mask is cluster_restatement's core flag, and on the bin scene with the floor off the statistical filter takes out the strays and
leaves the parts.  No compute entry point of the library runs here; tests/test_gpu_outlier.py holds the device to this restatement."""
import ctypes as C

import numpy as np
import pytest

import cluster_restatement as CR
import outlier_restatement as R
from test_cluster_abi import rest_of_scene

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_remove_statistical_outlier", "tdv_remove_statistical_outlier_dev", "tdv_remove_radius_outlier", "tdv_remove_radius_outlier_dev")
SCENE_PARAMS = [(20, 2.0), (20, 1.0), (10, 2.0), (30, 3.0)]


def test_symbols_and_struct(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.OutlierResultC) == 32
    assert [k for k, _ in tdv.OutlierResultC._fields_] == ["n_valid", "n_kept", "cloud_mean", "std_dev", "threshold"]
    assert tdv.OutlierResultC.cloud_mean.offset == 8 and tdv.OutlierResultC.threshold.offset == 24


GOOD_STAT = dict(nb_neighbors=3, std_ratio=2.0)
BAD_STAT = [("null ctx", {}), ("nb 0", dict(nb_neighbors=0)), ("nb < 0", dict(nb_neighbors=-4)), ("nb 256", dict(nb_neighbors=256)),
            ("ratio nan", dict(std_ratio=float("nan"))), ("ratio inf", dict(std_ratio=float("inf"))), ("ratio -inf", dict(std_ratio=float("-inf")))]
GOOD_RAD = dict(nb_points=2, radius=0.5)
BAD_RAD = [("null ctx", {}), ("nb < 0", dict(nb_points=-1)), ("radius 0", dict(radius=0.0)), ("radius < 0", dict(radius=-0.5)),
           ("radius nan", dict(radius=float("nan"))), ("radius inf", dict(radius=float("inf")))]


class Outputs:
    """Every output of a call on n points, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n, statistical, fill=0x5A):
        self.res = tdv.OutlierResultC(); C.memset(C.byref(self.res), fill, C.sizeof(self.res))
        self.mask = np.full(n, 7, np.uint8)
        self.per = np.full(n, -7, np.float64 if statistical else np.int32)
        self.index = np.full(n, -7, np.int32); self.rows = np.full((n, 3), -7, F); self.cols = np.full((n, 3), -7, F)
        self.before = self.snapshot()

    def snapshot(self):
        return bytes(self.res), self.mask.tobytes(), self.per.tobytes(), self.index.tobytes(), self.rows.tobytes(), self.cols.tobytes()

    def untouched(self):
        return self.snapshot() == self.before


def call(fn, ctx, pts, rgb, n, a, b, o, res=True):
    """Host arrays in every slot: a refused call must not look at them (the device entry points included)."""
    P = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    return fn(ctx, P(pts), P(rgb), n, a, b, C.byref(o.res) if res else None, P(o.mask), P(o.per), P(o.index), P(o.rows), P(o.cols))


def stat_call(lib, dev, ctx, pts, rgb, n, o, res=True, **kw):
    p = dict(GOOD_STAT, **kw)
    fn = lib.tdv_remove_statistical_outlier_dev if dev else lib.tdv_remove_statistical_outlier
    return call(fn, ctx, pts, rgb, n, p["nb_neighbors"], C.c_double(p["std_ratio"]), o, res)


def rad_call(lib, dev, ctx, pts, rgb, n, o, res=True, **kw):
    p = dict(GOOD_RAD, **kw)
    fn = lib.tdv_remove_radius_outlier_dev if dev else lib.tdv_remove_radius_outlier
    return call(fn, ctx, pts, rgb, n, p["nb_points"], C.c_float(p["radius"]), o, res)


@pytest.mark.parametrize("case", range(len(BAD_STAT)))
def test_statistical_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad parameter: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_outlier.py refuses each bad parameter on one."""
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); rgb = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4, True)
        assert stat_call(lib, dev, None, pts, rgb, 4, o, **BAD_STAT[case][1]) == TDV_ERR_BAD_ARG
        assert o.untouched()


@pytest.mark.parametrize("case", range(len(BAD_RAD)))
def test_radius_bad_arguments_leave_outputs_untouched(tdv, case):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); rgb = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4, False)
        assert rad_call(lib, dev, None, pts, rgb, 4, o, **BAD_RAD[case][1]) == TDV_ERR_BAD_ARG
        assert o.untouched()


def test_null_arrays_and_result(tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F)
    for fn, stat in ((stat_call, True), (rad_call, False)):
        for dev in (False, True):
            o = Outputs(tdv, 4, stat, 0x33)
            assert fn(lib, dev, None, None, None, 4, o) == TDV_ERR_BAD_ARG
            assert fn(lib, dev, None, pts, None, -1, o) == TDV_ERR_BAD_ARG
            assert fn(lib, dev, None, pts, None, 4, o, res=False) == TDV_ERR_BAD_ARG
            assert o.untouched()


# ---------------------------------------------------------------- restatement: hand-made cases
def same(a, b):
    for k in ("n_valid", "n_kept"):
        assert a[k] == b[k], k
    for k in ("cloud_mean", "std_dev", "threshold"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])
    for k in ("mask", "mean", "count", "index", "xyz", "rgb"):
        if a.get(k) is not None:
            assert a[k].tobytes() == b[k].tobytes(), k


def both_stat(pts, k, ratio, rgb=None):
    a = R.statistical(pts, k, ratio, rgb)
    same(a, R.statistical_brute(pts, k, ratio, rgb))
    return a


def both_rad(pts, nb, r, rgb=None):
    a = R.radius(pts, nb, r, rgb)
    same(a, R.radius_brute(pts, nb, r, rgb))
    return a


def test_single_point_and_fewer_points_than_neighbours():
    r = both_stat(np.array([[1, 2, 3]], F), 5, 2.0)
    assert (r["n_valid"], r["n_kept"]) == (0, 0) and r["mean"].tolist() == [0.0]       # its own list: itself at 0, not > 0
    assert np.isnan([r["cloud_mean"], r["std_dev"], r["threshold"]]).all()
    pts = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], F)                                # n < nb_neighbors: the lists are all n rows
    r = both_stat(pts, 20, 2.0)
    assert r["mean"].tolist() == [7 / 3, 8 / 3, 9 / 3] and r["n_valid"] == 3
    assert r["cloud_mean"] == np.float64(8) / np.float64(3) and r["n_kept"] == 3
    assert both_stat(np.zeros((0, 3), F), 4, 1.0)["n_valid"] == 0


def test_one_neighbour_is_the_point_itself():
    rng = np.random.default_rng(1)
    r = both_stat(rng.random((40, 3)).astype(F), 1, 2.0)
    assert (r["mean"] == 0).all() and r["n_valid"] == 0 and r["n_kept"] == 0 and np.isnan(r["threshold"])


def test_exactly_one_valid_point():
    pts = np.zeros((7, 3), F); pts[6] = [1, 0, 0]             # six duplicates: their 3 nearest are copies at 0
    r = both_stat(pts, 3, 2.0)
    assert r["valid"].tolist() == [False] * 6 + [True] and r["n_valid"] == 1
    assert r["cloud_mean"] == 2 / 3 and np.isnan(r["std_dev"]) and np.isnan(r["threshold"]) and r["n_kept"] == 0


def test_point_with_nb_neighbors_duplicates_is_invalid_and_removed():
    rng = np.random.default_rng(2)
    pts = rng.random((60, 3)).astype(F)
    pts[10:14] = pts[10]                                       # four copies: with k = 4 each finds only copies
    r = both_stat(pts, 4, 3.0)
    assert not r["valid"][10:14].any() and r["valid"].sum() == 56 and not r["mask"][10:14].any()
    assert both_stat(pts, 5, 3.0)["valid"].all()               # the fifth neighbour is another point


def test_nan_and_infinite_rows():
    rng = np.random.default_rng(3)
    pts = rng.random((50, 3)).astype(F)
    pts[5] = np.nan; pts[6, 1] = np.nan; pts[7] = np.inf; pts[8, 2] = -np.inf
    r = both_stat(pts, 6, 2.0)
    assert np.isnan(r["mean"][[5, 6]]).all() and np.isinf(r["mean"][[7, 8]]).all()      # no list; a list of +inf distances
    assert not r["valid"][5:9].any() and r["n_valid"] == 46 and not r["mask"][5:9].any()
    assert np.isfinite(r["threshold"]) and r["n_kept"] > 30
    r = both_stat(pts, 48, 2.0)                                 # lists longer than the finite rows: every mean is +inf or NaN
    assert r["n_valid"] == 0 and r["n_kept"] == 0
    q = both_rad(pts, 1, 0.3)
    assert q["count"][5:9].tolist() == [0] * 4 and q["n_valid"] == 46 and not q["mask"][5:9].any()


def test_negative_std_ratio():
    rng = np.random.default_rng(4)
    pts = rng.random((300, 3)).astype(F)
    r = both_stat(pts, 8, -0.5)
    assert r["threshold"] < r["cloud_mean"] and 0 < r["n_kept"] < 150
    assert np.array_equal(r["mask"] == 1, r["mean"] < r["threshold"])
    assert r["xyz"].tobytes() == pts[r["index"]].tobytes() and (np.diff(r["index"]) > 0).all()


def test_points_exactly_radius_apart():
    """Multiples of 2^-6 are exact in f32, and so are their squares: d2 == eps2, and <= counts the pair."""
    eps = 0.015625
    pts = np.zeros((9, 3), F); pts[:, 0] = np.arange(9) * eps
    rgb = np.arange(27, dtype=F).reshape(9, 3)
    r = both_rad(pts, 2, eps, rgb)
    assert r["mask"].tolist() == [0] + [1] * 7 + [0] and r["count"].tolist() == [2] + [3] * 7 + [2]
    assert r["index"].tolist() == list(range(1, 8)) and r["rgb"].tobytes() == rgb[1:8].tobytes()
    r = both_rad(pts, 2, np.nextafter(F(eps), F(0)))
    assert r["n_kept"] == 0 and r["count"].tolist() == [1] * 9
    assert both_rad(pts, 0, eps)["count"].tolist() == [1] * 9      # saturated at nb_points + 1


def test_variants_agree_on_random_clouds():
    rng = np.random.default_rng(5)
    for n, k, ratio in ((2, 2, 1.0), (64, 2, 2.0), (300, 20, 1.0), (700, 64, 2.0), (700, 65, -1.0), (500, 255, 0.5)):
        pts = rng.random((n, 3)).astype(F)
        if n > 100:
            pts[rng.integers(0, n, 5)] = np.nan
            pts[rng.integers(0, n, 5), 1] = -np.inf
            pts[rng.integers(0, n, 3), 0] = 1e19
            pts[40:44] = pts[40]
        both_stat(pts, k, ratio, rng.random((n, 3)).astype(F))
        both_rad(pts, k // 4, 0.08)
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.25)   # exact pitch: ties everywhere
    both_stat(g, 7, 1.0); both_stat(g, 20, 1.0)
    assert both_rad(g, 6, 0.25)["n_kept"] == 5 ** 3


def test_radius_mask_is_the_core_flag_of_clustering():
    rng = np.random.default_rng(6)
    pts = rng.random((2000, 3)).astype(F)
    pts[rng.integers(0, 2000, 9), 2] = np.inf
    for nb, r in ((3, 0.05), (0, 0.01), (12, 0.09)):
        got = R.radius(pts, nb, r)
        core = CR.cluster(pts, r, nb + 1)["core"]
        assert np.array_equal(got["mask"] == 1, core)
        assert CR.cluster_brute(pts[:500], r, nb + 1)["core"].tobytes() == (R.radius_brute(pts[:500], nb, r)["mask"] == 1).tobytes()


# ---------------------------------------------------------------- restatement: the scene
def test_scene_strays_go_parts_stay_and_the_gap_holds(synth):
    """The cluster scene with the floor off: at (20, 2.0) the statistical filter removes all 60 strays, at most 5 other points and no
    part point, the six parts still cluster at every R.PARAMS, and no mean lies within the statistics' bound of the threshold."""
    rest, part = rest_of_scene(synth)
    for k, ratio in SCENE_PARAMS:
        r = R.statistical(rest, k, ratio)
        assert R.gap_ok(r, len(rest), ratio), (k, ratio)
        assert R.statistics_bounds(r, len(rest), ratio)[2] < 1e-12 * r["threshold"]
        print(k, ratio, r["n_valid"], r["n_kept"], r["threshold"], np.abs(r["mean"][r["valid"]] - r["threshold"]).min() / r["threshold"])
    r = R.statistical(rest, 20, 2.0)
    gone = r["mask"] == 0
    assert gone[part == -2].all() and (part == -2).sum() == CR.SCENE["n_stray"]
    assert not gone[part >= 0].any() and gone.sum() - CR.SCENE["n_stray"] <= 5
    for eps, mp in CR.PARAMS:
        c = CR.cluster(r["xyz"], eps, mp, 20)
        assert c["result"]["n_clusters"] == 6, (eps, mp, c["result"])
