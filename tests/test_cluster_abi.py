"""CPU suite: Euclidean clustering (include/tdv_hip.h: tdv_cluster_dbscan).  The ABI exports the entry points, lists them in ABI_SYMBOLS,
gives the defaults and refuses every bad argument before it writes anything; the restatement (tests/cluster_restatement.py) follows the
header's rules on hand-made cases, its tree variant and its brute-force variant agree, and on a bin scene with the floor taken off
(tests/plane_restatement.py) it finds the six parts.  No compute entry point of the library runs here; tests/test_gpu_cluster.py holds
the device to this restatement."""
import ctypes as C

import numpy as np
import pytest

import cluster_restatement as R
import plane_restatement as PR

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_cluster_default_params", "tdv_cluster_dbscan", "tdv_cluster_dbscan_dev")


def test_symbols_defaults_and_sizes(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    p = tdv.cluster_params()
    assert (p.eps, p.min_points, p.min_cluster_size) == (0.0, 0, 1)          # eps and min_points are the caller's, as in Open3D
    p = tdv.cluster_params(eps=0.01, min_points=10)
    assert p.eps == F(0.01) and p.min_points == 10 and p.min_cluster_size == 1
    assert C.sizeof(tdv.ClusterParamsC) == 12 and C.sizeof(tdv.ClusterResultC) == 24
    assert [k for k, _ in tdv.ClusterResultC._fields_] == ["n_clusters", "n_core", "n_border", "n_noise", "n_dropped", "largest"]
    with pytest.raises(TypeError):
        tdv.cluster_params(no_such_option=1)


GOOD = dict(eps=0.01, min_points=3)
BAD = [("null ctx", {}), ("eps 0", dict(eps=0.0)), ("eps < 0", dict(eps=-0.01)), ("eps nan", dict(eps=float("nan"))),
       ("eps inf", dict(eps=float("inf"))), ("min_points 0", dict(min_points=0)), ("min_points < 0", dict(min_points=-3)),
       ("min_cluster_size 0", dict(min_cluster_size=0)), ("min_cluster_size < 0", dict(min_cluster_size=-1))]


class Outputs:
    """Every output of a call on n points, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n, fill=0x5A):
        self.res = tdv.ClusterResultC(); C.memset(C.byref(self.res), fill, C.sizeof(self.res))
        self.nl = C.c_int(-7)
        self.labels = np.full(n, -7, np.int32); self.order = np.full(n, -7, np.int32)
        self.rows = np.full((n, 3), -7, F); self.offsets = np.full(n + 1, -7, np.int32)
        self.before = self.snapshot()

    def snapshot(self):
        return bytes(self.res), self.nl.value, self.labels.tobytes(), self.order.tobytes(), self.rows.tobytes(), self.offsets.tobytes()

    def untouched(self):
        return self.snapshot() == self.before


def call(fn, ctx, pts, n, p, o, res=True, offsets=True, cap=None):
    """Host arrays in every slot: a refused call must not look at them (the device entry point included)."""
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return fn(ctx, P(pts), n, p, C.byref(o.res) if res else None, P(o.labels), P(o.order), P(o.rows), P(o.offsets) if offsets else None,
              (len(o.offsets) - 1) if cap is None else cap, C.byref(o.nl))


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad parameter: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_cluster.py refuses each bad parameter on one."""
    lib = tdv.lib()
    pts = np.zeros((4, 3), F)
    p = tdv.cluster_params(**dict(GOOD, **BAD[case][1]))
    for fn in (lib.tdv_cluster_dbscan, lib.tdv_cluster_dbscan_dev):
        o = Outputs(tdv, 4)
        assert call(fn, None, pts, 4, C.byref(p), o) == TDV_ERR_BAD_ARG
        assert o.untouched()


def test_null_arrays_and_params(tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); p = tdv.cluster_params(**GOOD)
    for fn in (lib.tdv_cluster_dbscan, lib.tdv_cluster_dbscan_dev):
        o = Outputs(tdv, 4, 0x33)
        assert call(fn, None, None, 4, C.byref(p), o) == TDV_ERR_BAD_ARG
        assert call(fn, None, pts, -1, C.byref(p), o) == TDV_ERR_BAD_ARG
        assert call(fn, None, pts, 4, None, o) == TDV_ERR_BAD_ARG
        assert call(fn, None, pts, 4, C.byref(p), o, res=False) == TDV_ERR_BAD_ARG
        assert call(fn, None, pts, 4, C.byref(p), o, cap=-1) == TDV_ERR_BAD_ARG
        assert call(fn, None, pts, 4, C.byref(p), o, offsets=False, cap=2) == TDV_ERR_BAD_ARG
        assert o.untouched()


# ---------------------------------------------------------------- restatement: hand-made cases
def both(pts, eps, min_points, min_cluster_size=1):
    """The tree variant's result, after checking that the brute-force variant gives the same bytes."""
    a = R.cluster(pts, eps, min_points, min_cluster_size)
    b = R.cluster_brute(pts, eps, min_points, min_cluster_size)
    assert a["result"] == b["result"]
    for k in ("labels", "order", "offsets", "grouped", "core", "border"):
        assert a[k].tobytes() == b[k].tobytes(), k
    return a


def test_points_exactly_eps_apart_chain():
    """Multiples of 2^-6 are exact in f32, and so are their squares: d2 == eps2, and <= keeps the pair (a strict test would not)."""
    eps = 0.015625
    pts = np.zeros((9, 3), F); pts[:, 0] = np.arange(9) * eps
    assert (R.d2_f32(pts[1:], pts[:-1]) == R.eps2_f32(eps)).all()
    r = both(pts, eps, 2)
    assert r["result"]["n_clusters"] == 1 and (r["labels"] == 0).all() and r["core"].all()
    r = both(pts, eps, 3)                                   # the ends have two neighbours: border points of the one cluster
    assert r["core"].tolist() == [False] + [True] * 7 + [False] and (r["labels"] == 0).all() and r["result"]["n_border"] == 2
    assert both(pts, np.nextafter(F(eps), F(0)), 2)["result"]["n_clusters"] == 0


def test_border_point_equidistant_from_two_clusters_joins_the_lower_index():
    """Two groups of four cores left and right of a point that is 1 from the nearest core of each (it has three neighbours, itself
    included: not core at min_points 4): the key (d2 bits, index) decides."""
    left = [[-1, 0, 0], [-1.5, 0, 0], [-1.5, 0.5, 0], [-1.5, -0.5, 0]]
    right = [[1, 0, 0], [1.5, 0, 0], [1.5, 0.5, 0], [1.5, -0.5, 0]]
    for first, second in ((left, right), (right, left)):
        pts = np.array(first + second + [[0, 0, 0]], F)     # rows 0-3: cluster 0, rows 4-7: cluster 1, row 8: the border point
        r = both(pts, 1.0, 4)
        assert r["core"].tolist() == [True] * 8 + [False] and r["border"][8]
        assert r["labels"].tolist() == [0] * 4 + [1] * 4 + [0]        # d2 ties at 1: core 0 against core 4
        assert r["result"]["n_clusters"] == 2                          # a border point joins, it does not connect
    pts = np.array(left + right + [[0.25, 0, 0]], F)        # nearer to the second cluster: distance beats index
    assert both(pts, 1.0, 4)["labels"].tolist() == [0] * 4 + [1] * 4 + [1]


def test_numbering_follows_the_lowest_core_index_not_the_size():
    rng = np.random.default_rng(1)
    small = rng.normal(0, 0.01, (5, 3)); big = rng.normal(0, 0.01, (40, 3)) + [10, 0, 0]
    pts = np.concatenate([small[:1], big, small[1:]]).astype(F)         # row 0 belongs to the small cluster
    r = both(pts, 0.1, 3)
    assert r["result"]["n_clusters"] == 2 and r["result"]["largest"] == 40
    assert r["labels"][0] == 0 and (r["labels"][1:41] == 1).all() and (r["labels"][41:] == 0).all()
    assert r["offsets"].tolist() == [0, 5, 45] and r["order"][:5].tolist() == [0, 41, 42, 43, 44]
    # a non-core row of low index does not open a cluster: row 0 is a lone point now
    pts = np.concatenate([[[50, 50, 50]], big, small]).astype(F)
    r = both(pts, 0.1, 3)
    assert r["labels"][0] == -1 and (r["labels"][1:41] == 0).all() and (r["labels"][41:] == 1).all()
    assert r["order"].tolist() == list(range(1, 46)) + [0]              # the noise goes last


def test_min_points_one_makes_every_finite_point_core():
    rng = np.random.default_rng(2)
    pts = rng.random((50, 3)).astype(F)
    pts[7] = np.nan; pts[20, 1] = np.inf
    r = both(pts, 1e-3, 1)
    finite = np.isfinite(pts).all(1)
    assert np.array_equal(r["core"], finite) and r["result"]["n_clusters"] == 48 and r["result"]["n_noise"] == 2
    assert np.array_equal(r["labels"][finite], np.arange(48))           # singletons in index order


def test_duplicates():
    base = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    pts = base[[0, 1, 0, 0, 2, 1, 0]]                                   # the first point four times, the second twice
    r = both(pts, 0.1, 2)
    assert r["labels"].tolist() == [0, 1, 0, 0, -1, 1, 0] and r["result"]["n_core"] == 6
    r = both(pts, 0.1, 4)
    assert r["labels"].tolist() == [0, -1, 0, 0, -1, -1, 0]


def test_nan_and_inf_rows_are_noise_and_bridge_nothing():
    a = np.array([[0, 0, 0], [0.5, 0, 0], [1, 0, 0]], F); b = a + F([3, 0, 0])
    for bad in ([np.nan, 0, 0], [2, np.nan, 0], [np.inf, 0, 0], [2, 0, -np.inf], [np.nan] * 3, [np.inf] * 3):
        pts = np.concatenate([a, [bad], b, [bad]]).astype(F)            # a finite row at (2, 0, 0) would join the two triples
        r = both(pts, 1.0, 2)
        assert r["labels"].tolist() == [0, 0, 0, -1, 1, 1, 1, -1], bad
        assert not r["core"][3] and not r["border"][3]
    assert both(np.concatenate([a, [[2, 0, 0]], b]).astype(F), 1.0, 2)["result"]["n_clusters"] == 1
    # two identical non-finite rows are not each other's neighbours either
    assert both(np.full((4, 3), np.inf, F), 1.0, 1)["result"] == dict(n_clusters=0, n_core=0, n_border=0, n_noise=4, n_dropped=0,
                                                                        largest=0, n_labelled=0)


def test_min_cluster_size_drops_and_renumbers():
    rng = np.random.default_rng(3)
    sizes = [30, 4, 25, 3, 12]
    pts = np.concatenate([rng.normal(0, 0.01, (m, 3)) + [5 * k, 0, 0] for k, m in enumerate(sizes)]).astype(F)
    r1 = both(pts, 0.1, 3)
    assert r1["result"]["n_clusters"] == 5 and np.diff(r1["offsets"]).tolist() == sizes
    r = both(pts, 0.1, 3, 10)
    assert r["result"] == dict(n_clusters=3, n_core=74, n_border=0, n_noise=7, n_dropped=2, largest=30, n_labelled=67)
    assert np.diff(r["offsets"]).tolist() == [30, 25, 12]
    assert np.array_equal(r["labels"], np.repeat([0, -1, 1, -1, 2], sizes))
    assert r["order"][-7:].tolist() == [30, 31, 32, 33, 59, 60, 61] and r["grouped"].tobytes() == pts[r["order"]].tobytes()
    assert both(pts, 0.1, 3, 31)["result"]["n_clusters"] == 0


def test_variants_agree_on_random_clouds():
    rng = np.random.default_rng(4)
    for n, eps, mp, mcs in ((0, 0.1, 3, 1), (1, 0.1, 1, 1), (2, 0.1, 2, 1), (300, 0.08, 4, 1), (700, 0.05, 3, 4), (1000, 0.1, 8, 1),
                            (1000, 0.02, 2, 2)):
        pts = rng.random((n, 3)).astype(F)
        if n > 100:
            pts[rng.integers(0, n, 5)] = np.nan
            pts[rng.integers(0, n, 5), 1] = -np.inf
        both(pts, eps, mp, mcs)
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.25)   # exact pitch: d2 == eps2
    r = both(g, 0.25, 7)
    assert r["result"]["n_clusters"] == 1 and r["result"]["n_core"] == 6 ** 3 and r["result"]["n_noise"] == 80     # the edges and corners have no core neighbour
    assert both(g, 0.2499, 2)["result"]["n_clusters"] == 0


# ---------------------------------------------------------------- restatement: the scene
def rest_of_scene(synth, **kw):
    pts, part = R.scene(synth, **kw)
    seg = PR.segment_planes(pts, R.PLANE)
    assert seg["n_planes"] == 1
    keep = seg["labels"] == -1
    return seg["rest"], part[keep]


def test_scene_floor_off_then_six_parts(synth):
    """With the floor taken off by one plane at 2 mm, eps 10 and 12 mm at min_points 10 find the six parts: each part's majority
    cluster holds at least 99 % of what is left of it.  At eps 8 mm / min_points 5 a speck of a few points makes a seventh cluster,
    which min_cluster_size = 20 drops."""
    rest, part = rest_of_scene(synth)
    assert (part == -1).mean() < 0.01 and len(rest) > 20000              # the floor is gone, the parts stay
    for eps, mp in R.PARAMS[:2]:
        r = R.cluster(rest, eps, mp)
        print(eps, mp, r["result"])
        assert r["result"]["n_clusters"] == 6, r["result"]
        major = []
        for b in range(6):
            lab = r["labels"][part == b]
            m = int(np.bincount(lab[lab >= 0]).argmax())
            major.append(m)
            assert (lab == m).mean() >= 0.99, (eps, b, (lab == m).mean())
        assert sorted(major) == list(range(6))                          # six different clusters
        assert (r["labels"][part == -2] == -1).all()                    # the strays are noise
    eps, mp = R.PARAMS[2]
    r = R.cluster(rest, eps, mp)
    print(eps, mp, r["result"], np.diff(r["offsets"]))
    assert r["result"]["n_clusters"] >= 6
    f = R.cluster(rest, eps, mp, 20)
    assert f["result"]["n_clusters"] == 6 and f["result"]["n_dropped"] == r["result"]["n_clusters"] - 6
    assert np.array_equal(f["labels"] >= 0, (r["labels"] >= 0) & (np.diff(r["offsets"])[np.maximum(r["labels"], 0)] >= 20))
