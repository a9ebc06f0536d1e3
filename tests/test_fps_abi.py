"""CPU suite: farthest point sampling (include/tdv_hip.h: tdv_farthest_point_down_sample).  The ABI exports the entry points, lists them
in ABI_SYMBOLS, has the documented struct layout and constants, and refuses every bad argument before it writes anything; the restatement
(tests/fps_restatement.py) is held to an independent definition (every sample recomputed from scratch from the explicit list of earlier
samples, no running array), to prefix stability, to the cover guarantee by brute force, to distinct indices on equal rows and to a row
permutation.  No compute entry point of the library runs here; tests/test_gpu_fps.py holds the device to this restatement byte for byte."""
import ctypes as C

import numpy as np
import pytest

import fps_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_farthest_point_down_sample", "tdv_farthest_point_down_sample_dev", "tdv_farthest_point_down_sample_batch_dev",
           "tdv_ctx_set_fps_path", "tdv_ctx_last_fps_path")


def test_symbols_constants_and_struct(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.FpsResultC) == 16
    assert [k for k, _ in tdv.FpsResultC._fields_] == ["n_usable", "n_selected", "path", "cover_d2"]
    assert tdv.FpsResultC.path.offset == 8 and tdv.FpsResultC.cover_d2.offset == 12
    assert (tdv.TDV_FPS_AUTO, tdv.TDV_FPS_WORKGROUP, tdv.TDV_FPS_GRID) == (0, 1, 2) == (R.AUTO, R.WORKGROUP, R.GRID)
    assert tdv.TDV_FPS_MAX_POINTS == R.MAX_POINTS == 1 << 22
    assert tdv.TDV_FPS_WORKGROUP_MAX == R.WORKGROUP_MAX and tdv.TDV_FPS_WORKGROUP_LANES == R.WORKGROUP_LANES
    assert R.WORKGROUP_MAX % R.WORKGROUP_LANES == 0
    assert lib.tdv_ctx_set_fps_path(None, 0) == TDV_ERR_BAD_ARG and lib.tdv_ctx_last_fps_path(None) == 0


# ---------------------------------------------------------------- arguments
GOOD = dict(n=4, num_samples=2, start_index=0, attr_width=3)
BAD = [("null ctx", {}), ("n < 0", dict(n=-1)), ("n > 2^22", dict(n=R.MAX_POINTS + 1)), ("num_samples < 0", dict(num_samples=-1)),
       ("start_index < 0", dict(start_index=-1)), ("start_index == n", dict(start_index=4)), ("attr_width < 0", dict(attr_width=-1))]


class Outputs:
    """Every output of a call with room for n samples, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n, width=3, fill=0x5A, clouds=1):
        self.res = (tdv.FpsResultC * clouds)(); C.memset(C.byref(self.res), fill, C.sizeof(self.res))
        self.index = np.full(n, -7, np.int32); self.d2 = np.full(n, -7, F); self.rows = np.full((n, 3), -7, F)
        self.cols = np.full((n, max(width, 1)), -7, F); self.out_off = np.full(clouds + 1, -7, np.int32)
        self.before = self.snapshot()

    def arrays(self):
        return self.index, self.d2, self.rows, self.cols, self.out_off

    def snapshot(self):
        return (bytes(self.res),) + tuple(a.tobytes() for a in self.arrays())

    def untouched(self):
        return self.snapshot() == self.before


def P(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def fps_call(lib, dev, ctx, pts, attr, o, res=True, cols=True, **kw):
    """Host arrays in every slot: a refused call must not look at them (the device entry point included)."""
    g = dict(GOOD, **kw)
    fn = lib.tdv_farthest_point_down_sample_dev if dev else lib.tdv_farthest_point_down_sample
    return fn(ctx, P(pts), g["n"], g["num_samples"], g["start_index"], P(attr), g["attr_width"], C.byref(o.res) if res else None, P(o.index),
              P(o.d2), P(o.rows), P(o.cols) if cols else None)


def fps_batch_call(lib, ctx, pts, attr, off, o, num_samples=2, attr_width=3, res=True, out_off=True, cols=True, n_clouds=None):
    return lib.tdv_farthest_point_down_sample_batch_dev(ctx, P(pts), P(attr), attr_width, P(off), len(off) - 1 if n_clouds is None else n_clouds,
                                                        num_samples, C.byref(o.res) if res else None, P(o.out_off) if out_off else None,
                                                        P(o.index), P(o.d2), P(o.rows), P(o.cols) if cols else None)


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_fps.py refuses each bad argument on one."""
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); attr = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4)
        assert fps_call(lib, dev, None, pts, attr, o, **BAD[case][1]) == TDV_ERR_BAD_ARG
        assert o.untouched()


def null_and_attr_cases(lib, dev, ctx, pts, attr, o):
    """The refusals that are not a number's: every one must return TDV_ERR_BAD_ARG."""
    yield fps_call(lib, dev, ctx, None, None, o, attr_width=0, cols=False)         # a NULL cloud with n > 0
    yield fps_call(lib, dev, ctx, pts, attr, o, res=False)                         # a NULL result
    yield fps_call(lib, dev, ctx, pts, None, o)                                    # attr_width > 0 with a NULL attr
    yield fps_call(lib, dev, ctx, pts, None, o, attr_width=0)                      # out_attr without attr


def batch_bad_cases(lib, ctx, pts, attr, o):
    good = np.array([0, 2, 4], np.int32)
    yield fps_batch_call(lib, ctx, pts, attr, good, o, n_clouds=-1)                # n_clouds < 0
    yield fps_batch_call(lib, ctx, pts, attr, None, o, n_clouds=2)                 # NULL offsets
    yield fps_batch_call(lib, ctx, pts, attr, good, o, out_off=False)              # NULL out offsets
    yield fps_batch_call(lib, ctx, pts, attr, good, o, res=False)                  # NULL results
    yield fps_batch_call(lib, ctx, pts, attr, np.array([1, 2, 4], np.int32), o)    # offsets that do not start at 0
    yield fps_batch_call(lib, ctx, pts, attr, np.array([0, 3, 2], np.int32), o)    # ... that decrease
    yield fps_batch_call(lib, ctx, pts, attr, np.array([0, R.MAX_POINTS + 1, R.MAX_POINTS + 2], np.int32), o)     # a cloud above 2^22
    yield fps_batch_call(lib, ctx, None, None, good, o, attr_width=0, cols=False)  # a NULL cloud array with rows
    yield fps_batch_call(lib, ctx, pts, attr, good, o, num_samples=-1)             # num_samples < 0
    yield fps_batch_call(lib, ctx, pts, attr, good, o, attr_width=-1)              # attr_width < 0
    yield fps_batch_call(lib, ctx, pts, None, good, o)                             # attr_width > 0 with a NULL attr
    yield fps_batch_call(lib, ctx, pts, None, good, o, attr_width=0)               # out_attr without attr


def test_null_arrays_and_attr(tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); attr = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4, fill=0x33)
        for status in null_and_attr_cases(lib, dev, None, pts, attr, o):
            assert status == TDV_ERR_BAD_ARG
        assert o.untouched()
    o = Outputs(tdv, 4, fill=0x33, clouds=2)
    for status in batch_bad_cases(lib, None, pts, attr, o):
        assert status == TDV_ERR_BAD_ARG
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against an independent definition
def cloud(n=3000, seed=1, nan_row=17, dup=(40, 2000)):
    """Random points with one NaN row and one duplicated row."""
    pts = np.random.default_rng(seed).random((n, 3)).astype(F)
    if nan_row is not None:
        pts[nan_row] = np.nan
    if dup and dup[1] < n:
        pts[dup[1]] = pts[dup[0]]
    return pts


def lattice():
    """8 x 8 x 2 at spacing 0.25: a handful of distinct distances, ties everywhere."""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    return (g * 0.25).astype(F)


def from_scratch(xyz, k, start):
    """Sample i as the arg-max over the unselected usable rows of the minimum of d2 over the explicit list of earlier samples: the same f32
    expression, no running array.  O(k^2 n)."""
    usable = np.isfinite(xyz).all(1)
    rows = np.flatnonzero(usable)
    k = min(k, len(rows))
    chosen, dist = [], []
    for i in range(k):
        if i == 0:
            j, d = (start if usable[start] else int(rows[0])), F(np.inf)
        else:
            left = np.array([r for r in rows if r not in set(chosen)])
            near = np.min(np.stack([R.d2_f32(xyz[left], xyz[s]) for s in chosen]), 0)
            best = near.max()
            j, d = int(left[np.flatnonzero(near == best)[0]]), best
        chosen.append(j); dist.append(d)
    return np.array(chosen, np.int32), np.array(dist, F)


@pytest.mark.parametrize("name, pts, k, start", [("random", cloud(400, 3, 5, (7, 300)), 60, 11), ("lattice", lattice(), 128, 0),
                                                 ("start unusable", cloud(300, 4, 0, None), 40, 0),
                                                 ("far apart", np.r_[cloud(100, 5, None, None), F([[1e30, 0, 0], [-1e30, 0, 0]])], 30, 3)])
def test_against_the_definition_from_scratch(name, pts, k, start):
    out = R.fps(pts, k, start)
    idx, d = from_scratch(pts, k, start)
    assert np.array_equal(out["index"], idx), name
    assert out["d2"].tobytes() == d.tobytes(), name
    assert out["n_selected"] == len(idx) == len(set(idx.tolist()))


def test_distinct_monotone_and_prefix_stable():
    pts = cloud()
    big = R.fps(pts, 512, 9)
    assert big["n_usable"] == 2999 and big["n_selected"] == 512 and len(set(big["index"].tolist())) == 512 and 17 not in big["index"]
    assert big["index"][0] == 9 and np.isinf(big["d2"][0]) and (np.diff(big["d2"][1:]) <= 0).all()
    small = R.fps(pts, 100, 9)
    for key in ("index", "d2", "xyz"):
        assert small[key].tobytes() == big[key][:100].tobytes(), key
    assert not ({40, 2000} <= set(big["index"].tolist())) or big["d2"][-1] == 0     # the duplicate of a sample has m = 0: it comes last, if at all


def test_lattice_exercises_the_tie_rule():
    out = R.fps(lattice(), 128, 0)
    assert sorted(out["index"].tolist()) == list(range(128)) and out["cover_d2"] == 0
    assert len(np.unique(out["d2"])) <= 12                                        # few distinct distances: nearly every choice is a tie


@pytest.mark.parametrize("k", [0, 1, 7, 200])
def test_cover_guarantee_by_brute_force(k):
    pts = cloud(500, 8)
    out = R.fps(pts, k, 3)
    usable = np.isfinite(pts).all(1)
    rest = usable.copy(); rest[out["index"]] = False
    if k == 0:
        assert out["n_selected"] == 0 and np.isinf(out["cover_d2"]) and out["cover_d2"] > 0      # no sample: nothing is covered
        return
    near = np.min(np.stack([R.d2_f32(pts, pts[s]) for s in out["index"]]), 0)
    assert out["cover_d2"] == near[rest].max() and (near[usable] <= out["cover_d2"]).all()
    assert out["cover_d2"] <= out["d2"][-1]                                       # the next sample would be no farther than the last
    assert R.fps(pts, 499, 3)["cover_d2"] == 0 and R.fps(pts, 499, 3)["cover_d2"].tobytes() == F(0).tobytes()     # nothing left: +0.0


def test_equal_rows_give_distinct_indices():
    pts = np.tile(F([[0.5, -1.0, 2.0]]), (50, 1))
    out = R.fps(pts, 20, 30)
    assert out["index"].tolist() == [30] + list(range(19))                         # every m is 0 after the first: the lowest index each time
    assert out["d2"][1:].tolist() == [0.0] * 19 and out["n_selected"] == 20
    few = R.fps(np.r_[pts[:3], F([[9, 9, 9]])], 10, 0)
    assert few["n_selected"] == 4 and sorted(few["index"].tolist()) == [0, 1, 2, 3] and few["index"][1] == 3


def test_row_permutation_without_ties():
    """A permutation that keeps the start row first yields the permuted result on a cloud with no ties."""
    pts = cloud(800, 12, None, None)
    attr = np.random.default_rng(2).random((800, 4)).astype(F)
    a = R.fps(pts, 300, 0, attr)
    assert len(np.unique(a["d2"])) == 300                                          # no two samples at one distance: no tie decided anything
    perm = np.r_[0, 1 + np.random.default_rng(3).permutation(799)]
    b = R.fps(pts[perm], 300, 0, attr[perm])
    assert np.array_equal(perm[b["index"]], a["index"])
    for key in ("d2", "xyz", "attr"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["cover_d2"] == b["cover_d2"]


def test_batch_restatement_offsets():
    pts = cloud(300, 6)
    off = np.array([0, 0, 1, 50, 300], np.int32)
    out, out_off = R.fps_batch(pts, off, 20)
    assert out_off.tolist() == [0, 0, 1, 21, 41] and out[2]["index"][0] == 0 and out[0]["cover_d2"] == 0
    assert out[2]["n_usable"] == 48 and out[3]["index"].max() < 250                # row 17 is NaN; indices count inside the cloud
