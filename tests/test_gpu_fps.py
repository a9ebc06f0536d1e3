"""Farthest point sampling on the device (include/tdv_hip.h: tdv_farthest_point_down_sample) against the restatement of
tests/fps_restatement.py, byte for byte: the result struct, index, out_d2, out_xyz and out_attr, from the host, the device and the batch
entry points, on both kernel families wherever the size allows, each test on a Context of its own.  The sizes are the wave (63, 64, 65), the
workgroup (T - 1, T, T + 1 with T = TDV_FPS_WORKGROUP_LANES: where a lane takes its second row) and the path (TDV_FPS_WORKGROUP_MAX, + 1)
edges."""
import ctypes as C

import numpy as np
import pytest
import torch

import fps_restatement as R
from test_fps_abi import BAD, Outputs, batch_bad_cases, cloud, fps_batch_call, fps_call, lattice, null_and_attr_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TDV_ERR_BAD_ARG = -2
F = np.float32
T = R.WORKGROUP_LANES
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 3000]
PATHS = ("workgroup", "grid")
MODE = {"auto": R.AUTO, "workgroup": R.WORKGROUP, "grid": R.GRID}
PAD = 7                                                      # entries past the capacity of every device output: never written


@pytest.fixture
def fctx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


def _up(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    t = torch.zeros(max(a.size, 4), dtype=getattr(torch, np.dtype(dtype).name), device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a.copy()).to(DEV))
    return t, t.data_ptr()


def _width(attr):
    return 0 if attr is None else np.asarray(attr).shape[-1]


def dev_call(ctx, pts, k, start=0, attr=None, skip=()):
    """tdv_farthest_point_down_sample_dev with every output asked for (but those in `skip`), read back with torch."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n, w = len(pts), _width(attr)
    cap = min(k, n) + PAD
    (pts_t, px), (it, pi), (dt, pd), (xt, pxo) = _up(pts), _up(np.full(cap, -9, np.int32), np.int32), _up(np.full(cap, -9, F)), _up(np.full((cap, 3), -9, F))
    (attr_t, pa), (ct, pc) = (_up(attr), _up(np.full(cap * max(w, 1), -9, F))) if attr is not None else ((None, None), (None, None))
    torch.cuda.synchronize()                                 # the uploads are torch's; the ctx runs on a stream of its own
    res = ctx.fps_dev(px, n, k, start, pa, w, None if "index" in skip else pi, None if "d2" in skip else pd, None if "xyz" in skip else pxo,
                      None if "attr" in skip else pc)
    torch.cuda.synchronize()
    m = res["n_selected"]
    out = dict(index=it.cpu().numpy(), d2=dt.cpu().numpy(), xyz=xt.cpu().numpy().reshape(-1, 3),
               attr=None if attr is None else ct.cpu().numpy()[:cap * w].reshape(cap, w) if w else np.zeros((cap, 0), F))
    for key, a in out.items():
        if a is not None and a.size:
            assert (a[0 if key in skip else m:] == -9).all(), (key, "written beyond n_selected" if key not in skip else "written though not asked for")
    res.update({key: (None if a is None or key in skip else a[:m]) for key, a in out.items()})
    return res


def same(ref, got, what, skip=()):
    assert [got[k] for k in R.RESULT[:3]] == [ref[k] for k in R.RESULT[:3]], (what, "result", {k: (got[k], ref[k]) for k in R.RESULT})
    assert F(got["cover_d2"]).tobytes() == F(ref["cover_d2"]).tobytes(), (what, "cover_d2", got["cover_d2"], ref["cover_d2"])
    for k in ("index", "d2", "xyz", "attr"):
        if ref[k] is not None and k not in skip:
            assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes(), (what, k)


def check(ctx, pts, k, start=0, attr=None, what=None, paths=PATHS):
    """Host and device entry points on each path against the restatement."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    base = R.fps(pts, k, start, attr)
    for path in paths:
        ctx.set_fps_path(path)
        ref = dict(base, path=R.path_of(len(pts), MODE[path]))
        for name, got in (("host", ctx.fps(pts, k, start, attr)), ("dev", dev_call(ctx, pts, k, start, attr))):
            same(ref, got, (what, len(pts), k, start, path, name))
            assert ctx.last_fps_path() == ("workgroup" if ref["path"] == R.WORKGROUP else "grid")
    ctx.set_fps_path("auto")
    return base


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_sample_counts(fctx, n):
    pts = cloud(n, 100 + n, nan_row=None, dup=None)
    for k in sorted({0, 1, 2, n // 2, n, n + 5}):
        ref = check(fctx, pts, k, start=n // 3, what="sizes")
        assert ref["n_selected"] == min(k, n)


def test_path_edge_under_auto(fctx):
    for n, path in ((R.WORKGROUP_MAX, "workgroup"), (R.WORKGROUP_MAX + 1, "grid")):
        pts = cloud(n, n, nan_row=5)
        ref = check(fctx, pts, 64, start=n - 1, what="path edge", paths=("auto",))
        assert fctx.last_fps_path() == path and ref["n_usable"] == n - 1


def test_full_permutation_500(fctx):
    ref = check(fctx, cloud(500, 77, nan_row=None, dup=None), 500, start=123, what="permutation")
    assert sorted(ref["index"].tolist()) == list(range(500)) and ref["cover_d2"] == 0


def test_start_index(fctx):
    pts = cloud(700, 31, nan_row=300, dup=None)
    pts[0] = np.inf
    for start, first in ((0, 1), (699, 699), (300, 1), (1, 1)):           # rows 0 and 300 are unusable: the lowest usable row instead
        assert check(fctx, pts, 50, start=start, what="start")["index"][0] == first


def test_lattice_equal_rows_and_few_distinct(fctx):
    ref = check(fctx, lattice(), 128, what="lattice")
    assert len(np.unique(ref["d2"])) <= 12
    same_rows = np.tile(F([[0.25, -3.0, 1.5]]), (1500, 1))
    assert check(fctx, same_rows, 40, start=1100, what="equal rows")["index"].tolist() == [1100] + list(range(39))
    few = np.repeat(np.random.default_rng(4).random((9, 3)).astype(F), 50, 0)      # 450 rows, 9 distinct points, 200 samples
    ref = check(fctx, few, 200, start=7, what="few distinct")
    assert len(set(ref["index"].tolist())) == 200 and (ref["d2"][9:] == 0).all()


def test_nonfinite_rows(fctx):
    pts = cloud(2100, 41, nan_row=0, dup=None)
    rng = np.random.default_rng(6)
    for value in (np.nan, np.inf, -np.inf):
        pts[rng.integers(1, 2100, 30), rng.integers(0, 3, 30)] = value
    pts[1030] = np.nan; pts[2099, 2] = -np.inf
    ref = check(fctx, pts, 300, start=0, what="non-finite")
    assert ref["n_usable"] < 2050 and np.isfinite(ref["xyz"]).all()
    none = np.full((70, 3), np.nan, F)
    ref = check(fctx, none, 10, start=3, what="no usable row")
    assert ref["n_usable"] == 0 and ref["n_selected"] == 0 and ref["cover_d2"] == 0


def test_huge_coordinates(fctx):
    pts = cloud(1300, 51, nan_row=None, dup=None)
    pts[[5, 640, 1299]] = F([[1e30, 0, 0], [-1e30, 2, 1], [0, 1e30, -1e30]])
    ref = check(fctx, pts, 200, start=9, what="1e30")
    assert np.isinf(ref["d2"][:4]).all() and set(ref["index"][1:4].tolist()) == {5, 640, 1299}       # a d2 of +inf between finite rows


@pytest.mark.parametrize("width", [0, 3, 33])
def test_attr_widths(fctx, width):
    pts = cloud(1500, 61)
    attr = np.random.default_rng(width).random((1500, width)).astype(F)
    ref = check(fctx, pts, 400, start=2, attr=attr, what="attr")
    assert ref["attr"].shape == (400, width)


def test_every_optional_output_null_in_turn(fctx):
    pts = cloud(1200, 71)
    attr = np.random.default_rng(1).random((1200, 5)).astype(F)
    ref = R.fps(pts, 90, 4, attr)
    for path in PATHS:
        fctx.set_fps_path(path)
        for skip in (("index",), ("d2",), ("xyz",), ("attr",), ("index", "d2", "xyz", "attr")):
            same(dict(ref, path=MODE[path]), dev_call(fctx, pts, 90, 4, attr, skip=skip), (path, skip), skip=skip)
        r = host_result_only(fctx, pts, attr)
        assert (r.n_usable, r.n_selected) == (ref["n_usable"], 90) and F(r.cover_d2).tobytes() == F(ref["cover_d2"]).tobytes()


def host_result_only(ctx, pts, attr):
    """The host entry point with every output NULL: the result alone."""
    import importlib
    tdv = importlib.import_module("3dvision_amd")
    res = tdv.FpsResultC()
    P = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    assert tdv.lib().tdv_farthest_point_down_sample(ctx._h, P(pts), len(pts), 90, 4, P(attr), attr.shape[1], C.byref(res), None, None, None, None) == 0
    return res


# ---------------------------------------------------------------- batch
BATCH_SIZES = [0, 1, 2, 64, 65, 1000, 0, 3000, R.WORKGROUP_MAX + 1]


def batch_dev_call(ctx, pts, off, k, attr=None, skip=()):
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    w = _width(attr)
    cap = int(np.minimum(np.diff(off), k).sum()) + PAD
    (pts_t, px), (it, pi), (dt, pd), (xt, pxo) = _up(pts), _up(np.full(cap, -9, np.int32), np.int32), _up(np.full(cap, -9, F)), _up(np.full((cap, 3), -9, F))
    (attr_t, pa), (ct, pc) = (_up(attr), _up(np.full(cap * max(w, 1), -9, F))) if attr is not None else ((None, None), (None, None))
    torch.cuda.synchronize()
    res, out_off = ctx.fps_batch_dev(px, off, k, pa, w, None if "index" in skip else pi, pd, pxo, pc)
    torch.cuda.synchronize()
    index, d2, xyz = it.cpu().numpy(), dt.cpu().numpy(), xt.cpu().numpy().reshape(-1, 3)
    cols = None if attr is None else ct.cpu().numpy()[:cap * w].reshape(cap, w)
    end = int(out_off[-1])
    assert (d2[end:] == -9).all() and (xyz[end:] == -9).all() and (index[0 if "index" in skip else end:] == -9).all(), "written past the end"
    assert cols is None or (cols[end:] == -9).all()
    out = []
    for b, r in enumerate(res):
        a, e = int(out_off[b]), int(out_off[b + 1])
        out.append(dict(r, index=index[a:e], d2=d2[a:e], xyz=xyz[a:e], attr=None if cols is None else cols[a:e]))
    return out, out_off


def batch_case(seed=5):
    off = np.concatenate([[0], np.cumsum(BATCH_SIZES)]).astype(np.int32)
    pts = np.random.default_rng(seed).random((int(off[-1]), 3)).astype(F)
    pts[off[5] + 7] = np.nan; pts[off[7]] = np.inf; pts[off[8] + 16000, 1] = np.nan          # unusable rows, one a cloud's row 0
    attr = np.random.default_rng(seed + 1).random((len(pts), 3)).astype(F)
    return pts, attr, off


def test_batch_against_restatement_and_single_calls(fctx):
    pts, attr, off = batch_case()
    refs, ref_off = R.fps_batch(pts, off, 256, attr)
    got, out_off = batch_dev_call(fctx, pts, off, 256, attr)
    assert fctx.last_fps_path() == "grid"                                        # one cloud is above the workgroup's capacity
    assert np.array_equal(out_off, ref_off) and out_off.dtype == np.int32
    for b, (r, g) in enumerate(zip(refs, got)):
        same(r, g, ("batch", b, BATCH_SIZES[b]))
        one = dev_call(fctx, pts[off[b]:off[b + 1]], 256, 0, attr[off[b]:off[b + 1]])
        same(one, g, ("batch against the single call", b))
    host = fctx.fps_batch(pts, off, 256, attr)
    for b, (r, g) in enumerate(zip(refs, host)):
        same(r, g, ("fps_batch", b))
    got, _ = batch_dev_call(fctx, pts, off, 256, attr, skip=("index",))          # attr rows without the caller's index array
    for b, (r, g) in enumerate(zip(refs, got)):
        same(r, g, ("batch without index", b), skip=("index",))


def test_batch_forced_paths_and_empty_batches(fctx, tdv):
    pts, attr, off = batch_case(9)
    off = off[:8]                                                                # the clouds up to 1,000 rows (and the empty ones)
    pts, attr = pts[:off[-1]], attr[:off[-1]]
    refs, ref_off = R.fps_batch(pts, off, 40, attr)
    for path in PATHS:
        fctx.set_fps_path(path)
        got, out_off = batch_dev_call(fctx, pts, off, 40, attr)
        assert np.array_equal(out_off, ref_off) and fctx.last_fps_path() == path
        for b, (r, g) in enumerate(zip(refs, got)):
            same(dict(r, path=MODE[path]), g, ("batch", path, b))
    fctx.set_fps_path("auto")
    res, out_off = fctx.fps_batch_dev(None, np.zeros(1, np.int32), 5)            # no cloud
    assert res == [] and out_off.tolist() == [0]
    res, out_off = fctx.fps_batch_dev(None, np.zeros(4, np.int32), 5)            # three clouds without a row
    assert out_off.tolist() == [0, 0, 0, 0] and [(r["n_usable"], r["n_selected"], r["path"], float(r["cover_d2"])) for r in res] == [(0, 0, 1, 0.0)] * 3
    many = np.arange(0, 1301 * 9, 9, dtype=np.int32)                             # more clouds than the plan's workgroup has lanes
    pts = np.random.default_rng(2).random((int(many[-1]), 3)).astype(F)
    refs, ref_off = R.fps_batch(pts, many, 4)
    got, out_off = batch_dev_call(fctx, pts, many, 4)
    assert np.array_equal(out_off, ref_off)
    for b in (0, 1, 1023, 1024, 1025, 1299):
        same(refs[b], got[b], ("1,300 clouds", b))


# ---------------------------------------------------------------- switches, refusals, repeatability
def test_refusals_on_a_real_context(fctx, tdv):
    lib = tdv.lib()
    pts = np.zeros((4, 3), F); attr = np.zeros((4, 3), F)
    for dev in (False, True):
        o = Outputs(tdv, 4)
        for case in BAD[1:]:
            assert fps_call(lib, dev, fctx._h, pts, attr, o, **case[1]) == TDV_ERR_BAD_ARG, case[0]
        for status in null_and_attr_cases(lib, dev, fctx._h, pts, attr, o):
            assert status == TDV_ERR_BAD_ARG
        assert o.untouched()
    o = Outputs(tdv, 4, clouds=2)
    for status in batch_bad_cases(lib, fctx._h, pts, attr, o):
        assert status == TDV_ERR_BAD_ARG
    assert o.untouched()
    assert lib.tdv_ctx_set_fps_path(fctx._h, 3) == TDV_ERR_BAD_ARG and lib.tdv_ctx_set_fps_path(fctx._h, -1) == TDV_ERR_BAD_ARG
    # n == 0 and num_samples == 0 are accepted
    r = fctx.fps(np.zeros((0, 3), F), 5)
    assert (r["n_usable"], r["n_selected"], r["path"], len(r["index"])) == (0, 0, R.WORKGROUP, 0) and r["cover_d2"] == 0
    assert fctx.fps_dev(None, 0, 0)["n_selected"] == 0


def test_forced_workgroup_above_capacity_is_refused(fctx, tdv):
    lib = tdv.lib()
    n = R.WORKGROUP_MAX + 1
    pts = np.zeros((n, 3), F)
    assert fctx.last_fps_path() == "auto"
    fctx.set_fps_path("workgroup")
    for dev in (False, True):
        o = Outputs(tdv, 4, width=0)
        assert fps_call(lib, dev, fctx._h, pts, None, o, n=n, attr_width=0, cols=False) == TDV_ERR_BAD_ARG
        assert o.untouched()
    o = Outputs(tdv, 4, width=0, clouds=2)
    assert fps_batch_call(lib, fctx._h, pts, None, np.array([0, 3, n + 3], np.int32), o, attr_width=0, cols=False) == TDV_ERR_BAD_ARG
    assert o.untouched() and fctx.last_fps_path() == "auto"
    assert fps_call(lib, False, fctx._h, pts, None, Outputs(tdv, 4, width=0), n=n - 1, attr_width=0, cols=False) == 0      # at capacity: accepted
    assert fctx.last_fps_path() == "workgroup"
    fctx.set_fps_path("grid")
    assert fctx.fps(pts[:10], 3)["path"] == R.GRID and fctx.last_fps_path() == "grid"


def test_two_identical_calls_give_identical_bytes(fctx):
    pts = cloud(20000, 81)
    attr = np.random.default_rng(8).random((20000, 3)).astype(F)
    for path, n in (("workgroup", 9000), ("grid", 20000)):
        fctx.set_fps_path(path)
        a, b = fctx.fps(pts[:n], 300, 5, attr[:n]), fctx.fps(pts[:n], 300, 5, attr[:n])
        same(a, b, ("twice", path))
        assert a["n_selected"] == 300 and len(set(a["index"].tolist())) == 300


def test_open3d_style_call(fctx):
    pts = cloud(900, 91, nan_row=None, dup=None)
    rows = fctx.farthest_point_down_sample(pts, 64, start_index=10)
    assert rows.tobytes() == R.fps(pts, 64, 10)["xyz"].tobytes() and rows.shape == (64, 3)
