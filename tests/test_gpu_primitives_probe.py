"""The shared device primitives underneath the stages - exclusive_scan_dev, sort_records_dev, segment_sort_records_dev (csrc/sort.hip),
the gather tail of outlier and ISS (csrc/flag_gather.hpp) and the fixed f64 tree (csrc/fixed_tree.hpp) - each called directly through
the study library's second probe (csrc/probe.hip: tdv_study_primitive, the very functions the product paths call) and held to numpy
BYTE FOR BYTE: the scan to a cumsum in int64 cast back, the sorts to np.lexsort on unsigned columns, the gather to np.flatnonzero, the
tree to tests/fixed_tree_restatement.py (written from the header's rule 4, addition by addition; a NaN of the restatement needs a NaN of
the device, payload free).  Every output buffer is prefilled with a sentinel and nothing beyond what the call owns may change.

The sizes are the ones at which the code changes path: the scan's last workgroup loops a second time above 1,024 blocks (4,194,304 items)
and loads scalar where its input is not 16-byte aligned; the bitonic launch chain is local passes only at 2,048 records, one single global
step at 4,096, one fused two-stride step at 8,192, a fused and a single step at 16,384, two fused steps at 32,768; a segment pads to the
next power of two up to the tile of 2,048; the tree's partial loop takes one term per thread up to 65,536 terms and two above.

The tests named test_probed_* need the study library: tests/test_gpu_study_build.py runs them in its study process."""
import ctypes as C

import numpy as np
import pytest
import torch

import fixed_tree_restatement as T
import outlier_restatement as OR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BAD_ARG = -2
INT_MAX = 2 ** 31 - 1
SENT = -77
ONES = np.uint32(0xffffffff)


def reach(count, least, what):
    print("reach: %s: %d (at least %d)" % (what, count, least))
    assert count >= least, "the inputs no longer reach '%s': %d < %d" % (what, count, least)


def up(a):
    """A numpy array's bytes on the device (uint32 travels as int32)."""
    a = np.array(a, copy=True)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def filled(count, dtype, value=SENT):
    return torch.full((max(int(count), 1),), value, dtype=dtype, device=DEV)


def same_f64(got, ref, what):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = (gn != rn) | (~gn & ~rn & (got.view(np.uint64) != ref.view(np.uint64)))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: device %r (%s) restatement %r (%s)" % (
            what, int(bad.sum()), bad.size, i, got[i], got[i].tobytes().hex(), ref[i], ref[i].tobytes().hex()))


# ------------------------------------------------------------------------------------------------ exclusive scan
PAD = 64


def scan_values(n, rng):
    yield "all 0", np.zeros(n, np.int32)
    yield "all 1", np.ones(n, np.int32)
    yield "random 0..3", rng.integers(0, 4, n).astype(np.int32)
    last = np.zeros(n, np.int32); last[-1] = 1
    yield "a single 1 in the last place", last
    full = np.ones(n, np.int32); full[0] = INT_MAX - (n - 1)
    assert int(full.astype(np.int64).sum()) == INT_MAX
    yield "a total of exactly INT_MAX", full


def run_scan(ctx, x, shift=0, what=None):
    """x scanned from an input that starts `shift` ints past a 16-byte boundary; the output and the total against the int64 cumsum."""
    n = len(x)
    d_in = filled(n + 4, torch.int32, 0)
    assert d_in.data_ptr() % 16 == 0
    d_in[shift:shift + n].copy_(up(x))
    d_out = filled(n + PAD, torch.int32); d_tot = filled(4, torch.int32)
    torch.cuda.synchronize()
    ctx.study_primitive("exclusive_scan", n, in0=d_in.data_ptr() + 4 * shift, out0=d_out.data_ptr(), out1=d_tot.data_ptr() + 4)
    inc = np.cumsum(x.astype(np.int64))
    want = np.concatenate([[0], inc[:-1]]).astype(np.int32)
    out = d_out.cpu().numpy()
    assert out[:n].tobytes() == want.tobytes(), (what, n, shift, "first difference at", int(np.flatnonzero(out[:n] != want)[0]))
    assert (out[n:] == SENT).all(), (what, n, shift, "written past n")
    assert d_tot.cpu().numpy().tolist() == [SENT, int(inc[-1]), SENT, SENT], (what, n, shift, d_tot.cpu().numpy(), int(inc[-1]))


SCAN_SIZES = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8193, 300001,
              4194304,                       # 1,024 blocks: the most one round of the last workgroup's loop takes
              4194305, 4194304 + 4097,       # a second round of one and of two blocks
              8388608 + 5]                   # three rounds


@pytest.mark.study
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_probed_exclusive_scan(ctx, n):
    rng = np.random.default_rng(n)
    for what, x in scan_values(n, rng):
        run_scan(ctx, x, 0, what)
        if n in (5, 4097, 300001):
            for shift in (1, 2, 3):
                run_scan(ctx, x, shift, what)


@pytest.mark.study
def test_probed_scan_ticket_returns_to_zero(tdv):
    """One context: a three-round, a one-block and a one-round scan, twice over - a ticket word left above 0 by any of them makes the next
    scan pick no last workgroup (or the wrong one) - and then a product call that scans, held to its restatement."""
    c = tdv.Context(0)
    try:
        rng = np.random.default_rng(77)
        xs = [rng.integers(0, 4, n).astype(np.int32) for n in (8388608 + 5, 5, 300001)]
        for rep in range(2):
            for x in xs:
                run_scan(c, x, 0, "ticket, repeat %d" % rep)
        pts = rng.random((1000, 3)).astype(np.float32)
        ref = OR.radius(pts, 5, 0.1)
        got = c.radius_outlier(pts, 5, 0.1)
        assert 0 < ref["n_kept"] < 1000 and (got["n_valid"], got["n_kept"]) == (ref["n_valid"], ref["n_kept"])
        for k in ("mask", "count", "index", "xyz"):
            assert np.ascontiguousarray(got[k]).tobytes() == ref[k].tobytes(), k
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ the bitonic sorts of 16-byte records
def record_families(n, rng):
    """(name, uint32 [n, 4]) - every family asserts that it holds what it claims."""
    r = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    reach(int((r[:, 0] >= 0x80000000).sum()), n // 4, "random: first words with the top bit set")
    yield "random over 32 bits", r

    alpha = np.array([0, 0x7fffffff, 0x80000001], np.uint32)
    a = np.empty((n, 4), np.uint32)
    a[:, :3] = alpha[rng.integers(0, 3, (n, 3))]
    a[:, 3] = rng.permutation(n).astype(np.uint32)
    reach(n - len(np.unique(a[:, :3], axis=0)), n - 27, "alphabet: records that share (x, y, z) with another")
    assert len(np.unique(a[:, 3])) == n
    yield "three-value alphabet, distinct w", a

    pool = rng.integers(0, 2 ** 32, (50, 4), dtype=np.uint64).astype(np.uint32)
    d = pool[rng.integers(0, 50, n)]
    reach(n - len(np.unique(d, axis=0)), n - 50, "exact duplicate records")
    yield "exact duplicates", d

    s = r[np.lexsort((r[:, 3], r[:, 2], r[:, 1], r[:, 0]))]
    yield "ascending", s
    yield "descending", s[::-1].copy()

    real = n - n // 3 - 1                                               # the voxel fallback: real < n_pow2 records, all-ones padding behind
    v = np.full((n, 4), ONES, np.uint32)
    v[:real, :3] = rng.integers(-40, 40, (real, 3)).astype(np.int32).view(np.uint32)      # voxel keys are signed ints
    minus1 = rng.random(real) < 0.05
    v[:real][minus1, :3] = ONES                                          # the voxel (-1, -1, -1): all-ones like the padding, but w < n
    v[:real, 3] = rng.permutation(real).astype(np.uint32)
    reach(int(((v[:, :3] == ONES).all(1) & (v[:, 3] < n)).sum()), max(real // 40, 1), "voxel: real records with x = y = z = 0xffffffff")
    reach(int((v[:real, 0] >= 0x80000000).sum()), real // 4, "voxel: negative keys")
    reach(int((v == ONES).all(1).sum()), n // 3, "voxel: all-ones padding records")
    yield "voxel keys and all-ones padding", v


def lexsorted(rec):
    return rec[np.lexsort((rec[:, 3], rec[:, 2], rec[:, 1], rec[:, 0]))]


@pytest.mark.study
@pytest.mark.parametrize("n", [2048, 4096, 8192, 16384, 32768, 262144])
def test_probed_sort_records(ctx, n):
    rng = np.random.default_rng(n + 1)
    for what, rec in record_families(n, rng):
        d = filled((n + PAD) * 4, torch.int32)
        d[:4 * n].copy_(up(rec).reshape(-1))
        torch.cuda.synchronize()
        ctx.study_primitive("sort_records", n, out0=d.data_ptr())
        out = d.cpu().numpy()
        got = out[:4 * n].view(np.uint32).reshape(n, 4)
        want = lexsorted(rec)
        assert got.tobytes() == want.tobytes(), (what, n, "first differing record", int(np.flatnonzero((got != want).any(1))[0]))
        assert (out[4 * n:] == SENT).all(), (what, n, "written past the records")
        if what.startswith("voxel"):                                     # the real (-1, -1, -1) records stand before the padding
            real = n - n // 3 - 1
            assert (got[:real, 3] < n).all() and (got[real:] == ONES).all()


@pytest.mark.study
def test_probed_segment_sort(ctx):
    """One launch per value family: segments of every edge length and random ones, in shuffled order, and records behind the last segment."""
    rng = np.random.default_rng(3)
    lens = np.array([0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048] + rng.integers(0, 2049, 40).tolist() + [0, 0, 2048], np.int64)
    lens = lens[rng.permutation(len(lens))]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    total, tail = int(start[-1]), 100
    assert lens.max() == 2048 and {0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048} <= set(lens.tolist())
    d_start = up(start)
    for what, rec in record_families(total + tail, rng):
        d = filled((total + tail + PAD) * 4, torch.int32)
        d[:4 * (total + tail)].copy_(up(rec).reshape(-1))
        torch.cuda.synchronize()
        ctx.study_primitive("segment_sort", len(lens), width=total + tail, in0=d_start.data_ptr(), out0=d.data_ptr())
        out = d.cpu().numpy()
        got = out[:4 * (total + tail)].view(np.uint32).reshape(-1, 4)
        for c in range(len(lens)):
            a, b = int(start[c]), int(start[c + 1])
            assert got[a:b].tobytes() == lexsorted(rec[a:b]).tobytes(), (what, "segment", c, "of length", b - a)
        assert got[total:].tobytes() == rec[total:].tobytes(), (what, "records after the last segment")
        assert (out[4 * (total + tail):] == SENT).all(), what


# ------------------------------------------------------------------------------------------------ flags -> scan -> gather
def run_compact(ctx, flag, xyz, attr, skip=None, what=None):
    n, width = len(flag), attr.shape[1]
    keep = np.flatnonzero(flag).astype(np.int32)
    m = len(keep)
    d_flag, d_xyz, d_attr = up(flag), up(xyz.reshape(-1)), up(attr.reshape(-1))
    d_idx, d_rows, d_cols, d_kept = filled(n + PAD, torch.int32), filled(3 * n + PAD, torch.float32), filled(width * n + PAD, torch.float32), filled(4, torch.int32)
    ptr = dict(out0=d_idx.data_ptr(), out1=d_rows.data_ptr(), out2=d_cols.data_ptr(), out3=d_kept.data_ptr() + 4)
    if skip:
        ptr[skip] = None
    torch.cuda.synchronize()
    ctx.study_primitive("compact", n, width=width, in0=d_flag.data_ptr(), in1=d_xyz.data_ptr(), in2=d_attr.data_ptr(), **ptr)
    idx, rows, cols, kept = d_idx.cpu().numpy(), d_rows.cpu().numpy(), d_cols.cpu().numpy(), d_kept.cpu().numpy()
    tag = (what, n, width, "skipped", skip)
    want = dict(out0=(idx, keep), out1=(rows, xyz[keep].reshape(-1)), out2=(cols, attr[keep].reshape(-1)))
    for k, (got, ref) in want.items():
        if k == skip:
            assert (got == SENT).all(), tag + (k, "written although NULL was passed")
        else:
            assert got[:len(ref)].tobytes() == ref.tobytes(), tag + (k,)
            assert (got[len(ref):] == SENT).all(), tag + (k, "rows beyond the kept count")
    assert kept.tolist() == ([SENT] * 4 if skip == "out3" else [SENT, m, SENT, SENT]), tag


@pytest.mark.study
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 100003])
def test_probed_compact(ctx, n):
    rng = np.random.default_rng(n + 2)
    xyz = rng.random((n, 3)).astype(np.float32)
    flags = {"all 0": np.zeros(n, np.int32), "all 1": np.ones(n, np.int32), "random": rng.integers(0, 2, n).astype(np.int32)}
    for width in (1, 3, 33):
        attr = rng.random((n, width)).astype(np.float32)
        for what, flag in flags.items():
            run_compact(ctx, flag, xyz, attr, None, what)
        if width == 3:
            for skip in ("out0", "out1", "out2", "out3"):
                run_compact(ctx, flags["random"] if n > 1 else flags["all 1"], xyz, attr, skip, "one output NULL")


# ------------------------------------------------------------------------------------------------ the fixed f64 tree
TREE_SIZES = [1, 63, 64, 65, 255, 256, 257, 65536, 65537, 131073]


def tree_terms(n, width, rng):
    yield "random non-negative", rng.random((n, width)) * 3.0
    big = rng.choice([1e15, -1e15, 3e12, -3e12], (n, width)) + rng.normal(size=(n, width))
    big[1::2] = -big[::2][:len(big[1::2])] + rng.normal(size=big[1::2].shape) * 1e-3         # pairs that almost cancel
    yield "mixed sign, heavy cancellation", big
    yield "all -0.0", np.full((n, width), -0.0)
    x = rng.random((n, width)); x[rng.integers(0, n), :] = np.inf
    yield "with +inf", x
    y = x.copy(); y[rng.integers(0, n), 0] = -np.inf
    yield "with +inf and -inf", y
    z = rng.random((n, width)); z[rng.integers(0, n), width - 1] = np.nan
    yield "with NaN", z


@pytest.mark.study
@pytest.mark.parametrize("n", TREE_SIZES)
def test_probed_tree_sum(ctx, n):
    nb = -(-n // 256)
    rng = np.random.default_rng(n + 3)
    for width in (1, 4, 6):
        for what, x in tree_terms(n, width, rng):
            d_x = up(x.reshape(-1))
            runs = []
            for rep in range(2):
                d_part, d_sum = filled(nb * width + PAD, torch.float64), filled(width + PAD, torch.float64)
                torch.cuda.synchronize()
                ctx.study_primitive("tree_sum", n, width=width, in0=d_x.data_ptr(), out0=d_part.data_ptr(), out1=d_sum.data_ptr())
                runs.append((d_part.cpu().numpy(), d_sum.cpu().numpy()))
            assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), (what, n, width, "two runs differ")
            part, total = runs[0]
            assert (part[nb * width:] == SENT).all() and (total[width:] == SENT).all(), (what, n, width, "written past the results")
            same_f64(part[:nb * width].reshape(nb, width), T.block_sums(x), (what, n, width, "workgroup sums"))
            same_f64(total[:width], T.tree_sum(x), (what, n, width, "tree sum"))
            if what == "all -0.0":                                       # the zero signs: -0.0 from a full workgroup, +0.0 at the end
                assert np.signbit(part[:(n // 256) * width]).all() and not np.signbit(total[:width]).any()


@pytest.mark.study
@pytest.mark.parametrize("n", TREE_SIZES)
def test_probed_tree_count_and_block_max(ctx, n):
    nb = -(-n // 256)
    rng = np.random.default_rng(n + 4)
    for what, v in (("flags", rng.integers(0, 2, n)), ("all 1", np.ones(n)), ("counts up to 1000", rng.integers(0, 1000, n))):
        v = v.astype(np.int32)
        d_v = up(v)
        runs = []
        for rep in range(2):
            d_cnt, d_tot = filled(nb + PAD, torch.int32), filled(4, torch.int32)
            torch.cuda.synchronize()
            ctx.study_primitive("tree_count", n, in0=d_v.data_ptr(), out0=d_cnt.data_ptr(), out1=d_tot.data_ptr() + 4)
            runs.append(d_cnt.cpu().numpy().tobytes() + d_tot.cpu().numpy().tobytes())
        assert runs[0] == runs[1]
        cnt = d_cnt.cpu().numpy()
        assert cnt[:nb].tobytes() == T.block_counts(v).tobytes() and (cnt[nb:] == SENT).all(), (what, n)
        assert d_tot.cpu().numpy().tolist() == [SENT, int(T.tree_count(v)), SENT, SENT] and int(T.tree_count(v)) == int(v.sum()), (what, n)
    x = rng.normal(size=n) * 10.0
    among = x.copy(); among[rng.random(n) < 0.3] = np.nan; among[0] = np.nan
    infs = x.copy(); infs[rng.integers(0, n)] = -np.inf; infs[rng.integers(0, n)] = np.inf
    for what, v in (("numbers", x), ("NaN among numbers", among), ("all NaN", np.full(n, np.nan)), ("infinities", infs), ("all -inf", np.full(n, -np.inf))):
        d_v = up(v)
        runs = []
        for rep in range(2):
            d_max = filled(nb + PAD, torch.float64)
            torch.cuda.synchronize()
            ctx.study_primitive("tree_block_max", n, in0=d_v.data_ptr(), out0=d_max.data_ptr())
            runs.append(d_max.cpu().numpy())
        assert runs[0].tobytes() == runs[1].tobytes(), (what, n, "two runs differ")
        assert (runs[0][nb:] == SENT).all()
        same_f64(runs[0][:nb], T.block_max(v), (what, n, "workgroup maxima"))
        if what == "all NaN":
            assert np.isnan(runs[0][:nb]).all()


# ------------------------------------------------------------------------------------------------ arguments
@pytest.mark.study
def test_probed_primitive_entry_point_arguments(ctx, tdv):
    """TDV_ERR_BAD_ARG (-2, include/tdv_hip.h) before anything is launched: an unknown op, negative counts, a NULL pointer with a count > 0,
    a record count that is no power of two >= 2,048, a segment longer than the tile, a scan of more than 2^30 items.  The buffers keep
    their pattern; n == 0 does nothing, whatever the pointers."""
    f = tdv.lib().tdv_study_primitive
    buf = filled(1 << 16, torch.int32, 0x5a5a5a5a)
    starts_long, starts_down, starts_past, starts_neg = up(np.array([0, 2049], np.int32)), up(np.array([0, 9, 5], np.int32)), \
        up(np.array([0, 100, 5000], np.int32)), up(np.array([-1, 10], np.int32))
    torch.cuda.synchronize()
    p = C.c_void_p(buf.data_ptr())

    def call(op, n, width=1, in0=p, in1=p, in2=p, out0=p, out1=p, out2=p, out3=p, h=ctx._h):
        return f(h, op, C.c_longlong(n), C.c_longlong(width), in0, in1, in2, out0, out1, out2, out3)
    for op in (-1, 7, 99):
        assert call(op, 4) == BAD_ARG, op
    for op in range(7):
        assert call(op, -1) == BAD_ARG and call(op, -(1 << 40)) == BAD_ARG, op
        assert call(op, 0, in0=None, in1=None, in2=None, out0=None, out1=None, out2=None, out3=None) == 0, op
    assert call(0, 4, h=None) == BAD_ARG
    needed = {0: ("in0", "out0", "out1"), 1: ("out0",), 2: ("in0", "out0"), 3: ("in0",), 4: ("in0", "out0", "out1"), 5: ("in0", "out0", "out1"),
              6: ("in0", "out0")}
    for op, names in needed.items():
        for name in names:
            assert call(op, 2048, 2048 if op == 2 else 1, **{name: None}) == BAD_ARG, (op, name)
    assert call(3, 16, in1=None) == BAD_ARG and call(3, 16, in2=None) == BAD_ARG          # rows asked for without their source
    for n in (1, 1000, 1024, 2047, 2049, 3000, 4095, 6144, (1 << 27)):
        assert call(1, n) == BAD_ARG, n
    for s, nseg in ((starts_long, 1), (starts_down, 2), (starts_past, 2), (starts_neg, 1)):
        assert call(2, nseg, 4096, in0=C.c_void_p(s.data_ptr())) == BAD_ARG, s
    assert call(0, (1 << 30) + 1) == BAD_ARG and call(5, (1 << 31) + 5) == BAD_ARG
    for width in (0, -3, 65):
        assert call(3, 16, width) == BAD_ARG and call(4, 16, width) == BAD_ARG, width
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5a5a5a5a).all()
    with pytest.raises(KeyError):
        ctx.study_primitive("no such op", 1)


def test_product_library_has_no_primitive_probe(ctx, tdv):
    assert not tdv.STUDY_BUILD, "this process must run the PRODUCT library"
    assert not hasattr(tdv.lib(), "tdv_study_primitive")
    with pytest.raises(tdv.TdvError):
        ctx.study_primitive("exclusive_scan", 1)
