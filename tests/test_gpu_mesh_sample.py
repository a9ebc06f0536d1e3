"""GPU suite: tdv_mesh_sample_points and tdv_mesh_sample_points_dev against tests/mesh_sample_restatement.py, byte for byte on every output
and the result struct: triangle counts on the scan's workgroup edges (255, 256, 257) and past 256 workgroup sums (65,540), sample counts on
the wave and workgroup edges, areas from one binade to thirty, bad and degenerate triangles - the bad indices placed so that a read of
them would leave the vertex array -, every optional output left out in turn, companion rows of width 0, 3 and 33, chunked draws (S7), and
Context.mesh_model_dev against the composition of this restatement with tests/fps_restatement.py.  Device buffers go through
state_cases.Env: outputs are pre-filled with 0xA5, and what a call must not write is compared with that."""
import numpy as np
import pytest

import mesh_cases
import mesh_sample_restatement as R
from mesh_sample_cases import binades_mesh, grid_mesh
from state_cases import Env
from test_mesh_sample_abi import BAD, Outputs, null_cases, sample_call, zero_weight_mesh

pytestmark = pytest.mark.gpu
F = np.float32
ROWS = dict(xyz=(3, F), normals=(3, F), triangle=(1, np.int32), bary=(2, F))      # per sample: columns and type (attr: the call's width)
PAD = 7                                                                            # rows of room past n_samples: never written


def run_dev(ctx, v, t, n, attr=None, seed=0, first=0, skip=(), env=None):
    """tdv_mesh_sample_points_dev with 0xA5-filled outputs of n + PAD rows: (outputs cut to n_sampled rows, the whole buffers)."""
    env = env or Env(ctx)
    width = 0 if attr is None else attr.shape[1]
    spec = dict(ROWS, attr=(width, F))
    bufs = {k: env.out((n + PAD) * max(c, 1), dt) for k, (c, dt) in spec.items() if k not in skip and not (k == "attr" and attr is None)}
    res = ctx.mesh_sample_dev(env.up(v), len(v), env.up(t), len(t), n, None if attr is None else env.up(attr), width, seed, first,
                              **{"d_out_" + k: b.data_ptr() for k, b in bufs.items()})
    m = res["n_sampled"]
    whole = {k: env.get(b, (n + PAD) * max(spec[k][0], 1), spec[k][1]) for k, b in bufs.items()}
    out = dict(res)
    for k, a in whole.items():
        c = spec[k][0]
        out[k] = a[:m * c].reshape((m, c) if k != "triangle" else (m,))
    return out, whole, spec


def same(ref, got, what, keys=None):
    for k in R.RESULT + ("surface_area",):
        a, b = ref[k], got[k]
        assert (np.float32(a).tobytes() == np.float32(b).tobytes()) if k == "area_max" else (a == b), (what, k, a, b)
    for k in keys if keys is not None else [k for k in R.OUTPUTS if k in got and got[k] is not None]:
        assert ref[k] is not None and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (what, k)


def untouched_beyond(whole, spec, m, what):
    """Rows beyond n_sampled still hold the fill."""
    for k, a in whole.items():
        rest = a[m * max(spec[k][0], 1) if spec[k][0] else 0:]
        assert (rest.view(np.uint8) == 0xA5).all(), (what, k)


def held(ctx, v, t, n, attr=None, seed=0, first=0, what="", host=False):
    ref = R.sample(v, t, n, attr, seed, first)
    got, whole, spec = run_dev(ctx, v, t, n, attr, seed, first)
    same(ref, got, (what, "dev"))
    untouched_beyond(whole, spec, ref["n_sampled"], what)
    if host:
        h = ctx.mesh_sample(v, t, n, attr, seed, first)
        same(ref, h, (what, "host"))
        assert (h["attr"] is None) == (attr is None)
    return ref, got


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("nt, n", [(1, 1), (2, 63), (255, 64), (256, 65), (257, 257), (65537 + 3, 100003), (257, 0), (4096, 4097),
                                   (4097, 4096), (8191, 1025), (8193, 5000)])
def test_triangle_and_sample_counts(ctx, nt, n):
    """The scan's workgroup of 256 on its edges, 257 workgroup sums (the second level of the scan past one turn's quarter), and sample
    counts around a wave and a workgroup; the first case through the host entry point as well.  4,096 triangles are the last mesh the
    sample kernel's LDS table holds whole; at 4,097 and 8,191 it holds every second entry (with a tail of one and of none short of a
    segment), at 8,193 every fourth; 4,096 and 4,097 samples are a workgroup's four turns and one more."""
    v, t = grid_mesh(nt, seed=nt)
    attr = np.random.default_rng(nt).random((len(v), 3)).astype(F)
    ref, got = held(ctx, v, t, n, attr, seed=nt & 7, what=(nt, n), host=nt == 1)
    assert ref["n_usable"] == nt and ref["n_sampled"] == n
    if n >= 100000:
        assert len(np.unique(got["triangle"])) > 0.6 * nt                          # the search reaches the whole of C (1 - exp(-1.5) = 0.78 of equal faces)


@pytest.mark.parametrize("which", ["box", "relief", "binades"])
def test_area_ranges(ctx, synth, which):
    if which == "box":
        v, t = mesh_cases.box((0.2, 0.12, 0.06), (0.01, -0.02, 0.3))
    elif which == "relief":
        v, t = mesh_cases.relief(synth.ReliefPart(seed=3), 0.002)
    else:
        v, t = binades_mesh()
    ref, _ = held(ctx, v, t, 5001, seed=11, what=which, host=True)
    if which == "binades":
        f = R.faces(v, t)
        assert f["area"].max() / f["area"][f["area"] > 0].min() > 2.0 ** 30 and ref["n_usable"] >= len(t) - 3 and ref["n_bad"] == 0
        lone = np.concatenate([v, np.array([[0, 0, 9], [3e-5, 0, 9], [0, 1e-5, 9]], F)])          # 1.5e-10 against ~1e4: below 2^-32 of it
        ref2, _ = held(ctx, lone, np.concatenate([t, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32), 5001, seed=11, what="with a sliver")
        assert ref2["n_degenerate"] == ref["n_degenerate"] + 1 and ref2["xyz"].tobytes() == ref["xyz"].tobytes()


# ---------------------------------------------------------------- bad input
def test_bad_triangles_take_no_part_and_read_nothing(ctx):
    """Indices of n_vertices, -1 and far beyond the array (a read of any of them would leave the tight vertex buffer), vertices of NaN and
    inf that only some triangles name, and coordinates of 1e30 whose area overflows: those triangles are bad, and the samples are those of
    the mesh with a zero-area triangle in each one's place.  Results only: nothing here can fault if the indices are tested before the reads."""
    v, t = grid_mesh(600, seed=2)
    nv = len(v)
    v = np.concatenate([v, np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0], [0, 1e30, 0], [0, 0, 0]], F)])
    nan, inf, big1, big2, zero = range(nv, nv + 5)
    bad = {0: (len(v), 1, 2), 5: (3, -1, 4), 255: (1, 2, 1 << 30), 256: (nan, 7, 8), 300: (9, inf, 10), 511: (zero, big1, big2),
           599: (-(1 << 31), 0, 1)}
    clean = t.copy()
    for k, tri in bad.items():
        t[k] = tri
        clean[k] = (0, 0, 0)
    attr = np.random.default_rng(3).random((len(v), 3)).astype(F)
    ref, got = held(ctx, v, t, 4000, attr, seed=5, what="bad triangles", host=True)
    assert (ref["n_bad"], ref["n_degenerate"], ref["n_usable"]) == (len(bad), 0, 600 - len(bad))
    assert not set(got["triangle"].tolist()) & set(bad)
    other, _, _ = run_dev(ctx, v, clean, 4000, attr, seed=5)
    assert (other["n_bad"], other["n_degenerate"]) == (0, len(bad)) and other["total_weight"] == got["total_weight"]
    for k in R.OUTPUTS:
        assert other[k].tobytes() == got[k].tobytes(), k
    # no vertex at all: every index is out of range
    r, whole, spec = run_dev(ctx, np.zeros((0, 3), F), np.array([[0, 1, 2]], np.int32), 10)
    assert (r["n_bad"], r["n_sampled"]) == (1, 0)
    untouched_beyond(whole, spec, 0, "no vertices")


@pytest.mark.parametrize("which", ["all bad", "all degenerate", "no triangles"])
def test_nothing_usable_writes_nothing(ctx, which):
    v, t, _ = zero_weight_mesh()
    if which == "all bad":
        t = np.array([[0, 1, 99], [-1, 0, 1]], np.int32)
    elif which == "all degenerate":
        t = t[[0, 3, 4, 5, 9]]
    else:
        t = t[:0]
    attr = np.ones((len(v), 2), F)
    ref, got = held(ctx, v, t, 300, attr, what=which, host=True)
    assert got["n_sampled"] == 0 and got["total_weight"] == 0 and got["n_usable"] == 0
    assert got["n_bad"] + got["n_degenerate"] == len(t)


# ---------------------------------------------------------------- optional outputs, companion rows
@pytest.mark.parametrize("width", [0, 3, 33])
def test_attr_widths(ctx, width):
    v, t = grid_mesh(700, seed=9)
    attr = np.random.default_rng(width).random((len(v), width)).astype(F)
    ref = R.sample(v, t, 1000, attr, seed=2)
    got, whole, spec = run_dev(ctx, v, t, 1000, attr, seed=2)
    same(ref, got, ("width", width))
    untouched_beyond(whole, spec, 1000, width)                                    # (width 0: the attr buffer is never written)
    h = ctx.mesh_sample(v, t, 1000, attr, seed=2)
    same(ref, h, ("width", width, "host"))


@pytest.mark.parametrize("skip", list(R.OUTPUTS) + ["all"])
def test_each_output_is_optional(ctx, skip):
    v, t = grid_mesh(300, seed=1)
    attr = np.random.default_rng(1).random((len(v), 4)).astype(F)
    ref = R.sample(v, t, 500, attr, seed=3)
    got, whole, spec = run_dev(ctx, v, t, 500, attr, seed=3, skip=R.OUTPUTS if skip == "all" else (skip,))
    same(ref, got, ("without", skip))
    assert set(whole) == (set() if skip == "all" else set(R.OUTPUTS) - {skip})
    untouched_beyond(whole, spec, 500, skip)


# ---------------------------------------------------------------- S7, arguments on a ctx
def test_chunks_are_the_whole(ctx):
    v, t = grid_mesh(5000, seed=6)
    whole, _, _ = run_dev(ctx, v, t, 1000, seed=8)
    parts = [run_dev(ctx, v, t, n, seed=8, first=f)[0] for f, n in ((0, 1), (1, 63), (64, 449), (513, 487))]
    for k in ("xyz", "normals", "triangle", "bary"):
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), k
    edge = (1 << 32) - 100                                                         # the counter's second word
    held(ctx, v, t, 300, seed=8, first=edge, what="across 2^32")
    far, _, _ = run_dev(ctx, v, t, 7, seed=8, first=(1 << 64) - 8)                 # the last a call may end on: first + n = 2^64 - 1
    same(R.sample(v, t, 7, seed=8, first_sample=(1 << 64) - 8), far, "the last seven")


def test_bad_arguments_on_a_context(tdv, ctx):
    o = Outputs(tdv)
    for what, kw in BAD[1:]:
        for dev in (False, True):
            assert sample_call(tdv, dev, ctx._h, o, **kw) == -2, what
    for what, status in null_cases(tdv, ctx._h, o):
        assert status == -2, what
    assert o.untouched()
    assert sample_call(tdv, False, ctx._h, o) == 0 and not o.untouched()          # ... and the good call it was all derived from runs


# ---------------------------------------------------------------- the even-spread model
@pytest.fixture(scope="module")
def relief(synth):
    return mesh_cases.relief(synth.ReliefPart(seed=3), 0.002)


@pytest.mark.parametrize("n_points", [64, 2048])
def test_mesh_model_is_the_composition(tdv, ctx, relief, n_points):
    v, t = relief
    px, pn, r = R.mesh_model(v, t, n_points, 8, seed=1)
    env = Env(ctx)
    ox, on = env.out(3 * n_points, F), env.out(3 * n_points, F)
    got = ctx.mesh_model_dev(env.up(v), len(v), env.up(t), len(t), n_points, ox.data_ptr(), on.data_ptr(), 8, 1)
    assert got["n_selected"] == n_points == r["n_selected"] and np.float32(got["cover_d2"]).tobytes() == np.float32(r["cover_d2"]).tobytes()
    assert env.get(ox, 3 * n_points, F).tobytes() == px.tobytes() and env.get(on, 3 * n_points, F).tobytes() == pn.tobytes()
    hx, hn, hr = ctx.mesh_model(v, t, n_points, 8, 1)
    assert hx.tobytes() == px.tobytes() and hn.tobytes() == pn.tobytes() and hr["n_selected"] == n_points
    sx, sn = ctx.sample_points_uniformly(v, t, 100, seed=1)
    first = R.sample(v, t, 100, seed=1)
    assert sx.tobytes() == first["xyz"].tobytes() and sn.tobytes() == first["normals"].tobytes()
    if n_points == tdv.TDV_PPF_MODEL_MAX:                                          # ... and the PPF model takes it as it stands
        import torch
        nbytes = ctx.ppf_model_bytes(n_points)
        table = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        info = ctx.ppf_model_dev(ox.data_ptr(), on.data_ptr(), n_points, table.data_ptr(), nbytes)
        assert info["n_pairs"] > 0 and info["diameter"] > 0.05 and info["nt"] == n_points
