"""CPU suite: mesh sampling (include/tdv_hip.h: tdv_mesh_sample_points).  The ABI exports the entry points, lists them in ABI_SYMBOLS, has
the documented struct layout, constants and defaults, and refuses every bad argument before it writes anything.  The restatement
(tests/mesh_sample_restatement.py) is held to independent definitions: the weights in fractions.Fraction on the f32 areas, the selection
by a linear walk over prefix sums kept as Python integers, rule S5's integers on their edge values.  Then the properties the rules
promise: on a box every point lies on its face and every normal is the face's outward unit normal, the triangle and barycentric outputs
reproduce the point, the faces receive their share of the samples, triangles of weight zero are never chosen, and a sample depends on its
global index alone (S7).  No compute entry point of the library runs here; tests/test_gpu_mesh_sample.py holds the device to this
restatement byte for byte."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import mesh_cases
import mesh_sample_restatement as R

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_mesh_sample_default_params", "tdv_mesh_sample_points", "tdv_mesh_sample_points_dev")
NAN, INF = float("nan"), float("inf")


def test_symbols_constants_structs_and_defaults(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.MeshSampleParamsC) == 16
    assert [(k, getattr(tdv.MeshSampleParamsC, k).offset) for k, _ in tdv.MeshSampleParamsC._fields_] == [("seed", 0), ("first_sample", 8)]
    assert C.sizeof(tdv.MeshSampleResultC) == 32
    assert [(k, getattr(tdv.MeshSampleResultC, k).offset) for k, _ in tdv.MeshSampleResultC._fields_] == [
        ("n_usable", 0), ("n_degenerate", 4), ("n_bad", 8), ("n_sampled", 12), ("weight_exponent", 16), ("area_max", 20), ("total_weight", 24)]
    assert tuple(k for k, _ in tdv.MeshSampleResultC._fields_) == R.RESULT
    assert tdv.TDV_MESH_SAMPLE_MAX == R.SAMPLE_MAX == 1 << 24
    assert tdv.TDV_MESH_MAX_VERTICES == R.MAX_VERTICES and tdv.TDV_MESH_MAX_TRIANGLES == R.MAX_TRIANGLES
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tdv_hip.h")).read()
    for name in ("MESH_SAMPLE_MAX", "MESH_MAX_VERTICES", "MESH_MAX_TRIANGLES"):
        text = header.split("#define TDV_%s " % name)[1].split("/*")[0].split("\n")[0].strip()
        assert eval(text) == getattr(tdv, "TDV_" + name), (name, text)
    assert "key (seed, %d)" % R.KEY_TAG in header                                  # S4's tag, as the header words it
    p = tdv.mesh_sample_params()
    assert (p.seed, p.first_sample) == (R.DEFAULTS["seed"], R.DEFAULTS["first_sample"]) == (0, 0)
    lib.tdv_mesh_sample_default_params(None)                                       # a NULL is ignored
    q = tdv.mesh_sample_params(seed=7, first_sample=(1 << 40) + 3)
    assert (q.seed, q.first_sample) == (7, (1 << 40) + 3)
    with pytest.raises(TypeError):
        tdv.mesh_sample_params(start=1)


# ---------------------------------------------------------------- arguments
GOOD = dict(n_vertices=4, n_triangles=2, attr_width=3, n_samples=5, seed=0, first_sample=0)
BAD = [("null ctx", {}), ("n_vertices < 0", dict(n_vertices=-1)), ("n_vertices > 2^22", dict(n_vertices=R.MAX_VERTICES + 1)),
       ("n_triangles < 0", dict(n_triangles=-1)), ("n_triangles > 2^22", dict(n_triangles=R.MAX_TRIANGLES + 1)),
       ("n_samples < 0", dict(n_samples=-1)), ("n_samples > 2^24", dict(n_samples=R.SAMPLE_MAX + 1)),
       ("first_sample + n_samples wraps", dict(first_sample=(1 << 64) - 3, n_samples=4)), ("attr_width < 0", dict(attr_width=-1))]
NULLS = ("vertices", "triangles", "params", "result", "attr")                      # ("attr": attr_width > 0 with a NULL attr, and out_attr without attr)


class Outputs:
    """Every output of a call with room for n samples, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n=8, width=3, fill=0x5A):
        self.res = tdv.MeshSampleResultC(); C.memset(C.byref(self.res), fill, C.sizeof(self.res))
        self.xyz = np.full((n, 3), -7, F); self.normals = np.full((n, 3), -7, F); self.triangle = np.full(n, -7, np.int32)
        self.bary = np.full((n, 2), -7, F); self.attr = np.full((n, max(width, 1)), -7, F)
        self.before = self.snapshot()

    def snapshot(self):
        return (bytes(self.res),) + tuple(a.tobytes() for a in (self.xyz, self.normals, self.triangle, self.bary, self.attr))

    def untouched(self):
        return self.snapshot() == self.before


def P(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def inputs():
    return np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F), np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.ones((4, 3), F)


def sample_call(tdv, dev, ctx, o, null=(), skip=(), **kw):
    """Host arrays in every slot: a refused call must not look at them (the device entry point included).  skip: outputs passed as NULL."""
    g = dict(GOOD, **kw)
    vtx, tri, attr = inputs()
    prm = tdv.MeshSampleParamsC(g["seed"], g["first_sample"])
    fn = tdv.lib().tdv_mesh_sample_points_dev if dev else tdv.lib().tdv_mesh_sample_points
    return fn(ctx, None if "vertices" in null else P(vtx), g["n_vertices"], None if "triangles" in null else P(tri), g["n_triangles"],
              None if "attr" in null else P(attr), g["attr_width"], g["n_samples"], None if "params" in null else C.byref(prm),
              None if "result" in null else C.byref(o.res), P(o.xyz), P(o.normals), P(o.triangle), P(o.bary),
              None if "out_attr" in skip else P(o.attr))


def null_cases(tdv, ctx, o):
    """(what, status) of every refusal that is not a number's, host and device form."""
    for dev in (False, True):
        for what in NULLS:
            yield what, sample_call(tdv, dev, ctx, o, null=(what,))
        yield "out_attr without attr", sample_call(tdv, dev, ctx, o, null=("attr",), attr_width=0)


@pytest.mark.parametrize("case", range(len(BAD)))
def test_bad_arguments_leave_outputs_untouched(tdv, case):
    """A NULL ctx, alone and with each bad argument: TDV_ERR_BAD_ARG, every output byte for byte as it was.  A real ctx needs a device:
    tests/test_gpu_mesh_sample.py refuses each bad argument on one."""
    o = Outputs(tdv)
    for dev in (False, True):
        assert sample_call(tdv, dev, None, o, **BAD[case][1]) == TDV_ERR_BAD_ARG, BAD[case][0]
    assert o.untouched()


def test_null_pointers(tdv):
    o = Outputs(tdv, fill=0x33)
    for what, status in null_cases(tdv, None, o):
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()


# ---------------------------------------------------------------- the restatement against independent definitions
def odd_mesh(seed=5, m=40):
    """Random triangles of areas over several binades, with a repeated index (zero area), a bad index and a NaN vertex among them."""
    rng = np.random.default_rng(seed)
    v = (rng.random((3 * m, 3)) * np.repeat(2.0 ** rng.integers(-6, 3, m), 3)[:, None]).astype(F)
    t = np.arange(3 * m, dtype=np.int32).reshape(m, 3)
    t[7] = (3, 3, 4); t[11] = (0, len(v), 1); v[3 * 20 + 1, 2] = np.nan
    return v, t


def test_weights_against_fractions():
    v, t = odd_mesh()
    f = R.faces(v, t)
    w, e, area_max = R.weights(f["area"], f["bad"])
    assert f["bad"].sum() == 2 and f["bad"][11] and f["bad"][20] and not f["bad"][7] and f["area"][7] == 0
    assert Fraction(2) ** e <= Fraction(float(area_max)) < Fraction(2) ** (e + 1)
    assert area_max == max(a for a, b in zip(f["area"], f["bad"]) if not b)
    for a, b, wt in zip(f["area"], f["bad"], w):
        exact = Fraction(0) if b else Fraction(float(a)) * Fraction(2) ** (31 - e)
        assert int(wt) == exact.numerator // exact.denominator                     # truncated
        assert int(wt) < 2 ** 32
    assert int(w.max()) >= 2 ** 31
    s = R.sample(v, t, 10)
    assert s["total_weight"] == sum(int(x) for x in w) == int(s["C"][-1]) and s["weight_exponent"] == e
    assert (s["n_usable"], s["n_degenerate"], s["n_bad"]) == (37, 1, 2)
    assert s["surface_area"] == float(Fraction(s["total_weight"]) * Fraction(2) ** (e - 31))
    assert abs(s["surface_area"] - float(f["area"].astype(np.float64).sum())) < 40 * 2.0 ** (e - 31)      # a truncation per triangle


def test_selection_against_a_linear_walk():
    v, t = odd_mesh(seed=6)
    n, seed, first = 3000, 9, 12345
    s = R.sample(v, t, n, seed=seed, first_sample=first)
    w = [int(x) for x in s["w"]]
    W = sum(w)
    r, _, _ = R.draws(np.arange(first, first + n, dtype=np.uint64), seed)
    hit = set()
    for k in range(n):
        target = (r[k] * W) >> 64
        assert 0 <= target < W
        run, chosen = 0, None
        for j, wj in enumerate(w):
            run += wj
            if run > target:
                chosen = j
                break
        assert chosen == s["triangle"][k] and w[chosen] > 0, k
        hit.add(chosen)
    assert len(hit) >= 15 and not hit & {7, 11, 20}                                # (the areas span 18 binades: the small ones are rarely met)


def test_barycentric_integers_on_their_edges():
    top = R.ONE - 1                                                                # the largest x >> 8
    raw = [(0, 0), (0, top), (top, 0), (top, top), (1, top), (top, 1), (1 << 23, 1 << 23), ((1 << 23) + 1, 1 << 23), (5, R.ONE - 5),
           (R.ONE - 5, 6)]
    i1, i2 = R.reflect([a for a, _ in raw], [b for _, b in raw])
    assert ((i1 >= 0) & (i2 >= 0) & (i1 + i2 <= R.ONE)).all()
    assert (i1[3], i2[3]) == (1, 1) and (i1[4], i2[4]) == (1, top) and (i1[7], i2[7]) == ((1 << 23) - 1, 1 << 23)      # == 2^24 stays
    u, v, w = R.bary(i1, i2)
    for a, b, x, y, z in zip(i1, i2, u, v, w):
        assert Fraction(float(x)) == Fraction(int(a), R.ONE) and Fraction(float(y)) == Fraction(int(b), R.ONE)
        assert Fraction(float(z)) == Fraction(R.ONE - int(a) - int(b), R.ONE)
        assert Fraction(float(x)) + Fraction(float(y)) + Fraction(float(z)) == 1 and min(x, y, z) >= 0
    # over random draws the same, and in f32 arithmetic: (1 - u) - v is exact and is w
    rng = np.random.default_rng(1)
    i1, i2 = R.reflect(rng.integers(0, R.ONE, 100000), rng.integers(0, R.ONE, 100000))
    u, v, w = R.bary(i1, i2)
    assert (i1 + i2 <= R.ONE).all() and ((F(1) - u) - v).tobytes() == w.tobytes() and (w >= 0).all()


# ---------------------------------------------------------------- the properties, on a box
SIZE = (0.2, 0.12, 0.06)


@pytest.fixture(scope="module")
def box():
    v, t = mesh_cases.box(SIZE)
    out = R.sample(v, t, 20000, seed=1)
    return v, t, out


def test_box_points_lie_on_their_faces_and_inside(box):
    """A face of the box has one coordinate equal in its three vertices, +-h (h the half extent as f32).  (w*h + u*h) + v*h with
    u + v + w == 1 exactly: three products and two sums, every intermediate of magnitude at most h up to its own rounding, so five
    roundings of at most half an ulp of h each - 2.5 ulp(h) from the plane.  The other coordinates are convex combinations of values in
    [-h, h] with the same five roundings: inside the box within 2.5 ulp(h).  (The prototype left 9e-9 m, 1.2 ulp of 0.1.)"""
    v, t, out = box
    h = np.abs(v).max(0)
    assert np.allclose(h, np.array(SIZE) / 2, rtol=1e-6)
    bound = 2.5 * np.spacing(h).astype(np.float64)
    p = out["xyz"].astype(np.float64)
    assert (np.abs(p) <= h.astype(np.float64) + bound).all()
    f = R.faces(v, t)
    axis = np.argmax(np.abs(f["n"]), 1)[out["triangle"]]                           # the face's axis; its plane is at va[axis]
    plane = f["va"][out["triangle"], axis].astype(np.float64)
    off = np.abs(p[np.arange(len(p)), axis] - plane)
    print("largest distance from the face's plane: %.3e m (bound %.3e)" % (off.max(), bound.max()))
    assert (off <= bound[axis]).all()


def test_box_normals_are_unit_and_outward(box):
    v, t, out = box
    n = out["normals"].astype(np.float64)
    assert (np.abs(np.sqrt((n * n).sum(1)) - 1.0) <= 2 * 2.0 ** -23).all()
    assert ((n * out["xyz"].astype(np.float64)).sum(1) > 0).all()                  # the box is centred on the origin
    assert set(map(tuple, np.rint(n).astype(int).tolist())) == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}


def test_triangle_and_bary_reproduce_the_point(box):
    v, t, out = box
    u, w2 = out["bary"][:, 0], out["bary"][:, 1]
    w = (F(1) - u) - w2                                                            # exact
    a, b, c = (v[t[out["triangle"], k]] for k in range(3))
    again = (w[:, None] * a + u[:, None] * b) + w2[:, None] * c
    assert again.dtype == F and again.tobytes() == out["xyz"].tobytes()
    assert (u >= 0).all() and (w2 >= 0).all() and (w >= 0).all()


def test_uniform_over_the_faces():
    """20,000 samples at seeds 1 to 5: each face's count within 5 binomial standard deviations of n * w_t / W.  Deterministic; 5 sigma
    over 60 counts has a false-alarm chance near 4e-5 for a correct sampler (the prototype of the rules: at most 3.85)."""
    v, t = mesh_cases.box(SIZE)
    n, worst = 20000, 0.0
    for seed in range(1, 6):
        s = R.sample(v, t, n, seed=seed)
        p = s["w"].astype(np.float64) / float(s["total_weight"])
        got = np.bincount(s["triangle"], minlength=len(t))
        dev = np.abs(got - n * p) / np.sqrt(n * p * (1 - p))
        worst = max(worst, float(dev.max()))
        assert (dev <= 5.0).all(), (seed, dev)
    print("largest deviation over 5 seeds x 12 faces: %.2f sigma" % worst)
    # and inside a face the points spread over it: the two triangles of a rectangle, each coordinate's mean near the face's centre
    s = R.sample(v, t, n, seed=1)
    assert np.abs(s["xyz"].mean(0)).max() < 0.003


# ---------------------------------------------------------------- zero weights, and S7
def zero_weight_mesh():
    """Unit right triangles between zero-area ones (first, last, a run of three in the middle) and a sliver of 5e-12, below 2^-32 of 0.5."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1e-5, 0, 1], [0, 1e-6, 1], [2, 2, 2]], F)
    good, zero, line, sliver = (0, 1, 2), (6, 6, 6), (0, 1, 1), (3, 4, 5)
    t = np.array([zero, good, good, line, zero, line, good, sliver, good, zero], np.int32)
    return v, t, [1, 2, 6, 8]


def test_zero_weight_triangles_are_never_chosen():
    v, t, good = zero_weight_mesh()
    s = R.sample(v, t, 5000, seed=3)
    f = R.faces(v, t)
    assert 0 < f["area"][7] < 2.0 ** -33 and s["w"][7] == 0 and f["area"][1] == 0.5
    assert (s["n_usable"], s["n_degenerate"], s["n_bad"], s["n_sampled"]) == (4, 6, 0, 5000)
    assert s["total_weight"] == 4 << 31 and s["weight_exponent"] == -1 and s["surface_area"] == 2.0
    assert sorted(set(s["triangle"].tolist())) == good
    # nothing usable: no samples, whatever was asked for
    none = R.sample(v, t[[0, 3, 4]], 100)
    assert (none["n_usable"], none["n_degenerate"], none["n_sampled"], none["total_weight"], none["weight_exponent"]) == (0, 3, 0, 0, 0)
    assert len(none["xyz"]) == 0 and R.sample(v, t[:0], 100)["n_sampled"] == 0
    bad = R.sample(np.array([[0, 0, 0], [1e30, 0, 0], [0, 1e30, 0]], F), [(0, 1, 2), (0, 1, 3)], 10)          # the area overflows; an index past the end
    assert (bad["n_bad"], bad["n_usable"], bad["n_sampled"]) == (2, 0, 0)


def test_a_sample_depends_on_its_global_index_alone():
    v, t = odd_mesh(seed=8)
    attr = np.random.default_rng(2).random((len(v), 4)).astype(F)
    whole = R.sample(v, t, 700, attr, seed=4)
    a, b = R.sample(v, t, 300, attr, seed=4), R.sample(v, t, 400, attr, seed=4, first_sample=300)
    for k in R.OUTPUTS:
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes(), k
    assert whole["attr"].shape == (700, 4) and R.sample(v, t, 700, attr, seed=5)["xyz"].tobytes() != whole["xyz"].tobytes()
    # across 2^32 the counter's second word takes over: the rows there are not the rows at g - 2^32
    edge = (1 << 32) - 3
    over = R.sample(v, t, 10, seed=4, first_sample=edge)
    lo, hi = R.sample(v, t, 3, seed=4, first_sample=edge), R.sample(v, t, 7, seed=4, first_sample=1 << 32)
    assert np.concatenate([lo["xyz"], hi["xyz"]]).tobytes() == over["xyz"].tobytes()
    assert hi["xyz"].tobytes() != whole["xyz"][:7].tobytes()
    r_hi, _, _ = R.draws(np.array([1 << 32], np.uint64), 4)
    r_lo, _, _ = R.draws(np.array([0], np.uint64), 4)
    assert r_hi != r_lo
