"""The ICP loop's loads in flight together (csrc/icp.hip: grid_nearest, acc_fetch / acc_points): same bits as before.

grid_nearest issues a step's eight table probes resp. eight list nodes unconditionally - a finished probe reloads its slot, an ended or
empty list reads node[0] - and k_icp_accumulate / k_icp_accumulate_multi fetch a lane's four points, then their gathers, from clamped
indices before adding the accepted ones in point order.  What can go wrong is a dummy load that counts, a clamped point that counts, a
candidate skipped, or a sum out of order.  So: the grid search against the brute-force search of the same context (accepted flags of
every source; index and d2 of every accepted one, byte for byte; a rejected source reads "none" from the grid, index 0 and d2 FLT_MAX,
where the scan reports its nearest target beyond the threshold), and whole ICP calls against the exact-sum oracle resp. the restatements
as tests/test_gpu_tree_sums_exact.py, tests/test_gpu_icp_loss.py, tests/test_gpu_gicp.py and tests/test_gpu_colored_icp.py hold them:
T, rmse, fitness, iterations and n_corr as bytes, on inputs none of whose sums is ambiguous.  Every test runs on a Context of its own."""
import numpy as np
import pytest

import colored_icp_restatement as R
import gicp_restatement as G
import icp_loss_restatement as L
from test_gpu_colored_icp import _cicp_dev, _problem as _colored_problem
from test_gpu_gicp import _gicp_dev, _problem as _gicp_problem
from test_gpu_tree_sums_exact import _batch, _chain, _icp_dev, _oracle, _problem, _same

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
EYE = np.eye(4, dtype=F)
GRID_CELL_FACTOR = F(2.2)      # csrc/icp.hip
GRID_PAD = 16


@pytest.fixture
def lctx(tdv):
    c = tdv.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the grid, restated (csrc/icp.hip: grid_key, grid_slot, k_grid_insert)
def _inv_cell(thr):
    return F(1.0) / F(GRID_CELL_FACTOR * F(thr))


def _cell_coords(p, thr):
    """(cell index [n, 3] int64, fraction inside the cell [n, 3] f32) of points p in f32, as the kernels compute them."""
    g = (np.asarray(p, F) * _inv_cell(thr)).astype(F)
    k = np.floor(g)
    return k.astype(np.int64), (g - k).astype(F)


def _key(c):
    m = 0x1fffff
    return ((int(c[0]) & m) << 42) | ((int(c[1]) & m) << 21) | (int(c[2]) & m)


def _table(tgt, thr):
    """(home slot of a key -> slot function, occupied slots, keys present) of the targets' table.  Which key sits where depends on the
    order of the insertions, the SET of occupied slots of a linear-probing table does not."""
    size, log2 = 1024, 10
    while size < 2 * len(tgt):
        size, log2 = size << 1, log2 + 1
    home = lambda key: ((key * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> (64 - log2)   # noqa: E731
    keys = {_key(c) for c in _cell_coords(tgt, thr)[0]}
    occupied = set()
    for key in keys:
        s = home(key)
        while s in occupied:
            s += 1
        assert s <= size - 1 + GRID_PAD - 2
        occupied.add(s)
    return home, occupied, keys


def _queried_cells(src, thr):
    """The eight cells grid_nearest looks at for every point of src (poses here are the identity): keys [n][8]."""
    k, f = _cell_coords(src, thr)
    step = np.where(f < F(0.5), -1, 1)
    return [[_key(k[i] + step[i] * np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])) for c in range(8)] for i in range(len(src))]


# ---------------------------------------------------------------- grid against brute force
def _grid_equals_brute(ctx, src, tgt, thr, search="grid", T=EYE):
    """The accepted flags of every source, index and d2 of every accepted one; 'none' for the rest.  Returns the accepted mask."""
    ctx.set_icp_search("brute")
    ref = ctx.icp_correspondences(src, tgt, T, thr)
    ctx.set_icp_search(search)
    got = ctx.icp_correspondences(src, tgt, T, thr)
    assert ctx.last_icp_search() == search
    acc = ref["accepted"]
    assert np.array_equal(got["accepted"], acc) and got["n_corr"] == ref["n_corr"] == int(acc.sum())
    assert np.array_equal(got["corr"][acc], ref["corr"][acc])
    assert got["d2"][acc].tobytes() == ref["d2"][acc].tobytes()
    assert not got["corr"][~acc].any() and (got["d2"][~acc] == FLT_MAX).all()
    return acc


def _long_list_problem(thr=0.004, nt=3000, ns=1500, seed=3):
    """nt targets of which 40 groups of 2 to 9 share a cell each (an exact duplicate in every group, a triple in every third),
    the rest spread over 60^3 cells; ns sources, two thirds of them inside the groups' cells."""
    rng = np.random.default_rng(seed)
    cell = float(GRID_CELL_FACTOR * F(thr))
    groups, sizes = [], []
    for g in range(40):
        k = 2 + g % 8                                            # 2 .. 9 points
        centre = (rng.integers(-30, 30, 3) + 0.5) * cell
        pts = centre + rng.uniform(-0.3, 0.3, (k, 3)) * cell     # well inside the cell
        pts[1] = pts[0]                                          # an exact duplicate: the lower index wins
        if g % 3 == 0 and k >= 3:
            pts[k - 1] = pts[0]
        groups.append(pts); sizes.append(k)
    rest = rng.uniform(-30, 30, (nt - sum(sizes), 3)) * cell
    tgt = np.concatenate(groups + [rest]).astype(F)
    tgt = tgt[rng.permutation(nt)]
    near = np.concatenate(groups)[rng.integers(0, sum(sizes), 2 * ns // 3)] + rng.uniform(-0.4, 0.4, (2 * ns // 3, 3)) * thr
    other = tgt[rng.integers(0, nt, ns - len(near))] + rng.uniform(-0.8, 0.8, (ns - len(near), 3)) * thr
    return np.concatenate([near, other]).astype(F), tgt, sizes


def test_long_cell_lists(lctx):
    thr = 0.004
    src, tgt, sizes = _long_list_problem(thr)
    _, counts = np.unique(_cell_coords(tgt, thr)[0], axis=0, return_counts=True)
    assert counts.max() >= 9 and (counts >= 2).sum() >= 40 and {2, 3, 4, 5, 6, 7, 8, 9} <= set(counts.tolist())
    acc = _grid_equals_brute(lctx, src, tgt, thr)
    assert acc.sum() > len(src) // 2
    # the duplicates decide by index: some accepted source's nearest target has an exact copy at a higher index
    dup = {tuple(p) for p, c in zip(*np.unique(tgt, axis=0, return_counts=True)) if c > 1}
    lctx.set_icp_search("grid")
    got = lctx.icp_correspondences(src, tgt, EYE, thr)
    first = {tuple(p): i for i, p in reversed(list(enumerate(tgt)))}
    hits = [i for i in got["corr"][acc] if tuple(tgt[i]) in dup]
    assert len(hits) > 20 and all(first[tuple(tgt[i])] == i for i in hits)


def test_nothing_near(lctx, synth):
    """Every source more than two cells from any target: eight empty cells, every list load a dummy, 'none' for all."""
    thr = 0.004
    tgt, _ = synth.sample_object(2000, 5)
    src = (tgt[:1500] + F([0.0, 0.0, 1.0])).astype(F)            # the part is 0.1 m high: a metre above it
    _, _, keys = _table(tgt, thr)
    assert not any(k in keys for q in _queried_cells(src[:200], thr) for k in q)
    acc = _grid_equals_brute(lctx, src, tgt, thr)
    assert not acc.any()


def test_probe_runs_beyond_the_second_entry(lctx, synth):
    """synth.sample_object(4000, 7) at a threshold of 2 mm: 2,747 occupied cells in a table of 8,192 slots.  Of the 12,000 cells that the
    1,500 sources (targets moved by up to 0.8 thresholds per axis) query, 7,846 are absent from the table, and 1,365 of those hash to a
    slot that is occupied together with the next one - the probe of such a cell cannot end with its first load of two entries,
    wherever the insertions put the keys."""
    thr = 0.002
    tgt, _ = synth.sample_object(4000, 7)
    rng = np.random.default_rng(8)
    src = (tgt[rng.permutation(4000)[:1500]] + rng.uniform(-0.8, 0.8, (1500, 3)) * thr).astype(F)
    home, occupied, keys = _table(tgt, thr)
    assert 2000 <= len(keys) <= 4000
    beyond = sum(1 for q in _queried_cells(src, thr) for k in q if k not in keys and home(k) in occupied and home(k) + 1 in occupied)
    assert beyond >= 100, beyond
    acc = _grid_equals_brute(lctx, src, tgt, thr)
    assert 100 < acc.sum() < 1500


EDGE_NS = [1, 63, 255, 257, 1023, 1025, 4097]


@pytest.mark.parametrize("nt", [1, 127])
@pytest.mark.parametrize("search", ["grid", "pruned"])
def test_edge_sizes(lctx, orc, synth, search, nt):
    """Sizes at which a lane's four points straddle the end of the cloud: the correspondences against the brute-force search, and one
    fixed iteration against the exact-sum oracle.  (Point-to-point against a single target point is left to the correspondences: every
    q is that point, the centred cross-covariance cancels to rounding and the oracle reports its sums ambiguous.)"""
    thr = 0.02
    tgt, nrm = synth.sample_object(nt, 11)
    for ns in EDGE_NS:
        rng = np.random.default_rng(ns)
        src = (tgt[rng.integers(0, nt, ns)] + rng.uniform(-0.9, 0.9, (ns, 3)) * thr).astype(F)   # about two thirds within the threshold
        T0 = synth.perturb(EYE, seed=ns, angle_deg=1.0, trans=0.002).astype(F)
        acc = _grid_equals_brute(lctx, src, tgt, thr, search, T0)
        for p2plane in ((True,) if nt == 1 else (True, False)):
            ref = _oracle(orc, src, tgt, nrm, T0, thr, 1, p2plane, "nt %d ns %d" % (nt, ns))
            assert ref[4] == (int(acc.sum()) if ref[3] else 0)
            got = _icp_dev(lctx, src, tgt, nrm, T0, thr, 1, p2plane, True)
            assert lctx.last_icp_search() == search
            _same(got, ref, "%s nt %d ns %d p2plane %s" % (search, nt, ns, p2plane))


# ---------------------------------------------------------------- the accumulation tree: whole calls against the oracle
TREE_NS = [1025, 1279, 1793, 4097]     # tails after one, two, three or none of a block's four point rows
K = 3
ACCEPT = {   # nt, threshold, start pose off by (degrees, metres)
    "all": (127, 0.05, 0.5, 0.001),
    "mixed": (127, 0.02, 2.0, 0.003),
    "none": (127, 0.02, 0.0, 5.0),
}


def _tree_problem(synth, ns, accept):
    """(src, tgt, nrm, T0, thr); 'all': a scene without outliers under a threshold wider than the sparse target's spacing."""
    nt, thr, angle, trans = ACCEPT[accept]
    tgt, nrm = synth.sample_object(nt, ns + 100)
    src, T_gt = synth.make_scene(ns, ns + 100, outlier_frac=0.0 if accept == "all" else 0.10)
    T0 = synth.perturb(T_gt, seed=ns + 101, angle_deg=angle, trans=trans).astype(F)
    return src, tgt, nrm, T0, thr


@pytest.mark.parametrize("p2plane", [True, False])
@pytest.mark.parametrize("accept", list(ACCEPT))
@pytest.mark.parametrize("ns", TREE_NS)
def test_accumulation_tree(lctx, orc, synth, ns, accept, p2plane):
    """Three fixed iterations equal three chained one-iteration exact-sum oracle calls; nothing accepted keeps the start pose."""
    src, tgt, nrm, T0, thr = _tree_problem(synth, ns, accept)
    if accept == "all":                              # every source's nearest target within the threshold at the start pose
        assert orc.icp_correspondences(src, tgt, None, T0, thr, False)["accepted"].all()
    ref = _chain(orc, src, tgt, nrm, T0, thr, K, p2plane, "%s ns %d" % (accept, ns))
    assert (ref[3], ref[4] > 0) == ((0, False) if accept == "none" else (K, True))
    if accept == "mixed":
        assert 3 <= ref[4] < len(src)
    for search in ("grid", "pruned"):
        lctx.set_icp_search(search)
        got = _icp_dev(lctx, src, tgt, nrm, T0, thr, K, p2plane, True)
        assert lctx.last_icp_search() in ("grid", "pruned")
        _same(got, ref, "%s %s ns %d" % (search, accept, ns))


def _held(got, ref, what):
    assert not ref["ambiguous"], "%s: a sum of the restatement is ambiguous - pick another input" % what
    assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), (what, got.iterations, ref["iterations"], got.n_corr, ref["n_corr"])
    assert F(got.rmse).tobytes() == F(ref["rmse"]).tobytes() and F(got.fitness).tobytes() == F(ref["fitness"]).tobytes(), what
    assert got.transformation.tobytes() == ref["T"].tobytes(), (what, got.transformation, ref["T"])


def test_robust_loss(lctx, orc, synth):
    """Tukey at 10 mm, point-to-plane, 1,279 points: the weighted terms and n_eff through the grouped fetch."""
    src, tgt, nrm, T0 = _problem(synth, 1279, 127, seed=1379)
    ref = L.icp(orc, src, tgt, nrm, T0, 0.02, K, True, "tukey", 0.01, fixed=True)
    assert ref["iterations"] == K
    lctx.set_icp_loss("tukey", 0.01)
    for search in ("grid", "pruned"):
        lctx.set_icp_search(search)
        _held(_icp_dev(lctx, src, tgt, nrm, T0, 0.02, K, True, True), ref, "tukey " + search)
        assert lctx.last_icp_search() == search


def test_gicp(lctx, orc, synth):
    src, sn, tgt, nrm, T0 = _gicp_problem(orc, synth, 1279, 127, seed=1379)
    ref = G.gicp(orc, src, sn, tgt, nrm, T0, 0.02, K, fixed=True)
    assert ref["iterations"] == K
    for search in ("grid", "pruned"):
        lctx.set_icp_search(search)
        _held(_gicp_dev(lctx, src, sn, tgt, nrm, T0, 0.02, K, True), ref, "gicp " + search)
        assert lctx.last_icp_search() == search


def test_colored_icp(lctx, orc, synth):
    src, srgb, tgt, nrm, tc, T0 = _colored_problem(orc, synth, 1279, 127, seed=1379)
    ref = R.colored_icp(orc, src, srgb, tgt, nrm, tc, T0, 0.02, K, fixed=True)
    assert ref["iterations"] == K
    for search in ("grid", "pruned"):
        lctx.set_icp_search(search)
        _held(_cicp_dev(lctx, src, srgb, tgt, nrm, tc, T0, 0.02, K, True), ref, "colored " + search)
        assert lctx.last_icp_search() == search


@pytest.mark.parametrize("p2plane", [True, False])
def test_batch_of_unequal_instances(lctx, orc, synth, p2plane):
    """icp_batch_dev, three instances of 1,793, 300 and 1,025 points: k_icp_accumulate_multi's groups against the oracle."""
    tgt, nrm = synth.sample_object(127, 42)
    clouds, T0s = [], []
    for b, n in enumerate((1793, 300, 1025)):
        s, T_gt = synth.make_scene(n, 700 + b)
        clouds.append(s)
        T0s.append(synth.perturb(T_gt, seed=710 + b, angle_deg=2.0, trans=0.003))
    T0s = np.stack(T0s).astype(F)
    lctx.set_icp_search("grid")
    got = _batch(lctx, clouds, tgt, nrm, T0s, 0.02, K, p2plane, True)
    assert lctx.last_icp_search() == "grid"
    for b, c in enumerate(clouds):
        ref = _chain(orc, c, tgt, nrm, T0s[b], 0.02, K, p2plane, "instance %d" % b)
        assert ref[3] == K
        _same(got[b], ref, "instance %d (%d points)" % (b, len(c)))
