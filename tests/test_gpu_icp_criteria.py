"""The convergence criteria of an ICP level (include/tdv_hip.h: tdv_icp_level.relative_fitness, relative_rmse; csrc/icp.hip: icp_update,
init_states, run_flags) on every ICP path, against the references under the same bounds (tests/icp_criteria_cases.py, which builds and
asserts the fixtures on the CPU).  A schedule of one level with the clouds as given reaches the paths through multi_scale_icp_dev and
multi_scale_icp_batch_dev; the sizes and the ctx's switches choose the kernel:

  small/tree, small/reference     700 x 370, AUTO: the whole loop in k_icp_small (no query tells it from the two launches; the size rule
                                  is small_fits')
  brute/tree, brute/reference     TDV_ICP_SMALL=0, BRUTE: k_icp_nn_scan + k_icp_accumulate resp. k_icp_fold_ref
  pruned                          k_icp_nn_pruned + k_icp_accumulate
  grid/two, grid/one, grid/one+cache    k_icp_nn_grid + k_icp_accumulate, k_icp_iterate without and with the probe cache

Per case the bounds land the stop on iterations 2, 4, 5, 12 and 13 (run_bursts looks at the state after 4 and after 12), on the f32
difference itself (no stop: the rule is <) and one ulp above it (stop), where only the fitness term binds, where both are finite and
the rmse term alone would stop earlier, never ((inf, 0): max_iterations), and at the defaults ((inf, 1e-6) and (FLT_MAX, 1e-6): the
bytes of icp_dev / gicp_dev).  Point-to-plane and reference-order sums are the reference's bytes; point-to-point under tree sums takes
test_gpu_icp_loss.py's pose tolerance and nothing else.  All tree-sum paths of a case return the same bytes."""
import numpy as np
import pytest

import icp_criteria_cases as K
from state_cases import Env

pytestmark = pytest.mark.gpu
F = np.float32
M, MB = K.M, K.MB
# name: search, TDV_ICP_SMALL, launches, probe cache, accumulation, what last_icp_search / last_icp_launches report
PATHS = {
    "small/tree": ("auto", None, "auto", "auto", "tree", "brute", "two"),
    "small/reference": ("auto", None, "auto", "auto", "reference", "brute", "two"),
    "brute/tree": ("brute", "0", "auto", "auto", "tree", "brute", "two"),
    "brute/reference": ("brute", "0", "auto", "auto", "reference", "brute", "two"),
    "pruned": ("pruned", None, "auto", "auto", "tree", "pruned", "two"),
    "grid/two": ("grid", None, "two", "off", "tree", "grid", "two"),
    "grid/one": ("grid", None, "one", "off", "tree", "grid", "one"),
    "grid/one+cache": ("grid", None, "one", "on", "tree", "grid", "one"),
}
TREE = [p for p in PATHS if PATHS[p][4] == "tree"]


@pytest.fixture
def cctx(tdv, monkeypatch):
    c = tdv.Context(0)
    yield c, monkeypatch
    c.close()


def _set_path(ctx, mp, path, loss="l2"):
    search, small, launches, cache, accumulate, _, _ = PATHS[path]
    ctx.set_icp_search(search); ctx.set_icp_launches(launches); ctx.set_icp_probe_cache(cache); ctx.set_icp_accumulation(accumulate)
    ctx.set_icp_loss(loss, K.LOSSES.get(loss))
    if small is None:
        mp.delenv("TDV_ICP_SMALL", raising=False)
    else:
        mp.setenv("TDV_ICP_SMALL", small)


def _key(r):
    return (r.transformation.tobytes(), F(r.rmse).tobytes(), F(r.fitness).tobytes(), int(r.iterations), int(r.n_corr))


def _against(got, ref, exact_pose, synth, what):
    assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), (what, got.iterations, ref["iterations"], got.n_corr, ref["n_corr"])
    assert F(got.rmse).tobytes() == F(ref["rmse"]).tobytes(), (what, got.rmse, ref["rmse"])
    assert F(got.fitness).tobytes() == F(ref["fitness"]).tobytes(), (what, got.fitness, ref["fitness"])
    if exact_pose:
        assert got.transformation.tobytes() == ref["T"].tobytes(), (what, got.transformation, ref["T"])
    else:
        ang, tr = synth.pose_error(got.transformation, ref["T"])
        assert ang <= 1e-4 and tr <= 1e-6, (what, ang, tr)


def _single(tdv, ctx, mp, orc, synth, name, estimation, paths, loss="l2"):
    """Every run of the case on every path: the reference's result, the path the ctx reports, one result over the tree-sum paths."""
    s = K.scene(orc, name)
    ns, nt = len(s["src"]), len(s["tgt"])
    env = Env(ctx)
    ps, psn, pt, pn = env.up(s["src"]), env.up(s["sn"]), env.up(s["tgt"]), env.up(s["nrm"])
    est = "point_to_plane" if estimation == "plane_without_normals" else estimation
    d_nrm = None if estimation == "plane_without_normals" else pn
    d_sn = psn if estimation == "gicp" else None
    p2point = estimation in ("point_to_point", "plane_without_normals")
    by_run = {}
    for path in paths:
        accumulate, search, launches = PATHS[path][4], PATHS[path][5], PATHS[path][6]
        if estimation == "gicp":
            launches = "two"          # the one-launch iteration is point-to-plane's and point-to-point's (icp_plan)
        _set_path(ctx, mp, path, loss)
        c = K.case(orc, name, estimation, loss, accumulate)
        stops = []
        for label, rf, rr, want, ref in c["runs"]:
            got = ctx.multi_scale_icp_dev(ps, ns, pt, d_nrm, nt, s["T0"], estimation=est, d_src_normals=d_sn,
                                          levels=tdv.icp_levels([None], [s["thr"]], [M], rf, rr)).levels[0]
            what = (name, estimation, loss, path, label, rf, rr)
            assert (ctx.last_icp_search(), ctx.last_icp_launches()) == (search, launches), (what, ctx.last_icp_search(), ctx.last_icp_launches())
            if path == "grid/one+cache":
                assert ctx.last_icp_probe_misses() >= ns, (what, ctx.last_icp_probe_misses())
            else:
                assert ctx.last_icp_probe_misses() == -1, (what, ctx.last_icp_probe_misses())
            assert (got.ns, got.nt) == (ns, nt)
            stops.append(got.iterations)
            _against(got, ref, not (p2point and accumulate == "tree"), synth, what)
            assert got.iterations == want, (what, got.iterations, want)
            if accumulate == "tree":
                by_run.setdefault(label, {})[path] = _key(got)
            if label.startswith("default"):          # the defaults are the entry points that have no criteria, on the same ctx
                if estimation == "gicp":
                    plain = ctx.gicp_dev(ps, psn, ns, pt, pn, nt, s["T0"], s["thr"], M)
                else:
                    plain = ctx.icp_dev(ps, ns, pt, d_nrm, nt, s["T0"], s["thr"], M, est == "point_to_plane")
                assert _key(got) == _key(plain), what
        print("%s %s %s %s: reach %s, stops %s" % (name, estimation, loss, path, c["reach"], stops))
        if estimation == "point_to_plane" and loss == "l2":
            assert set(K.KS) <= set(stops), (name, path, stops)
    for label, keys in by_run.items():
        assert len(set(keys.values())) == 1, (name, estimation, loss, label, "tree-sum paths differ", sorted(keys))


SINGLE = [("small", e, list(PATHS)) for e in ("point_to_plane", "point_to_point", "plane_without_normals")] + \
         [("mid", "point_to_plane", [p for p in PATHS if not p.startswith("small")])] + \
         [("large", e, [p for p in PATHS if not p.startswith("small")]) for e in ("point_to_plane", "point_to_point", "plane_without_normals")]


@pytest.mark.parametrize("name,estimation,paths", SINGLE, ids=["%s-%s" % (n, e) for n, e, _ in SINGLE])
def test_single_call_stops_where_the_reference_does(tdv, cctx, orc, synth, name, estimation, paths):
    ctx, mp = cctx
    _single(tdv, ctx, mp, orc, synth, name, estimation, paths)


@pytest.mark.parametrize("name", ["small", "large"])
def test_gicp_stops_where_the_restatement_does(tdv, cctx, orc, synth, name):
    ctx, mp = cctx
    paths = [p for p in TREE if not p.startswith("grid/one") and (name == "small" or not p.startswith("small"))]
    _single(tdv, ctx, mp, orc, synth, name, "gicp", paths)


@pytest.mark.parametrize("loss", list(K.LOSSES))
def test_robust_losses_stop_where_the_restatement_does(tdv, cctx, orc, synth, loss):
    ctx, mp = cctx
    _single(tdv, ctx, mp, orc, synth, "small", "point_to_plane", ["small/tree", "grid/one", "grid/two"], loss)


# ---------------------------------------------------------------- the three branches of icp_batch_run_dev
# name: scene (its target), the real instances' sizes, search, accumulation, what last_icp_search reports (None: per instance, the last one's)
BATCHES = {
    "small batch/tree": ("mid", (700, 300, 513), "auto", "tree", "brute"),            # (1) icp_small_batch_dev: every cloud and the target <= 2,048
    "small batch/reference": ("mid", (700, 300, 513), "auto", "reference", "brute"),
    "together": ("large", (2049, 700, 1025), "grid", "tree", "grid"),                 # (2) k_icp_nn_grid_multi + k_icp_accumulate_multi
    "per instance/reference": ("large", (2049, 700, 1025), "grid", "reference", "grid"),      # (3) icp_run_dev per instance
    "per instance/pruned": ("large", (2049, 700, 1025), "pruned", "tree", "pruned"),
}


@pytest.mark.parametrize("branch", list(BATCHES))
def test_batch_instances_stop_where_the_reference_does(tdv, cctx, orc, synth, branch):
    ctx, mp = cctx
    name, sizes, search, accumulate, reports = BATCHES[branch]
    mp.delenv("TDV_ICP_SMALL", raising=False)
    ctx.set_icp_search(search); ctx.set_icp_accumulation(accumulate)
    s = K.scene(orc, name)
    b = K.batch_case(orc, name, sizes, accumulate)
    assert 2 in b["stops"] and MB in b["stops"] and len(set(b["stops"])) == len(sizes) >= 3, b["stops"]      # (on the oracle alone)
    off = np.concatenate([[0], np.cumsum([len(c) for c in b["clouds"]])]).astype(np.int32)
    env = Env(ctx)
    pt, pn, nt = env.up(s["tgt"]), env.up(s["nrm"]), len(s["tgt"])
    lv = tdv.icp_levels([None], [s["thr"]], [MB], b["rf"], b["rr"])
    got = ctx.multi_scale_icp_batch_dev(env.up(np.concatenate(b["clouds"])), off, pt, pn, nt, b["T0s"], levels=lv)
    assert ctx.last_icp_search() == reports, (branch, ctx.last_icp_search())
    assert len(got) == len(b["clouds"])
    print(branch, "bounds", b["rf"], b["rr"], "stops", [g.iterations for g in got])
    for i, (cloud, ref) in enumerate(zip(b["clouds"], b["refs"])):
        one = ctx.multi_scale_icp_dev(env.up(cloud), len(cloud), pt, pn, nt, b["T0s"][i], levels=lv)
        assert _key(got[i]) == _key(one) and (got[i].levels[0].ns, got[i].levels[0].nt) == (len(cloud), nt), (branch, "instance", i)
        if ref is None:          # no points, and one point: n_corr < 3 at the first iteration
            assert got[i].iterations == 0 and got[i].transformation.tobytes() == b["T0s"][i].tobytes(), (branch, i)
        else:
            _against(got[i], ref, True, synth, (branch, "instance", i))
    assert [g.iterations for g in got[2:]] == b["stops"]
