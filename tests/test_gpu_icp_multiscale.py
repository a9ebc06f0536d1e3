"""Multi-scale ICP (include/tdv_hip.h: tdv_icp_multiscale) on the device.

The scene: synth.sample_object(3000, 42) as the model with its analytic normals, synth.make_scene(3000, 100 + seed) as the scan, started
6 deg / 10 mm off the ground truth (synth.perturb(T_gt, seed=200 + seed, angle_deg=6.0, trans=0.01)).  With sp = synth.mean_spacing(3000)
= 5.61 mm the schedule is (voxel, distance, iterations) = (4 sp, 8 sp, 20), (2 sp, 3 sp, 20), (as given, 0.4 sp, 50).  Its coarse levels
(about 350 / 192 and 1,000 / 711 points) fall under the 2,048-point one-launch loop (k_icp_small), its last level (3,000 x 3,000) does
not: one call crosses both kernel families.

* chain equality: per level the one call returns, in bits, what the stagewise public calls return on the same ctx - voxel_downsample_normals_dev
  (FIRST) of source and target, then icp_dev / gicp_dev from the level before's pose;
* the batch is per instance the single call, over clouds of 0, 1, 700, 2,049 and 3,000 points (the 1-point cloud takes the n_corr < 3 break);
* the oracle anchor: under reference-order sums every level is orc.icp on the level's clouds, in bits; under tree sums it is
  orc.icp(exact=True) wherever that is not flagged ambiguous;
* what the schedule buys is a property of the fixture, asserted on the oracle alone (so that it cannot hide a device failure): from the
  6 deg / 10 mm start the oracle's single-scale error is at least 10x its three-level error on seeds 1 and 3 (measured: 16-17x);
* the convergence criteria stop where the recorded per-iteration (fitness, rmse) say they must (test_gpu_icp_criteria.py holds them to the
  references on every ICP path);
* every refused call writes nothing;
* a batched voxel level says which way it went (tdv_ctx_last_voxel_batch_redone): clouds planted with at most 16 points in every voxel keep
  the batched table - the NRM kernels under GICP - and one voxel of 17 points in one instance has the level redone cloud by cloud; either
  way every instance is the single call, and one flipped source normal changes the GICP level's bytes;
* robust loss, launch form and probe cache apply at every level as they do to the stagewise calls, and last_icp_launches /
  last_icp_probe_misses report the last level;
* NaN, +-inf and far-out rows of the source and of its normals go through the schedule as through the stagewise chain, and under
  reference-order sums as through the oracle's own voxel grid and ICP."""
import ctypes as C

import numpy as np
import pytest

from state_cases import Env
from test_gpu_voxel_normals import unit

pytestmark = pytest.mark.gpu
F = np.float32
N = 3000
BAD_ARG = -2


def schedule(synth):
    sp = synth.mean_spacing(N)
    return [(F(4 * sp), F(8 * sp), 20), (F(2 * sp), F(3 * sp), 20), (None, F(0.4 * sp), 50)]


@pytest.fixture(scope="module")
def scene(tdv, synth):
    """Model, scans of seeds 1 and 3, their starts; the scan's normals (GICP) from the library's own estimator.  Never modified."""
    tgt, nrm = synth.sample_object(N, 42)
    S = dict(tgt=tgt, nrm=nrm, sched=schedule(synth))
    c = tdv.Context(0)
    try:
        for seed in (1, 3):
            src, T_gt = synth.make_scene(N, 100 + seed)
            S[seed] = dict(src=src, T_gt=T_gt, T0=synth.perturb(T_gt, seed=200 + seed, angle_deg=6.0, trans=0.01), sn=c.estimate_normals(src, 30))
    finally:
        c.close()
    for v in (tgt, nrm, S[1]["src"], S[1]["sn"], S[3]["src"], S[3]["sn"]):
        v.setflags(write=False)
    return S


def bits(r):
    out = (r.transformation.tobytes(), F(r.fitness).tobytes(), F(r.rmse).tobytes(), int(r.iterations), int(r.n_corr))
    return out + ((int(r.ns), int(r.nt)) if hasattr(r, "ns") else ())


def levels_of(tdv, sched, **kw):
    return tdv.icp_levels([v for v, _, _ in sched], [d for _, d, _ in sched], [it for _, _, it in sched], **kw)


class Settings:
    def __init__(self, ctx, search="auto", accumulate="tree"):
        self.ctx, self.search, self.accumulate = ctx, search, accumulate

    def __enter__(self):
        self.ctx.set_icp_search(self.search); self.ctx.set_icp_accumulation(self.accumulate)

    def __exit__(self, *a):
        self.ctx.set_icp_search("auto"); self.ctx.set_icp_accumulation("tree")


def stagewise(ctx, env, src, sn, tgt, nrm, T0, sched, estimation):
    """The chain of public calls: per level (result bits + point counts, the level's host clouds)."""
    gicp = estimation == "gicp"
    ps, pt = env.up(src), env.up(tgt)
    psn = env.up(sn) if gicp else None
    ptn = env.up(nrm) if nrm is not None else None
    T = T0
    out = []
    for voxel, dist, iters in sched:
        if voxel is not None:
            osx, osn = env.out(3 * len(src), F), env.out(3 * len(src), F)
            otx, otn = env.out(3 * len(tgt), F), env.out(3 * len(tgt), F)
            ns = ctx.voxel_downsample_normals_dev(ps, psn, len(src), voxel, osx.data_ptr(), osn.data_ptr() if gicp else None, len(src))
            nt = ctx.voxel_downsample_normals_dev(pt, ptn, len(tgt), voxel, otx.data_ptr(), otn.data_ptr() if ptn else None, len(tgt))
            a = (osx.data_ptr(), osn.data_ptr() if gicp else None, ns, otx.data_ptr(), otn.data_ptr() if ptn else None, nt)
            clouds = (env.get(osx, 3 * ns, F).reshape(-1, 3), env.get(otx, 3 * nt, F).reshape(-1, 3),
                      env.get(otn, 3 * nt, F).reshape(-1, 3) if ptn else None)
        else:
            a = (ps, psn, len(src), pt, ptn, len(tgt))
            clouds = (src, tgt, nrm)
        if gicp:
            r = ctx.gicp_dev(a[0], a[1], a[2], a[3], a[4], a[5], T, dist, iters)
        else:
            r = ctx.icp_dev(a[0], a[2], a[3], a[4], a[5], T, dist, iters, estimation == "point_to_plane")
        out.append((bits(r) + (a[2], a[5]), clouds, T))
        T = r.transformation
    return out


CHAIN = [(e, acc, s) for e in ("point_to_plane", "point_to_point", "plane_without_normals") for acc in ("tree", "reference") for s in ("auto", "grid")] + \
        [("gicp", "tree", s) for s in ("auto", "grid")]


@pytest.mark.parametrize("estimation,accumulate,search", CHAIN)
def test_single_call_is_the_stagewise_chain(tdv, ctx, scene, estimation, accumulate, search):
    p = scene[1]
    nrm = None if estimation == "plane_without_normals" else scene["nrm"]
    est = "point_to_plane" if estimation == "plane_without_normals" else estimation
    env = Env(ctx)
    with Settings(ctx, search, accumulate):
        chain = stagewise(ctx, env, p["src"], p["sn"], scene["tgt"], nrm, p["T0"], scene["sched"], est)
        got = ctx.multi_scale_icp_dev(env.up(p["src"]), N, env.up(scene["tgt"]), None if nrm is None else env.up(nrm), N, p["T0"], estimation=est,
                                      d_src_normals=env.up(p["sn"]) if est == "gicp" else None, levels=levels_of(tdv, scene["sched"]))
        host = ctx.multi_scale_icp(p["src"], scene["tgt"], None, None, p["T0"], estimation=est, target_normals=nrm,
                                   source_normals=p["sn"] if est == "gicp" else None, levels=levels_of(tdv, scene["sched"]))
    assert len(got.levels) == 3
    for l, (lv, (ref, _, _)) in enumerate(zip(got.levels, chain)):
        assert bits(lv) == ref, (estimation, accumulate, search, "level", l, lv, ref[1:])
        assert bits(host.levels[l]) == ref, (estimation, accumulate, search, "host, level", l)
    assert bits(got) == bits(got.levels[-1])[:5]
    # the call crosses both kernel families, and every level iterated
    assert got.levels[0].ns < 2048 and got.levels[1].ns < 2048 and got.levels[0].nt < 2048 and got.levels[2].ns == N and got.levels[2].nt == N
    assert 300 <= got.levels[0].ns <= 400 and 150 <= got.levels[0].nt <= 250 and 900 <= got.levels[1].ns <= 1100 and 650 <= got.levels[1].nt <= 800
    assert all(lv.iterations >= 2 for lv in got.levels), [lv.iterations for lv in got.levels]


SIZES = (0, 1, 700, 2049, 3000)


@pytest.mark.parametrize("estimation,accumulate", [("point_to_plane", "tree"), ("point_to_plane", "reference"), ("gicp", "tree")])
def test_batch_is_the_single_call_per_instance(tdv, ctx, scene, estimation, accumulate):
    p = scene[1]
    gicp = estimation == "gicp"
    src = np.concatenate([p["src"][:n] for n in SIZES]); sn = np.concatenate([p["sn"][:n] for n in SIZES])
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    T0s = np.stack([p["T0"]] * len(SIZES))
    env = Env(ctx)
    pt, ptn = env.up(scene["tgt"]), env.up(scene["nrm"])
    with Settings(ctx, "auto", accumulate):
        got = ctx.multi_scale_icp_batch_dev(env.up(src), off, pt, ptn, N, T0s, estimation=estimation, d_src_normals=env.up(sn) if gicp else None,
                                            levels=levels_of(tdv, scene["sched"]))
        assert len(got) == len(SIZES)
        for b, n in enumerate(SIZES):
            one = ctx.multi_scale_icp_dev(env.up(p["src"][:n]), n, pt, ptn, N, p["T0"], estimation=estimation,
                                          d_src_normals=env.up(p["sn"][:n]) if gicp else None, levels=levels_of(tdv, scene["sched"]))
            assert [bits(l) for l in got[b].levels] == [bits(l) for l in one.levels], (estimation, accumulate, "instance", b, n)
    # the empty cloud and the one that collapses below 3 voxels: no level applies an iteration, the start pose is passed on unchanged
    for b in (0, 1):
        for l, lv in enumerate(got[b].levels):
            assert lv.transformation.tobytes() == p["T0"].astype(F).tobytes() and lv.iterations == 0 and lv.n_corr == 0 and lv.fitness == 0 and lv.rmse == 0
            assert lv.ns == SIZES[b] and lv.nt == got[4].levels[l].nt
    assert got[3].levels[2].ns == 2049 and got[3].levels[0].ns < 2048 and all(lv.iterations >= 2 for lv in got[4].levels)
    # the host-cloud form makes the offsets itself
    with Settings(ctx, "auto", accumulate):
        host = ctx.multi_scale_icp_batch([p["src"][:n] for n in SIZES], scene["tgt"].copy(), None, None, T0s, estimation=estimation, target_normals=scene["nrm"].copy(),
                                         source_normals=[p["sn"][:n] for n in SIZES] if gicp else None, levels=levels_of(tdv, scene["sched"]))
    assert [[bits(l) for l in r.levels] for r in host] == [[bits(l) for l in r.levels] for r in got]


@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
@pytest.mark.parametrize("accumulate", ["reference", "tree"])
def test_levels_against_the_oracle(tdv, ctx, orc, scene, estimation, accumulate):
    p = scene[1]
    env = Env(ctx)
    with Settings(ctx, "auto", accumulate):
        chain = stagewise(ctx, env, p["src"], p["sn"], scene["tgt"], scene["nrm"], p["T0"], scene["sched"], estimation)
        got = ctx.multi_scale_icp_dev(env.up(p["src"]), N, env.up(scene["tgt"]), env.up(scene["nrm"]), N, p["T0"], estimation=estimation,
                                      levels=levels_of(tdv, scene["sched"]))
    held = 0
    for l, (lv, (_, (s_l, t_l, n_l), T_in), (_, dist, iters)) in enumerate(zip(got.levels, chain, scene["sched"])):
        ref = orc.icp(s_l, t_l, n_l, T_in, dist, iters, estimation == "point_to_plane", exact=accumulate == "tree")
        if accumulate == "tree" and ref["ambiguous"]:
            continue
        held += 1
        assert (lv.transformation.tobytes(), F(lv.fitness).tobytes(), F(lv.rmse).tobytes(), lv.iterations) == \
               (ref["T"].tobytes(), F(ref["fitness"]).tobytes(), F(ref["rmse"]).tobytes(), ref["iterations"]), (estimation, accumulate, "level", l)
    assert held == 3 if accumulate == "reference" else held >= 1, held


def _oracle_first_order(orc, pts, nrm, voxel):
    x, m, first = orc.voxel_downsample(pts, nrm, voxel)
    perm = np.argsort(first, kind="stable")
    return x[perm], (None if m is None else unit(m[perm]))


@pytest.mark.parametrize("seed", [1, 3])
def test_what_the_schedule_buys_on_the_oracle(orc, synth, scene, seed):
    p = scene[seed]
    sched = scene["sched"]
    single = orc.icp(p["src"], scene["tgt"], scene["nrm"], p["T0"], sched[-1][1], sched[-1][2], True)
    T = p["T0"]
    for voxel, dist, iters in sched:
        s_l, t_l, n_l = (p["src"], scene["tgt"], scene["nrm"]) if voxel is None else \
            (_oracle_first_order(orc, p["src"], None, voxel)[0],) + _oracle_first_order(orc, scene["tgt"], scene["nrm"], voxel)
        r = orc.icp(s_l, t_l, n_l, T, dist, iters, True)
        T = r["T"] if r["iterations"] > 0 else T
    (a1, t1), (a3, t3) = synth.pose_error(single["T"], p["T_gt"]), synth.pose_error(T, p["T_gt"])
    print("seed %d: single scale %.2e rad %.3f mm, three levels %.2e rad %.3f mm" % (seed, a1, 1e3 * t1, a3, 1e3 * t3))
    assert a3 < 1e-3 and t3 < 1e-3, (a3, t3)
    assert a1 >= 10 * a3 or t1 >= 10 * t3, ((a1, t1), (a3, t3))


# ---------------------------------------------------------------- the convergence criteria
M = 9


def _stop(obs, rel_fitness, rel_rmse):
    """The iteration count the rule gives on the recorded (fitness, rmse) of iterations 1 .. M (obs[k - 1]): the first k >= 2 with both
    differences below their bounds, else M."""
    for k in range(2, len(obs) + 1):
        if abs(F(obs[k - 2][0]) - F(obs[k - 1][0])) < rel_fitness and abs(F(obs[k - 2][1]) - F(obs[k - 1][1])) < rel_rmse:
            return k
    return len(obs)


def test_criteria_stop_where_the_recorded_iterations_say(tdv, ctx, scene):
    p = scene[1]
    voxel, dist, _ = scene["sched"][1]
    env = Env(ctx)
    ps, pt, ptn = env.up(p["src"]), env.up(scene["tgt"]), env.up(scene["nrm"])

    def run(iters, rf, rr):
        r = ctx.multi_scale_icp_dev(ps, N, pt, ptn, N, p["T0"], levels=tdv.icp_levels([voxel], [dist], [iters], rf, rr))
        return r.levels[0]
    runs = [run(k, float("inf"), 0.0) for k in range(1, M + 1)]                   # relative_rmse 0: the rule never fires
    assert [r.iterations for r in runs] == list(range(1, M + 1))
    obs = [(r.fitness, r.rmse) for r in runs]
    d_fit = [abs(F(a[0]) - F(b[0])) for a, b in zip(obs[:-1], obs[1:])]
    d_rmse = [abs(F(a[1]) - F(b[1])) for a, b in zip(obs[:-1], obs[1:])]
    print("fitness differences", d_fit); print("rmse differences", d_rmse)
    default = _stop(obs, float("inf"), F(1e-6))
    assert bits(run(M, float("inf"), 1e-6)) == bits(runs[default - 1]), "the default criteria are not the reference's rule"

    def pick(diffs, fitness_binds):
        for a, b in zip(diffs[:-1], diffs[1:]):
            if a > b > 0 or a > b == 0:
                bound = float(np.sqrt(float(a) * float(b))) if b > 0 else float(a) / 2          # strictly between the two differences
                k = _stop(obs, bound, float("inf")) if fitness_binds else _stop(obs, float("inf"), bound)
                if 2 < k < M - 1 and k != default:
                    return bound, k
        return None
    # the rmse term binds
    found = pick(d_rmse, False)
    assert found, "no rmse bound with a stop strictly inside 2 .. M - 1 that differs from the default's"
    rr, k = found
    got = run(M, float("inf"), rr)
    assert got.iterations == k and bits(got) == bits(runs[k - 1]), (got.iterations, k, rr)
    # the fitness term binds: with relative_rmse = +inf the rmse term alone would stop at the second iteration
    found = pick(d_fit, True)
    assert found, "no fitness bound with a stop strictly inside 2 .. M - 1 that differs from the default's"
    rf, k = found
    assert _stop(obs, float("inf"), float("inf")) == 2 != k
    got = run(M, rf, float("inf"))
    assert got.iterations == k and bits(got) == bits(runs[k - 1]), (got.iterations, k, rf)


# ---------------------------------------------------------------- refused calls write nothing
def test_bad_arguments_write_nothing(tdv, ctx, scene, synth):
    lib = tdv.lib()
    p = scene[1]
    env = Env(ctx)
    ps, psn, pt, ptn = env.up(p["src"]), env.up(p["sn"]), env.up(scene["tgt"]), env.up(scene["nrm"])
    sp = synth.mean_spacing(N)
    T0 = (C.c_float * 16)(*tdv.to_colmajor16(p["T0"]))
    off = (C.c_int * 2)(0, N)
    nan, inf = float("nan"), float("inf")
    good = dict(voxel_sizes=[4 * sp, 2 * sp, None], max_correspondence_distances=[8 * sp, 3 * sp, 0.4 * sp], max_iterations=5)

    def refused(levels, n_levels, estimation=0, src_normals=psn, what=""):
        out = (tdv.IcpLevelResultC * 16)(); C.memset(out, 0x5A, C.sizeof(out)); before = bytes(out)
        v = C.c_void_p
        st = [lib.tdv_icp_multiscale_dev(ctx._h, v(ps), v(src_normals), N, v(pt), v(ptn), N, T0, levels, n_levels, estimation, C.c_float(1e-3), out),
              lib.tdv_icp_multiscale_batch_dev(ctx._h, v(ps), v(src_normals), off, 1, v(pt), v(ptn), N, T0, levels, n_levels, estimation, C.c_float(1e-3), out),
              lib.tdv_icp_multiscale(ctx._h, v(p["src"].ctypes.data), v(p["sn"].ctypes.data if src_normals else None), N, v(scene["tgt"].ctypes.data),
                                     v(scene["nrm"].ctypes.data), N, T0, levels, n_levels, estimation, C.c_float(1e-3), out)]
        assert st == [BAD_ARG] * 3, (what, st)
        assert bytes(out) == before, what

    lv = tdv.icp_levels(**good)
    refused(lv, 0, what="no levels")
    refused(tdv.icp_levels([(10 - i) * sp for i in range(9)], 8 * sp, 5), 9, what="nine levels")
    refused(None, 3, what="NULL levels")
    refused(tdv.icp_levels([2 * sp, 2 * sp, None], **{k: good[k] for k in good if k != "voxel_sizes"}), 3, what="voxel sizes that do not decrease")
    refused(tdv.icp_levels([2 * sp, 4 * sp, None], **{k: good[k] for k in good if k != "voxel_sizes"}), 3, what="voxel sizes that grow")
    refused(tdv.icp_levels([4 * sp, None, sp], **{k: good[k] for k in good if k != "voxel_sizes"}), 3, what="a non-last level as given")
    refused(tdv.icp_levels([4 * sp, 0.0, None], **{k: good[k] for k in good if k != "voxel_sizes"}), 3, what="a non-last level with voxel 0")
    refused(tdv.icp_levels([4 * sp, 2 * sp, nan], **{k: good[k] for k in good if k != "voxel_sizes"}), 3, what="a NaN voxel")
    for d in (0.0, -0.01, nan, inf):
        refused(tdv.icp_levels(good["voxel_sizes"], [8 * sp, d, 0.4 * sp], 5), 3, what="distance %r" % d)
    refused(tdv.icp_levels(good["voxel_sizes"], good["max_correspondence_distances"], [5, -1, 5]), 3, what="negative iterations")
    for rf, rr in ((-1.0, 1e-6), (0.0, 1e-6), (nan, 1e-6), (inf, -1e-6), (inf, nan)):
        refused(tdv.icp_levels(relative_fitness=[inf, rf, inf], relative_rmse=[1e-6, rr, 1e-6], **good), 3, what="criteria %r %r" % (rf, rr))
    refused(lv, 3, estimation=2, what="an unknown estimation")
    refused(lv, 3, estimation=tdv.TDV_ICP_GICP, src_normals=None, what="GICP without source normals")
    with Settings(ctx, "auto", "reference"):
        refused(lv, 3, estimation=tdv.TDV_ICP_GICP, what="GICP under reference-order sums")
        ctx.set_icp_loss("huber", 0.002)
        try:
            refused(lv, 3, what="a robust loss under reference-order sums")
        finally:
            ctx.set_icp_loss("l2")
    # ... and the schedule itself is accepted
    out = (tdv.IcpLevelResultC * 3)()
    assert lib.tdv_icp_multiscale_dev(ctx._h, C.c_void_p(ps), None, N, C.c_void_p(pt), C.c_void_p(ptn), N, T0, lv, 3, 0, C.c_float(1e-3), out) == 0
    assert out[2].ns == N and out[2].icp.iterations > 0
    # an empty batch, and a target without points: as tdv_icp_batch_dev
    assert lib.tdv_icp_multiscale_batch_dev(ctx._h, None, None, None, 0, C.c_void_p(pt), C.c_void_p(ptn), N, None, lv, 3, 0, C.c_float(1e-3), None) == 0
    r = ctx.multi_scale_icp_dev(ps, N, None, None, 0, p["T0"], levels=lv)
    assert all(l.iterations == 0 and l.nt == 0 and l.transformation.tobytes() == p["T0"].astype(F).tobytes() for l in r.levels)
    assert [l.ns for l in r.levels][2] == N


# ---------------------------------------------------------------- which way the batched voxel level went
PLANT_SIZES = (0, 1, 1025, 1300)          # back to back the third crosses point 1,024 and the fourth point 2,048 (the voxel kernels' tiles)
ROW = 16                                  # member slots of a voxel in the batched table (csrc/voxel.hip: VH_K)


def _f32_keys(pts, voxel):
    return np.floor(pts * F(F(1.0) / F(voxel))).astype(np.int64)


def _voxel_counts(pts, voxel):
    return np.unique(_f32_keys(pts, voxel), axis=0, return_counts=True)[1] if len(pts) else np.zeros(0, np.int64)


def _planted(pool, voxel, n, fullest, rng):
    """n points of the pool with 1 .. ROW points in every voxel but the first, which gets `fullest`: shuffled."""
    keys = _f32_keys(pool, voxel)
    _, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    rich = [v for v in np.argsort(-cnt, kind="stable") if cnt[v] >= fullest]
    assert rich, "no voxel of the pool holds %d points" % fullest
    take, left = [], n
    for j, v in enumerate([rich[0]] + [v for v in rng.permutation(len(cnt)) if v != rich[0]]):
        k = fullest if j == 0 else int(min(cnt[v], 1 + (j % ROW), left))
        k = min(k, left)
        take.append(np.flatnonzero(inv == v)[:k]); left -= k
        if left == 0:
            break
    assert left == 0, "the pool is too small for %d points" % n
    idx = np.concatenate(take)
    return pool[idx[rng.permutation(len(idx))]].copy()


@pytest.fixture(scope="module")
def planted(orc, synth, scene):
    """Schedules A and B of one voxelised level plus the final one over clouds planted from a 20,000-point scan: in A every voxel of every
    instance holds at most 16 points (one holds exactly 16), in B exactly one voxel of the 1,025-point instance holds 17.  Asserted on the
    f32 keys; the source normals (GICP) are the oracle's estimates."""
    sp = synth.mean_spacing(N)
    voxel = F(4 * sp)
    pool, T_gt = synth.make_scene(20000, 77)
    T0 = synth.perturb(T_gt, seed=78, angle_deg=3.0, trans=0.005).astype(F)
    out = dict(sched=[(voxel, F(8 * sp), 12), (None, F(1.5 * sp), 12)], T0=T0, voxel=voxel)
    for name, fullest in (("A", ROW), ("B", ROW + 1)):
        rng = np.random.default_rng(5)
        clouds = [pool[:0], pool[7:8].copy(), _planted(pool, voxel, 1025, fullest, rng), _planted(pool[10000:], voxel, 1300, ROW, rng)]
        counts = [_voxel_counts(c, voxel) for c in clouds]
        over = [int((c > ROW).sum()) for c in counts]
        assert [len(c) for c in clouds] == list(PLANT_SIZES)
        assert over == ([0, 0, 0, 0] if name == "A" else [0, 0, 1, 0]) and max(int(c.max()) for c in counts[1:]) == fullest, (name, over)
        normals = [np.zeros((0, 3), F), F([[0, 0, 1]])] + [np.asarray(orc.estimate_normals(c), F) for c in clouds[2:]]
        out[name] = dict(clouds=clouds, normals=normals, off=np.concatenate([[0], np.cumsum(PLANT_SIZES)]).astype(np.int32))
    return out


@pytest.mark.parametrize("estimation", ["gicp", "point_to_plane"])
def test_batched_voxel_level_reports_which_way_it_went(tdv, orc, scene, planted, estimation):
    gicp = estimation == "gicp"
    ctx = tdv.Context(0)
    try:
        assert ctx.last_voxel_batch_redone() == -1          # before any call
        env = Env(ctx)
        pt, ptn = env.up(scene["tgt"]), env.up(scene["nrm"])
        lv = levels_of(tdv, planted["sched"])
        T0s = np.stack([planted["T0"]] * len(PLANT_SIZES))
        for name, redone in (("A", 0), ("B", 1), ("A", 0)):
            p = planted[name]
            src, sn = np.concatenate(p["clouds"]), np.concatenate(p["normals"])
            got = ctx.multi_scale_icp_batch_dev(env.up(src), p["off"], pt, ptn, N, T0s, estimation=estimation, d_src_normals=env.up(sn) if gicp else None, levels=lv)
            assert ctx.last_voxel_batch_redone() == redone, (name, ctx.last_voxel_batch_redone())
            for b, (c, n) in enumerate(zip(p["clouds"], p["normals"])):
                one = ctx.multi_scale_icp_dev(env.up(c), len(c), pt, ptn, N, planted["T0"], estimation=estimation, d_src_normals=env.up(n) if gicp else None, levels=lv)
                assert ctx.last_voxel_batch_redone() == redone          # the single call has no batched voxel pass: the query keeps the batch's answer
                assert [bits(l) for l in got[b].levels] == [bits(l) for l in one.levels], (estimation, name, "instance", b)
                assert got[b].levels[0].ns == len(_voxel_counts(c, planted["voxel"])) and got[b].levels[1].ns == len(c), (name, b)
            assert all(lv_.iterations >= 2 for b in (2, 3) for lv_ in got[b].levels), name
            # the voxel stage alone, on the same clouds, goes the same way
            o = env.out(3 * len(src), F)
            voff = ctx.voxel_downsample_batch_dev(env.up(src), p["off"], float(planted["voxel"]), o.data_ptr())
            assert ctx.last_voxel_batch_redone() == redone, (name, "voxel_downsample_batch_dev")
            assert list(np.diff(voff)) == [lv_.ns for lv_ in (got[b].levels[0] for b in range(len(PLANT_SIZES)))]
    finally:
        ctx.close()


def test_a_flipped_source_normal_changes_the_gicp_level(tdv, ctx, scene, planted):
    """The GICP fixture does read the source normals of its voxelised level: one flipped normal changes that level's bytes."""
    p = planted["A"]
    env = Env(ctx)
    pt, ptn = env.up(scene["tgt"]), env.up(scene["nrm"])
    lv = levels_of(tdv, planted["sched"])
    c, n = p["clouds"][2], p["normals"][2]
    keys = _f32_keys(c, planted["voxel"])
    i = next(i for i in range(len(c)) if 2 <= (keys == keys[i]).all(1).sum() <= 4 and np.abs(n[i]).max() > 0)      # a voxel of a few points: its mean normal turns
    flipped = n.copy(); flipped[i] = -n[i]
    runs = [ctx.multi_scale_icp_dev(env.up(c), len(c), pt, ptn, N, planted["T0"], estimation="gicp", d_src_normals=env.up(m), levels=lv) for m in (n, n, flipped)]
    assert bits(runs[0].levels[0]) == bits(runs[1].levels[0])
    assert bits(runs[0].levels[0]) != bits(runs[2].levels[0])
    assert runs[0].levels[0].ns == runs[2].levels[0].ns


# ---------------------------------------------------------------- the ctx's settings apply at every level
LEVEL_SETTINGS = {          # what is set on the ctx, and what the queries report after the call (its last level, 3,000 x 3,000 through the grid)
    "huber": dict(loss=("huber", 0.002), launches="two", misses=False),
    "tukey": dict(loss=("tukey", 0.004), launches="two", misses=False),
    "launches one": dict(set_launches="one", launches="one", misses=True),          # (AUTO takes the cache with the one-launch iteration)
    "launches two": dict(set_launches="two", launches="two", misses=False),
    "probe cache on": dict(cache="on", launches="two", misses=True),
    "probe cache off": dict(set_launches="one", cache="off", launches="one", misses=False),
}


@pytest.mark.parametrize("setting", list(LEVEL_SETTINGS))
def test_levels_run_under_the_ctx_settings(tdv, scene, setting):
    """Robust loss, launch form and probe cache through the three-level schedule with the grid search: every level is the stagewise chain
    on the same ctx, and last_icp_launches / last_icp_probe_misses report the last level."""
    p, cfg = scene[1], LEVEL_SETTINGS[setting]
    ctx = tdv.Context(0)
    try:
        ctx.set_icp_search("grid")
        if "loss" in cfg:
            ctx.set_icp_loss(*cfg["loss"])
        ctx.set_icp_launches(cfg.get("set_launches", "auto")); ctx.set_icp_probe_cache(cfg.get("cache", "auto"))
        env = Env(ctx)
        chain = stagewise(ctx, env, p["src"], p["sn"], scene["tgt"], scene["nrm"], p["T0"], scene["sched"], "point_to_plane")
        got = ctx.multi_scale_icp_dev(env.up(p["src"]), N, env.up(scene["tgt"]), env.up(scene["nrm"]), N, p["T0"], levels=levels_of(tdv, scene["sched"]))
        assert (ctx.last_icp_search(), ctx.last_icp_launches()) == ("grid", cfg["launches"]), (setting, ctx.last_icp_search(), ctx.last_icp_launches())
        misses = ctx.last_icp_probe_misses()
        assert (misses >= got.levels[-1].ns) if cfg["misses"] else (misses == -1), (setting, misses)
        for l, (lv, (ref, _, _)) in enumerate(zip(got.levels, chain)):
            assert bits(lv) == ref, (setting, "level", l, lv, ref[1:])
        assert all(lv.iterations >= 2 for lv in got.levels), [lv.iterations for lv in got.levels]
        if "loss" in cfg:          # the loss does weigh: the same schedule without it ends elsewhere
            ctx.set_icp_loss("l2")
            plain = ctx.multi_scale_icp_dev(env.up(p["src"]), N, env.up(scene["tgt"]), env.up(scene["nrm"]), N, p["T0"], levels=levels_of(tdv, scene["sched"]))
            assert bits(plain.levels[0]) != bits(got.levels[0])
    finally:
        ctx.close()


POISON_ROWS = [0, 5, 17, 62, 63, 64, 100, 640, 1023, 1024]          # test_gpu_icp_probe_cache.py: test_non_finite_and_far_out_sources_in_a_wave
POISON_VALS = [np.nan, np.inf, -np.inf, 3e7, -3e7, 1e19, -1e19, np.nan, np.inf, 2e3]


def _poisoned(a):
    a = a.copy()
    for k, (r, v) in enumerate(zip(POISON_ROWS, POISON_VALS)):
        a[r, k % 3] = F(v)
    return a


@pytest.mark.parametrize("estimation,accumulate", [("point_to_plane", "reference"), ("point_to_plane", "tree"), ("gicp", "tree")])
def test_non_finite_rows_through_the_schedule(tdv, ctx, orc, scene, estimation, accumulate):
    """NaN, +-inf and far-out coordinates in rows of the source (and, GICP, of its normals) through the three levels: each level is the
    stagewise chain, and under reference-order sums it is orc.icp on the oracle's own voxel clouds, whose sizes are the level's ns, nt."""
    p = scene[1]
    gicp = estimation == "gicp"
    src, sn = _poisoned(p["src"]), (_poisoned(p["sn"]) if gicp else p["sn"])
    env = Env(ctx)
    with Settings(ctx, "auto", accumulate):
        chain = stagewise(ctx, env, src, sn, scene["tgt"], scene["nrm"], p["T0"], scene["sched"], estimation)
        got = ctx.multi_scale_icp_dev(env.up(src), N, env.up(scene["tgt"]), env.up(scene["nrm"]), N, p["T0"], estimation=estimation,
                                      d_src_normals=env.up(sn) if gicp else None, levels=levels_of(tdv, scene["sched"]))
    for l, (lv, (ref, _, _)) in enumerate(zip(got.levels, chain)):
        assert bits(lv) == ref, (estimation, accumulate, "level", l, lv, ref[1:])
    assert all(lv.iterations >= 2 and lv.n_corr > 100 for lv in got.levels), [(lv.iterations, lv.n_corr) for lv in got.levels]      # the finite rest did register
    T = p["T0"]
    for l, (lv, (voxel, dist, iters)) in enumerate(zip(got.levels, scene["sched"])):
        s_l, t_l, n_l = (src, scene["tgt"], scene["nrm"]) if voxel is None else \
            (_oracle_first_order(orc, src, None, voxel)[0],) + _oracle_first_order(orc, scene["tgt"], scene["nrm"], voxel)
        assert (lv.ns, lv.nt) == (len(s_l), len(t_l)), (estimation, "level", l, lv.ns, len(s_l), lv.nt, len(t_l))
        if accumulate == "reference":
            r = orc.icp(s_l, t_l, n_l, T, dist, iters, True)
            assert (lv.transformation.tobytes(), F(lv.fitness).tobytes(), F(lv.rmse).tobytes(), lv.iterations) == \
                   (r["T"].tobytes(), F(r["fitness"]).tobytes(), F(r["rmse"]).tobytes(), r["iterations"]), (estimation, "level", l)
            T = r["T"] if r["iterations"] > 0 else T
