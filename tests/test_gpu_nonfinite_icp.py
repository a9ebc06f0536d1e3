"""Robust-loss ICP, GICP and the multi-instance batches on poisoned input (NaN, +-inf, 1e19 coordinates, NaN / infinite / 1e20
normals, NaN and infinite start poses), against the restatements and against the single calls.  tests/test_gpu_nonfinite.py holds
the stages and single-problem L2 ICP to the oracle; its conventions hold here: NaN positions equal, every other value byte for byte.

A correspondence with a non-finite term enters the sums as the header says, (double)w * term: a zero weight on an infinite term is
NaN, and an f64 tree of terms with an infinity is that infinity (pyoracle.exact_sum gives the same, in any order).

Batches: (a) every instance equals its single call, (b) every clean instance equals the same batch with the poisoned instances
replaced by clean ones, (c) the search the batch reports does not change with the poison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gicp_restatement as G
import icp_loss_restatement as R
from test_gpu_nonfinite import ICP_KINDS, NEG_NAN, _icp_problem, _poison_icp, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PATHS = {   # search mode, TDV_ICP_SMALL (tests/test_gpu_icp_loss.py)
    "small": ("auto", None),
    "brute": ("brute", "0"),
    "pruned": ("pruned", None),
    "grid": ("grid", None),
}
LOSSES = {"huber": 0.004, "tukey": 0.008, "cauchy": 0.004}
GICP_LOSSES = {"l2": 0.0, "huber": 0.05, "tukey": 0.1, "cauchy": 0.05}
GICP_KINDS = ICP_KINDS + ["snrm_nan", "snrm_inf", "snrm_huge"]


@pytest.fixture
def pctx(tdv, monkeypatch):
    c = tdv.Context(0)
    yield c, monkeypatch
    c.close()


def _up(a):
    a = np.ascontiguousarray(a, F).reshape(-1)
    t = torch.zeros(max(a.size, 3), dtype=torch.float32, device=DEV)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a).to(DEV))
    return t, t.data_ptr()


def _set_path(ctx, mp, path):
    search, small = PATHS[path]
    ctx.set_icp_search(search)
    if small is None:
        mp.delenv("TDV_ICP_SMALL", raising=False)
    else:
        mp.setenv("TDV_ICP_SMALL", small)


def _key(r):
    """A result's bytes; NaN entries of T as one pattern (the device's own NaNs are compared with the device's)."""
    T = np.where(np.isnan(r.transformation), F(np.nan), r.transformation).astype(F)
    return (T.tobytes(), np.float32(r.rmse).tobytes(), np.float32(r.fitness).tobytes(), r.iterations, r.n_corr)


def _against(got, ref, exact_pose, synth, what):
    """The device result against a restatement's: iterations, n_corr, rmse, fitness exact; T byte for byte (NaN positions equal)
    when exact_pose, else NaN positions equal and 1e-4 rad / 1e-6 m.  False (nothing asserted) when a sum of ref is ambiguous."""
    if exact_pose and ref["ambiguous"]:
        return False
    assert (got.iterations, got.n_corr) == (ref["iterations"], ref["n_corr"]), (what, got.iterations, ref["iterations"], got.n_corr, ref["n_corr"])
    _same(np.float32(got.rmse), ref["rmse"], what); _same(np.float32(got.fitness), ref["fitness"], what)
    if exact_pose:
        _same(got.transformation, ref["T"], what)
    else:
        assert np.array_equal(np.isnan(got.transformation), np.isnan(ref["T"])), what
        if not np.isnan(ref["T"]).any():
            ang, tr = synth.pose_error(got.transformation, ref["T"])
            assert ang <= 1e-4 and tr <= 1e-6, (what, ang, tr)
    return True


# ---------------------------------------------------------------- robust-loss ICP
@pytest.mark.parametrize("kind", ICP_KINDS)
@pytest.mark.parametrize("p2plane", [True, False])
def test_icp_loss_poisoned(pctx, orc, synth, kind, p2plane):
    """Huber, Tukey and Cauchy on every search path, free-running and fixed, against tests/icp_loss_restatement.py."""
    ctx, mp = pctx
    src, tgt, nrm, T0 = _icp_problem(synth, 1500, 1200, 9)
    src, tgt, nrm = _poison_icp(src, tgt, nrm, kind, np.random.default_rng(1))
    thr, iters = 0.004, 8
    ks, ps = _up(src); kt, pt = _up(tgt); kn, pn = _up(nrm)
    held = 0
    for loss, scale in LOSSES.items():
        ctx.set_icp_loss(loss, scale)
        for fixed in (False, True):
            ref = R.icp(orc, src, tgt, nrm, T0, thr, iters, p2plane, loss, scale, fixed)
            for path in PATHS:
                _set_path(ctx, mp, path)
                got = ctx.icp_dev(ps, len(src), pt, pn if p2plane else None, len(tgt), T0, thr, iters, p2plane, fixed_iterations=fixed)
                held += _against(got, ref, p2plane, synth, (kind, loss, fixed, path))
    assert held >= 12, "%s: too many restated sums are ambiguous" % kind


def test_nonfinite_residual_weights_enter_the_sums(pctx, orc, synth):
    """An infinite normal on the accepted correspondences: Tukey's weight there is 0, and 0 * inf is NaN in the sums, so the step is
    NaN (include/tdv_hip.h, the loss block); the restatement says so too, and so does an infinite J * J under L2 with 1e20 normals."""
    ctx, _ = pctx
    src, tgt, nrm, T0 = _icp_problem(synth, 1500, 1200, 9)
    ks, ps = _up(src); kt, pt = _up(tgt)
    c = orc.icp_correspondences(src, tgt, None, T0, 0.004, False)
    hit = np.unique(c["corr"][c["accepted"].astype(bool)])[:5]
    for loss, val in (("tukey", np.inf), ("l2", 1e20)):
        bad = nrm.copy()
        bad[hit, 2] = np.float32(val)                       # (z: no sum of these two cases is ambiguous)
        ctx.set_icp_loss(loss, LOSSES.get(loss, 0.0))
        ref = R.icp(orc, src, tgt, bad, T0, 0.004, 1, True, loss, LOSSES.get(loss, 0.0))
        assert np.isnan(ref["T"]).all() or np.isnan(ref["T"][:3]).any(), loss
        kn, pn = _up(bad)
        got = ctx.icp_dev(ps, len(src), pt, pn, len(tgt), T0, 0.004, 1, True)
        assert _against(got, ref, True, synth, loss)


# ---------------------------------------------------------------- GICP
def _src_normals(orc, src, kind, rng):
    sn = np.asarray(orc.estimate_normals(src), F).copy()
    rows = np.unique(np.concatenate([[0, len(src) - 1], rng.choice(len(src), 20, replace=False)]))
    if kind == "snrm_nan":
        sn[rows] = NEG_NAN
    elif kind == "snrm_inf":
        sn[rows, rng.integers(0, 3, len(rows))] = np.inf
    elif kind == "snrm_huge":
        sn[rows, rng.integers(0, 3, len(rows))] = 1e19
    return sn


@pytest.mark.parametrize("kind", GICP_KINDS)
def test_gicp_poisoned(pctx, orc, synth, kind):
    """GICP under L2 and the three losses, every search path, free-running and fixed, against tests/gicp_restatement.py."""
    ctx, mp = pctx
    src, tgt, nrm, T0 = _icp_problem(synth, 1200, 1000, 9)
    rng = np.random.default_rng(2)
    if kind.startswith("snrm"):
        sn = _src_normals(orc, src, kind, rng)
    else:
        sn = _src_normals(orc, src, "clean", rng)
        src, tgt, nrm = _poison_icp(src, tgt, nrm, kind, np.random.default_rng(1))
    thr, iters = 0.004, 6
    ks, ps = _up(src); kq, pq = _up(sn); kt, pt = _up(tgt); kn, pn = _up(nrm)
    held = 0
    for loss, scale in GICP_LOSSES.items():
        ctx.set_icp_loss(loss, scale)
        for fixed in (False, True):
            ref = G.gicp(orc, src, sn, tgt, nrm, T0, thr, iters, kind=loss, scale=scale, fixed=fixed)
            for path in PATHS:
                _set_path(ctx, mp, path)
                got = ctx.gicp_dev(ps, pq, len(src), pt, pn, len(tgt), T0, thr, iters, G.EPSILON, fixed)
                held += _against(got, ref, True, synth, (kind, loss, fixed, path))
    assert held >= 16, "%s: too many restated sums are ambiguous" % kind


# ---------------------------------------------------------------- batch isolation
# regimes of tests/test_gpu_icp_loss.py::test_batch_one_iteration: search mode, instance sizes, model size, fixed options
REGIMES = {
    "multi": ("grid", [3, 64, 257, 0, 1025, 2049, 4097, 255, 1500], 6000, (False, True)),
    "small_batch": ("auto", [3, 64, 257, 0, 1025, 2048, 255, 300, 700], 500, (False,)),
    "fallback_pruned": ("pruned", [3, 64, 257, 0, 1025, 2049, 4097, 255, 1500], 6000, (False, True)),
    "fallback_brute_fixed": ("brute", [3, 64, 257, 0, 1025, 2049, 4097, 255, 1500], 6000, (True,)),
}
POISONED = (1, 2, 4, 5, 6)     # 1: NaN rows, 2: all NaN, 4: +-inf / 1e19 rows, 5: NaN in T0, 6: inf in T0 (8: GICP NaN normals)


def _batch_instances(synth, sizes, seed=300):
    clouds, T0s = [], []
    for b, n in enumerate(sizes):
        src, T_gt = synth.make_scene(max(n, 1), seed + b)
        clouds.append(src[:n].copy())
        T0s.append(synth.perturb(T_gt, seed=seed + 100 + b, angle_deg=2.0, trans=0.003))
    return clouds, np.stack(T0s).astype(F)


def _poison_batch(clouds, T0s):
    clouds = [c.copy() for c in clouds]; T0s = T0s.copy()
    clouds[1][::3, 1] = NEG_NAN; clouds[1][0] = np.nan
    clouds[2][:] = np.nan
    c4 = clouds[4]
    c4[0, 0] = np.inf; c4[len(c4) - 1, 2] = -np.inf; c4[255] = 1e19; c4[256, 1] = -np.inf; c4[::50, 2] = 1e19
    T0s[5][1, 3] = np.nan
    T0s[6][0, 0] = np.inf; T0s[6][2, 3] = -np.inf
    return clouds, T0s


def _cat(clouds, normals=None):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    cat = np.concatenate(clouds).astype(F)
    return cat, (np.concatenate(normals).astype(F) if normals is not None else None), off


def _isolation(ctx, run_batch, run_single, clean, poisoned, poisoned_ids, what):
    """(a) instance == single call, (b) clean instances unchanged by the poison, (c) same search reported."""
    ref = run_batch(*clean)
    search_clean = ctx.last_icp_search()
    got = run_batch(*poisoned)
    assert ctx.last_icp_search() == search_clean, (what, ctx.last_icp_search(), search_clean)
    for b in range(len(got)):
        single = run_single(poisoned, b)
        if single is not None:
            assert _key(got[b]) == _key(single), (what, "instance %d against its single call" % b)
        if b not in poisoned_ids:
            assert _key(got[b]) == _key(ref[b]), (what, "clean instance %d changed by its neighbours' poison" % b)
    assert any(np.isnan(got[b].transformation).any() or got[b].iterations == 0 for b in poisoned_ids), what
    return got


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("setting", ["tree_l2", "reference_l2", "tree_tukey", "tree_huber_point"])
def test_icp_batch_isolation(pctx, synth, regime, setting):
    ctx, _ = pctx
    search, sizes, nt, fixeds = REGIMES[regime]
    ctx.set_icp_search(search)
    p2plane = setting != "tree_huber_point"
    if setting.startswith("reference"):
        ctx.set_icp_accumulation("reference")
    if setting in ("tree_tukey", "tree_huber_point"):
        ctx.set_icp_loss(setting.split("_")[1], LOSSES[setting.split("_")[1]])
    tgt, nrm = synth.sample_object(nt, 42)
    clean_c, clean_T = _batch_instances(synth, sizes)
    bad_c, bad_T = _poison_batch(clean_c, clean_T)
    kt, pt = _up(tgt); kn, pn = _up(nrm)
    keep = []

    def run_batch(clouds, T0s, fixed):
        cat, _, off = _cat(clouds)
        k, p = _up(cat); keep.append(k)
        return ctx.icp_batch_dev(p, off, pt, pn if p2plane else None, nt, T0s, 0.004, 10, p2plane, fixed)

    def run_single(inp, b):
        clouds, T0s, fixed = inp
        if len(clouds[b]) == 0:
            return None
        k, p = _up(clouds[b]); keep.append(k)
        return ctx.icp_dev(p, len(clouds[b]), pt, pn if p2plane else None, nt, T0s[b], 0.004, 10, p2plane, fixed_iterations=fixed)

    for fixed in fixeds:
        _isolation(ctx, run_batch, run_single, (clean_c, clean_T, fixed), (bad_c, bad_T, fixed), POISONED, (regime, setting, fixed))
    if regime == "multi" and setting == "tree_l2":          # a poisoned shared model: NaN and infinite rows, infinite normals
        rng = np.random.default_rng(5)
        rows = rng.choice(nt, 300, replace=False)
        tgt2, nrm2 = tgt.copy(), nrm.copy()
        tgt2[rows[:100]] = np.nan; tgt2[rows[100:200], 0] = np.inf; nrm2[rows[200:], 1] = -np.inf
        kt, pt = _up(tgt2); kn, pn = _up(nrm2)
        for fixed in fixeds:
            got = run_batch(bad_c, bad_T, fixed)
            for b in range(len(got)):
                single = run_single((bad_c, bad_T, fixed), b)
                if single is not None:
                    assert _key(got[b]) == _key(single), ("poisoned model", b, fixed)


GICP_REGIMES = {
    "multi": ("grid", [3, 300, 20000, 0, 2049, 1500, 700, 255, 900], 6000, (False, True)),
    "small": ("auto", [3, 300, 0, 2048, 1500, 255, 700, 64, 900], 500, (False,)),
    "fallback_brute": ("brute", [3, 300, 20000, 0, 2049, 1500, 700, 255, 900], 6000, (False, True)),
}


@pytest.mark.parametrize("regime", list(GICP_REGIMES))
@pytest.mark.parametrize("loss", ["l2", "tukey"])
def test_gicp_batch_isolation(pctx, orc, synth, regime, loss):
    ctx, _ = pctx
    search, sizes, nt, fixeds = GICP_REGIMES[regime]
    ctx.set_icp_search(search)
    ctx.set_icp_loss(loss, GICP_LOSSES[loss])
    tgt, nrm = synth.sample_object(nt, 42)
    clean_c, clean_T = _batch_instances(synth, sizes, seed=800)
    clean_n = [np.asarray(orc.estimate_normals(c), F) if len(c) > 30 else np.tile(F([0, 0, 1]), (len(c), 1)) for c in clean_c]
    bad_c, bad_T = _poison_batch(clean_c, clean_T)
    bad_n = [n.copy() for n in clean_n]
    bad_n[8][::4] = NEG_NAN
    kt, pt = _up(tgt); kn, pn = _up(nrm)
    keep = []

    def run_batch(clouds, normals, T0s, fixed):
        cat, catn, off = _cat(clouds, normals)
        k, p = _up(cat); kq, q = _up(catn); keep.extend([k, kq])
        return ctx.gicp_batch_dev(p, q, off, pt, pn, nt, T0s, 0.004, 10, G.EPSILON, fixed)

    def run_single(inp, b):
        clouds, normals, T0s, fixed = inp
        if len(clouds[b]) == 0:
            return None
        k, p = _up(clouds[b]); kq, q = _up(normals[b]); keep.extend([k, kq])
        return ctx.gicp_dev(p, q, len(clouds[b]), pt, pn, nt, T0s[b], 0.004, 10, G.EPSILON, fixed)

    for fixed in fixeds:
        _isolation(ctx, run_batch, run_single, (clean_c, clean_n, clean_T, fixed), (bad_c, bad_n, bad_T, fixed), POISONED + (8,),
                   (regime, loss, fixed))


def test_refine_batch_isolation(pctx, tdv, synth):
    """tdv_refine_batch_dev with NaN and infinite start poses among clean ones, against a clean and a poisoned model: every instance
    equals the stagewise chain depth_to_cloud -> voxel_downsample -> icp; the clean ones equal the all-clean batch."""
    from test_gpu_icp_batch import _model, _scene, _start_poses
    ctx, _ = pctx
    voxel = 0.004
    depth, masks, intr, poses = _scene(synth, 4)
    n_inst = len(masks)
    d_mx, d_mn, nm = _model(ctx, tdv, synth, voxel)
    T0s = _start_poses(synth, poses, n_inst).astype(F)
    bad_T = T0s.copy(); bad_T[1][0, 3] = np.nan; bad_T[3][1, 1] = np.inf
    prm = tdv.batch_params(voxel_size=voxel, zmax=1.5, icp_max_iterations=30, voxel_order=tdv.TDV_VOXEL_ORDER_FIRST, **intr)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(DEV); d_masks = torch.from_numpy(masks).to(DEV)

    def run(T):
        return ctx.refine_batch_dev(d_depth.data_ptr(), None, d_masks.data_ptr(), n_inst, prm, T, d_mx.data_ptr(), d_mn.data_ptr(), nm)

    for model in ("clean", "poisoned"):
        if model == "poisoned":
            mx = d_mx[:nm].cpu().numpy().copy()
            rng = np.random.default_rng(6)
            rows = rng.choice(nm, nm // 8, replace=False)
            mx[rows, rng.integers(0, 3, len(rows))] = np.array([np.inf, -np.inf, NEG_NAN, 1e19], F)[rng.integers(0, 4, len(rows))]
            d_mx[:nm].copy_(torch.from_numpy(mx).to(DEV))
        mx, mn = d_mx[:nm].cpu().numpy(), d_mn[:nm].cpu().numpy()
        ref = run(T0s)
        got = run(bad_T)
        for b, r in enumerate(got):
            xyz, _ = ctx.depth_to_cloud(depth, masks[b], None, 1000.0, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 1.5)
            if len(xyz) == 0:
                assert r["status"] == 1 and r["T"].tobytes() == bad_T[b].tobytes(), (model, b)
                continue
            src, _ = ctx.voxel_downsample(xyz, None, voxel, tdv.TDV_VOXEL_ORDER_FIRST)
            fine = ctx.icp(src, mx, mn, bad_T[b], voxel * 0.4, 30, True)
            assert r["status"] == 0 and r["icp_iterations"] == fine.iterations, (model, b, r["icp_iterations"], fine.iterations)
            _same(r["T"], fine.transformation, (model, b))
            _same(np.float32(r["fitness"]), np.float32(fine.fitness), (model, b)); _same(np.float32(r["rmse"]), np.float32(fine.rmse), (model, b))
            if b not in (1, 3):
                assert r["T"].tobytes() == ref[b]["T"].tobytes() and r["icp_iterations"] == ref[b]["icp_iterations"], (model, b)
                assert np.float32(r["rmse"]).tobytes() == np.float32(ref[b]["rmse"]).tobytes(), (model, b)


# ---------------------------------------------------------------- RANSAC with the bail-out off
def test_ransac_non_finite_without_bailout(tdv):
    """TDV_RANSAC_BAILOUT is read once per process (csrc/ransac.hip): test_ransac_non_finite runs again in a process of its own with
    the bail-out off."""
    env = dict(os.environ, TDV_RANSAC_BAILOUT="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_nonfinite.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_ransac_non_finite", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    print(tail)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert " passed" in tail and "skipped" not in tail, tail
