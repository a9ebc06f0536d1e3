"""tdv_ppf_match_batch_dev against its definition: per instance, tdv_ppf_match_dev (include/tdv_hip.h), byte for byte - poses with their scores
and cluster fields, n_poses and peaks - on batches whose work items outnumber the workgroups of every counter variant, on ragged batches with
empty, tiny, tile-sized, non-finite and unusable instances, in both orders, at other parameters, down the chain into tdv_icp_batch_dev, and
for the empty cases and the refusals on a real ctx.  tests/test_gpu_ppf.py holds the single call to the restatement; where an instance's
restatement is at hand (ppf_scene.restated, ppf_restatement.peaks) the batch's peaks are held to it directly."""
import numpy as np
import pytest
import torch

import ppf_batch_cases as B
import ppf_restatement as R
import ppf_scene as S
from state_cases import Env
from test_gpu_ppf import device_buffers, same_peaks
from test_ppf_abi import TDV_ERR_BAD_ARG
from test_ppf_batch_abi import batch_refusals

pytestmark = pytest.mark.gpu
F = np.float32
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sc(synth):
    return B.scene(synth, 1)


@pytest.fixture(scope="module")
def ref(synth):
    return S.restated(synth)


@pytest.fixture(scope="module")
def eight(ctx, synth, sc):
    """The eight-instance batch and its single calls at the defaults, computed once: dict(setup, batch, peak_off, singles)."""
    st = B.Setup(ctx, Env(ctx), B.clouds_of(synth, B.EIGHT), sc["model"], sc["model_normals"])
    got, peak_off = st.batch()
    return dict(setup=st, batch=got, peak_off=peak_off, results=st.results, singles=st.singles())


def test_eight_instances_equal_their_single_calls(eight, ref):
    """2,320 work items on at most 2,048 workgroups: workgroups take several items, of different instances."""
    st = eight["setup"]
    assert int(st.peak_off[-1]) == 2320 and (eight["peak_off"] == st.peak_off).all()
    B.same(eight["singles"], eight["batch"], "eight instances")
    assert all(len(bl) > 0 for bl, _ in eight["batch"]) and len(eight["batch"][B.EIGHT.index(1)][0]) == 8
    same_peaks(ref["peaks"], eight["batch"][B.EIGHT.index(1)][1], "instance 1 against the restatement")


def ragged(sc):
    """Sizes 0, 1, 4, 5, 6, 511, 512, 513 and 1,446 (the first rows of the scene), empty instances first, in the middle and last, the 700
    points with NaN / inf / zero-normal rows of test_non_finite_scene_points_and_normals, and 64 points whose normals are all zero."""
    s, n = sc["scene"], sc["scene_normals"]
    nf_s, nf_n = s[:700].copy(), n[:700].copy()
    nf_s[0, 0] = np.nan; nf_s[35] = np.inf; nf_n[70, 1] = np.nan; nf_n[105] = -np.inf; nf_n[140] = 0.0          # reference points
    nf_s[3, 2] = np.nan; nf_s[36, 1] = -np.inf; nf_n[71] = np.nan; nf_n[106, 0] = np.inf; nf_n[141] = 0.0       # partners
    cut = lambda k: (s[:k], n[:k])   # noqa: E731
    return [cut(0), cut(1), cut(4), cut(5), cut(6), cut(511), (s[100:164], np.zeros((64, 3), F)), cut(0), cut(512), cut(513), (nf_s, nf_n),
            cut(len(s)), cut(0)]


def test_ragged_batch(ctx, sc, ref):
    clouds = ragged(sc)
    assert [len(p) for p, _ in clouds] == [0, 1, 4, 5, 6, 511, 64, 0, 512, 513, 700, 1446, 0]
    st = B.Setup(ctx, Env(ctx), clouds, sc["model"], sc["model_normals"])
    got, peak_off = st.batch()
    assert (peak_off == st.peak_off).all()
    want = st.singles()
    B.same(want, got, "ragged")
    n_poses = [len(bl) for bl, _ in got]
    assert [k for k, m in enumerate(n_poses) if m == 0] == [k for k, (bl, _) in enumerate(want) if not bl]
    assert all(n_poses[k] == 0 for k in (0, 1, 6, 7, 12)) and n_poses[11] == 8 and n_poses[10] > 0
    for k, (p, n) in enumerate(clouds):
        if 0 < len(p) < 520:
            same_peaks(R.peaks(p, n, ref["model"]), got[k][1], "instance %d (%d points) against the restatement" % (k, len(p)))
        elif len(p) == 0:
            assert len(got[k][1]) == 0
    assert (got[6][1]["votes"] == 0).all() and len(got[6][1]) == 13
    same_peaks(ref["peaks"], got[11][1], "the whole scene against the restatement")


@pytest.mark.parametrize("bins", [30, 64, 128])
def test_the_three_counter_variants(tdv, ctx, synth, sc, bins):
    """330 x 30 = 9,900 cells (small LDS), x 64 = 21,120 (large LDS), x 128 = 42,240 (slabs): 870 items, more than the 512 workgroups of a
    slab launch."""
    cells = len(sc["model"]) * bins
    assert cells == {30: 9900, 64: 21120, 128: 42240}[bins] and (cells > tdv.TDV_PPF_LDS_CELLS) == (bins == 128)
    st = B.Setup(ctx, Env(ctx), B.clouds_of(synth, (1, 2, 4)), sc["model"], sc["model_normals"], rotation_bins=bins, ref_stride=5)
    assert int(st.peak_off[-1]) == 870
    got, _ = st.batch()
    B.same(st.singles(), got, "rotation_bins %d" % bins)
    assert all(len(bl) > 0 for bl, _ in got)


def test_position_independence(ctx, synth, sc, eight):
    st = B.Setup(ctx, Env(ctx), B.clouds_of(synth, B.EIGHT[::-1]), sc["model"], sc["model_normals"])
    got, _ = st.batch()
    B.same(eight["batch"][::-1], got, "the batch reversed")
    some = B.Setup(ctx, Env(ctx), B.clouds_of(synth, (B.EIGHT[5], B.EIGHT[0])) + [(sc["scene"][:0], sc["scene_normals"][:0])] +
                   B.clouds_of(synth, (B.EIGHT[5],)), sc["model"], sc["model_normals"])
    got, _ = some.batch()
    B.same([eight["batch"][5], eight["batch"][0], ([], np.zeros(0, R.PEAK)), eight["batch"][5]], got, "other neighbours")


def test_parameters(ctx, synth, sc, ref, eight):
    one = B.Setup(ctx, Env(ctx), B.clouds_of(synth, (1,)), sc["model"], sc["model_normals"])
    got, _ = one.batch()
    want = one.singles()
    B.same(want, got, "a batch of one")
    B.same([eight["batch"][B.EIGHT.index(1)]], got, "a batch of one against its place among eight")
    got, _ = one.batch(peaks=False)                                  # without d_peaks: the same poses
    assert got[0][0] == want[0][0]
    for kw in (dict(max_poses=3), dict(cluster_translation_relative=1e6, cluster_rotation=float(F(3.14159274)))):
        st = B.Setup(ctx, Env(ctx), B.clouds_of(synth, (1, 2, 4)), sc["model"], sc["model_normals"], **kw)
        got, _ = st.batch()
        B.same(st.singles(), got, kw)
        assert len(got[0][0]) == (3 if "max_poses" in kw else 1) and all(0 < len(bl) <= 8 for bl, _ in got)
    pk = ref["peaks"]                                                # one cluster: every vote of instance 1
    assert dict(got[0][0][0][4])["votes"] == int(pk["votes"].sum())


def test_chain_batch_into_icp_batch(ctx, synth, sc, ref, eight):
    """The best-fitness pose of every instance into tdv_icp_batch_dev: test_chain_best_pose_into_icp's bounds before and after."""
    st = eight["setup"]
    best = [max(res, key=lambda r: r.fitness) for res in eight["results"]]
    diameter = float(ref["model"]["diameter"])
    for k, b in zip(B.EIGHT, best):
        ang, tr = synth.pose_error(b.transformation, B.scene(synth, k)["T_gt"])
        print("instance %d: PPF fitness %.3f angle %.4f rad translation %.5f m" % (k, b.fitness, ang, tr))
        assert ang <= 2.0 * np.pi / 30.0 and tr <= 0.1 * diameter, (k, ang, tr)
    fine = ctx.icp_batch_dev(st.d_src, st.off, st.d_tgt, st.d_tn, st.nt, np.stack([b.transformation for b in best]), S.THR, S.ICP_ITERS)
    for k, f in zip(B.EIGHT, fine):
        ang, tr = synth.pose_error(f.transformation, B.scene(synth, k)["T_gt"])
        print("instance %d: ICP %d iterations: %.5f rad, %.2e m" % (k, f.iterations, ang, tr))
        assert ang < 1e-2 and tr < 1e-3, (k, ang, tr)


def test_refusals_on_a_real_context(tdv, ctx, synth, sc, eight):
    dev = device_buffers(tdv)
    o, calls = batch_refusals(tdv, ctx._h, dev)
    for what, status in calls:
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()
    ctx.synchronize()
    assert all(int(t.min()) == 0xA5 == int(t.max()) for t in dev["keep"][1:]), "a refused call wrote device memory"
    st = B.Setup(ctx, Env(ctx), B.clouds_of(synth, B.EIGHT[:2]), sc["model"], sc["model_normals"])         # ... and the ctx still works
    B.same(eight["batch"][:2], st.batch()[0], "after the refusals")


def test_empty_cases(ctx, synth, sc):
    """n_instances == 0, a 1-point model and a model with zero normals (a table without pairs): OK, no pose, every peak offset 0, no peak."""
    clouds = B.clouds_of(synth, (1, 2))
    for what, cl, m, mn in (("no instance", [], sc["model"], sc["model_normals"]), ("a 1-point model", clouds, sc["model"][:1], sc["model_normals"][:1]),
                            ("zero model normals", clouds, sc["model"][:40], np.zeros((40, 3), F)),
                            ("only empty instances", [(sc["scene"][:0], sc["scene_normals"][:0])] * 3, sc["model"], sc["model_normals"])):
        st = B.Setup(ctx, Env(ctx), cl, m, mn)
        d_pk = st.env.out(int(st.peak_off[-1]) + 1, R.PEAK)
        out, peak_off = ctx.ppf_match_batch_dev(st.d_src, st.d_sn, st.off, st.d_tgt, st.d_tn, st.nt, st.table.data_ptr(), st.info, S.THR,
                                                d_peaks=d_pk.data_ptr())
        assert out == [([], [])] * len(cl) and len(peak_off) == len(cl) + 1 and not peak_off.any(), what
        pk = st.env.get(d_pk, int(st.peak_off[-1]) + 1, R.PEAK).view(np.uint8)
        assert pk.min() == 0xA5 == pk.max(), what
    res = ctx.ppf_match_batch([p for p, _ in clouds], [n for _, n in clouds], sc["model"][:1], sc["model_normals"][:1], S.THR, want_peaks=True)
    assert [(r, m, len(pk)) for r, m, pk in res] == [([], [], 0)] * 2


def test_host_arrays_front_end(ctx, synth, sc, eight):
    """Context.ppf_match_batch: lists of host arrays, uploaded with torch, the table from ppf_model_dev."""
    ks = B.EIGHT[:3]
    clouds = B.clouds_of(synth, ks)
    res = ctx.ppf_match_batch([p for p, _ in clouds], [n for _, n in clouds], sc["model"], sc["model_normals"], S.THR, want_peaks=True)
    B.same(eight["batch"][:3], [(B.blob(r, m), pk) for r, m, pk in res], "host arrays")
    res = ctx.ppf_match_batch([p for p, _ in clouds], [n for _, n in clouds], sc["model"], sc["model_normals"], S.THR)
    assert [B.blob(r, m) for r, m in res] == [bl for bl, _ in eight["batch"][:3]]
    with pytest.raises(ValueError):
        ctx.ppf_match_batch([p for p, _ in clouds], [n[:-1] for _, n in clouds], sc["model"], sc["model_normals"], S.THR)


def test_search_mode_does_not_enter(tdv, synth, sc, eight):
    """Every ICP search switch gives the batch's bytes, and after a call that scored a pose the ctx reports the brute scan."""
    c = tdv.Context(0)
    try:
        for mode in ("brute", "pruned", "grid", "auto"):
            c.set_icp_search(mode)
            st = B.Setup(c, Env(c), B.clouds_of(synth, B.EIGHT[:2]), sc["model"], sc["model_normals"])
            B.same(eight["batch"][:2], st.batch()[0], mode)
            assert tdv.lib().tdv_ctx_last_icp_search(c._h) == c.ICP_SEARCH["brute"], mode
    finally:
        c.close()
