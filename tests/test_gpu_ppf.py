"""tdv_ppf_model_dev, tdv_ppf_match_dev and tdv_ppf_match against the numpy restatement of the header's rules (tests/ppf_restatement.py) on
the scene the restatement alone solves (tests/ppf_scene.py, tests/test_ppf_abi.py): the model table, the peaks (on every accumulator path:
the two LDS variants and the workspace slabs, at the model sizes where the path changes), non-finite inputs, the poses with their
clusters and scores, the chain into ICP, the empty cases, the refusals on a real ctx, and the host form against the device form."""
import numpy as np
import pytest
import torch

import ppf_restatement as R
import ppf_scene as S
from test_ppf_abi import TDV_ERR_BAD_ARG, refusals

pytestmark = pytest.mark.gpu
F = np.float32
DEV = torch.device("cuda", 0)
TABLE = ("offsets", "pair", "alpha_bits", "key")


@pytest.fixture(scope="module")
def sc(synth):
    return S.build(synth)


@pytest.fixture(scope="module")
def ref(synth):
    return S.restated(synth)


def same_table(want, got, what):
    for k in ("diameter", "distance_step"):
        assert F(want[k]).tobytes() == F(got[k]).tobytes(), (what, k, want[k], got[k])
    for k in ("n_pairs", "n_keys", "nt"):
        assert want[k] == got[k], (what, k, want[k], got[k])
    for k in TABLE:
        assert want[k].dtype == got[k].dtype and want[k].tobytes() == got[k].tobytes(), (what, k)


def same_peaks(want, got, what):
    bad = np.flatnonzero(want != got)
    assert want.shape == got.shape and len(bad) == 0, (what, len(bad), want[bad[:4]], got[bad[:4]])


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (through the ordered integer image of the bits)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def dense_model(synth, nt):
    """The first nt points of a finer sampling of the part: a model of exactly nt points."""
    p, n = S._surface(synth.ReliefPart(3), 0.0027)
    assert len(p) >= nt
    return p[:nt].astype(F), n[:nt].astype(F)


# ---------------------------------------------------------------- the model table
@pytest.mark.parametrize("flip", [0, 1])
def test_model_table_equals_the_restatement(ctx, sc, flip):
    m, n = sc["model"][:300].copy(), sc["model_normals"][:300].copy()
    m[7] = m[3]                                   # a duplicated point: |d| = 0 both ways
    m[20, 1] = np.nan; m[50, 0] = np.inf; m[51, 2] = -np.inf
    n[80] = 0.0                                   # a zero normal
    n[90, 2] = np.nan; n[100] = 1e-30             # ... a non-finite one, and one whose squared length underflows to 0
    want = R.model_table(m, n, flip_model_normals=flip)
    assert 60000 < want["n_pairs"] < 300 * 299 - 6 * 2 * 299 + 100
    same_table(want, ctx.ppf_model(m, n, flip_model_normals=flip), "flip %d" % flip)


def test_model_table_of_the_scene_model_and_other_bins(ctx, sc, ref):
    same_table(ref["model"], ctx.ppf_model(sc["model"], sc["model_normals"]), "defaults")
    kw = dict(distance_step_relative=0.08, angle_bins=17)
    same_table(R.model_table(sc["model"], sc["model_normals"], **kw), ctx.ppf_model(sc["model"], sc["model_normals"], **kw), kw)


# ---------------------------------------------------------------- peaks
def test_peaks_equal_the_restatement_on_the_scene(ctx, sc, ref):
    """330 x 30 counters: the small LDS variant; with 31 rotation bins the large one."""
    _, _, pk = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, want_peaks=True)
    assert (ref["peaks"]["votes"] > 0).sum() > 200
    same_peaks(ref["peaks"], pk, "defaults")
    m = dict(ref["model"], params=R.params(rotation_bins=31, ref_stride=15))
    _, _, pk = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, want_peaks=True, rotation_bins=31, ref_stride=15)
    same_peaks(R.peaks(sc["scene"], sc["scene_normals"], m), pk, "31 rotation bins")


@pytest.mark.parametrize("nt,bins", [(1300, 30), (1301, 30), (152, 256), (153, 256)])
def test_peaks_on_both_sides_of_the_lds_limit(tdv, ctx, synth, sc, nt, bins):
    """nt * rotation_bins <= TDV_PPF_LDS_CELLS: counters in LDS; one model point more: slabs of the workspace.  A handful of reference points."""
    in_lds = nt * bins <= tdv.TDV_PPF_LDS_CELLS
    assert in_lds == (nt in (1300, 152)) and ((nt + 1) * bins > tdv.TDV_PPF_LDS_CELLS if in_lds else (nt - 1) * bins <= tdv.TDV_PPF_LDS_CELLS)
    m, n = dense_model(synth, nt)
    kw = dict(rotation_bins=bins, ref_stride=241)
    model = R.model_table(m, n, **kw)
    want = R.peaks(sc["scene"], sc["scene_normals"], model)
    assert len(want) == 6 and (want["votes"] > 0).sum() >= 4
    _, _, pk = ctx.ppf_match(sc["scene"], sc["scene_normals"], m, n, S.THR, want_peaks=True, **kw)
    same_peaks(want, pk, (nt, bins))


def test_non_finite_scene_points_and_normals(ctx, sc, ref):
    """NaN and infinite coordinates and normals at reference positions (multiples of ref_stride) and at partner positions: skipped in
    every role, no other effect."""
    s, n = sc["scene"][:700].copy(), sc["scene_normals"][:700].copy()
    s[0, 0] = np.nan; s[35] = np.inf; n[70, 1] = np.nan; n[105] = -np.inf; n[140] = 0.0          # reference points
    s[3, 2] = np.nan; s[36, 1] = -np.inf; n[71] = np.nan; n[106, 0] = np.inf; n[141] = 0.0       # partners
    want = R.peaks(s, n, ref["model"])
    assert (want["votes"][[0, 7, 14, 21, 28]] == 0).all() and (want["votes"] > 0).sum() > 100
    _, _, pk = ctx.ppf_match(s, n, sc["model"], sc["model_normals"], S.THR, want_peaks=True)
    same_peaks(want, pk, "non-finite scene")


# ---------------------------------------------------------------- poses
def test_poses_clusters_and_scores(ctx, sc, ref):
    res, more = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR)
    want = ref["poses"]
    assert len(res) == len(want) == 8
    for k, (r, m, w) in enumerate(zip(res, more, want)):
        assert m == {key: w[key] for key in ("votes", "members", "ref", "model_index", "bin")}, (k, m, w)
        u = ulps(r.transformation, w["T"])
        assert u.max() <= 2, (k, u, r.transformation, w["T"])        # both sides compute in f64 and round once: the last bit of sin / cos
        n_corr, fitness, rmse = R.score(ctx.icp_correspondences(sc["scene"], sc["model"], r.transformation, S.THR))
        assert (r.n_corr, F(r.fitness).tobytes(), F(r.rmse).tobytes()) == (n_corr, F(fitness).tobytes(), F(rmse).tobytes()), (k, r, n_corr, fitness, rmse)
    assert [m["votes"] for m in more] == sorted((m["votes"] for m in more), reverse=True)


def test_fewer_poses_and_one_cluster(ctx, sc, ref):
    """max_poses cuts the ranked list; with thresholds that take in everything there is one cluster: the first peak's, with every vote."""
    res, more = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, max_poses=3)
    assert [m["votes"] for m in more] == [w["votes"] for w in ref["poses"][:3]]
    res, more = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, cluster_translation_relative=1e6,
                              cluster_rotation=float(F(3.14159274)))
    pk = ref["peaks"]
    first = pk[np.argsort(-pk["votes"].astype(np.int64), kind="stable")[0]]
    assert len(more) == 1 and more[0] == dict(votes=int(pk["votes"].sum()), members=int((pk["votes"] > 0).sum()), ref=int(first["ref"]),
                                              model_index=int(first["model_index"]), bin=int(first["bin"]))


def test_chain_best_pose_into_icp(ctx, synth, sc, ref):
    res, _ = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR)
    best = max(res, key=lambda r: r.fitness)
    ang, tr = synth.pose_error(best.transformation, sc["T_gt"])
    assert ang <= 2.0 * np.pi / 30.0 and tr <= 0.1 * float(ref["model"]["diameter"]), (ang, tr)
    d = [torch.from_numpy(np.array(sc[k])).to(DEV) for k in ("scene", "model", "model_normals")]
    torch.cuda.synchronize()
    fine = ctx.icp_dev(d[0].data_ptr(), len(sc["scene"]), d[1].data_ptr(), d[2].data_ptr(), len(sc["model"]), best.transformation, S.THR, S.ICP_ITERS)
    ang_f, tr_f = synth.pose_error(fine.transformation, sc["T_gt"])
    print("PPF best pose: fitness %.3f angle %.4f rad translation %.5f m; ICP %d iterations: %.5f rad, %.2e m" %
          (best.fitness, ang, tr, fine.iterations, ang_f, tr_f))
    assert ang_f < 1e-2 and tr_f < 1e-3                              # the bounds of the chain tests (tests/test_oracle_chain.py)


# ---------------------------------------------------------------- empty cases, refusals, the two forms
def test_degenerate_inputs_give_no_pose(ctx, sc):
    none = np.zeros((0, 3), F)
    for s, sn, t, tn in ((none, none, sc["model"], sc["model_normals"]), (sc["scene"], sc["scene_normals"], none, none),
                         (sc["scene"], sc["scene_normals"], sc["model"][:1], sc["model_normals"][:1]),
                         (sc["scene"][:50], sc["scene_normals"][:50], sc["model"][:40], np.zeros((40, 3), F))):     # a table without pairs
        res, more, pk = ctx.ppf_match(s, sn, t, tn, S.THR, want_peaks=True)
        assert res == [] and more == [] and len(pk) == 0
    for nt in (0, 1):
        got = ctx.ppf_model(sc["model"][:nt], sc["model_normals"][:nt])
        assert got["n_pairs"] == 0 and got["diameter"] == 0 and not got["offsets"].any()


def device_buffers(tdv):
    """Device memory for every pointer slot of the device entry points at the sizes the refusal list uses (clouds of up to
    TDV_PPF_MODEL_MAX + 1 points, the table of a 4-point model, one peak per reference point)."""
    cloud = torch.zeros(3 * (tdv.TDV_PPF_MODEL_MAX + 1), dtype=torch.float32, device=DEV)
    model = torch.full((4 << 20,), 0xA5, dtype=torch.uint8, device=DEV)
    peaks = torch.full((64,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    return dict(cloud=cloud.data_ptr(), model=model.data_ptr(), model_bytes=model.numel(), peaks=peaks.data_ptr(), keep=(cloud, model, peaks))


def test_refusals_on_a_real_context(tdv, ctx, sc):
    dev = device_buffers(tdv)
    o, calls = refusals(tdv, ctx._h, dev)
    for what, status in calls:
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()
    ctx.synchronize()
    assert all(int(t.min()) == 0xA5 == int(t.max()) for t in dev["keep"][1:]), "a refused call wrote device memory"
    res, _ = ctx.ppf_match(sc["scene"][:300], sc["scene_normals"][:300], sc["model"], sc["model_normals"], S.THR)     # ... and the ctx still works
    assert len(res) > 0


def dev_call(ctx, sc, env_up, env_out, env_get, **kw):
    """tdv_ppf_model_dev + tdv_ppf_match_dev on device buffers: (info, table words, poses, dicts, peaks)."""
    ns, nt = len(sc["scene"]), len(sc["model"])
    d = [env_up(sc[k]) for k in ("scene", "scene_normals", "model", "model_normals")]
    nbytes = ctx.ppf_model_bytes(nt, **kw)
    buf = env_out(nbytes, np.uint8)
    info = ctx.ppf_model_dev(d[2], d[3], nt, buf.data_ptr(), nbytes, **kw)
    n_ref = (ns + 4) // 5
    d_pk = env_out(n_ref, R.PEAK)
    res, more, got_ref = ctx.ppf_match_dev(d[0], d[1], ns, d[2], d[3], nt, buf.data_ptr(), info, S.THR, d_peaks=d_pk.data_ptr(), **kw)
    assert got_ref == n_ref
    return info, env_get(buf, nbytes, np.uint8), res, more, env_get(d_pk, n_ref, R.PEAK)


def pose_blob(res, more):
    return [(r.transformation.tobytes(), F(r.fitness).tobytes(), F(r.rmse).tobytes(), r.n_corr, tuple(sorted(m.items()))) for r, m in zip(res, more)]


def test_host_form_equals_the_device_form(ctx, sc, ref):
    from state_cases import Env
    env = Env(ctx)
    info, words, res, more, pk = dev_call(ctx, sc, env.up, env.out, env.get)
    h_res, h_more, h_pk = ctx.ppf_match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"], S.THR, want_peaks=True)
    assert info["n_pairs"] == ref["model"]["n_pairs"] and F(info["diameter"]) == ref["model"]["diameter"]
    assert words[:4 * (info["n_keys"] + 1)].view(np.int32).tobytes() == ref["model"]["offsets"].tobytes()
    same_peaks(ref["peaks"], pk, "device form")
    same_peaks(h_pk, pk, "host against device form")
    assert pose_blob(res, more) == pose_blob(h_res, h_more)


def test_the_dict_of_ppf_model_is_an_info_too(ctx, sc):
    """Context.ppf_match_dev takes the dict of ppf_model_dev or the larger one of ppf_model: the fields of tdv_ppf_model_info count."""
    ns, nt = len(sc["scene"]), len(sc["model"])
    d = [torch.from_numpy(np.array(sc[k])).to(DEV) for k in ("scene", "scene_normals", "model", "model_normals")]
    nbytes = ctx.ppf_model_bytes(nt)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    info = ctx.ppf_model_dev(d[2].data_ptr(), d[3].data_ptr(), nt, buf.data_ptr(), nbytes)
    full = ctx.ppf_model(sc["model"], sc["model_normals"])
    assert {k: full[k] for k in info} == info and "offsets" in full
    a = ctx.ppf_match_dev(d[0].data_ptr(), d[1].data_ptr(), ns, d[2].data_ptr(), d[3].data_ptr(), nt, buf.data_ptr(), info, S.THR)
    b = ctx.ppf_match_dev(d[0].data_ptr(), d[1].data_ptr(), ns, d[2].data_ptr(), d[3].data_ptr(), nt, buf.data_ptr(), full, S.THR)
    assert pose_blob(a[0], a[1]) == pose_blob(b[0], b[1]) and a[2] == b[2] == (ns + 4) // 5
