"""CPU suite: PPF matching (include/tdv_hip.h: tdv_ppf_match).  The ABI exports the entry points, lists them in ABI_SYMBOLS, has the documented
defaults and struct layouts and refuses every bad argument before it writes anything; the restatement (tests/ppf_restatement.py) alone
finds the pose of the shared scene (tests/ppf_scene.py) within one rotation bin and the cluster translation bound, and the oracle's ICP
takes that pose to the ground truth within the bounds of tests/test_oracle_chain.py.  No compute entry point of the library runs here;
tests/test_gpu_ppf.py holds the device to this restatement."""
import ctypes as C

import numpy as np
import pytest

import ppf_restatement as R
import ppf_scene as S

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_ppf_default_params", "tdv_ppf_model_bytes", "tdv_ppf_model_dev", "tdv_ppf_match_dev", "tdv_ppf_match")
NAN, INF = float("nan"), float("inf")


def test_symbols_defaults_and_structs(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)
    assert C.sizeof(tdv.PpfParamsC) == 32 and C.sizeof(tdv.PpfModelInfoC) == 20 and C.sizeof(tdv.PpfPoseC) == 96
    assert tdv.PPF_PEAK_DTYPE.itemsize == 16 and tdv.PPF_PEAK_DTYPE == R.PEAK
    assert [k for k, _ in tdv.PpfPoseC._fields_] == ["T", "fitness", "rmse", "n_corr", "votes", "members", "ref", "model_index", "bin"]
    p = tdv.ppf_params()
    got = {k: getattr(p, k) for k, _ in tdv.PpfParamsC._fields_}
    want = dict(distance_step_relative=F(0.05), angle_bins=30, rotation_bins=30, ref_stride=5, max_poses=8, cluster_translation_relative=F(0.1),
                cluster_rotation=F(2.0 * np.pi / 30.0), flip_model_normals=0)
    assert got == want
    assert {k: (F(v) if isinstance(v, float) else v) for k, v in R.DEFAULTS.items()} == want
    assert tdv.ppf_params(ref_stride=7).ref_stride == 7
    with pytest.raises(TypeError):
        tdv.ppf_params(stride=1)
    assert (tdv.TDV_PPF_MODEL_MAX, tdv.TDV_PPF_POSES_MAX, tdv.TDV_PPF_KEYS_MAX, tdv.TDV_PPF_LDS_CELLS) == (2048, 64, 1 << 24, 39000)
    header = open(tdv.LIB_PATH.rsplit("/3dvision_amd/", 1)[0] + "/include/tdv_hip.h").read()
    for name in ("MODEL_MAX 2048", "POSES_MAX 64", "KEYS_MAX (1 << 24)", "LDS_CELLS 39000"):
        assert "#define TDV_PPF_" + name in header


def test_model_bytes_is_the_documented_layout(tdv):
    lib = tdv.lib()
    for nt in (0, 1, 2, 300, 2048):
        b = C.c_size_t(7)
        assert lib.tdv_ppf_model_bytes(nt, C.byref(tdv.ppf_params()), C.byref(b)) == 0
        n_keys = R.key_space(R.params())[1]
        assert n_keys == 21 * 27000
        assert b.value == 4 * ((n_keys + 1 + 3) // 4 * 4 + 2 * (nt * (nt - 1) if nt >= 2 else 0))


# ---------------------------------------------------------------- arguments
BAD = [("step nan", dict(distance_step_relative=NAN)), ("step 0", dict(distance_step_relative=0.0)), ("step < 0", dict(distance_step_relative=-0.05)),
       ("step > 1", dict(distance_step_relative=1.5)), ("step inf", dict(distance_step_relative=INF)),
       ("angle_bins 0", dict(angle_bins=0)), ("angle_bins 65", dict(angle_bins=65)), ("rotation_bins 0", dict(rotation_bins=0)),
       ("rotation_bins 257", dict(rotation_bins=257)), ("too many keys", dict(distance_step_relative=0.001, angle_bins=64)),
       ("ref_stride 0", dict(ref_stride=0)), ("max_poses 0", dict(max_poses=0)), ("max_poses 65", dict(max_poses=65)),
       ("cluster translation nan", dict(cluster_translation_relative=NAN)), ("cluster translation inf", dict(cluster_translation_relative=INF)),
       ("cluster translation < 0", dict(cluster_translation_relative=-0.1)), ("cluster rotation nan", dict(cluster_rotation=NAN)),
       ("cluster rotation < 0", dict(cluster_rotation=-0.1)), ("cluster rotation > pi", dict(cluster_rotation=3.2)), ("flip 2", dict(flip_model_normals=2))]
BAD_THR = [NAN, INF, 0.0, -0.01]


class Outputs:
    """Every host output of the three calls, filled with a pattern; untouched() compares them with it."""

    def __init__(self, tdv, n_ref=4, fill=0x5A):
        self.poses = (tdv.PpfPoseC * tdv.TDV_PPF_POSES_MAX)(); C.memset(self.poses, fill, C.sizeof(self.poses))
        self.info = tdv.PpfModelInfoC(); C.memset(C.byref(self.info), fill, C.sizeof(self.info))
        self.n_poses, self.n_ref, self.bytes = C.c_int(-7), C.c_int(-7), C.c_size_t(7)
        self.peaks = np.full(n_ref, -7, R.PEAK)
        self.before = self.snapshot()

    def snapshot(self):
        return bytes(self.poses), bytes(self.info), self.n_poses.value, self.n_ref.value, self.bytes.value, self.peaks.tobytes()

    def untouched(self):
        return self.snapshot() == self.before


P = lambda x: None if x is None else (C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p))   # noqa: E731


def _ppf_call(tdv, which, ctx, o, src=None, sn=None, ns=4, tgt=None, tn=None, nt=4, thr=0.01, model=None, model_bytes=None, info=True, prm=True,
             poses=True, n_poses=True, good_info=None, dev=None, **kw):
    """One of "bytes", "model", "match_dev", "match".  A refused call must not look at its arrays: with a NULL ctx host arrays stand in every
    pointer slot; on a real ctx `dev` (device_buffers in tests/test_gpu_ppf.py) puts device memory into the device entry points' slots, so
    that a refusal that went missing would run on valid buffers and fail the test instead of faulting."""
    lib = tdv.lib()
    p = tdv.ppf_params(**kw)
    pp = C.byref(p) if prm else None
    on_dev = dev is not None and which in ("model", "match_dev")
    z = dev["cloud"] if on_dev else np.zeros((max(ns, nt, 1), 3), F)
    src, sn, tgt, tn = (z if a is None else (None if a is False else a) for a in (src, sn, tgt, tn))
    model = ((dev["model"] if on_dev else np.zeros(1 << 20, np.uint32)) if model is None else (None if model is False else model))
    if isinstance(model, str):                                       # "odd": a misaligned pointer
        model = (dev["model"] if on_dev else np.zeros(64, np.uint8).ctypes.data) + 1
    peaks = dev["peaks"] if on_dev else o.peaks
    if which == "bytes":
        return lib.tdv_ppf_model_bytes(nt, pp, C.byref(o.bytes))
    if which == "model":
        nbytes = (dev["model_bytes"] if on_dev else 1 << 40) if model_bytes is None else model_bytes
        return lib.tdv_ppf_model_dev(ctx, P(tgt), P(tn), nt, pp, P(model), C.c_size_t(nbytes), C.byref(o.info) if info else None)
    po, npo = (o.poses if poses else None), (C.byref(o.n_poses) if n_poses else None)
    if which == "match":
        return lib.tdv_ppf_match(ctx, P(src), P(sn), ns, P(tgt), P(tn), nt, C.c_float(thr), pp, po, npo, P(o.peaks), C.byref(o.n_ref))
    gi = tdv.PpfModelInfoC(**dict(dict(diameter=1.0, distance_step=0.05, n_pairs=0, n_keys=R.key_space(R.params())[1], nt=nt), **(good_info or {})))
    return lib.tdv_ppf_match_dev(ctx, P(src), P(sn), ns, P(tgt), P(tn), nt, P(model), C.byref(gi) if info else None, C.c_float(thr), pp, po, npo,
                                 P(peaks), C.byref(o.n_ref))


ppf_call = _ppf_call


def refusals(tdv, ctx, dev=None):
    """Every refusal the header names, as (what, status) - on `ctx` (NULL here; a real one in tests/test_gpu_ppf.py).  The caller checks the
    statuses and that `o` is untouched."""
    o = Outputs(tdv)
    calls = []
    ppf_call = lambda *a, **kw: _ppf_call(*a, dev=dev, **kw)   # noqa: E731
    for what, kw in BAD:
        for which in ("bytes", "model", "match_dev", "match"):
            calls.append((what + " / " + which, ppf_call(tdv, which, ctx, o, **kw)))
    for thr in BAD_THR:
        for which in ("match_dev", "match"):
            calls.append(("thr %r / %s" % (thr, which), ppf_call(tdv, which, ctx, o, thr=thr)))
    for which in ("bytes", "model", "match_dev", "match"):
        calls.append(("NULL params / " + which, ppf_call(tdv, which, ctx, o, prm=False)))
        calls.append(("nt < 0 / " + which, ppf_call(tdv, which, ctx, o, nt=-1)))
        calls.append(("nt > max / " + which, ppf_call(tdv, which, ctx, o, nt=tdv.TDV_PPF_MODEL_MAX + 1)))
    for which in ("model", "match_dev", "match"):
        calls.append(("NULL model cloud / " + which, ppf_call(tdv, which, ctx, o, tgt=False)))
        calls.append(("NULL model normals / " + which, ppf_call(tdv, which, ctx, o, tn=False)))
    for which in ("match_dev", "match"):
        calls.append(("ns < 0 / " + which, ppf_call(tdv, which, ctx, o, ns=-1)))
        calls.append(("NULL scene / " + which, ppf_call(tdv, which, ctx, o, src=False)))
        calls.append(("NULL scene normals / " + which, ppf_call(tdv, which, ctx, o, sn=False)))
        calls.append(("NULL poses / " + which, ppf_call(tdv, which, ctx, o, poses=False)))
        calls.append(("NULL n_poses / " + which, ppf_call(tdv, which, ctx, o, n_poses=False)))
    for which in ("model", "match_dev"):
        calls.append(("NULL info / " + which, ppf_call(tdv, which, ctx, o, info=False)))
        calls.append(("NULL d_model / " + which, ppf_call(tdv, which, ctx, o, model=False)))
        calls.append(("misaligned d_model / " + which, ppf_call(tdv, which, ctx, o, model="odd")))
    calls.append(("model_bytes too small", ppf_call(tdv, "model", ctx, o, model_bytes=1000)))
    for what, gi in (("nt", dict(nt=5)), ("n_keys", dict(n_keys=17)), ("n_pairs < 0", dict(n_pairs=-1)), ("n_pairs > cap", dict(n_pairs=13)),
                     ("diameter nan", dict(diameter=NAN)), ("diameter < 0", dict(diameter=-1.0)), ("step inf", dict(distance_step=INF)),
                     ("step < 0", dict(distance_step=-0.1))):
        calls.append(("info: " + what, ppf_call(tdv, "match_dev", ctx, o, good_info=gi)))
    return o, calls


def test_bad_arguments_leave_outputs_untouched(tdv):
    """With a NULL ctx (a real ctx needs a device: tests/test_gpu_ppf.py runs the same list on one).  tdv_ppf_model_bytes takes no ctx: its
    refusals are the parameters' own, and a good call right after them still answers."""
    o, calls = refusals(tdv, None)
    for what, status in calls:
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()
    assert tdv.lib().tdv_ppf_model_bytes(4, C.byref(tdv.ppf_params()), None) == TDV_ERR_BAD_ARG
    assert ppf_call(tdv, "bytes", None, o) == 0 and o.bytes.value > 0


# ---------------------------------------------------------------- the restatement alone on the shared scene
def restatement_speaks_of_the_library(tdv, model):
    """The restatement's parameters, key space, table size and peak record are the library's: a test on the restatement alone would
    otherwise say nothing about it."""
    p = tdv.ppf_params()
    assert {k: (F(v) if isinstance(v, float) else v) for k, v in model["params"].items()} == {k: getattr(p, k) for k, _ in tdv.PpfParamsC._fields_}
    assert R.PEAK == tdv.PPF_PEAK_DTYPE
    b = C.c_size_t()
    assert tdv.lib().tdv_ppf_model_bytes(model["nt"], C.byref(p), C.byref(b)) == 0
    assert b.value == 4 * ((model["n_keys"] + 1 + 3) // 4 * 4 + 2 * model["nt"] * (model["nt"] - 1)) and model["n_pairs"] <= model["nt"] * (model["nt"] - 1)


def test_restatement_finds_the_pose_and_icp_refines_it(tdv, orc, synth):
    sc = S.build(synth)
    assert 250 <= len(sc["model"]) <= 350 and 1300 <= len(sc["scene"]) <= 1700
    ref = S.restated(synth)
    model, poses = ref["model"], ref["poses"]
    assert model["n_pairs"] > 50000 and len(poses) >= 2
    restatement_speaks_of_the_library(tdv, model)
    scored = [R.score(orc.icp_correspondences(sc["scene"], sc["model"], sc["model_normals"], p["T"], S.THR)) for p in poses]
    best = max(range(len(poses)), key=lambda k: scored[k][1])
    ang, tr = synth.pose_error(poses[best]["T"], sc["T_gt"])
    print("best-fitness pose %d of %d: votes %d, members %d, fitness %.3f, angle %.4f rad, translation %.5f m" %
          (best, len(poses), poses[best]["votes"], poses[best]["members"], scored[best][1], ang, tr))
    assert ang <= 2.0 * np.pi / 30.0 and tr <= 0.1 * float(model["diameter"])
    fine = orc.icp(sc["scene"], sc["model"], sc["model_normals"], poses[best]["T"], S.THR, S.ICP_ITERS, True)
    ang_f, tr_f = synth.pose_error(fine["T"], sc["T_gt"])
    print("ICP: %d iterations, fitness %.3f, angle %.5f rad, translation %.2e m" % (fine["iterations"], fine["fitness"], ang_f, tr_f))
    assert ang_f < 1e-2 and tr_f < 1e-3                              # the bounds of tests/test_oracle_chain.py


def test_restatement_properties(tdv, synth):
    """What the rules promise, checked on the restatement itself: the table's order is total and its offsets index it; a model with
    negated normals and flip_model_normals is the model."""
    sc = S.build(synth)
    m = S.restated(synth)["model"]
    restatement_speaks_of_the_library(tdv, m)
    k = m["key"].astype(np.int64) * (1 << 32) + m["pair"]
    assert (np.diff(k) > 0).all()
    off = m["offsets"]
    assert off[0] == 0 and off[-1] == m["n_pairs"] and (np.diff(off) >= 0).all()
    some = np.flatnonzero(np.diff(off))[::97]
    for key in some:
        assert (m["key"][off[key]:off[key + 1]] == key).all()
    flipped = R.model_table(sc["model"], -sc["model_normals"], flip_model_normals=1)
    for name in ("offsets", "pair", "alpha_bits", "key"):
        assert flipped[name].tobytes() == m[name].tobytes(), name
