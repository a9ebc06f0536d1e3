"""CPU suite: tdv_ppf_match_batch_dev (include/tdv_hip.h: tdv_ppf_match, the batch paragraph).  The ABI exports the entry point and lists it
in ABI_SYMBOLS; it refuses every bad argument of tdv_ppf_match_dev and those of its own (a negative count, missing, shifted or decreasing
offsets, counts beyond INT_MAX) before it writes anything; Context.ppf_match_batch refuses instances whose normals do not match their points
before it touches a device.  No compute entry point runs here; tests/test_gpu_ppf_batch.py holds the batch to the single call."""
import ctypes as C

import numpy as np
import pytest

import ppf_restatement as R
from test_ppf_abi import BAD, BAD_THR, INF, NAN, P, TDV_ERR_BAD_ARG

F = np.float32
INT_MAX = 2 ** 31 - 1


class BatchOutputs:
    """Every host output of the batch call, filled with a pattern; untouched() compares them with it (test_ppf_abi.Outputs, for a batch of
    up to `n` instances)."""

    def __init__(self, tdv, n=4, n_ref=8, fill=0x5A):
        self.poses = (tdv.PpfPoseC * (n * tdv.TDV_PPF_POSES_MAX))(); C.memset(self.poses, fill, C.sizeof(self.poses))
        self.n_poses = np.full(n, -7, np.int32)
        self.peak_off = np.full(n + 1, -7, np.int32)
        self.peaks = np.full(n_ref, -7, R.PEAK)
        self.before = self.snapshot()

    def snapshot(self):
        return bytes(self.poses), self.n_poses.tobytes(), self.peak_off.tobytes(), self.peaks.tobytes()

    def untouched(self):
        return self.snapshot() == self.before


GOOD_OFF = (0, 2, 2, 4)


def batch_call(tdv, ctx, o, off=GOOD_OFF, n=None, src=None, sn=None, tgt=None, tn=None, nt=4, thr=0.01, model=None, info=True, prm=True, poses=True,
               n_poses=True, good_info=None, dev=None, **kw):
    """tdv_ppf_match_batch_dev with one argument made bad.  A refused call must not look at its arrays: with a NULL ctx host arrays stand in
    every pointer slot; on a real ctx `dev` (device_buffers in tests/test_gpu_ppf.py) puts device memory there, so that a refusal that went
    missing would run on valid buffers and fail the test instead of faulting."""
    lib = tdv.lib()
    p = tdv.ppf_params(**kw)
    h_off = None if off is None else np.asarray(off, np.int32)
    n = (len(h_off) - 1 if h_off is not None else 0) if n is None else n
    z = dev["cloud"] if dev else np.zeros((max(int(h_off[-1]) if h_off is not None and len(h_off) and 0 < h_off[-1] < 4096 else 4, nt, 1), 3), F)
    src, sn, tgt, tn = (z if a is None else (None if a is False else a) for a in (src, sn, tgt, tn))
    model = ((dev["model"] if dev else np.zeros(1 << 20, np.uint32)) if model is None else (None if model is False else model))
    if isinstance(model, str):                                       # "odd": a misaligned pointer
        model = (dev["model"] if dev else np.zeros(64, np.uint8).ctypes.data) + 1
    gi = tdv.PpfModelInfoC(**dict(dict(diameter=1.0, distance_step=0.05, n_pairs=0, n_keys=R.key_space(R.params())[1], nt=nt), **(good_info or {})))
    return lib.tdv_ppf_match_batch_dev(ctx, P(src), P(sn), P(h_off), n, P(tgt), P(tn), nt, P(model), C.byref(gi) if info else None, C.c_float(thr),
                                       C.byref(p) if prm else None, o.poses if poses else None, P(o.n_poses) if n_poses else None,
                                       P(dev["peaks"] if dev else o.peaks), P(o.peak_off))


def too_many_slots(tdv, ctx, o, dev=None):
    """2^25 + 1 empty instances at 64 poses each: 2^31 + 64 pose slots.  (The other count the header names, the sum of the instances'
    reference points, cannot pass INT_MAX while the offsets are ints - ceil(n / ref_stride) <= n - so no call reaches that refusal.)"""
    n = INT_MAX // 64 + 2
    return batch_call(tdv, ctx, o, off=np.zeros(n + 1, np.int32), max_poses=64, dev=dev)


def batch_refusals(tdv, ctx, dev=None):
    """Every refusal the header names for the batch, as (what, status) - on `ctx` (NULL here; a real one in tests/test_gpu_ppf_batch.py)."""
    o = BatchOutputs(tdv)
    call = lambda **kw: batch_call(tdv, ctx, o, dev=dev, **kw)   # noqa: E731
    calls = [(what, call(**kw)) for what, kw in BAD]
    calls += [("thr %r" % thr, call(thr=thr)) for thr in BAD_THR]
    calls += [("NULL params", call(prm=False)), ("nt < 0", call(nt=-1)), ("nt > max", call(nt=tdv.TDV_PPF_MODEL_MAX + 1)),
              ("NULL model cloud", call(tgt=False)), ("NULL model normals", call(tn=False)), ("NULL scene", call(src=False)),
              ("NULL scene normals", call(sn=False)), ("NULL poses", call(poses=False)), ("NULL n_poses", call(n_poses=False)),
              ("NULL info", call(info=False)), ("NULL d_model", call(model=False)), ("misaligned d_model", call(model="odd"))]
    for what, gi in (("nt", dict(nt=5)), ("n_keys", dict(n_keys=17)), ("n_pairs < 0", dict(n_pairs=-1)), ("n_pairs > cap", dict(n_pairs=13)),
                     ("diameter nan", dict(diameter=NAN)), ("diameter < 0", dict(diameter=-1.0)), ("step inf", dict(distance_step=INF)),
                     ("step < 0", dict(distance_step=-0.1))):
        calls.append(("info: " + what, call(good_info=gi)))
    # the batch's own
    calls += [("n_instances < 0", call(n=-1)), ("NULL offsets", call(off=None, n=3)), ("offsets start at 1", call(off=(1, 2, 3, 4))),
              ("offsets start below 0", call(off=(-1, 2, 3, 4))), ("offsets decrease", call(off=(0, 3, 2, 4))),
              ("offsets decrease at the end", call(off=(0, 2, 4, 3))), ("n_instances * max_poses beyond INT_MAX", too_many_slots(tdv, ctx, o, dev))]
    return o, calls


def test_symbol_is_exported_and_listed(tdv):
    assert hasattr(tdv.lib(), "tdv_ppf_match_batch_dev")
    assert "tdv_ppf_match_batch_dev" in tdv.ABI_SYMBOLS
    header = open(tdv.LIB_PATH.rsplit("/3dvision_amd/", 1)[0] + "/include/tdv_hip.h").read()
    assert "int tdv_ppf_match_batch_dev(" in header
    assert callable(tdv.Context.ppf_match_batch_dev) and callable(tdv.Context.ppf_match_batch)


def test_bad_arguments_leave_outputs_untouched(tdv):
    """With a NULL ctx (tests/test_gpu_ppf_batch.py runs the same list on a real one)."""
    o, calls = batch_refusals(tdv, None)
    assert len(calls) > 50
    for what, status in calls:
        assert status == TDV_ERR_BAD_ARG, what
    assert o.untouched()


def test_mismatched_normals_raise_before_a_device_is_touched(tdv):
    """Context.ppf_match_batch on an object that has no ctx: the check comes first, so nothing else is reached."""
    c = tdv.Context.__new__(tdv.Context)
    c._h = C.c_void_p()
    pts = [np.zeros((5, 3), F), np.zeros((3, 3), F)]
    with pytest.raises(ValueError):
        c.ppf_match_batch(pts, [np.zeros((5, 3), F), np.zeros((4, 3), F)], np.zeros((4, 3), F), np.zeros((4, 3), F), 0.01)
    with pytest.raises(ValueError):
        c.ppf_match_batch(pts, [np.zeros((5, 3), F)], np.zeros((4, 3), F), np.zeros((4, 3), F), 0.01)
    with pytest.raises(ValueError):
        c.ppf_match_batch(pts, pts, np.zeros((4, 3), F), np.zeros((3, 3), F), 0.01)
