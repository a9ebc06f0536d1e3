"""Shared by the GPU tests of tdv_ppf_match_batch_dev: the instances (tests/ppf_scene.py: build(synth, 3, k), one model, a scene per k), and
the batch and its reference - the single call tdv_ppf_match_dev on each instance - through the device entry points on the buffers of a
state_cases.Env.  Both sides use one upload of the clouds back to back and one table; the single calls take pointers into that upload."""
import numpy as np

import ppf_restatement as R
import ppf_scene as S

F = np.float32
EIGHT = (2, 4, 5, 1, 7, 8, 9, 10)          # instance 1 fourth: its peaks are the restatement's (ppf_scene.restated)
_SCENES = {}


def scene(synth, k):
    """build(synth, 3, k), once per process and read-only."""
    if k not in _SCENES:
        _SCENES[k] = S.build(synth, 3, k)
    return _SCENES[k]


def clouds_of(synth, ks):
    return [(scene(synth, k)["scene"], scene(synth, k)["scene_normals"]) for k in ks]


def blob(res, more):
    return [(r.transformation.tobytes(), F(r.fitness).tobytes(), F(r.rmse).tobytes(), r.n_corr, tuple(sorted(m.items()))) for r, m in zip(res, more)]


class Setup:
    """The clouds of a batch and the model on the device, and the model's table for `kw`."""

    def __init__(self, ctx, env, clouds, model, model_normals, **kw):
        self.ctx, self.env, self.kw = ctx, env, kw
        self.ns = [len(p) for p, _ in clouds]
        self.off = np.zeros(len(clouds) + 1, np.int32)
        self.off[1:] = np.cumsum(self.ns)
        stride = kw.get("ref_stride", 5)
        self.n_ref = [(n + stride - 1) // stride for n in self.ns]
        self.peak_off = np.zeros(len(clouds) + 1, np.int32)
        self.peak_off[1:] = np.cumsum(self.n_ref)
        cat = lambda i: np.concatenate([np.asarray(c[i], F).reshape(-1, 3) for c in clouds] + [np.zeros((1, 3), F)])   # noqa: E731 (never empty)
        self.d_src, self.d_sn = env.up(cat(0)), env.up(cat(1))
        self.nt = len(model)
        self.d_tgt, self.d_tn = env.up(np.asarray(model, F)), env.up(np.asarray(model_normals, F))
        nbytes = ctx.ppf_model_bytes(self.nt, **kw)
        self.table = env.out(nbytes, np.uint8)
        self.info = ctx.ppf_model_dev(self.d_tgt, self.d_tn, self.nt, self.table.data_ptr(), nbytes, **kw)

    def batch(self, thr=S.THR, peaks=True):
        """One tdv_ppf_match_batch_dev call: [(pose blob, peaks) per instance], and the peak offsets it returned."""
        total = int(self.peak_off[-1])
        d_pk = self.env.out(total + 1, R.PEAK)
        out, peak_off = self.ctx.ppf_match_batch_dev(self.d_src, self.d_sn, self.off, self.d_tgt, self.d_tn, self.nt, self.table.data_ptr(), self.info,
                                                     thr, d_peaks=d_pk.data_ptr() if peaks else None, **self.kw)
        pk = self.env.get(d_pk, total + 1, R.PEAK)
        assert pk[total:].tobytes() == b"\xA5" * 16, "the call wrote past the last peak"
        if not peaks:
            assert pk.tobytes() == b"\xA5" * (16 * (total + 1))
        self.results = [res for res, _ in out]
        return [(blob(res, more), pk[peak_off[b]:peak_off[b + 1]]) for b, (res, more) in enumerate(out)], peak_off

    def singles(self, thr=S.THR):
        """tdv_ppf_match_dev on each instance alone: [(pose blob, peaks)]; an instance for which the call is accepted and empty has no peak."""
        d_pk = self.env.out(int(self.peak_off[-1]) + 1, R.PEAK)
        got = []
        for b, ns in enumerate(self.ns):
            res, more, n_ref = self.ctx.ppf_match_dev(self.d_src + 12 * int(self.off[b]), self.d_sn + 12 * int(self.off[b]), ns, self.d_tgt, self.d_tn,
                                                      self.nt, self.table.data_ptr(), self.info, thr,
                                                      d_peaks=d_pk.data_ptr() + 16 * int(self.peak_off[b]), **self.kw)
            assert n_ref in (0, self.n_ref[b])
            got.append((blob(res, more), n_ref))
        pk = self.env.get(d_pk, int(self.peak_off[-1]) + 1, R.PEAK)
        return [(bl, pk[self.peak_off[b]:self.peak_off[b] + n_ref]) for b, (bl, n_ref) in enumerate(got)]


def same(want, got, what):
    """Two lists of (pose blob, peaks), byte for byte."""
    assert len(want) == len(got), (what, len(want), len(got))
    for b, ((wb, wp), (gb, gp)) in enumerate(zip(want, got)):
        bad = np.flatnonzero(wp != gp) if wp.shape == gp.shape else None
        assert bad is not None and len(bad) == 0, (what, "peaks of instance", b, wp.shape, gp.shape, None if bad is None else (wp[bad[:4]], gp[bad[:4]]))
        assert len(wb) == len(gb), (what, "poses of instance", b, len(wb), len(gb))
        for k, (w, g) in enumerate(zip(wb, gb)):
            assert w == g, (what, "instance", b, "pose", k, w[3:], g[3:])
