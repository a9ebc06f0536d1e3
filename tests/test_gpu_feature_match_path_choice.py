"""Which search answers a descriptor match, at the sizes where the answer changes (csrc/fmatch.hip: fm_wants_index,
fm_indexes_sources): the packed index from 4,096 sources and 2,048 targets on, the plain scan one row below either, and the two
switches that are read per call.  Every result is the oracle's, through the host entry point and the device-resident one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INDEXED = ("leaf_major", "walk")
SIZES = [((4095, 2048), ("scan",)), ((4096, 2047), ("scan",)), ((4096, 2048), INDEXED)]
_cases = {}


def _case(synth, orc, ns, nt):
    """(sources, targets, the oracle's correspondences), computed once per size."""
    if (ns, nt) not in _cases:
        fs, ft = synth.random_features(ns, 11), synth.random_features(nt, 12)
        _cases[ns, nt] = (fs, ft, orc.feature_match(fs, ft))
    return _cases[ns, nt]


def _match_host(ctx, fs, ft):
    return ctx.feature_match(fs, ft)


def _match_dev(ctx, fs, ft):
    d_fs, d_ft = torch.from_numpy(fs).to(DEV), torch.from_numpy(ft).to(DEV)
    d_c = torch.full((len(fs),), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()                       # filled on the null stream; the ctx works on its own non-blocking stream
    ctx.feature_match_dev(d_fs.data_ptr(), len(fs), d_ft.data_ptr(), len(ft), d_c.data_ptr())
    ctx.synchronize()
    return d_c.cpu().numpy()


@pytest.mark.parametrize("match", [_match_host, _match_dev], ids=["host", "dev"])
@pytest.mark.parametrize("size,paths", SIZES, ids=["%dx%d" % s for s, _ in SIZES])
def test_path_by_size(ctx, orc, synth, match, size, paths):
    fs, ft, ref = _case(synth, orc, *size)
    got = match(ctx, fs, ft)
    assert ctx.last_feature_match_path() in paths, ctx.last_feature_match_path()
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("match", [_match_host, _match_dev], ids=["host", "dev"])
@pytest.mark.parametrize("knob,value,path", [("TDV_FM_BRUTE", "1", "scan"), ("TDV_FM_LEAFMAJOR", "0", "walk")])
def test_switches_read_per_call(ctx, orc, synth, match, knob, value, path):
    fs, ft, ref = _case(synth, orc, 4096, 2048)
    saved = {k: os.environ.get(k) for k in ("TDV_FM_BRUTE", "TDV_FM_LEAFMAJOR")}
    try:
        for k in saved:
            os.environ.pop(k, None)
        os.environ[knob] = value
        got = match(ctx, fs, ft)
        assert ctx.last_feature_match_path() == path, ctx.last_feature_match_path()
        assert np.array_equal(got, ref), int((got != ref).sum())
        del os.environ[knob]
        match(ctx, fs, ft)                          # the switch is gone: the next call is an indexed one again
        assert ctx.last_feature_match_path() in INDEXED, ctx.last_feature_match_path()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
