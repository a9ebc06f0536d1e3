"""tdv_iss_keypoints and tdv_iss_keypoints_dev under the conditions tests/test_gpu_ctx_state.py sets for the other entry points: their
outputs are a function of the arguments only, never of what the ctx did before or of the stream it runs on.  Both entry points are held
to the restatement (tests/iss_restatement.py) byte for byte - at given radii, and at the default radii through the reported resolution,
as tests/test_gpu_iss.py does - on a workspace poisoned with 0x00 and 0xFF, after a larger call has grown the arena, right after a
bad-argument return, and on a caller's stream.  Device buffers go through state_cases.Env and StreamEnv."""
import numpy as np
import pytest
import torch

import iss_restatement as R
from state_cases import DEV, Env, StreamEnv
from test_gpu_iss import same
from test_iss_abi import Outputs, iss_call

pytestmark = pytest.mark.gpu
F = np.float32
N, WIDTH = 5000, 4
GIVEN = dict(salient_radius=0.009, non_max_radius=0.006)


@pytest.fixture(scope="module")
def case(synth):
    """The cloud, its attr rows, and the restatement at the given radii (computed once, never modified)."""
    pts = synth.sample_object(N, 21)[0].astype(np.float64)
    pts = (pts + np.random.default_rng(21).normal(0, 2e-4, pts.shape) + [0.1, -0.2, 0.6]).astype(F)
    pts[17] = np.nan; pts[4000, 1] = np.inf
    attr = np.random.default_rng(22).random((N, WIDTH)).astype(F)
    ref = R.iss(pts, attr, **GIVEN)
    assert ref["n_keypoints"] > 30
    exact = R.resolution(pts)[0]
    for a in (pts, attr):
        a.setflags(write=False)
    return dict(pts=pts, attr=attr, ref=ref, exact=exact, default_refs={})


def _dev(ctx, env, case, **params):
    om, os_, oe, ou = env.out(N, np.uint8), env.out(N, np.float64), env.out(3 * N, np.float64), env.out(N, np.int32)
    oi, ox, oa = env.out(N, np.int32), env.out(3 * N, F), env.out(WIDTH * N, F)
    res = ctx.iss_keypoints_dev(env.up(case["pts"]), N, env.up(case["attr"]), WIDTH, om.data_ptr(), os_.data_ptr(), oe.data_ptr(), ou.data_ptr(),
                                oi.data_ptr(), ox.data_ptr(), oa.data_ptr(), **params)
    m = res["n_keypoints"]
    return dict(res, mask=env.get(om, N, np.uint8), saliency=env.get(os_, N, np.float64), eigenvalues=env.get(oe, 3 * N, np.float64).reshape(-1, 3),
                support=env.get(ou, N, np.int32), index=env.get(oi, m, np.int32), xyz=env.get(ox, 3 * m, F).reshape(-1, 3),
                attr=env.get(oa, WIDTH * m, F).reshape(m, WIDTH))


def held(ctx, case, what, env=None):
    """Host and device entry points, at the given and at the default radii, against the restatement."""
    env = env or Env(ctx)
    for name, call in (("host", lambda **kw: ctx.iss(case["pts"], case["attr"], **kw)), ("dev", lambda **kw: _dev(ctx, env, case, **kw))):
        got = call(**GIVEN)
        same(case["ref"], got, (what, name, "given radii"))
        assert np.isnan(got["resolution"])
        got = call()
        res = np.float64(got["resolution"])
        assert abs(res - case["exact"]) <= R.resolution_bound(case["exact"], N), (what, name, res, case["exact"])
        rs, rn = R.default_radii(res)
        key = (F(rs).tobytes(), F(rn).tobytes())
        if key not in case["default_refs"]:
            case["default_refs"][key] = R.iss(case["pts"], case["attr"], salient_radius=rs, non_max_radius=rn)
        same(case["default_refs"][key], got, (what, name, "default radii"))


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_workspace(tdv, case, byte):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")                                   # ... and the arena and staging now cover the calls
        ctx.workspace_fill(byte)
        before = ctx.workspace_high_water()
        held(ctx, case, "workspace filled with 0x%02X" % byte)
        assert ctx.workspace_high_water() == before, "the calls grew the workspace: part of what they used was not poisoned"
    finally:
        ctx.close()


def test_after_a_larger_call_has_grown_the_arena(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        small = ctx.workspace_high_water()
        big = np.random.default_rng(3).random((400000, 3)).astype(F)
        r = ctx.iss(big, np.zeros((len(big), 33), F), salient_radius=0.02, non_max_radius=0.015)
        assert r["n_finite"] == len(big) and ctx.workspace_high_water() > max(small, 64 << 20)      # past the first block
        held(ctx, case, "after the larger call")                         # the call that coalesces the blocks, and those after it
    finally:
        ctx.close()


def test_after_a_bad_argument_return(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(ctx, case, "first calls")
        for dev in (False, True):
            o = Outputs(tdv, N, WIDTH)
            assert iss_call(tdv.lib(), dev, ctx._h, case["pts"], case["attr"], N, o, attr_width=WIDTH, salient_radius=0.0) == -2
            assert o.untouched()
            held(ctx, case, "right after a bad-argument return of the %s entry point" % ("device" if dev else "host"))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["null", "torch"])
def test_callers_stream(tdv, case, kind):
    torch.cuda.synchronize()
    ts = torch.cuda.default_stream(DEV) if kind == "null" else torch.cuda.Stream(DEV)
    handle = int(ts.cuda_stream)
    ctx = tdv.Context(0, stream=handle)
    try:
        assert int(ctx.stream or 0) == handle
        held(ctx, case, "a caller's stream (%s)" % kind, StreamEnv(ctx, ts))
    finally:
        ctx.close()
        torch.cuda.synchronize()
