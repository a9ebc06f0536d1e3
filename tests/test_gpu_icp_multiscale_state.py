"""tdv_voxel_downsample_normals(_dev) and tdv_icp_multiscale(_dev, _batch_dev) under the conditions tests/test_gpu_ctx_state.py sets for
the other entry points: their outputs are a function of the arguments and the ctx's settings only, never of what the ctx did before or of
the stream it runs on.  The baseline - every call's outputs as bytes, taken once on a context of its own (and tied to the stagewise chain
and the oracle by tests/test_gpu_icp_multiscale.py and tests/test_gpu_voxel_normals.py) - must come back on a workspace poisoned with 0x00
and 0xFF, after a larger call has grown the arena, right after a bad-argument return, and on a caller's stream.  The level clouds of a
schedule live in the workspace and every level rewinds it: what a level leaves behind is exactly what the next one is handed.
Device buffers go through state_cases.Env and StreamEnv."""
import ctypes as C

import numpy as np
import pytest
import torch

from state_cases import DEV, Env, StreamEnv
from test_gpu_icp_multiscale import N, bits, levels_of, schedule

pytestmark = pytest.mark.gpu
F = np.float32
OFF = np.array([0, 700, 700, 701, 3000], np.int32)          # the batch: the scan's rows as four clouds, one empty, one of a single point
BAD_ARG = -2


@pytest.fixture(scope="module")
def case(tdv, synth):
    tgt, nrm = synth.sample_object(N, 42)
    src, T_gt = synth.make_scene(N, 101)
    D = dict(tgt=tgt, nrm=nrm, src=src, T0=synth.perturb(T_gt, seed=201, angle_deg=6.0, trans=0.01), sched=schedule(synth),
             rgb=np.random.default_rng(5).random((N, 3)).astype(F))
    c = tdv.Context(0)
    try:
        D["sn"] = c.estimate_normals(src, 30)
        for v in D.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        D["base"] = calls(tdv, c, Env(c), D)
    finally:
        c.close()
    return D


def calls(tdv, ctx, env, D):
    """Every new entry point once; everything they return, as bytes."""
    out = {}
    voxel = D["sched"][1][0]
    for order in (tdv.TDV_VOXEL_ORDER_FIRST, tdv.TDV_VOXEL_ORDER_REFERENCE):
        ox, on, oc = env.out(3 * N, F), env.out(3 * N, F), env.out(3 * N, F)
        m = ctx.voxel_downsample_normals_dev(env.up(D["tgt"]), env.up(D["nrm"]), N, voxel, ox.data_ptr(), on.data_ptr(), N, env.up(D["rgb"]), oc.data_ptr(), order)
        out["voxel_dev", order] = (m, env.get(ox, 3 * m, F).tobytes(), env.get(on, 3 * m, F).tobytes(), env.get(oc, 3 * m, F).tobytes())
        out["voxel_host", order] = tuple(a.tobytes() for a in ctx.voxel_downsample_normals(D["tgt"], D["nrm"], voxel, D["rgb"], order))
        assert out["voxel_host", order] == out["voxel_dev", order][1:]
    ps, psn, pt, ptn = env.up(D["src"]), env.up(D["sn"]), env.up(D["tgt"]), env.up(D["nrm"])
    for est in ("point_to_plane", "gicp"):
        lv = levels_of(tdv, D["sched"])
        sn = psn if est == "gicp" else None
        out["dev", est] = [bits(l) for l in ctx.multi_scale_icp_dev(ps, N, pt, ptn, N, D["T0"], estimation=est, d_src_normals=sn, levels=lv).levels]
        out["host", est] = [bits(l) for l in ctx.multi_scale_icp(D["src"], D["tgt"], None, None, D["T0"], estimation=est, target_normals=D["nrm"],
                                                                 source_normals=D["sn"] if est == "gicp" else None, levels=lv).levels]
        out["batch", est] = [[bits(l) for l in r.levels]
                             for r in ctx.multi_scale_icp_batch_dev(ps, OFF, pt, ptn, N, np.stack([D["T0"]] * 4), estimation=est, d_src_normals=sn, levels=lv)]
        assert out["host", est] == out["dev", est]
    return out


def held(tdv, ctx, case, what, env=None):
    got = calls(tdv, ctx, env or Env(ctx), case)
    for k, v in case["base"].items():
        assert got[k] == v, (what, k)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poisoned_workspace(tdv, case, byte):
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")                              # ... and the arena and staging now cover the calls
        ctx.workspace_fill(byte)
        before = ctx.workspace_high_water()
        held(tdv, ctx, case, "workspace filled with 0x%02X" % byte)
        assert ctx.workspace_high_water() == before, "the calls grew the workspace: part of what they used was not poisoned"
    finally:
        ctx.close()


def test_after_a_larger_call_has_grown_the_arena(tdv, case):
    ctx = tdv.Context(0)
    try:
        held(tdv, ctx, case, "first calls")
        small = ctx.workspace_high_water()
        rng = np.random.default_rng(3)
        big = rng.random((1500000, 3)).astype(F); big_n = rng.normal(size=big.shape).astype(F)
        x, n, _ = ctx.voxel_downsample_normals(big, big_n, 0.01, None, tdv.TDV_VOXEL_ORDER_FIRST)
        assert len(x) == len(n) > 500000 and ctx.workspace_high_water() > max(small, 64 << 20)      # past the first block
        held(tdv, ctx, case, "after the larger call")                    # the call that coalesces the blocks, and those after it
    finally:
        ctx.close()


def test_after_a_bad_argument_return(tdv, case):
    ctx = tdv.Context(0)
    lib = tdv.lib()
    try:
        held(tdv, ctx, case, "first calls")
        env = Env(ctx)
        ps, pt, ptn = env.up(case["src"]), env.up(case["tgt"]), env.up(case["nrm"])
        T0 = (C.c_float * 16)(*tdv.to_colmajor16(case["T0"]))
        lv = levels_of(tdv, case["sched"][::-1])                          # voxel sizes that grow, and a non-last level as given
        out = (tdv.IcpLevelResultC * 12)(); C.memset(out, 0x5A, C.sizeof(out)); before = bytes(out)
        v = C.c_void_p
        assert lib.tdv_icp_multiscale_dev(ctx._h, v(ps), None, N, v(pt), v(ptn), N, T0, lv, 3, 0, C.c_float(1e-3), out) == BAD_ARG
        assert bytes(out) == before
        held(tdv, ctx, case, "right after a bad-argument return of the device entry point")
        off = (C.c_int * 5)(*OFF[::-1])
        assert lib.tdv_icp_multiscale_batch_dev(ctx._h, v(ps), None, off, 4, v(pt), v(ptn), N, T0, levels_of(tdv, case["sched"]), 3, 0, C.c_float(1e-3), out) == BAD_ARG
        assert bytes(out) == before
        held(tdv, ctx, case, "right after a bad-argument return of the batch entry point")
        m = C.c_int(77)
        ox = env.out(3 * N, F)
        assert lib.tdv_voxel_downsample_normals_dev(ctx._h, v(pt), v(ptn), None, N, C.c_float(-1.0), 0, v(ox.data_ptr()), v(ox.data_ptr()), None, N, C.byref(m)) == BAD_ARG
        held(tdv, ctx, case, "right after a bad-argument return of the voxel entry point")
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
        held(tdv, ctx, case, "a caller's stream (%s)" % kind, StreamEnv(ctx, ts))
    finally:
        ctx.close()
        torch.cuda.synchronize()
