"""Depth odometry on the device (include/tdv_hip.h: tdv_depth_odometry_dev, rules O1 to O9) against the restatement
(tests/odometry_restatement.py), byte for byte: the maps, the compacted rows and their count with the three capacity forms; the pyramid
through every level's count of valid pixels and sums; the 29 sums at several poses and levels; the whole result of a pair, host and
device form; the sequence's poses and pairs, and pair-by-pair equality with the single call.  Shapes: width*height one below, at and
one above a workgroup and two (17x15, 16x16, 257x1, 1x257), odd sides (33x17, 65x47), 1x1 and 2x2, and the rendered pairs of
tests/odometry_cases.py at 96x72 and 160x120 with 1 to 3 levels.  The accuracy condition is the restatement's (tests/test_odometry_abi.py);
the device inherits it through byte equality and is given no tolerance of its own."""
import numpy as np
import pytest

import odometry_cases as K
import odometry_restatement as R
from state_cases import Env
from test_odometry_abi import BAD, NULLS, Outputs, odom_call

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(17, 15), (16, 16), (257, 1), (1, 257), (33, 17), (65, 47), (1, 1), (2, 2)]
SCALE = 1000.0


def frame(w, h, seed):
    """A smooth surface around 0.5 m with a step, holes (0) and a patch beyond any zmax used here (3 m); uint16 [h, w], scale 1000."""
    rng = np.random.default_rng(1000 * w + h + 7)                                 # holes: the same in every frame of a shape
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 0.5 + 0.04 * np.sin(0.31 * u + 0.05 * seed) * np.cos(0.23 * v) + 0.03 * u / max(w, 1) + 0.0007 * seed
    z[:, (2 * w) // 3:] += 0.08                                                    # a step well above the default depth_diff
    raw = np.round(z * SCALE).astype(np.uint16)
    raw[rng.random((h, w)) < 0.04] = 0
    raw[h // 2:h // 2 + 2, w // 4:w // 4 + 3] = 3000
    return raw


def intrinsics(w, h):
    f = 1.1 * max(w, h, 8)
    return (SCALE, f, 1.05 * f, (w - 1) / 2.0, (h - 1) / 2.0)


def max_levels(w, h):
    n = 1
    while n < R.MAX_LEVELS and (min(w, h) >> n) >= 1:
        n += 1
    return n


def small_pose(seed=1, angle=0.4, trans=0.001):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    return K.synth.make_transform(axis / np.linalg.norm(axis), angle, tuple(trans * rng.normal(size=3))).astype(F)


def same_result(got, ref, what):
    assert got["T"].tobytes() == np.asarray(ref["T"], F).tobytes(), (what, got["T"], ref["T"])
    assert F(got["fitness"]).tobytes() == F(ref["fitness"]).tobytes() and F(got["rmse"]).tobytes() == F(ref["rmse"]).tobytes(), (what, got, ref)
    assert (got["n_corr"], got["iterations"], got["n_corr_level"]) == (ref["n_corr"], ref["iterations"], ref["n_corr_level"]), (what, got, ref)


def device_maps(ctx, env, raw, intr, capacity=None, **kw):
    """tdv_depth_maps_dev with every output: dict as R.maps, plus n and fits."""
    h, w = raw.shape
    npx = w * h
    cap = npx if capacity is None else capacity
    vm, nm, ox, on = env.out(3 * npx, F), env.out(3 * npx, F), env.out(3 * max(cap, 1), F), env.out(3 * max(cap, 1), F)
    n, fits = ctx.depth_maps_dev(env.up(raw), w, h, *intr, vm.data_ptr(), nm.data_ptr(), ox.data_ptr() if cap else None,
                                 on.data_ptr() if cap else None, cap, **kw)
    rows = n if fits else 0
    return dict(n=n, fits=fits, vertex_map=env.get(vm, 3 * npx, F).reshape(h, w, 3), normal_map=env.get(nm, 3 * npx, F).reshape(h, w, 3),
                xyz=env.get(ox, 3 * rows, F).reshape(-1, 3), normals=env.get(on, 3 * rows, F).reshape(-1, 3),
                raw_xyz=env.get(ox, 3 * max(cap, 1), F), raw_maps=(env.get(vm, 3 * npx, F), env.get(nm, 3 * npx, F)))


@pytest.mark.parametrize("shape", SHAPES + [(96, 72)], ids=lambda s: "%dx%d" % s)
def test_maps_rows_count_and_capacity_forms(tdv, ctx, shape):
    w, h = shape
    raw = frame(w, h, 0) if shape != (96, 72) else K.pair(shape, 2.0)["src"]
    intr = intrinsics(w, h) if shape != (96, 72) else K.pair(shape, 2.0)["intr"]
    for kw in (dict(), dict(zmax=0.56, depth_diff=0.002)):
        ref = R.maps(raw, intr, **kw)
        n = len(ref["xyz"])
        env = Env(ctx)
        got = device_maps(ctx, env, raw, intr, **kw)
        assert got["fits"] and got["n"] == n, (got["n"], n)
        for k in ("vertex_map", "normal_map", "xyz", "normals"):
            assert got[k].tobytes() == ref[k].tobytes(), (shape, kw, k)
        host = ctx.depth_maps(raw, intr, **kw)
        for k in ("vertex_map", "normal_map", "xyz", "normals"):
            assert host[k].tobytes() == ref[k].tobytes(), (shape, kw, k, "host")
        exact = device_maps(ctx, Env(ctx), raw, intr, capacity=n, **kw)
        assert exact["fits"] and exact["n"] == n and exact["xyz"].tobytes() == ref["xyz"].tobytes()
        query = ctx.depth_maps_dev(Env(ctx).up(raw), w, h, *intr, None, None, None, None, 0, **kw)
        assert query == (n, n == 0)
        if n:
            short = device_maps(ctx, Env(ctx), raw, intr, capacity=n - 1, **kw)
            assert not short["fits"] and short["n"] == n
            pattern = np.full(1, 0xA5A5A5A5, np.uint32).view(F)[0].tobytes()       # Env.out's fill: nothing was written, the maps included
            for a in (short["raw_xyz"],) + short["raw_maps"]:
                assert a.tobytes() == pattern * len(a), "a refused call wrote"
    if w > 1 and h > 1 and shape != (2, 2):
        assert len(R.maps(raw, intr)["xyz"]) > 0
    # no read-back form: maps only
    env = Env(ctx)
    vm = env.out(3 * w * h, F)
    assert ctx.depth_maps_dev(env.up(raw), w, h, *intr, vm.data_ptr(), want_count=False) == (None, True)
    assert env.get(vm, 3 * w * h, F).tobytes() == R.maps(raw, intr)["vertex_map"].tobytes()


def poses_for(shape):
    far = np.eye(4, dtype=F); far[2, 3] = -5.0                                    # every point behind the camera
    out = np.eye(4, dtype=F); out[0, 3] = 50.0                                    # ... out of the frame
    nan = np.eye(4, dtype=F); nan[1, 1] = np.nan
    return [("identity", np.eye(4, dtype=F)), ("small", small_pose()), ("behind", far), ("out of frame", out), ("nan", nan)]


def check_terms(ctx, src, tgt, intr, shape, levels, poses, **kw):
    w, h = shape
    p = R.params(n_levels=levels, **kw)
    ps, pt = R.pyramid(src, intr, p), R.pyramid(tgt, intr, p)
    env = Env(ctx)
    d_src, d_tgt = env.up(src), env.up(tgt)
    hit = 0
    for l in range(levels):
        for name, T in poses:
            got, n_valid = ctx.depth_odometry_terms_dev(d_src, d_tgt, w, h, *intr, T, l, n_levels=levels, **kw)
            ref = R.sums(ps[l], pt[l], T, p)
            assert n_valid == ps[l]["n_valid"], (shape, l, name)
            assert got.tobytes() == ref.tobytes(), (shape, l, name, got, ref)
            if name in ("behind", "out of frame", "nan"):
                assert not got.any(), (shape, l, name)
            hit += int(ref[0])
    return hit


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_sums_and_valid_counts_at_every_level(tdv, ctx, shape):
    w, h = shape
    src, tgt, intr = frame(w, h, 1), frame(w, h, 0), intrinsics(w, h)
    hit = check_terms(ctx, src, tgt, intr, shape, max_levels(w, h), poses_for(shape))
    if min(w, h) > 2:
        assert hit > 0, "no pixel of this shape found a partner: the case shows nothing"
    check_terms(ctx, src, tgt, intr, shape, 1, poses_for(shape)[:2], zmax=0.56, depth_diff=0.0015)


@pytest.mark.parametrize("size", sorted(K.SIZES), ids=lambda s: "%dx%d" % s)
def test_sums_on_the_rendered_pairs(tdv, ctx, size):
    c = K.pair(size, 2.0)
    hit = check_terms(ctx, c["src"], c["tgt"], c["intr"], size, 3, poses_for(size)[:3] + [("truth", c["T_gt"].astype(F))], depth_diff=0.004)
    assert hit > 1000
    check_terms(ctx, c["src"], c["tgt"], c["intr"], size, 2, [("truth", c["T_gt"].astype(F))], zmax=0.301, depth_diff=0.0005)


def check_pair(ctx, orc, src, tgt, intr, what, T0=None, host=True, **kw):
    h, w = src.shape
    ref = R.odometry(orc, src, tgt, intr, T0, **kw)
    env = Env(ctx)
    same_result(ctx.depth_odometry_dev(env.up(src), env.up(tgt), w, h, *intr, T0, **kw), ref, (what, "dev"))
    if host:
        same_result(ctx.depth_odometry(src, tgt, intr, T0, **kw), ref, (what, "host"))
    return ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_result_small_shapes(tdv, ctx, orc, shape):
    w, h = shape
    src, tgt, intr = frame(w, h, 1), frame(w, h, 0), intrinsics(w, h)
    L = max_levels(w, h)
    ref = check_pair(ctx, orc, src, tgt, intr, "all levels", n_levels=L, max_iterations=(4, 3, 2, 2))
    if min(w, h) <= 2:                                                             # no normal at all: the start pose, zeros
        assert ref["T"].tobytes() == np.eye(4, dtype=F).tobytes() and ref["n_corr"] == 0 and not any(ref["iterations"])
    else:
        assert sum(ref["iterations"]) > 0
    T0 = small_pose(3)
    check_pair(ctx, orc, src, tgt, intr, "start pose", T0, n_levels=1, max_iterations=(3,))
    check_pair(ctx, orc, src, tgt, intr, "zmax inside, small depth_diff", T0, host=False, n_levels=1, max_iterations=(2,), zmax=0.56, depth_diff=0.0015)
    for name, T in poses_for(shape)[2:]:
        r = check_pair(ctx, orc, src, tgt, intr, name, T, host=False, n_levels=L, max_iterations=(2, 2, 2, 2))
        assert r["n_corr"] == 0 and not any(r["iterations"]) and r["T"].tobytes() == T.tobytes()
    zeros = np.zeros_like(src)
    for s, t, name in ((zeros, tgt, "a source of zeros"), (src, zeros, "a target of zeros")):
        r = check_pair(ctx, orc, s, t, intr, name, T0, host=False, n_levels=L)
        assert r["n_corr"] == 0 and r["T"].tobytes() == T0.tobytes()


@pytest.mark.parametrize("size", sorted(K.SIZES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_result_rendered_pairs(tdv, ctx, orc, size, levels):
    c = K.pair(size, 2.0 if levels < 3 else 4.0)
    ref = check_pair(ctx, orc, c["src"], c["tgt"], c["intr"], "default iterations", n_levels=levels, depth_diff=K.ACCURACY_DEPTH_DIFF)
    assert ref["iterations"][levels - 1] > 0 and ref["n_corr"] > 500
    if levels == 3:
        check_pair(ctx, orc, c["src"], c["tgt"], c["intr"], "levels skipped", host=False, n_levels=3, max_iterations=(0, 1, 0), depth_diff=0.004)
        check_pair(ctx, orc, c["src"], c["tgt"], c["intr"], "one iteration each", host=False, n_levels=3, max_iterations=(1, 1, 1), depth_diff=0.004)
        none = check_pair(ctx, orc, c["src"], c["tgt"], c["intr"], "no iteration at all", host=False, n_levels=3, max_iterations=(0, 0, 0))
        assert none["T"].tobytes() == np.eye(4, dtype=F).tobytes()
        cut = check_pair(ctx, orc, c["src"], c["tgt"], c["intr"], "depth_diff cuts partners", host=False, n_levels=2, depth_diff=0.0006)
        assert cut["n_corr_level"][1] < ref["n_corr_level"][1]
        check_pair(ctx, orc, c["src"], c["tgt"], c["intr"], "zmax inside the scene", host=False, n_levels=2, zmax=0.3005, depth_diff=0.004)


@pytest.mark.parametrize("n_frames", [0, 1, 2, 5])
@pytest.mark.parametrize("with_init", [False, True], ids=["identity", "init"])
def test_sequence(tdv, ctx, orc, n_frames, with_init):
    s = K.sequence((96, 72), 5)
    frames = s["frames"][:n_frames]
    kw = dict(depth_diff=K.ACCURACY_DEPTH_DIFF, max_iterations=(6, 4, 3))
    init = np.stack([small_pose(k, 0.3, 0.0005) for k in range(n_frames)]) if with_init and n_frames else None
    ref_poses, ref_pairs = R.sequence(orc, frames, s["intr"], init, **kw)
    env = Env(ctx)
    poses, pairs = ctx.depth_odometry_sequence_dev(env.up(frames), n_frames, 96, 72, *s["intr"], init=init, **kw)
    assert poses.tobytes() == ref_poses.tobytes() and len(pairs) == n_frames
    for k in range(n_frames):
        same_result(pairs[k], ref_pairs[k], ("pair", k))
        if k:                                                                      # ... and the single call on the same ctx, byte for byte
            one = ctx.depth_odometry_dev(env.up(frames[k]), env.up(frames[k - 1]), 96, 72, *s["intr"], None if init is None else init[k], **kw)
            same_result(pairs[k], one, ("single call", k))
    host_poses, host_pairs = ctx.depth_odometry_sequence(frames, s["intr"], init, **kw) if n_frames else (poses, pairs)
    assert host_poses.tobytes() == ref_poses.tobytes()
    if n_frames == 5 and not with_init:
        assert all(p["n_corr"] > 500 for p in pairs[1:])


def test_sequence_of_odd_frames_with_an_empty_one(tdv, ctx, orc):
    """Pairs that stop at different iterations in the same launches, one of them against a frame of zeros."""
    w, h = 65, 47
    frames = np.stack([frame(w, h, 0), frame(w, h, 1), np.zeros((h, w), np.uint16), frame(w, h, 2), frame(w, h, 4)])
    intr = intrinsics(w, h)
    ref_poses, ref_pairs = R.sequence(orc, frames, intr, n_levels=3, max_iterations=(9, 5, 3))
    poses, pairs = ctx.depth_odometry_sequence(frames, intr, n_levels=3, max_iterations=(9, 5, 3))
    assert poses.tobytes() == ref_poses.tobytes()
    for k in range(5):
        same_result(pairs[k], ref_pairs[k], k)
    assert pairs[2]["n_corr"] == 0 and pairs[3]["n_corr"] == 0 and pairs[1]["n_corr"] > 0 and pairs[4]["n_corr"] > 0


def live_buffers(env):
    return dict(frames=env.up(np.full(65 * 8 * 6, 3000, np.uint16)), vm=env.out(144, F).data_ptr(), nm=env.out(144, F).data_ptr(),
                xyz=env.out(144, F).data_ptr(), normals=env.out(144, F).data_ptr())


def test_bad_arguments_on_a_live_context(tdv, ctx):
    env = Env(ctx)
    buffers = live_buffers(env)
    o = Outputs()
    for what, kw, where in BAD[1:]:
        for which in where:
            assert odom_call(tdv, which, ctx._h, o, buffers=buffers, **kw) == -2, (what, which)
    for name, where in NULLS.items():
        for which in where:
            assert odom_call(tdv, which, ctx._h, o, null=(name,), buffers=buffers) == -2, (name, which)
    assert o.untouched()
    # ... and the same arguments unspoilt are accepted: width * height == 0 and a level count that fits
    for which in ("maps_dev", "maps", "terms", "pair_dev", "pair", "sequence"):
        assert odom_call(tdv, which, ctx._h, Outputs(), buffers=buffers) == 0, which
        assert odom_call(tdv, which, ctx._h, Outputs(), buffers=buffers, width=0) == 0, which
