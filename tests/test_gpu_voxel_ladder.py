"""The voxel stage's ladder (csrc/voxel.hip: voxel_first_order - pixel windows, table, counting sort, full sort) through every caller of it,
at the smallest shapes that reach each rung.

Three clouds back to back - 0, 700 and 1,500 points, cells planted as in test_gpu_voxel.py::test_member_counts_around_the_hash_path_row_size
(shuffled input order, negative cells) - in three variants:
  table      at most 16 points in every voxel: the table keeps the batch, redone == 0;
  counting   one voxel of 17 points in the last cloud: the batch is redone cloud by cloud (redone == 1), the last cloud's table hands it
             to the counting sort's bucket kernel;
  sort       one voxel of 100 points, past VX_MAX_BUCKET = 96: that cloud's counting sort hands it to the full sort and k_voxel_means.
Per variant, byte for byte: tdv_voxel_downsample_batch_dev's rows and offsets == the per-cloud tdv_voxel_downsample_dev calls in
TDV_VOXEL_ORDER_FIRST, concatenated (with colours) == the oracle's voxels ordered by its `first` indices; the per-cloud call in
TDV_VOXEL_ORDER_REFERENCE with TDV_VOXEL_DEVICE_ORDER at 0 and at 1 == the oracle's rows; per cloud with normals
(tdv_voxel_downsample_normals_dev, what a multi-scale level runs for one instance) == the oracle's unit means; and the multi-scale batch
(GICP: the NRM kernels) reports the same `redone`, the oracle's voxel count per instance, and per instance the single call's bits.

The pinhole entry: one on-grid cloud of a 40 x 30 pixel box reports `pixels`, the same cloud moved by a third of a pixel reports `table`;
both are the oracle's voxels.

Rows of this table that other tests hold and this one leaves out: redone == 0 / 1 of the multi-scale level and of the batch entry on clouds
planted from a scan (test_gpu_icp_multiscale.py::test_batched_voxel_level_reports_which_way_it_went); the pixel windows against the table
and the oracle at frame size, and every other reason for a tile to hand over (test_gpu_voxel_pixels.py); voxels of 1 .. 17 points through
the host entry, with colours (test_gpu_voxel.py::test_member_counts_around_the_hash_path_row_size)."""
import os

import numpy as np
import pytest
import torch

from state_cases import Env
from test_gpu_icp_multiscale import bits
from test_gpu_voxel_normals import unit
from test_gpu_voxel_pixels import CAM, F as FOCAL, _clouds, _frame

pytestmark = pytest.mark.gpu
F = np.float32
VOXEL = F(0.01)
SIZES = (0, 700, 1500)
FULLEST = {"table": 16, "counting": 17, "sort": 100}          # VH_K = 16 member slots, VX_MAX_BUCKET = 96 records (csrc/voxel.hip)


def _cloud(rng, n, fullest):
    """n points in distinct cells (negative ones among them) holding 1 .. 16 points each, the first cell `fullest`; shuffled"""
    cells = np.concatenate([rng.permutation(np.arange(-150, 150))[:, None], rng.integers(-30, 30, (300, 2))], axis=1)      # distinct in x
    counts, left = [], n
    for k in range(len(cells)):
        c = min(left, fullest if k == 0 else 1 + k % 16)
        counts.append(c); left -= c
        if left == 0:
            break
    assert left == 0
    pts = np.concatenate([(cells[k] + 0.05 + 0.9 * rng.random((c, 3))) * float(VOXEL) for k, c in enumerate(counts)]).astype(F)
    return pts[rng.permutation(len(pts))]


def _counts(pts):
    keys = np.floor(pts * F(F(1.0) / VOXEL)).astype(np.int64)
    return np.unique(keys, axis=0, return_counts=True)[1]


@pytest.fixture(scope="module", params=list(FULLEST))
def planted(request, orc):
    """The variant's clouds, colours and unit normals, and the oracle's voxels of every cloud in both orders.  Never modified."""
    rng = np.random.default_rng(len(request.param))
    clouds = [_cloud(rng, n, FULLEST[request.param] if n == SIZES[-1] else 16) for n in SIZES]
    assert [int(_counts(c).max()) if len(c) else 0 for c in clouds] == [0, 16, FULLEST[request.param]]       # on the f32 keys the device forms
    assert min(int(c.min() / float(VOXEL)) for c in clouds[1:]) < -10
    rgb = [rng.random((len(c), 3)).astype(F) for c in clouds]
    nrm = [unit(rng.standard_normal((len(c), 3)).astype(F)) for c in clouds]
    ref, first_order, first_nrm = [], [], []
    for c, col, nr in zip(clouds, rgb, nrm):
        x, m, first = orc.voxel_downsample(c, col, float(VOXEL)) if len(c) else (c, col, np.zeros(0, np.int64))
        perm = np.argsort(first, kind="stable")
        ref.append((x, m)); first_order.append((x[perm], m[perm]))
        first_nrm.append(unit(orc.voxel_downsample(c, nr, float(VOXEL))[1][perm]) if len(c) else nr)
    for a in clouds + rgb + nrm:
        a.setflags(write=False)
    return dict(name=request.param, redone=0 if request.param == "table" else 1, clouds=clouds, rgb=rgb, nrm=nrm, ref=ref, first=first_order,
                first_nrm=first_nrm, off=np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32))


def _per_cloud(ctx, tdv, env, pts, rgb, order):
    n = len(pts)
    o_xyz, o_rgb = env.out(3 * n, F), env.out(3 * n, F)
    v = ctx.voxel_downsample_dev(env.up(pts), env.up(rgb), n, float(VOXEL), o_xyz.data_ptr(), o_rgb.data_ptr(), n, order=order)
    return env.get(o_xyz, 3 * v, F).reshape(-1, 3), env.get(o_rgb, 3 * v, F).reshape(-1, 3)


def test_batch_entry_per_cloud_calls_and_oracle_agree(tdv, ctx, planted):
    env = Env(ctx)
    p = planted
    total = int(p["off"][-1])
    out = env.out(3 * total, F)
    voff = ctx.voxel_downsample_batch_dev(env.up(np.concatenate(p["clouds"])), p["off"], float(VOXEL), out.data_ptr())
    assert ctx.last_voxel_batch_redone() == p["redone"] and ctx.last_voxel_grouping() == "table", p["name"]
    assert list(np.diff(voff)) == [len(x) for x, _ in p["first"]]
    rows = env.get(out, 3 * int(voff[-1]), F).reshape(-1, 3)
    assert rows.tobytes() == np.concatenate([x for x, _ in p["first"]]).tobytes(), p["name"]
    for b, (c, col) in enumerate(zip(p["clouds"], p["rgb"])):
        x, m = _per_cloud(ctx, tdv, env, c, col, tdv.TDV_VOXEL_ORDER_FIRST)
        assert x.tobytes() == p["first"][b][0].tobytes() and m.tobytes() == p["first"][b][1].tobytes(), (p["name"], b)
        assert x.tobytes() == rows[voff[b]:voff[b + 1]].tobytes()


@pytest.mark.parametrize("device_order", ["0", "1"])
def test_reference_order_per_cloud_by_either_way(tdv, ctx, planted, device_order):
    env = Env(ctx)
    try:
        os.environ["TDV_VOXEL_DEVICE_ORDER"] = device_order
        got = [_per_cloud(ctx, tdv, env, c, col, tdv.TDV_VOXEL_ORDER_REFERENCE) for c, col in zip(planted["clouds"], planted["rgb"])]
    finally:
        os.environ.pop("TDV_VOXEL_DEVICE_ORDER", None)
    for b, (x, m) in enumerate(got):
        assert x.tobytes() == planted["ref"][b][0].tobytes() and m.tobytes() == planted["ref"][b][1].tobytes(), (planted["name"], device_order, b)


def test_multiscale_level_goes_the_same_way(tdv, ctx, synth, planted):
    env = Env(ctx)
    p = planted
    for b, (c, nr) in enumerate(zip(p["clouds"], p["nrm"])):          # what a level runs for one instance: the normals ride the same rungs
        n = len(c)
        o_xyz, o_nrm = env.out(3 * n, F), env.out(3 * n, F)
        v = ctx.voxel_downsample_normals_dev(env.up(c), env.up(nr), n, float(VOXEL), o_xyz.data_ptr(), o_nrm.data_ptr(), n)
        assert env.get(o_xyz, 3 * v, F).tobytes() == p["first"][b][0].tobytes() and env.get(o_nrm, 3 * v, F).tobytes() == p["first_nrm"][b].tobytes(), (p["name"], b)
    tgt, tn = synth.sample_object(500, 42)
    pt, ptn = env.up(tgt), env.up(tn)
    lv = tdv.icp_levels([VOXEL, None], [F(0.5), F(0.5)], [2, 1])
    T0 = np.eye(4, dtype=F)
    got = ctx.multi_scale_icp_batch_dev(env.up(np.concatenate(p["clouds"])), p["off"], pt, ptn, len(tgt), np.stack([T0] * len(SIZES)), estimation="gicp",
                                        d_src_normals=env.up(np.concatenate(p["nrm"])), levels=lv)
    assert ctx.last_voxel_batch_redone() == p["redone"], p["name"]
    for b, (c, nr) in enumerate(zip(p["clouds"], p["nrm"])):
        one = ctx.multi_scale_icp_dev(env.up(c), len(c), pt, ptn, len(tgt), T0, estimation="gicp", d_src_normals=env.up(nr), levels=lv)
        assert [bits(l) for l in got[b].levels] == [bits(l) for l in one.levels], (p["name"], b)
        assert got[b].levels[0].ns == len(p["first"][b][0]) and got[b].levels[1].ns == len(c)
    assert ctx.last_voxel_batch_redone() == p["redone"]              # the single calls have no batched pass: the batch's answer stands


def test_pinhole_entry_on_and_off_the_pixel_grid(ctx, orc):
    depth, label, n_inst = _frame(11, 1, (40, 30))
    d_xyz, off = _clouds(ctx, depth, label, n_inst)
    n = int(off[-1])
    assert n_inst == 1 and 1000 <= n <= 1200
    voxel = float(F(1.2 * 0.45 / FOCAL))
    shifted = d_xyz.clone()
    shifted[:, 0] += shifted[:, 2] / (3.0 * FOCAL)                   # a third of a pixel in u: still row-major, no longer on the grid
    for cloud, how in ((d_xyz, "pixels"), (shifted, "table")):
        out = torch.empty_like(cloud)
        voff = ctx.voxel_downsample_batch_dev(cloud.data_ptr(), off, voxel, out.data_ptr(), pinhole=CAM)
        assert ctx.last_voxel_grouping() == how and ctx.last_voxel_batch_redone() == 0
        x, _, first = orc.voxel_downsample(cloud[:n].cpu().numpy(), None, voxel)
        assert list(voff) == [0, len(x)] and out[:len(x)].cpu().numpy().tobytes() == x[np.argsort(first, kind="stable")].tobytes(), how
