"""tdv_voxel_downsample_normals and its _dev form (include/tdv_hip.h) against the CPU oracle, byte for byte.

The reference: orc.voxel_downsample(xyz, normals, v) - the oracle's colour slot is a generic 3-wide mean (f32 sums in ascending input
index, divided by (float)count) - brought to unit length here in numpy f32 with the stated tree, l2 = x*x + (y*y + z*z), l = sqrt(l2),
divided where l2 > 0 and l is finite (numpy's f32 element operations round once each and do not contract).  The oracle emits the
reference's container order: TDV_VOXEL_ORDER_REFERENCE is compared row by row, TDV_VOXEL_ORDER_FIRST through the oracle's `first` indices.
Points and colours must be tdv_voxel_downsample_dev's bytes.

Shapes: one point; 257 points in one voxel (past the hash table's 16-member rows AND the counting sort's 96-record buckets: the full
sort's k_voxel_means, and its run crosses a 256-thread block); two opposite normals in one voxel (the mean is zero and stays zero); a NaN
normal in a voxel; 5,000 random points at ~1,200 voxels with and without colours (the hash table, more than one 1,024-point tile); the
same points at ~250 voxels (about 20 per voxel: the counting-sort path's bucket kernel)."""
import numpy as np
import pytest

from state_cases import Env

pytestmark = pytest.mark.gpu
F = np.float32


def unit(m):
    m = np.ascontiguousarray(m, F)
    with np.errstate(all="ignore"):
        x, y, z = m[:, 0], m[:, 1], m[:, 2]
        l2 = x * x + (y * y + z * z)
        l = np.sqrt(l2)
        ok = (l2 > 0) & np.isfinite(l)
        out = m.copy()
        out[ok] = m[ok] / l[ok, None]
    assert out.dtype == F
    return out


def _random(n, seed, box):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * box - box / 2 + [0.3, -0.2, 0.7]).astype(F)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    return pts, nrm, rng.random((n, 3)).astype(F)


def _cases():
    c = {}
    c["one_point"] = (np.array([[0.011, -0.52, 0.3]], F), np.array([[0.6, 0.0, -0.8]], F), None, 0.01, 1)
    rng = np.random.default_rng(257)
    p257 = ((rng.random((257, 3)) * 0.9 + 0.05) * 0.01 + [-0.05, 0.02, 0.4]).astype(F)       # inside cell (-5, 2, 40)
    n257 = rng.normal(size=(257, 3)); n257[:, 2] = np.abs(n257[:, 2]) + 1.0
    c["257_in_one_voxel"] = (p257, (n257 / np.linalg.norm(n257, axis=1, keepdims=True)).astype(F), rng.random((257, 3)).astype(F), 0.01, 1)
    c["opposite_normals"] = (np.array([[0.001, 0.002, 0.003], [0.004, 0.005, 0.006], [0.5, 0.5, 0.5]], F),
                             np.array([[0.6, 0.0, -0.8], [-0.6, 0.0, 0.8], [0.0, 1.0, 0.0]], F), None, 0.01, 2)
    pn, nn, _ = _random(40, 5, 0.03)
    nn[7, 1] = np.nan
    c["nan_normal"] = (pn, nn, None, 0.01, None)
    pts, nrm, rgb = _random(5000, 11, 0.102)           # 10.2 voxels a side: 1,219 voxels at 0.01, 252 at 0.018
    c["5000_at_1200"] = (pts, nrm, None, 0.01, None)
    c["5000_at_1200_colours"] = (pts, nrm, rgb, 0.01, None)
    c["5000_at_250_colours"] = (pts, nrm, rgb, 0.018, None)
    for v in c.values():
        for a in v[:3]:
            if a is not None:
                a.setflags(write=False)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def refs(orc):
    """The oracle's voxels (reference order), its first indices, and the unit normals: computed once, shared, never modified."""
    out = {}
    for name, (pts, nrm, rgb, voxel, n_vox) in CASES.items():
        x, mean_n, first = orc.voxel_downsample(pts, nrm, voxel)
        c = orc.voxel_downsample(pts, rgb, voxel)[1] if rgb is not None else None
        if n_vox is not None:
            assert len(x) == n_vox, (name, len(x))
        out[name] = dict(xyz=x, nrm=unit(mean_n), mean=mean_n, rgb=c, first=first)
    assert 1100 <= len(out["5000_at_1200"]["xyz"]) <= 1300 and 200 <= len(out["5000_at_250_colours"]["xyz"]) <= 320
    return out


def _ordered(ref, order, tdv):
    perm = np.argsort(ref["first"], kind="stable") if order == tdv.TDV_VOXEL_ORDER_FIRST else np.arange(len(ref["xyz"]))
    return ref["xyz"][perm], ref["nrm"][perm], None if ref["rgb"] is None else ref["rgb"][perm]


def _dev(ctx, pts, nrm, rgb, voxel, order):
    env = Env(ctx)
    n = len(pts)
    ox, on = env.out(3 * n, F), env.out(3 * n, F)
    oc = env.out(3 * n, F) if rgb is not None else None
    m = ctx.voxel_downsample_normals_dev(env.up(pts), env.up(nrm), n, voxel, ox.data_ptr(), on.data_ptr(), n,
                                         None if rgb is None else env.up(rgb), None if oc is None else oc.data_ptr(), order)
    got = (env.get(ox, 3 * m, F).reshape(-1, 3), env.get(on, 3 * m, F).reshape(-1, 3), None if oc is None else env.get(oc, 3 * m, F).reshape(-1, 3))
    # the plain entry point's bytes
    px, pc = env.out(3 * n, F), (env.out(3 * n, F) if rgb is not None else None)
    m2 = ctx.voxel_downsample_dev(env.up(pts), None if rgb is None else env.up(rgb), n, voxel, px.data_ptr(), None if pc is None else pc.data_ptr(), n, order)
    plain = (env.get(px, 3 * m2, F).reshape(-1, 3), None if pc is None else env.get(pc, 3 * m2, F).reshape(-1, 3))
    return got, plain


@pytest.mark.parametrize("order", ["first", "reference"])
@pytest.mark.parametrize("name", list(CASES))
def test_against_oracle(tdv, ctx, refs, name, order):
    pts, nrm, rgb, voxel, _ = CASES[name]
    o = tdv.TDV_VOXEL_ORDER_FIRST if order == "first" else tdv.TDV_VOXEL_ORDER_REFERENCE
    rx, rn, rc = _ordered(refs[name], o, tdv)
    (gx, gn, gc), (px, pc) = _dev(ctx, pts, nrm, rgb, voxel, o)
    assert gx.tobytes() == rx.tobytes(), (name, order, "points")
    bad = np.flatnonzero((gn.view(np.uint32) != rn.view(np.uint32)).any(axis=1)) if gn.shape == rn.shape else None
    assert gn.tobytes() == rn.tobytes(), (name, order, "normals", gn.shape, rn.shape, None if bad is None else (bad[:5], gn[bad[:3]], rn[bad[:3]]))
    assert (gc is None) == (rc is None) and (gc is None or gc.tobytes() == rc.tobytes()), (name, order, "colours")
    assert gx.tobytes() == px.tobytes() and (gc is None or gc.tobytes() == pc.tobytes()), (name, order, "not tdv_voxel_downsample_dev's bytes")
    # the host entry point: the same bytes
    hx, hn, hc = ctx.voxel_downsample_normals(pts, nrm, voxel, rgb, o)
    assert hx.tobytes() == rx.tobytes() and hn.tobytes() == rn.tobytes() and (hc is None or hc.tobytes() == rc.tobytes()), (name, order, "host")


def test_the_edge_cases_are_what_they_claim(refs):
    """The fixtures reach the rule's branches: a zero mean that stays zero, a NaN mean that stays NaN, unit length elsewhere."""
    r = refs["opposite_normals"]
    z = np.flatnonzero((r["mean"] == 0).all(axis=1))
    assert len(z) == 1 and (r["nrm"][z] == 0).all()
    r = refs["nan_normal"]
    assert np.isnan(r["nrm"]).any(axis=1).sum() == 1
    n = refs["5000_at_1200"]["nrm"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    m = refs["5000_at_1200"]["mean"].astype(np.float64)
    assert (np.linalg.norm(m, axis=1) < 0.9).sum() > 300             # means well short of unit length: the division does something


def test_without_normals_is_the_plain_call(tdv, ctx):
    pts, nrm, rgb, voxel, _ = CASES["5000_at_1200_colours"]
    a = ctx.voxel_downsample_normals(pts, None, voxel, rgb, tdv.TDV_VOXEL_ORDER_FIRST)
    b = ctx.voxel_downsample(pts, rgb, voxel, tdv.TDV_VOXEL_ORDER_FIRST)
    assert a[1] is None and a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[1].tobytes()
