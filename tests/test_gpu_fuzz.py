"""Randomised differential tests of the exact pruned searches (kNN lists, radius lists, ICP correspondences) against
the CPU oracle's brute-force scans (reference src/registration.cpp:63-102, :325-359), on geometries chosen to stress
the Morton order and the bounding-box bounds: flat and collinear clouds (zero extent on an axis), heavy duplication,
tight clusters far apart, large coordinate offsets, tiny scales, and mixtures.  Every comparison is exact."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _make(kind, n, rng):
    if kind == "uniform":
        p = rng.random((n, 3))
    elif kind == "flat":            # zero extent in z
        p = rng.random((n, 3)); p[:, 2] = 0.25
    elif kind == "line":            # zero extent in y and z
        p = np.zeros((n, 3)); p[:, 0] = rng.random(n)
    elif kind == "grid":            # massive exact distance ties
        m = int(np.ceil(n ** (1 / 3)))
        g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)[:n]
        p = g * 0.01
    elif kind == "dups":            # every point repeated several times
        base = rng.random((max(1, n // 5), 3))
        p = base[rng.integers(0, len(base), n)]
    elif kind == "clusters":        # tight clusters far apart
        c = rng.random((8, 3)) * 100.0
        p = c[rng.integers(0, 8, n)] + rng.normal(0, 1e-3, (n, 3))
    elif kind == "offset":          # large offset, small extent: coarse float spacing
        p = 1000.0 + rng.random((n, 3)) * 0.05
    elif kind == "tiny":
        p = rng.random((n, 3)) * 1e-4
    elif kind == "identical":       # one point repeated n times: every distance ties at 0, zero-size boxes
        p = np.tile(rng.random((1, 3)), (n, 1))
    elif kind == "mixed":
        a = rng.random((n // 2, 3)); b = np.full((n - n // 2, 3), 0.5) + rng.normal(0, 1e-6, (n - n // 2, 3))
        p = np.concatenate([a, b], 0)[rng.permutation(n)]
    elif kind in ("nan_rows", "inf_rows", "huge"):   # a uniform cloud with poisoned rows: row 0, the last row, rows around 256, a few at random
        p = rng.random((n, 3))
        rows = np.unique(np.concatenate([[0, n - 1], [r for r in (255, 256) if r < n], rng.integers(0, n, max(1, n // 100))]).astype(np.int64))
        val = {"nan_rows": np.nan, "inf_rows": np.inf, "huge": 1e19}[kind]
        cols = rng.integers(0, 4, len(rows))               # 3: the whole row
        for r, c in zip(rows, cols):
            if c == 3:
                p[r] = val
            else:
                p[r, c] = val if r % 2 == 0 else -val
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, np.float32)


def _extent(p):
    """Largest axis extent of the clean rows: the poisoned kinds keep radii and thresholds at the clean cloud's scale."""
    q = p[(np.abs(p) < 1e18).all(1)]
    return float(np.ptp(q, axis=0).max()) if len(q) else 0.0


KINDS = ["uniform", "flat", "line", "grid", "dups", "clusters", "offset", "tiny", "mixed", "identical", "nan_rows", "inf_rows", "huge"]


# NaN rows: every query's distances hold NaN, and the reference's std::partial_sort over (d2, index) pairs has no strict weak order
# to follow - its lists are then an artefact of libstdc++'s algorithm, not a defined answer.  Infinite rows: only their own queries
# see NaN (inf - inf); the lists and normals of the finite queries (distances finite or +inf) are compared.
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "nan_rows"])
def test_knn_lists_fuzz(ctx, orc, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    for trial in range(3):
        n = int(rng.integers(40, 2600))
        k = int(rng.choice([1, 5, 16, 30, 31, 32, 40, 64, 100]))
        pts = _make(kind, n, rng)
        ref_n, ref_knn = orc.estimate_normals(pts, k, want_knn=True)
        got_n, got_knn = ctx.estimate_normals(pts, k, want_knn=True)
        if kind != "inf_rows":
            assert np.array_equal(got_knn, ref_knn), (kind, n, k)
            # normals come from an eigen-solver on the same sums: identical inputs -> identical bits (NaN rows compare as bytes)
            assert got_n.tobytes() == ref_n.tobytes(), (kind, n, k)
            continue
        q = np.isfinite(pts).all(1)
        assert (~q).any() and q.any()
        assert np.array_equal(got_knn[q], ref_knn[q]), (kind, n, k)
        gn, rn = got_n[q], ref_n[q]           # (NaN positions, then the other bytes: NaN payloads differ between x86 and the GPU)
        assert np.array_equal(np.isnan(gn), np.isnan(rn)), (kind, n, k)
        assert gn[~np.isnan(gn)].tobytes() == rn[~np.isnan(rn)].tobytes(), (kind, n, k)


@pytest.mark.parametrize("kind", KINDS)
def test_radius_lists_fuzz(ctx, orc, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 1)
    for trial in range(3):
        n = int(rng.integers(40, 2200))
        pts = _make(kind, n, rng)
        ext = _extent(pts) or 1.0
        radius = float(ext * rng.choice([0.01, 0.05, 0.2, 2.0]))   # from a handful of neighbours to everything (cap 100)
        nrm = np.zeros_like(pts); nrm[:, 2] = 1.0
        ref = orc.compute_fpfh(pts, nrm, radius, want_neighbors=True)
        got = ctx.compute_fpfh(pts, nrm, radius, want_neighbors=True)
        assert np.array_equal(got[2], ref[2]), (kind, n, radius)
        assert np.array_equal(got[1], ref[1]), (kind, n, radius)


@pytest.mark.parametrize("kind", KINDS)
def test_icp_pruned_correspondences_fuzz(ctx, orc, synth, kind):
    rng = np.random.default_rng(zlib.crc32(kind.encode()) + 2)
    try:
        for trial in range(6):
            ctx.set_icp_search("pruned" if trial % 2 == 0 else "grid")
            ns, nt = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
            tgt = _make(kind, nt, rng)
            src = _make(kind, ns, rng)
            ext = _extent(tgt) or 1.0
            thr = float(ext * rng.choice([1e-3, 0.02, 0.3, 5.0]))
            T = synth.make_transform(rng.normal(size=3), float(rng.uniform(0, 10)), tuple(rng.normal(0, 0.01 * ext, 3)))
            ref = orc.icp_correspondences(src, tgt, None, T, thr, point_to_plane=False)
            got = ctx.icp_correspondences(src, tgt, T, thr)
            acc = ref["accepted"].astype(bool)
            assert np.array_equal(got["accepted"], ref["accepted"]), (kind, ns, nt, thr)
            assert np.array_equal(got["corr"][acc], ref["corr"][acc]), (kind, ns, nt, thr)
            assert got["d2"][acc].tobytes() == ref["d2"][acc].tobytes(), (kind, ns, nt, thr)
            assert got["n_corr"] == ref["n_corr"]
    finally:
        ctx.set_icp_search("auto")


def test_feature_match_pruned_fuzz(ctx, orc):
    """Descriptor rows with structure along the ordering key, exact duplicates, zeros and constant columns."""
    rng = np.random.default_rng(77)
    for trial in range(4):
        ns, nt = int(rng.integers(4096, 7000)), int(rng.integers(2048, 4000))
        base = rng.random((16, 33)).astype(np.float32)
        ft = base[rng.integers(0, 16, nt)] + rng.normal(0, 10.0 ** -float(rng.integers(2, 7)), (nt, 33)).astype(np.float32)
        fs = base[rng.integers(0, 16, ns)] + rng.normal(0, 1e-3, (ns, 33)).astype(np.float32)
        ft = np.abs(ft); fs = np.abs(fs)
        ft /= ft.sum(1, keepdims=True); fs /= fs.sum(1, keepdims=True)
        ft[nt // 2: nt // 2 + 200] = ft[:200]          # duplicates: lowest index must win
        fs[:100] = ft[nt // 2: nt // 2 + 100]
        if trial == 3:
            ft[:, 5] = 0; fs[:, 16] = 0
        assert np.array_equal(ctx.feature_match(fs, ft), orc.feature_match(fs, ft)), trial


def test_feature_match_leaf_major_fuzz(ctx, orc):
    """The leaf-major index search at sizes with several groups of leaves (its group boxes, the per-pool lists, partly filled
    waves and work units), against the plain scan on the same device (TDV_FM_BRUTE, itself held against the oracle above and in
    test_gpu_ransac.py) and, on a sample of the sources, against the oracle; its two-round variant and round 2's walk over the
    same index return the same correspondences.  Clustered rows, duplicates, non-finite rows, sources far from every target."""
    import os
    rng = np.random.default_rng(2025)
    for trial, (ns, nt, ncl) in enumerate(((4097, 9001, 40), (20011, 16500, 300), (70001, 30000, 1500))):
        centres = rng.random((ncl, 33)).astype(np.float32)
        ft = centres[rng.integers(0, ncl, nt)] + rng.normal(0, 2e-2, (nt, 33)).astype(np.float32)
        fs = centres[rng.integers(0, ncl, ns)] + rng.normal(0, 2e-2, (ns, 33)).astype(np.float32)
        ft[nt // 2: nt // 2 + 300] = ft[:300]; fs[:200] = ft[nt // 2: nt // 2 + 200]     # duplicated targets: the lower index wins
        fs[300] = 50.0; fs[301] = -7.0; fs[302, 4] = np.nan; fs[303, 9] = np.inf          # far away / match nothing
        ft[17, 0] = np.nan; ft[18, 3] = np.inf                                            # never chosen
        got = {}
        try:
            study = os.environ.get("TDV_LIB_VARIANT") == "study"        # (the two-round variant lives in the study library; elsewhere the knob is inert)
            for name, knob, value in (("leaf-major", None, None), ("two rounds", "TDV_LM_ROUNDS" if study else None, "2"), ("walk", "TDV_FM_LEAFMAJOR", "0"), ("scan", "TDV_FM_BRUTE", "1")):
                if knob:
                    os.environ[knob] = value
                got[name] = ctx.feature_match(fs, ft)
                if knob:
                    del os.environ[knob]
        finally:
            for knob in ("TDV_LM_ROUNDS", "TDV_FM_LEAFMAJOR", "TDV_FM_BRUTE"):
                os.environ.pop(knob, None)
        for name in ("leaf-major", "two rounds", "walk"):
            assert np.array_equal(got[name], got["scan"]), (trial, name, int((got[name] != got["scan"]).sum()))
        pick = np.concatenate([np.arange(0, 320), rng.integers(0, ns, 700)])
        assert np.array_equal(got["leaf-major"][pick], orc.feature_match(fs[pick], ft)), trial
        low = np.delete(got["leaf-major"][:200], [17, 18])              # (targets 17 and 18 are the non-finite rows: their copies win)
        assert got["leaf-major"][302] == 0 and got["leaf-major"][303] == 0 and (low < nt // 2).all() and (got["leaf-major"][17:19] >= nt // 2).all()


@pytest.mark.parametrize("scale", [1e-4, 1.0, 3e4])
def test_feature_match_principal_box_margins(ctx, orc, scale):
    """The packed-index search prunes with boxes in the targets' principal coordinates, a bound that is only safe with
    a rounding margin (fmatch.hip, principal_bound_note).  Data that stress it: rows on a thin curved filament (almost
    all variance in one direction, tiny but decisive off-axis differences), a large common offset (cancellation in
    x - mean), magnitudes from 1e-4 to 3e4, queries far off the filament, and exact ties."""
    rng = np.random.default_rng(int(scale * 1000) % 97 + 5)
    ns, nt = 5200, 3100
    axis = rng.normal(size=33); axis /= np.linalg.norm(axis)
    bend = rng.normal(size=33); bend -= bend @ axis * axis; bend /= np.linalg.norm(bend)

    def rows(n, jitter):
        t = rng.random(n)
        x = np.outer(t, axis) + np.outer(0.05 * np.sin(6 * t), bend) + rng.normal(0, jitter, (n, 33))
        return x

    off = rng.random(33) * 40.0
    ft = ((rows(nt, 1e-5) + off) * scale).astype(np.float32)
    fs = ((rows(ns, 1e-5) + off) * scale).astype(np.float32)
    fs[:300] = ((rows(300, 0.3) + off) * scale).astype(np.float32)        # outliers: far from every target
    ft[2000:2100] = ft[100:200]; fs[300:400] = ft[2000:2100]              # ties: the lower index wins
    got = ctx.feature_match(fs, ft)
    ref = orc.feature_match(fs, ft)
    assert np.array_equal(got, ref), int((got != ref).sum())
