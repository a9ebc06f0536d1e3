"""The sorted-cloud descriptor (csrc/tdv_internal.hpp: SortedCloud; csrc/sorted_cloud.hpp) at the sizes where one 64-point leaf, one
4096-point group of leaves, or the padding between n and pad is exactly full or exactly one over: a swapped n_leaf / n_top or a lost
`p < n` shows there.  The outlier, cluster and ISS suites already sit on such sizes; the feature suite stops at 3001 points and never
crosses a group, and the pruned ICP search meets a target above 4096 only at 5000 and 70000.  Comparisons and tolerances are those of
test_gpu_features.py (test_knn_lists_and_normals, test_fpfh) and of test_gpu_icp.py (test_pruned_search_matches_oracle): exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [64, 4096, 4097, 8193]
K = 30
RADIUS = 0.05          # test_fpfh's middle case


def _cloud(synth, n, seed=42):
    pts, _ = synth.sample_object(n, seed)
    T = synth.gt_transform(seed)
    Tinv = np.linalg.inv(T.astype(np.float64))
    return (pts.astype(np.float64) @ Tinv[:3, :3].T + Tinv[:3, 3]).astype(np.float32)  # camera-frame cloud, z ~ 0.8


_REF = {}


def _reference(orc, synth, n):
    """cloud, the oracle's normals and kNN lists: computed once per size, shared by both tests, never written to"""
    if n not in _REF:
        pts = _cloud(synth, n)
        pts[50] = pts[10]; pts[51] = pts[10]  # duplicates: ties resolved by lower index
        nrm, knn = orc.estimate_normals(pts, K, want_knn=True)
        for a in (pts, nrm, knn):
            a.setflags(write=False)
        _REF[n] = (pts, nrm, knn)
    return _REF[n]


@pytest.mark.parametrize("n", SIZES)
def test_knn_lists_and_normals_at_leaf_and_group_edges(ctx, orc, synth, n):
    pts, ref_n, ref_knn = _reference(orc, synth, n)
    got_n, got_knn = ctx.estimate_normals(pts, K, want_knn=True)
    assert np.array_equal(got_knn, ref_knn)
    bit = got_n.tobytes() == ref_n.tobytes()
    print("normals bitwise equal:", bit, "max abs diff", np.abs(got_n - ref_n).max())
    assert bit


@pytest.mark.parametrize("n", SIZES)
def test_fpfh_at_leaf_and_group_edges(ctx, orc, synth, n):
    pts, nrm, _ = _reference(orc, synth, n)
    ref_d, ref_nb, ref_cnt = orc.compute_fpfh(pts, nrm, RADIUS, want_neighbors=True)
    got_d, got_nb, got_cnt = ctx.compute_fpfh(pts, nrm, RADIUS, want_neighbors=True)
    assert np.array_equal(got_cnt, ref_cnt)
    assert np.array_equal(got_nb, ref_nb)
    same = (got_d.view(np.uint32) == ref_d.view(np.uint32)).all(1)
    print("fpfh rows bitwise equal: %d / %d ; max abs diff %.3g" % (same.sum(), n, np.abs(got_d - ref_d).max()))
    assert same.all(), "rows differing: %d of %d" % ((~same).sum(), n)


@pytest.fixture
def pruned(ctx):
    ctx.set_icp_search("pruned")
    yield ctx
    ctx.set_icp_search("auto")


@pytest.mark.parametrize("thr", [0.004, 10.0])
@pytest.mark.parametrize("nt", [63, 64, 65, 4096, 4097])
def test_pruned_search_at_leaf_and_group_edges(pruned, orc, synth, nt, thr):
    """Accepted correspondences (index, d2) identical to the oracle's full scan; the rest are rejected in both."""
    ns = 257
    tgt, nrm = synth.sample_object(nt, 42)
    src, T_gt = synth.make_scene(ns, 42)
    T = synth.perturb(T_gt)
    ref = orc.icp_correspondences(src, tgt, nrm, T, thr)
    got = pruned.icp_correspondences(src, tgt, T, thr)
    assert pruned.last_icp_search() == "pruned"
    acc = ref["accepted"].astype(bool)
    assert np.array_equal(got["accepted"], ref["accepted"])
    assert np.array_equal(got["corr"][acc], ref["corr"][acc])
    assert got["d2"][acc].tobytes() == ref["d2"][acc].tobytes()
    assert got["n_corr"] == ref["n_corr"]
    if thr >= 10.0:
        assert acc.all()   # loose threshold: the walk still returns the true nearest neighbour of every point
