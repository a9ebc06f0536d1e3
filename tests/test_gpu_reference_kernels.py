"""The product's depth, deproject and ICP kernels against the REFERENCE'S OWN GPU kernels (cuda/depth_processing.cu, cuda/pointcloud.cu,
cuda/icp.cu), compiled unchanged for gfx950 into oracle/_ref/libtdv_ref_kernels.so by oracle/ref_kernels.py and called through
oracle/refkernels.py.  This is the one pin to code written by the reference's authors; where the library is missing the tests FAIL
(they do not skip): run __graft_entry__.build() on a machine that holds the reference tree.

Bars (inputs, float64 evaluations and bounds: tests/ref_kernel_cases.py; measured figures: profiles/r25/reference_kernels.md):
  depth preprocess   bit for bit (TDV_MASK_NONZERO is the kernel's `!= 0` rule; fl(1.0f / s) equals fl32(fl64(1.0 / s)))
  bilateral filter   bit for bit; the oracle (host expf) within twice the reference kernel's own error against float64
  deproject          count, z and NaN positions exact; x, y, colours within 3 * 2^-24 relative and NOT all equal: the product divides
                     where the reference's kernel multiplies by a rounded reciprocal (the product follows src/pipeline.cpp)
  correspondences    accepted sets and indices equal, d2 within the derived bound of float64, no row excluded as a tie or an edge
  normal equations   the reference kernel's JtJ / Jtr and the oracle's ATA / ATb within n u sum|term| of the float64 sums
"""
import numpy as np
import pytest

import ref_kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    from oracle import refkernels
    refkernels.lib()              # raises, naming build(), when the library is absent
    return refkernels


def _ratio(diff, bound):
    """max of diff / bound over the entries with a positive bound (a zero bound means every term, and so every sum, is exactly zero)."""
    return float(np.where(bound > 0, np.abs(diff) / np.where(bound > 0, bound, 1), 0).max())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ depth preprocess
@pytest.mark.parametrize("size", K.PREPROCESS_SIZES, ids=lambda s: "%dx%d" % s)
def test_depth_preprocess_equals_reference_kernel(ctx, tdv, ref, size):
    h, w = size
    raw, mask = K.preprocess_frame(h, w)
    frames = [(raw, mask)]
    if size == (1, 1):
        frames = [(np.full((1, 1), v, np.uint16), np.full((1, 1), m, np.uint8)) for v in (0, 65535, 1234) for m in (0, 1, 255)]
    else:
        assert raw.min() == 0 and raw.max() == 65535
    if w >= 256:
        assert all(len(np.unique(row)) == 256 for row in mask)
    for raw, mask in frames:
        for scale in K.PREPROCESS_SCALES:
            want = ref.depth_preprocess(raw, mask, scale, apply_mask=True)
            got = ctx.depth_preprocess(raw, mask, scale, tdv.TDV_MASK_NONZERO)
            assert _same(got, want), (size, scale, int((got != want).sum()))
            assert np.array_equal(want == 0, (mask == 0) | (raw == 0))
            unmasked = ref.depth_preprocess(raw, mask, scale, apply_mask=False)
            assert _same(unmasked, ref.depth_preprocess(raw, None, scale, apply_mask=True))      # a null mask is no mask
            assert _same(ctx.depth_preprocess(raw, None, scale), unmasked), (size, scale)
            # the declared divergence: the product's default rule is src/pipeline.cpp's threshold(mask, 10), the kernel's is `!= 0`;
            # they differ exactly on the mask bytes 1..10
            default = ctx.depth_preprocess(raw, mask, scale)
            assert np.array_equal(default != want, (mask >= 1) & (mask <= 10) & (raw != 0)), (size, scale)


# ------------------------------------------------------------------ bilateral filter
@pytest.mark.parametrize("name", K.BILATERAL_IMAGES)
def test_bilateral_filter_equals_reference_kernel(ctx, orc, ref, name):
    d = K.bilateral_image(name)
    for ss, sr in K.BILATERAL_SIGMAS:
        want = ref.bilateral_filter(d, ss, sr)
        got = ctx.bilateral_filter(d, ss, sr)
        f64 = K.bilateral_f64(d, ss, sr)
        e_ref = float(np.abs(want - f64).max()); e_got = float(np.abs(got - f64).max())
        o = orc.bilateral_filter(d, ss, sr)
        e_orc = float(np.abs(o - f64).max())
        print("bilateral %s sigma (%g, %g): differing pixels %d of %d; max |kernel - f64| %.3e, |product - f64| %.3e, |oracle - f64| %.3e"
              % (name, ss, sr, int((got != want).sum()), d.size, e_ref, e_got, e_orc))
        assert np.array_equal(want == 0, d == 0)
        assert _same(got, want), (name, ss, sr, int((got != want).sum()))
        # the oracle calls the host's expf: zero pattern equal, error against float64 within twice the reference kernel's own
        assert np.array_equal(o == 0, want == 0)
        assert e_orc <= 2 * e_ref, (name, ss, sr, e_orc, e_ref)
    if name == "lone_corner":
        assert want[0, 0] == np.float32(0.5) and want[39, 129] == np.float32(0.6) and want[0, 129] == np.float32(0.7) and np.count_nonzero(want) == 3
    if name == "zero":
        assert not want.any()


# ------------------------------------------------------------------ deproject
@pytest.mark.parametrize("zmax", [0.5, 1.5, 10.0])
@pytest.mark.parametrize("frame,intr", [((0, 97, 131), "plain"), ((3, 211, 307), "plain"), ((0, 97, 131), "negative_fx")],
                         ids=["97x131", "211x307", "97x131-negative-fx"])
def test_deproject_against_reference_kernel(ctx, ref, frame, intr, zmax):
    d, bgr = K.deproject_frame(*frame)
    fx, fy, cx, cy = K.INTRINSICS[intr]
    rows, n = ref.deproject(d, bgr, fx, fy, cx, cy, zmax)
    xyz, rgb = ctx.deproject(d, bgr, fx, fy, cx, cy, zmax)
    keep = K.expected_pixels(d, zmax)
    assert n == len(xyz) == len(keep) and n > 0                                         # the count is exact
    pix_ref = K.pixel_index(rows[:, 3:6]); pix_got = K.pixel_index(rgb)
    assert np.array_equal(pix_got, keep)                                                 # the product's rows are in row-major order
    order = np.argsort(pix_ref, kind="stable")
    assert np.array_equal(pix_ref[order], keep)                                          # the kernel kept the same pixels, each once
    rows = rows[order]
    assert _same(xyz[:, 2], rows[:, 2]) and _same(xyz[:, 2], d.ravel()[keep])            # z bit for bit (a NaN as the same NaN)
    assert np.array_equal(np.isnan(xyz), np.isnan(rows[:, :3])) and np.isnan(xyz).any()  # the NaN depth is kept by both
    got = np.concatenate([xyz[:, :2], rgb], axis=1).astype(np.float64); want = rows[:, [0, 1, 3, 4, 5]].astype(np.float64)
    ok = ~np.isnan(want)
    diff = np.abs(got - want)[ok]; scale = np.maximum(np.abs(got), np.abs(want))[ok]
    rel = np.where(scale > 0, diff / np.where(scale > 0, scale, 1), 0)
    print("deproject %s zmax %g: %d rows; max relative difference %.3e (bound %.3e); differing values %d of %d"
          % (frame, zmax, n, rel.max(), 3 * K.U, int((diff != 0).sum()), diff.size))
    assert (diff <= 3 * K.U * scale).all(), rel.max()
    # the declared divergence: x / fx against x * fl(1 / fx), c / 255 against c * fl(1 / 255) are not the same float everywhere
    for col in (0, 1, 2):                            # x, y and the red channel (every byte value) each differ somewhere
        assert (got[ok[:, col], col] != want[ok[:, col], col]).any(), col


# ------------------------------------------------------------------ ICP correspondences
@pytest.mark.parametrize("search", ["brute", "pruned", "grid"])
@pytest.mark.parametrize("thr", K.ICP_THRESHOLDS)
@pytest.mark.parametrize("scene", K.ICP_SCENES, ids=lambda s: "%dx%d" % s[:2])
def test_icp_correspondences_against_reference_kernel(ctx, ref, scene, thr, search):
    src, tgt, _, T, f64 = K.icp_scene(*scene)
    rows = K.icp_rows(f64, thr)
    assert not rows["tie"].any() and not rows["edge"].any()              # no row is excluded: every one is compared
    want = ref.find_correspondences(src, tgt, T, thr)
    ctx.set_icp_search(search)
    try:
        got = ctx.icp_correspondences(src, tgt, T, thr)
    finally:
        ctx.set_icp_search("auto")
    acc = rows["accepted"]
    assert 30 <= acc.sum() < len(src)
    ref_acc = want["corr"] >= 0
    assert np.array_equal(ref_acc, acc) and np.array_equal(got["accepted"], acc) and got["n_corr"] == acc.sum()
    assert np.array_equal(want["corr"][acc], f64["index"][acc])
    rows_got = np.ones(len(src), bool) if search == "brute" else acc     # the scan reports every row's nearest, the pruned searches the accepted rows'
    assert np.array_equal(got["corr"][rows_got], f64["index"][rows_got])
    assert np.array_equal(got["corr"][acc], want["corr"][acc])
    assert (np.abs(want["d2"][acc].astype(np.float64) - f64["first"][acc]) <= rows["B"][acc]).all()
    assert (np.abs(got["d2"][rows_got].astype(np.float64) - f64["first"][rows_got]) <= rows["B"][rows_got]).all()
    assert (want["corr"][~acc] == -1).all() and (want["d2"][~acc] == K.FLT_MAX).all()      # rejected rows in the reference
    print("icp %s thr %g %s (ran %s): %d accepted; max |d2 - f64| / B: kernel %.3f, product %.3f; d2 bit-equal on %d of %d accepted"
          % (scene, thr, search, ctx.last_icp_search(), acc.sum(), (np.abs(want["d2"][acc] - f64["first"][acc]) / rows["B"][acc]).max(),
             (np.abs(got["d2"][acc] - f64["first"][acc]) / rows["B"][acc]).max(), int((got["d2"][acc] == want["d2"][acc]).sum()), acc.sum()))


@pytest.mark.parametrize("search", ["brute", "pruned", "grid"])
def test_icp_threshold_edge_and_tie_against_reference_kernel(ctx, orc, ref, search):
    """Exact arithmetic, so no bound: a tie goes to the lowest index on both sides; a point at exactly the threshold is accepted by the
    product and the oracle (registration.cpp:338) and rejected by the reference's kernel (strict `<` on squares) - a declared divergence
    (DESIGN.md 2); one float either side of the threshold all agree."""
    src, tgt, T, thr = K.icp_edge_scene()
    sq = (src * src).astype(np.float32)
    d2_cpu = sq[:, 0] + (sq[:, 1] + sq[:, 2])                    # Eigen's squaredNorm: c0 + (c1 + c2)
    d2_kernel = (sq[:, 0] + sq[:, 1]) + sq[:, 2]                 # cuda/icp.cu:41
    kernel_accepts = d2_kernel < np.float32(thr) * np.float32(thr)
    cpu_accepts = ~(np.sqrt(d2_cpu) > np.float32(thr))
    assert kernel_accepts.tolist() == [False, True, False, False] and cpu_accepts.tolist() == [True, True, False, True]
    assert d2_cpu[3] == np.float32(0.25 + 2.0 ** -25) and np.sqrt(np.nextafter(d2_cpu[3], np.float32(1))) > np.float32(thr)
    want = ref.find_correspondences(src, tgt, T, thr)
    ctx.set_icp_search(search)
    try:
        got = ctx.icp_correspondences(src, tgt, T, thr)
    finally:
        ctx.set_icp_search("auto")
    o = orc.icp_correspondences(src, tgt, None, T, thr, point_to_plane=False)
    assert want["corr"].tolist() == [-1, 1, -1, -1] and want["d2"][1] == d2_kernel[1] and (want["d2"][[0, 2, 3]] == K.FLT_MAX).all()
    assert got["accepted"].tolist() == cpu_accepts.tolist() == o["accepted"].tolist() and got["n_corr"] == 3 == o["n_corr"]
    acc = cpu_accepts
    assert got["corr"][acc].tolist() == [1, 1, 1] == o["corr"][acc].tolist()              # index 1, not its duplicate 37
    assert got["d2"][acc].tobytes() == d2_cpu[acc].tobytes() == o["d2"][acc].tobytes()


# ------------------------------------------------------------------ one step's normal equations
def test_normal_equations_reference_kernel_and_oracle(ctx, orc, ref):
    """launchBuildLinearSystem on the product's accepted correspondences and the TRANSFORMED source (what registration.cpp:340-358
    accumulates; the reference's GPU caller passes the untransformed cloud, src/gpu_impl.cpp:202) against the oracle's ATA / ATb.
    Sign convention, asserted below: Jtr = + sum J r with r = (p - q) . n; the solver is then given -Jtr (registration.cpp:361)."""
    thr = 0.01
    src, tgt, nrm, T, f64 = K.icp_scene(700, 600, 42)
    got = ctx.icp_correspondences(src, tgt, T, thr)
    acc = got["accepted"]
    assert np.array_equal(acc, K.icp_rows(f64, thr)["accepted"])
    p = K.transformed_f32(src, T)
    corr = np.where(acc, got["corr"], -1).astype(np.int32)
    d2 = np.where(acc, got["d2"], K.FLT_MAX).astype(np.float32)
    JtJ, Jtr = ref.build_linear_system(p, tgt, nrm, corr, d2, thr)
    o = orc.icp_correspondences(src, tgt, nrm, T, thr)
    assert np.array_equal(o["accepted"], acc) and np.array_equal(o["corr"], got["corr"])
    JJ, Jr_kernel = K.normal_equation_terms(p, tgt, nrm, got["corr"], acc, "kernel")
    _, Jr_oracle = K.normal_equation_terms(p, tgt, nrm, got["corr"], acc, "oracle")
    A64, A_bound = K.sum_bound(JJ)
    bk64, bk_bound = K.sum_bound(Jr_kernel)
    bo64, bo_bound = K.sum_bound(Jr_oracle)
    assert np.array_equal(o["ATA"], o["ATA"].T)                                     # sequential sums of equal terms: exactly symmetric
    assert (np.abs(JtJ - JtJ.T) <= 2 * A_bound).all()                               # float atomics in any order: symmetric within the bound
    assert (np.abs(JtJ.astype(np.float64) - A64) <= A_bound).all()
    assert (np.abs(o["ATA"].astype(np.float64) - A64) <= A_bound).all()
    assert (np.abs(Jtr.astype(np.float64) - bk64) <= bk_bound).all()
    assert (np.abs(o["ATb"].astype(np.float64) - bo64) <= bo_bound).all()
    decided = np.abs(bk64) > 2 * bk_bound                                           # entries whose sign the bound cannot flip
    assert decided.any() and (np.sign(Jtr[decided]) == np.sign(bk64[decided])).all() and (np.sign(o["ATb"][decided]) == np.sign(bk64[decided])).all()
    print("normal equations: %d terms; max |JtJ - f64| / bound %.3f (kernel) %.3f (oracle); Jtr %.3f, ATb %.3f; kernel JtJ exactly symmetric: %s; "
          "max |JtJ - ATA| %.3e, |Jtr - ATb| %.3e"
          % (acc.sum(), _ratio(JtJ - A64, A_bound), _ratio(o["ATA"] - A64, A_bound), _ratio(Jtr - bk64, bk_bound), _ratio(o["ATb"] - bo64, bo_bound), np.array_equal(JtJ, JtJ.T), np.abs(JtJ - o["ATA"]).max(), np.abs(Jtr - o["ATb"]).max()))
