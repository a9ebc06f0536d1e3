"""The oracle against what the REFERENCE'S OWN GPU kernels computed on an MI355X (tests/golden/ref_kernels.npz, recorded by
tests/golden/make_golden_ref_kernels.py from oracle/_ref/libtdv_ref_kernels.so).  CPU only: it keeps the oracle pinned to the
reference's code on machines without a GPU, and against host or compiler drift.  Bars as in tests/test_gpu_reference_kernels.py:
  orc.bilateral_filter      zero pattern equal; |oracle - f64| <= 2 max|recorded kernel - f64| (host expf against the device's)
  orc.unproject             count and pixels exact, z the input's bits; x, y and colours within 3 * 2^-24 relative of the kernel's, and
                            not everywhere equal (the oracle divides as src/pipeline.cpp does, the kernel multiplies by a rounded reciprocal)
  orc.icp_correspondences   no row excluded; accepted sets and indices equal; both sides' d2 within B of float64
  its ATA / ATb             they and the recorded JtJ / Jtr within n u sum|term| of the float64 sums; Jtr = + sum J r
"""
import hashlib
import json
import os

import numpy as np
import pytest

import ref_kernel_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def rec():
    vec = dict(np.load(os.path.join(GOLDEN, "ref_kernels.npz")))
    with open(os.path.join(GOLDEN, "meta_ref_kernels.json")) as f:
        return vec, json.load(f)


def test_fixture_is_small_and_complete(rec):
    vec, meta = rec
    assert os.path.getsize(os.path.join(GOLDEN, "ref_kernels.npz")) <= os.path.getsize(os.path.join(GOLDEN, "vectors.npz"))
    assert set(vec) == {"bilateral_0", "bilateral_1", "bilateral_2", "deproject_xy", "deproject_colour_of_byte", "icp_corr_0", "icp_d2_0",
                        "icp_corr_1", "icp_d2_1", "bilateral_3", "JtJ", "Jtr", "system_corr"}
    assert meta["bilateral"]["sigmas"] == [list(s) for s in K.BILATERAL_SIGMAS] and meta["icp"]["thresholds"] == K.ICP_THRESHOLDS


def test_oracle_bilateral_against_recorded_kernel(orc, rec):
    vec, meta = rec
    d = K.bilateral_image(meta["bilateral"]["image"])
    assert sha(d) == meta["bilateral"]["input_sha"], "the input generator no longer gives the recorded image"
    for k, (ss, sr) in enumerate(K.BILATERAL_SIGMAS):
        want = vec["bilateral_%d" % k]
        f64 = K.bilateral_f64(d, ss, sr)
        o = orc.bilateral_filter(d, ss, sr)
        e_ref = float(np.abs(want - f64).max()); e_orc = float(np.abs(o - f64).max())
        print("bilateral sigma (%g, %g): max |kernel - f64| %.3e, |oracle - f64| %.3e, pixels where the oracle differs from the kernel %d of %d"
              % (ss, sr, e_ref, e_orc, int((o != want).sum()), d.size))
        assert np.array_equal(want == 0, d == 0) and np.array_equal(o == 0, d == 0)
        assert 0 < e_ref < 1e-6                      # the recorded kernel is itself a float32 evaluation of the formula
        assert e_orc <= 2 * e_ref, (ss, sr, e_orc, e_ref)


def test_oracle_unproject_against_recorded_kernel(orc, rec):
    vec, meta = rec
    m = meta["deproject"]
    d, bgr = K.deproject_frame(*m["frame"])
    assert sha(d) == m["depth_sha"] and sha(bgr) == m["bgr_sha"], "the input generator no longer gives the recorded frame"
    xyz, rgb = orc.unproject(d, bgr, m["fx"], m["fy"], m["cx"], m["cy"], m["zmax"])
    keep = K.expected_pixels(d, m["zmax"])
    assert len(xyz) == m["count"] == len(keep) == len(vec["deproject_xy"])
    assert np.array_equal(K.pixel_index(rgb), keep)
    assert xyz[:, 2].tobytes() == d.ravel()[keep].tobytes()
    byte_of = np.stack([keep & 255, (keep >> 8) & 255, (keep >> 16) & 255], axis=1)
    want = np.concatenate([vec["deproject_xy"], vec["deproject_colour_of_byte"][byte_of]], axis=1).astype(np.float64)
    got = np.concatenate([xyz[:, :2], rgb], axis=1).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any()
    ok = ~np.isnan(want)
    diff = np.abs(got - want)[ok]; scale = np.maximum(np.abs(got), np.abs(want))[ok]
    assert (diff <= 3 * K.U * scale).all()
    for col in (0, 1, 2):                            # x, y and the red channel (every byte value) each differ somewhere: the declared divergence
        assert (got[ok[:, col], col] != want[ok[:, col], col]).any(), col


def test_oracle_correspondences_against_recorded_kernel(orc, rec):
    vec, meta = rec
    src, tgt, nrm, T, f64 = K.icp_scene(*meta["icp"]["scene"])
    assert (sha(src), sha(tgt), sha(T)) == (meta["icp"]["src_sha"], meta["icp"]["tgt_sha"], meta["icp"]["T_sha"]), "the scene generator no longer gives the recorded scene"
    for k, thr in enumerate(K.ICP_THRESHOLDS):
        rows = K.icp_rows(f64, thr)
        assert not rows["tie"].any() and not rows["edge"].any()
        acc = rows["accepted"]
        corr, d2 = vec["icp_corr_%d" % k], vec["icp_d2_%d" % k]
        o = orc.icp_correspondences(src, tgt, nrm, T, thr)
        assert np.array_equal(corr >= 0, acc) and np.array_equal(o["accepted"], acc) and o["n_corr"] == acc.sum() > 30
        assert np.array_equal(corr[acc], f64["index"][acc]) and np.array_equal(o["corr"], f64["index"])
        assert (np.abs(d2[acc].astype(np.float64) - f64["first"][acc]) <= rows["B"][acc]).all()
        assert (np.abs(o["d2"].astype(np.float64) - f64["first"]) <= rows["B"]).all()
        assert (corr[~acc] == -1).all() and (d2[~acc] == K.FLT_MAX).all()


def test_oracle_normal_equations_against_recorded_kernel(orc, rec):
    vec, meta = rec
    m = meta["system"]
    src, tgt, nrm, T, f64 = K.icp_scene(*m["scene"])
    p = K.transformed_f32(src, T)
    assert (sha(src), sha(tgt), sha(nrm), sha(T), sha(p)) == (m["src_sha"], m["tgt_sha"], m["normals_sha"], m["T_sha"], m["transformed_sha"]), \
        "the scene generator no longer gives the recorded scene"
    o = orc.icp_correspondences(src, tgt, nrm, T, m["thr"])
    acc = o["accepted"]
    assert acc.sum() == m["accepted"] and np.array_equal(vec["system_corr"] >= 0, acc) and np.array_equal(vec["system_corr"][acc], o["corr"][acc])
    JJ, Jr_kernel = K.normal_equation_terms(p, tgt, nrm, o["corr"], acc, "kernel")
    _, Jr_oracle = K.normal_equation_terms(p, tgt, nrm, o["corr"], acc, "oracle")
    A64, A_bound = K.sum_bound(JJ)
    bk64, bk_bound = K.sum_bound(Jr_kernel)
    bo64, bo_bound = K.sum_bound(Jr_oracle)
    JtJ, Jtr = vec["JtJ"], vec["Jtr"]
    assert np.array_equal(o["ATA"], o["ATA"].T) and (np.abs(JtJ - JtJ.T) <= 2 * A_bound).all()
    assert (np.abs(JtJ.astype(np.float64) - A64) <= A_bound).all() and (np.abs(o["ATA"].astype(np.float64) - A64) <= A_bound).all()
    assert (np.abs(Jtr.astype(np.float64) - bk64) <= bk_bound).all() and (np.abs(o["ATb"].astype(np.float64) - bo64) <= bo_bound).all()
    # the float32 terms the bound is about are the oracle's own: added in source order they give its sums to the bit
    A32 = np.zeros((6, 6), np.float32); b32 = np.zeros(6, np.float32)
    for k in range(len(JJ)):
        A32 += JJ[k]; b32 += Jr_oracle[k]
    assert A32.tobytes() == o["ATA"].tobytes() and b32.tobytes() == o["ATb"].tobytes()
    decided = np.abs(bk64) > 2 * bk_bound            # sign convention: Jtr = + sum J r, r = (p - q) . n
    assert decided.any() and (np.sign(Jtr[decided]) == np.sign(bk64[decided])).all() and (np.sign(o["ATb"][decided]) == np.sign(bo64[decided])).all()


def test_oracle_threshold_edge_and_tie(orc):
    """The constructed exact scene of the GPU test, on the CPU: the oracle accepts d == thr and the largest d2 whose root rounds to thr
    (registration.cpp:338), where the reference's kernel rule `d2 < thr^2` (cuda/icp.cu:48, run on the GPU by
    tests/test_gpu_reference_kernels.py) does not; a tie goes to the lowest index."""
    src, tgt, T, thr = K.icp_edge_scene()
    sq = (src * src).astype(np.float32)
    d2 = sq[:, 0] + (sq[:, 1] + sq[:, 2])
    o = orc.icp_correspondences(src, tgt, None, T, thr, point_to_plane=False)
    assert o["accepted"].tolist() == [True, True, False, True] == (~(np.sqrt(d2) > np.float32(thr))).tolist()
    assert (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) < np.float32(thr) * np.float32(thr)).tolist() == [False, True, False, False]
    assert o["corr"].tolist() == [1, 1, 1, 1] and o["d2"].tobytes() == d2.tobytes() and o["n_corr"] == 3
