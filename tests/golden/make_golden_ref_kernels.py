"""Records what the REFERENCE'S OWN GPU kernels (oracle/_ref/libtdv_ref_kernels.so, see oracle/ref_kernels.py) compute on an MI355X into
tests/golden/ref_kernels.npz, with the inputs' seeds, shapes and hashes in meta_ref_kernels.json.  Run once on the GPU:

    python tests/golden/make_golden_ref_kernels.py [output directory, default tests/golden]

The arrays are data those kernels wrote, not their text.  tests/test_oracle_reference_kernels.py holds the oracle to them on machines
without a GPU; the inputs come from tests/ref_kernel_cases.py, by seed.  Recorded:
  bilateral_<k>   launchBilateralFilter on the 70 x 65 image at the three sigma pairs
  deproject_xy    launchDeproject on the 97 x 131 frame (zmax 1.5), rows sorted by pixel index: x and y; z is checked here to be the input's
                  bits and the colours to be one float per byte value, stored as the 256-entry table deproject_colour_of_byte
  icp_corr_<t>, icp_d2_<t>   launchFindCorrespondences on the (1000, 257, seed 7) scene at both thresholds
  JtJ, Jtr        launchBuildLinearSystem on the (700, 600, seed 42) scene at 0.01, from that launcher's own correspondences and the
                  float32 transformed source
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before any HIP library)
import ref_kernel_cases as K  # noqa: E402
from oracle import refkernels as ref  # noqa: E402

DEPROJECT = dict(frame=(0, 97, 131), intrinsics="plain", zmax=1.5)
SYSTEM = dict(scene=(700, 600, 42), thr=0.01)
CORR_SCENE = (1000, 257, 7)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main(out_dir):
    vec, meta = {}, {}
    d = K.bilateral_image("70x65")
    meta["bilateral"] = dict(image="70x65", shape=list(d.shape), input_sha=sha(d), sigmas=K.BILATERAL_SIGMAS)
    for k, (ss, sr) in enumerate(K.BILATERAL_SIGMAS):
        vec["bilateral_%d" % k] = ref.bilateral_filter(d, ss, sr)

    depth, bgr = K.deproject_frame(*DEPROJECT["frame"])
    fx, fy, cx, cy = K.INTRINSICS[DEPROJECT["intrinsics"]]
    rows, n = ref.deproject(depth, bgr, fx, fy, cx, cy, DEPROJECT["zmax"])
    pix = K.pixel_index(rows[:, 3:6]); order = np.argsort(pix, kind="stable")
    rows = rows[order]; pix = pix[order]
    keep = K.expected_pixels(depth, DEPROJECT["zmax"])
    assert np.array_equal(pix, keep)
    assert rows[:, 2].tobytes() == depth.ravel()[keep].tobytes()
    byte_of = np.stack([pix & 255, (pix >> 8) & 255, (pix >> 16) & 255], axis=1)
    table = np.zeros(256, np.float32); seen = np.zeros(256, bool)
    table[byte_of.ravel()] = rows[:, 3:6].ravel(); seen[byte_of.ravel()] = True
    assert seen.all() and rows[:, 3:6].tobytes() == table[byte_of].tobytes()          # the colour is a function of the byte alone
    vec["deproject_xy"] = rows[:, :2].copy(); vec["deproject_colour_of_byte"] = table
    meta["deproject"] = dict(DEPROJECT, fx=fx, fy=fy, cx=cx, cy=cy, count=int(n), depth_sha=sha(depth), bgr_sha=sha(bgr))

    src, tgt, nrm, T, _ = K.icp_scene(*CORR_SCENE)
    meta["icp"] = dict(scene=list(CORR_SCENE), thresholds=K.ICP_THRESHOLDS, src_sha=sha(src), tgt_sha=sha(tgt), T_sha=sha(T))
    for k, thr in enumerate(K.ICP_THRESHOLDS):
        r = ref.find_correspondences(src, tgt, T, thr)
        vec["icp_corr_%d" % k] = r["corr"]; vec["icp_d2_%d" % k] = r["d2"]

    src, tgt, nrm, T, _ = K.icp_scene(*SYSTEM["scene"])
    r = ref.find_correspondences(src, tgt, T, SYSTEM["thr"])
    p = K.transformed_f32(src, T)
    JtJ, Jtr = ref.build_linear_system(p, tgt, nrm, r["corr"], r["d2"], SYSTEM["thr"])
    vec["JtJ"] = JtJ; vec["Jtr"] = Jtr; vec["system_corr"] = r["corr"]
    meta["system"] = dict(scene=list(SYSTEM["scene"]), thr=SYSTEM["thr"], accepted=int((r["corr"] >= 0).sum()), src_sha=sha(src), tgt_sha=sha(tgt),
                          normals_sha=sha(nrm), T_sha=sha(T), transformed_sha=sha(p))
    meta["device"] = torch.cuda.get_device_name(0)
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "ref_kernels.npz"), **vec)
    with open(os.path.join(out_dir, "meta_ref_kernels.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", out_dir, {k: v.shape for k, v in vec.items()}, os.path.getsize(os.path.join(out_dir, "ref_kernels.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
