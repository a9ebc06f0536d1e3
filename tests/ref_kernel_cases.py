"""Inputs, float64 evaluations and derived bounds shared by tests/test_gpu_reference_kernels.py (the product's kernels against the
reference's own GPU kernels, oracle/refkernels.py), tests/golden/make_golden_ref_kernels.py (which records those kernels' outputs
on the GPU) and tests/test_oracle_reference_kernels.py (the oracle against the recorded outputs, on the CPU).  Everything is
generated from seeds; nothing here reads the reference tree."""
import importlib

import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32
FLT_MAX = np.finfo(np.float32).max

# ------------------------------------------------------------------ depth preprocess
PREPROCESS_SIZES = [(1, 1), (7, 5), (97, 131), (33, 1023), (3, 256)]
PREPROCESS_SCALES = [1000.0, 999.0, 4000.0, 0.25]


def preprocess_frame(h, w):
    """raw: full-range uint16 with 0 and 65535 present (each alone on a 1 x 1 frame is a case of its own in the test); mask: every
    byte value 0..255 in every row that is wide enough to hold them (w >= 256), otherwise the values cycle through the frame."""
    rng = np.random.default_rng(h * 10007 + w)
    raw = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    raw.flat[0] = 65535
    raw.flat[-1] = 0 if raw.size > 1 else 65535
    if raw.size > 2:
        raw.flat[raw.size // 2] = 0
    mask = np.empty((h, w), np.uint8)
    for r in range(h):
        row = (np.arange(w) + 37 * r) % 256
        mask[r] = rng.permutation(row).astype(np.uint8)
    return raw, mask


# ------------------------------------------------------------------ bilateral filter
# radius 3, 1, and 5 by clamping (tests/test_gpu_depth.py); and 3 only because int(2 sigma + 0.5) rounds 2.6 UP, which the first three do not tell
# from int(2 sigma)
BILATERAL_SIGMAS = [(1.5, 0.02), (0.6, 0.01), (4.0, 0.05), (1.3, 0.03)]


def bilateral_image(name):
    def noisy(h, w, seed, zeros=0.15):
        rng = np.random.default_rng(seed)
        d = (0.8 + 0.05 * rng.random((h, w))).astype(np.float32)
        d[rng.random(d.shape) < zeros] = 0.0
        return d
    if name == "123x211":                                            # the image of tests/test_gpu_depth.py::test_bilateral_filter
        return noisy(123, 211, 5)
    if name == "1x1":
        return np.full((1, 1), 0.9, np.float32)
    if name == "5x300":                                              # fewer rows than the window
        return noisy(5, 300, 6)
    if name == "70x64":                                              # a 64-pixel segment exactly full
        return noisy(70, 64, 7)
    if name == "70x65":                                              # ... and one pixel over
        return noisy(70, 65, 8)
    if name == "zero":
        return np.zeros((40, 130), np.float32)
    if name == "lone_corner":
        d = np.zeros((40, 130), np.float32); d[0, 0] = 0.5; d[39, 129] = 0.6; d[0, 129] = 0.7
        return d
    raise KeyError(name)


BILATERAL_IMAGES = ["123x211", "1x1", "5x300", "70x64", "70x65", "zero", "lone_corner"]


def bilateral_f64(d, sigma_spatial, sigma_range):
    """The filter's formula in float64 (cuda/depth_processing.cu:100-121).  The radius and the two exponent scales are the float32
    values every implementation is handed (host code, the same three lines everywhere); all pixel arithmetic is float64."""
    ss, sr = np.float32(sigma_spatial), np.float32(sigma_range)
    radius = min(5, int(np.float32(2.0) * ss + np.float32(0.5)))
    k_s = float(np.float32(-0.5) / (ss * ss)); k_r = float(np.float32(-0.5) / (sr * sr))
    h, w = d.shape
    pad = np.zeros((h + 2 * radius, w + 2 * radius), np.float64)
    pad[radius:radius + h, radius:radius + w] = d
    c = d.astype(np.float64)
    sw = np.zeros((h, w)); sv = np.zeros((h, w))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            nb = pad[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
            wgt = np.where(nb > 0, np.exp((dx * dx + dy * dy) * k_s + (nb - c) ** 2 * k_r), 0.0)
            sw += wgt; sv += wgt * nb
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(sw > 0, sv / sw, c)
    return np.where(c > 0, out, 0.0)


# ------------------------------------------------------------------ deproject
INTRINSICS = dict(plain=(611.5, 609.25, 153.2, 101.7), negative_fx=(-611.5, 609.25, 153.2, 101.7))


def deproject_frame(seed, h, w):
    """Depth from tests/test_gpu_depth.py's _random_frame (scaled and masked by plain numpy: raw * fl(1/1000), zero where mask <= 10),
    one NaN pixel, and a colour image that carries the pixel index in its 24 bits (R low byte, then G, then B)."""
    from test_gpu_depth import _random_frame
    raw, mask, _ = _random_frame(seed, h, w)
    d = raw.astype(np.float32) * np.float32(1.0 / 1000.0)
    d[mask <= 10] = 0
    d[h // 2, w // 3] = np.nan
    idx = np.arange(h * w, dtype=np.uint32).reshape(h, w)
    bgr = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=2).astype(np.uint8)
    return d, bgr


def pixel_index(colours):
    """The pixel index back from r g b float colours: rint(c * 255) per channel."""
    c = np.rint(colours.astype(np.float64) * 255.0).astype(np.int64)
    assert c.min() >= 0 and c.max() <= 255
    return c[:, 0] + 256 * c[:, 1] + 65536 * c[:, 2]


def expected_pixels(d, zmax):
    """Row-major indices of the pixels both sides keep: !(z <= 0 || z > zmax), so a NaN depth stays."""
    z = d.ravel()
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~((z <= 0) | (z > np.float32(zmax))))


# ------------------------------------------------------------------ ICP correspondences
ICP_SCENES = [(700, 600, 42), (1000, 257, 7), (65, 4097, 3)]
ICP_THRESHOLDS = [0.004, 0.01]
_scene_cache = {}


def icp_scene(ns, nt, seed):
    """(src, tgt, tgt_normals, T) with T a perturbed ground truth; and the float64 side, computed once and shared."""
    key = (ns, nt, seed)
    if key not in _scene_cache:
        synth = importlib.import_module("3dvision_amd.synth")
        tgt, nrm = synth.sample_object(nt, seed)
        src, T_gt = synth.make_scene(ns, seed)
        T = synth.perturb(T_gt, seed).astype(np.float32)
        _scene_cache[key] = (src, tgt, nrm, T, nearest_f64(src, tgt, T))
    return _scene_cache[key]


def nearest_f64(src, tgt, T):
    """Per source point, in float64 on the float32 inputs: nearest and second-nearest squared distance, the nearest index, and
    E = sqrt(3) * 4u * max_row(|R||s| + |t|): the norm of the error of a float32 transformed point (gamma_4 for three products and
    three sums per row, whatever their order)."""
    T64 = T.astype(np.float64); s = src.astype(np.float64); t = tgt.astype(np.float64)
    p = s @ T64[:3, :3].T + T64[:3, 3]
    d2 = ((p[:, None, :] - t[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(s))
    first = d2[rows, order[:, 0]]
    second = d2[rows, order[:, 1]] if t.shape[0] > 1 else np.full(len(s), np.inf)
    mag = np.abs(s) @ np.abs(T64[:3, :3]).T + np.abs(T64[:3, 3])
    E = np.sqrt(3.0) * 4 * U * mag.max(axis=1)
    return dict(index=order[:, 0], first=first, second=second, E=E)


def d2_bound(d2, E):
    """B(d2) = 2 sqrt(d2) E + 8u d2 + E^2: a float32 squared distance from a float32 transformed point against the float64 one.
    |p' - p| <= E moves the distance by at most E, so d2 by 2 sqrt(d2) E + E^2; the three differences, three squares and two sums
    add at most (1+u)^2 (1+u) (1+u)^2 - 1 < 8u relative."""
    return 2 * np.sqrt(d2) * E + 8 * U * d2 + E * E


def icp_rows(f64, thr):
    """What float64 says about each row at threshold thr, and which rows a float32 side may legitimately decide differently:
    `tie` (the two nearest closer than their two bounds) and `edge` (the nearest within its bound, plus 2u thr^2 for the float32
    square of the threshold or the square root's rounding, of thr^2)."""
    thr2 = float(np.float32(thr)) ** 2
    B1 = d2_bound(f64["first"], f64["E"]); B2 = d2_bound(f64["second"], f64["E"])
    tie = ~(f64["second"] - f64["first"] > B1 + B2)
    edge = ~(np.abs(f64["first"] - thr2) > B1 + 2 * U * thr2)
    return dict(accepted=f64["first"] < thr2, tie=tie, edge=edge, B=B1)


def icp_edge_scene():
    """A constructed scene whose float32 arithmetic is exact on every side (identity transform, coordinates on the x axis): 40 targets,
    the origin twice (indices 1 and 37, a tie the lowest index wins on both sides) and the rest far away; sources at distance exactly
    thr = 0.5, one float below, one float above, and (0.5, 2^-13, 2^-13), whose squared distance summed as the CPU path sums it,
    0.25 + (2^-26 + 2^-26) = 0.25 + 2^-25, is the largest float whose square root still rounds to 0.5.  At d == thr the reference's
    CPU path accepts (registration.cpp:338, `d > thr` rejects) and its GPU kernel rejects (cuda/icp.cu:48, `d2 < thr^2` accepts): the
    product follows the CPU path."""
    tgt = np.zeros((40, 3), np.float32); tgt[:, 0] = 10.0 + np.arange(40); tgt[1] = 0; tgt[37] = 0
    half = np.float32(0.5)
    src = np.zeros((4, 3), np.float32); src[:, 0] = [half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), half]
    src[3, 1:] = 2.0 ** -13
    return src, tgt, np.eye(4, dtype=np.float32), 0.5


def transformed_f32(src, T):
    """The source under T in float32 as the oracle forms it (small_linalg.hpp mulv: c0 + (c1 + c2), then + t)."""
    R = T[:3, :3].astype(np.float32); t = T[:3, 3].astype(np.float32); s = src.astype(np.float32)
    cols = []
    for i in range(3):
        cols.append((R[i, 0] * s[:, 0] + (R[i, 1] * s[:, 1] + R[i, 2] * s[:, 2])) + t[i])
    return np.stack(cols, axis=1).astype(np.float32)


def normal_equation_terms(p, tgt, nrm, corr, accepted, residual_order):
    """float32 terms of one point-to-plane step over the accepted rows: J = [p x n | n], r = (p - q) . n with the three products
    summed as 'oracle' (a + (b + c), small_linalg.hpp dot3) or 'kernel' ((a + b) + c, cuda/icp.cu:127).  Returns (JJ [n,6,6], Jr [n,6])."""
    p = p[accepted]; q = tgt[corr[accepted]]; n = nrm[corr[accepted]]
    J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], axis=1).astype(np.float32)
    a, b, c = ((p[:, k] - q[:, k]) * n[:, k] for k in range(3))
    r = (a + (b + c)) if residual_order == "oracle" else ((a + b) + c)
    assert J.dtype == np.float32 and r.dtype == np.float32
    return J[:, :, None] * J[:, None, :], J * r[:, None]


def sum_bound(terms):
    """(float64 sum, n u sum|term|) over axis 0: any-order float32 summation of n terms stays within the second of the first."""
    t = terms.astype(np.float64)
    return t.sum(axis=0), len(t) * U * np.abs(t).sum(axis=0)
