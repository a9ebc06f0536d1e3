"""Callers of the reference's own GPU kernels — TEST INFRASTRUCTURE ONLY.

oracle/_ref/libtdv_ref_kernels.so is the reference's cuda/*.cu compiled for gfx950 by oracle/ref_kernels.py (run by
__graft_entry__.build() where the reference tree exists).  This module loads it and calls its five launchers through
ctypes, by their mangled names, looked up in the library by the launcher's plain name.  There is no C++ wrapper.

Inputs are numpy arrays or torch tensors on the device; device buffers are torch tensors, results come back as numpy.
Every launcher runs on the null stream and synchronises the device itself before it returns.  What each launcher needs,
read from its source:

  launchDepthPreprocess      reads the mask only with apply_mask and a non-null pointer; forms 1.0f / scale in f32.
  launchBilateralFilter      radius int(2 sigma_s + 0.5), clamped to 5 (it prints a line to stderr when it clamps).
  launchDeproject            ALWAYS reads the colour image (BGR, 3 bytes a pixel); clears the counter itself; writes
                             interleaved x y z r g b rows in the order its atomics come out, up to width * height rows.
  launchFindCorrespondences  transform as 16 row-major floats (it reads the first 12); takes max_distance and squares it;
                             a rejected row reads -1 / FLT_MAX.
  launchBuildLinearSystem    clears JtJ (row-major 6 x 6) and Jtr itself; reads `source` AS GIVEN.  The reference's caller
                             (src/gpu_impl.cpp:197-206) hands it the untransformed cloud; a caller that wants the normal
                             equations of registration.cpp:340-358 passes the transformed one.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import ref_kernels

LIB_PATH = ref_kernels.LIB
_LIB = None


class RefKernelsMissing(RuntimeError):
    pass


def lib():
    """{plain launcher name: ctypes function}.  Raises when the library has not been built: there is nothing to fall back on."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RefKernelsMissing("%s is not built: run __graft_entry__.build() on a machine that holds the reference tree "
                                    "(oracle/ref_kernels.py); the reference's kernels are the only pin these tests have, "
                                    "so nothing stands in for them." % LIB_PATH)
        if "torch" not in sys.modules:   # torch first, as 3dvision_amd.lib() does: one HIP runtime in the process
            import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        fns = {}
        for name, mangled in ref_kernels.mangled_names(LIB_PATH).items():
            fns[name] = getattr(l, mangled)
            fns[name].restype = None
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        fns["launchDepthPreprocess"].argtypes = [vp, vp, vp, i, i, f, C.c_bool]
        fns["launchBilateralFilter"].argtypes = [vp, vp, i, i, f, f]
        fns["launchDeproject"].argtypes = [vp, vp, vp, vp, i, i, f, f, f, f, f]
        fns["launchFindCorrespondences"].argtypes = [vp, vp, vp, vp, i, i, vp, f]
        fns["launchBuildLinearSystem"].argtypes = [vp, vp, vp, vp, vp, vp, vp, i, f]
        _LIB = fns
    return _LIB


def _dev(a, dtype, device=0):
    """A contiguous tensor of `dtype` on the device from a numpy array or a tensor (uint16 travels as int16 bits)."""
    import torch
    if isinstance(a, torch.Tensor):
        t = a.to(torch.device("cuda", device)).contiguous()
        assert t.element_size() == np.dtype(dtype).itemsize, (t.dtype, dtype)
        return t
    a = np.ascontiguousarray(a, dtype)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(torch.device("cuda", device))


def _empty(shape, dtype, device=0):
    import torch
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", device))


def _sync():
    import torch
    torch.cuda.synchronize()


def depth_preprocess(raw, mask, scale, apply_mask=True):
    """float32 [h, w]: raw * (1.0f / scale), zero where the mask byte is 0 (apply_mask and a mask given)."""
    import torch
    fn = lib()["launchDepthPreprocess"]
    h, w = raw.shape
    assert h > 0 and w > 0
    d_raw = _dev(raw, np.uint16)
    d_mask = None if mask is None else _dev(mask, np.uint8)
    assert d_raw.numel() == h * w and (d_mask is None or d_mask.numel() == h * w)
    d_out = _empty((h, w), torch.float32)
    _sync()
    fn(d_raw.data_ptr(), None if d_mask is None else d_mask.data_ptr(), d_out.data_ptr(), w, h, float(scale), bool(apply_mask))
    return d_out.cpu().numpy()


def bilateral_filter(depth, sigma_spatial, sigma_range):
    import torch
    fn = lib()["launchBilateralFilter"]
    h, w = depth.shape
    assert h > 0 and w > 0
    d_in = _dev(depth, np.float32)
    assert d_in.numel() == h * w
    d_out = _empty((h, w), torch.float32)
    _sync()
    fn(d_in.data_ptr(), d_out.data_ptr(), w, h, float(sigma_spatial), float(sigma_range))
    return d_out.cpu().numpy()


def deproject(depth, bgr, fx, fy, cx, cy, max_depth):
    """(rows float32 [count, 6] as x y z r g b in the kernel's own, arbitrary order, count)."""
    import torch
    fn = lib()["launchDeproject"]
    h, w = depth.shape
    assert h > 0 and w > 0 and bgr is not None, "launchDeproject always reads the colour image"
    d_depth = _dev(depth, np.float32)
    d_bgr = _dev(bgr, np.uint8)
    assert d_depth.numel() == h * w and d_bgr.numel() == 3 * h * w
    d_rows = _empty((h * w, 6), torch.float32)      # the capacity the launcher computes: width * height rows
    d_count = _empty((1,), torch.int32)
    _sync()
    fn(d_depth.data_ptr(), d_bgr.data_ptr(), d_rows.data_ptr(), d_count.data_ptr(), w, h, float(fx), float(fy), float(cx), float(cy),
       float(max_depth))
    n = int(d_count.cpu()[0])
    assert 0 <= n <= h * w, n
    return d_rows[:n].cpu().numpy(), n


def find_correspondences(src, tgt, T, max_distance):
    """dict(corr int32 [ns] (-1 when rejected), d2 float32 [ns] (FLT_MAX when rejected)); T is an ordinary row-major [4, 4]."""
    import torch
    fn = lib()["launchFindCorrespondences"]
    d_src = _dev(src, np.float32); d_tgt = _dev(tgt, np.float32)
    ns, nt = d_src.shape[0], d_tgt.shape[0]
    assert ns > 0 and nt > 0 and d_src.numel() == 3 * ns and d_tgt.numel() == 3 * nt
    d_T = _dev(np.asarray(T, np.float32).reshape(16), np.float32)
    d_corr = _empty((ns,), torch.int32); d_d2 = _empty((ns,), torch.float32)
    _sync()
    fn(d_src.data_ptr(), d_tgt.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), ns, nt, d_T.data_ptr(), float(max_distance))
    return dict(corr=d_corr.cpu().numpy(), d2=d_d2.cpu().numpy())


def build_linear_system(source, tgt, tgt_normals, corr, d2, max_distance):
    """(JtJ float32 [6, 6], Jtr float32 [6]) over the rows with corr >= 0 and d2 < max_distance^2; `source` is read as given."""
    import torch
    fn = lib()["launchBuildLinearSystem"]
    d_src = _dev(source, np.float32); d_tgt = _dev(tgt, np.float32); d_nrm = _dev(tgt_normals, np.float32)
    ns, nt = d_src.shape[0], d_tgt.shape[0]
    corr = np.ascontiguousarray(corr, np.int32)
    assert ns > 0 and d_src.numel() == 3 * ns and d_tgt.numel() == 3 * nt and d_nrm.numel() == 3 * nt and len(corr) == ns and len(d2) == ns
    assert corr.max() < nt, "a correspondence index past the target would be read out of bounds"
    d_corr = _dev(corr, np.int32); d_d2 = _dev(d2, np.float32)
    d_JtJ = _empty((36,), torch.float32); d_Jtr = _empty((6,), torch.float32)
    _sync()
    fn(d_src.data_ptr(), d_tgt.data_ptr(), d_nrm.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(), d_JtJ.data_ptr(), d_Jtr.data_ptr(), ns,
       float(max_distance))
    return d_JtJ.cpu().numpy().reshape(6, 6), d_Jtr.cpu().numpy()
