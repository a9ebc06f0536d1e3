"""CPU suite: multi-scale ICP and the voxel grid that keeps normals (include/tdv_hip.h: tdv_icp_multiscale, tdv_voxel_downsample_normals).
The ABI exports the six entry points, every one that takes a ctx refuses a null ctx before it looks at another argument (the other
arguments here are all invalid as well) and writes nothing, and tdv_icp_level_default writes the stated defaults.  No compute entry point
of the library runs here; tests/test_gpu_voxel_normals.py and tests/test_gpu_icp_multiscale.py hold the device to the oracle."""
import ctypes as C
import math

import numpy as np

TDV_ERR_BAD_ARG = -2
F = np.float32
SYMBOLS = ("tdv_voxel_downsample_normals", "tdv_voxel_downsample_normals_dev", "tdv_icp_level_default", "tdv_icp_multiscale",
           "tdv_icp_multiscale_dev", "tdv_icp_multiscale_batch_dev")


def test_symbols(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)


def test_level_default(tdv):
    lv = tdv.IcpLevelC()
    C.memset(C.byref(lv), 0x5A, C.sizeof(lv))
    tdv.lib().tdv_icp_level_default(C.byref(lv))
    assert lv.voxel_size == -1.0 and lv.max_correspondence_distance == 0.0 and lv.max_iterations == 30
    assert math.isinf(lv.relative_fitness) and lv.relative_fitness > 0
    assert np.float32(lv.relative_rmse).tobytes() == np.float32(1e-6).tobytes()
    assert C.sizeof(tdv.IcpLevelC) == 20 and C.sizeof(tdv.IcpLevelResultC) == C.sizeof(tdv.IcpResultC) + 8
    tdv.lib().tdv_icp_level_default(None)                      # nothing to write to: returns


def test_null_ctx_before_anything_else(tdv):
    lib = tdv.lib()
    out = (tdv.IcpLevelResultC * 2)(); C.memset(out, 0x5A, C.sizeof(out)); before = bytes(out)
    n_out = C.c_int(77)
    # every other argument is bad too: NULL arrays with points, negative counts, no levels - the null ctx is what is answered
    assert lib.tdv_icp_multiscale(None, None, None, -1, None, None, -1, None, None, 0, 99, C.c_float(float("nan")), out) == TDV_ERR_BAD_ARG
    assert lib.tdv_icp_multiscale_dev(None, None, None, -1, None, None, -1, None, None, 0, 99, C.c_float(float("nan")), out) == TDV_ERR_BAD_ARG
    assert lib.tdv_icp_multiscale_batch_dev(None, None, None, None, -1, None, None, -1, None, None, 0, 99, C.c_float(float("nan")), out) == TDV_ERR_BAD_ARG
    assert lib.tdv_voxel_downsample_normals(None, None, None, None, -1, C.c_float(-1.0), 7, None, None, None, -1, C.byref(n_out)) == TDV_ERR_BAD_ARG
    assert lib.tdv_voxel_downsample_normals_dev(None, None, None, None, -1, C.c_float(-1.0), 7, None, None, None, -1, C.byref(n_out)) == TDV_ERR_BAD_ARG
    assert bytes(out) == before and n_out.value == 77
    # ... and with good arguments
    pts = np.zeros((4, 3), F); p = pts.ctypes.data_as(C.c_void_p)
    T0 = (C.c_float * 16)(*tdv.to_colmajor16(np.eye(4)))
    lv = tdv.icp_levels([0.02, None], [0.04, 0.01], [5, 5])
    off = (C.c_int * 2)(0, 4)
    assert lib.tdv_icp_multiscale(None, p, p, 4, p, p, 4, T0, lv, 2, 0, C.c_float(1e-3), out) == TDV_ERR_BAD_ARG
    assert lib.tdv_icp_multiscale_dev(None, p, p, 4, p, p, 4, T0, lv, 2, 0, C.c_float(1e-3), out) == TDV_ERR_BAD_ARG
    assert lib.tdv_icp_multiscale_batch_dev(None, p, p, off, 1, p, p, 4, T0, lv, 2, 0, C.c_float(1e-3), out) == TDV_ERR_BAD_ARG
    assert bytes(out) == before


def test_icp_levels_broadcasts(tdv):
    lv = tdv.icp_levels([0.04, 0.02, None], 0.01, [20, 20, 50], relative_rmse=1e-5)
    assert lv.n_levels == 3
    assert [np.float32(l.voxel_size) for l in lv[:3]] == [np.float32(0.04), np.float32(0.02), np.float32(-1.0)]
    assert all(np.float32(l.max_correspondence_distance) == np.float32(0.01) for l in lv[:3])
    assert [l.max_iterations for l in lv[:3]] == [20, 20, 50]
    assert all(math.isinf(l.relative_fitness) and np.float32(l.relative_rmse) == np.float32(1e-5) for l in lv[:3])
