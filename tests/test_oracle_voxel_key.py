"""CPU suite: the voxel key's float -> int conversion is x86's cvttss2si (include/tdv_hip.h, tdv_voxel_downsample): truncation
inside int range, INT_MIN for NaN and everything outside it.  The oracle states it without the undefined cast; here it is held to
the conversion NumPy's cast compiles to on x86, and the oracle's voxel grid to that key."""
import platform

import numpy as np
import pytest

INT_MIN = -2 ** 31
EDGES = np.array([np.nan, -np.nan, np.inf, -np.inf, 2.0 ** 31, np.nextafter(np.float32(2.0 ** 31), np.float32(0)), -2.0 ** 31,
                  np.nextafter(np.float32(-2.0 ** 31), np.float32(-np.inf)), np.nextafter(np.float32(-2.0 ** 31), np.float32(0)),
                  1e19, -1e19, 3e9, -3e9, -0.0, 0.0, 1e-40, -1e-40, 0.5, -0.5, 1.0, -1.0, 2147483520.0, -2147483520.0, 8388608.5],
                 np.float32)
EXPECT = [INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN, 2147483520, INT_MIN, INT_MIN, -2147483520, INT_MIN, INT_MIN, INT_MIN, INT_MIN,
          0, 0, 0, -1, 0, -1, 1, -1, 2147483520, -2147483520, 8388608]


def _keys(orc, v):
    import ctypes as C
    v = np.ascontiguousarray(v, np.float32)
    out = np.empty(len(v), np.int32)
    orc.lib().orc_voxel_key(v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p))
    return out


def test_key_conversion_edges(orc):
    assert _keys(orc, EDGES).tolist() == EXPECT


@pytest.mark.skipif(platform.machine() not in ("x86_64", "AMD64"), reason="NumPy's cast is cvttss2si only on x86")
def test_key_conversion_is_numpys_x86_cast(orc):
    rng = np.random.default_rng(3)
    v = np.concatenate([EDGES, (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 12, 4000)).astype(np.float32)])
    with np.errstate(invalid="ignore"):
        ref = np.floor(v).astype(np.int32)
    assert np.array_equal(_keys(orc, v), ref)


def test_poisoned_points_share_the_int_min_voxel(orc):
    """NaN, +inf, -inf and x = 3e7 m at 1 cm voxels: one voxel keyed (INT_MIN, 0, 0) with a NaN centroid; the two points near the
    origin are a clean voxel of their own.  -2^31 m at 1 m is a finite coordinate whose key is INT_MIN too: the same voxel."""
    pts = np.array([[0.001, 0.002, 0.003], [np.nan, 0.001, 0.001], [np.inf, 0.002, 0.002], [-np.inf, 0.003, 0.003],
                    [3e7, 0.004, 0.004], [0.002, 0.001, 0.001]], np.float32)
    xyz, _, first = orc.voxel_downsample(pts, None, 0.01)
    by_first = {int(f): x for f, x in zip(first, xyz)}
    assert sorted(by_first) == [0, 1]
    assert by_first[0].tobytes() == np.array([0.0015, 0.0015, 0.002], np.float32).tobytes()
    assert np.isnan(by_first[1][0]) and by_first[1][1:].tobytes() == np.array([0.0025, 0.0025], np.float32).tobytes()
    edge = np.array([[-2.0 ** 31, 0.2, 0.2], [np.nan, 0.5, 0.5], [5.0, 0.5, 0.5]], np.float32)
    xyz, _, first = orc.voxel_downsample(edge, None, 1.0)
    assert sorted(first.tolist()) == [0, 2]
