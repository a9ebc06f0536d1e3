"""CPU suite: the voxel stage's shared rules (csrc/voxel_rules.hpp: voxel_cell, voxel_key_code, through the library's host export
tdv_voxel_rules) - the one statement every voxel kernel compiles, held on a machine without a GPU.  The cells are held to the
oracle's key conversion (orc_voxel_key) of floorf(p * inv), the codes to the reference's combiner (src/registration.cpp:20-27) written
out here in uint64 arithmetic over std::hash<int> = the sign-extended value."""
import ctypes as C

import numpy as np
import pytest

from test_oracle_voxel_key import EDGES

VOXELS = (1.0, 0.05, 0.004)


def _inputs():
    rng = np.random.default_rng(3)
    v = np.concatenate([EDGES, (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 12, 4000)).astype(np.float32)])
    # every value in each axis, the other two axes running through the same values out of step
    return np.ascontiguousarray(np.stack([v, np.roll(v, 7), np.roll(v, 1301)], axis=1), np.float32)


def _rules(tdv, xyz, voxel):
    n = len(xyz)
    cells = np.empty((n, 3), np.int32)
    codes = np.empty(n, np.uint64)
    st = tdv.lib().tdv_voxel_rules(xyz.ctypes.data_as(C.c_void_p), C.c_int(n), C.c_float(voxel), cells.ctypes.data_as(C.c_void_p),
                                   codes.ctypes.data_as(C.c_void_p))
    assert st == 0
    return cells, codes


def _orc_keys(orc, floored):
    v = np.ascontiguousarray(floored, np.float32)
    out = np.empty(len(v), np.int32)
    orc.lib().orc_voxel_key(v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p))
    return out


def _combine(cells):
    """registration.cpp:20-27: h = hash(x); h ^= hash(y) + 0x9e3779b9 + (h << 6) + (h >> 2); the same with z"""
    hx, hy, hz = (cells[:, a].astype(np.int64).astype(np.uint64) for a in range(3))     # std::hash<int>: static_cast<size_t>(value)
    k = np.uint64(0x9e3779b9)
    with np.errstate(over="ignore"):
        h = hx.copy()
        h ^= hy + k + (h << np.uint64(6)) + (h >> np.uint64(2))
        h ^= hz + k + (h << np.uint64(6)) + (h >> np.uint64(2))
    return h


@pytest.mark.parametrize("voxel", VOXELS)
def test_cells_are_the_oracles_key_of_the_floored_product(tdv, orc, voxel):
    xyz = _inputs()
    cells, _ = _rules(tdv, xyz, voxel)
    inv = np.float32(1.0) / np.float32(voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        floored = np.floor(xyz * inv)                # f32 throughout
    assert floored.dtype == np.float32
    ref = _orc_keys(orc, floored.reshape(-1)).reshape(-1, 3)
    assert np.array_equal(cells, ref)


@pytest.mark.parametrize("voxel", VOXELS)
def test_codes_are_the_references_combiner_of_the_cells(tdv, voxel):
    cells, codes = _rules(tdv, _inputs(), voxel)
    assert np.array_equal(codes, _combine(cells))
    assert len(np.unique(cells[:, 0])) > 1000 and cells.min() == -2 ** 31       # negative cells, INT_MIN among them, all through the sign extension


def test_bad_arguments(tdv):
    xyz = _inputs()[:4]
    cells = np.empty((4, 3), np.int32); codes = np.empty(4, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = tdv.lib().tdv_voxel_rules
    assert f(p(xyz), C.c_int(-1), C.c_float(1.0), p(cells), p(codes)) < 0
    assert f(p(xyz), C.c_int(4), C.c_float(0.0), p(cells), p(codes)) < 0
    assert f(p(xyz), C.c_int(4), C.c_float(float("nan")), p(cells), p(codes)) < 0
    assert f(None, C.c_int(4), C.c_float(1.0), p(cells), p(codes)) < 0
    assert f(p(xyz), C.c_int(4), C.c_float(1.0), None, p(codes)) < 0
    assert f(p(xyz), C.c_int(4), C.c_float(1.0), p(cells), None) < 0
    assert f(None, C.c_int(0), C.c_float(1.0), None, None) == 0
