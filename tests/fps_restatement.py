"""Farthest point sampling as include/tdv_hip.h (tdv_farthest_point_down_sample) states it, in numpy f32: a running-minimum array and an
arg-max per sample.  tests/test_fps_abi.py holds it to an independent definition; tests/test_gpu_fps.py holds the device to it byte for
byte."""
import numpy as np

F = np.float32
MAX_POINTS = 1 << 22
WORKGROUP_LANES = 1024
WORKGROUP_MAX = 16384
AUTO, WORKGROUP, GRID = 0, 1, 2
RESULT = ("n_usable", "n_selected", "path", "cover_d2")


def d2_f32(p, s):
    """Rule 3: (dx * dx + dy * dy) + dz * dz, every operation rounded to f32."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - s).astype(F)
        return ((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)


def path_of(n, mode=AUTO):
    return mode if mode != AUTO else (WORKGROUP if n <= WORKGROUP_MAX else GRID)


def fps(xyz, num_samples, start_index=0, attr=None, mode=AUTO):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    usable = np.isfinite(xyz).all(1)                                              # rule 1
    n_usable = int(usable.sum())
    k = min(int(num_samples), n_usable)                                           # rule 2
    m = np.full(n, np.inf, F)
    cand = usable.copy()
    index, d2 = np.zeros(k, np.int32), np.zeros(k, F)
    for i in range(k):
        if i == 0:
            j = start_index if usable[start_index] else int(np.argmax(usable))   # rule 5
        else:
            j = int(np.argmax(np.where(cand, m, F(-1))))                          # rule 6: the first of the largest
        index[i], d2[i] = j, m[j]
        cand[j] = False                                                           # rule 7
        d = d2_f32(xyz, xyz[j])
        with np.errstate(invalid="ignore"):
            m = np.where(usable & (d < m), d, m)                                  # rule 4
    cover = F(np.where(cand, m, F(0)).max()) if cand.any() else F(0)              # rule 9
    return dict(n_usable=n_usable, n_selected=k, path=path_of(n, mode), cover_d2=cover, index=index, d2=d2, xyz=xyz[index].copy(),
                attr=None if attr is None else np.ascontiguousarray(attr, F)[index].copy())


def fps_batch(xyz, offsets, num_samples, attr=None, mode=AUTO):
    """Per cloud the single call at start row 0, and the out offsets."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    out = [fps(xyz[a:b], num_samples, 0, None if attr is None else attr[a:b], mode) for a, b in zip(offsets[:-1], offsets[1:])]
    return out, np.concatenate([[0], np.cumsum([o["n_selected"] for o in out])]).astype(np.int32)
