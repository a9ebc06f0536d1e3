"""The fixed f64 summation tree of include/tdv_hip.h (tdv_remove_statistical_outlier, rule 4; cited by ISS rule 8) restated in numpy
float64 from the header's text, addition by addition.  It shares nothing with the device code (csrc/fixed_tree.hpp).

  - the term of point i belongs to workgroup i // 256, thread i % 256; a thread without a point holds +0.0;
  - a workgroup sum is, per wave of 64, v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1 (lane 0 holds the wave's sum), then
    (w0 + w1) + (w2 + w3) over the four waves;
  - one workgroup then adds the workgroup sums t, t + 256, t + 512, ... in that order into thread t, starting from +0.0, and sums its 256
    threads the same way.

Only lane 0 of a wave matters, and lane 0 after the step `off` depends on the lanes below 2 * off alone: the vectorised form keeps the
lower half of the live lanes at every step.  tests/test_fixed_tree_restatement.py holds it to a lane-by-lane simulation of the shuffle.

Terms may be [n] or [n, width] (width independent sums, as the plane fit's 4 and 6); numpy neither contracts nor reorders the additions.
"""
import numpy as np

WG = 256
WAVE = 64
OFFSETS = (32, 16, 8, 4, 2, 1)


def _workgroup_tree(v):
    """v[..., 256, width] -> [..., width]: the shuffle tree per wave, then (w0 + w1) + (w2 + w3)."""
    w = v.reshape(v.shape[:-2] + (WG // WAVE, WAVE, v.shape[-1]))
    for off in OFFSETS:
        w = w[..., :off, :] + w[..., off:2 * off, :]
    w = w[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def _as_columns(terms, dtype):
    t = np.asarray(terms, dtype)
    flat = t.ndim <= 1
    return (t.reshape(-1, 1) if flat else t.reshape(len(t), int(np.prod(t.shape[1:])))), flat


def _block_reduce(terms, dtype):
    t, flat = _as_columns(terms, dtype)
    n, width = t.shape
    nb = -(-n // WG)
    v = np.zeros((nb * WG, width), dtype)                    # +0.0 (0) in the threads without a point
    v[:n] = t
    with np.errstate(invalid="ignore", over="ignore"):
        out = _workgroup_tree(v.reshape(nb, WG, width))
    return out[:, 0] if flat else out


def _partials_reduce(part, dtype):
    p, flat = _as_columns(part, dtype)
    nb, width = p.shape
    v = np.zeros((WG, width), dtype)                         # thread t starts at +0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for b0 in range(0, nb, WG):                          # ... and adds part[t], part[t + 256], ... in that order
            rows = p[b0:b0 + WG]
            v[:len(rows)] = v[:len(rows)] + rows
        out = _workgroup_tree(v)
    return out[0] if flat else out


def block_sums(terms):
    """float64 [ceil(n / 256)] (or [.., width]): every workgroup's sum."""
    return _block_reduce(terms, np.float64)


def partials_sum(part):
    """One workgroup's sum of the workgroup sums `part`: a float64 (or [width])."""
    return _partials_reduce(part, np.float64)


def tree_sum(terms):
    return partials_sum(block_sums(terms))


def block_counts(flags):
    """The same tree over int32 counts (integer sums are associative: stated for completeness)."""
    return _block_reduce(flags, np.int32)


def partials_count(cnt):
    return _partials_reduce(cnt, np.int32)


def tree_count(flags):
    return partials_count(block_counts(flags))


def block_max(values):
    """float64 [ceil(n / 256)]: the largest value of every workgroup with fmax semantics - a NaN never wins, so a workgroup's result is
    NaN only where all of its values are.  (A thread without a point holds NaN.)  Order-free."""
    t = np.asarray(values, np.float64).reshape(-1)
    nb = -(-len(t) // WG)
    v = np.full(nb * WG, np.nan)
    v[:len(t)] = t
    return np.fmax.reduce(v.reshape(nb, WG), axis=1) if nb else np.zeros(0)


# ------------------------------------------------------------------------------------------------ the slow form, for the test of this file
def wave_sum_by_lanes(v64):
    """Lane 0 after the six shuffle steps, every lane simulated: lane l adds the value lane l + off held BEFORE the step, and a lane whose
    partner lies beyond the wave adds its own value (what __shfl_down returns there)."""
    v = [np.float64(x) for x in v64]
    assert len(v) == WAVE
    with np.errstate(invalid="ignore", over="ignore"):
        for off in OFFSETS:
            old = list(v)
            v = [old[l] + (old[l + off] if l + off < WAVE else old[l]) for l in range(WAVE)]
    return v[0]


def workgroup_sum_by_lanes(v256):
    w = [wave_sum_by_lanes(v256[WAVE * k:WAVE * k + WAVE]) for k in range(WG // WAVE)]
    with np.errstate(invalid="ignore", over="ignore"):
        return (w[0] + w[1]) + (w[2] + w[3])


def tree_sum_by_lanes(terms):
    t = [np.float64(x) for x in np.asarray(terms, np.float64).reshape(-1)]
    nb = -(-len(t) // WG)
    t += [np.float64(0.0)] * (nb * WG - len(t))
    part = [workgroup_sum_by_lanes(t[WG * b:WG * b + WG]) for b in range(nb)]
    v = [np.float64(0.0)] * WG
    with np.errstate(invalid="ignore", over="ignore"):
        for b, p in enumerate(part):                         # ascending b: thread b % 256 takes them in order
            v[b % WG] = v[b % WG] + p
    return workgroup_sum_by_lanes(v), np.array(part, np.float64)
