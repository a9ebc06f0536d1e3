"""tests/fixed_tree_restatement.py against itself and against exact sums, on the CPU: the vectorised restatement of the header's fixed f64
tree (include/tdv_hip.h, tdv_remove_statistical_outlier rule 4) equals a lane-by-lane simulation of the shuffle, equals the exact sum
where the sum is exact, stays within the depth bound of math.fsum that the GPU tests also assert - and is NOT math.fsum: at least one
input gives other bits, so holding the device to the restatement byte for byte (tests/test_gpu_outlier.py, test_gpu_iss.py,
test_gpu_primitives_probe.py) asks more than the bound did."""
import math

import numpy as np
import pytest

import fixed_tree_restatement as T
import outlier_restatement as OR

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 65536, 65537, 131073]


def _terms(n, seed=0):
    return np.random.default_rng(1000 + n + seed).random(n) * 3.0 + 1e-3


@pytest.mark.parametrize("n", SIZES)
def test_vectorised_equals_lane_by_lane(n):
    x = _terms(n)
    slow, slow_part = T.tree_sum_by_lanes(x)
    part = T.block_sums(x)
    assert part.shape == (-(-n // 256),) and part.tobytes() == slow_part.tobytes()
    assert np.float64(T.tree_sum(x)).tobytes() == np.float64(slow).tobytes()
    assert np.float64(T.partials_sum(part)).tobytes() == np.float64(slow).tobytes()


def test_lane_zero_does_not_see_what_out_of_range_lanes_add():
    """In the simulation a lane whose partner lies beyond the wave adds its own value, as __shfl_down does; were the partner's value 0 or
    garbage instead, lane 0 would hold the same sum."""
    x = _terms(64, 5)

    def lane0(beyond):
        v = [np.float64(a) for a in x]
        for off in T.OFFSETS:
            old = list(v)
            v = [old[l] + (old[l + off] if l + off < 64 else beyond(old[l])) for l in range(64)]
        return v[0]
    want = T.wave_sum_by_lanes(x)
    assert lane0(lambda own: np.float64(0.0)).tobytes() == want.tobytes() == lane0(lambda own: np.float64(1e300)).tobytes()
    assert want.tobytes() == T.block_sums(x)[0].tobytes()                # three waves of +0.0 beside it change nothing


@pytest.mark.parametrize("n", SIZES)
def test_exact_on_small_integers(n):
    rng = np.random.default_rng(n)
    x = rng.integers(-1000, 1000, n).astype(np.float64)
    assert T.tree_sum(x) == float(int(x.sum()))
    flags = rng.integers(0, 2, n).astype(np.int32)
    assert T.tree_count(flags) == int(flags.sum()) and T.tree_count(flags).dtype == np.int32
    assert np.array_equal(T.block_counts(flags), np.add.reduceat(flags, np.arange(0, n, 256)) if n else np.zeros(0, np.int32))
    w = rng.integers(-50, 50, (n, 6)).astype(np.float64)
    assert T.tree_sum(w).shape == (6,) and np.array_equal(T.tree_sum(w), w.sum(0))
    for a in range(6):                                                     # the columns are independent sums
        assert T.tree_sum(w[:, a]).tobytes() == T.tree_sum(w)[a].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_within_the_depth_bound_of_fsum(n):
    """The bound of outlier_restatement.statistics_bounds for a sum of non-negative terms: relative error below (depth + 1) * 2^-53."""
    x = _terms(n, 7)
    exact = math.fsum(x)
    got = float(T.tree_sum(x))
    bound = (OR.tree_depth(n) + 1) * OR.U * exact
    print(n, "tree %.17g fsum %.17g bound %.3g" % (got, exact, bound))
    assert abs(got - exact) <= bound


def test_the_order_is_not_fsum_and_not_another_tree():
    """Over 200 inputs of 1,000 terms: the restated order gives other bits than the exact sum on some (so byte equality with the restatement
    asks more than the bound), and other bits than two nearby orders - (w0 + w2) + (w1 + w3) over the waves, and a serial sum - on some."""
    differ_fsum = differ_waves = differ_serial = 0
    for seed in range(200):
        x = _terms(1000, seed)
        t = np.float64(T.tree_sum(x))
        differ_fsum += t.tobytes() != np.float64(math.fsum(x)).tobytes()
        v = np.zeros(1024); v[:1000] = x
        swapped = []
        for b in range(4):
            w = [T.wave_sum_by_lanes(v[256 * b + 64 * k:256 * b + 64 * k + 64]) for k in range(4)]
            swapped.append((w[0] + w[2]) + (w[1] + w[3]))
        differ_waves += t.tobytes() != np.float64(T.partials_sum(np.array(swapped))).tobytes()
        differ_serial += t.tobytes() != np.add.accumulate(x)[-1].tobytes()
    print("of 200 inputs: %d differ from fsum, %d from the swapped wave order, %d from the serial sum" % (differ_fsum, differ_waves, differ_serial))
    assert differ_fsum >= 20 and differ_waves >= 20 and differ_serial >= 20


def test_zero_signs_and_non_finite_terms():
    """A thread starts at +0.0 and an absent thread holds +0.0: a full workgroup of -0.0 sums to -0.0, the final sum never does."""
    z = np.full(512, -0.0)
    assert np.signbit(T.block_sums(z)).all() and not np.signbit(T.tree_sum(z))
    assert np.signbit(T.block_sums(z[:300])).tolist() == [True, False]
    assert not np.signbit(T.tree_sum(np.zeros(0))) and T.tree_sum(np.zeros(0)) == 0.0
    x = _terms(700)
    x[5] = np.inf
    assert T.tree_sum(x) == np.inf
    x[600] = -np.inf
    assert np.isnan(T.tree_sum(x))
    x[:] = 1.0; x[3] = np.nan
    assert np.isnan(T.tree_sum(x)) and np.isnan(T.block_sums(x)[0]) and T.block_sums(x)[1] == 256.0


def test_block_max_is_fmax():
    x = _terms(600)
    x[7] = np.nan; x[300] = np.inf; x[512:] = np.nan
    got = T.block_max(x)
    assert got[0] == np.nanmax(x[:256]) and got[1] == np.inf and np.isnan(got[2]) and got.shape == (3,)
    assert T.block_max(np.array([-3.0, np.nan, -np.inf])).tolist() == [-3.0]
