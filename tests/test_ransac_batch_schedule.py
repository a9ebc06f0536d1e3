"""CPU suite: the batch schedule of a RANSAC call with bail-out (csrc/ransac_cut.hpp: ransac_batch_size, through the library's host
export tdv_ransac_batch_size).  The driver's rule - a batch that starts at iteration it0 holds min(size(it0), max_iterations - it0)
hypotheses - is restated here over the export and held to the sizes every call had before batches grew: 8,192, then 65,536 each,
for every max_iterations up to FIRST + 4 BATCH = 270,336, where growth may begin and not before."""
import functools

import pytest

FIRST, BATCH = 8192, 65536
GROW_AT = FIRST + 4 * BATCH          # 270,336
GROWN_SIZES = (131072, 262144)


@pytest.fixture(scope="module")
def size(tdv):
    lib = tdv.lib()

    @functools.lru_cache(maxsize=None)
    def f(it0):
        return int(lib.tdv_ransac_batch_size(it0))
    return f


def _batches(size, max_iterations):
    """the driver's loop: (it0, count) per batch"""
    out, it0 = [], 0
    while it0 < max_iterations:
        cnt = min(size(it0), max_iterations - it0)
        out.append((it0, cnt))
        assert cnt > 0, (max_iterations, it0)
        it0 += cnt
    return out


def _before(max_iterations):
    """the sizes of a call before batches grew"""
    out, it0 = [], 0
    while it0 < max_iterations:
        cnt = min(FIRST if it0 == 0 else BATCH, max_iterations - it0)
        out.append((it0, cnt))
        it0 += cnt
    return out


def test_the_sizes_of_every_call_that_does_not_reach_growth(size):
    for m in range(1, GROW_AT + 1):
        got = _batches(size, m)
        assert got == _before(m), m
        assert sum(c for _, c in got) == m


def test_growth_starts_at_270336_and_not_before(size):
    assert size(0) == FIRST
    for it0 in (1, FIRST, FIRST + BATCH, FIRST + 3 * BATCH, GROW_AT - 1):
        assert size(it0) == BATCH, it0
    grown = size(GROW_AT)
    assert grown in GROWN_SIZES
    for it0 in (GROW_AT, GROW_AT + 1, GROW_AT + grown, 2000000, 2**31 - 1):
        assert size(it0) >= BATCH and size(it0) in (BATCH,) + GROWN_SIZES, it0
    # a ramp may pass through 131,072 on its way to 262,144, never back down
    sizes = [size(it0) for it0, _ in _batches(size, GROW_AT + 8 * 262144)]
    assert sizes == sorted(sizes)


@pytest.mark.parametrize("extra", [1, 1025, 131072, 131073, 262144, 262145, 2 * 262144 + 1025, 2000000 - GROW_AT])
def test_a_grown_call_sums_to_its_iterations_and_ends_in_a_partial_batch(size, extra):
    m = GROW_AT + extra
    got = _batches(size, m)
    assert sum(c for _, c in got) == m
    assert all(c > 0 for _, c in got)
    assert got[:5] == _before(GROW_AT)                    # what came before growth is what it was
    assert all(c == size(it0) for it0, c in got[:-1])     # only the last batch may be partial: what is left of the call
    it0, last = got[-1]
    assert last == m - it0 and 0 < last <= size(it0)


def test_bad_argument(tdv):
    assert tdv.lib().tdv_ransac_batch_size(-1) < 0
