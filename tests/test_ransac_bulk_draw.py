"""RANSAC's index stream drawn in bulk (csrc/ctx.hip: whole 624-word twist blocks, Lemire's accept test per word, compaction
past the rejected words) equals std::mt19937 + std::uniform_int_distribution<size_t> (the oracle) triple for triple: long runs
that cross many twist blocks and the 1,024-triple chunks of tdv_sample_triples, ranges that reject often (just above 2^31 about
every second word) or never (powers of two), small clouds, n = 1, 2, 3, other seeds."""
import numpy as np
import pytest


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 640, 200000, 2 ** 20, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 12345, 3 * 2 ** 30 + 7,
                               2 ** 32 - 1, 2 ** 32])
def test_bulk_draw_equals_the_standard_library(tdv, orc, n):
    count = 70001 if n in (3, 200000, 2 ** 31 + 1) else 5003
    assert np.array_equal(tdv.sample_triples(n, count), orc.sample_triples(n, count)), n


@pytest.mark.parametrize("seed", [0, 1, 7, 4294967295])
def test_bulk_draw_other_seeds(tdv, orc, seed):
    for n in (3, 1000, 2 ** 31 + 3):
        assert np.array_equal(tdv.sample_triples(n, 2500, seed=seed), orc.sample_triples(n, 2500, seed=seed)), (seed, n)


def test_bulk_draw_prefixes_agree(tdv):
    """a shorter draw is a prefix of a longer one whatever block or chunk boundary it ends on"""
    full = tdv.sample_triples(2 ** 31 + 1, 3000)
    for count in (1, 207, 208, 209, 1023, 1024, 1025, 2999):
        assert np.array_equal(tdv.sample_triples(2 ** 31 + 1, count), full[:count]), count
