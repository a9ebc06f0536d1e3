"""CPU suite: how job B of k_ransac_score_fast hands out its work (csrc/ransac_cut.hpp: score_unit, score_unit_block, through the
library's host exports).  The kernel's loop - a workgroup goes round the hypothesis blocks from its own start block and draws tickets
from the (XCD, block) word until the word has no unit left - is restated here over those two functions and run for every list
length, chunk range and grid: every (block, chunk) must be scored exactly once, nothing outside [r0, r1), whoever draws what."""
import ctypes as C
import functools

import numpy as np
import pytest

RS_BLOCK = 1024                    # hypotheses per block (csrc/ransac.hip)
N_LIST = [0, 1, 63, 64, 1023, 1024, 1025, 8191, 65536]
GRIDS = [8, 16, 504, 512, 6144]


@pytest.fixture(scope="module")
def cut(tdv):
    lib = tdv.lib()
    U = lib.tdv_ransac_score_unit_chunks()
    assert 1 <= U <= 1024

    @functools.lru_cache(maxsize=None)
    def unit(ticket, r0, r1, xcd):
        c0, c1 = C.c_int(-7), C.c_int(-7)
        ok = lib.tdv_ransac_score_unit(ticket, r0, r1, xcd, C.byref(c0), C.byref(c1))
        assert ok in (0, 1)
        return (c0.value, c1.value) if ok else None

    @functools.lru_cache(maxsize=None)
    def block(wg, visit, n_blk):
        return lib.tdv_ransac_score_unit_block(wg, visit, n_blk)

    return U, unit, block


def _ranges(U):
    # the issue's lengths; an XCD's share is an eighth of the range, so the same boundaries once more at eight times the length
    lengths = [0, 1, 7, 8, 9, U - 1, U, U + 1, 1000, 8 * U - 1, 8 * U, 8 * U + 1, 8 * U + 8]
    return [(r0, r0 + n) for n in sorted(set(lengths)) for r0 in (0, 14864)]


def _share_units(unit, r0, r1, xcd):
    """the units of an XCD's share, ticket by ticket, and that no later ticket - workgroups overdraw by one per visit - gives any"""
    units = []
    while unit(len(units), r0, r1, xcd) is not None:
        units.append(unit(len(units), r0, r1, xcd))
    for t in (len(units), len(units) + 1, len(units) + 6144 * 64, 2 ** 31 - 1, -1):
        assert unit(t, r0, r1, xcd) is None, (t, r0, r1, xcd)
    return units


def test_units_tile_the_range(cut):
    U, unit, _ = cut
    for r0, r1 in _ranges(U):
        cover = np.zeros(max(r1 - r0, 0), np.int32)
        for xcd in range(8):
            for c0, c1 in _share_units(unit, r0, r1, xcd):
                assert r0 <= c0 < c1 <= r1 and c1 - c0 <= U, (r0, r1, xcd, c0, c1)
                cover[c0 - r0:c1 - r0] += 1
        assert (cover == 1).all(), (r0, r1)


def test_every_workgroup_reaches_every_block(cut):
    _, _, block = cut
    for n_blk in sorted({(n + RS_BLOCK - 1) // RS_BLOCK for n in N_LIST} - {0}):
        for wg in range(max(GRIDS) // 8):
            assert sorted(block(wg, v, n_blk) for v in range(n_blk)) == list(range(n_blk)), (wg, n_blk)


@functools.lru_cache(maxsize=None)
def _drawn(block, n_blk, wgs, n_units):
    """One XCD: `wgs` workgroups run the kernel's loop, one ticket draw each in turn (the schedule that interleaves them most);
    returns, per block, the tickets that named a unit, in the order they were drawn."""
    word = [0] * n_blk
    taken = [[] for _ in range(n_blk)]
    visit = [0] * wgs
    live = list(range(wgs))
    while live:
        still = []
        for w in live:
            b = block(w, visit[w], n_blk)
            t = word[b]; word[b] += 1
            if t < n_units:
                taken[b].append(t)           # scores the unit, then draws from the same word again
            else:
                visit[w] += 1                # the block is drained: on to the next one
            if visit[w] < n_blk:
                still.append(w)
        live = still
    return taken


@pytest.mark.parametrize("grid", GRIDS)
def test_every_block_and_chunk_is_scored_once(cut, grid):
    U, unit, block = cut
    for r0, r1 in _ranges(U):
        shares = [_share_units(unit, r0, r1, xcd) for xcd in range(8)]
        for n_list in N_LIST:
            n_blk = (n_list + RS_BLOCK - 1) // RS_BLOCK
            cover = np.zeros((n_blk, max(r1 - r0, 0)), np.int32)
            for xcd in range(8):
                wgs = len(range(xcd, grid, 8))           # dispatch ids xcd, xcd + 8, ...
                assert wgs >= 1
                if n_blk == 0:
                    continue                             # the kernel returns before it draws
                for b, tickets in enumerate(_drawn(block, n_blk, wgs, len(shares[xcd]))):
                    for t in tickets:
                        c0, c1 = shares[xcd][t]
                        cover[b, c0 - r0:c1 - r0] += 1
            assert (cover == 1).all(), (grid, n_list, r0, r1)
