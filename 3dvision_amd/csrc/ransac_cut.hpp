// How k_ransac_score_fast's dispatches (ransac.hip) cut the points: the rules host and device - and tests/test_ransac_unit_cut.py,
// through hostops.hip - share.  Plain integer functions; no device state.
#pragma once
#include <hip/hip_runtime.h>

#ifndef RS_WG_TARGET
#define RS_WG_TARGET 6144
#endif
#ifndef RS_UNIT
#define RS_UNIT 16           // chunks per unit of job B (measured 8, 16, 32: profiles/r10/ransac_live_scheduling.md)
#endif

namespace tdv {

// The point-range cut: into how many ranges a job-A scoring dispatch with hb hypothesis blocks cuts the points, so that it has about
// RS_WG_TARGET workgroups, of at least 32 chunks each (at least 1: the first term is, whatever hb).
__host__ __device__ __forceinline__ int point_ranges(int hb, int n_pchunks) { return min(min((RS_WG_TARGET + hb - 1) / hb, max(1, n_pchunks / 32)), 512); }

// Job B's cut (round 10).  Its chunks [r0, r1) go to the eight XCDs in eight contiguous shares (an L2 keeps holding an eighth of the
// pairs); an XCD's share of ONE hypothesis block is handed out in units of RS_UNIT chunks by a ticket word per (XCD, block): ticket
// t is the t-th unit of the share.  false: no such unit (the share is drained, or empty - fewer chunks than XCDs).  Every
// (block, chunk) belongs to exactly one (xcd, ticket), whatever the grid: who draws which ticket does not matter.
__host__ __device__ __forceinline__ bool score_unit(int ticket, int r0, int r1, int xcd, int& c0, int& c1) {
    const int n = r1 > r0 ? r1 - r0 : 0, share = (n + 7) / 8;
    const int x0 = min(n, xcd * share), x1 = min(n, x0 + share);
    if (ticket < 0 || ticket > share / RS_UNIT) return false;          // (also keeps ticket * RS_UNIT inside an int)
    c0 = r0 + x0 + ticket * RS_UNIT; c1 = min(r0 + x1, c0 + RS_UNIT);
    return c0 < c1;
}
// The order in which workgroup wg of an XCD (its dispatch id / 8) visits the n_blk hypothesis blocks: it starts at block wg mod n_blk,
// so the workgroups spread evenly over the blocks, and goes round once - any single workgroup reaches every block.
__host__ __device__ __forceinline__ int score_unit_block(int wg, int visit, int n_blk) { return (int)(((unsigned)wg + (unsigned)visit) % (unsigned)n_blk); }

// The batch schedule of a call with bail-out (ransac.hip: RansacRun), stated once: the size of the batch that starts at iteration it0
// (the call's last batch is what is left of max_iterations).  A short first batch sets a best count for the bound; batches of
// kRansacBatch keep the early exit's granularity while the call is young; from kRansacGrowAt on a batch holds `grown` hypotheses,
// because a batch's one-workgroup kernels, its hypothesis kernel and the fine level's partly filled round cost per batch, not per
// hypothesis (profiles/r27/ransac_batch_growth.md).  grown == kRansacBatch: no growth.
constexpr int kRansacFirst = 8192, kRansacBatch = 65536, kRansacGrown = 131072;
constexpr int kRansacGrowAt = kRansacFirst + 4 * kRansacBatch;     // 270,336: beyond every shape the per-batch tests are written around
__host__ __device__ __forceinline__ int ransac_batch_size(int it0, int grown = kRansacGrown) {
    return it0 == 0 ? kRansacFirst : it0 < kRansacGrowAt ? kRansacBatch : grown;
}

// The leaf order of a call whose context leaves it to the library (TDV_RANSAC_LEAVES_AUTO): class-major leaves from this many pairs
// on, Morton leaves below.  Measured (profiles/r29/ransac_leaf_classes.md): the smallest size of the table from which the class-major
// order never lies under the Morton order's range.  It cannot go below 30,001: the suite holds the product library's Morton lists at
// 9,999 and 30,000 pairs against the study library's class-major ones (tests/test_gpu_ransac_far_bound.py:
// test_best_found_in_the_bounded_batch, tests/test_gpu_ransac_bound_lists.py: test_main_shorter_fine_list_same_result), and on a
// 9,999-pair cloud the scored share counts whole blocks of 1,024 hypotheses, which a strict inequality there rests on.
constexpr int kRansacLeafClassesMin = 50000;
static_assert(kRansacLeafClassesMin > 30000, "the suite compares Morton lists at 30,000 pairs");

// The fine level's cut (k_ransac_bound_fine, round 29).  The undecided list has nb slot blocks of 64 hypotheses, the fine leaves
// n_lpairs pairs, the grid `grid` workgroups of RB_SPLIT waves, as many as the chip holds at once.  A unit is (slot block, one of R
// ranges of the leaf pairs); workgroup w takes the units w, w + grid, ...  Every workgroup derives R alike from the list's length:
// the R that makes the longest workgroup's path shortest, counted in leaf pairs a wave walks - rounds of units, each a wave's share
// of a range plus kFineUnitCost for the unit's fixed part (the pose's loads, two barriers, the ticket).  Few slot blocks get many
// ranges, many get one and several units per workgroup.  A wave's share stays at kFineMinWalk pairs or more while R > 1.  Only
// speed depends on R: the verdict of a slot block is its last arrival's, whatever the cut.
constexpr int kFineUnitCost = 6, kFineMinWalk = 8, kFineMaxRanges = 64;
// The cost of a cut into r ranges with r in its low 7 bits: the smallest key is the cut, the fewer ranges on equal cost.  All ones:
// no such cut.  (A key per candidate, so that the device asks its 64 lanes at once: a scalar loop over the candidates, three integer
// divisions each, cost the kernel 19 us per launch - profiles/r29/ransac_leaf_classes.md.)
__host__ __device__ __forceinline__ unsigned long long fine_cut_key(int r, int nb, int n_lpairs, int grid, int waves) {
    if (r < 1 || r > kFineMaxRanges) return ~0ull;
    const int walk = ((n_lpairs + r - 1) / r + waves - 1) / waves;
    if (r > 1 && walk < kFineMinWalk) return ~0ull;
    const unsigned units = (unsigned)nb * (unsigned)r, rounds = (units + (unsigned)grid - 1u) / (unsigned)grid;      // (nb <= 2^25: a list of 2^31 slots)
    return ((unsigned long long)rounds * (unsigned)(walk + kFineUnitCost)) << 7 | (unsigned)r;
}
__host__ __device__ __forceinline__ int fine_ranges(int nb, int n_lpairs, int grid, int waves) {
    if (nb <= 0 || grid <= 0) return 1;
    unsigned long long best = ~0ull;
    for (int r = 1; r <= kFineMaxRanges; ++r) { const unsigned long long k = fine_cut_key(r, nb, n_lpairs, grid, waves); best = k < best ? k : best; }
    return (int)(best & 127ull);
}

}  // namespace tdv
