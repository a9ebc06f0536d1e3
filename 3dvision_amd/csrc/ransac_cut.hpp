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

}  // namespace tdv
