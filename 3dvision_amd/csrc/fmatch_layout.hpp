// The packed descriptor index as memory: what csrc/fmatch_index.hip writes (the packing is described there) and csrc/fmatch.hip
// reads.  Every layout is described here once.  A LEAF = FX_LEAF consecutive rows of one column of the packing, a GROUP = FX_GROUP
// consecutive leaves, a CHUNK = 64 consecutive groups.
//   T       [nleaf][FD][FX_LEAF]   row r = column r % FX_LEAF of leaf r / FX_LEAF (row_elem): one dimension of a whole leaf is one
//                                  coalesced 256-B load, lane = row.  Padding rows are +inf in every dimension: they never win.
//   torig   [rows]                 the row's index in the caller's table; INT_MAX = padding
//   lbox    [ngroup][min | max][FD][FX_GROUP]   33-D boxes of the leaves over their real rows, transposed per group: one dimension
//                                  of a group's 64 boxes is one coalesced load, lane = leaf.  A leaf of padding (and a leaf past
//                                  the end) has the empty box (+inf, -inf): its bound is +inf.
//   pbox    [ngroup][min | max][PD][FX_GROUP]   the leaves' boxes in the rows' principal coordinates (principal_coords)
//   gbox    [nchunk][min | max][FD][64]          the groups' 33-D boxes, the same layout one level up (lane = group)
//   gpbox   [nchunk][min | max][PD][64]          ... and their principal-coordinate boxes
//   sleaf   [nleaf][LM_BOX], sgroup [ngroup][LM_BOX]   the same boxes once more, one box = LM_BOX consecutive floats
//                                  min[FD] | max[FD] | pmin[PD] | pmax[PD]: what the leaf-major search stages in LDS
//   basis   [3][FD] directions | mean[FD]
//   b0      [S0 + 1]   p0 of the first row of every slab;   b1 [S0 * S1 + 1]   p1 of the first row of every column
//   col_leaf0 [S0 * S1 + 1]   first leaf of every column;   leaf_p2 [nleaf]   p2 of the first row of every leaf
//   amax    [1]        largest |x_d - mean_d| over the targets, as float bits (scales the rounding margin of the p-boxes)
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>

namespace tdv {

constexpr int FD = 33;            // descriptor dimensions
constexpr int PD = 3;             // principal coordinates
constexpr int FX_LEAF = 64;       // rows per leaf
constexpr int FX_GROUP = 64;      // leaves per group
constexpr int LM_BOX = 72;        // floats per box of sleaf / sgroup: min[33] | max[33] | pmin[3] | pmax[3]

#ifdef __HIPCC__
__device__ __forceinline__ size_t row_elem(size_t row, int d) { return (row / FX_LEAF) * (size_t)(FD * FX_LEAF) + (size_t)d * FX_LEAF + row % FX_LEAF; }

// Principal coordinates p_r(x) = sum_d (x_d - mean_d) * b_r[d], r = 0..2, as evaluated HERE (plain f32, d ascending):
// the one routine both sides use.  *amax receives (integer atomic max on the bits of a non-negative float) the largest
// |x_d - mean_d| seen, +inf for non-finite input: it scales the rounding margin of the principal-direction boxes.
// basis: [3][33] directions, then mean[33]
__device__ __forceinline__ void principal_coords(const float* __restrict__ x, const float* __restrict__ basis, float& a0, float& a1, float& a2, float& am) {
    a0 = 0.f; a1 = 0.f; a2 = 0.f; am = 0.f;
#pragma unroll
    for (int d = 0; d < FD; ++d) {
        const float v = x[d] - basis[3 * FD + d];
        a0 += v * basis[d]; a1 += v * basis[FD + d]; a2 += v * basis[2 * FD + d];
        const float av = fabsf(v);
        am = (av <= am) ? am : av;          // NaN: the comparison is false -> am = NaN, mapped to +inf below
    }
    if (!(am <= FLT_MAX)) am = INFINITY;
}
#endif

}  // namespace tdv
