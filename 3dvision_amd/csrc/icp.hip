// ICP on gfx950: brute-force nearest-neighbour correspondence search + normal equations +
// small solve, the whole loop resident on the device.
//
// Replaces GPURegistration::icpRefine (/root/reference/src/gpu_impl.cpp:141-260, kernels
// cuda/icp.cu:14-55 and :90-142); results follow the CPU oracle Registration::icpRefine
// (/root/reference/src/registration.cpp:297-414), including where the CUDA path differs
// (transformed point in J and r, inclusive threshold, n_corr<3 break, point-to-point mode).
//
// Kernel design (VALU-bound, not HBM- and not MFMA-bound: 8 f32 ops per pair, K=3):
//  * icp_nn_scan: each lane keeps NN_SPL transformed source points in VGPRs; the target cloud
//    is read as structure-of-arrays through the SCALAR data path (wave-uniform s_load_dwordx16
//    of 16 x, 16 y, 16 z), so every distance op is one VALU instruction with an SGPR operand and
//    neither LDS nor vector-memory instructions sit in the inner loop.  Argmin is two-level:
//    the loop tracks min d2 and the first CHUNK of 16 targets that reached it (strict <),
//    8 + 0.5 + 0.3 VALU ops per pair; the exact index inside the chunk is recovered later by
//    re-evaluating 16 distances.  d2 = dx*dx + (dy*dy + dz*dz) with no FMA contraction, so the
//    argmin is bit-identical to the CPU scan (lowest index wins ties).
//    The grid is (source blocks) x (target splits) so that >> 256 workgroups are in flight;
//    splits are combined in split order with strict <, which preserves the tie rule.
//  * icp_accumulate: one lane per source; resolves the index, applies the sqrt-free inclusive
//    threshold, builds J = [p x n | n], r = (p-q).n (or the point-to-point moments) and reduces
//    in a FIXED order (wave64 shuffles -> LDS -> one slab per block); f64 accumulators.
//    The block that finishes last (atomic ticket) folds the slabs in fixed order, one lane solves the 6x6 system
//    (pivoted LDL^T) or the 3x3 Kabsch SVD, updates T on the device and evaluates convergence: two launches per
//    iteration.
//  * icp_iterate (hash grid, tree sums, point-to-plane or point-to-point, 150,000 to 262,144 sources): search and sums in ONE launch
//    per iteration - the search keeps its shape, one lane per source point; the lanes hand float records over in LDS and the sixteen
//    waves of the workgroup form the slab from them in icp_accumulate's f64 tree, bit for bit.
//  * icp_nn_pruned (large clouds, same correspondences bit for bit): the target is put in Morton order once per
//    call; ONE WAVE PER SOURCE POINT tests the target's 4096- and 64-point bounding boxes one per lane, visits them
//    best-first, and evaluates the points of the boxes that can hold a neighbour within the bound one per lane
//    (bound = the inclusive acceptance threshold, then the best distance found).  Float subtraction, multiplication
//    and addition are monotone under round-to-nearest, so the box bound needs no margin; ties keep the lowest
//    original target index as the scan does.  accumulate/solve run unchanged.
//  * many instances against one target (icp_batch_run_dev: tdv_icp_batch_dev, tdv_refine_batch_dev): one hash grid over the target
//    for the call, then k_icp_nn_grid_multi + k_icp_accumulate_multi - two launches per iteration for the whole batch, blocks padded
//    per instance, each instance with the slab layout its single call would use, so that its bits are the single call's.
//  * robust losses (tdv_ctx_set_icp_loss): every accepted correspondence's terms are scaled by its weight in acc_terms, the one place
//    all tree-sum paths form them; the kernels take ROBUST as a template parameter, so the L2 instantiations are the code without it.
//  * generalized ICP (tdv_gicp, MODE 3): plane-to-plane terms from both clouds' normals in acc_terms, the same 6x6 system, slab layout
//    and solve as point-to-plane.  Its extra kernel arguments (the source normals, c = 1 - epsilon) are IcpArgs<3>, the kernels' last
//    parameter: a struct typed by MODE that is empty for modes 0-2, so that their kernels keep their arguments and their code.
//  * colored ICP (tdv_colored_icp, MODE 4): point-to-plane's row plus a photometric row on the target's tangent plane in acc_terms, the
//    same 6x6 system and slab layout.  Its extra arguments (source colours, the target's colour table, lg, lc) are IcpArgs<4>.
//    Per correspondence, corr_pt turns IcpArgs<MODE> into the CorrPt<MODE> that acc_terms takes; on the host, icp_dispatch picks the
//    instantiation from the call's IcpObjective.
// No float atomics anywhere: two runs give identical bits.
#include "tdv_internal.hpp"
#include "device_linalg.hpp"
#include "icp_terms.hpp"
#include "sorted_cloud.hpp"
#include "lds_scan.hpp"
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <algorithm>

namespace tdv {

constexpr int NN_SPL = 2;      // source points per lane
constexpr int NN_CH = 16;      // targets per chunk (one s_load_dwordx16 per coordinate)
#ifndef NN_BLOCK_VALUE
#define NN_BLOCK_VALUE 128
#endif
#ifndef NN_WG_TARGET
#define NN_WG_TARGET 12288
#endif
constexpr int NN_BLOCK = NN_BLOCK_VALUE;    // two waves per workgroup (no LDS, no barrier): many workgroups with few target splits,
                                 // so the per-split partials (8 B per source per split) stay small
constexpr int NN_SRC_PER_BLOCK = NN_SPL * NN_BLOCK;
constexpr double PRUNED_MIN_PAIRS = 1e8;   // auto mode: pruned search from this many source x target pairs ...
constexpr int PRUNED_MIN_TARGETS = 4096;    // ... and targets (measured: 50k x 10k 0.042 vs 0.081 ms, 128k x 9.4k see DESIGN)
constexpr int ACC_NV = 32;     // reduction slots per block (29 used p2plane, 17 p2point; with a robust loss 30 and 19)

// IcpLoss and loss_weight, IcpState, ICP_RUN_*, icp_update, CorrTgt, corr_jr, corr_rec and rec_terms: icp_terms.hpp, shared with the
// depth odometry (odometry.hip)

__global__ void k_aos_to_soa_pad(const float* __restrict__ aos, int n, int n_pad, float pad,
                                 float* __restrict__ x, float* __restrict__ y, float* __restrict__ z) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    if (i < n) { x[i] = aos[3 * i]; y[i] = aos[3 * i + 1]; z[i] = aos[3 * i + 2]; }
    else { x[i] = pad; y[i] = pad; z[i] = pad; }
}

__global__ __launch_bounds__(NN_BLOCK)
void k_icp_nn_scan(const float* __restrict__ src, int ns, int ns_pad,
                   const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
                   int n_chunks, int chunks_per_split,
                   const IcpState* __restrict__ st,
                   float* __restrict__ pd2, int* __restrict__ pchunk) {
    if (st->done) return;
    // XCD-aware deal (round 4, as k_ransac_score_fast): workgroups are dispatched x-fastest and an XCD takes every eighth of them, so with
    // the plain mapping every XCD's L2 pulled ALL target splits (PMC round 3: 49.7 MB per launch for 7.2 MB).  When the split count is a
    // multiple of 8 an XCD takes every eighth SPLIT and all source blocks of it: its L2 holds an eighth of the targets.
    int bxi = blockIdx.x, split = blockIdx.y;
    if ((gridDim.y & 7) == 0) {
        const int lin = blockIdx.y * gridDim.x + blockIdx.x, k = lin >> 3;
        bxi = k % gridDim.x; split = (k / gridDim.x) * 8 + (lin & 7);
    }
    const int c0 = split * chunks_per_split;
    const int c1 = min(n_chunks, c0 + chunks_per_split);
    const int base = bxi * NN_SRC_PER_BLOCK + threadIdx.x;
    float px[NN_SPL], py[NN_SPL], pz[NN_SPL], best[NN_SPL];
    int bc[NN_SPL];
#pragma unroll
    for (int s = 0; s < NN_SPL; ++s) {
        int i = min(base + s * NN_BLOCK, ns - 1);
        transform_point(st->T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px[s], py[s], pz[s]);
        best[s] = FLT_MAX; bc[s] = 0;
    }
    for (int c = c0; c < c1; ++c) {
        const int j = c * NN_CH;
        float qx[NN_CH], qy[NN_CH], qz[NN_CH];
#pragma unroll
        for (int t = 0; t < NN_CH; ++t) { qx[t] = tx[j + t]; qy[t] = ty[j + t]; qz[t] = tz[j + t]; }
#pragma unroll
        for (int s = 0; s < NN_SPL; ++s) {
            float m = FLT_MAX;
#pragma unroll
            for (int t = 0; t < NN_CH; ++t) {
                float dx = px[s] - qx[t], dy = py[s] - qy[t], dz = pz[s] - qz[t];
                float d2 = dx * dx + (dy * dy + dz * dz);
                m = fminf(m, d2);
            }
            bool lt = m < best[s];
            best[s] = lt ? m : best[s];
            bc[s] = lt ? j : bc[s];
        }
    }
#pragma unroll
    for (int s = 0; s < NN_SPL; ++s) {
        size_t o = (size_t)split * ns_pad + base + s * NN_BLOCK;
        pd2[o] = best[s]; pchunk[o] = bc[s];
    }
}

// ---- exact pruned search --------------------------------------------------------------------------------------
#ifndef PN_WAVES_VALUE
#define PN_WAVES_VALUE 1
#endif
constexpr int PN_WAVES = PN_WAVES_VALUE;   // waves per workgroup (measured at 200k: 1 wave 0.169 ms, 4: 0.177, 16: 0.217)
#ifndef PN_PTS_VALUE
#define PN_PTS_VALUE 1
#endif
// Consecutive source points per wave; their results leave as ONE store per array.  With 1 every result is its own 4-B
// partial-line write (13 MB of WRITE_SIZE per launch for 1.6 MB of results at 200k), which costs bytes but no time: the
// kernel is bound by its box walk, and longer waves balance worse — measured at 200k x 200k (tools/studies/icp_probe.py,
// profiles/r2/history/icp_nn_points_per_wave.jsonl): 1: 0.131 ms, 4: 0.141, 8: 0.144, 16: 0.155, 32: 0.166 ms per launch.
constexpr int PN_PTS = PN_PTS_VALUE;

// One wave per source point at a time, PN_PTS consecutive points per wave (lane p keeps point p's result and the wave
// stores them together).  The 4096-point boxes are tested one per lane and visited best-first (smallest lower
// bound first, until it exceeds the bound); inside one, its 64 leaves (64 points each) are tested one per lane, and
// the points of a leaf that passes are evaluated one per lane (coalesced).  bound = the inclusive acceptance
// threshold, then the best distance found so far.  Each lane keeps its own (d2, original index) minimum; the wave
// minimum in that lexicographic order is the brute-force scan's answer (lowest index on ties).
__global__ __launch_bounds__(64 * PN_WAVES)
void k_icp_nn_pruned(const float* __restrict__ src, int ns, SortedCloud c /* the target */, const IcpState* __restrict__ st, float tau,
                     float* __restrict__ out_d2, int* __restrict__ out_idx) {
    if (st->done) return;
    const int lane = threadIdx.x & 63;
    const int i0 = (blockIdx.x * PN_WAVES + (threadIdx.x >> 6)) * PN_PTS;
    if (i0 >= ns) return;   // wave-uniform
    float res_d = FLT_MAX; int res_o = 0;   // lane p: the result of point i0 + p
    for (int p = 0; p < PN_PTS && i0 + p < ns; ++p) {
    const int i = i0 + p;
    float px, py, pz;
    transform_point(st->T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
    float B = tau;           // wave-uniform; a target passes iff d2 <= B
    float bd = INFINITY;     // this lane's best
    int bo = INT_MAX;
    for (int tb = 0; tb < c.n_top; tb += 64) {
        const int t = tb + lane;
        float lbt = t < c.n_top ? d2_box_bound<D2::REF>(c.tbox, c.n_top, t, px, py, pz) : INFINITY;
        while (true) {
            // best-first over the remaining 4096-point boxes of this group
            float m = lbt;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
            if (!(m <= B) || m == INFINITY) break;   // +inf marks visited / absent boxes whatever the bound is
            const int tl = __ffsll((long long)__ballot(lbt == m)) - 1;   // wave-uniform lane of that box
            if (lane == tl) lbt = INFINITY;                               // visited
            const int u = (tb + tl) * 64 + lane;
            const float lbl = u < c.n_leaf ? d2_box_bound<D2::REF>(c.lbox, c.n_leaf, u, px, py, pz) : INFINITY;
            unsigned long long lmask = __ballot(u < c.n_leaf && lbl <= B);
            while (lmask) {
                const int bl = __ffsll((long long)lmask) - 1;
                lmask &= lmask - 1;
                if (__shfl(lbl, bl, 64) > B) continue;   // the bound may have dropped since the test
                const int j = ((tb + tl) * 64 + bl) * 64 + lane;   // arrays are padded with +inf to a multiple of 256
                float dx = px - c.sx[j], dy = py - c.sy[j], dz = pz - c.sz[j];
                float d2 = dx * dx + (dy * dy + dz * dz);
                const bool cand = j < c.n && d2 <= B && d2 <= bd;
                if (__any(cand)) {
                    const int o = c.orig[j];
                    const bool take = cand && (d2 < bd || o < bo);
                    bd = take ? d2 : bd;
                    bo = take ? o : bo;
                    float nb = bd;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) nb = fminf(nb, __shfl_xor(nb, off, 64));
                    B = fminf(B, nb);
                }
            }
        }
    }
    // lexicographic (d2, index) minimum over the lanes
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(bd, off, 64); const int oo = __shfl_xor(bo, off, 64);
        const bool take = od < bd || (od == bd && oo < bo);
        bd = take ? od : bd; bo = take ? oo : bo;
    }
    if (lane == p) { res_d = bo == INT_MAX ? FLT_MAX : bd; res_o = bo == INT_MAX ? 0 : bo; }
    }
    if (lane < PN_PTS && i0 + lane < ns) { out_d2[i0 + lane] = res_d; out_idx[i0 + lane] = res_o; }
}

// ---- hash-grid search ------------------------------------------------------------------------------------------------
// ICP accepts a correspondence only within `thr`, and the reference's pipeline sets thr = 0.4 x the voxel size: far below
// the point spacing.  One LANE per source point looks its neighbourhood up in a hash grid over the target and verifies
// what it finds with the scan's distance expression, instead of one WAVE per source point walking box levels.
// Cells are 2.2 thr wide, so per axis a neighbour within thr lies in the query's cell or in ONE adjacent cell, the one on
// the side of the cell the query sits in: 8 probes of an open-addressing table (8-B entries: 32-bit tag of the cell key, list head), all loaded
// before the first is looked at.  The points of a cell form a linked list of original indices (order irrelevant: the
// lowest (d2, index) is kept).  Every candidate is verified (d2 <= tau), so a tag collision or the garbage cell of a
// far-away query can only cost time.  Completeness: in cell units a pair within thr is at most r = 1/2.2 (1 + 1e-6) apart
// per axis; a computed coordinate fl(x * inv_cell) is within e = 2^-23 |coordinate| (two roundings) of the real one, i.e.
// e <= 2^-6 while |coordinate| < 2^17 - which k_grid_insert checks on every target (a query within thr of a target is in
// range with it).  A query with computed fraction f < 0.5 in cell k sees a neighbour's computed coordinate inside
// [k - r - 2e, k + 0.5 + r + 2e) and r + 2e < 0.486: cells k - 1 and k; symmetrically k and k + 1 for f >= 0.5.
constexpr unsigned GRID_EMPTY = ~0u;
#ifndef GRID_SLOTS_PER_POINT_X4
#define GRID_SLOTS_PER_POINT_X4 8      // table slots per target point, in quarters (8 = the power of two >= 2 n)
#endif
constexpr float GRID_CELL_FACTOR = 2.2f;
constexpr float GRID_MAX_COORD = 131072.0f;      // 2^17 cells
constexpr int GRID_PAD = 16;                    // slots past the table's end: probing never wraps (an insertion that would run past them makes the grid unusable)
constexpr int GRID_MAX_PER_CELL = 32;            // average over the occupied cells above which the grid is not used (measured at 200k x 200k, threshold in spacings: 2 -> 19 per cell, grid 0.13 ms vs walk 0.20; 4 -> 77 per cell, 0.37 vs 0.21)
struct __attribute__((aligned(8))) GridEntry { unsigned tag; int head; };   // tag: 32 bits of the cell key's hash (two cells that share a tag and a probe chain share a list: every candidate is verified anyway)
__device__ __forceinline__ unsigned long long grid_key(int ix, int iy, int iz) {
    return ((unsigned long long)((unsigned)ix & 0x1fffffu) << 42) | ((unsigned long long)((unsigned)iy & 0x1fffffu) << 21) | (unsigned long long)((unsigned)iz & 0x1fffffu);
}
__device__ __forceinline__ unsigned grid_slot(unsigned long long key, int shift) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift); }
__device__ __forceinline__ unsigned grid_tag(unsigned long long key) {
    const unsigned t = (unsigned)((key * 0xD6E8FEB86659FD93ull) >> 32);
    return t == GRID_EMPTY ? GRID_EMPTY - 1u : t;
}

// flags[0]: a coordinate out of range / non-finite; flags[1]: occupied cells
__global__ __launch_bounds__(256)
void k_grid_insert(const float* __restrict__ tgt, int nt, float inv_cell, GridEntry* table, float4* __restrict__ node,
                   unsigned mask, int shift, int* __restrict__ flags) {
    __shared__ int s_new, s_bad;
    if (threadIdx.x == 0) { s_new = 0; s_bad = 0; }
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    bool fresh = false, bad = false;
    if (j < nt) {
        const float x = tgt[3 * j], y = tgt[3 * j + 1], z = tgt[3 * j + 2];
        const float fx = x * inv_cell, fy = y * inv_cell, fz = z * inv_cell;
        bad = !(fabsf(fx) < GRID_MAX_COORD && fabsf(fy) < GRID_MAX_COORD && fabsf(fz) < GRID_MAX_COORD);
        if (!bad) {
            const unsigned long long key = grid_key((int)floorf(fx), (int)floorf(fy), (int)floorf(fz));
            const unsigned tag = grid_tag(key);
            unsigned slot = grid_slot(key, shift);
            const unsigned last = mask + (unsigned)GRID_PAD - 2u;    // the two slots after it stay empty: a two-entry probe at `last` reads inside the table and ends there
            for (;;) {
                unsigned k = table[slot].tag;
                if (k == GRID_EMPTY) { k = atomicCAS(&table[slot].tag, GRID_EMPTY, tag); if (k == GRID_EMPTY) { fresh = true; break; } }
                if (k == tag) break;
                if (++slot > last) { bad = true; break; }            // no wrap-around (half full at most: a run this long at the very end is a freak; the caller falls back to the box walk)
            }
            if (!bad) node[j] = make_float4(x, y, z, __int_as_float(atomicExch(&table[slot].head, j)));   // the point and the next index of its cell's list
        }
    }
    const unsigned long long mf = __ballot(fresh), mb = __ballot(bad);
    if ((threadIdx.x & 63) == 0) { if (mf) atomicAdd(&s_new, __popcll(mf)); if (mb) atomicAdd(&s_bad, 1); }
    __syncthreads();
    if (threadIdx.x == 0) { if (s_new) atomicAdd(&flags[1], s_new); if (s_bad) atomicOr(&flags[0], 1); }
}

// ---- the probe cache: a source point's eight list heads, kept between the iterations of one call ---------------------------------
// What the probes of grid_nearest find - j[0..7], each cell's list head or -1 - is a function of the point's cell (cx, cy, cz), its
// three neighbour signs and the table, and the table does not change during a call.  After a call's first iterations the pose moves by
// far less than half a cell, so nearly every point asks the same eight questions again.  Per source point the call's workspace keeps
// the six integers packed into 8 bytes (18 bits per cell coordinate: |coordinate| < GRID_MAX_COORD = 2^17; three sign bits; a valid
// bit) and the eight heads, struct of arrays: a wave's loads are whole lines.  The key array is zeroed (invalid) once per call
// (icp_run_dev), so no head outlives its table.  A lane takes the cached heads only if the key it computes THIS iteration from this
// iteration's pose equals the stored one: the heads are then the ones the probes would find, exactly.  A lane whose transformed point
// is non-finite or outside GRID_MAX_COORD never hits and never stores.
struct ProbeCache { uint2* key; uint4* head; int* misses; };      // key[ns]; head[2 ns]: heads 0-3 at [i], 4-7 at [ns + i]; misses: one word
struct ProbeLane { uint2 key; uint4 h0, h1; };                     // what a lane loaded, early (beside its source point)
constexpr unsigned PROBE_VALID = 0x80000000u;
// PROBE: 0 no cache; 1 the cache; study build only - 2 the cached heads taken as they are, no compare and no probe loop (an upper bound
// on the gain: the heads come from the call's first iteration, which runs 1); 3 the probe loop alone, no list walk (nothing is found)
__device__ __forceinline__ ProbeLane probe_load(const ProbeCache& pc, int i, int ns) {
    ProbeLane l;
    l.key = pc.key[i]; l.h0 = pc.head[i]; l.h1 = pc.head[(size_t)ns + i];
    return l;
}

// the search of one query point p: lowest (d2, original index) among the targets with d2 <= tau, (INFINITY, INT_MAX) if none.
// PROBE != 0: point i's cached heads lc (probe_load) are taken where their key holds, the heads found otherwise are stored, and
// `missed` tells whether this lane probed.
template <int PROBE = 0>
__device__ __forceinline__ void grid_nearest(const GridEntry* __restrict__ table, const float4* __restrict__ node, unsigned mask, int shift,
                                             float inv_cell, float px, float py, float pz, float tau, float& bd, int& bo,
                                             float* bq = nullptr /* 3: the winner's coordinates as node[] holds them, k_grid_insert's copy of the target's */,
                                             const ProbeCache* pc = nullptr, const ProbeLane* lc = nullptr, int i = 0, int ns = 0, bool* missed = nullptr) {
    const float gx = px * inv_cell, gy = py * inv_cell, gz = pz * inv_cell;
    const float kx = floorf(gx), ky = floorf(gy), kz = floorf(gz);
    const int cx = (int)kx, cy = (int)ky, cz = (int)kz;
    const int sx = (gx - kx < 0.5f) ? -1 : 1, sy = (gy - ky < 0.5f) ? -1 : 1, sz = (gz - kz < 0.5f) ? -1 : 1;   // the adjacent cell that can matter
    // The eight cells are probed TOGETHER, two consecutive table entries per cell and round trip: a wave waits once per step
    // of the longest probe run among its 512 cells, not once per step of every cell in turn (200k x 200k: 33.3 -> 30.6 us;
    // 800k sources: 81.9 -> 73.7 us; tools/studies/icp_grid_scaling.py).  Probing does not wrap (k_grid_insert).
    // Every step's eight loads are UNCONDITIONAL and stand back to back, and only then is any of them looked at: a load under
    // `if (pending & (1u << c))` becomes an exec-masked block of its own with a full wait (vmcnt(0)) in front of it, eight
    // serial round trips per step instead of one.  A cell whose probe has ended reads table[0] instead - one cached line for all
    // such lanes (64 lanes reloading 64 slots of their own cost the texture path more than the round trips saved) - and what
    // it reads is not looked at.
    unsigned tag[8], slot[8];
    int j[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const unsigned long long key = grid_key(cx + ((c & 1) ? sx : 0), cy + ((c & 2) ? sy : 0), cz + ((c & 4) ? sz : 0));
        tag[c] = grid_tag(key);
        slot[c] = grid_slot(key, shift);
        j[c] = -1;
    }
    (void)mask;
    unsigned pending = 0xffu;
    bool hit = false, in_range = false;
    uint2 key2 = make_uint2(0u, 0u);
    if constexpr (PROBE == 1 || PROBE == 2) {
        in_range = fabsf(gx) < GRID_MAX_COORD && fabsf(gy) < GRID_MAX_COORD && fabsf(gz) < GRID_MAX_COORD;      // false for NaN
        key2.x = ((unsigned)cx & 0x3ffffu) | ((unsigned)cy << 18);
        key2.y = (((unsigned)cy >> 14) & 0xfu) | (((unsigned)cz & 0x3ffffu) << 4) | (sx > 0 ? 1u << 22 : 0u) | (sy > 0 ? 1u << 23 : 0u) |
                 (sz > 0 ? 1u << 24 : 0u) | PROBE_VALID;
        hit = PROBE == 2 || (in_range && lc->key.x == key2.x && lc->key.y == key2.y);
        if (hit) {
            j[0] = (int)lc->h0.x; j[1] = (int)lc->h0.y; j[2] = (int)lc->h0.z; j[3] = (int)lc->h0.w;
            j[4] = (int)lc->h1.x; j[5] = (int)lc->h1.y; j[6] = (int)lc->h1.z; j[7] = (int)lc->h1.w;
            pending = 0u;      // this lane sits the loop out; a wave whose lanes all hit skips it
        }
        *missed = !hit;
    }
    while (pending) {
        uint4 e[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) e[c] = *reinterpret_cast<const uint4*>(&table[(pending & (1u << c)) ? slot[c] : 0u]);   // 16 bytes at an 8-byte-aligned address
        const unsigned was = pending;
        pending = 0u;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool on = (was & (1u << c)) != 0u;
            const bool hit0 = on && e[c].x == tag[c], go1 = on && !hit0 && e[c].x != GRID_EMPTY;
            const bool hit1 = go1 && e[c].z == tag[c], next = go1 && !hit1 && e[c].z != GRID_EMPTY;
            j[c] = hit0 ? (int)e[c].y : hit1 ? (int)e[c].w : j[c];
            slot[c] += next ? 2u : 0u;
            pending |= next ? 1u << c : 0u;
        }
    }
    if constexpr (PROBE == 1) {
        if (!hit && in_range) {
            pc->key[i] = key2;
            pc->head[i] = make_uint4((unsigned)j[0], (unsigned)j[1], (unsigned)j[2], (unsigned)j[3]);
            pc->head[(size_t)ns + i] = make_uint4((unsigned)j[4], (unsigned)j[5], (unsigned)j[6], (unsigned)j[7]);
        }
    }
    bd = INFINITY; bo = INT_MAX;
    if constexpr (PROBE == 3) {      // the probes alone: their heads kept alive, nothing walked
        if ((j[0] & j[1] & j[2] & j[3] & j[4] & j[5] & j[6] & j[7]) == 0x7ffffff1) bo = 0;
        return;
    }
    auto take = [&](const float4 t, int idx, bool live) {
        const float ex = px - t.x, ey = py - t.y, ez = pz - t.z;
        const float d2 = ex * ex + (ey * ey + ez * ez);    // the scan's expression
        if (live && d2 <= tau && (d2 < bd || (d2 == bd && idx < bo))) {
            bd = d2; bo = idx;
            if (bq) { bq[0] = t.x; bq[1] = t.y; bq[2] = t.z; }
        }
    };
    // the cells' lists (cells hold one or two points): the eight lists advance TOGETHER, one round trip per step of the longest
    // list among a wave's 512 cells instead of a sum over the cells.  Again eight unconditional loads back to back (`if (nx[c]
    // >= 0) t[c] = node[nx[c]]` serialises like the probes above): an empty cell and a list that has ended read node[0], which
    // exists for every nt >= 1 and is one cached line for all such lanes, and take() is told not to count it.
    int nx[8];
    bool more = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) { nx[c] = j[c]; more |= nx[c] >= 0; }
    while (more) {
        float4 t[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) t[c] = node[nx[c] >= 0 ? nx[c] : 0];
        more = false;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool live = nx[c] >= 0;
            take(t[c], nx[c], live);
            nx[c] = live ? __float_as_int(t[c].w) : -1;
            more |= nx[c] >= 0;
        }
    }
}

// One lane per source point.  (Running this search inside k_icp_accumulate - one launch per iteration, no correspondence
// arrays in between - was measured slower twice, 110 us against 44 + 35 and later 56.5 against 49.6 at 200k x 200k: that kernel's 29
// double accumulators and four points in flight leave one wave per SIMD to hide the probes' latency.  k_icp_iterate below fuses the
// other way round: this kernel's shape and registers for the search, the sums formed afterwards from records in LDS.)
// PROBE: the probe cache (grid_nearest); the lanes that probed are counted per workgroup and added to *pc.misses by one thread, only when
// there are any (one add per WAVE, 782 to one word per launch at 50,000 sources, cost a short call 8 us per iteration).
template <int PROBE = 0>
__global__ __launch_bounds__(256)
void k_icp_nn_grid(const float* __restrict__ src, int ns, const GridEntry* __restrict__ table, const float4* __restrict__ node,
                   unsigned mask, int shift, float inv_cell, const IcpState* __restrict__ st, float tau,
                   float* __restrict__ out_d2, int* __restrict__ out_idx, ProbeCache pc) {
    if (st->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if constexpr (PROBE == 0) {
        if (i >= ns) return;
        float px, py, pz;
        transform_point(st->T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
        float bd; int bo;
        grid_nearest(table, node, mask, shift, inv_cell, px, py, pz, tau, bd, bo);
        out_d2[i] = bo == INT_MAX ? FLT_MAX : bd;
        out_idx[i] = bo == INT_MAX ? 0 : bo;
    } else {
        __shared__ int wave_misses[4];      // every thread reaches the barrier: st->done is uniform, a lane past ns searches nothing but stays
        bool missed = false;
        if (i < ns) {
            const float s0 = src[3 * i], s1 = src[3 * i + 1], s2 = src[3 * i + 2];
            const ProbeLane lc = probe_load(pc, i, ns);      // beside the source point: one wait for both
            float px, py, pz;
            transform_point(st->T, s0, s1, s2, px, py, pz);
            float bd; int bo;
            grid_nearest<PROBE>(table, node, mask, shift, inv_cell, px, py, pz, tau, bd, bo, nullptr, &pc, &lc, i, ns, &missed);
            out_d2[i] = bo == INT_MAX ? FLT_MAX : bd;
            out_idx[i] = bo == INT_MAX ? 0 : bo;
        }
        const unsigned long long mm = __ballot(missed);
        if ((threadIdx.x & 63) == 0) wave_misses[threadIdx.x >> 6] = __popcll(mm);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (wave_misses[0] + wave_misses[1]) + (wave_misses[2] + wave_misses[3]);
            if (m) atomicAdd(pc.misses, m);
        }
    }
}

// Sum over the 64 lanes with DPP row operations on the two halves of the double (no LDS crossbar round trips, unlike
// __shfl_down): valid in lane 63.  A fixed order, like the shuffle tree it replaces.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double wave_sum_lane63(double v) {
    v += dpp_f64<0xB1, 0xF>(v);     // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E, 0xF>(v);     // quad_perm [2,3,0,1]
    v += dpp_f64<0x141, 0xF>(v);    // row_half_mirror
    v += dpp_f64<0x140, 0xF>(v);    // row_mirror: every lane of a 16-lane row holds the row sum
    v += dpp_f64<0x142, 0xA>(v);    // row_bcast15 into rows 1 and 3 (a disabled row receives +0)
    v += dpp_f64<0x143, 0xC>(v);    // row_bcast31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The pieces of one accumulation launch, shared by k_icp_accumulate (one problem) and k_icp_accumulate_multi (one problem per
// instance of a batch): the sums of one accepted correspondence, the block's slab and the fold of the last block, the update.
// MODE 0: point-to-plane (21 upper-triangular JtJ + 6 Jtr), MODE 1: point-to-point moments, MODE 2: count / error only, MODE 3: GICP
// (21 upper-triangular JtMJ + 6 JtMe, point-to-plane's slots), MODE 4: colored ICP (point-to-plane's slots, two rows per
// correspondence).  ROBUST: + n_eff (correspondences of weight > 0) last, point-to-point
// the weight sum W before it.
template <int MODE, bool ROBUST = false>
constexpr int acc_nv() { return (MODE == 0 || MODE >= 3) ? (ROBUST ? 30 : 29) : (MODE == 1 ? (ROBUST ? 19 : 17) : 2); }

// the pose a launch reads at its start: the 3x4 part column by column, and the bottom row
__device__ __forceinline__ void acc_load_pose(const IcpState* st, float* T /* 12 */, float* Tb /* 4 */) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) T[c * 3 + r] = st->T[c * 4 + r];
    Tb[0] = st->T[3]; Tb[1] = st->T[7]; Tb[2] = st->T[11]; Tb[3] = st->T[15];     // (0 0 0 1 unless the caller's start pose says otherwise)
}

// p = R*s + t with each row evaluated as r0*sx + (r1*sy + r2*sz), then + t (see transform_point), from acc_load_pose's T
__device__ __forceinline__ void acc_transform(const float* T, float sx, float sy, float sz, float& px, float& py, float& pz) {
    px = (T[0] * sx + (T[3] * sy + T[6] * sz)) + T[9];
    py = (T[1] * sx + (T[4] * sy + T[7] * sz)) + T[10];
    pz = (T[2] * sx + (T[5] * sy + T[8] * sz)) + T[11];
}

// a = R*s, the rotation of acc_transform without the translation (a source normal into the current pose); LD: the pose's column
// pitch, 3 for acc_load_pose's T, 4 for a column-major 4x4
template <int LD = 3>
__device__ __forceinline__ void acc_rotate(const float* T, float sx, float sy, float sz, float& ax, float& ay, float& az) {
    ax = T[0] * sx + (T[LD] * sy + T[2 * LD] * sz);
    ay = T[1] * sx + (T[LD + 1] * sy + T[2 * LD + 1] * sz);
    az = T[2] * sx + (T[LD + 2] * sy + T[2 * LD + 2] * sz);
}

// What MODE's kernels take beyond the common arguments, by value as their LAST parameter (the other arguments keep their places):
// nothing, GICP's source normals (laid out like the source points) and c = 1 - epsilon, or colored ICP's source colours (laid out
// like the source points), the target's colour table (float4 (I, d) per point), lg = sqrtf(lambda) and lc = sqrtf(1 - lambda).
template <int MODE> struct IcpArgs {};
template <> struct IcpArgs<3> { const float* src_normals; float c; };
template <> struct IcpArgs<4> { const float* src_rgb; const float* tgt_color; float lg, lc; };

// ... and what acc_terms takes per correspondence besides p and the target: nothing, GICP's a = R ns (the source normal in the
// current pose) and c, or colored ICP's colour table, the source point's intensity Is = ((r + g) + b) / 3.0f, lg and lc.
template <int MODE> struct CorrPt {};
template <> struct CorrPt<3> { float ax, ay, az, c; };
template <> struct CorrPt<4> { const float* tgt_color; float Is, lg, lc; };

// CorrPt of source point i (its index in the arrays laid out like the source points, in the caller's index type: the address
// arithmetic stays the caller's) in the pose T of column pitch LD (acc_rotate)
template <int MODE, int LD = 3, class Index>
__device__ __forceinline__ CorrPt<MODE> corr_pt(const IcpArgs<MODE>& a, const float* T, Index i) {
    if constexpr (MODE == 3) {
        CorrPt<3> x;
        acc_rotate<LD>(T, a.src_normals[3 * i], a.src_normals[3 * i + 1], a.src_normals[3 * i + 2], x.ax, x.ay, x.az);
        x.c = a.c;
        return x;
    } else if constexpr (MODE == 4) {
        const float* __restrict__ rgb = a.src_rgb + 3 * (size_t)i;
        return CorrPt<4>{a.tgt_color, ((rgb[0] + rgb[1]) + rgb[2]) / 3.0f, a.lg, a.lc};
    } else return {};
}

// What a correspondence gathers from the target side, by the target's index: the point q, the normal n (point-to-plane, GICP,
// colored ICP) and colored ICP's (I, d).  The FETCH half of corr_terms / acc_terms: a caller with several correspondences in hand
// fetches them all before it looks at any (k_icp_accumulate), the others fetch and use (corr_terms, acc_terms).  (CorrTgt: icp_terms.hpp)
template <int MODE>
__device__ __forceinline__ CorrTgt corr_fetch(int idx, const float* tgt, const float* tgt_normals, const CorrPt<MODE>& X) {
    CorrTgt G;
    if (MODE == 2) return G;
    G.q[0] = tgt[3 * idx]; G.q[1] = tgt[3 * idx + 1]; G.q[2] = tgt[3 * idx + 2];
    if (MODE != 1) { G.n[0] = tgt_normals[3 * idx]; G.n[1] = tgt_normals[3 * idx + 1]; G.n[2] = tgt_normals[3 * idx + 2]; }
    if constexpr (MODE == 4) G.tc = reinterpret_cast<const float4*>(X.tgt_color)[idx];   // (Iq, d)
    return G;
}

// One accepted correspondence, source point p (transformed) paired with target idx, in the float steps of registration.cpp: its
// target q and, point-to-plane, J and r (corr_jr).  Every path's sums and records are built from these (acc_terms, ref_record), so
// that every path sees the same bits.
template <int MODE>
__device__ __forceinline__ void corr_terms(float px, float py, float pz, int idx, const float* tgt, const float* tgt_normals,
                                           float* q /* 3 */, float* J /* 6 */, float& r) {
    const CorrTgt G = corr_fetch<MODE == 0 ? 0 : 1>(idx, tgt, tgt_normals, CorrPt<MODE == 0 ? 0 : 1>{});
    q[0] = G.q[0]; q[1] = G.q[1]; q[2] = G.q[2];
    if (MODE == 0) corr_jr(px, py, pz, G, J, r);
}

// the tree sums' terms of one accepted correspondence at squared distance d2, handed to put(k, term) for k = 0 .. acc_nv<MODE>() - 1:
// {1, d2, then MODE 0 the 21 upper-triangular J[a] * J[b] and the 6 J[a] * r, each product formed in float and widened; MODE 1 p, q
// and the 9 p[a] * q[b], p and q widened first}.  put is the caller's way of combining them (+= into a lane's sums, = into a fresh
// slab row: 0.0 + -0.0 is +0.0); each term is put as it is formed.
// MODE 3 (GICP): the 21 + 6 terms of include/tdv_hip.h (tdv_gicp) from p, the target point and normal and X, each formed in float in
// the header's order and widened.
// MODE 4 (colored ICP): the 21 + 6 terms of include/tdv_hip.h (tdv_colored_icp) from p, the target point and normal and X: per slot
// (double)(JG[a] * JG[b]) + (double)(JC[a] * JC[b]), resp. * rG and * rC, each product formed in float.  ROBUST: each row weighted
// by its own residual, (double)wG * (JG product) + (double)wC * (JC product), n_eff = (wG > 0 || wC > 0).
// ROBUST: the weight w = loss_weight(L, e) of this correspondence (e = r point-to-plane, sqrtf(d2) point-to-point, GICP the
// Mahalanobis residual sqrtf(fmaxf(0, e . g))) scales every term after the first two: (double)w * term, exact for the f32 products of
// point-to-plane and GICP and for p and q; w * (P[a] * Q[b]) is rounded once.  Then point-to-point W = w, and last n_eff = (w > 0).
// {1, d2} stay unweighted: n_corr, rmse and fitness are L2's.
// This is the ADD half, from the target as corr_fetch<MODE> fetched it (G); acc_terms below fetches and adds.
template <int MODE, bool ROBUST = false, class Put>
__device__ __forceinline__ void acc_terms_add(float px, float py, float pz, float d2, const CorrTgt& G, IcpLoss L, CorrPt<MODE> X, Put put) {
    if constexpr (MODE == 0 || MODE == 1) {     // through the record, as the one-launch iteration forms them (rec_terms)
        CorrRec R;
        corr_rec<MODE>(px, py, pz, d2, G, R);
        rec_terms<MODE, ROBUST>(R, L, put);
        return;
    }
    put(0, 1.0); put(1, (double)d2);
    if (MODE == 2) return;
    if constexpr (MODE == 4) {
        float J[6], en;
        const float* q = G.q;
        corr_jr(px, py, pz, G, J, en);     // J = [p x n | n], en = (p - q) . n
        const float nx = J[3], ny = J[4], nz = J[5];
        const float4 tc = G.tc;   // (Iq, d)
        const float lg = X.lg, lc = X.lc;
        // e_t = e - en n, the source point's offset projected on the target's tangent plane; g = (d . n) n - d = -m
        const float ex = px - q[0], ey = py - q[1], ez = pz - q[2];
        const float etx = ex - en * nx, ety = ey - en * ny, etz = ez - en * nz;
        const float dn = tc.y * nx + (tc.z * ny + tc.w * nz);
        const float gx = dn * nx - tc.y, gy = dn * ny - tc.z, gz = dn * nz - tc.w;
        const float de = tc.y * etx + (tc.z * ety + tc.w * etz);
        const float rG = lg * en, rC = lc * (X.Is - (tc.x + de));
        float JG[6], JC[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) JG[a] = lg * J[a];
        JC[0] = lc * (py * gz - pz * gy); JC[1] = lc * (pz * gx - px * gz); JC[2] = lc * (px * gy - py * gx);
        JC[3] = lc * gx; JC[4] = lc * gy; JC[5] = lc * gz;
        float wG = 1.f, wC = 1.f;
        if (ROBUST) { wG = loss_weight(L, rG); wC = loss_weight(L, rC); }
        const double wGd = wG, wCd = wC;
        const auto term = [&](float g, float c) { return ROBUST ? wGd * (double)g + wCd * (double)c : (double)g + (double)c; };
        int k = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) put(k++, term(JG[a] * JG[b], JC[a] * JC[b]));
#pragma unroll
        for (int a = 0; a < 6; ++a) put(k++, term(JG[a] * rG, JC[a] * rC));
        if (ROBUST) put(29, (wG > 0.f || wC > 0.f) ? 1.0 : 0.0);
        return;
    }
    if constexpr (MODE == 3) {
        const float qx = G.q[0], qy = G.q[1], qz = G.q[2];
        const float nx = G.n[0], ny = G.n[1], nz = G.n[2];
        const float c = X.c, ax = X.ax, ay = X.ay, az = X.az;
        // C = 2 I - c (a a^T + n n^T) in f32; M = C^-1 from the cofactors in f64 (C's condition number is about 1 / epsilon: in f32 the
        // cancellation in the cofactors and the determinant would cost ~1e-7 / epsilon of M), rounded to f32
        const float C00 = 2.f - c * (ax * ax + nx * nx), C11 = 2.f - c * (ay * ay + ny * ny), C22 = 2.f - c * (az * az + nz * nz);
        const float C01 = -(c * (ax * ay + nx * ny)), C02 = -(c * (ax * az + nx * nz)), C12 = -(c * (ay * az + ny * nz));
        const double D00 = C00, D11 = C11, D22 = C22, D01 = C01, D02 = C02, D12 = C12;
        const double A00 = D11 * D22 - D12 * D12, A11 = D00 * D22 - D02 * D02, A22 = D00 * D11 - D01 * D01;
        const double A01 = D02 * D12 - D01 * D22, A02 = D01 * D12 - D02 * D11, A12 = D01 * D02 - D00 * D12;
        const double sdet = 1.0 / (D00 * A00 + (D01 * A01 + D02 * A02));
        const float M00 = (float)(A00 * sdet), M11 = (float)(A11 * sdet), M22 = (float)(A22 * sdet);
        const float M01 = (float)(A01 * sdet), M02 = (float)(A02 * sdet), M12 = (float)(A12 * sdet);
        // e = p - q, g = M e
        const float ex = px - qx, ey = py - qy, ez = pz - qz;
        const float gx = M00 * ex + (M01 * ey + M02 * ez), gy = M01 * ex + (M11 * ey + M12 * ez), gz = M02 * ex + (M12 * ey + M22 * ez);
        float w = 1.f;
        if (ROBUST) w = loss_weight(L, sqrtf(fmaxf(0.f, ex * gx + (ey * gy + ez * gz))));
        const double wd = w;
        const auto term = [&](int k, float t) { put(k, ROBUST ? wd * (double)t : (double)t); };
        // J = [-[p]x | I]: J_a . x = (p x x)_a for a < 3.  P_j = p x (row j of M) = the column j of J_w^T M; K_b = (P_0[b], P_1[b], P_2[b]) = M J_b
        const float P00 = py * M02 - pz * M01, P01 = pz * M00 - px * M02, P02 = px * M01 - py * M00;
        const float P10 = py * M12 - pz * M11, P11 = pz * M01 - px * M12, P12 = px * M11 - py * M01;
        const float P20 = py * M22 - pz * M12, P21 = pz * M02 - px * M22, P22 = px * M12 - py * M02;
        term(2, py * P20 - pz * P10);  term(3, py * P21 - pz * P11);  term(4, py * P22 - pz * P12);       // H00, H01, H02 = (p x K_b)_0
        term(5, P00);  term(6, P10);  term(7, P20);                                                       // H03, H04, H05
        term(8, pz * P01 - px * P21);  term(9, pz * P02 - px * P22);                                      // H11, H12 = (p x K_b)_1
        term(10, P01); term(11, P11); term(12, P21);                                                      // H13, H14, H15
        term(13, px * P12 - py * P02);                                                                    // H22 = (p x K_2)_2
        term(14, P02); term(15, P12); term(16, P22);                                                      // H23, H24, H25
        term(17, M00); term(18, M01); term(19, M02); term(20, M11); term(21, M12); term(22, M22);         // H33 .. H55
        term(23, py * gz - pz * gy); term(24, pz * gx - px * gz); term(25, px * gy - py * gx);           // v0..2 = p x g
        term(26, gx); term(27, gy); term(28, gz);                                                         // v3..5 = g
        if (ROBUST) put(29, w > 0.f ? 1.0 : 0.0);
        return;
    }
}

template <int MODE, bool ROBUST = false, class Put>
__device__ __forceinline__ void acc_terms(float px, float py, float pz, float d2, int idx, const float* tgt, const float* tgt_normals,
                                          IcpLoss L, CorrPt<MODE> X, Put put) {
    acc_terms_add<MODE, ROBUST>(px, py, pz, d2, corr_fetch<MODE>(idx, tgt, tgt_normals, X), L, X, put);
}

// this lane's sums += one accepted correspondence (p, target idx at squared distance best)
template <int MODE, bool ROBUST = false>
__device__ __forceinline__ void acc_add(double* v, float px, float py, float pz, float best, int idx,
                                        const float* __restrict__ tgt, const float* __restrict__ tgt_normals, IcpLoss L, CorrPt<MODE> X) {
    acc_terms<MODE, ROBUST>(px, py, pz, best, idx, tgt, tgt_normals, L, X, [v](int k, double t) { v[k] += t; });
}

// LDS of one accumulation block
struct AccShared {
    double red[8][ACC_NV];
    double tot[ACC_NV];
    float solve_ws[56];
    bool is_last;
};

// Every block reduces its lanes' sums v[] to its slab slabs[slab] (fixed order: wave64 DPP -> LDS); the block that takes the last
// of nblocks tickets folds slabs[0 .. nblocks) in a fixed order into sh.tot[] and returns true (all its threads) - the result
// does not depend on which block that is.  The caller's thread 0 of that block then resets *ticket and updates the state.
// The first half's end: the four wave sums sh.red[0 .. 3][k] (lane 63 of accumulate wave g wrote red[g][k]) combined into slabs[slab].
template <int NV>
__device__ __forceinline__ void acc_slab_store(double* slabs, int slab, AccShared& sh) {
    __syncthreads();
    if (threadIdx.x < ACC_NV) {
        double s = 0.0;
        if (threadIdx.x < NV) s = (sh.red[0][threadIdx.x] + sh.red[1][threadIdx.x]) + (sh.red[2][threadIdx.x] + sh.red[3][threadIdx.x]);
        slabs[(size_t)slab * ACC_NV + threadIdx.x] = s;
    }
}

// The second half: ticket and fold, by a workgroup of 256 threads or more whose wave 0 wrote its slab (acc_slab_store).  Threads past
// the first 256 only join the barriers.
__device__ __forceinline__ bool acc_ticket_fold(double* slabs, int nblocks, unsigned* ticket, AccShared& sh) {
    // ---- last block: fold ----------------------------------------------------------------------------------------------
    // Release by the wave that wrote the slab (wave 0; thread 0 then moves the ticket), acquire by the block that folds.
    // __threadfence() by every thread was a write-back AND an invalidate of the XCD's L2 (buffer_wbl2 + buffer_inv) from all
    // four waves of all 196 blocks - invalidating the target lines the blocks still running were gathering.
    if (threadIdx.x < 64) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (threadIdx.x == 0) sh.is_last = atomicAdd(ticket, 1u) == (unsigned)nblocks - 1u;
    __syncthreads();
    if (!sh.is_last) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int vv = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (threadIdx.x < 256) {
        // slabs were written by other blocks of this launch: the agent-scope fence above makes them visible to plain loads
        // sixteen slab rows per thread and round, all loads of a round in flight together (the fold is a chain of round trips:
        // 196 blocks at 200k points were 7 rounds of 4 loads, now 2 rounds of 16); fixed order, as before
        const double* sl = slabs;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int b2 = g; b2 < nblocks; b2 += 128) {
            double a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = b2 + 8 * j < nblocks ? sl[(size_t)(b2 + 8 * j) * ACC_NV + vv] : 0.0;
#pragma unroll
            for (int j = 0; j < 16; j += 4) { s0 += a[j]; s1 += a[j + 1]; s2 += a[j + 2]; s3 += a[j + 3]; }
        }
        sh.red[g][vv] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (threadIdx.x < ACC_NV)
        sh.tot[vv] = ((sh.red[0][vv] + sh.red[1][vv]) + (sh.red[2][vv] + sh.red[3][vv])) + ((sh.red[4][vv] + sh.red[5][vv]) + (sh.red[6][vv] + sh.red[7][vv]));
    __syncthreads();
    return true;
}

template <int MODE, bool ROBUST = false>
__device__ __forceinline__ bool acc_slab_fold(const double* v, double* slabs, int slab, int nblocks, unsigned* ticket, AccShared& sh) {
    constexpr int NV = acc_nv<MODE, ROBUST>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum_lane63(v[k]);
        if (lane == 63) sh.red[wave][k] = s;
    }
    acc_slab_store<NV>(slabs, slab, sh);
    return acc_ticket_fold(slabs, nblocks, ticket, sh);
}

// thread 0 of the folding block: solve, update, stopping rule from the folded sums (pose as acc_load_pose read it)
template <int MODE, bool ROBUST = false>
__device__ __forceinline__ void acc_finish(AccShared& sh, int ns, IcpState* st, int fixed_iterations, int iter0, float rmse0, const float* T, const float* Tb) {
    if (MODE == 2) st->n_corr = (int)(sh.tot[0] + 0.5);
    else {
        float T16[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) { T16[c * 4] = T[c * 3]; T16[c * 4 + 1] = T[c * 3 + 1]; T16[c * 4 + 2] = T[c * 3 + 2]; T16[c * 4 + 3] = Tb[c]; }
        icp_update<MODE, false, ROBUST>(sh.tot, ns, st, fixed_iterations, iter0, rmse0, T16, sh.solve_ws);
    }
}

// nearest target of source i from the search's output: (best d2, index).  direct (pruned / grid search): the one entry is the final
// (d2, target index); else (brute-force scan) the minimum over the splits, in the lowest target of its chunk at that distance
__device__ __forceinline__ void resolve_nn(int i, int ns_pad, int nsplit, const float* __restrict__ pd2, const int* __restrict__ pchunk, int direct,
                                           const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
                                           float px, float py, float pz, float& best, int& idx) {
    best = FLT_MAX; int bc = 0;
    for (int s = 0; s < nsplit; ++s) {
        const float d = pd2[(size_t)s * ns_pad + i];
        const int c = pchunk[(size_t)s * ns_pad + i];
        if (d < best) { best = d; bc = c; }
    }
    idx = 0;
    if (direct) idx = bc;
    else if (best < FLT_MAX) {
        idx = bc;
#pragma unroll
        for (int t = NN_CH - 1; t >= 0; --t) {
            const float dx = px - tx[bc + t], dy = py - ty[bc + t], dz = pz - tz[bc + t];
            if (dx * dx + (dy * dy + dz * dz) == best) idx = bc + t;
        }
    }
}

// ---- the direct path's points of a lane (pruned / grid search: one (d2, target index) per source), fetched TOGETHER ----------------
// A lane's points do not depend on one another, but a loop that takes them one by one waits three times per point: for the source
// point and its d2, for its target index, and for the gather of that target.  At one wave per SIMD (196 blocks of 125 VGPRs at 200k
// points) nothing else hides those waits.  So the work is cut in three: acc_fetch issues every point's source, d2 and index loads;
// acc_points transforms and applies the acceptance test, issues every point's gathers (corr_pt, corr_fetch), and only then adds
// the accepted points' terms into v[] in ascending point order - the f64 order of the loop it replaces.  All loads are
// unconditional, from a clamped source index resp. target 0 for a rejected point: a load under `if (accepted)` is an exec-masked
// block of its own with a full wait in front of it.
constexpr int ACC_GROUP = 4;     // points fetched together (make_plan's acc_ppt)
template <int P> struct AccSrc { float sx[P], sy[P], sz[P], d[P]; int c[P]; };

// point q of the group is source i0 + 256 q of the ns points at src / pd2 / pidx (a point past the end reads the last one)
template <int P>
__device__ __forceinline__ AccSrc<P> acc_fetch(const float* __restrict__ src, const float* __restrict__ pd2, const int* __restrict__ pidx, int i0, int ns) {
    AccSrc<P> S;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int i = i0 + 256 * q, il = i < ns ? i : ns - 1;
        S.sx[q] = src[3 * il]; S.sy[q] = src[3 * il + 1]; S.sz[q] = src[3 * il + 2];
        S.d[q] = pd2[il]; S.c[q] = pidx[il];
    }
    return S;
}

// the first nq points of the group S (those below ns): outputs, gathers, then v[] += the accepted ones' terms.  off: where the
// ns points start in the arrays laid out like the source points (corr_pt), in the caller's index type
template <int MODE, bool ROBUST, int P, class Index>
__device__ __forceinline__ void acc_points(double* v, const AccSrc<P>& S, int i0, int nq, int ns, const float* T, float tau_accept,
                                           const float* __restrict__ tgt, const float* __restrict__ tgt_normals, IcpLoss loss,
                                           const IcpArgs<MODE>& a, Index off,
                                           int* __restrict__ out_corr, float* __restrict__ out_d2, uint8_t* __restrict__ out_acc) {
    float px[P], py[P], pz[P], best[P];
    bool acc[P];
    CorrPt<MODE> X[P];
    CorrTgt G[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int i = i0 + 256 * q, il = i < ns ? i : ns - 1;
        const bool valid = q < nq && i < ns;
        acc_transform(T, S.sx[q], S.sy[q], S.sz[q], px[q], py[q], pz[q]);
        best[q] = S.d[q] < FLT_MAX ? S.d[q] : FLT_MAX;          // resolve_nn's direct case: one split
        const int idx = S.d[q] < FLT_MAX ? S.c[q] : 0;
        acc[q] = valid && best[q] <= tau_accept;
        if (valid) {
            if (out_corr) out_corr[i] = idx;
            if (out_d2) out_d2[i] = best[q];
            if (out_acc) out_acc[i] = acc[q] ? 1 : 0;
        }
        X[q] = corr_pt(a, T, off + il);
        G[q] = corr_fetch<MODE>(acc[q] ? idx : 0, tgt, tgt_normals, X[q]);
    }
    // (branches, not a select per sum: as one straight block the scheduler moves the gathers back down to their uses to save registers)
#pragma unroll
    for (int q = 0; q < P; ++q)
        if (acc[q]) acc_terms_add<MODE, ROBUST>(px[q], py[q], pz[q], best[q], G[q], loss, X[q], [v](int k, double t) { v[k] += t; });
}

// One launch per iteration: every block reduces its points to one slab; the block that finishes LAST (atomic ticket) folds all
// slabs in a fixed order, solves, and updates the state on the device.
template <int MODE, int ACC_PPT, bool ROBUST = false>   // ACC_PPT source points per thread (summed per lane in index order); ROBUST: loss L
__global__ __launch_bounds__(256)
void k_icp_accumulate(const float* __restrict__ src, int ns, int ns_pad,
                      const float* __restrict__ tgt, const float* __restrict__ tgt_normals,
                      const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
                      int nsplit, const float* __restrict__ pd2, const int* __restrict__ pchunk, int direct,
                      IcpState* st, float tau_accept, int fixed_iterations, IcpLoss loss,
                      double* slabs, unsigned* ticket,
                      int* __restrict__ out_corr, float* __restrict__ out_d2, uint8_t* __restrict__ out_acc, IcpArgs<MODE> args) {
    if (st->done) return;       // (the loads below ahead of this wait: 0.2 us, the kernel's own spread - profiles/r15)
    const IcpArgs<MODE> a = args;
    const int i0 = blockIdx.x * (256 * ACC_PPT) + threadIdx.x;
    AccSrc<ACC_PPT> S;
    if (direct) S = acc_fetch<ACC_PPT>(src, pd2, pchunk, i0, ns);   // (nsplit is 1 on that path: pd2 and pchunk hold one entry per source)
    const int iter0 = st->iter; const float rmse0 = st->rmse;
    float T[12], Tb[4];
    acc_load_pose(st, T, Tb);
    double v[ACC_NV];
#pragma unroll
    for (int k = 0; k < ACC_NV; ++k) v[k] = 0.0;
    if (direct) acc_points<MODE, ROBUST>(v, S, i0, ACC_PPT, ns, T, tau_accept, tgt, tgt_normals, loss, a, 0, out_corr, out_d2, out_acc);
    else {
        // the brute-force scan's splits (nsplit > 1, one point per thread outside study runs) keep the loop that takes a lane's
        // points one by one: resolve_nn's loads depend on the minimum over the splits
#pragma unroll 1
        for (int q = 0; q < ACC_PPT; ++q) {
            const int i = i0 + q * 256;
            if (i >= ns) continue;
            float px, py, pz;
            acc_transform(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
            float best; int idx;
            resolve_nn(i, ns_pad, nsplit, pd2, pchunk, direct, tx, ty, tz, px, py, pz, best, idx);
            const bool acc = best <= tau_accept;
            if (out_corr) out_corr[i] = idx;
            if (out_d2) out_d2[i] = best;
            if (out_acc) out_acc[i] = acc ? 1 : 0;
            if (!acc) continue;
            const CorrPt<MODE> X = corr_pt(a, T, i);
            acc_add<MODE, ROBUST>(v, px, py, pz, best, idx, tgt, tgt_normals, loss, X);
        }
    }
    __shared__ AccShared sh;
    if (!acc_slab_fold<MODE, ROBUST>(v, slabs, blockIdx.x, gridDim.x, ticket, sh)) return;
    if (threadIdx.x != 0) return;
    *ticket = 0u;   // ready for the next launch (stream order)
    acc_finish<MODE, ROBUST>(sh, ns, st, fixed_iterations, iter0, rmse0, T, Tb);
}

// ---- one launch per iteration: k_icp_nn_grid and k_icp_accumulate<MODE, 4> in one kernel (MODE 0 and 1) ----------------------------
// The search keeps its shape - one lane per source point, nothing but the search in its registers - and the sums do not live in the
// searching lanes: every lane leaves the float record of its correspondence (corr_rec) in LDS, and after one barrier the sixteen waves
// form the slab from the records.  Workgroup blk is slab blk of k_icp_accumulate<MODE, 4>: 1,024 consecutive source points, thread t
// searching point blk * 1024 + t, which is point q = t >> 8 of that kernel's lane L = t & 255.
//   search   p = acc_transform (transform_point's expression: the bits both of today's kernels see), grid_nearest, which also hands back
//            the winner's coordinates as node[] holds them (k_grid_insert's copy of the target's: no gather of tgt is left); the normal
//            by the found index (index 0 when nothing was found, unconditionally, as acc_points); the record, d2 = FLT_MAX for a point
//            past ns or without a neighbour (tau_accept < FLT_MAX on this path, so the test where the terms are added rejects it).
//   sums     wave w takes accumulate wave g = w & 3 (lanes 64 g .. 64 g + 63 of L) and the terms [8 s, 8 s + 8) of s = w >> 2.  A lane reads
//            its four records in q order and adds the accepted ones' terms (rec_terms: the products formed in float and widened, as
//            k_icp_accumulate forms them from the same record) into f64 sums that start at 0.0; wave_sum_lane63; lane 63 stores
//            sh.red[g][k]; acc_slab_store combines the four.  Per term that is k_icp_accumulate's tree, lane by lane: the same q
//            order in a lane, the same DPP order over the same 64 lanes, the same four-wave combine, the same slab - so the slab has
//            its bits, and ticket, fold and update are its code (acc_ticket_fold, acc_finish).
// Every barrier is reached by all 1,024 threads: st->done is uniform, and a lane past ns searches nothing but stays.
constexpr int IT_THREADS = 1024;
constexpr int IT_TERMS = 8;          // terms per wave (acc_nv <= 32 = 4 subsets of 8)
template <int MODE> constexpr int rec_words() { return MODE == 0 ? 8 : 7; }

// the sums of the terms [8 S, 8 S + 8) over this lane's four records, reduced over the wave into sh.red[g]
template <int MODE, bool ROBUST, int S>
__device__ __forceinline__ void it_sum_subset(const float (*rec)[IT_THREADS], int L, int g, float tau_accept, IcpLoss loss, AccShared& sh) {
    constexpr int NV = acc_nv<MODE, ROBUST>(), K0 = IT_TERMS * S, NK = NV - K0 < IT_TERMS ? NV - K0 : IT_TERMS;
    if constexpr (NK > 0) {
        CorrRec R[ACC_GROUP];
#pragma unroll
        for (int q = 0; q < ACC_GROUP; ++q)
#pragma unroll
            for (int j = 0; j < rec_words<MODE>(); ++j) R[q].f[j] = rec[j][256 * q + L];
        double v[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) v[k] = 0.0;
#pragma unroll
        for (int q = 0; q < ACC_GROUP; ++q)
            if (R[q].f[0] <= tau_accept)
                rec_terms<MODE, ROBUST>(R[q], loss, [&v](int k, double t) { if (k >= K0 && k < K0 + NK) v[k - K0] += t; });
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const double s = wave_sum_lane63(v[k]);
            if ((threadIdx.x & 63) == 63) sh.red[g][K0 + k] = s;
        }
    }
}

// PROBE: the probe cache (grid_nearest).  Every wave leaves the number of its lanes that probed in LDS; after the barrier that is there
// anyway thread 0 adds the workgroup's total to *pc.misses - only if it is not zero, so a converged iteration issues no atomic.
template <int MODE, bool ROBUST, int PROBE = 0>
__global__ __launch_bounds__(IT_THREADS)
void k_icp_iterate(const float* __restrict__ src, int ns, const float* __restrict__ tgt_normals,
                   const GridEntry* __restrict__ table, const float4* __restrict__ node, unsigned mask, int shift, float inv_cell,
                   IcpState* st, float tau, int fixed_iterations, IcpLoss loss, double* slabs, unsigned* ticket, ProbeCache pc) {
    static_assert(MODE == 0 || MODE == 1, "the one-launch iteration exists for point-to-plane and point-to-point");
    static_assert(ACC_GROUP * 256 == IT_THREADS && 4 * IT_TERMS == ACC_NV, "a workgroup is one slab of k_icp_accumulate<MODE, 4>");
    if (st->done) return;
    __shared__ float rec[rec_words<MODE>()][IT_THREADS];
    __shared__ AccShared sh;
    const int iter0 = st->iter; const float rmse0 = st->rmse;
    float T[12], Tb[4];
    acc_load_pose(st, T, Tb);
    // ---- search ------------------------------------------------------------------------------------------------------------
    const int t = threadIdx.x, i = blockIdx.x * IT_THREADS + t;
    CorrRec R;
#pragma unroll
    for (int j = 0; j < REC_WORDS; ++j) R.f[j] = 0.f;
    R.f[0] = FLT_MAX;
    bool missed = false;
    if (i < ns) {
        const float s0 = src[3 * i], s1 = src[3 * i + 1], s2 = src[3 * i + 2];
        ProbeLane lc;
        if constexpr (PROBE != 0) lc = probe_load(pc, i, ns);      // beside the source point: one wait for both
        float px, py, pz;
        acc_transform(T, s0, s1, s2, px, py, pz);
        float bd; int bo;
        CorrTgt G;
        grid_nearest<PROBE>(table, node, mask, shift, inv_cell, px, py, pz, tau, bd, bo, G.q, &pc, &lc, i, ns, &missed);
        const bool found = bo != INT_MAX;
        const int idx = found ? bo : 0;
        if (MODE == 0) { G.n[0] = tgt_normals[3 * idx]; G.n[1] = tgt_normals[3 * idx + 1]; G.n[2] = tgt_normals[3 * idx + 2]; }
        if (!found) G.q[0] = G.q[1] = G.q[2] = 0.f;
        corr_rec<MODE>(px, py, pz, found ? bd : FLT_MAX, G, R);
    }
#pragma unroll
    for (int j = 0; j < rec_words<MODE>(); ++j) rec[j][t] = R.f[j];
    __shared__ int wave_misses[IT_THREADS / 64];
    if constexpr (PROBE != 0) {
        const unsigned long long mm = __ballot(missed);
        if ((t & 63) == 0) wave_misses[t >> 6] = __popcll(mm);
    }
    __syncthreads();
    if constexpr (PROBE != 0) {
        if (t == 0) {
            int m = 0;
#pragma unroll
            for (int k = 0; k < IT_THREADS / 64; ++k) m += wave_misses[k];
            if (m) atomicAdd(pc.misses, m);
        }
    }
    // ---- sums --------------------------------------------------------------------------------------------------------------
    const int w = t >> 6, g = w & 3, L = 64 * g + (t & 63);
    switch (w >> 2) {      // wave-uniform
    case 0: it_sum_subset<MODE, ROBUST, 0>(rec, L, g, tau, loss, sh); break;
    case 1: it_sum_subset<MODE, ROBUST, 1>(rec, L, g, tau, loss, sh); break;
    case 2: it_sum_subset<MODE, ROBUST, 2>(rec, L, g, tau, loss, sh); break;
    default: it_sum_subset<MODE, ROBUST, 3>(rec, L, g, tau, loss, sh); break;
    }
    acc_slab_store<acc_nv<MODE, ROBUST>()>(slabs, blockIdx.x, sh);
    if (!acc_ticket_fold(slabs, gridDim.x, ticket, sh)) return;
    if (threadIdx.x != 0) return;
    *ticket = 0u;   // ready for the next launch (stream order)
    acc_finish<MODE, ROBUST>(sh, ns, st, fixed_iterations, iter0, rmse0, T, Tb);
}

// ---- many instances against one target: two launches per iteration for the whole batch -------------------------------------
// Instance b = source points [src_off, src_off + ns) of the concatenated clouds with its own state st[b].  Each instance's range is
// padded to whole blocks in both kernels, so no block straddles two instances; blk_inst maps a block to its instance (the NN
// blocks first, then the accumulation blocks: one table, uploaded once per call).  The accumulation keeps, per instance, the
// points-per-thread and slab layout icp_run_dev picks for that instance alone (1 on the brute-force path, make_plan's 4 on the
// pruned and grid paths): the f64 tree - and therefore every bit of the result - is the single call's.
struct IcpInst {
    int src_off, ns;            // the instance's points in the concatenated clouds
    int nn_blk0;                // its first block in k_icp_nn_grid_multi's grid (256 points per block)
    int acc_blk0, acc_blocks;   // its first block in k_icp_accumulate_multi's grid, and how many (= its slabs, from slab acc_blk0 on)
    int ppt;                    // source points per thread of its accumulation
};

// k_icp_nn_grid for every instance: one lane per source point, transformed by its own instance's pose; blocks of finished
// instances return at once.  Output in the direct format at the point's position in the concatenated clouds.
__global__ __launch_bounds__(256)
void k_icp_nn_grid_multi(const float* __restrict__ src, const IcpInst* __restrict__ inst, const int* __restrict__ blk_inst,
                         const GridEntry* __restrict__ table, const float4* __restrict__ node, unsigned mask, int shift, float inv_cell,
                         const IcpState* __restrict__ st_all, float tau, float* __restrict__ out_d2, int* __restrict__ out_idx) {
    const int b = blk_inst[blockIdx.x];
    const IcpState* __restrict__ st = st_all + b;
    if (st->done) return;
    const IcpInst in = inst[b];
    const int i = (blockIdx.x - in.nn_blk0) * 256 + threadIdx.x;
    if (i >= in.ns) return;
    const int g = in.src_off + i;
    float px, py, pz;
    transform_point(st->T, src[3 * g], src[3 * g + 1], src[3 * g + 2], px, py, pz);
    float bd; int bo;
    grid_nearest(table, node, mask, shift, inv_cell, px, py, pz, tau, bd, bo);
    out_d2[g] = bo == INT_MAX ? FLT_MAX : bd;
    out_idx[g] = bo == INT_MAX ? 0 : bo;
}

// k_icp_accumulate for every instance: instance b's blocks write its slabs and take its ticket word tickets[b]; the last of them
// folds, solves and updates st[b].  The points-per-thread count is uniform over a block (runtime loop, as the single kernel's).
template <int MODE, bool ROBUST = false>
__global__ __launch_bounds__(256)
void k_icp_accumulate_multi(const float* __restrict__ src, const IcpInst* __restrict__ inst, const int* __restrict__ blk_inst,
                            const float* __restrict__ tgt, const float* __restrict__ tgt_normals,
                            const float* __restrict__ pd2, const int* __restrict__ pidx,
                            IcpState* st_all, float tau_accept, int fixed_iterations, IcpLoss loss, double* slabs, unsigned* tickets,
                            IcpArgs<MODE> args) {
    const int b = blk_inst[blockIdx.x];
    IcpState* st = st_all + b;
    if (st->done) return;
    const IcpInst in = inst[b];
    const int lb = blockIdx.x - in.acc_blk0;
    const float* __restrict__ s0 = src + (size_t)in.src_off * 3;
    const float* __restrict__ d0 = pd2 + in.src_off;
    const int* __restrict__ c0 = pidx + in.src_off;
    // as k_icp_accumulate's direct path, in groups of ACC_GROUP points (in.ppt is make_plan's 4 outside study runs: one group)
    const int i0 = lb * (256 * in.ppt) + threadIdx.x;
    AccSrc<ACC_GROUP> S = acc_fetch<ACC_GROUP>(s0, d0, c0, i0, in.ns);
    const int iter0 = st->iter; const float rmse0 = st->rmse;
    float T[12], Tb[4];
    acc_load_pose(st, T, Tb);
    double v[ACC_NV];
#pragma unroll
    for (int k = 0; k < ACC_NV; ++k) v[k] = 0.0;
#pragma unroll 1
    for (int q0 = 0; q0 < in.ppt; q0 += ACC_GROUP) {
        if (q0) S = acc_fetch<ACC_GROUP>(s0, d0, c0, i0 + 256 * q0, in.ns);
        acc_points<MODE, ROBUST>(v, S, i0 + 256 * q0, in.ppt - q0, in.ns, T, tau_accept, tgt, tgt_normals, loss, args, (size_t)in.src_off,
                                 (int*)nullptr, (float*)nullptr, (uint8_t*)nullptr);
    }
    __shared__ AccShared sh;
    if (!acc_slab_fold<MODE, ROBUST>(v, slabs + (size_t)in.acc_blk0 * ACC_NV, lb, in.acc_blocks, tickets + b, sh)) return;
    if (threadIdx.x != 0) return;
    tickets[b] = 0u;   // ready for the next launch (stream order)
    acc_finish<MODE, ROBUST>(sh, in.ns, st, fixed_iterations, iter0, rmse0, T, Tb);
}

// ---- reference-order accumulation (round 4; TDV_ICP_ACCUMULATE_REFERENCE) ------------------------------------------------
// The CPU path adds every accepted correspondence to its sums one after the other, in float, in ascending source index
// (/root/reference/src/registration.cpp:340-341 n_corr and total_error, :353-354 ATA and ATb; point-to-point: the two means
// :376-381, then the centred cross-covariance :383-386).  A float sum depends on its order, so the f64 tree above agrees with
// it to ~1e-7 only - which once moved a translation by 1.27e-6 m on a 5-iteration C5 instance (round 3's log) and could, in
// principle, flip the stopping rule |delta rmse| < 1e-6 (:406).  In this mode the sums ARE the reference's, bit for bit.
//
// What bounds it: a sum in the reference's rounding is ONE chain of dependent float additions - lane k of one wave owns
// accumulator k, and a wave issues a VALU instruction every 4 cycles whatever else the chip does.  Everything is arranged so
// that this wave executes one v_add_f32 and a quarter of a 16-byte LDS read per ACCEPTED correspondence and nothing else:
//   k_icp_flags / k_icp_scan_counts / k_icp_rows   (whole chip) the accepted correspondences, in source order, as dense 32-byte
//                records {d2, J[6], r} resp. {d2, p, q}: block counts, their exclusive scan, then every block writes its
//                records at its offset (order-preserving compaction: rejected points - 3 of 4 at the pipeline's 0.4-voxel
//                threshold - cost the chain nothing).  n_corr is the scan's total.
//   k_icp_fold_ref  ONE workgroup of 9 waves.  Waves 1-8 are loaders, one record slot per lane: they fetch tile t + 4 (512
//                records) into a 3-deep register ring, expand tile t + 1 into the 28 per-accumulator term rows
//                (J[a] * J[b], J[a] * r: the products the CPU forms, unfused) in LDS, double buffered; wave 0 adds tile t, lane
//                k walking row k in order.  A first version streamed 28 precomputed floats per point: 924 us per fold at
//                200k points, bound by what ONE CU can pull from HBM (~11 B per cycle, MI355X_MICROARCH.md) - hence the
//                8-float records and the expansion on the CU.  Then the one-thread solve / update / stopping rule of the
//                tree mode, on float sums.
// Selectable per ctx like the search; the f64 tree stays the default.
constexpr int REF_NR_PLANE = 28;     // term rows, point-to-plane: d2, 21 upper-triangular J^T J, 6 J^T r
constexpr int REF_NR_POINT = 9;      // term rows, point-to-point: pass 0 d2, p.xyz, q.xyz (7); pass 1 the 9 centred products
constexpr int REF_TILE = 512;        // records per LDS tile
constexpr int REF_LD = REF_TILE + 4; // row pitch in LDS (floats): lane k's 16-byte reads start 4 banks after lane k-1's
constexpr int REF_RING = 3;          // register stages of a loader lane (tiles in flight ahead of the expansion)

// the dense record of one accepted correspondence at squared distance d2 (corr_terms):
//   point-to-plane {d2, J0, J1, J2 | J3, J4, J5, r}     point-to-point {d2, px, py, pz | qx, qy, qz, 0}
template <int MODE>
__device__ __forceinline__ void ref_record(float px, float py, float pz, float d2, int idx, const float* tgt, const float* tgt_normals,
                                           float4& a, float4& b) {
    float q[3], J[6], r;
    corr_terms<MODE>(px, py, pz, idx, tgt, tgt_normals, q, J, r);
    if (MODE == 0) { a = make_float4(d2, J[0], J[1], J[2]); b = make_float4(J[3], J[4], J[5], r); }
    else { a = make_float4(d2, px, py, pz); b = make_float4(q[0], q[1], q[2], 0.f); }
}

// accepted correspondences per block of 256 source points
__global__ __launch_bounds__(256)
void k_icp_flags(int ns, int ns_pad, int nsplit, const float* __restrict__ pd2, const IcpState* __restrict__ st, float tau_accept, int* __restrict__ cnt) {
    if (st->done) return;
    __shared__ int s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    float best = FLT_MAX;
    if (i < ns) for (int s = 0; s < nsplit; ++s) best = fminf(best, pd2[(size_t)s * ns_pad + i]);
    const unsigned long long m = __ballot(i < ns && best <= tau_accept);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_c, __popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = s_c;
}

// off[b] = cnt[0] + ... + cnt[b - 1], off[nblocks] = the total (n_corr); one workgroup, chunks of 1024 counts
__global__ __launch_bounds__(1024)
void k_icp_scan_counts(const int* __restrict__ cnt, int nblocks, const IcpState* __restrict__ st, int* __restrict__ off) {
    if (st->done) return;
    __shared__ int s_w[16], s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const int c = b < nblocks ? cnt[b] : 0;
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int a = __shfl_up(inc, o, 64); if (lane >= o) inc += a; }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        int base = s_carry;
        for (int w = 0; w < wave; ++w) base += s_w[w];
        if (b < nblocks) off[b] = base + inc - c;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = base + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nblocks] = s_carry;
}

// the accepted correspondences as records rec[2 * pos], rec[2 * pos + 1] (ref_record; pos ascending with the source index)
template <int MODE>
__global__ __launch_bounds__(256)
void k_icp_rows(const float* __restrict__ src, int ns, int ns_pad,
                const float* __restrict__ tgt, const float* __restrict__ tgt_normals,
                const float* __restrict__ tx, const float* __restrict__ ty, const float* __restrict__ tz,
                int nsplit, const float* __restrict__ pd2, const int* __restrict__ pchunk, int direct,
                const IcpState* __restrict__ st, float tau_accept, const int* __restrict__ off, float4* __restrict__ rec) {
    if (st->done) return;
    __shared__ int s_w[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool acc = false; float best = FLT_MAX; int idx = 0; float px = 0.f, py = 0.f, pz = 0.f;
    if (i < ns) {
        transform_point(st->T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
        resolve_nn(i, ns_pad, nsplit, pd2, pchunk, direct, tx, ty, tz, px, py, pz, best, idx);
        acc = best <= tau_accept;
    }
    const unsigned long long m = __ballot(acc);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    if (!acc) return;
    int pos = off[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += s_w[w];
    ref_record<MODE>(px, py, pz, best, idx, tgt, tgt_normals, rec[2 * (size_t)pos], rec[2 * (size_t)pos + 1]);
}

// lane's running sum += the entries [0, m) of its LDS row, in order (m a multiple of 4): REF_CHAIN_G x 16 bytes of LDS reads, then
// 4 x REF_CHAIN_G dependent adds with the waits counted down (the compiler's schedule, checked in the ISA).  Reading one group
// AHEAD of the adds (two register groups) was measured slower at every group size (173 us per fold at 200k points -> 237-325).
#ifndef REF_CHAIN_G
#define REF_CHAIN_G 8
#endif
__device__ __forceinline__ float ref_chain(float s, const float* __restrict__ row, int m) {
    constexpr int G = REF_CHAIN_G;
    const float4* __restrict__ r4 = reinterpret_cast<const float4*>(row);
    int q = 0;
    for (; q + G <= m / 4; q += G) {
        float4 a[G];
#pragma unroll
        for (int j = 0; j < G; ++j) a[j] = r4[q + j];
#pragma unroll
        for (int j = 0; j < G; ++j) { s += a[j].x; s += a[j].y; s += a[j].z; s += a[j].w; }
    }
    for (; q < m / 4; ++q) { const float4 a = r4[q]; s += a.x; s += a.y; s += a.z; s += a.w; }
    return s;
}

// the per-accumulator terms of one record into column `col` of an LDS tile (rows[k][col]); PASS 1 (point-to-point): centred products
template <int MODE, int PASS>
__device__ __forceinline__ void ref_expand(float (*rows)[REF_LD], int col, const float4 a, const float4 b, bool live, const float* __restrict__ means) {
    if (MODE == 0) {
        const float J[6] = {a.y, a.z, a.w, b.x, b.y, b.z};
        rows[0][col] = a.x;
        int k = 1;
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = u; v < 6; ++v) rows[k++][col] = J[u] * J[v];       // J[v] * J[u] is the same float: ATA stays symmetric bit for bit
#pragma unroll
        for (int u = 0; u < 6; ++u) rows[k++][col] = J[u] * b.w;
    } else if (PASS == 0) {
        rows[0][col] = a.x; rows[1][col] = a.y; rows[2][col] = a.z; rows[3][col] = a.w; rows[4][col] = b.x; rows[5][col] = b.y; rows[6][col] = b.z;
    } else {
        const float P[3] = {a.y - means[0], a.z - means[1], a.w - means[2]}, Q[3] = {b.x - means[3], b.y - means[4], b.z - means[5]};
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) rows[u * 3 + v][col] = live ? P[u] * Q[v] : 0.f;      // registration.cpp:385 (a padding slot adds +0)
    }
}

template <int MODE, int PASS>
__device__ __forceinline__ float ref_fold_pass(const float4* __restrict__ rec, int n_corr, float (*buf)[REF_NR_PLANE][REF_LD], const float* __restrict__ means) {
    constexpr int NSUM = MODE == 0 ? REF_NR_PLANE : (PASS == 0 ? 7 : 9);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool loader = wave >= 1;
    const int slot = (int)threadIdx.x - 64;                   // a loader lane's record slot inside a tile
    const int ntiles = (n_corr + REF_TILE - 1) / REF_TILE;
    float ring[REF_RING][8];                                   // a loader lane's records in flight (compile-time indices only)
    float s = 0.f;
#define TDV_REF_ISSUE(X, D) do { const long long pos__ = (long long)(X) * REF_TILE + slot;                                                   \
        float4 a__ = make_float4(0.f, 0.f, 0.f, 0.f), b__ = a__;           /* zeros past the end: their terms are +0 */                       \
        if ((X) < ntiles && pos__ < n_corr) { a__ = rec[2 * pos__]; b__ = rec[2 * pos__ + 1]; }                                               \
        ring[D][0] = a__.x; ring[D][1] = a__.y; ring[D][2] = a__.z; ring[D][3] = a__.w; ring[D][4] = b__.x; ring[D][5] = b__.y; ring[D][6] = b__.z; ring[D][7] = b__.w; } while (0)
#define TDV_REF_EXPAND(X, D) do { if ((X) < ntiles) ref_expand<MODE, PASS>(buf[(X) & 1], slot, make_float4(ring[D][0], ring[D][1], ring[D][2], ring[D][3]),   \
        make_float4(ring[D][4], ring[D][5], ring[D][6], ring[D][7]), (long long)(X) * REF_TILE + slot < n_corr, means); } while (0)
    if (loader) {
        TDV_REF_ISSUE(0, 0); TDV_REF_ISSUE(1, 1); TDV_REF_ISSUE(2, 2);
        TDV_REF_EXPAND(0, 0);
        TDV_REF_ISSUE(3, 0);
    }
    __syncthreads();
    // period x: loaders expand tile x + 1 out of ring[(x + 1) % 3] and refill that stage with tile x + 4; wave 0 adds tile x.
    // Unrolled by the ring's depth so that every register stage is a compile-time index.
    static_assert(REF_RING == 3, "the period loop below is written for three stages");
    for (int t = 0; t < ntiles; t += REF_RING) {
        if (loader) { TDV_REF_EXPAND(t + 1, 1); TDV_REF_ISSUE(t + 4, 1); }
        else if (wave == 0 && lane < NSUM && t < ntiles) s = ref_chain(s, buf[t & 1][lane], (min(REF_TILE, n_corr - t * REF_TILE) + 3) & ~3);
        __syncthreads();
        if (loader) { TDV_REF_EXPAND(t + 2, 2); TDV_REF_ISSUE(t + 5, 2); }
        else if (wave == 0 && lane < NSUM && t + 1 < ntiles) s = ref_chain(s, buf[(t + 1) & 1][lane], (min(REF_TILE, n_corr - (t + 1) * REF_TILE) + 3) & ~3);
        __syncthreads();
        if (loader) { TDV_REF_EXPAND(t + 3, 0); TDV_REF_ISSUE(t + 6, 0); }
        else if (wave == 0 && lane < NSUM && t + 2 < ntiles) s = ref_chain(s, buf[(t + 2) & 1][lane], (min(REF_TILE, n_corr - (t + 2) * REF_TILE) + 3) & ~3);
        __syncthreads();
    }
#undef TDV_REF_ISSUE
#undef TDV_REF_EXPAND
    return s;
}

template <int MODE>
__global__ __launch_bounds__(64 + REF_TILE)
void k_icp_fold_ref(const float4* __restrict__ rec, const int* __restrict__ d_total, int ns, IcpState* st, int fixed_iterations) {
    if (st->done) return;
    __shared__ __attribute__((aligned(16))) float buf[2][REF_NR_PLANE][REF_LD];      // (point-to-point uses 9 of the 28 rows)
    __shared__ double tot[ACC_NV];
    __shared__ float means[6];
    __shared__ float solve_ws[56];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_corr = *d_total;
    if (threadIdx.x < ACC_NV) tot[threadIdx.x] = 0.0;
    __syncthreads();
    float s = ref_fold_pass<MODE, 0>(rec, n_corr, buf, means);
    if (wave == 0) {
        if (MODE == 0) { if (lane < REF_NR_PLANE) tot[1 + lane] = (double)s; }
        else if (lane == 0) tot[1] = (double)s;
        else if (lane < 7) means[lane - 1] = s / static_cast<float>(n_corr);          // registration.cpp:380-381 (n_corr < 3: unused below)
    }
    __syncthreads();
    if (MODE == 1) {
        s = ref_fold_pass<MODE, 1>(rec, n_corr, buf, means);
        if (wave == 0 && lane < 9) tot[8 + lane] = (double)s;
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    tot[0] = (double)n_corr;
    if (MODE == 1) for (int a = 0; a < 6; ++a) tot[2 + a] = (double)means[a];
    icp_update<MODE, true>(tot, ns, st, fixed_iterations, st->iter, st->rmse, st->T, solve_ws);
}

// ---- the whole loop in ONE launch, for small problems (round 3) ----------------------------------------------------------
// A 400 x 400 instance (config C5's size) spent 13 iterations' worth of launches - two per iteration, each 9-12 us of pure
// latency - and a state read-back per burst: 140 us of an instance's 340 us of kernels.  Here one workgroup of 16 waves keeps
// the target in LDS and runs search, normal equations, solve, update and the stopping rule for every iteration itself, then
// stores the final state straight into pinned host memory.
//  * search: one lane per source point scans the targets in LDS in ascending order with strict < and the scan's expression
//    d2 = dx*dx + (dy*dy + dz*dz): the scan's answer.
//  * accumulation: exactly k_icp_accumulate<MODE, 1>'s tree - 256 consecutive points form a block whose four wave sums (DPP) are
//    added as (w0 + w1) + (w2 + w3) into a slab, slabs folded in the same pattern - so a call gives the same bits whichever path
//    its size selects.
constexpr int SM_MAX_N = 2048;           // sources and targets the one-launch loop takes
constexpr int SM_THREADS = 1024;         // lanes of its workgroup
constexpr long long SM_MAX_PAIRS_SINGLE = 1ll << 18;    // ... in a single call (tools/studies/icp_small_probe.py)
constexpr long long SM_MAX_PAIRS_BATCH = 1ll << 20;     // ... per problem of a batch
// A grid of several workgroups runs one problem each (the batch's small instances against the shared model): problem b takes the
// source points [src_off[b], src_off[b + 1]) of src0 and the states st_in[b] / st_out[b]; src_off == nullptr: one problem.
// 1,024 lanes and room for 2,048 x 2,048 points.
// args' arrays are laid out like src0.
template <int MODE, bool REF, bool ROBUST = false>   // REF: reference-order accumulation (see k_icp_fold_ref), tile by tile in LDS; ROBUST: loss
__global__ __launch_bounds__(SM_THREADS)
void k_icp_small(const float* __restrict__ src0, int ns0, const int* __restrict__ src_off, const float* __restrict__ tgt, const float* __restrict__ tgt_normals, int nt,
                 const IcpState* __restrict__ st_in0, float tau_accept, int max_iterations, int fixed_iterations, IcpLoss loss,
                 IcpState* __restrict__ st_out0, IcpState* __restrict__ st_host, IcpArgs<MODE> args) {
    static_assert(!(REF && ROBUST), "reference-order sums have no loss");
    static_assert(!(REF && MODE >= 3), "GICP and colored ICP take tree sums");
    const int prob = blockIdx.x;
    const float* __restrict__ src = src_off ? src0 + (size_t)src_off[prob] * 3 : src0;
    const int ns = src_off ? src_off[prob + 1] - src_off[prob] : ns0;
    const IcpState* __restrict__ st_in = st_in0 + prob;
    IcpState* __restrict__ st_out = st_out0 + prob;
    if (ns == 0) { if (threadIdx.x == 0) *st_out = *st_in; return; }   // (an instance without points: the caller ignores its state)
    __shared__ __attribute__((aligned(16))) float tx[SM_MAX_N], ty[SM_MAX_N], tz[SM_MAX_N];
    __shared__ float sbest[SM_MAX_N];
    __shared__ int sidx[SM_MAX_N];
    __shared__ double red[SM_THREADS / 64][ACC_NV];       // wave sums, four per virtual block
    __shared__ double slab[SM_MAX_N / 256][ACC_NV];
    __shared__ double fold[8][ACC_NV];
    __shared__ double tot[ACC_NV];
    __shared__ float solve_ws[56];
    __shared__ IcpState st;
    constexpr int NRR = MODE == 0 ? REF_NR_PLANE : REF_NR_POINT;
    __shared__ __attribute__((aligned(16))) float rrows[REF ? NRR : 1][REF_LD];
    __shared__ float rmeans[6];
    static_assert(!REF || SM_THREADS >= REF_TILE, "one point per thread and tile");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt4 = (nt + 3) / 4;                          // targets in chunks of four, the last one padded with +inf (lds_scan.hpp)
    lds_stage_targets(tgt, nt, tx, ty, tz, SM_THREADS);
    if (threadIdx.x == 0) st = *st_in;
    __syncthreads();
    constexpr int NV = acc_nv<MODE, ROBUST>();
    const int nblocks = (ns + 255) / 256;
    for (int it = 0; it < max_iterations; ++it) {
        float T[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k] = st.T[k];
        const int iter0 = st.iter; const float rmse0 = st.rmse;
        // (a) nearest target of every source point: one LANE per source, the targets read from LDS at a wave-uniform address
        // (a broadcast, no bank conflict) in ascending order with strict <: the scan's answer.  (One WAVE per source with a
        // cross-lane (d2, index) minimum at the end was 3x slower at 400 x 400: six dependent shuffle rounds per source.)
        for (int i = threadIdx.x; i < ns; i += SM_THREADS) {
            float px, py, pz;
            transform_point(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
            lds_nearest(px, py, pz, tx, ty, tz, nt4, sbest[i], sidx[i]);     // the scan kernel's two-level argmin (lds_scan.hpp)
        }
        __syncthreads();
        if constexpr (REF) {
            // (b') the reference's sums: tiles of REF_TILE points - every thread expands its point's record into the per-accumulator term
            // rows in LDS (k_icp_fold_ref's ref_expand; a rejected point's terms are +0: s + 0 == s), lane k of wave 0 adds row k in
            // index order, the chain continuing from tile to tile
            int n_acc = 0;
            constexpr int NPASS = MODE == 0 ? 1 : 2;
            for (int pass = 0; pass < NPASS; ++pass) {
                const int nsum = MODE == 0 ? REF_NR_PLANE : (pass == 0 ? 7 : 9);
                float s = 0.f;
                for (int base = 0; base < ns; base += REF_TILE) {
                    bool acc = false;
                    if (threadIdx.x < REF_TILE) {
                        const int i = base + threadIdx.x;
                        float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
                        if (i < ns) {
                            const float best = sbest[i];
                            acc = best <= tau_accept;
                            if (acc) {
                                float px, py, pz;
                                transform_point(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
                                ref_record<MODE>(px, py, pz, best, sidx[i], tgt, tgt_normals, ra, rb);
                            }
                        }
                        if (pass == 0) ref_expand<MODE, 0>(rrows, threadIdx.x, ra, rb, acc, rmeans);
                        else ref_expand<MODE, 1>(rrows, threadIdx.x, ra, rb, acc, rmeans);
                    }
                    const int c = __syncthreads_count(acc);
                    if (pass == 0) n_acc += c;
                    if (wave == 0 && lane < nsum) s = ref_chain(s, rrows[lane], (min(REF_TILE, ns - base) + 3) & ~3);
                    __syncthreads();
                }
                if (wave == 0 && lane < nsum) {
                    if (MODE == 0) tot[1 + lane] = (double)s;
                    else if (pass == 0) { if (lane == 0) tot[1] = (double)s; else rmeans[lane - 1] = s / static_cast<float>(n_acc); }
                    else tot[8 + lane] = (double)s;
                }
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                tot[0] = (double)n_acc;
                if (MODE == 1) for (int a = 0; a < 6; ++a) tot[2 + a] = (double)rmeans[a];
                icp_update<MODE, true>(tot, ns, &st, fixed_iterations, iter0, rmse0, T, solve_ws);
            }
            __syncthreads();
            if (st.done) break;
            continue;
        }
        // (b) slabs: virtual block B = points [256 B, 256 B + 256), one point per lane
        for (int B0 = 0; B0 < nblocks; B0 += SM_THREADS / 256) {
            const int B = B0 + (threadIdx.x >> 8);
            const int i = B * 256 + (threadIdx.x & 255);
            double v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = 0.0;
            if (B < nblocks && i < ns) {
                float px, py, pz;
                transform_point(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
                const float best = sbest[i]; const int idx = sidx[i];
                if (best <= tau_accept) {
                    const CorrPt<MODE> X = corr_pt<MODE, 4>(args, T, (src_off ? (size_t)src_off[prob] : 0) + i);
                    acc_terms<MODE, ROBUST>(px, py, pz, best, idx, tgt, tgt_normals, loss, X, [&v](int k, double t) { v[k] = t; });
                }
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const double s = wave_sum_lane63(v[k]);
                if (lane == 63) red[wave][k] = s;
            }
            __syncthreads();
            if (B < nblocks && (threadIdx.x & 255) < ACC_NV) {
                const int k = threadIdx.x & 255, w0 = (threadIdx.x >> 8) * 4;
                slab[B][k] = k < NV ? (red[w0][k] + red[w0 + 1][k]) + (red[w0 + 2][k] + red[w0 + 3][k]) : 0.0;
            }
            __syncthreads();
        }
        // (c) fold, in k_icp_accumulate's pattern (group g of 32 threads takes slabs g, g + 8, ...: here at most one each)
        if (threadIdx.x < 256) {
            const int vv = threadIdx.x & 31, g = threadIdx.x >> 5;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            if (g < nblocks) s0 += slab[g][vv];
            fold[g][vv] = (s0 + s1) + (s2 + s3);
        }
        __syncthreads();
        if (threadIdx.x < ACC_NV) {
            const int vv = threadIdx.x;
            tot[vv] = ((fold[0][vv] + fold[1][vv]) + (fold[2][vv] + fold[3][vv])) + ((fold[4][vv] + fold[5][vv]) + (fold[6][vv] + fold[7][vv]));
        }
        __syncthreads();
        // (d) solve, update, stopping rule
        if (threadIdx.x == 0) icp_update<MODE, false, ROBUST>(tot, ns, &st, fixed_iterations, iter0, rmse0, T, solve_ws);
        __syncthreads();
        if (st.done) break;
    }
    if (threadIdx.x == 0) {
        *st_out = st;
        if (st_host) { *st_host = st; __threadfence_system(); }
    }
}

namespace {

struct NnPlan {
    int ns_pad, nt_pad, n_chunks, blocks_x, nsplit, chunks_per_split, acc_blocks, acc_ppt;
};

NnPlan make_plan(int ns, int nt) {
    NnPlan p;
    p.ns_pad = (int)align_up((size_t)ns, NN_SRC_PER_BLOCK);
    p.nt_pad = (int)align_up((size_t)nt, NN_CH);
    p.n_chunks = p.nt_pad / NN_CH;
    p.blocks_x = p.ns_pad / NN_SRC_PER_BLOCK;
    // aim for ~12k workgroups (48 per CU: measured best at 200k x 200k) but keep >= 16 chunks (256 targets) per split
    int want = (NN_WG_TARGET + p.blocks_x - 1) / std::max(p.blocks_x, 1);     // (ns = 0: an empty instance of a batch)
    int max_split = std::max(1, p.n_chunks / 16);
    p.nsplit = std::max(1, std::min(std::min(want, max_split), 64));
    p.chunks_per_split = (p.n_chunks + p.nsplit - 1) / p.nsplit;
    p.nsplit = (p.n_chunks + p.chunks_per_split - 1) / p.chunks_per_split;
    static const int ppt_env = study_env("TDV_ICP_PPT") ? atoi(study_env("TDV_ICP_PPT")) : 0;
    // only 1, 2, 4 and 8 points per thread are instantiated (ppt_dispatch below); anything else would size the grid for a kernel that is never launched
    p.acc_ppt = (kStudyBuild && (ppt_env == 1 || ppt_env == 2 || ppt_env == 4 || ppt_env == 8)) ? ppt_env : 4;   // 4: make_plan's default; the brute-force path uses 1
    p.acc_blocks = (ns + 256 * p.acc_ppt - 1) / (256 * p.acc_ppt);
    return p;
}

// whether the one-launch loop (k_icp_small) takes ns x nt points, at most max_pairs pairs
bool small_fits(int ns, int nt, long long max_pairs) {
    const bool off = getenv("TDV_ICP_SMALL") && atoi(getenv("TDV_ICP_SMALL")) == 0;   // A/B knob (read per call: the tests switch it)
    return !off && ns <= SM_MAX_N && nt <= SM_MAX_N && (long long)ns * nt <= max_pairs;
}

// The path of one problem of ns source x nt target points at threshold thr on ctx.  icp_run_dev takes it, and icp_batch_run_dev
// follows it per instance: that is what gives an instance the single call's bits.
struct IcpPlan {
    int search;     // TDV_ICP_SEARCH_GRID / _PRUNED / _BRUTE, what ctx->last_icp_search reports
    bool direct;    // pruned walk or grid: one search result per source, the final (d2, original target index)
    bool small;     // the whole loop in one launch (k_icp_small)
    CellGrid cg;    // the target's hash grid, searched when cg.usable
    NnPlan p;       // the scan's shape and the accumulation's acc_ppt / acc_blocks
    bool one_launch;   // search and sums of an iteration in one kernel (k_icp_iterate), what ctx->last_icp_launches reports
    bool probe_cache;  // the grid search keeps each point's list heads between iterations (grid_nearest<1>)
};

// Source counts between which TDV_ICP_LAUNCHES_AUTO takes k_icp_iterate.  Measured (tools/studies/icp_grid_scaling.py --forms two,one,
// a 200k-point target, us per iteration two launches / one, profiles/r19/icp_one_launch.md): 100k 32.0 / 35.1, 125k 31.8 / 34.8,
// 150k 36.7 / 35.3, 175k 37.7 / 35.2, 200k 41.5 / 36.3, 225k 43.0 / 36.3, 250k 43.8 / 36.3, 262,144 44.1 / 37.3, 263,169 46.9 / 56.6,
// 300k 49.8 / 61.0, 400k 61.8 / 63.6.  The kernel lasts about as long as ONE workgroup's 1,024 points take their CU (25.7 us for 13
// workgroups), so it wins once the two launches' per-point part has outgrown that, and loses again from the 257th workgroup on: the
// part has 256 CUs, and a CU that gets a second workgroup runs twice as long.
constexpr int ONE_LAUNCH_MIN_SOURCES = 150000;
constexpr int ONE_LAUNCH_MAX_SOURCES = 262144;      // 256 workgroups
// With the probe cache (grid_nearest<1>) the rule stays.  Over 100 iterations the cached kernel beats the cached and the uncached two
// launches from 50,000 sources on (75k 20.8 / 21.7 / 30.4 us, 100k 21.6 / 22.6 / 31.5, 400k 40.1 / 41.3 / 61.2), but a call of four
// iterations from a near start - the pipeline's - is a tie or loses 1 to 3 % against the uncached two launches at 75k to 125k, and at 300k
// loses 12 %; inside the range the cached kernel is never behind (profiles/r22/icp_probe_cache.md, sections 5 and 6).
//
// Iterations a call must be allowed for TDV_ICP_PROBE_CACHE_AUTO to take the cache: the first iteration only fills it (a memset of the
// keys, three more loads and a 40-byte store per point), every later one gains.  Measured per call at 200k x 200k against the uncached
// call: 2 iterations +1 to +4 us, 3 iterations -2 to +3 us, 4 iterations -2 to -8 us, 8 iterations -30 us.
constexpr int PROBE_CACHE_MIN_ITERATIONS = 4;

// Search: brute force for small problems (the two Morton sorts cost more than they save), the exact pruned walk for large ones, the
// hash grid (tgt_grid if it was built for this nt and thr, else built here) on request or by size like the walk, used when its build
// says the cells are small enough.  All give the same correspondences bit for bit.
// obj: the single call's objective and max_iterations its iteration limit; without them (a batch) the plan keeps two launches per
// iteration and the uncached search.
int icp_plan(tdv_ctx* ctx, const float* d_tgt, int ns, int nt, float thr, const CellGrid* tgt_grid, IcpPlan& pl,
             const IcpObjective* obj = nullptr, int max_iterations = 0) {
    const int mode = ctx->icp_search;
    const float tau = tau_le(thr);
    bool pruned = tau < FLT_MAX &&      // (unbounded threshold: keep the scan's handling of overflowing distances)
                  (mode == TDV_ICP_SEARCH_PRUNED || (mode == TDV_ICP_SEARCH_AUTO && nt >= PRUNED_MIN_TARGETS && (double)ns * (double)nt >= PRUNED_MIN_PAIRS));
    pl.cg = CellGrid{};
    if (tau < FLT_MAX && (mode == TDV_ICP_SEARCH_GRID || (mode == TDV_ICP_SEARCH_AUTO && pruned))) {
        if (tgt_grid && tgt_grid->n == nt && tgt_grid->thr == thr) pl.cg = *tgt_grid;
        else TDV_TRY(cell_grid_build(ctx, d_tgt, nt, thr, &pl.cg));
        pruned = true;              // the grid's results arrive in the walk's format; an unusable grid falls back to the walk
    }
    pl.search = pl.cg.usable ? TDV_ICP_SEARCH_GRID : (pruned ? TDV_ICP_SEARCH_PRUNED : TDV_ICP_SEARCH_BRUTE);
    pl.direct = pruned;
    // (one workgroup walks all ns x nt pairs of an iteration: measured per iteration 22 us at 400 x 398 against 28 us for the two
    //  launches, but 65 us at 1,000 x 1,000 and 237 us at 2,000 x 2,000 against 25-27: a single problem only takes this path while the
    //  pair count is small; a BATCH of such problems is another matter - there the grid is the parallelism, icp_small_batch_dev)
    pl.small = !pruned && small_fits(ns, nt, SM_MAX_PAIRS_SINGLE);
    pl.p = make_plan(ns, nt);
    if (pruned) pl.p.nsplit = 1;
    else if (pl.small || !study_env("TDV_ICP_PPT")) { pl.p.acc_ppt = 1; pl.p.acc_blocks = (ns + 255) / 256; }   // (k_icp_small's tree is the 1's)
    // one launch per iteration: the hash grid, tree sums in slabs of 4 x 256 points, point-to-plane or point-to-point
    const bool can_one = obj && pl.cg.usable && pl.p.acc_ppt == ACC_GROUP && ctx->icp_accumulate != TDV_ICP_ACCUMULATE_REFERENCE &&
                         (obj->kind == ICP_POINT_TO_PLANE || obj->kind == ICP_POINT_TO_POINT);
    pl.one_launch = can_one && (ctx->icp_launches == TDV_ICP_LAUNCHES_ONE ||
                                (ctx->icp_launches == TDV_ICP_LAUNCHES_AUTO && ns >= ONE_LAUNCH_MIN_SOURCES && ns <= ONE_LAUNCH_MAX_SOURCES));
    // the probe cache: a single call's grid search (a batch's _multi kernels and register_batch's lanes keep the uncached search).  AUTO
    // takes it with the one-launch iteration in a call long enough to gain from it (the two launches gain only from about eight
    // iterations on: at 200k sources a call of four is 13 us slower with it); ON in either form from two iterations on (one iteration
    // could only fill it).
    pl.probe_cache = obj && pl.cg.usable &&
                     ((ctx->icp_probe_cache == TDV_ICP_PROBE_CACHE_ON && max_iterations >= 2) ||
                      (ctx->icp_probe_cache == TDV_ICP_PROBE_CACHE_AUTO && pl.one_launch && max_iterations >= PROBE_CACHE_MIN_ITERATIONS));
    return TDV_OK;                                    // measured: 50k x 10k brute 7.6k vs 6.4k iters/s with 1 point per thread
}

struct IcpBuffers {
    float *tx, *ty, *tz, *pd2; int* pchunk; double* slabs; IcpState* st; unsigned* ticket;
};

int alloc_buffers(tdv_ctx* ctx, const NnPlan& p, IcpBuffers& b) {
    float* soa = nullptr;
    TDV_TRY(ws_alloc(ctx, (size_t)3 * p.nt_pad, &soa));
    b.tx = soa; b.ty = soa + p.nt_pad; b.tz = soa + 2 * (size_t)p.nt_pad;
    TDV_TRY(ws_alloc(ctx, (size_t)p.nsplit * p.ns_pad, &b.pd2));
    TDV_TRY(ws_alloc(ctx, (size_t)p.nsplit * p.ns_pad, &b.pchunk));
    TDV_TRY(ws_alloc(ctx, (size_t)p.acc_blocks * ACC_NV, &b.slabs));
    TDV_TRY(ws_alloc(ctx, 1, &b.st));
    b.ticket = ctx->scan_ticket + 1;     // the ctx's persistent ticket words (zero between launches: the last workgroup resets it)
    return TDV_OK;
}

// n states before the first iteration: start pose T0s + 16 b (host, column-major), the call's convergence criteria, everything else 0
void init_states(IcpState* h, const float* T0s, int n, float rel_fitness = INFINITY, float rel_rmse = 1e-6f) {
    std::memset(h, 0, (size_t)n * sizeof(IcpState));
    for (int b = 0; b < n; ++b) {
        std::memcpy(h[b].T, T0s + 16 * (size_t)b, 64); std::memcpy(h[b].res_T, T0s + 16 * (size_t)b, 64);
        h[b].rel_fitness = rel_fitness; h[b].rel_rmse = rel_rmse;
    }
}

// the result before any iteration: registration.cpp:309-311
void result_defaults(const float* T0, tdv_icp_result& out) {
    std::memcpy(out.T, T0, 64);
    out.fitness = 0.f; out.rmse = 0.f; out.iterations = 0; out.n_corr = 0;
}

// the result of a final state
void state_result(const IcpState& h, tdv_icp_result& out) {
    std::memcpy(out.T, h.res_T, 64);
    out.fitness = h.fitness; out.rmse = h.rmse; out.iterations = h.applied; out.n_corr = h.last_n_corr_applied;
}

// the ctx's loss as the kernels take it, and whether it is a robust one (the ROBUST instantiations)
IcpLoss ctx_loss(const tdv_ctx* ctx) { return IcpLoss{ctx->icp_loss, ctx->icp_loss_scale}; }
// the kernels' `fixed_iterations` argument (ICP_RUN_*) of a call
int run_flags(int fixed_iterations, const IcpObjective& obj) {
    const bool defaults = obj.rel_fitness == INFINITY && obj.rel_rmse == 1e-6f;
    return (fixed_iterations ? ICP_RUN_FIXED : 0) | (defaults ? 0 : ICP_RUN_CRITERIA);
}
bool ctx_robust(const tdv_ctx* ctx) { return ctx->icp_loss != TDV_ICP_LOSS_L2; }

// The kernels' extra arguments from an objective of kind MODE
template <int MODE> IcpArgs<MODE> kernel_args(const IcpObjective& o) {
    if constexpr (MODE == ICP_GICP) return {o.src_normals, o.c};
    else if constexpr (MODE == ICP_COLORED) return {o.src_rgb, o.tgt_color, o.lg, o.lc};
    else return {};
}

// The one place that turns an objective's kind and the ctx's loss and accumulation into template arguments: calls f(MODE, ROBUST, REF)
// with integral constants, for the combinations that are instantiated - reference-order sums exist for point-to-plane and
// point-to-point and take no loss (the entry points refuse the rest: icp_objective_check).  Point-to-plane without target normals is
// point-to-point.
template <class F>
void icp_dispatch(const tdv_ctx* ctx, const IcpObjective& obj, const float* d_tgt_normals, const F& f) {
    const IcpKind kind = (obj.kind == ICP_POINT_TO_PLANE && !d_tgt_normals) ? ICP_POINT_TO_POINT : obj.kind;
    const bool robust = ctx_robust(ctx), ref = ctx->icp_accumulate == TDV_ICP_ACCUMULATE_REFERENCE;
    const auto mode = [&](auto M) {
        if constexpr (decltype(M)::value < ICP_GICP) { if (ref) return f(M, std::false_type{}, std::true_type{}); }
        return robust ? f(M, std::true_type{}, std::false_type{}) : f(M, std::false_type{}, std::false_type{});
    };
    switch (kind) {
    case ICP_POINT_TO_PLANE: return mode(std::integral_constant<int, ICP_POINT_TO_PLANE>{});
    case ICP_POINT_TO_POINT: return mode(std::integral_constant<int, ICP_POINT_TO_POINT>{});
    case ICP_GICP: return mode(std::integral_constant<int, ICP_GICP>{});
    case ICP_COLORED: return mode(std::integral_constant<int, ICP_COLORED>{});
    }
}

// ... and k_icp_accumulate's points per thread: f(ACC_PPT) for make_plan's values (2 and 8 points per thread: study build)
template <class F>
void ppt_dispatch(int ppt, const F& f) {
#ifdef TDV_STUDY
    if (ppt == 8) return f(std::integral_constant<int, 8>{});
    if (ppt == 2) return f(std::integral_constant<int, 2>{});
#endif
    if (ppt == 4) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 1>{});
}

// k_icp_small over n_prob workgroups (src_off == nullptr: one problem of ns points) for obj, with the ctx's accumulation and loss
void launch_icp_small(tdv_ctx* ctx, int n_prob, const float* d_src, int ns, const int* d_src_off, const float* d_tgt, const float* d_tgt_normals, int nt,
                      const IcpObjective& obj, const IcpState* st_in, float tau, int max_iterations, int fixed_iterations, IcpState* st_out, IcpState* st_host) {
    icp_dispatch(ctx, obj, d_tgt_normals, [&](auto M, auto R, auto REF) {
        constexpr int MODE = decltype(M)::value;
        k_icp_small<MODE, decltype(REF)::value, decltype(R)::value><<<n_prob, SM_THREADS, 0, ctx->stream>>>(
            d_src, ns, d_src_off, d_tgt, MODE == ICP_POINT_TO_POINT ? nullptr : d_tgt_normals, nt, st_in, tau, max_iterations, run_flags(fixed_iterations, obj), ctx_loss(ctx),
            st_out, st_host, kernel_args<MODE>(obj));
    });
}

// Iterations are enqueued in bursts between two looks at the n states d_st (read back into the pinned h[0 .. n)); once a state is done
// the remaining launches of a burst return at once, and the loop ends when all are.  The reference's stopping rule fires after 3-4
// iterations in the pipeline's setting (0.4-voxel threshold from a RANSAC start), so the first burst is short; fixed-iteration runs
// take long bursts.  iteration() enqueues one iteration.
template <class F>
int run_bursts(tdv_ctx* ctx, IcpState* h, const IcpState* d_st, int n, int max_iterations, int fixed_iterations, const F& iteration) {
    for (int it = 0; it < max_iterations;) {
        const int burst = std::min(fixed_iterations ? 32 : (it == 0 ? 4 : 8), max_iterations - it);
        for (int k = 0; k < burst; ++k) iteration();
        TDV_CHECK_LAUNCH(ctx);
        it += burst;
        TDV_HIP(ctx, hipMemcpyAsync(h, d_st, (size_t)n * sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
        TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool all_done = true;
        for (int b = 0; b < n && all_done; ++b) all_done = h[b].done != 0;
        if (all_done) break;
    }
    return TDV_OK;
}

}  // namespace

int cell_grid_build(tdv_ctx* ctx, const float* d_tgt, int nt, float thr, CellGrid* g) {
    if (!ctx || !d_tgt || !g || nt <= 0) return TDV_ERR_BAD_ARG;
    *g = CellGrid{};
    g->thr = thr; g->n = nt;
    const float cell = GRID_CELL_FACTOR * thr;
    const float inv_cell = 1.0f / cell;
    if (!(thr > 0.f) || !(cell <= FLT_MAX) || !(inv_cell > 0.f) || !(inv_cell <= FLT_MAX)) return TDV_OK;   // usable = 0
    size_t size = 1024; int log2 = 10;
    while (size < (size_t)GRID_SLOTS_PER_POINT_X4 * (size_t)nt / 4) { size <<= 1; ++log2; }
    GridEntry* table; float4* node; int* flags;
    TDV_TRY(ws_alloc(ctx, size + GRID_PAD, &table));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &node));
    TDV_TRY(ws_alloc(ctx, 2, &flags));
    hipStream_t s = ctx->stream;
    TDV_HIP(ctx, hipMemsetAsync(table, 0xff, (size + GRID_PAD) * sizeof(GridEntry), s));      // key = empty, head = -1
    TDV_HIP(ctx, hipMemsetAsync(flags, 0, 8, s));
    k_grid_insert<<<(nt + 255) / 256, 256, 0, s>>>(d_tgt, nt, inv_cell, table, node, (unsigned)(size - 1), 64 - log2, flags);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(pin_reserve(ctx, 64));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, flags, 8, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    const int* h = reinterpret_cast<const int*>(ctx->pin);
    const int bad = h[0], cells = h[1];
    g->table = table; g->node = node; g->mask = (unsigned)(size - 1); g->shift = 64 - log2; g->inv_cell = inv_cell;
    static const int max_per_cell = study_env("TDV_GRID_MAX_PER_CELL") ? atoi(study_env("TDV_GRID_MAX_PER_CELL")) : GRID_MAX_PER_CELL;   // tuning knob
    g->usable = (!bad && cells > 0 && (long long)nt <= (long long)max_per_cell * cells) ? 1 : 0;
    return TDV_OK;
}

int icp_run_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                const float* T0, float thr, int max_iterations, IcpObjective obj, int fixed_iterations,
                tdv_icp_result* out, const SortedCloud* tgt_sorted, const CellGrid* tgt_grid) {
    if (!ctx || !d_src || !d_tgt || !T0 || !out || ns < 0 || nt < 0 || max_iterations < 0) return TDV_ERR_BAD_ARG;
    const bool ref_acc = ctx->icp_accumulate == TDV_ICP_ACCUMULATE_REFERENCE;
    if (obj.kind >= ICP_GICP && (!d_tgt_normals || ref_acc || !(obj.kind == ICP_GICP ? obj.src_normals : obj.src_rgb) ||
                                 (obj.kind == ICP_COLORED && !obj.tgt_color)))
        return TDV_ERR_BAD_ARG;                                                              // (icp_objective_check's)
    TDV_HIP(ctx, hipSetDevice(ctx->device));
    result_defaults(T0, *out);
    if (max_iterations == 0) return TDV_OK;
    if (ns == 0 || nt == 0) return TDV_OK;  // n_corr == 0 < 3 -> break at the first iteration
    const float tau = tau_le(thr);
    IcpPlan pl;
    TDV_TRY(icp_plan(ctx, d_tgt, ns, nt, thr, tgt_grid, pl, &obj, max_iterations));
    ctx->last_icp_search = pl.search;
    ctx->last_icp_launches = pl.one_launch ? TDV_ICP_LAUNCHES_ONE : TDV_ICP_LAUNCHES_TWO;
    ctx->last_icp_probe_misses = -1;
    const NnPlan& p = pl.p;
    const CellGrid& cg = pl.cg;
    const IcpLoss loss = ctx_loss(ctx);
    TDV_TRY(pin_reserve(ctx, 2 * sizeof(IcpState)));
    IcpState* h = reinterpret_cast<IcpState*>(ctx->pin);
    init_states(h, T0, 1, obj.rel_fitness, obj.rel_rmse);
    hipStream_t s = ctx->stream;
    // small problems: the whole loop in one launch (k_icp_small), same bits as the launches below
    if (pl.small) {
        IcpState* d_st;
        TDV_TRY(ws_alloc(ctx, 2, &d_st));
        IcpState* h_res = h + 1;                          // the kernel stores its final state here itself (pinned memory: no copy kernel)
        h_res->iter = -1;
        TDV_HIP(ctx, hipMemcpyAsync(d_st, h, sizeof(IcpState), hipMemcpyHostToDevice, s));
        {
            ScopedTimer tm(ctx, TDV_TIMER_ICP_NN);
            launch_icp_small(ctx, 1, d_src, ns, nullptr, d_tgt, d_tgt_normals, nt, obj, d_st, tau, max_iterations, fixed_iterations, d_st + 1, h_res);
        }
        TDV_CHECK_LAUNCH(ctx);
        TDV_HIP(ctx, hipStreamSynchronize(s));
        if (h_res->iter < 0) { snprintf(ctx->err, sizeof(ctx->err), "icp: the result did not reach the host"); return TDV_ERR_INTERNAL; }
        state_result(*h_res, *out);
        return TDV_OK;
    }
    IcpBuffers b;
    TDV_TRY(alloc_buffers(ctx, p, b));
    TDV_HIP(ctx, hipMemcpyAsync(b.st, h, sizeof(IcpState), hipMemcpyHostToDevice, s));
    SortedCloud st{};
    if (cg.usable) {
        // nothing to prepare
    } else if (pl.direct) {
        if (tgt_sorted && tgt_sorted->n == nt) st = *tgt_sorted;   // the batch orders the shared model once
        else TDV_TRY(spatial_sort_cloud(ctx, d_tgt, nt, st));
    } else {
        k_aos_to_soa_pad<<<(p.nt_pad + 255) / 256, 256, 0, s>>>(d_tgt, nt, p.nt_pad, INFINITY, b.tx, b.ty, b.tz);
    }
    TDV_CHECK_LAUNCH(ctx);
    const int direct = pl.direct ? 1 : 0;
    // reference-order accumulation: dense records of the accepted correspondences + one-workgroup ordered fold instead of k_icp_accumulate
    const int ref_blocks = (ns + 255) / 256;
    float4* ref_rec = nullptr; int *ref_cnt = nullptr, *ref_off = nullptr;
    if (ref_acc) {
        TDV_TRY(ws_alloc(ctx, (size_t)2 * ns, &ref_rec));
        TDV_TRY(ws_alloc(ctx, (size_t)ref_blocks, &ref_cnt));
        TDV_TRY(ws_alloc(ctx, (size_t)ref_blocks + 1, &ref_off));
    }
    const GridEntry* gtable = cg.usable ? reinterpret_cast<const GridEntry*>(cg.table) : nullptr;
    const float4* gnode = cg.usable ? reinterpret_cast<const float4*>(cg.node) : nullptr;
    const dim3 grid(p.blocks_x, p.nsplit);
    // the probe cache of this call: keys invalid before the first iteration, so no head of another table, call or arena is ever taken
    ProbeCache pc{};
    const bool cached = pl.probe_cache;
    if (cached) {
        TDV_TRY(ws_alloc(ctx, (size_t)ns, &pc.key));
        TDV_TRY(ws_alloc(ctx, (size_t)2 * ns, &pc.head));
        pc.misses = &b.st->probe_misses;
        TDV_HIP(ctx, hipMemsetAsync(pc.key, 0, (size_t)ns * sizeof(uint2), s));
    }
    // study build: TDV_ICP_PROBE_STUDY=heads / probe times the iteration without its probe loop resp. without its list walk (grid_nearest's
    // PROBE 2 and 3: not results, an upper bound on what the cache can save); the call's first iteration fills the cache for `heads`
    const char* probe_study = study_env("TDV_ICP_PROBE_STUDY");
    const int study_probe = !(cached && probe_study) ? 0 : !strcmp(probe_study, "heads") ? 2 : !strcmp(probe_study, "probe") ? 3 : 0;
    if (study_probe) TDV_HIP(ctx, hipMemsetAsync(pc.head, 0xff, (size_t)2 * ns * sizeof(uint4), s));      // (`heads` never compares: no head a lane did not store)
    int iteration_no = 0;
    (void)iteration_no;
    // f(PROBE) for this iteration's form of the grid search
    const auto probe_dispatch = [&](const auto& f) {
#ifdef TDV_STUDY
        if (study_probe && iteration_no > 0) return study_probe == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 3>{});
#endif
        return cached ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
    };
    const int run = run_flags(fixed_iterations, obj);
    TDV_TRY(run_bursts(ctx, h, b.st, 1, max_iterations, fixed_iterations, [&]() {
        if (pl.one_launch) {
            ScopedTimer tm(ctx, TDV_TIMER_ICP_NN);      // the whole iteration: one launch
            icp_dispatch(ctx, obj, d_tgt_normals, [&](auto M, auto R, auto) {
                constexpr int MODE = decltype(M)::value;
                if constexpr (MODE == ICP_POINT_TO_PLANE || MODE == ICP_POINT_TO_POINT)      // (icp_plan's rule)
                    probe_dispatch([&](auto P) {
                        k_icp_iterate<MODE, decltype(R)::value, decltype(P)::value><<<p.acc_blocks, IT_THREADS, 0, s>>>(
                            d_src, ns, MODE == ICP_POINT_TO_POINT ? nullptr : d_tgt_normals, gtable, gnode, cg.mask, cg.shift, cg.inv_cell, b.st, tau,
                            run, loss, b.slabs, b.ticket, pc);
                    });
            });
            ++iteration_no;
            return;
        }
        {
            ScopedTimer tm(ctx, TDV_TIMER_ICP_NN);
            if (gtable)
                probe_dispatch([&](auto P) {
                    k_icp_nn_grid<decltype(P)::value><<<(ns + 255) / 256, 256, 0, s>>>(d_src, ns, gtable, gnode, cg.mask, cg.shift, cg.inv_cell, b.st, tau,
                                                                                       b.pd2, b.pchunk, pc);
                });
            else if (pl.direct)
                k_icp_nn_pruned<<<(ns + PN_WAVES * PN_PTS - 1) / (PN_WAVES * PN_PTS), 64 * PN_WAVES, 0, s>>>(
                    d_src, ns, st, b.st, tau, b.pd2, b.pchunk);
            else
                k_icp_nn_scan<<<grid, NN_BLOCK, 0, s>>>(d_src, ns, p.ns_pad, b.tx, b.ty, b.tz, p.n_chunks,
                                                        p.chunks_per_split, b.st, b.pd2, b.pchunk);
        }
        icp_dispatch(ctx, obj, d_tgt_normals, [&](auto M, auto R, auto REF) {
            constexpr int MODE = decltype(M)::value;
            const float* nrm = MODE == ICP_POINT_TO_POINT ? nullptr : d_tgt_normals;
            if constexpr (decltype(REF)::value) {
                k_icp_flags<<<ref_blocks, 256, 0, s>>>(ns, p.ns_pad, p.nsplit, b.pd2, b.st, tau, ref_cnt);
                k_icp_scan_counts<<<1, 1024, 0, s>>>(ref_cnt, ref_blocks, b.st, ref_off);
                k_icp_rows<MODE><<<ref_blocks, 256, 0, s>>>(d_src, ns, p.ns_pad, d_tgt, nrm, b.tx, b.ty, b.tz, p.nsplit, b.pd2, b.pchunk, direct, b.st, tau, ref_off, ref_rec);
                k_icp_fold_ref<MODE><<<1, 64 + REF_TILE, 0, s>>>(ref_rec, ref_off + ref_blocks, ns, b.st, run);
            } else {
                ppt_dispatch(p.acc_ppt, [&](auto P) {
                    k_icp_accumulate<MODE, decltype(P)::value, decltype(R)::value><<<p.acc_blocks, 256, 0, s>>>(
                        d_src, ns, p.ns_pad, d_tgt, nrm, b.tx, b.ty, b.tz, p.nsplit, b.pd2, b.pchunk, direct, b.st, tau, run, loss, b.slabs, b.ticket,
                        nullptr, nullptr, nullptr, kernel_args<MODE>(obj));
                });
            }
        });
        ++iteration_no;
    }));
    if (cached) ctx->last_icp_probe_misses = h->probe_misses;
    state_result(*h, *out);
    return TDV_OK;
}

// whether icp_small_batch_dev takes problems of up to ns_max points against nt targets on this ctx (its kernel scans: no search but
// AUTO or BRUTE asks for anything else)
bool icp_small_batch_fits(const tdv_ctx* ctx, int ns_max, int nt) {
    return (ctx->icp_search == TDV_ICP_SEARCH_AUTO || ctx->icp_search == TDV_ICP_SEARCH_BRUTE) && small_fits(ns_max, nt, SM_MAX_PAIRS_BATCH);
}

// icp_run_dev for n_prob small problems against one target in ONE launch: problem b = source points [d_src_off[b], d_src_off[b+1])
// of d_src (each at most SM_MAX_N, as nt), start pose T0s[b] (host, column-major).  Results as icp_run_dev's, bit for bit (the same
// kernel).  One upload, one launch, one download.
int icp_small_batch_dev(tdv_ctx* ctx, const float* d_src, const int* d_src_off, int n_prob, const float* d_tgt, const float* d_tgt_normals, int nt,
                        const float* T0s, float thr, int max_iterations, IcpObjective obj, tdv_icp_result* out) {
    if (!ctx || !d_src || !d_src_off || !d_tgt || !T0s || !out || n_prob < 0 || nt <= 0 || nt > SM_MAX_N || max_iterations < 0) return TDV_ERR_BAD_ARG;
    if (n_prob == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    const float tau = tau_le(thr);
    IcpState* d_st;
    TDV_TRY(ws_alloc(ctx, (size_t)2 * n_prob, &d_st));
    TDV_TRY(pin_reserve(ctx, (size_t)n_prob * sizeof(IcpState)));
    IcpState* h = reinterpret_cast<IcpState*>(ctx->pin);
    init_states(h, T0s, n_prob, obj.rel_fitness, obj.rel_rmse);
    TDV_HIP(ctx, hipMemcpyAsync(d_st, h, (size_t)n_prob * sizeof(IcpState), hipMemcpyHostToDevice, s));
    if (max_iterations > 0) {
        ScopedTimer tm(ctx, TDV_TIMER_ICP_NN);
        // (A quarter-size shape - 256 lanes, more problems resident at once - was measured against this one on C5's 1,024 instances in
        // round 3: 1.59 ms against 1.33 ms.  The pass lasts as long as its slowest problem and a lone workgroup iterates faster with
        // 16 waves; the variant is gone, profiles/r3/history keeps the numbers.)
        launch_icp_small(ctx, n_prob, d_src, 0, d_src_off, d_tgt, d_tgt_normals, nt, obj, d_st, tau, max_iterations, 0, d_st + n_prob, nullptr);
        TDV_CHECK_LAUNCH(ctx);
        TDV_HIP(ctx, hipMemcpyAsync(h, d_st + n_prob, (size_t)n_prob * sizeof(IcpState), hipMemcpyDeviceToHost, s));
    }
    TDV_HIP(ctx, hipStreamSynchronize(s));
    ctx->last_icp_search = TDV_ICP_SEARCH_BRUTE;
    ctx->last_icp_launches = TDV_ICP_LAUNCHES_TWO;
    ctx->last_icp_probe_misses = -1;
    for (int b = 0; b < n_prob; ++b) state_result(h[b], out[b]);
    return TDV_OK;
}

// icp_run_dev for n instances against one target in one call: instance b = h_count[b] points from point h_start[b] of d_src, start
// pose T0s + 16 b.  Arguments are the caller's to check.  Per instance the result is icp_run_dev's for that cloud on this ctx, bit for
// bit.  With tree sums, the AUTO or GRID search and a usable hash grid over the target (built once here) all instances iterate
// together: k_icp_nn_grid_multi + k_icp_accumulate_multi, two launches per iteration for the whole batch, one read-back of all
// states per burst.  Otherwise: small problems in one k_icp_small launch (icp_small_batch_dev), else icp_run_dev per instance with
// the shared grid or Morton order.
int icp_batch_run_dev(tdv_ctx* ctx, const float* d_src, const int* h_start, const int* h_count, int n, const float* d_tgt, const float* d_tgt_normals,
                      int nt, const float* T0s, float thr, int max_iterations, IcpObjective obj, int fixed_iterations, tdv_icp_result* out) {
    for (int b = 0; b < n; ++b) result_defaults(T0s + 16 * (size_t)b, out[b]);
    if (n == 0) return TDV_OK;
    int ns_max = 0, span = 0;
    bool contiguous = h_start[0] == 0;
    for (int b = 0; b < n; ++b) {
        ns_max = std::max(ns_max, h_count[b]);
        span = std::max(span, h_start[b] + h_count[b]);
        if (b + 1 < n && h_start[b + 1] != h_start[b] + h_count[b]) contiguous = false;
    }
    if (max_iterations == 0 || nt == 0 || ns_max == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    const float tau = tau_le(thr);
    const int search = ctx->icp_search;
    // (1) small problems: every instance in one launch of the kernel the single call runs for them (it has no fixed-iteration mode)
    if (!fixed_iterations && contiguous && icp_small_batch_fits(ctx, ns_max, nt)) {
        std::vector<int> off((size_t)n + 1, 0);
        for (int b = 0; b < n; ++b) off[b + 1] = off[b] + h_count[b];
        int* d_off;
        TDV_TRY(ws_alloc(ctx, (size_t)n + 1, &d_off));
        TDV_HIP(ctx, hipMemcpyAsync(d_off, off.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, s));   // (off outlives the call's sync)
        return icp_small_batch_dev(ctx, d_src, d_off, n, d_tgt, d_tgt_normals, nt, T0s, thr, max_iterations, obj, out);
    }
    // the target's hash grid at this threshold, once for the call (icp_run_dev uses a grid under AUTO or GRID)
    CellGrid cg{}; bool have_grid = false;
    if (tau < FLT_MAX && (search == TDV_ICP_SEARCH_AUTO || search == TDV_ICP_SEARCH_GRID)) {
        TDV_TRY(cell_grid_build(ctx, d_tgt, nt, thr, &cg));
        have_grid = true;
    }
    IcpPlan pl;     // (with the grid above icp_plan builds nothing)
    if (ctx->icp_accumulate == TDV_ICP_ACCUMULATE_REFERENCE || !cg.usable) {
        // (3) one icp_run_dev per instance, with the shared grid or, if any instance walks it, the shared Morton order
        SortedCloud sorted{}; bool have_sorted = false;
        for (int b = 0; b < n && !have_sorted; ++b) {
            TDV_TRY(icp_plan(ctx, d_tgt, h_count[b], nt, thr, have_grid ? &cg : nullptr, pl));
            if (pl.search == TDV_ICP_SEARCH_PRUNED) { TDV_TRY(spatial_sort_cloud(ctx, d_tgt, nt, sorted)); have_sorted = true; }
        }
        for (int b = 0; b < n; ++b) {
            const WsMark mark = ws_mark(ctx);
            TDV_TRY(icp_run_dev(ctx, d_src + (size_t)h_start[b] * 3, h_count[b], d_tgt, d_tgt_normals, nt, T0s + 16 * (size_t)b, thr, max_iterations,
                                obj.at(h_start[b]), fixed_iterations, &out[b], have_sorted ? &sorted : nullptr, have_grid ? &cg : nullptr));
            ws_rewind(ctx, mark);
        }
        return TDV_OK;
    }
    // (2) all instances together.  Per instance, the accumulation shape icp_run_dev would take for it alone (icp_plan): make_plan's
    // points per thread where it searches with the grid, else the brute-force path's 1 (which the one-launch path k_icp_small reproduces).
    std::vector<IcpInst> inst((size_t)n);
    int nn_blocks = 0, acc_blocks = 0;
    for (int b = 0; b < n; ++b) {
        const int ns = h_count[b];
        TDV_TRY(icp_plan(ctx, d_tgt, ns, nt, thr, &cg, pl));
        IcpInst& in = inst[b];
        in.src_off = h_start[b]; in.ns = ns; in.ppt = pl.p.acc_ppt;
        in.nn_blk0 = nn_blocks; in.acc_blk0 = acc_blocks;
        in.acc_blocks = pl.p.acc_blocks;
        nn_blocks += (ns + 255) / 256;
        acc_blocks += in.acc_blocks;
    }
    // one upload: initial states | instance table | block -> instance (NN blocks, then accumulation blocks); pinned staging of the ctx
    const size_t st_bytes = (size_t)n * sizeof(IcpState), inst_bytes = (size_t)n * sizeof(IcpInst);
    const size_t up_bytes = st_bytes + inst_bytes + ((size_t)nn_blocks + acc_blocks) * sizeof(int);
    TDV_TRY(pin_reserve(ctx, up_bytes));      // (after cell_grid_build, which reads its flags back through the same staging)
    IcpState* h = reinterpret_cast<IcpState*>(ctx->pin);
    init_states(h, T0s, n, obj.rel_fitness, obj.rel_rmse);
    for (int b = 0; b < n; ++b) if (h_count[b] == 0) h[b].done = 1;   // no points: n_corr = 0 < 3, the result is the start pose
    std::memcpy(ctx->pin + st_bytes, inst.data(), inst_bytes);
    int* h_blk = reinterpret_cast<int*>(ctx->pin + st_bytes + inst_bytes);
    for (int b = 0; b < n; ++b) {
        for (int k = 0; k < (h_count[b] + 255) / 256; ++k) *h_blk++ = b;
    }
    for (int b = 0; b < n; ++b) {
        for (int k = 0; k < inst[b].acc_blocks; ++k) *h_blk++ = b;
    }
    char* d_up; float* pd2; int* pidx; double* slabs; unsigned* tickets;
    TDV_TRY(ws_alloc(ctx, up_bytes, &d_up));
    TDV_TRY(ws_alloc(ctx, (size_t)span, &pd2));
    TDV_TRY(ws_alloc(ctx, (size_t)span, &pidx));
    TDV_TRY(ws_alloc(ctx, (size_t)acc_blocks * ACC_NV, &slabs));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &tickets));
    TDV_HIP(ctx, hipMemcpyAsync(d_up, ctx->pin, up_bytes, hipMemcpyHostToDevice, s));
    TDV_HIP(ctx, hipMemsetAsync(tickets, 0, (size_t)n * sizeof(unsigned), s));      // the last block of an instance resets its word
    IcpState* d_st = reinterpret_cast<IcpState*>(d_up);
    const IcpInst* d_inst = reinterpret_cast<const IcpInst*>(d_up + st_bytes);
    const int* d_blk_nn = reinterpret_cast<const int*>(d_up + st_bytes + inst_bytes);
    const int* d_blk_acc = d_blk_nn + nn_blocks;
    const GridEntry* gtable = reinterpret_cast<const GridEntry*>(cg.table);
    const float4* gnode = reinterpret_cast<const float4*>(cg.node);
    const IcpLoss loss = ctx_loss(ctx);
    ctx->last_icp_search = TDV_ICP_SEARCH_GRID;
    ctx->last_icp_launches = TDV_ICP_LAUNCHES_TWO;
    ctx->last_icp_probe_misses = -1;
    const int run = run_flags(fixed_iterations, obj);
    TDV_TRY(run_bursts(ctx, h, d_st, n,max_iterations, fixed_iterations, [&]() {
        {
            ScopedTimer tm(ctx, TDV_TIMER_ICP_NN);
            k_icp_nn_grid_multi<<<nn_blocks, 256, 0, s>>>(d_src, d_inst, d_blk_nn, gtable, gnode, cg.mask, cg.shift, cg.inv_cell, d_st, tau, pd2, pidx);
        }
        icp_dispatch(ctx, obj, d_tgt_normals, [&](auto M, auto R, auto) {      // (tree sums: see above)
            constexpr int MODE = decltype(M)::value;
            k_icp_accumulate_multi<MODE, decltype(R)::value><<<acc_blocks, 256, 0, s>>>(
                d_src, d_inst, d_blk_acc, d_tgt, MODE == ICP_POINT_TO_POINT ? nullptr : d_tgt_normals, pd2, pidx, d_st, tau, run, loss, slabs, tickets,
                kernel_args<MODE>(obj));
        });
    }));
    for (int b = 0; b < n; ++b) state_result(h[b], out[b]);
    return TDV_OK;
}

int icp_loss_check(tdv_ctx* ctx) {
    if (ctx->icp_loss != TDV_ICP_LOSS_L2 && ctx->icp_accumulate == TDV_ICP_ACCUMULATE_REFERENCE) {
        snprintf(ctx->err, sizeof(ctx->err), "icp: a robust loss (tdv_ctx_set_icp_loss) cannot run with reference-order accumulation, whose float "
                 "sums are the reference's and have no loss; set TDV_ICP_LOSS_L2 or TDV_ICP_ACCUMULATE_TREE");
        return TDV_ERR_BAD_ARG;
    }
    return TDV_OK;
}

int icp_objective_check(tdv_ctx* ctx, const IcpObjective& obj, const float* tgt_normals, bool device) {
    if (obj.kind < ICP_GICP) return icp_loss_check(ctx);
    // (below, reference-order sums are refused: no loss check needed)
    const bool gicp = obj.kind == ICP_GICP;
    if (gicp) {
        if (!obj.src_normals || !tgt_normals || !std::isfinite(obj.param) || !(obj.param > 0.f && obj.param <= 1.f)) return TDV_ERR_BAD_ARG;
    } else {
        if (!obj.src_rgb || !tgt_normals || !obj.tgt_color || !std::isfinite(obj.param) || !(obj.param >= 0.f && obj.param <= 1.f)) return TDV_ERR_BAD_ARG;
        if (device && (reinterpret_cast<uintptr_t>(obj.tgt_color) & 15) != 0) {
            snprintf(ctx->err, sizeof(ctx->err), "colored_icp: the target colour table is read as float4 and must be 16-byte aligned");
            return TDV_ERR_BAD_ARG;
        }
    }
    if (ctx->icp_accumulate == TDV_ICP_ACCUMULATE_REFERENCE) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: reference-order accumulation reproduces the reference's float sums, and the reference has no "
                 "%s ICP; set TDV_ICP_ACCUMULATE_TREE", gicp ? "gicp" : "colored_icp", gicp ? "generalized" : "colored");
        return TDV_ERR_BAD_ARG;
    }
    return TDV_OK;
}

// (the loss does not enter: one correspondence pass, its outputs and n_corr only)
int icp_correspondences_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt,
                            const float* T, float thr, IcpOutputs outs, int* n_corr) {
    if (!ctx || !d_src || !d_tgt || !T || ns <= 0 || nt <= 0) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipSetDevice(ctx->device));
    NnPlan p = make_plan(ns, nt);
    p.acc_ppt = 1; p.acc_blocks = (ns + 255) / 256;   // one point per thread in the outputs-only pass
    bool pruned = (ctx->icp_search == TDV_ICP_SEARCH_PRUNED || ctx->icp_search == TDV_ICP_SEARCH_GRID) && tau_le(thr) < FLT_MAX;
    CellGrid grid{};
    if (pruned && ctx->icp_search == TDV_ICP_SEARCH_GRID) TDV_TRY(cell_grid_build(ctx, d_tgt, nt, thr, &grid));
    ctx->last_icp_search = grid.usable ? TDV_ICP_SEARCH_GRID : (pruned ? TDV_ICP_SEARCH_PRUNED : TDV_ICP_SEARCH_BRUTE);
    if (pruned) p.nsplit = 1;
    IcpBuffers b;
    TDV_TRY(alloc_buffers(ctx, p, b));
    TDV_TRY(pin_reserve(ctx, sizeof(IcpState)));
    IcpState* h = reinterpret_cast<IcpState*>(ctx->pin);
    init_states(h, T, 1);
    hipStream_t s = ctx->stream;
    TDV_HIP(ctx, hipMemcpyAsync(b.st, h, sizeof(IcpState), hipMemcpyHostToDevice, s));
    const float tau = tau_le(thr);
    if (grid.usable) {
        k_icp_nn_grid<<<(ns + 255) / 256, 256, 0, s>>>(d_src, ns, reinterpret_cast<const GridEntry*>(grid.table), reinterpret_cast<const float4*>(grid.node),
                                                       grid.mask, grid.shift, grid.inv_cell, b.st, tau, b.pd2, b.pchunk, ProbeCache{});
    } else if (pruned) {   // explicit request only: entries beyond the threshold come back as corr 0 / d2 FLT_MAX
        SortedCloud st{};
        TDV_TRY(spatial_sort_cloud(ctx, d_tgt, nt, st));
        k_icp_nn_pruned<<<(ns + PN_WAVES * PN_PTS - 1) / (PN_WAVES * PN_PTS), 64 * PN_WAVES, 0, s>>>(
            d_src, ns, st, b.st, tau, b.pd2, b.pchunk);
    } else {
        k_aos_to_soa_pad<<<(p.nt_pad + 255) / 256, 256, 0, s>>>(d_tgt, nt, p.nt_pad, INFINITY, b.tx, b.ty, b.tz);
        k_icp_nn_scan<<<dim3(p.blocks_x, p.nsplit), NN_BLOCK, 0, s>>>(d_src, ns, p.ns_pad, b.tx, b.ty, b.tz, p.n_chunks,
                                                                      p.chunks_per_split, b.st, b.pd2, b.pchunk);
    }
    k_icp_accumulate<2, 1><<<p.acc_blocks, 256, 0, s>>>(d_src, ns, p.ns_pad, d_tgt, nullptr, b.tx, b.ty, b.tz, p.nsplit,
                                                        b.pd2, b.pchunk, pruned ? 1 : 0, b.st, tau, 0, IcpLoss{TDV_ICP_LOSS_L2, 0.f}, b.slabs, b.ticket, outs.corr, outs.d2, outs.accepted, IcpArgs<2>{});
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipMemcpyAsync(h, b.st, sizeof(IcpState), hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    if (n_corr) *n_corr = h->n_corr;
    return TDV_OK;
}

}  // namespace tdv
