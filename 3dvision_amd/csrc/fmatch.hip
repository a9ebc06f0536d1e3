// Descriptor correspondences of RANSAC on gfx950 (f32 VALU work; nothing here is HBM- or MFMA-bound).
//
// Replaces the matching loop of Registration::ransacRegistration (/root/reference/src/registration.cpp:216-232):
// for every source descriptor the target with the smallest 33-D squared distance, accumulated in d order without FMA,
// strict <, lowest target index on ties.  Which search answers a call (fm_wants_index, fm_indexes_sources):
//   * fewer than 4,096 sources or 2,048 targets, or TDV_FM_BRUTE set: the reference's scan (k_feature_match_scan) - source
//     descriptors in VGPRs, targets broadcast through the scalar data path, 98 VALU ops per pair;
//   * otherwise a packed index of the targets is built (fmatch_index.hip; layouts in fmatch_layout.hpp) and searched
//     LEAF-MAJOR (k_lm_*, the default): the sources are located and ordered by their home leaf, every source meets its home
//     leaf, one round of box tests collects the (leaf, source) pairs that are left, and the pairs are evaluated leaf by leaf
//     with full waves;
//   * descriptors without structure overflow the leaf-major pair room (and TDV_FM_LEAFMAJOR=0, or more than 16,384 leaves,
//     skip it): the call then WALKS the same index, one wave per two sources (k_fm_query); what a wave gives up on goes to
//     8 waves per source pair (k_fm_query_overflow) or, if nearly every box passes, to the plain scan over just those sources.
// The study build (fmatch_study.hpp) adds the variants that lost their measurement: round 1's key-ordered pruned scan, the
// walk with 1 or 4 sources per wave, two rounds of box tests, the scan without early exit, and the statistics reports.
// Every distance that is evaluated is the reference's expression; every target that is not evaluated is excluded by a
// box lower bound computed with the same expression on the per-dimension gaps (float sub/mul/add are monotone, so
// lb <= fl(dist) for every row of the box, no margin), or by the tie rule (equal bound, only higher indices inside).
#include "tdv_internal.hpp"
#include "fmatch_layout.hpp"
#include <cfloat>
#include <climits>
#include <cmath>
#include <algorithm>
#include <cstdlib>

namespace tdv {

constexpr int FM_SPL = 2;
#ifndef FM_BLOCK_VALUE
#define FM_BLOCK_VALUE 256
#endif
constexpr int FM_BLOCK = FM_BLOCK_VALUE;
constexpr int FM_SRC_PER_BLOCK = FM_SPL * FM_BLOCK;
constexpr int FM_SEED = 256;   // targets of the seeding launch

// EARLY: partial-distance early exit.  dist accumulates non-negative terms in d order, and fl(a + b) >= a for b >= 0,
// so once the partial sum is >= the lane's best the final distance cannot pass the strict "<": a target is dropped
// as soon as that holds for every lane of the wave (checked after 11 and 22 of the 33 dimensions).  `seed` (the exact
// best over the first targets, computed by a first launch) lets every split start with a tight bound.
// `list` / `n_list`: scan only these sources (the sources the packed-index search gave up on), results at the source's own
// row.  `seed`: a per-source starting bound.  SEED_FROM_LOWER: the seed is the exact best over LOWER target indices
// (part 0 seeding the later splits), so strict < keeps the lowest-index rule.  Otherwise the seed is a distance found
// somewhere in the table: the scan starts one ulp above it and walks every target in ascending order with strict <, so
// it finds that distance again and keeps the lowest index that reaches the minimum.
template <bool EARLY, bool SEED_FROM_LOWER>
__global__ __launch_bounds__(FM_BLOCK)
void k_feature_match_scan(const float* __restrict__ fs, int ns, int ns_pad,
                          const float* __restrict__ ft, int j_begin, int j_end, int per_split,
                          const float* __restrict__ seed, const int* __restrict__ list, int n_list,
                          float* __restrict__ pd, int* __restrict__ pj) {
    const int split = blockIdx.y;
    const int j0 = j_begin + split * per_split;
    const int j1 = min(j_end, j0 + per_split);
    const int base = blockIdx.x * FM_SRC_PER_BLOCK + threadIdx.x;
    const int n_here = list ? n_list : ns;
    float f[FM_SPL][FD];
    float best[FM_SPL]; int bj[FM_SPL]; int src[FM_SPL];
#pragma unroll
    for (int s = 0; s < FM_SPL; ++s) {
        const int t = base + s * FM_BLOCK;
        src[s] = list ? list[min(t, n_here - 1)] : t;
        const int i = min(max(src[s], 0), ns - 1);
#pragma unroll
        for (int d = 0; d < FD; ++d) f[s][d] = fs[(size_t)i * FD + d];
        if (seed) {
            const float sd = seed[i];
            best[s] = SEED_FROM_LOWER ? sd : ((sd < FLT_MAX && sd >= 0.f) ? __int_as_float(__float_as_int(sd) + 1) : FLT_MAX);
            bj[s] = -1;
        } else { best[s] = FLT_MAX; bj[s] = 0; }
        if (t >= n_here || src[s] < 0) src[s] = -1;    // padding lane: duplicate work, no output
    }
    for (int j = j0; j < j1; ++j) {
        const float* __restrict__ g = ft + (size_t)j * FD;  // wave-uniform -> scalar loads
        float q[FD];
#pragma unroll
        for (int d = 0; d < FD; ++d) q[d] = g[d];
        float dist[FM_SPL];
#pragma unroll
        for (int s = 0; s < FM_SPL; ++s) dist[s] = 0.f;
#pragma unroll
        for (int seg = 0; seg < 3; ++seg) {
#pragma unroll
            for (int s = 0; s < FM_SPL; ++s)
#pragma unroll
                for (int d = seg * 11; d < seg * 11 + 11; ++d) { float diff = f[s][d] - q[d]; dist[s] += diff * diff; }
            if (EARLY && seg < 2) {
                bool alive = false;
#pragma unroll
                for (int s = 0; s < FM_SPL; ++s) alive = alive || (dist[s] < best[s]);
                if (!__any(alive)) goto next_target;
            }
        }
#pragma unroll
        for (int s = 0; s < FM_SPL; ++s) {
            bool lt = dist[s] < best[s];
            best[s] = lt ? dist[s] : best[s];
            bj[s] = lt ? j : bj[s];
        }
    next_target:;
    }
#pragma unroll
    for (int s = 0; s < FM_SPL; ++s) {
        if (src[s] < 0 || src[s] >= ns) continue;
        size_t o = (size_t)split * ns_pad + src[s];
        pd[o] = best[s]; pj[o] = bj[s];
    }
}
// the listed sources' partial results, combined in split order with strict < (lowest target index wins ties)
__global__ void k_feature_match_combine_list(const int* __restrict__ list, int n_list, int ns, int ns_pad, int nparts, const float* __restrict__ pd,
                                             const int* __restrict__ pj, int* __restrict__ corr) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_list) return;
    const int i = list[t];
    if (i < 0 || i >= ns) return;
    float best = FLT_MAX; int bj = 0;
    for (int p0 = 0; p0 < nparts; p0 += 8) {   // 16 loads in flight
        float d[8]; int j[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int p = min(p0 + u, nparts - 1);
            d[u] = pd[(size_t)p * ns_pad + i]; j[u] = pj[(size_t)p * ns_pad + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (p0 + u < nparts && j[u] >= 0 && d[u] < best) { best = d[u]; bj = j[u]; }
    }
    corr[i] = bj;
}

// partial results are combined in launch/split order with strict <: the lowest target index wins ties
__global__ void k_feature_match_combine(int ns, int ns_pad, int nparts, const float* __restrict__ pd,
                                        const int* __restrict__ pj, int* __restrict__ corr) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    float best = FLT_MAX; int bj = 0;
    for (int s = 0; s < nparts; ++s) {
        float d = pd[(size_t)s * ns_pad + i];
        if (d < best) { best = d; bj = pj[(size_t)s * ns_pad + i]; }
    }
    corr[i] = bj;
}

// The sources of an indexed call are ordered by a counting sort over buckets of home leaves (a bucket = a leaf up to 16,384 leaves).
constexpr int FMP_KEY_BITS = 7;
constexpr int FMP_BUCKETS = 1 << (2 * FMP_KEY_BITS);   // 16384 (64 KB of LDS counters in the ordering kernels)
// Real descriptors crowd a few buckets, so both passes count in an LDS histogram first (one global atomic per
// non-empty bucket and workgroup instead of one per row).
constexpr int FMP_SORT_BLOCK = 1024;
__global__ __launch_bounds__(FMP_SORT_BLOCK)
void k_fm_scatter(const int* __restrict__ bucket_of, int n, const int* __restrict__ start, int* __restrict__ cursor,
                  int* __restrict__ perm) {
    __shared__ int h[FMP_BUCKETS];      // rows of this workgroup per bucket, then the workgroup's base inside the bucket
    for (int b = threadIdx.x; b < FMP_BUCKETS; b += FMP_SORT_BLOCK) h[b] = 0;
    __syncthreads();
    const int i = blockIdx.x * FMP_SORT_BLOCK + threadIdx.x;
    int b = 0, local = 0;
    if (i < n) { b = bucket_of[i]; local = atomicAdd(&h[b], 1); }
    __syncthreads();
    for (int c = threadIdx.x; c < FMP_BUCKETS; c += FMP_SORT_BLOCK) if (h[c]) h[c] = atomicAdd(&cursor[c], h[c]);
    __syncthreads();
    if (i < n) perm[start[b] + h[b] + local] = i;   // order inside a bucket is irrelevant to the result
}

// The set bit of m nearest to position c, the higher one on a tie (the inside-out order c, c+1, c-1, c+2, ... restricted to
// the set bits), or -1: two shifts, a find-first and a count-leading on the wave's scalar unit instead of walking the
// positions one by one (that walk was 2,000 of the 4,800 instructions of a wave of the descriptor search).
__device__ __forceinline__ int nearest_set_bit(unsigned long long m, int c) {
    if (!m) return -1;
    const unsigned long long up = m >> c;                                  // bit 0 = position c
    const unsigned long long dn = c > 0 ? m << (64 - c) : 0ull;            // bit 63 = position c - 1
    const int du = up ? __ffsll((long long)up) - 1 : 128;
    const int dd = dn ? __clzll((long long)dn) + 1 : 128;
    return du <= dd ? c + du : c - dd;
}

#ifndef FMQ_WAVES_PER_SIMD
#define FMQ_WAVES_PER_SIMD 4
#endif

// home leaf of every source: its cell of the target packing (slab by p0, column by p1, leaf by p2)
__global__ void k_fm_locate(const float* __restrict__ fs, int ns, const float* __restrict__ basis, int S0, int S1,
                            const float* __restrict__ b0, const float* __restrict__ b1, const int* __restrict__ col_leaf0,
                            const float* __restrict__ leaf_p2, int bucket_shift, int* __restrict__ home, int* __restrict__ bucket_of,
                            float* __restrict__ sp /* [ns][4]: p0 p1 p2 - */, unsigned* __restrict__ amax) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, am = 0.f;
    if (i < ns) principal_coords(fs + (size_t)i * FD, basis, a0, a1, a2, am);
    {   // one atomic per workgroup (per wave they queue on one address for longer than the kernel's own work takes)
        __shared__ unsigned s_max;
        if (threadIdx.x == 0) s_max = 0u;
        __syncthreads();
        float wm = am;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wm = fmaxf(wm, __shfl_xor(wm, off, 64));
        if ((threadIdx.x & 63) == 0) atomicMax(&s_max, __float_as_uint(wm));
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(amax, s_max);
    }
    if (i >= ns) return;
    *reinterpret_cast<float4*>(sp + (size_t)i * 4) = make_float4(a0, a1, a2, 0.f);
    int k = 0;
    for (int s = 1; s < S0; ++s) k += (b0[s] <= a0) ? 1 : 0;           // boundaries ascend; NaN compares false -> cell 0
    int j = 0;
    for (int s = 1; s < S1; ++s) j += (b1[k * S1 + s] <= a1) ? 1 : 0;
    const int c = k * S1 + j;
    const int l0 = col_leaf0[c], l1 = col_leaf0[c + 1];
    int l = l0;
    for (int s = l0 + 1; s < l1; ++s) l += (leaf_p2[s] <= a2) ? 1 : 0;
    l = min(l, max(l1 - 1, l0));
    home[i] = l;
    bucket_of[i] = l >> bucket_shift;
}
__global__ __launch_bounds__(FMP_SORT_BLOCK)
void k_fm_bucket_hist(const int* __restrict__ bucket_of, int n, int* __restrict__ hist) {
    __shared__ int h[FMP_BUCKETS];
    for (int b = threadIdx.x; b < FMP_BUCKETS; b += FMP_SORT_BLOCK) h[b] = 0;
    __syncthreads();
    const int i = blockIdx.x * FMP_SORT_BLOCK + threadIdx.x;
    if (i < n) atomicAdd(&h[bucket_of[i]], 1);
    __syncthreads();
    for (int b = threadIdx.x; b < FMP_BUCKETS; b += FMP_SORT_BLOCK) if (h[b]) atomicAdd(&hist[b], h[b]);
}

typedef float v2f __attribute__((ext_vector_type(2)));
// a candidate as one word, (distance bits : original index): for distances >= 0 unsigned order is (distance, index) order, and NaN
// and +inf have larger bit patterns than FLT_MAX - a strict < on keys takes the lowest index among equal distances and nothing the
// reference's `dist < best_dist` would not take
__device__ __forceinline__ unsigned long long fm_key(float dist, int orig) { return ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)orig; }
// A lane's descriptor (a row of a leaf, or a source): 33 floats kept as 17 aligned register pairs, so that packed arithmetic can name
// either half of a pair (op_sel) instead of the compiler giving every element a pair of its own.
struct FmRow {
    v2f p[(FD + 1) / 2];
    __device__ __forceinline__ float at(int d) const { return (d & 1) ? p[d >> 1].y : p[d >> 1].x; }
    __device__ __forceinline__ void load(const float* __restrict__ f, int stride) {      // element d at f[d * stride]
#pragma unroll
        for (int d = 0; d < FD; ++d) { if (d & 1) p[d >> 1].y = f[d * stride]; else p[d >> 1].x = f[d * stride]; }
        p[FD >> 1].y = 0.f;
    }
};

// the descriptors of the K sources of every wave, interleaved: fsk[wave][d][k] = fs[sperm[K wave + k]][d] (a wave past the
// end of an uneven count repeats the last source, as FmWave does): (q_k[d], q_k+1[d]) is then one aligned SGPR pair
__global__ void k_fm_interleave_rows(const float* __restrict__ fs, const int* __restrict__ sperm, int ns, int K, float* __restrict__ fsk) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nwave = ((size_t)ns + K - 1) / K;
    if (e >= nwave * K * FD) return;
    const size_t w = e / ((size_t)K * FD); const int r = (int)(e % ((size_t)K * FD)), d = r / K, k = r % K;
    fsk[e] = fs[(size_t)sperm[min((int)(K * w) + k, ns - 1)] * FD + d];
}

// ---- wave-level helpers (DPP: no LDS traffic) ----------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
// minimum over the 64 lanes, returned wave-uniform (an SGPR after readlane)
__device__ __forceinline__ float wave_min_f32(float v) {
    v = fminf(v, dpp_f32<0xB1, 0xF>(v));    // quad_perm [1,0,3,2]
    v = fminf(v, dpp_f32<0x4E, 0xF>(v));    // quad_perm [2,3,0,1]
    v = fminf(v, dpp_f32<0x141, 0xF>(v));   // row_half_mirror
    v = fminf(v, dpp_f32<0x140, 0xF>(v));   // row_mirror: every lane of a 16-lane row holds the row minimum
    v = fminf(v, dpp_f32<0x142, 0xA>(v));   // row_bcast15 into rows 1 and 3
    v = fminf(v, dpp_f32<0x143, 0xC>(v));   // row_bcast31 into rows 2 and 3: lane 63 holds the wave minimum
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// K sources per wave, LANE = TARGET-SIDE ITEM (a row of a leaf, a leaf box of a group, a group box): every lane does
// useful, distinct work, and the K source descriptors are wave-uniform (scalar loads of the wave's own 132-B rows, which
// stay in the scalar cache).  The sources of a wave share a home leaf (they were ordered by it), so they need nearly the
// same leaves: a leaf fetched once (33 coalesced 256-B loads, lane = row) serves all K of them.
//   (what was tried on the way, at 143k x 151k real descriptors: profiles/r2/history/feature_match_designs.md)
// Per source and lane a running (distance, original index) minimum over the rows that lane has seen; its wave minimum is
// the source's bound.  A box is opened when its bound <= the source's bound (<=: an equal distance with a lower index
// could still win; the exact lowest-index rule is applied by the final lexicographic reduction).
// Order: home leaf, home group, then every group whose box passes (tested once, lane = group, with the bounds the home
// group left), inside-out from the home group; inside a group the leaves whose boxes pass (lane = leaf), inside-out.
// Bounds only shrink, so a mask computed earlier can open a leaf too many, never skip one.
struct FmTables {   // device pointers of a packed index + the per-call source-side arrays (plain struct: passed by value)
    const float* fs; const int* sperm; const int* home_of; int ns;
    const float* fs2;   // even K: the descriptors of every wave's K sources interleaved, [wave][33][K] (k_fm_interleave_rows); else null
    const float* T; const int* torig; int nleaf, ngroup;
    const float *lbox, *gbox, *pbox, *gpbox;
    const float* sp; const unsigned *amax_t, *amax_s; float pscale;
};

// The search state of one wave: K sources, lane = target-side item.  SHARED: the bounds are also kept in LDS words
// (integer atomic min on the bits of a non-negative float) so that several waves working on the same sources tighten
// each other's bounds.
template <int K, bool SHARED>
struct FmWave {
    const FmTables& t;
    const int lane;
    int src[K];
    const float* q2 = nullptr;    // even K: this wave's interleaved sources, [33][K] (wave-uniform)
    unsigned long long lkey[K];   // this lane's best (distance bits : original index): unsigned order == (distance, index) order for distances >= 0
    float bound[K];
    float pmargin;
    int home, hg;
    int* s_bound;                 // SHARED only
    unsigned n_open = 0, n_leaf_tests = 0, n_group_tests = 0;

    __device__ __forceinline__ FmWave(const FmTables& tt, int s0, int* sb) : t(tt), lane(threadIdx.x & 63), s_bound(sb) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            src[k] = __builtin_amdgcn_readfirstlane(t.sperm[min(s0 + k, t.ns - 1)]);   // past the end: the last source again
            lkey[k] = (unsigned long long)__float_as_uint(FLT_MAX) << 32; bound[k] = FLT_MAX;   // registration.cpp:218-219: only dist < FLT_MAX is ever taken
        }
        if (K % 2 == 0) q2 = t.fs2 + (size_t)(s0 / K) * (K * FD);
        home = min(t.nleaf - 1, max(0, __builtin_amdgcn_readfirstlane(t.home_of[src[K / 2]])));
        hg = home / FX_GROUP;
        // rounding margin of a principal-coordinate gap (principal_bound_note): 3e-5 * largest |x_d - mean_d| on either side
        pmargin = 3e-5f * fmaxf(__uint_as_float(__builtin_amdgcn_readfirstlane(*t.amax_t)), __uint_as_float(__builtin_amdgcn_readfirstlane(*t.amax_s)));
    }
    __device__ __forceinline__ void refresh() {
        if (SHARED) {
#pragma unroll
            for (int k = 0; k < K; ++k) bound[k] = fminf(bound[k], __int_as_float(__builtin_amdgcn_readfirstlane(s_bound[k])));
        }
    }
    using RowBuf = FmRow;
    __device__ __forceinline__ void load_leaf(int leaf, RowBuf& row, int& ro) const {
        row.load(t.T + (size_t)leaf * (FD * FX_LEAF) + lane, FX_LEAF);
        ro = t.torig[(size_t)leaf * FX_LEAF + lane];
    }
    __device__ __forceinline__ void eval_leaf(const RowBuf& row, int ro) {
        if constexpr (K % 2 == 0) {
            // two sources at once: every op one v_pk_*_f32 on (source k, source k + 1) - the same IEEE operations per
            // element, half the instructions; the wave's descriptors sit interleaved in memory so that (q_k[d], q_k+1[d]) is
            // one aligned SGPR pair
            const float* __restrict__ qk = q2;   // (left to the compiler, the K x 33 values stay in SGPRs across leaves, a few of them
                                                 // parked in VGPR lanes; re-reading them per leaf through the scalar cache doubled the time)
            v2f dist[K / 2];
#pragma unroll
            for (int j = 0; j < K / 2; ++j) dist[j] = (v2f){0.f, 0.f};
#pragma unroll
            for (int d = 0; d < FD; ++d) {
                const v2f pr = row.p[d >> 1];
                const v2f rw = (d & 1) ? __builtin_shufflevector(pr, pr, 1, 1) : __builtin_shufflevector(pr, pr, 0, 0);
#pragma unroll
                for (int j = 0; j < K / 2; ++j) {
                    const v2f q = {qk[K * d + 2 * j], qk[K * d + 2 * j + 1]};
                    const v2f diff = q - rw;          // registration.cpp:222-224
                    dist[j] += diff * diff;
                }
            }
#pragma unroll
            for (int j = 0; j < K / 2; ++j) {
                const unsigned long long k0 = fm_key(dist[j].x, ro);
                const unsigned long long k1 = fm_key(dist[j].y, ro);
                lkey[2 * j] = k0 < lkey[2 * j] ? k0 : lkey[2 * j];
                lkey[(2 * j + 1) % K] = k1 < lkey[(2 * j + 1) % K] ? k1 : lkey[(2 * j + 1) % K];
            }
            ++n_open;
            return;
        }
#pragma unroll
        for (int k = 0; k < K && K % 2 != 0; ++k) {
            const float* __restrict__ q = t.fs + (size_t)src[k] * FD;   // wave-uniform -> scalar loads
            float dist = 0.f;
#pragma unroll
            for (int d = 0; d < FD; ++d) { const float diff = q[d] - row.at(d); dist += diff * diff; }   // registration.cpp:222-224
            // strict < on (distance, index): the lowest index among equal distances; NaN and +inf have larger bit patterns than
            // FLT_MAX and are never taken, like `dist < best_dist` in the reference
            const unsigned long long key = fm_key(dist, ro);
            lkey[k] = key < lkey[k] ? key : lkey[k];
        }
        ++n_open;
    }
    // the sources' bounds = wave minimum of the lanes' best distances; needed only where boxes are tested
    __device__ __forceinline__ void update_bounds() {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float m = wave_min_f32(__uint_as_float((unsigned)(lkey[k] >> 32)));
            if (m < bound[k]) {
                bound[k] = m;
                if (SHARED && lane == 0) atomicMin(&s_bound[k], __float_as_int(m));
            }
        }
    }
    __device__ __forceinline__ void open_leaf(int leaf) {
        RowBuf row; int ro;
        load_leaf(leaf, row, ro);
        eval_leaf(row, ro);
    }
    // lanes = the 64 boxes of one block; bit b of the result: some source may still find a better row in box b.
    // principal_bound_note — the 3-D box is tested first (6 loads), the 33-D box (66 loads) only if it leaves anything.
    // Why the 3-D bound is safe although a projection is not monotone in float arithmetic: for orthonormal directions
    // sum_r (p_r(q) - p_r(t))^2 <= |q - t|^2 in real numbers.  (i) The f32 directions are orthonormal to 1.2e-7 (checked on
    // the host, else pscale = 0 disables the test).  (ii) A computed coordinate (33 sequential mul/add, no FMA) is within
    // 34 u * sqrt(33) * M = 1.2e-5 M of its real value, M = largest |x_d - mean_d|: a computed gap to the box exceeds the
    // real gap to any row by at most 2.5e-5 M; pmargin = 3e-5 M is subtracted.  (iii) fl(dist) >= |q - t|^2 (1 - 36 u).
    // pscale = 1 - 1e-4 covers (i), (iii) and the rounding of the three squares with a factor 30 to spare.  Non-finite
    // input makes M = +inf: gaps clamp to 0 and only the 33-D test decides.
    __device__ __forceinline__ unsigned long long box_mask(const float* __restrict__ blk, const float* __restrict__ pblk, bool own_bounds = true) {
        if (own_bounds) update_bounds();      // (pass B tests the group boxes with bounds every wave shares: see there)
        float lbp[K]; bool pa[K];
#pragma unroll
        for (int k = 0; k < K; ++k) lbp[k] = 0.f;
#pragma unroll
        for (int r = 0; r < PD; ++r) {
            const float lo = pblk[r * 64 + lane], hi = pblk[(PD + r) * 64 + lane];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float pq = t.sp[(size_t)src[k] * 4 + r];   // wave-uniform -> scalar load
                const float g = fmaxf(fmaxf(lo - pq, pq - hi) - pmargin, 0.f);
                lbp[k] += g * g;
            }
        }
        unsigned long long any = 0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) { pa[k] = !(lbp[k] * t.pscale > bound[k]); any |= __ballot(pa[k]); }
        if (!any) return 0ull;
        float lb[K];
#pragma unroll
        for (int k = 0; k < K; ++k) lb[k] = 0.f;
        if constexpr (K % 2 == 0) {       // packed over pairs of sources, as in eval_leaf
            const float* __restrict__ qk = q2;
            v2f lb2[K / 2];
#pragma unroll
            for (int j = 0; j < K / 2; ++j) lb2[j] = (v2f){0.f, 0.f};
#pragma unroll 11
            for (int d = 0; d < FD; ++d) {
                const float lo = blk[d * 64 + lane], hi = blk[(FD + d) * 64 + lane];
#pragma unroll
                for (int j = 0; j < K / 2; ++j) {
                    const v2f q = {qk[K * d + 2 * j], qk[K * d + 2 * j + 1]};
                    const v2f a = (v2f){lo, lo} - q, b = q - (v2f){hi, hi};
                    const v2f g = {fmaxf(fmaxf(a.x, b.x), 0.f), fmaxf(fmaxf(a.y, b.y), 0.f)};
                    lb2[j] += g * g;
                }
            }
#pragma unroll
            for (int j = 0; j < K / 2; ++j) { lb[2 * j] = lb2[j].x; lb[(2 * j + 1) % K] = lb2[j].y; }
        } else
#pragma unroll 11   // 22 loads in flight; full unrolling hoists all 66 and spills
        for (int d = 0; d < FD && K % 2 != 0; ++d) {   // one dimension of the 64 boxes at a time: two coalesced loads, K bounds advance
            const float lo = blk[d * 64 + lane], hi = blk[(FD + d) * 64 + lane];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float qd = t.fs[(size_t)src[k] * FD + d];   // wave-uniform -> scalar load
                const float g = fmaxf(fmaxf(lo - qd, qd - hi), 0.f);
                lb[k] += g * g;
            }
        }
        unsigned long long m = 0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) m |= __ballot(pa[k] && lb[k] <= bound[k]);    // an empty box (+inf, -inf) has lb = +inf: never set
        return m;
    }
    __device__ __forceinline__ unsigned long long leaf_mask(int g) {
        ++n_leaf_tests;
        unsigned long long m = box_mask(t.lbox + (size_t)g * (2 * FD * FX_GROUP), t.pbox + (size_t)g * (2 * PD * FX_GROUP));
        if (g == hg) m &= ~(1ull << (home - g * FX_GROUP));
        return m;
    }
    __device__ __forceinline__ unsigned long long group_mask(int c, bool own_bounds = true) {
        ++n_group_tests;
        unsigned long long m = box_mask(t.gbox + (size_t)c * (2 * FD * 64), t.gpbox + (size_t)c * (2 * PD * 64), own_bounds);
        if (hg >= 0 && hg / 64 == c) m &= ~(1ull << (hg % 64));
        return m;
    }
    // The leaves of group g whose boxes pass, inside-out from the home side.  The mask is known before the first leaf is
    // opened, so the next leaf's 34 loads are issued before the current leaf is evaluated (two register buffers): a wave
    // that opens many leaves no longer pays a full memory round trip for each.
    // Returns false when the leaf budget ran out before the group was finished (pass A: the caller gives the sources up).
    __device__ __forceinline__ bool visit_group(int g, unsigned budget = 0xffffffffu) {
        const int l0 = g * FX_GROUP, cnt = min(FX_GROUP, t.nleaf - l0);
        if (cnt <= 0) return true;        // a group past the end: its empty box "passes" for a NaN query (every gap is NaN -> 0)
        unsigned long long m = leaf_mask(g);
        const int centre = (g == hg) ? home - l0 : (g < hg ? cnt - 1 : 0);   // enter a neighbouring group from the home side
        if (cnt < 64) m &= (1ull << cnt) - 1ull;
        auto next = [&]() -> int {
            const int l = nearest_set_bit(m, centre);
            if (l < 0) return -1;
            m &= ~(1ull << l);
            return l0 + l;
        };
        int cur = next();
        if (cur < 0) return true;
        RowBuf a, b; int roa, rob = 0;
        load_leaf(cur, a, roa);
        for (;;) {
            if (n_open >= budget) return false;
            const int n1 = next();
            if (n1 >= 0) load_leaf(n1, b, rob);
            eval_leaf(a, roa);
            if (n1 < 0) break;
            if (n_open >= budget) return false;
            const int n2 = next();
            if (n2 >= 0) load_leaf(n2, a, roa);
            eval_leaf(b, rob);
            if (n2 < 0) break;
        }
        return true;
    }
    // lowest (distance, original index) of source k over the lanes
    __device__ __forceinline__ void result(int k, float& bd, int& bo) const {
        unsigned hi = (unsigned)(lkey[k] >> 32), lo = (unsigned)lkey[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned oh = __shfl_xor(hi, off, 64), ol = __shfl_xor(lo, off, 64);
            const bool tk = oh < hi || (oh == hi && ol < lo);
            hi = tk ? oh : hi; lo = tk ? ol : lo;
        }
        bd = __uint_as_float(hi);
        bo = hi == __float_as_uint(FLT_MAX) ? INT_MAX : (int)lo;      // nothing below FLT_MAX was seen
    }
};

// where the scan class starts in the walk's overflow list (pass B's class starts at 0; each class holds at most ns wave starts)
__host__ __device__ __forceinline__ int fm_scan_class_offset(int ns) { return ns + 1; }

// Pass A: one wave per K sources.  Home leaf, home group, then every group whose box passes (tested once per chunk of 64
// groups, lane = group, with the bounds the home group left), inside-out from the home group.  A wave whose sources
// turn out to be outliers (far from every target: most boxes pass) stops after `leaf_limit` leaves, stores what it has
// (part_d / part_j) and puts its sources on the overflow list: pass B spreads them over 8 waves each.  Without that the
// call waits for a few waves that open hundreds of leaves one after the other (measured: 580 leaves, 1.3 of 1.5 ms).
template <int K, bool STATS>
__global__ __launch_bounds__(FM_BLOCK, FMQ_WAVES_PER_SIMD)
void k_fm_query(FmTables t, int blocks_per_xcd, int leaf_limit, int heavy_groups, int* __restrict__ overflow_count /* [2]: pass B, scan */, int* __restrict__ overflow_list,
                int* __restrict__ overflow_src, float* __restrict__ part_d, int* __restrict__ part_j, int* __restrict__ corr, unsigned long long* __restrict__ stats) {
    // Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one).  Give every XCD a CONTIGUOUS stretch of
    // the home-ordered sources: neighbouring waves open the same leaves, so the stretch's leaves (1/8 of the table) stay
    // in that XCD's 4 MB L2 instead of every L2 seeing the whole table.
    const int block = (blockIdx.x & 7) * blocks_per_xcd + (blockIdx.x >> 3);
    const int wid = block * (FM_BLOCK / 64) + (threadIdx.x >> 6);
    const int s0 = __builtin_amdgcn_readfirstlane(wid * K);
    if (s0 >= t.ns) return;
    unsigned long long t_start = 0;
    if (STATS) t_start = wall_clock64();
    FmWave<K, false> w(t, s0, nullptr);
    w.open_leaf(w.home);
    bool overflow = !w.visit_group(w.hg, (unsigned)leaf_limit);
    const int nchunk = (t.ngroup + 63) / 64;
    int groups_left = overflow ? t.ngroup : 0;       // estimate of what is left when the wave gives up
    for (int c = 0; c < nchunk && !overflow; ++c) {     // (chunks in index order; within a chunk inside-out from the home group's side)
        unsigned long long m = w.group_mask(c);
        const int g0 = c * 64, cnt = min(64, t.ngroup - g0);
        const int centre = w.hg < g0 ? 0 : (w.hg >= g0 + cnt ? cnt - 1 : w.hg - g0);
        if (cnt < 64) m &= (1ull << cnt) - 1ull;
        while (m) {
            const int g = nearest_set_bit(m, centre);
            if ((int)w.n_open >= leaf_limit || !w.visit_group(g0 + g, (unsigned)leaf_limit)) {
                overflow = true;
                groups_left = __popcll(m) + 64 * (nchunk - 1 - c);
                break;
            }
            m &= ~(1ull << g);
        }
    }
    // Sources given up with few groups left go to pass B (8 waves each on the index); with many groups left nearly every
    // box passes (an outlier, or a plateau of near-identical rows) and the plain scan is the efficient way to finish them.
    const bool to_scan = overflow && groups_left >= heavy_groups;
    int slot = 0;
    if (overflow && w.lane == 0) slot = atomicAdd(overflow_count + (to_scan ? 1 : 0), 1);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float bd; int bo;
        w.result(k, bd, bo);
        if (w.lane == 0 && s0 + k < t.ns) {
            if (overflow) { part_d[w.src[k]] = bd; part_j[w.src[k]] = bo; }
            else corr[w.src[k]] = bo == INT_MAX ? 0 : bo;   // nothing finite -> the reference keeps index 0
        }
    }
    if (overflow && w.lane == 0) {
        if (!to_scan) overflow_list[slot] = s0;
        else {
            overflow_list[fm_scan_class_offset(t.ns) + slot] = s0;     // second half of the list: the scan class, as wave starts ...
#pragma unroll
            for (int k = 0; k < K; ++k) overflow_src[slot * K + k] = s0 + k < t.ns ? w.src[k] : -1;   // ... and as sources
        }
    }
    if (STATS && w.lane == 0) {   // [0] waves, [1] group-chunk tests, [2] groups visited, [3] leaves opened, [4] most leaves opened by one wave
        const unsigned long long dt = wall_clock64() - t_start;   // 100 MHz ticks
        atomicAdd(&stats[0], 1ull); atomicAdd(&stats[1], (unsigned long long)w.n_group_tests); atomicAdd(&stats[2], (unsigned long long)w.n_leaf_tests);
        atomicAdd(&stats[3], (unsigned long long)w.n_open); atomicMax(&stats[4], (unsigned long long)w.n_open);
        atomicAdd(&stats[5], dt); atomicMax(&stats[6], dt);
    }
}

// Pass B: the sources pass A gave up on, one workgroup of 8 waves per K of them.  Every wave tests the group boxes
// with the same bounds (pass A's best, which already saw the home neighbourhood) and takes every 8th passing group;
// bounds found by one wave reach the others through LDS.  The result is the lexicographic minimum of pass A's partial
// answer and the 8 waves' answers, so it does not matter that pass A's groups are visited again.
constexpr int FMB_WAVES = 8;
template <int K, bool STATS>
__global__ __launch_bounds__(FMB_WAVES * 64)
void k_fm_query_overflow(FmTables t, const int* __restrict__ overflow_count, const int* __restrict__ overflow_list,
                         const float* __restrict__ part_d, const int* __restrict__ part_j, int* __restrict__ corr,
                         unsigned long long* __restrict__ stats) {
    __shared__ int s_bound[K];
    __shared__ float s_fd[FMB_WAVES][K];
    __shared__ int s_fj[FMB_WAVES][K];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int count = *overflow_count;
    for (int e = blockIdx.x; e < count; e += gridDim.x) {
        const int s0 = overflow_list[e];
        FmWave<K, true> w(t, s0, s_bound);
        if (threadIdx.x < K) s_bound[threadIdx.x] = __float_as_int(fminf(part_d[t.sperm[min(s0 + (int)threadIdx.x, t.ns - 1)]], FLT_MAX));
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) w.bound[k] = __int_as_float(s_bound[k]);
        w.hg = -1;                                   // no group is special here: pass A's partial answer covers what it saw
        w.home = -1;
        const int nchunk = (t.ngroup + 63) / 64;
        int turn = 0;
        for (int c = 0; c < nchunk; ++c) {
            float keep[K];
#pragma unroll
            for (int k = 0; k < K; ++k) keep[k] = w.bound[k];
#pragma unroll
            for (int k = 0; k < K; ++k) w.bound[k] = __int_as_float(__float_as_int(part_d[w.src[k]]));   // the bound every wave shares
            unsigned long long m = w.group_mask(c, false);
#pragma unroll
            for (int k = 0; k < K; ++k) w.bound[k] = keep[k];
            const int g0 = c * 64;
            if (t.ngroup - g0 < 64) m &= (1ull << (t.ngroup - g0)) - 1ull;    // groups past the end (see visit_group)
            while (m) {
                const int g = __builtin_ctzll(m);
                m &= m - 1;
                if (turn++ % FMB_WAVES != wave) continue;
                w.refresh();
                w.visit_group(g0 + g);
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float bd; int bo;
            w.result(k, bd, bo);
            if (w.lane == 0) { s_fd[wave][k] = bd; s_fj[wave][k] = bo; }
        }
        __syncthreads();
        if (threadIdx.x < K && s0 + (int)threadIdx.x < t.ns) {
            const int k = threadIdx.x;
            const int i = t.sperm[s0 + k];
            float bd = part_d[i]; int bo = part_j[i];
            for (int v = 0; v < FMB_WAVES; ++v) {
                const float od = s_fd[v][k]; const int oo = s_fj[v][k];
                if (od < bd || (od == bd && oo < bo)) { bd = od; bo = oo; }
            }
            corr[i] = bo == INT_MAX ? 0 : bo;
        }
        if (STATS && w.lane == 0) { atomicAdd(&stats[8], 1ull); atomicAdd(&stats[9], (unsigned long long)w.n_open); atomicMax(&stats[10], (unsigned long long)w.n_open); }
        __syncthreads();   // the LDS words are reused by the next entry
    }
}

// ---- leaf-major search (round 3; the default) --------------------------------------------------------------------------
// k_fm_query spends 40 % of its instructions on box tests (lane = box, one or two sources per wave) and walks a source's
// leaves one after the other: 13 % of the lane-op peak, and a few sources that need hundreds of leaves decide when the call
// ends.  Here the roles are swapped - LANE = SOURCE everywhere, boxes and target rows staged in LDS and read back as
// broadcasts - and the leaves are not walked by the sources that need them but COLLECTED per leaf and evaluated with full waves:
//   k_lm_plan<false> + k_lm_eval<true>   round 0: every source against its home leaf.  The search order is sorted by home
//                   leaf, so it already is the per-leaf list; the histogram the ordering made gives the work units.
//   k_lm_boxes<3>   a workgroup = 64 sources in home-leaf order, lane = source in each of its 4 waves.  Group boxes, then the
//                   leaf boxes of every group some lane cannot exclude - the 3-D principal box first, the 33-D box where any
//                   lane passes it - with the bound round 0 left.  A box a source cannot exclude is a (leaf, source) PAIR;
//                   a wave records them as entries (leaf, first source, lane mask) and counts them per pool and leaf.
//   k_lm_plan<true> one workgroup: sources per leaf (summed over the pools), exclusive scans -> where each leaf's sources go,
//                   where each pool's share of a leaf goes, and the list of work units (a leaf x up to 64 of its sources).
//   k_lm_scatter    one workgroup per pool, write positions in LDS: the entries' sources to their leaf's stretch.
//   k_lm_eval<false> one wave per unit: the leaf (8.4 KB) staged in the wave's own LDS, 64 rows x 33 dimensions against 64
//                   sources, two rows per packed instruction: 3 x 33 x 32 v_pk_*_f32 per unit, the reference's operations
//                   in the reference's order (registration.cpp:222-224); 64 % of the nominal lane-op peak.  A lane that found
//                   a smaller (distance, index) key lowers its source's key with a 64-bit atomic min.
//   k_lm_finish     keys -> correspondences; the overflow flag straight into pinned host memory.
// A source that needs hundreds of leaves simply owns hundreds of pairs spread over as many units: there is no tail and no
// overflow pass.  Exactness as before: every row that is not evaluated lies in a box whose bound (same expression, same
// order, monotone float operations) exceeds a distance the source had already reached; bounds only shrink, so a pair
// emitted early is at worst superfluous.  The result is the minimum over 64-bit (distance bits : original index) keys,
// which does not depend on the order of the atomics.  Descriptors without structure (every box passes) overflow the entry
// pools or the pair room (32 per source): the call then falls back to k_fm_query and its scan class.
// What was measured on the way (143k x 151k relief descriptors): profiles/r3/history/feature_match_leaf_major.md.
constexpr int LM_WAVES = 4;       // waves per workgroup of the evaluation
#ifndef LM_BOX_WAVES_VALUE
#define LM_BOX_WAVES_VALUE 4
#endif
constexpr int LM_BOX_WAVES = LM_BOX_WAVES_VALUE;   // waves that share the 64 sources of a box-test workgroup (query at 143k x 151k with 1 / 2 / 4 / 8: 0.67 / 0.55 / 0.49 / 0.55-0.63 ms)
constexpr int LM_ENTRIES = 96;    // (leaf, lane mask) entries a wave buffers in LDS before it reserves room for them in its pool
constexpr int LM_PAIRS_PER_SOURCE = 32;
constexpr int LM_POOLS = 64;
constexpr unsigned long long LM_KEY_NONE = (unsigned long long)0x7f7fffffu << 32;   // FLT_MAX : 0 - only dist < FLT_MAX is ever taken (registration.cpp:218-219)

struct LmLists {
    int *pool_count, *entry_cursor, *overflow;            // zeroed per round: [LM_POOLS][nleaf] (sources per pool and leaf) [LM_POOLS] [1]
    int *leaf_count, *pool_start;                         // written by k_lm_plan: [nleaf] sources per leaf, [LM_POOLS][nleaf] where a pool's sources of a leaf go
    int4* entries; int pool_cap;                          // (leaf, first source of the workgroup, lane mask): LM_POOLS pools of pool_cap entries, every pool
                                                          // with its own cursor (one cursor for everything: 9,000 returning atomics on one address, 50 us)
    int pair_cap;                                         // room in sorted_src
    int *leaf_start, *unit_start;                         // [nleaf + 1]
    int *unit_leaf;                                       // [pair_cap / 64 + nleaf + 2]
    int *sorted_src;                                      // [pair_cap]
    unsigned long long* keys;                             // [ns]
    int unit_cap;                                         // room in unit_leaf
};
struct LmSrc : FmRow { float pq[PD]; };     // a lane's source: its descriptor and principal coordinates
// The original row indices of a leaf as k_lm_eval reads them (rarely: only where a lane can improve): the "constant" address space
// tells the compiler that nothing in the kernel writes them, which lets it use the scalar path although the kernel stores keys.
typedef const __attribute__((address_space(4))) int* lm_cint_p;


__device__ __forceinline__ void lm_load_source(const FmTables& t, int src, LmSrc& q) {
    q.load(t.fs + (size_t)src * FD, 1);
#pragma unroll
    for (int r = 0; r < PD; ++r) q.pq[r] = t.sp[(size_t)src * 4 + r];
}
// The scalar path cannot feed this: a leaf is 8.4 KB, the scalar cache 16 KB per CU and its fill path slow (waves of one
// CU on different leaves evict each other: 193 us for the home leaves alone).  Rows and boxes are therefore STAGED IN LDS -
// coalesced vector loads in, broadcast reads (every lane the same address) out.
typedef float v4f_lm __attribute__((ext_vector_type(4)));
// the wave's own copy of a leaf: rows[d * 64 + r]
__device__ __forceinline__ void lm_stage_leaf(const float* __restrict__ T, int leaf, float* rows, int lane) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(T + (size_t)leaf * (FD * FX_LEAF));
    float4* dst = reinterpret_cast<float4*>(rows);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < (FD * FX_LEAF / 4 + 63) / 64; ++k) { const int e = k * 64 + lane; if (e < FD * FX_LEAF / 4) dst[e] = src[e]; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// One staged leaf against every lane's source; key = the lane's best (distance bits : original index) so far.
__device__ __forceinline__ void lm_eval_leaf(const float* rows, const int* __restrict__ torig, int leaf, const LmSrc& q, unsigned long long& key) {
    const lm_cint_p ro = (lm_cint_p)(torig + (size_t)leaf * FX_LEAF);
#pragma unroll 1
    for (int r0 = 0; r0 < FX_LEAF; r0 += 16) {
        v2f acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = (v2f){0.f, 0.f};
#pragma unroll
        for (int d = 0; d < FD; ++d) {
            const v2f pr = q.p[d >> 1];
            const v2f qq = (d & 1) ? __builtin_shufflevector(pr, pr, 1, 1) : __builtin_shufflevector(pr, pr, 0, 0);
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                const v4f_lm r4 = *reinterpret_cast<const v4f_lm*>(rows + d * FX_LEAF + r0 + 4 * j4);   // 4 rows of dimension d: one broadcast ds_read_b128
                const v2f d0 = qq - (v2f){r4[0], r4[1]}, d1 = qq - (v2f){r4[2], r4[3]};              // registration.cpp:222-224
                acc[2 * j4] += d0 * d0; acc[2 * j4 + 1] += d1 * d1;
            }
        }
        // the 16 distances against the lane's best: the keys are only built where some lane can improve (or tie)
        float mn = fminf(acc[0].x, acc[0].y);
#pragma unroll
        for (int j = 1; j < 8; ++j) mn = fminf(mn, fminf(acc[j].x, acc[j].y));
        if (__any(mn <= __uint_as_float((unsigned)(key >> 32)))) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned long long k0 = fm_key(acc[j].x, ro[r0 + 2 * j]);
                const unsigned long long k1 = fm_key(acc[j].y, ro[r0 + 2 * j + 1]);
                key = k0 < key ? k0 : key;      // strict < on (distance, index): NaN and +inf have larger bit patterns than FLT_MAX
                key = k1 < key ? k1 : key;
            }
        }
    }
}
// box: 72 floats in LDS (min[33] | max[33] | pmin[3] | pmax[3]), the same for every lane
__device__ __forceinline__ bool lm_pass3(const float* box, const LmSrc& q, float pmargin, float pscale, float bound) {   // principal_bound_note (FmWave::box_mask)
    float lbp = 0.f;
#pragma unroll
    for (int r = 0; r < PD; ++r) {
        const float g = fmaxf(fmaxf(box[2 * FD + r] - q.pq[r], q.pq[r] - box[2 * FD + PD + r]) - pmargin, 0.f);
        lbp += g * g;
    }
    return !(lbp * pscale > bound);
}
__device__ __forceinline__ float lm_bound33(const float* box, const LmSrc& q) {
    float lb = 0.f;
#pragma unroll
    for (int d = 0; d < FD; ++d) {
        const float qd = (d & 1) ? q.p[d >> 1].y : q.p[d >> 1].x;
        const float g = fmaxf(fmaxf(box[d] - qd, qd - box[FD + d]), 0.f);
        lb += g * g;
    }
    return lb;
}

// Rounds 1 and 2: box tests.  A WORKGROUP = 64 sources in home-leaf order (lane = source in each of its LM_BOX_WAVES waves); the
// boxes of a group are staged in LDS by the whole workgroup and its waves share the leaves between them (leaf i of the group
// goes to wave i % LM_BOX_WAVES).  (First version: one wave per 64 sources, boxes through the scalar path - a chain of dependent
// scalar loads with two waves per SIMD: 267 us for what is 20 us of instructions.)
// ROUND 1: the leaves of the workgroup's home group(s); ROUND 2: every other group, group boxes first.  The four waves hold the
// same sources, so every mask that steers the staging is the same in all of them: the barriers are reached together.
template <int ROUND>
__global__ __launch_bounds__(64 * LM_BOX_WAVES)
void k_lm_boxes(FmTables t, const float* __restrict__ sleaf, const float* __restrict__ sgroup, LmLists L, unsigned long long* __restrict__ stats) {
    const unsigned long long t_begin = stats ? wall_clock64() : 0ull;
    unsigned n3 = 0, n33 = 0, nemit = 0;        // (TDV_FM_STATS: 3-D tests, 33-D tests, boxes emitted by this wave)
    __shared__ __attribute__((aligned(16))) float s_box[FX_GROUP * LM_BOX];
    __shared__ int s_leaf[LM_BOX_WAVES][LM_ENTRIES];
    __shared__ unsigned long long s_mask[LM_BOX_WAVES][LM_ENTRIES];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s0 = blockIdx.x * 64;
    if (s0 >= t.ns) return;
    const bool valid = s0 + lane < t.ns;
    const int src = t.sperm[min(s0 + lane, t.ns - 1)];          // past the end: the last source again (tested, never emitted)
    LmSrc q;
    {   // the workgroup's 64 descriptors: rows in (four threads per 132-B row), through LDS, a lane's own row out
        constexpr int PITCH = FD + 4;                            // 37 floats: a lane reading its row meets no bank twice
        const int part = threadIdx.x & 3;
        for (int r = threadIdx.x >> 2; r < 64; r += (64 * LM_BOX_WAVES) >> 2) {
            const float* __restrict__ row = t.fs + (size_t)t.sperm[min(s0 + r, t.ns - 1)] * FD;
            for (int d = part; d < FD; d += 4) s_box[r * PITCH + d] = row[d];
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < FD; ++d) { if (d & 1) q.p[d >> 1].y = s_box[lane * PITCH + d]; else q.p[d >> 1].x = s_box[lane * PITCH + d]; }
        q.p[FD >> 1].y = 0.f;
        const float4 pc = *reinterpret_cast<const float4*>(t.sp + (size_t)src * 4);
        q.pq[0] = pc.x; q.pq[1] = pc.y; q.pq[2] = pc.z;
    }
    const int home = min(t.nleaf - 1, max(0, t.home_of[src])), hg = home / FX_GROUP;
    const float pmargin = 3e-5f * fmaxf(__uint_as_float(__builtin_amdgcn_readfirstlane(*t.amax_t)), __uint_as_float(__builtin_amdgcn_readfirstlane(*t.amax_s)));
    const float bound = __uint_as_float((unsigned)(L.keys[src] >> 32));
    const unsigned long long t_loaded = stats ? (bound == -1.f ? 1ull : wall_clock64()) : 0ull;   // (reads `bound`: the clock is taken after the loads have landed)
    int n_ent = 0;
    auto stage = [&](const float* __restrict__ boxes, int count) {     // count boxes -> s_box, by the whole workgroup
        __syncthreads();
        const float4* __restrict__ from = reinterpret_cast<const float4*>(boxes);
        float4* to = reinterpret_cast<float4*>(s_box);
        for (int e = threadIdx.x; e < count * (LM_BOX / 4); e += 64 * LM_BOX_WAVES) to[e] = from[e];
        __syncthreads();
    };
    auto flush = [&]() {
        if (n_ent == 0) return;
        const int pool = (blockIdx.x * LM_BOX_WAVES + wave) % LM_POOLS;
        int base = 0;
        if (lane == 0) base = atomicAdd(L.entry_cursor + pool, n_ent);
        __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < n_ent; e += 64)      // one instruction for all the boxes' counters, nothing waits for them; per pool: a counter per leaf alone
            atomicAdd(&L.pool_count[(size_t)pool * t.nleaf + s_leaf[wave][e]], __popcll(s_mask[wave][e]));   // queued ~20 atomics from all over the chip on one address
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + n_ent > L.pool_cap) { if (lane == 0) *L.overflow = 1; }
        else
            for (int e = lane; e < n_ent; e += 64) {
                const unsigned long long m = s_mask[wave][e];
                L.entries[(size_t)pool * L.pool_cap + base + e] = make_int4(s_leaf[wave][e], s0, (int)(unsigned)m, (int)(unsigned)(m >> 32));
            }
        __builtin_amdgcn_wave_barrier();
        n_ent = 0;
    };
    auto leaves_of_group = [&](int g) {
        const int l0 = g * FX_GROUP, cnt = min(FX_GROUP, t.nleaf - l0);
        stage(sleaf + (size_t)l0 * LM_BOX, cnt);
        for (int i = wave; i < cnt; i += LM_BOX_WAVES) {
            const int l = l0 + i;
            const float* box = s_box + i * LM_BOX;
            const bool p3 = lm_pass3(box, q, pmargin, t.pscale, bound);
            ++n3;
            if (!__any(p3)) continue;
            ++n33;
            const float lb = lm_bound33(box, q);
            const unsigned long long m = __ballot(valid && p3 && lb <= bound && l != home);   // (its home leaf: round 0 evaluated it; an empty box (+inf, -inf) has lb = +inf: never set)
            if (!m) continue;
            if (lane == 0) { s_leaf[wave][n_ent] = l; s_mask[wave][n_ent] = m; }
            ++nemit;
            if (++n_ent == LM_ENTRIES) flush();
        }
    };
    if (ROUND == 1) {
        unsigned long long todo = __ballot(valid);
        while (todo) {                                           // the workgroup's distinct home groups
            const int g = __builtin_amdgcn_readlane(hg, __builtin_ctzll(todo));
            todo &= ~__ballot(hg == g);
            leaves_of_group(g);
        }
    } else {
        for (int g0 = 0; g0 < t.ngroup; g0 += 64) {
            const int gcnt = min(64, t.ngroup - g0);
            stage(sgroup + (size_t)g0 * LM_BOX, gcnt);
            unsigned long long gm = 0ull;                        // groups some lane cannot exclude (the same in all four waves)
            for (int i = 0; i < gcnt; ++i) {
                if (ROUND == 2 && __ballot(hg == g0 + i)) continue;   // one of the home groups: round 1 tested its leaves for every lane
                const float* box = s_box + i * LM_BOX;
                const bool p3 = lm_pass3(box, q, pmargin, t.pscale, bound);
                if (!__any(p3)) continue;
                const float lb = lm_bound33(box, q);
                if (__ballot(valid && p3 && lb <= bound)) gm |= 1ull << i;
            }
            while (gm) {
                const int g = g0 + __builtin_ctzll(gm);
                gm &= gm - 1ull;
                leaves_of_group(g);
            }
        }
    }
    const unsigned long long t_f0 = stats ? wall_clock64() : 0ull;
    flush();
    if (stats && lane == 0) {      // [0] waves [1] ticks total [2] ticks until the source is loaded [3] ticks of the last flush [4] 3-D tests [5] 33-D tests [6] boxes emitted [7] max ticks
        const unsigned long long t_end = wall_clock64();
        atomicAdd(&stats[0], 1ull); atomicAdd(&stats[1], t_end - t_begin); atomicAdd(&stats[2], t_loaded - t_begin); atomicAdd(&stats[3], t_end - t_f0);
        atomicAdd(&stats[4], (unsigned long long)n3); atomicAdd(&stats[5], (unsigned long long)n33); atomicAdd(&stats[6], (unsigned long long)nemit); atomicMax(&stats[7], t_end - t_begin);
    }
}

// leaf_start / unit_start: exclusive scans of the pair counts and of the unit counts (a unit = up to 64 sources of one leaf).
// POOLS: the counts come per pool; every pool also learns where its sources of every leaf go (pool order inside a leaf).
template <bool POOLS>
__global__ __launch_bounds__(1024)
void k_lm_plan(LmLists L, int nleaf) {
    __shared__ int s_w[2][16], s_carry[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { s_carry[0] = 0; s_carry[1] = 0; }
    __syncthreads();
    const bool dead = *L.overflow != 0;                      // the entry pool ran over: nothing below may be trusted, the call falls back
    for (int l0 = 0; l0 < nleaf; l0 += 1024) {
        const int l = l0 + threadIdx.x;
        int c = 0;
        int pc_of[POOLS ? LM_POOLS : 1];                     // (registers: the loop is unrolled; loads first, stores later, so that they overlap)
        if (l < nleaf && !dead) {
            if (POOLS) {
#pragma unroll
                for (int p = 0; p < LM_POOLS; ++p) pc_of[p] = L.pool_count[(size_t)p * nleaf + l];
#pragma unroll
                for (int p = 0; p < LM_POOLS; ++p) c += pc_of[p];
                L.leaf_count[l] = c;
            } else c = L.leaf_count[l];
        }
        const int u = (c + 63) >> 6;
        int ic = c, iu = u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int a = __shfl_up(ic, off, 64), b = __shfl_up(iu, off, 64); if (lane >= off) { ic += a; iu += b; } }
        if (lane == 63) { s_w[0][wave] = ic; s_w[1][wave] = iu; }
        __syncthreads();
        int bc = s_carry[0], bu = s_carry[1];
        for (int w = 0; w < wave; ++w) { bc += s_w[0][w]; bu += s_w[1][w]; }
        const int pc = bc + ic - c, pu = bu + iu - u;
        if (l < nleaf) {
            L.leaf_start[l] = pc; L.unit_start[l] = pu;
            // (the entry pools admit up to 64 sources per entry, i.e. more units than unit_leaf holds when the descriptors have no
            //  structure: such a call falls back below - and must not have written past the array on its way there)
            for (int k = 0; k < u && pu + k < L.unit_cap; ++k) L.unit_leaf[pu + k] = l;
            if (POOLS && !dead) {
                int run = pc;
#pragma unroll
                for (int p = 0; p < LM_POOLS; ++p) { L.pool_start[(size_t)p * nleaf + l] = run; run += pc_of[p]; }
            }
        }
        __syncthreads();
        if (threadIdx.x == 1023) { s_carry[0] = bc + ic; s_carry[1] = bu + iu; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool fits = s_carry[0] <= L.pair_cap && s_carry[1] <= L.unit_cap;          // (round 0: the sources themselves)
        if (!fits) *L.overflow = 1;
        L.leaf_start[nleaf] = s_carry[0]; L.unit_start[nleaf] = fits ? s_carry[1] : 0;
    }
}

// every entry's sources to their leaf's stretch of sorted_src: ONE WORKGROUP PER POOL, with the pool's write positions (one per leaf) in
// LDS.  A wave takes 64 entries - a returning LDS atomic per lane - then goes through them entry by entry with lane = source.
// (Positions from returning atomics on one global counter per leaf: 45 us however the rest was arranged - some twenty atomics from all
// over the chip on one address wait for each other.)
__global__ __launch_bounds__(1024)
void k_lm_scatter(LmLists L, int nleaf) {      // grid LM_POOLS, dynamic LDS nleaf ints
    extern __shared__ int s_cur[];
    if (*L.overflow) return;
    const int pool = blockIdx.x;
    for (int l = threadIdx.x; l < nleaf; l += 1024) s_cur[l] = L.pool_start[(size_t)pool * nleaf + l];
    __syncthreads();
    const int n = min(L.entry_cursor[pool], L.pool_cap);
    const int4* __restrict__ ent = L.entries + (size_t)pool * L.pool_cap;
    int* __restrict__ out = L.sorted_src;
    const int lane = threadIdx.x & 63;
    for (int i0 = threadIdx.x - lane; i0 < n; i0 += 1024) {
        const bool valid = i0 + lane < n;
        const int4 e = valid ? ent[i0 + lane] : make_int4(0, 0, 0, 0);
        const unsigned long long m = ((unsigned long long)(unsigned)e.w << 32) | (unsigned)e.z;
        const int base = valid ? atomicAdd(&s_cur[e.x], __popcll(m)) : 0;
        const int cnt = min(64, n - i0);
        for (int k = 0; k < cnt; ++k) {
            const unsigned long long mk = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(e.w, k) << 32) | (unsigned)__builtin_amdgcn_readlane(e.z, k);
            const int bk = __builtin_amdgcn_readlane(base, k), sk = __builtin_amdgcn_readlane(e.y, k);
            if ((mk >> lane) & 1ull) out[bk + __popcll(mk & ((1ull << lane) - 1ull))] = sk + lane;     // (the position in the search order: k_lm_eval looks the source up)
        }
    }
}

// INIT: round 0 - the units are the sources of every leaf that are at home there (L.sorted_src = the search order itself, L.leaf_count =
// the histogram the ordering made); every source occurs exactly once and gets its first key.
template <bool INIT>
__global__ __launch_bounds__(64 * LM_WAVES)
void k_lm_eval(FmTables t, LmLists L) {
    __shared__ __attribute__((aligned(16))) float s_rows[LM_WAVES][FD * FX_LEAF];
    if (*L.overflow) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = L.unit_start[t.nleaf];
    // workgroups are dealt round-robin over the 8 XCDs: every XCD takes a contiguous stretch of the units (= of the leaves)
    const int vblocks = (total + LM_WAVES - 1) / LM_WAVES, per_xcd = (vblocks + 7) / 8;
    const int xcd = blockIdx.x & 7, step = max(1, (int)gridDim.x >> 3);
    for (int j = blockIdx.x >> 3; j < per_xcd; j += step) {
        const int u = __builtin_amdgcn_readfirstlane((xcd * per_xcd + j) * LM_WAVES + wave);
        if (u >= total) continue;
        const int leaf = __builtin_amdgcn_readfirstlane(L.unit_leaf[u]);
        const int chunk = u - L.unit_start[leaf];
        const int p0 = L.leaf_start[leaf] + chunk * 64, cnt = L.leaf_count[leaf] - chunk * 64;
        const bool valid = lane < cnt;
        const int listed = L.sorted_src[p0 + (valid ? lane : 0)];
        const int src = INIT ? listed : t.sperm[listed];         // (round 0 walks the search order itself; later rounds list positions in it)
        const unsigned long long before = INIT ? LM_KEY_NONE : L.keys[src];
        LmSrc q;
        lm_load_source(t, src, q);
        unsigned long long key = before;
        lm_stage_leaf(t.T, leaf, s_rows[wave], lane);
        lm_eval_leaf(s_rows[wave], t.torig, leaf, q, key);
        if (INIT) { if (valid) L.keys[src] = key; }
        else if (valid && key < before) atomicMin(&L.keys[src], key);
    }
}

__global__ void k_lm_finish(const unsigned long long* __restrict__ keys, int ns, const int* __restrict__ ovf1, const int* __restrict__ ovf2,
                            int* __restrict__ corr, int* __restrict__ host_flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { host_flag[0] = (*ovf1 | *ovf2) ? 1 : 0; __threadfence_system(); }
    if (i >= ns) return;
    const unsigned long long k = keys[i];
    corr[i] = (unsigned)(k >> 32) == 0x7f7fffffu ? 0 : (int)(unsigned)k;   // nothing finite -> the reference keeps index 0
}

// ---- host side: each rule once ------------------------------------------------------------------------------------------
// Every TDV_FM_* / TDV_LM_* switch is read here and nowhere else; none of them changes a correspondence.  The first two are real
// getenv()s read per call in both libraries; the rest exist in the study library only: A/B switches per call, tuning values once.
struct FmKnobs {
    bool brute, walk_only;   // TDV_FM_BRUTE: the plain scan whatever the sizes.  TDV_FM_LEAFMAJOR=0: the walk instead of the leaf-major search
    bool keyorder, stats;    // TDV_FM_KEYORDER: round 1's key-ordered scan instead of the index.  TDV_FM_STATS: box-test / leaf counts on stderr
    int lm_rounds;           // TDV_LM_ROUNDS=2: the home groups' boxes first, the other groups with the bounds those left
    int leaf_limit;          // TDV_FM_LIMIT: leaves a wave of pass A opens before it hands over (32 while a leaf cost what it did in the middle
                             // of round 2; 128 since: relief part 0.81 -> 0.73 ms, cuboid 200k x 200k 4.05 -> 2.04 ms, random rows 16.8 -> 17.7 ms)
    int heavy_groups;        // TDV_FM_HEAVY: a wave that gives up with this many groups left hands its sources to the scan class
    int force_k;             // TDV_FM_K: sources per wave of the walk (0 = the default, 2; 1 and 4 measured slower)
    int eval_blocks;         // TDV_LM_EVAL_BLOCKS: a multiple of 8 (1024 / 2048 / 4096 / 8192: 0.51 / 0.49 / 0.477 / 0.478 ms at 143k x 151k)
    bool early;              // TDV_FM_NO_EARLY_EXIT unset: the plain scan drops a target once no lane of the wave can still take it
};
static FmKnobs fm_knobs() {
    auto number = [](const char* v, int otherwise) { return v ? atoi(v) : otherwise; };
    static const int leaf_limit = number(study_env("TDV_FM_LIMIT"), 128), heavy_groups = number(study_env("TDV_FM_HEAVY"), 8);
    static const int force_k = number(study_env("TDV_FM_K"), 0), eval_blocks = number(study_env("TDV_LM_EVAL_BLOCKS"), 4096);
    static const bool early = study_env("TDV_FM_NO_EARLY_EXIT") == nullptr;
    const char* lm = getenv("TDV_FM_LEAFMAJOR");
    FmKnobs k;
    k.brute = getenv("TDV_FM_BRUTE") != nullptr; k.walk_only = lm && atoi(lm) == 0;
    k.keyorder = study_env("TDV_FM_KEYORDER") != nullptr; k.stats = study_env("TDV_FM_STATS") != nullptr;
    k.lm_rounds = number(study_env("TDV_LM_ROUNDS"), 1) == 2 ? 2 : 1;
    k.leaf_limit = leaf_limit; k.heavy_groups = heavy_groups; k.force_k = force_k; k.eval_blocks = eval_blocks; k.early = early;
    return k;
}

// "This call uses the index" (tdv_internal.hpp): targets worth indexing and no switch that asks for another search; enough
// sources to pay for locating and ordering them.
constexpr int FM_INDEX_MIN_TARGETS = 2048, FM_INDEX_MIN_SOURCES = 4096;
bool fm_wants_index(int nt) { const FmKnobs k = fm_knobs(); return nt >= FM_INDEX_MIN_TARGETS && !k.brute && !k.keyorder; }
bool fm_indexes_sources(int ns) { return ns >= FM_INDEX_MIN_SOURCES; }

// A scan's second grid dimension: n items (targets, or boxes of them) cut so that blocks_x * splits comes to about want_blocks
// workgroups, at least min_per_split items in a split, at most max_splits of them: `asked`.  nsplit = the splits of per_split items
// that hold something.
struct ScanSplits { int asked, nsplit, per_split; };
static ScanSplits scan_splits(int blocks_x, int n, int want_blocks, int min_per_split, int max_splits) {
    if (n <= 0) return ScanSplits{0, 0, 0};
    const int want = (want_blocks + blocks_x - 1) / blocks_x;
    const int asked = std::max(1, std::min(std::min(want, std::max(1, n / min_per_split)), max_splits));
    const int per_split = (n + asked - 1) / asked;
    return ScanSplits{asked, (n + per_split - 1) / per_split, per_split};
}

// The plain scan over every target.  Part 0: the first FM_SEED targets in one split; its exact best seeds the bound of every later
// split.  EARLY = false (study build, TDV_FM_NO_EARLY_EXIT): everything in one launch without bounds.
template <bool EARLY>
static int fm_scan_all(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr) {
    hipStream_t s = ctx->stream;
    const int ns_pad = (int)align_up((size_t)ns, FM_SRC_PER_BLOCK), blocks_x = ns_pad / FM_SRC_PER_BLOCK;
    const int n_seed = EARLY ? std::min(nt, FM_SEED) : 0;
    const ScanSplits sp = scan_splits(blocks_x, nt - n_seed, 4096, 64, 64);
    const int nparts = sp.nsplit + (n_seed ? 1 : 0);
    float* pd; int* pj;
    TDV_TRY(ws_alloc(ctx, (size_t)nparts * ns_pad, &pd));
    TDV_TRY(ws_alloc(ctx, (size_t)nparts * ns_pad, &pj));
    {
        ScopedTimer tm(ctx, TDV_TIMER_FEATURE_MATCH);
        if constexpr (EARLY) {
            k_feature_match_scan<true, true><<<dim3(blocks_x, 1), FM_BLOCK, 0, s>>>(d_fs, ns, ns_pad, d_ft, 0, n_seed, n_seed, nullptr, nullptr, 0, pd, pj);
            if (sp.nsplit)   // (ordering the sources by seed distance was measured: no gain on FPFH descriptors, so rows stay in place)
                k_feature_match_scan<true, true><<<dim3(blocks_x, sp.nsplit), FM_BLOCK, 0, s>>>(d_fs, ns, ns_pad, d_ft, n_seed, nt, sp.per_split, pd, nullptr, 0, pd + ns_pad, pj + ns_pad);
        } else {
            k_feature_match_scan<false, true><<<dim3(blocks_x, sp.nsplit), FM_BLOCK, 0, s>>>(d_fs, ns, ns_pad, d_ft, 0, nt, sp.per_split, nullptr, nullptr, 0, pd, pj);
        }
    }
    k_feature_match_combine<<<(ns + 255) / 256, 256, 0, s>>>(ns, ns_pad, nparts, pd, pj, d_corr);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// ---- one indexed call: locate and order the sources; the leaf-major search; where that does not answer, the walk ----------
struct FmZeroed {          // what one memset clears before the sources are located
    int hist[FMP_BUCKETS], cursor[FMP_BUCKETS];   // sources per bucket of home leaves (bucket = leaf up to FMP_BUCKETS leaves); k_fm_scatter's write positions
    int overflow_count[2];                        // the walk: waves given up to pass B, waves given up to the scan class
    unsigned amax_s; int unused;                  // largest |x_d - mean_d| over the sources, as float bits
};
static_assert(sizeof(FmZeroed) == ((size_t)2 * FMP_BUCKETS + 4) * 4, "one memset: hist | cursor | overflow_count[2] | amax_s");
struct FmRun {             // the call's arguments and switches, and what it allocated
    tdv_ctx* ctx; const FmIndex& ix; const float* fs; int ns; int* corr; FmKnobs knobs;
    int bucket_shift = 0;          // home leaf -> bucket of the ordering's histogram
    FmZeroed* z = nullptr;
    int *home = nullptr, *bucket_of = nullptr, *sperm = nullptr, *start = nullptr, *d_total = nullptr;   // per source: home leaf, its bucket; the search order; bucket starts
    float* sp = nullptr;           // [ns][4]: the sources' principal coordinates
    // the walk's hand-over: the wave starts given up to pass B | to the scan class (one array, the second list fm_scan_class_offset
    // into it), the scan class once more as sources, pass A's partial answers
    int *overflow_walk = nullptr, *overflow_scan = nullptr, *overflow_src = nullptr, *part_j = nullptr; float* part_d = nullptr;
};
static int fm_alloc(FmRun& r) {
    tdv_ctx* ctx = r.ctx; const size_t ns = (size_t)r.ns;
    while ((r.ix.nleaf >> r.bucket_shift) > FMP_BUCKETS) ++r.bucket_shift;
    TDV_TRY(ws_alloc(ctx, 1, &r.z));
    TDV_TRY(ws_alloc(ctx, 2 * ns + 8, &r.overflow_walk));
    r.overflow_scan = r.overflow_walk + fm_scan_class_offset(r.ns);
    TDV_TRY(ws_alloc(ctx, ns + 8, &r.overflow_src));
    TDV_TRY(ws_alloc(ctx, ns, &r.part_d));
    TDV_TRY(ws_alloc(ctx, ns, &r.part_j));
    TDV_TRY(ws_alloc(ctx, ns * 4, &r.sp));
    TDV_TRY(ws_alloc(ctx, ns, &r.home));
    TDV_TRY(ws_alloc(ctx, ns, &r.bucket_of));
    TDV_TRY(ws_alloc(ctx, ns, &r.sperm));
    TDV_TRY(ws_alloc(ctx, (size_t)FMP_BUCKETS + 1, &r.start));
    return ws_alloc(ctx, 1, &r.d_total);
}
// Step 1: every source's home leaf (its cell of the target packing), and the search order: the sources sorted by home leaf.
static int fm_locate_and_order(FmRun& r) {
    tdv_ctx* ctx = r.ctx; hipStream_t s = ctx->stream; const FmIndex& ix = r.ix; const int ns = r.ns;
    TDV_HIP(ctx, hipMemsetAsync(r.z, 0, sizeof(FmZeroed), s));
    k_fm_locate<<<(ns + 255) / 256, 256, 0, s>>>(r.fs, ns, ix.basis, ix.S0, ix.S1, ix.b0, ix.b1, ix.col_leaf0, ix.leaf_p2, r.bucket_shift, r.home, r.bucket_of, r.sp, &r.z->amax_s);
    const int sblocks = (ns + FMP_SORT_BLOCK - 1) / FMP_SORT_BLOCK;
    k_fm_bucket_hist<<<sblocks, FMP_SORT_BLOCK, 0, s>>>(r.bucket_of, ns, r.z->hist);
    TDV_TRY(exclusive_scan_dev(ctx, r.z->hist, FMP_BUCKETS, r.start, r.d_total));
    k_fm_scatter<<<sblocks, FMP_SORT_BLOCK, 0, s>>>(r.bucket_of, ns, r.start, r.z->cursor, r.sperm);
    return TDV_OK;
}
static FmTables fm_tables(const FmRun& r, const float* fs2) {
    const FmIndex& ix = r.ix;
    FmTables t;
    t.fs = r.fs; t.sperm = r.sperm; t.home_of = r.home; t.ns = r.ns; t.fs2 = fs2;
    t.T = ix.T; t.torig = ix.torig; t.nleaf = ix.nleaf; t.ngroup = ix.ngroup;
    t.lbox = ix.lbox; t.gbox = ix.gbox; t.pbox = ix.pbox; t.gpbox = ix.gpbox;
    t.sp = r.sp; t.amax_t = ix.amax; t.amax_s = &r.z->amax_s; t.pscale = ix.pscale;
    return t;
}

// Step 2, the leaf-major search.  What one memset clears for it: per round of box tests [LM_POOLS][nleaf] pool_count | [LM_POOLS]
// entry_cursor | overflow (two rounds: the second is the study build's), then round 0's overflow word.  The sizes depend on nleaf, so
// instead of a struct with a static_assert this is the one place that knows the offsets.
struct LmZeroed {
    int* base; int nleaf;
    size_t per_round() const { return (size_t)LM_POOLS * nleaf + LM_POOLS + 1; }
    size_t words() const { return 2 * per_round() + 1; }
    int* pool_count(int round) const { return base + (size_t)(round - 1) * per_round(); }     // round = 1, 2
    int* entry_cursor(int round) const { return pool_count(round) + (size_t)LM_POOLS * nleaf; }
    int* overflow(int round) const { return round == 0 ? base + 2 * per_round() : entry_cursor(round) + LM_POOLS; }
};
struct LmRun {
    LmZeroed z; size_t pair_cap, pool_cap, unit_cap;
    int4* entries; int *sorted_src, *leaf_count, *pool_start, *leaf_start, *unit_start, *unit_leaf; unsigned long long* keys;
    unsigned long long* d_stats;       // study build, TDV_FM_STATS: [2][8] (k_lm_boxes)
};
// The lists of one round.  Round 0 (every source against its home leaf): the search order is sorted by home leaf, so it IS the
// sorted pair list, and the histogram the ordering made is the count per leaf.
static LmLists lm_lists(const FmRun& r, const LmRun& m, int round) {
    LmLists L{};
    L.overflow = m.z.overflow(round); L.keys = m.keys;
    L.leaf_start = m.leaf_start; L.unit_start = m.unit_start; L.unit_leaf = m.unit_leaf; L.unit_cap = (int)m.unit_cap;
    if (round == 0) { L.leaf_count = r.z->hist; L.sorted_src = r.sperm; L.pair_cap = INT_MAX; return L; }
    L.pool_count = m.z.pool_count(round); L.entry_cursor = m.z.entry_cursor(round); L.pool_start = m.pool_start;
    L.entries = m.entries; L.pool_cap = (int)m.pool_cap;
    L.leaf_count = m.leaf_count; L.sorted_src = m.sorted_src; L.pair_cap = (int)m.pair_cap;
    return L;
}

// Step 3, the walk.  Pass A over every source, then the sources it gave up on: few of them -> pass B (8 waves each on the packed
// index); many of them (descriptors without structure, or a plateau of near-identical rows: no box can exclude anything) -> the
// plain scan over just those sources, seeded with pass A's distances, which is the efficient way to do brute force.
// K sources per wave: 2.  K = 1 / 4 and STATS are instantiated by the study build alone (fmatch_study.hpp).
int fm_walk_report(tdv_ctx* ctx, const FmTables& t, int K, const unsigned long long* d_stats, int n_b, int n_scan);   // fmatch_study.hpp
template <int K, bool STATS>
static int fm_walk(FmRun& r) {
    tdv_ctx* ctx = r.ctx; hipStream_t s = ctx->stream; const FmIndex& ix = r.ix;
    float* fs2 = nullptr;
    if constexpr (K % 2 == 0) {
        const size_t n2 = ((size_t)r.ns + K - 1) / K * K * FD;
        TDV_TRY(ws_alloc(ctx, n2, &fs2));
        k_fm_interleave_rows<<<(unsigned)((n2 + 255) / 256), 256, 0, s>>>(r.fs, r.sperm, r.ns, K, fs2);
    }
    const FmTables t = fm_tables(r, fs2);
    int* overflow_count = r.z->overflow_count;
    const int waves = (t.ns + K - 1) / K;
    const int blocks_per_xcd = ((waves + FM_BLOCK / 64 - 1) / (FM_BLOCK / 64) + 7) / 8, blocks = blocks_per_xcd * 8;
    unsigned long long* d_stats = nullptr;
    if constexpr (STATS) { TDV_TRY(ws_alloc(ctx, 12, &d_stats)); TDV_HIP(ctx, hipMemsetAsync(d_stats, 0, 96, s)); }
    k_fm_query<K, STATS><<<blocks, FM_BLOCK, 0, s>>>(t, blocks_per_xcd, r.knobs.leaf_limit, r.knobs.heavy_groups, overflow_count, r.overflow_walk, r.overflow_src, r.part_d, r.part_j, r.corr, d_stats);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(pin_reserve(ctx, 256));
    int* h_over = reinterpret_cast<int*>(ctx->pin);
    TDV_HIP(ctx, hipMemcpyAsync(h_over, overflow_count, 8, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    const int n_b = h_over[0], n_scan = h_over[1];
    // the scan only pays when it has enough sources to fill the chip; a handful of outliers is cheaper on pass B
    const bool scan_them = (long long)n_scan * K >= 2048;
    for (int cls = 0; cls < 2; ++cls) {
        const int n = cls == 0 ? n_b : (scan_them ? 0 : n_scan);
        if (n > 0) k_fm_query_overflow<K, STATS><<<std::min(n, 1024), FMB_WAVES * 64, 0, s>>>(t, overflow_count + cls, cls ? r.overflow_scan : r.overflow_walk, r.part_d, r.part_j, r.corr, d_stats);
    }
    if (n_scan > 0 && scan_them) {
        const int n_list = n_scan * K;
        const int ns_pad = (int)align_up((size_t)t.ns, FM_SRC_PER_BLOCK), blocks_x = (n_list + FM_SRC_PER_BLOCK - 1) / FM_SRC_PER_BLOCK;
        const ScanSplits sp = scan_splits(blocks_x, ix.nt, 6144, 128, 256);   // few sources: many target splits, or the chip stays empty
        float* pd; int* pj;
        TDV_TRY(ws_alloc(ctx, (size_t)sp.nsplit * ns_pad, &pd));
        TDV_TRY(ws_alloc(ctx, (size_t)sp.nsplit * ns_pad, &pj));
        k_feature_match_scan<true, false><<<dim3(blocks_x, sp.nsplit), FM_BLOCK, 0, s>>>(t.fs, t.ns, ns_pad, ix.ft, 0, ix.nt, sp.per_split, r.part_d, r.overflow_src, n_list, pd, pj);
        k_feature_match_combine_list<<<(n_list + 255) / 256, 256, 0, s>>>(r.overflow_src, n_list, t.ns, ns_pad, sp.nsplit, pd, pj, r.corr);
    }
    TDV_CHECK_LAUNCH(ctx);
    if constexpr (STATS) TDV_TRY(fm_walk_report(ctx, t, K, d_stats, n_b, n_scan));
    return TDV_OK;
}

#ifdef TDV_STUDY
#include "fmatch_study.hpp"     // the key-ordered scan, the K = 1 / 4 walks, the second round of box tests, the statistics reports
#endif

// *done = false: the pair pool ran over (descriptors without structure) - the caller walks the index instead.  One synchronisation,
// like the walk.  One round of box tests after the home leaves: 12.1 pairs per source at 143k x 151k.  (Study build, TDV_LM_ROUNDS=2:
// 9.7 pairs per source, but a second set of launches: 0.525 against 0.487 ms.)
static int fm_leaf_major(FmRun& r, bool* done) {
    tdv_ctx* ctx = r.ctx; hipStream_t s = ctx->stream; const FmIndex& ix = r.ix;
    *done = false;
    const int nleaf = ix.nleaf, ns = r.ns, waves = (ns + 63) / 64;
    LmRun m{};
    m.z.nleaf = nleaf;
    m.pair_cap = (size_t)LM_PAIRS_PER_SOURCE * (size_t)ns + 4096;
    m.pool_cap = ((size_t)ns + 4096) / LM_POOLS + 64;     // entries: one box x up to 64 sources each
    if (m.pair_cap > (size_t)INT_MAX / 2) return TDV_OK;
    m.unit_cap = m.pair_cap / 64 + (size_t)nleaf + 2;
    TDV_TRY(ws_alloc(ctx, m.z.words(), &m.z.base));
    TDV_TRY(ws_alloc(ctx, m.pool_cap * LM_POOLS, &m.entries));
    TDV_TRY(ws_alloc(ctx, m.pair_cap, &m.sorted_src));
    TDV_TRY(ws_alloc(ctx, (size_t)nleaf, &m.leaf_count));
    TDV_TRY(ws_alloc(ctx, (size_t)LM_POOLS * nleaf, &m.pool_start));
    TDV_TRY(ws_alloc(ctx, (size_t)nleaf + 1, &m.leaf_start));
    TDV_TRY(ws_alloc(ctx, (size_t)nleaf + 1, &m.unit_start));
    TDV_TRY(ws_alloc(ctx, m.unit_cap, &m.unit_leaf));
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &m.keys));
    TDV_TRY(pin_reserve(ctx, 256));
    int* h_flag = reinterpret_cast<int*>(ctx->pin);
    h_flag[0] = 1;
    TDV_HIP(ctx, hipMemsetAsync(m.z.base, 0, m.z.words() * 4, s));
    const FmTables t = fm_tables(r, nullptr);
    if (r.knobs.stats) { TDV_TRY(ws_alloc(ctx, 16, &m.d_stats)); TDV_HIP(ctx, hipMemsetAsync(m.d_stats, 0, 128, s)); }
    const int rounds = ix.ngroup > 1 ? r.knobs.lm_rounds : 1;
    const LmLists L0 = lm_lists(r, m, 0);
    k_lm_plan<false><<<1, 1024, 0, s>>>(L0, nleaf);
    k_lm_eval<true><<<r.knobs.eval_blocks, 64 * LM_WAVES, 0, s>>>(t, L0);
    for (int round = 1; round <= rounds; ++round) {
        const LmLists L = lm_lists(r, m, round);
        if (rounds == 1 && ix.ngroup > 1) k_lm_boxes<3><<<waves, 64 * LM_BOX_WAVES, 0, s>>>(t, ix.sleaf, ix.sgroup, L, m.d_stats);      // every group, group boxes first
        else if (round == 1) k_lm_boxes<1><<<waves, 64 * LM_BOX_WAVES, 0, s>>>(t, ix.sleaf, ix.sgroup, L, m.d_stats);                   // a single group (or the first of two rounds): the home groups' leaves
#ifdef TDV_STUDY
        else lm_study_second_round(s, t, ix, L, waves, m.d_stats);
#endif
        k_lm_plan<true><<<1, 1024, 0, s>>>(L, nleaf);
        k_lm_scatter<<<LM_POOLS, 1024, (size_t)nleaf * 4, s>>>(L, nleaf);
        k_lm_eval<false><<<r.knobs.eval_blocks, 64 * LM_WAVES, 0, s>>>(t, L);
    }
    k_lm_finish<<<(ns + 255) / 256, 256, 0, s>>>(m.keys, ns, m.z.overflow(1), m.z.overflow(2), r.corr, h_flag);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipStreamSynchronize(s));
    *done = h_flag[0] == 0;
#ifdef TDV_STUDY
    if (m.d_stats) TDV_TRY(lm_study_report(r, m));
#endif
    return TDV_OK;
}

int feature_match_indexed_dev(tdv_ctx* ctx, const float* d_fs, int ns, const FmIndex& ix, int* d_corr) {
    if (!ctx || !d_fs || !d_corr || ns < 0) return TDV_ERR_BAD_ARG;
    if (ns == 0) return TDV_OK;
    FmRun r{ctx, ix, d_fs, ns, d_corr, fm_knobs()};
    TDV_TRY(fm_alloc(r));
    ScopedTimer tm(ctx, TDV_TIMER_FEATURE_MATCH);
    TDV_TRY(fm_locate_and_order(r));
    if (!r.knobs.walk_only && ix.sleaf && r.bucket_shift == 0) {     // (bucket_shift: more than 16,384 leaves - the ordering's histogram is then not per leaf)
        bool done = false;
        TDV_TRY(fm_leaf_major(r, &done));
        if (done) { ctx->last_fm_path = TDV_FM_PATH_LEAF_MAJOR; return TDV_OK; }
    }
    ctx->last_fm_path = TDV_FM_PATH_WALK;
#ifdef TDV_STUDY
    return fm_study_walk(r);
#else
    return fm_walk<2, false>(r);
#endif
}

int feature_match_dev(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr) {
    if (!ctx || !d_fs || !d_ft || !d_corr || ns < 0 || nt < 0) return TDV_ERR_BAD_ARG;
    if (ns == 0) return TDV_OK;
    if (nt == 0) { TDV_HIP(ctx, hipMemsetAsync(d_corr, 0, (size_t)ns * 4, ctx->stream)); return TDV_OK; }
    ctx->last_fm_path = TDV_FM_PATH_SCAN;
    if (fm_indexes_sources(ns) && fm_wants_index(nt)) {
        FmIndex ix;
        TDV_TRY(fm_index_build(ctx, d_ft, nt, &ix));
        return feature_match_indexed_dev(ctx, d_fs, ns, ix, d_corr);
    }
#ifdef TDV_STUDY
    bool answered = false;
    const int rc = fm_study_match(ctx, d_fs, ns, d_ft, nt, d_corr, &answered);      // the key-ordered scan, the scan without early exit
    if (answered) return rc;
#endif
    return fm_scan_all<true>(ctx, d_fs, ns, d_ft, nt, d_corr);
}

}  // namespace tdv
