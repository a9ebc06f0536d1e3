// The searches over a SortedCloud (tdv_internal.hpp; knn.hip builds it: spatial_sort_cloud), one wave per query.  Every kernel that looks
// for a point's neighbours goes through this header: it takes the descriptor by value and uses
//   d2_point / d2_box_bound   the distance of two points and its exact lower bound against a box, in one of two expression trees;
//   walk_in_order             the two-level walk in curve order at a fixed radius: 64 group boxes per step, one per lane, then the 64
//                             leaves of a group that passes (cluster.hip, outlier.hip's radius count, iss.hip);
//   query_wave_collect        a query's sorted neighbour row (k_query_wave in knn.hip: the lists of normals and FPFH; k_outlier_mean and
//                             k_iss_nn take their figure from the row while it is still in the wave).  Its bound drops as the row fills
//                             and its seeded kNN start visits a group's leaves nearest first: a loop of its own, as is the best-first
//                             group loop of ICP's pruned search (icp.hip).  Both use only the descriptor and the bound.
// Device code only, compiled without contraction (the library's -ffp-contract=off).
#pragma once
#include "tdv_internal.hpp"
#include <cmath>

namespace tdv {

// XCD-aware block order (cdna_hip_programming.md T1, bijective form): workgroups are dealt round-robin over the 8
// XCDs, so block b of the launch takes the logical position that gives every XCD one CONTIGUOUS eighth of the curve-
// ordered work: the rows a workgroup gathers are then mostly in its own XCD's 4 MiB L2.  A speed choice only.
__device__ __forceinline__ int xcd_contiguous_block(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = b & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// The two expression trees a squared distance is summed in: the reference's x + (y + z) (registration.cpp: kNN, radius lists, ICP) and
// (x + y) + z (include/tdv_hip.h: tdv_cluster_dbscan rule 1, which the outlier radius filter and ISS share).
enum class D2 { REF, DBSCAN };
template <D2 TREE>
__device__ __forceinline__ float d2_sum(float x, float y, float z) { return TREE == D2::REF ? x + (y + z) : (x + y) + z; }

// d2 between the points p and q
template <D2 TREE>
__device__ __forceinline__ float d2_point(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return d2_sum<TREE>(dx * dx, dy * dy, dz * dz);
}

// Lower bound of d2_point<TREE> between q and ANY point inside box idx of a [6][count] box array: per-axis gaps by one f32 subtraction
// each, then the SAME expression tree.  f32 subtraction, multiplication and addition are monotone under round-to-nearest, so term by term
// and sum by sum the bound never exceeds the fl(d2) of a point in the box: no margin is needed, and "bound > B" proves that nothing in
// the box passes "d2 <= B".  That argument runs along one tree, which is why the bound takes the tree of the distance it guards: against
// the other tree's d2 it could come out one rounding too high.  NaN gaps count as 0 (fmaxf): such a box is looked at.
template <D2 TREE>
__device__ __forceinline__ float d2_box_bound(const float* __restrict__ box, int count, int idx, float qx, float qy, float qz) {
    const float q[3] = {qx, qy, qz};
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float bmin = box[(size_t)a * count + idx], bmax = box[(size_t)(3 + a) * count + idx];
        g[a] = fmaxf(0.f, fmaxf(bmin - q[a], q[a] - bmax));
    }
    return d2_sum<TREE>(g[0] * g[0], g[1] * g[1], g[2] * g[2]);
}

// The two-level walk in curve order at a fixed bound: visit(leaf) for every leaf whose box may hold a point with d2_point<TREE> <= bound
// of q, until it returns true.  64 group boxes per step, one per lane, then the 64 leaves of a group that passes.  Wave-uniform control
// flow.  (query_wave_collect keeps a loop of its own: its bound drops as the row fills.  Run through this function, then with a leaf
// range and a re-test of a dropped bound, the radius lists' k_query_wave<4> took 427 us against the parent's 383 us at 200k points:
// profiles/r16/sorted_cloud_descriptor.md, section 3.)
template <D2 TREE, class Visit>
__device__ __forceinline__ void walk_in_order(const SortedCloud& c, float qx, float qy, float qz, float bound, int lane, Visit&& visit) {
    for (int tb = 0; tb < c.n_top; tb += 64) {
        const int t = tb + lane;
        unsigned long long tmask = __ballot(t < c.n_top && d2_box_bound<TREE>(c.tbox, c.n_top, min(t, c.n_top - 1), qx, qy, qz) <= bound);
        while (tmask) {
            const int bt = __ffsll((long long)tmask) - 1;
            tmask &= tmask - 1;
            const int u = (tb + bt) * 64 + lane;
            unsigned long long lmask = __ballot(u < c.n_leaf && d2_box_bound<TREE>(c.lbox, c.n_leaf, min(u, c.n_leaf - 1), qx, qy, qz) <= bound);
            while (lmask) {
                const int bl = __ffsll((long long)lmask) - 1;
                lmask &= lmask - 1;
                if (visit((tb + bt) * 64 + bl)) return;
            }
        }
    }
}

// ------------------------------------------------------------------ one wave per query: walk, collect, select
#ifndef QW_WAVES_VALUE
#define QW_WAVES_VALUE 1
#endif
constexpr int QW_WAVES = QW_WAVES_VALUE;   // queries (waves) per workgroup of k_query_wave (measured kNN 200k: 1: 0.383 ms, 4: 0.401, 16: 0.487)
// kNN start, measured at 50k/100k/200k (k = 30): own leaf only 0.55/0.55/1.00 ms; own leaf +-1 0.23/0.41/0.61; with nearest-leaf-first
// inside a group 0.19/0.37/0.67 (kept: it also protects clouds of uneven density); +-2 leaves no better
constexpr int QW_SEED_SPAN = 1;
constexpr bool QW_BEST_FIRST = true;

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int j) {
    const unsigned lo = __shfl_xor((unsigned)v, j, 64), hi = __shfl_xor((unsigned)(v >> 32), j, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// Ascending bitonic sort of the first NSORT (64, 128, ... 64*R) keys of a wave; element i = r*64 + lane.  The
// network is fully unrolled (compile-time strides: the exchanges become DPP / swizzle / permute with constant
// patterns and the direction masks fold to one bit test each).  Keys are distinct (distinct indices) except the ~0
// padding, which sorts last.
template <int R, int NSORT>
__device__ __forceinline__ void wave_sort_keys_fixed(unsigned long long (&key)[R], int lane) {
#pragma unroll
    for (int kk = 2; kk <= NSORT; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j >= 1; j >>= 1) {
            if (j >= 64) {   // partner is another key of the same lane
                const int dr = j >> 6;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if ((r & dr) != 0 || (r + dr) * 64 >= NSORT) continue;
                    const bool asc = ((r * 64) & kk) == 0;   // kk >= 128 here: the bit lies in r, not in the lane
                    const bool swap = asc == (key[r + dr] < key[r]);
                    const unsigned long long a = key[r], c = key[r + dr];
                    key[r] = swap ? c : a;
                    key[r + dr] = swap ? a : c;
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r * 64 >= NSORT) continue;
                    const unsigned long long other = shfl_xor_u64(key[r], j);
                    const bool keep_min = ((((r * 64) | lane) & kk) == 0) == ((lane & j) == 0);
                    key[r] = ((other < key[r]) == keep_min) ? other : key[r];
                }
            }
        }
    }
}
template <int R>
__device__ __forceinline__ void wave_sort_keys(unsigned long long (&key)[R], int m, int lane) {
    // the span is wave-uniform: the smallest power-of-two multiple of 64 that holds m keys
    if (m <= 64) wave_sort_keys_fixed<R, 64>(key, lane);
    else if (R >= 2 && m <= 128) wave_sort_keys_fixed<R, (R >= 2 ? 128 : 64)>(key, lane);
    else if (R >= 4 && m <= 256) wave_sort_keys_fixed<R, (R >= 4 ? 256 : 64)>(key, lane);
    else wave_sort_keys_fixed<R, 64 * R>(key, lane);
}

// row[0..m) -> registers, sorted ascending
template <int R>
__device__ __forceinline__ void load_sort_row(const unsigned long long* row, int m, int lane, unsigned long long (&key)[R]) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the row was written by other lanes of this wave
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = r * 64 + lane;
        key[r] = e < m ? row[e] : ~0ull;
    }
    wave_sort_keys<R>(key, m, lane);
}

// The search of one query by one wave: walks the cloud for the query at sorted position sp, collects into `row` (LDS, 64 * R keys of
// this wave) every target with d2 <= the bound (bound0 at the start; it drops to the k-th as the row fills) and leaves the row sorted in
// `key` (element e = r * 64 + lane; 64-bit keys d2 bits : tie-break id, ~0 past the end).  Returns the number of keys found (it may
// exceed k: the first min(k, found) are the list).  Requires k <= 64 * R - 64.  Wave-uniform control flow; no block-level barrier.
// OPTIONAL = false: the caller's cloud is a single cloud whose ties break by original index (spatial_sort_cloud's, as it comes): the
// descriptor's okey and inst_leaf are not looked at, and neither branch is compiled in.
template <int R, int SEED_SPAN, bool BEST_FIRST, bool OPTIONAL = true>
__device__ __forceinline__ int query_wave_collect(const SortedCloud& c, int sp, float bound0, int seed_own, int k,
                                                  unsigned long long* row, int lane, unsigned long long (&key)[R]) {
    constexpr int ROW = 64 * R;
    const float qx = c.sx[sp], qy = c.sy[sp], qz = c.sz[sp];
    const int* okey = OPTIONAL ? c.okey : nullptr;
    const int* inst_leaf = OPTIONAL ? c.inst_leaf : nullptr;
    float B = bound0;                         // wave-uniform; only ever decreases
    int wcnt = 0;                             // wave-uniform fill of the row

    // keep the best k of the row (needs wcnt >= k) and drop the bound to the k-th.  No sort: the k-th smallest key is
    // found by bisection on its bits with ballot counts (distance bits first, then — only when several candidates tie
    // at that distance — the index bits), and the survivors are packed by ballot prefix.
    auto compact = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned hi[R], lo[R]; bool has[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = r * 64 + lane;
            has[r] = e < wcnt;
            const unsigned long long key = has[r] ? row[e] : ~0ull;
            hi[r] = (unsigned)(key >> 32); lo[r] = (unsigned)key;
        }
        auto count_if = [&](auto pred) {
            int cnt = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) cnt += __popcll(__ballot(has[r] && pred(r)));
            return cnt;
        };
        unsigned kd = 0;   // k-th smallest distance bits: count(hi < kd) < k <= count(hi <= kd)
        for (int b = 31; b >= 0; --b) {
            const unsigned cand = kd | (1u << b);
            if (count_if([&](int r) { return hi[r] < cand; }) < k) kd = cand;
        }
        const int below = count_if([&](int r) { return hi[r] < kd; });
        unsigned ki = 0xffffffffu;   // among the candidates AT that distance keep the (k - below) lowest indices
        if (count_if([&](int r) { return hi[r] <= kd; }) > k) {
            ki = 0;
            const int need = k - below;
            for (int b = 31; b >= 0; --b) {
                const unsigned cand = ki | (1u << b);
                if (count_if([&](int r) { return hi[r] == kd && lo[r] < cand; }) < need) ki = cand;
            }
        }
        int base = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool keep = has[r] && (hi[r] < kd || (hi[r] == kd && lo[r] <= ki));
            const unsigned long long km = __ballot(keep);
            if (keep) row[base + __popcll(km & ((1ull << lane) - 1ull))] = ((unsigned long long)hi[r] << 32) | lo[r];
            base += __popcll(km);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        wcnt = base;   // == k
        B = __uint_as_float(kd);
    };
    // the 64 targets of one leaf, one per lane
    auto eval_leaf = [&](int leaf) {
        const int pidx = leaf * 64 + lane;   // arrays are padded with +inf to a multiple of 256
        const float d2 = d2_point<D2::REF>(c.sx[pidx], c.sy[pidx], c.sz[pidx], qx, qy, qz);   // (points[i] - query)
        bool acc = pidx < c.n && d2 <= B;
        unsigned long long am = __ballot(acc);
        if (!am) return;
        if (wcnt + __popcll(am) > ROW) {   // the row cannot take them all (wcnt > ROW - 64 >= k)
            compact();
            acc = acc && d2 <= B;
            am = __ballot(acc);
            if (!am) return;
        }
        const int at = wcnt + __popcll(am & ((1ull << lane) - 1ull));
        if (acc) row[at] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)(okey ? okey[pidx] : c.orig[pidx]);
        wcnt += __popcll(am);
    };

    const int own = sp >> 6;
    // Several clouds in one array (the batch's small instances, each padded to whole leaves with NaN coordinates): the walk
    // stays inside the query's own cloud - boxes of other clouds are never looked at, whatever their coordinates.
    int l_lo = 0, l_hi = c.n_leaf;
    if (inst_leaf) {
        int a = 0, z = c.n_inst;
        while (z - a > 1) { const int m = (a + z) >> 1; if (inst_leaf[m] <= own) a = m; else z = m; }
        l_lo = inst_leaf[a]; l_hi = inst_leaf[a + 1];
    }
    const int seed_lo = seed_own ? max(l_lo, own - SEED_SPAN) : 1, seed_hi = seed_own ? min(l_hi - 1, own + SEED_SPAN) : 0;
    if (seed_own) {
        // unbounded start: the query's own leaf (its 64 curve neighbours) gives the first bound, its curve-adjacent
        // leaves follow; the walk skips them
        eval_leaf(own);
        if (wcnt >= k) compact();
        for (int l = seed_lo; l <= seed_hi; ++l) if (l != own) eval_leaf(l);
    }
    // Validity is tracked explicitly (never through "+inf <= bound"): the bound itself is +inf while an unbounded
    // search has seen fewer than k points, or for an unbounded radius.
    const int t_hi = inst_leaf ? ((l_hi - 1) >> 6) + 1 : c.n_top;
    for (int tb = inst_leaf ? (l_lo >> 6) : 0; tb < t_hi; tb += 64) {
        const int t = tb + lane;
        const bool t_valid = t < t_hi;
        const float lbt = t_valid ? d2_box_bound<D2::REF>(c.tbox, c.n_top, t, qx, qy, qz) : INFINITY;
        unsigned long long tmask = __ballot(t_valid && lbt <= B);
        while (tmask) {
            const int bt = __ffsll((long long)tmask) - 1;
            tmask &= tmask - 1;
            if (__shfl(lbt, bt, 64) > B) continue;   // the bound may have dropped since the test
            const int u = (tb + bt) * 64 + lane;
            bool pending = u >= l_lo && u < l_hi && !(u >= seed_lo && u <= seed_hi);   // a leaf of this group (and cloud) not evaluated yet
            const float lbl = pending ? d2_box_bound<D2::REF>(c.lbox, c.n_leaf, u, qx, qy, qz) : INFINITY;
            if (BEST_FIRST && seed_own) {
                while (true) {   // nearest leaf first: the bound tightens before the far leaves are looked at
                    const bool cand = pending && lbl <= B;
                    if (!__any(cand)) break;
                    float m = cand ? lbl : INFINITY;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
                    const int bl = __ffsll((long long)__ballot(cand && lbl == m)) - 1;
                    if (lane == bl) pending = false;
                    eval_leaf((tb + bt) * 64 + bl);
                }
            } else {                                     // walk_in_order's leaf loop, with the re-test of a dropped bound
                unsigned long long lmask = __ballot(pending && lbl <= B);
                while (lmask) {
                    const int bl = __ffsll((long long)lmask) - 1;
                    lmask &= lmask - 1;
                    if (__shfl(lbl, bl, 64) > B) continue;
                    eval_leaf((tb + bt) * 64 + bl);
                }
            }
        }
    }
    load_sort_row<R>(row, wcnt, lane, key);
    return wcnt;
}

}  // namespace tdv
