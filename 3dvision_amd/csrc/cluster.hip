// Euclidean clustering (DBSCAN) on gfx950: include/tdv_hip.h (tdv_cluster_dbscan) states every rule.
//
// Every output is an integer, and no step depends on the order in which the device works: the neighbour test is one f32 expression, the
// components are what a union-find ends with whatever the order of its unions, sizes are integer atomics, the numbering is a scan over
// the original index and the grouped order a stable sort.  The host enqueues everything up front and reads back at the end.
//  (i)   spatial_sort_cloud: the cloud along a Morton curve with the boxes of its 64-point leaves and 4096-point groups (knn.hip).
//  (ii)  k_cluster_count: one wave per query in curve order.  The walk tests 64 group boxes per step, then the 64 leaf boxes of a group
//        that passes, then a passing leaf's 64 points, one per lane, with a ballot and a popcount.  A box is skipped when an exact lower
//        bound of d2 over it (the same expression tree: no margin) exceeds eps2.  The walk ends once min_points are counted: only the
//        core flag leaves the kernel.
//  (iii) k_cluster_link: the same walk, to the end.  A core query unites itself with every core neighbour of lower index (the pair is
//        symmetric: the higher index of a pair does the work) in a lock-free union-find over `parent`, indexed by original index, that
//        always hooks the HIGHER root under the LOWER: parent[x] <= x throughout, every find strictly descends, and a component's final
//        root is its lowest core index.  Every access to parent in this kernel is an agent-scope atomic (load, compare-exchange, min);
//        no result depends on how fresh a read is: a stale parent is still an ancestor, and a failed compare-exchange finds again from
//        the value it saw, which is lower.  A non-core query keeps the minimum of (d2 bits << 32 | index) over its core neighbours.
//  (iv)  k_cluster_flatten (a launch of its own: parent is final): the root of every core point, the root flags, the core count.
//  (v)   exclusive_scan_dev over the root flags in original index: cluster ids in ascending order of the lowest core index.
//  (vi)  k_cluster_assign: the label of every point before the size filter, sizes by integer atomics, the border count.
//  (vii) k_cluster_keep + scan: the clusters of at least min_cluster_size members and their new ids; k_cluster_sizes + scan: offsets.
//  (viii) k_cluster_final: labels and the sort keys; k_cluster_result: the result record.
//  (ix)  radix_sort_pairs_dev (stable) on the label, noise last: the grouped order; k_cluster_gather: the grouped coordinates.
// Loops: the walk runs over box and leaf counts; a find descends (at most n steps); a unite retries only after another lane's
// successful hook of the root it held, and its two arguments never rise.  Nothing waits for another lane.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "sorted_cloud.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <algorithm>

namespace tdv {

namespace {

constexpr int CL_WAVES = 4;                        // queries (waves) per workgroup of the two walks
constexpr unsigned long long CL_NO_KEY = ~0ull;    // a non-core point without a core neighbour

// device state of one call (workspace), read back at the end
struct ClusterState {
    int n_found;      // clusters before the size filter
    int n_kept;       // clusters after it
    int n_labelled;   // members of the kept clusters
    int n_core, n_border, largest;
    tdv_cluster_result res;
};

// core_s[sorted position] and core[original index] = the point has at least min_points neighbours (itself included); parent[i] = i
__global__ __launch_bounds__(64 * CL_WAVES) void k_cluster_count(SortedCloud c, float eps2, int min_points, int* __restrict__ core_s,
                                                                  int* __restrict__ core, int* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const int sp = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    if (sp >= c.n) return;                                   // wave-uniform
    const float qx = c.sx[sp], qy = c.sy[sp], qz = c.sz[sp];
    int cnt = 0;
    // A query that is not its own neighbour (d2(q, q) is NaN: a NaN or infinite coordinate) has none: every d2 to it is NaN or +inf, and
    // eps2 is finite.  Its walk would pass every box (a NaN gap counts as 0) only to count nothing.
    if (d2_point<D2::DBSCAN>(qx, qy, qz, qx, qy, qz) <= eps2) walk_in_order<D2::DBSCAN>(c, qx, qy, qz, eps2, lane, [&](int leaf) {
        const int p = leaf * 64 + lane;                      // the arrays are padded to a multiple of 256
        const bool nb = p < c.n && d2_point<D2::DBSCAN>(c.sx[p], c.sy[p], c.sz[p], qx, qy, qz) <= eps2;
        cnt += __popcll(__ballot(nb));
        return cnt >= min_points;
    });
    if (lane == 0) {
        const int i = c.orig[sp], is_core = cnt >= min_points ? 1 : 0;
        core_s[sp] = is_core; core[i] = is_core; parent[i] = i;
    }
}

__device__ __forceinline__ int cluster_parent(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x as far as this lane can see, and the path from x pointed at it.  parent[y] <= y always, and a point that has a
// parent below itself never becomes a root again: the first loop strictly descends, the second runs over indices above r only.
__device__ __forceinline__ int cluster_find(int* parent, int x) {
    int r = x;
    for (;;) {
        const int p = cluster_parent(parent, r);
        if (p >= r) break;
        r = p;
    }
    while (x > r) {
        const int p = cluster_parent(parent, x);
        if (p >= x) break;
        if (p > r) atomicMin(parent + x, r);                 // r is an ancestor of x: so is whatever lies below parent[x] afterwards
        x = p;
    }
    return r;
}

// One component for a and b; returns a root of it as this lane saw it.  A compare-exchange fails only when another lane hooked the
// root `hi` in between; the retry starts from what that lane wrote, below hi.
__device__ __forceinline__ int cluster_unite(int* parent, int a, int b) {
    for (;;) {
        a = cluster_find(parent, a);
        b = cluster_find(parent, b);
        if (a == b) return a;
        const int hi = max(a, b), lo = min(a, b);
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        a = seen; b = lo;
    }
}

// core queries: unions with the core neighbours of lower index; the others: bkey[original index] = their nearest core neighbour's key
__global__ __launch_bounds__(64 * CL_WAVES) void k_cluster_link(SortedCloud c, float eps2, const int* __restrict__ core_s, int* parent,
                                                                 unsigned long long* __restrict__ bkey) {
    const int lane = threadIdx.x & 63;
    const int sp = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    if (sp >= c.n) return;                                   // wave-uniform
    const float qx = c.sx[sp], qy = c.sy[sp], qz = c.sz[sp];
    const int i = c.orig[sp];
    const bool is_core = core_s[sp] != 0;                    // wave-uniform
    int mine = i;                                            // an ancestor of i (core queries)
    unsigned long long best = CL_NO_KEY;                     // per lane (the others)
    if (d2_point<D2::DBSCAN>(qx, qy, qz, qx, qy, qz) <= eps2) walk_in_order<D2::DBSCAN>(c, qx, qy, qz, eps2, lane, [&](int leaf) {     // as in k_cluster_count
        const int p = leaf * 64 + lane;
        const float d2 = d2_point<D2::DBSCAN>(c.sx[p], c.sy[p], c.sz[p], qx, qy, qz);
        if (p < c.n && d2 <= eps2 && core_s[p]) {
            const int j = c.orig[p];
            if (is_core) {
                // j already hangs under this lane's root (the usual case once a neighbourhood is linked): one load, no find
                if (j < i && cluster_parent(parent, j) != mine) mine = cluster_unite(parent, mine, j);
            } else {
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j;
                best = key < best ? key : best;
            }
        }
        return false;
    });
    if (is_core) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)best, off, 64), hi = __shfl_xor((unsigned)(best >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        best = o < best ? o : best;
    }
    if (lane == 0) bkey[i] = best;
}

// sum over a workgroup of 256 into *dst (one integer atomic per workgroup)
__device__ __forceinline__ void cluster_block_count(int v, int* dst) {
    __shared__ int w[4];
    v = wave_sum_i32(v);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { const int s = (w[0] + w[1]) + (w[2] + w[3]); if (s) atomicAdd(dst, s); }
}

__global__ void k_cluster_init(ClusterState* st) {
    if (threadIdx.x != 0) return;
    ClusterState z{};
    *st = z;
}

// comp[i] = the root of core point i (-1 for the others); is_root[i]
__global__ __launch_bounds__(256) void k_cluster_flatten(const int* __restrict__ core, const int* __restrict__ parent, int n,
                                                         int* __restrict__ comp, int* __restrict__ is_root, ClusterState* st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    if (i < n) {
        c = core[i];
        int r = -1;
        if (c) { r = i; for (;;) { const int p = parent[r]; if (p >= r) break; r = p; } }
        comp[i] = r;
        is_root[i] = (c && r == i) ? 1 : 0;
    }
    cluster_block_count(c, &st->n_core);
}

// raw[i] = the cluster of point i before the size filter (-1: noise); size[cluster] += 1
__global__ __launch_bounds__(256) void k_cluster_assign(const int* __restrict__ core, const int* __restrict__ comp,
                                                        const unsigned long long* __restrict__ bkey, const int* __restrict__ cid, int n,
                                                        int* __restrict__ raw, int* __restrict__ size, ClusterState* st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int border = 0;
    if (i < n) {
        int from = -1;
        if (core[i]) from = i;
        else if (bkey[i] != CL_NO_KEY) { from = (int)(unsigned)bkey[i]; border = 1; }
        const int l = from < 0 ? -1 : cid[comp[from]];
        raw[i] = l;
        if (l >= 0) atomicAdd(size + l, 1);
    }
    cluster_block_count(border, &st->n_border);
}

// over c <= n: keep[c] = cluster c exists and has at least min_cluster_size members
__global__ __launch_bounds__(256) void k_cluster_keep(const int* __restrict__ size, const ClusterState* __restrict__ st, int n1,
                                                      int min_cluster_size, int* __restrict__ keep) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n1) keep[c] = (c < st->n_found && size[c] >= min_cluster_size) ? 1 : 0;
}

// kept_size[new id] = size (kept_size is zeroed before); the largest
__global__ __launch_bounds__(256) void k_cluster_sizes(const int* __restrict__ size, const int* __restrict__ keep, const int* __restrict__ newid,
                                                       int n1, int* __restrict__ kept_size, ClusterState* st) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n1 || !keep[c]) return;
    kept_size[newid[c]] = size[c];
    atomicMax(&st->largest, size[c]);
}

// labels (optional) and the sort's (key, value) = (label, noise as n_kept; original index)
__global__ __launch_bounds__(256) void k_cluster_final(const int* __restrict__ raw, const int* __restrict__ keep, const int* __restrict__ newid,
                                                       const ClusterState* __restrict__ st, int n, int* __restrict__ labels,
                                                       unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int l = raw[i];
    l = (l >= 0 && keep[l]) ? newid[l] : -1;
    if (labels) labels[i] = l;
    if (keys) { keys[i] = (unsigned long long)(unsigned)(l < 0 ? st->n_kept : l); vals[i] = (unsigned)i; }
}

__global__ void k_cluster_result(ClusterState* st, int n) {
    if (threadIdx.x != 0) return;
    tdv_cluster_result r;
    r.n_clusters = st->n_kept; r.n_core = st->n_core; r.n_border = st->n_border; r.n_noise = n - st->n_labelled;
    r.n_dropped = st->n_found - st->n_kept; r.largest = st->largest;
    st->res = r;
}

__global__ __launch_bounds__(256) void k_cluster_gather(const float* __restrict__ xyz, const int* __restrict__ order, int n, float* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const size_t j = (size_t)order[k];
    out[3 * (size_t)k] = xyz[3 * j]; out[3 * (size_t)k + 1] = xyz[3 * j + 1]; out[3 * (size_t)k + 2] = xyz[3 * j + 2];
}

// every argument, before anything is enqueued (include/tdv_hip.h: tdv_cluster_dbscan)
bool cluster_args_ok(const tdv_ctx* ctx, const float* xyz, int n, const tdv_cluster_params* p, const tdv_cluster_result* result,
                     const int* offsets, int capacity) {
    if (!ctx || !p || !result || n < 0 || (n > 0 && !xyz)) return false;
    if (capacity < 0 || (capacity > 0 && !offsets)) return false;
    if (!std::isfinite(p->eps) || !(p->eps > 0.f)) return false;
    return p->min_points >= 1 && p->min_cluster_size >= 1;
}

// The whole call on device memory.  h_labels / h_order / h_grouped (host, optional) receive d_labels / d_order / d_grouped.
int cluster_run_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_cluster_params& prm, tdv_cluster_result* result, int* d_labels,
                    int* d_order, float* d_grouped, int* offsets, int capacity, int* n_labelled, int* h_labels, int* h_order,
                    float* h_grouped) {
    if (n == 0) {
        std::memset(result, 0, sizeof(*result));
        if (offsets) offsets[0] = 0;
        if (n_labelled) *n_labelled = 0;
        return TDV_OK;
    }
    hipStream_t s = ctx->stream;
    const int n1 = n + 1, nb = (n + 255) / 256, nb1 = (n1 + 255) / 256;
    const bool want_order = d_order || d_grouped;
    ClusterState* st;
    int *core, *parent, *comp, *is_root, *cid, *raw, *size, *keep, *newid, *kept_size, *offs, *core_s;
    unsigned long long *bkey, *keys = nullptr, *keys_out = nullptr;
    unsigned* vals = nullptr;
    TDV_TRY(ws_alloc(ctx, 1, &st));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &core));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &parent));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &bkey));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &comp));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &is_root));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &cid));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &raw));
    TDV_TRY(ws_alloc(ctx, (size_t)2 * n1, &size));                 // size | kept_size: one memset
    kept_size = size + n1;
    TDV_TRY(ws_alloc(ctx, (size_t)n1, &keep));
    TDV_TRY(ws_alloc(ctx, (size_t)n1, &newid));
    TDV_TRY(ws_alloc(ctx, (size_t)n1, &offs));
    if (want_order) {
        TDV_TRY(ws_alloc(ctx, (size_t)n, &keys));
        TDV_TRY(ws_alloc(ctx, (size_t)n, &keys_out));
        TDV_TRY(ws_alloc(ctx, (size_t)n, &vals));
        if (!d_order) TDV_TRY(ws_alloc(ctx, (size_t)n, &d_order));
    }
    TDV_TRY(pin_reserve(ctx, sizeof(ClusterState) + (size_t)n1 * sizeof(int)));
    SortedCloud sc;
    TDV_TRY(spatial_sort_cloud(ctx, d_xyz, n, sc));
    TDV_TRY(ws_alloc(ctx, (size_t)sc.pad, &core_s));
    const float eps2 = std::min(prm.eps * prm.eps, FLT_MAX);    // finite: an infinite d2 never passes
    const int walk_blocks = (n + CL_WAVES - 1) / CL_WAVES;

    TDV_HIP(ctx, hipMemsetAsync(size, 0, (size_t)2 * n1 * sizeof(int), s));
    k_cluster_init<<<1, 64, 0, s>>>(st);
    k_cluster_count<<<walk_blocks, 64 * CL_WAVES, 0, s>>>(sc, eps2, prm.min_points, core_s, core, parent);
    k_cluster_link<<<walk_blocks, 64 * CL_WAVES, 0, s>>>(sc, eps2, core_s, parent, bkey);
    k_cluster_flatten<<<nb, 256, 0, s>>>(core, parent, n, comp, is_root, st);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(exclusive_scan_dev(ctx, is_root, n, cid, &st->n_found));
    k_cluster_assign<<<nb, 256, 0, s>>>(core, comp, bkey, cid, n, raw, size, st);
    k_cluster_keep<<<nb1, 256, 0, s>>>(size, st, n1, prm.min_cluster_size, keep);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(exclusive_scan_dev(ctx, keep, n1, newid, &st->n_kept));
    k_cluster_sizes<<<nb1, 256, 0, s>>>(size, keep, newid, n1, kept_size, st);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(exclusive_scan_dev(ctx, kept_size, n1, offs, &st->n_labelled));
    k_cluster_final<<<nb, 256, 0, s>>>(raw, keep, newid, st, n, d_labels, keys, vals);
    k_cluster_result<<<1, 64, 0, s>>>(st, n);
    TDV_CHECK_LAUNCH(ctx);
    if (want_order) {
        int end_bit = 1;
        while (end_bit < 31 && (1ll << end_bit) <= (long long)n) end_bit += 1;      // the key is at most n
        TDV_TRY(radix_sort_pairs_dev(ctx, keys, keys_out, vals, reinterpret_cast<unsigned*>(d_order), (size_t)n, end_bit));
        if (d_grouped) k_cluster_gather<<<nb, 256, 0, s>>>(d_xyz, d_order, n, d_grouped);
        TDV_CHECK_LAUNCH(ctx);
    }
    TDV_TRY(download(ctx, h_labels, d_labels, (size_t)n));
    TDV_TRY(download(ctx, h_order, d_order, (size_t)n));
    TDV_TRY(download(ctx, h_grouped, d_grouped, (size_t)n * 3));
    ClusterState hs;
    TDV_TRY(fetch_state(ctx, st, &hs));
    *result = hs.res;
    if (n_labelled) *n_labelled = hs.n_labelled;
    if (hs.n_kept > capacity) {
        snprintf(ctx->err, sizeof(ctx->err), "tdv_cluster_dbscan: %d clusters, offsets has room for %d", hs.n_kept, capacity);
        return TDV_ERR_BAD_ARG;
    }
    if (offsets) {
        int* h_offs = reinterpret_cast<int*>(ctx->pin + sizeof(ClusterState));
        TDV_TRY(download(ctx, h_offs, offs, (size_t)hs.n_kept + 1));
        TDV_TRY(finish(ctx));
        std::memcpy(offsets, h_offs, (size_t)(hs.n_kept + 1) * sizeof(int));
    }
    return TDV_OK;
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_cluster_default_params(tdv_cluster_params* p) {
    if (!p) return;
    p->eps = 0.f; p->min_points = 0; p->min_cluster_size = 1;
}

int tdv_cluster_dbscan(tdv_ctx* ctx, const float* xyz, int n, const tdv_cluster_params* params, tdv_cluster_result* result, int* labels,
                       int* order, float* grouped_xyz, int* offsets, int offsets_capacity, int* n_labelled) {
    if (!cluster_args_ok(ctx, xyz, n, params, result, offsets, offsets_capacity)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float *d_xyz, *d_grouped = nullptr;
    int *d_labels = nullptr, *d_order = nullptr;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    if (n > 0) {
        if (labels) TDV_TRY(ws_alloc(ctx, (size_t)n, &d_labels));
        if (order) TDV_TRY(ws_alloc(ctx, (size_t)n, &d_order));
        if (grouped_xyz) TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &d_grouped));
    }
    return cluster_run_dev(ctx, d_xyz, n, *params, result, d_labels, d_order, d_grouped, offsets, offsets_capacity, n_labelled, labels, order,
                           grouped_xyz);
}

int tdv_cluster_dbscan_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_cluster_params* params, tdv_cluster_result* result,
                           int* d_labels, int* d_order, float* d_grouped_xyz, int* offsets, int offsets_capacity, int* n_labelled) {
    if (!cluster_args_ok(ctx, d_xyz, n, params, result, offsets, offsets_capacity)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return cluster_run_dev(ctx, d_xyz, n, *params, result, d_labels, d_order, d_grouped_xyz, offsets, offsets_capacity, n_labelled, nullptr,
                           nullptr, nullptr);
}

}  // extern "C"
