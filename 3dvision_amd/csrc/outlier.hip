// Outlier removal on gfx950: include/tdv_hip.h (tdv_remove_statistical_outlier, tdv_remove_radius_outlier) states every rule.
//
// The host enqueues everything up front; nothing returns to it between the kernels, and the call reads back once, at the end.
// Statistical filter:
//  (i)   spatial_sort_cloud: the cloud along a Morton curve with the boxes of its leaves and groups (knn.hip).
//  (ii)  k_outlier_mean: ONE WAVE PER QUERY in curve order, the walk of k_query_wave (sorted_cloud.hpp: query_wave_collect).  When the walk ends the query's
//        sorted row is in the wave's registers: every lane takes the f64 square root of its entries, lane order is list order, and the
//        k additions run serially over the lanes' values (readlane).  One f64 leaves the kernel per query: no n x k list is written.
//  (iii) k_outlier_partial (pass 0): per workgroup of 256 points in ORIGINAL index order the f64 sum of the valid means (fixed_tree.hpp's
//        fixed order: shuffle tree over the wave, then the four waves) and the valid count; k_outlier_tree: one workgroup adds the
//        partials (thread t takes t, t + 256, ... in order, then the same block sum) and one lane forms cloud_mean.
//  (iv)  k_outlier_partial (pass 1) and k_outlier_tree again on (mean - cloud_mean)^2: std_dev and threshold in one lane.
//  (v)   k_outlier_flag, exclusive_scan_dev, k_gather_flagged (flag_gather.hpp): mask, then index, xyz and rgb of the kept rows in ascending index.
// Radius filter: k_outlier_count is k_cluster_count's walk (sorted_cloud.hpp: walk_in_order) with its early stop at nb_points + 1; then (v).
// No float atomics: the counts are integers, the f64 sums have the one order above, so two calls give the same bits.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "sorted_cloud.hpp"
#include "fixed_tree.hpp"
#include "flag_gather.hpp"
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <algorithm>

namespace tdv {

namespace {

constexpr int OL_WAVES = 4;       // queries (waves) per workgroup of k_outlier_count, as k_cluster_count
constexpr int OL_MEAN_WAVES = 1;  // ... of k_outlier_mean, as k_query_wave (QW_WAVES: measured there)

// device state of one call (workspace), read back at the end
struct OutlierState {
    int n_valid, n_kept;
    double cloud_mean, std_dev, threshold;
};

// rule 3: a point's mean takes part in the statistics (count_i = 0 left the NaN above, which fails here)
__device__ __forceinline__ bool outlier_valid(double m) { return m > 0.0 && m < (double)INFINITY; }

// mean[original index] = rule 2 for every point, from the query's sorted row while it is in the wave
template <int R>
__global__ __launch_bounds__(64 * OL_MEAN_WAVES)
void k_outlier_mean(SortedCloud c, int k, double* __restrict__ mean) {
    constexpr int ROW = 64 * R;
    __shared__ unsigned long long rows[OL_MEAN_WAVES][ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sp = xcd_contiguous_block(blockIdx.x, gridDim.x) * OL_MEAN_WAVES + wave;   // curve order: an XCD works on one stretch
    if (sp >= c.n) return;                                                                // wave-uniform
    unsigned long long key[R];
    const int wcnt = query_wave_collect<R, QW_SEED_SPAN, QW_BEST_FIRST, false>(c, sp, INFINITY, 1, k, rows[wave], lane, key);
    const int cnt = min(k, wcnt);                                                         // count_i; wave-uniform
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int m = min(64, cnt - 64 * r);                                              // entries of the list in this register
        if (m <= 0) break;
        const double d = sqrt((double)__uint_as_float((unsigned)(key[r] >> 32)));         // one square root per lane
        const int lo = (int)(unsigned)__double_as_longlong(d), hi = (int)(unsigned)(__double_as_longlong(d) >> 32);
        for (int l = 0; l < m; ++l) {                                                     // list order: the k additions are serial
            const unsigned long long b = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, l) << 32) |
                                         (unsigned)__builtin_amdgcn_readlane(lo, l);
            s += __longlong_as_double((long long)b);
        }
    }
    if (lane == 0) mean[c.orig[sp]] = cnt > 0 ? s / (double)cnt : tree_nan();
}

// part[b] = the sum over points [256 b, 256 b + 256) of: pass 0, the valid means (cnt[b] = how many); pass 1, their squared deviations
__global__ __launch_bounds__(256) void k_outlier_partial(const double* __restrict__ mean, int n, const OutlierState* __restrict__ st, int pass,
                                                         double* __restrict__ part, int* __restrict__ cnt) {
    __shared__ double lds4[4];
    __shared__ int ldc4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double m = i < n ? mean[i] : 0.0;
    const bool valid = i < n && outlier_valid(m);
    double v = 0.0;
    if (valid) {
        if (pass == 0) v = m;
        else { const double d = m - st->cloud_mean; v = d * d; }
    }
    const double s = tree_block_sum(v, lds4);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
    if (pass == 0) {
        const int c = tree_block_count(valid ? 1 : 0, ldc4);
        if (threadIdx.x == 0) cnt[blockIdx.x] = c;
    }
}

// One workgroup: the fixed tree over the nb partials, then one lane.  Pass 0: n_valid and cloud_mean.  Pass 1: std_dev and threshold.
__global__ __launch_bounds__(256) void k_outlier_tree(OutlierState* st, const double* __restrict__ part, const int* __restrict__ cnt, int nb,
                                                      int pass, double std_ratio) {
    __shared__ double lds4[4];
    __shared__ int ldc4[4];
    const double s = tree_partials_sum(part, nb, lds4);
    if (pass == 0) {
        const int c = tree_partials_count(cnt, nb, ldc4);
        if (threadIdx.x == 0) {
            st->n_valid = c; st->n_kept = 0;
            st->cloud_mean = c > 0 ? s / (double)c : tree_nan();
        }
    } else if (threadIdx.x == 0) {
        const int c = st->n_valid;
        const double sd = c > 1 ? sqrt(s / (double)(c - 1)) : tree_nan();
        st->std_dev = sd;
        st->threshold = st->cloud_mean + std_ratio * sd;
    }
}

// rule 5: flag[i] (and mask[i]) = kept
__global__ __launch_bounds__(256) void k_outlier_flag(const double* __restrict__ mean, int n, const OutlierState* __restrict__ st,
                                                      int* __restrict__ flag, uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double m = mean[i];
    const int kept = (outlier_valid(m) && m < st->threshold) ? 1 : 0;
    flag[i] = kept;
    if (mask) mask[i] = (uint8_t)kept;
}

// Radius filter: cnt = the neighbours of the query (itself included) as far as the walk counted them: it stops once cap = nb_points + 1
// are seen, and the count is saturated there.  flag / mask[original index] = kept (cnt > nb_points), count[original index] = cnt.
__global__ __launch_bounds__(64 * OL_WAVES) void k_outlier_count(SortedCloud c, float eps2, int nb_points, int cap, int* __restrict__ flag,
                                                                 uint8_t* __restrict__ mask, int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int sp = blockIdx.x * OL_WAVES + (threadIdx.x >> 6);
    if (sp >= c.n) return;                                   // wave-uniform
    const float qx = c.sx[sp], qy = c.sy[sp], qz = c.sz[sp];
    int cnt = 0;
    // a query that is not its own neighbour (a NaN or infinite coordinate) has none: as in k_cluster_count
    if (d2_point<D2::DBSCAN>(qx, qy, qz, qx, qy, qz) <= eps2) walk_in_order<D2::DBSCAN>(c, qx, qy, qz, eps2, lane, [&](int leaf) {
        const int p = leaf * 64 + lane;                      // the arrays are padded to a multiple of 256
        const bool nb = p < c.n && d2_point<D2::DBSCAN>(c.sx[p], c.sy[p], c.sz[p], qx, qy, qz) <= eps2;
        cnt += __popcll(__ballot(nb));
        return cnt >= cap;
    });
    if (lane == 0) {
        const int i = c.orig[sp];
        cnt = min(cnt, cap);
        const int kept = cnt > nb_points ? 1 : 0;
        flag[i] = kept;
        if (mask) mask[i] = (uint8_t)kept;
        if (count) count[i] = cnt;
    }
}

// n_valid of the radius filter: the points that count themselves (count > 0 <=> a finite row); integers, any order
__global__ __launch_bounds__(256) void k_outlier_radius_state(const float* __restrict__ xyz, int n, float eps2, OutlierState* st) {
    __shared__ int ldc4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    int v = 0;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        v = d2_point<D2::DBSCAN>(x, y, z, x, y, z) <= eps2 ? 1 : 0;
    }
    const int c = tree_block_count(v, ldc4);
    if (threadIdx.x == 0 && c) atomicAdd(&st->n_valid, c);
}

__global__ void k_outlier_init(OutlierState* st) {
    if (threadIdx.x != 0) return;
    OutlierState z{};
    *st = z;
}

// every argument, before anything is enqueued (include/tdv_hip.h)
bool outlier_cloud_ok(const tdv_ctx* ctx, const float* xyz, int n, const tdv_outlier_result* result) {
    return ctx && result && n >= 0 && (n == 0 || xyz);
}
bool statistical_args_ok(const tdv_ctx* ctx, const float* xyz, int n, int nb_neighbors, double std_ratio, const tdv_outlier_result* result) {
    return outlier_cloud_ok(ctx, xyz, n, result) && nb_neighbors >= 1 && nb_neighbors <= 255 && std::isfinite(std_ratio);
}
bool radius_args_ok(const tdv_ctx* ctx, const float* xyz, int n, int nb_points, float radius, const tdv_outlier_result* result) {
    return outlier_cloud_ok(ctx, xyz, n, result) && nb_points >= 0 && std::isfinite(radius) && radius > 0.f;
}

// device outputs of a call (each optional) and, for the host entry points, where they go
struct OutlierOut {
    uint8_t* mask = nullptr; double* mean = nullptr; int* count = nullptr; int* index = nullptr; float* xyz = nullptr; float* rgb = nullptr;
};

// The whole call on device memory: statistical (nb_neighbors > 0) or radius.  h (host entry points): where the device outputs go.
int outlier_run_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, int nb_neighbors, double std_ratio, int nb_points, float radius,
                    tdv_outlier_result* result, OutlierOut d, const OutlierOut* h) {
    std::memset(result, 0, sizeof(*result));
    const bool statistical = nb_neighbors > 0;
    if (n == 0) {
        if (statistical) result->cloud_mean = result->std_dev = result->threshold = std::nan("");
        return TDV_OK;
    }
    hipStream_t s = ctx->stream;
    const int nb = (n + 255) / 256;
    if (!d_rgb) d.rgb = nullptr;
    OutlierState* st;
    int *flag, *pos;
    TDV_TRY(ws_alloc(ctx, 1, &st));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &flag));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &pos));
    TDV_TRY(pin_reserve(ctx, sizeof(OutlierState)));
    SortedCloud sc;
    if (statistical) {
        double* part; int* cnt;
        if (!d.mean) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.mean));
        TDV_TRY(ws_alloc(ctx, (size_t)nb, &part));
        TDV_TRY(ws_alloc(ctx, (size_t)nb, &cnt));
        TDV_TRY(spatial_sort_cloud(ctx, d_xyz, n, sc));
        const int k = std::min(nb_neighbors, n);
        const unsigned grid = (unsigned)((n + OL_MEAN_WAVES - 1) / OL_MEAN_WAVES);
#define TDV_OL_MEAN(RR) k_outlier_mean<RR><<<grid, 64 * OL_MEAN_WAVES, 0, s>>>(sc, k, d.mean)
        if (k <= 64) TDV_OL_MEAN(2);                              // the row widths of k_query_wave (knn.hip: query_to_lists)
        else if (k <= 192) TDV_OL_MEAN(4);
        else TDV_OL_MEAN(8);
#undef TDV_OL_MEAN
        k_outlier_partial<<<nb, 256, 0, s>>>(d.mean, n, st, 0, part, cnt);
        k_outlier_tree<<<1, 256, 0, s>>>(st, part, cnt, nb, 0, std_ratio);
        k_outlier_partial<<<nb, 256, 0, s>>>(d.mean, n, st, 1, part, cnt);
        k_outlier_tree<<<1, 256, 0, s>>>(st, part, cnt, nb, 1, std_ratio);
        k_outlier_flag<<<nb, 256, 0, s>>>(d.mean, n, st, flag, d.mask);
    } else {
        TDV_TRY(spatial_sort_cloud(ctx, d_xyz, n, sc));
        const float eps2 = std::min(radius * radius, FLT_MAX);    // finite: an infinite d2 never passes (tdv_cluster_dbscan, rule 1)
        const int cap = nb_points == INT_MAX ? INT_MAX : nb_points + 1;
        k_outlier_init<<<1, 64, 0, s>>>(st);
        k_outlier_radius_state<<<nb, 256, 0, s>>>(d_xyz, n, eps2, st);
        k_outlier_count<<<(n + OL_WAVES - 1) / OL_WAVES, 64 * OL_WAVES, 0, s>>>(sc, eps2, nb_points, cap, flag, d.mask, d.count);
    }
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(compact_flagged(ctx, flag, n, pos, &st->n_kept, d_xyz, d_rgb, 3, d.index, d.xyz, d.rgb));
    if (h) {
        TDV_TRY(download(ctx, h->mask, d.mask, (size_t)n));
        TDV_TRY(download(ctx, h->mean, d.mean, (size_t)n));
        TDV_TRY(download(ctx, h->count, d.count, (size_t)n));
    }
    OutlierState hs;
    TDV_TRY(fetch_state(ctx, st, &hs));
    result->n_valid = hs.n_valid; result->n_kept = hs.n_kept;
    if (statistical) { result->cloud_mean = hs.cloud_mean; result->std_dev = hs.std_dev; result->threshold = hs.threshold; }
    // host entry points: the kept rows, n_kept of them
    if (!h) return TDV_OK;
    return download_rows(ctx, (size_t)hs.n_kept, {{h->index, d.index, sizeof(int)}, {h->xyz, d.xyz, 3 * sizeof(float)},
                                                  {h->rgb, d.rgb, 3 * sizeof(float)}});
}

// host arrays: upload, device outputs for what is asked for, outlier_run_dev
int outlier_run_host(tdv_ctx* ctx, const float* xyz, const float* rgb, int n, int nb_neighbors, double std_ratio, int nb_points, float radius,
                     tdv_outlier_result* result, const OutlierOut& h) {
    TDV_TRY(call_begin(ctx));
    float *d_xyz, *d_rgb;
    OutlierOut d;
    const size_t n3 = (size_t)n * 3;
    TDV_TRY(upload(ctx, xyz, n3, &d_xyz));
    TDV_TRY(upload(ctx, rgb, n3, &d_rgb));
    if (n > 0) {
        if (h.mask) TDV_TRY(ws_alloc(ctx, align_up((size_t)n, 16), &d.mask));
        if (h.mean) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.mean));
        if (h.count) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.count));
        if (h.index) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.index));
        if (h.xyz) TDV_TRY(ws_alloc(ctx, n3, &d.xyz));
        if (h.rgb && rgb) TDV_TRY(ws_alloc(ctx, n3, &d.rgb));
    }
    return outlier_run_dev(ctx, d_xyz, d_rgb, n, nb_neighbors, std_ratio, nb_points, radius, result, d, &h);
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

int tdv_remove_statistical_outlier(tdv_ctx* ctx, const float* xyz, const float* rgb, int n, int nb_neighbors, double std_ratio,
                                   tdv_outlier_result* result, uint8_t* mask, double* mean, int* index, float* out_xyz, float* out_rgb) {
    if (!statistical_args_ok(ctx, xyz, n, nb_neighbors, std_ratio, result)) return TDV_ERR_BAD_ARG;
    OutlierOut h; h.mask = mask; h.mean = mean; h.index = index; h.xyz = out_xyz; h.rgb = out_rgb;
    return outlier_run_host(ctx, xyz, rgb, n, nb_neighbors, std_ratio, 0, 0.f, result, h);
}

int tdv_remove_statistical_outlier_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, int nb_neighbors, double std_ratio,
                                       tdv_outlier_result* result, uint8_t* d_mask, double* d_mean, int* d_index, float* d_out_xyz,
                                       float* d_out_rgb) {
    if (!statistical_args_ok(ctx, d_xyz, n, nb_neighbors, std_ratio, result)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    OutlierOut d; d.mask = d_mask; d.mean = d_mean; d.index = d_index; d.xyz = d_out_xyz; d.rgb = d_out_rgb;
    return outlier_run_dev(ctx, d_xyz, d_rgb, n, nb_neighbors, std_ratio, 0, 0.f, result, d, nullptr);
}

int tdv_remove_radius_outlier(tdv_ctx* ctx, const float* xyz, const float* rgb, int n, int nb_points, float radius, tdv_outlier_result* result,
                              uint8_t* mask, int* count, int* index, float* out_xyz, float* out_rgb) {
    if (!radius_args_ok(ctx, xyz, n, nb_points, radius, result)) return TDV_ERR_BAD_ARG;
    OutlierOut h; h.mask = mask; h.count = count; h.index = index; h.xyz = out_xyz; h.rgb = out_rgb;
    return outlier_run_host(ctx, xyz, rgb, n, 0, 0.0, nb_points, radius, result, h);
}

int tdv_remove_radius_outlier_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, int nb_points, float radius,
                                  tdv_outlier_result* result, uint8_t* d_mask, int* d_count, int* d_index, float* d_out_xyz, float* d_out_rgb) {
    if (!radius_args_ok(ctx, d_xyz, n, nb_points, radius, result)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    OutlierOut d; d.mask = d_mask; d.count = d_count; d.index = d_index; d.xyz = d_out_xyz; d.rgb = d_out_rgb;
    return outlier_run_dev(ctx, d_xyz, d_rgb, n, 0, 0.0, nb_points, radius, result, d, nullptr);
}

}  // extern "C"
