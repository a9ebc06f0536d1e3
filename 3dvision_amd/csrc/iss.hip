// ISS keypoints on gfx950: include/tdv_hip.h (tdv_iss_keypoints) states every rule.
//
// The host enqueues everything up front; nothing returns to it between the kernels, and the call reads back once, at the end.
//  (i)   spatial_sort_cloud: the cloud along a Morton curve with the boxes of its leaves and groups (knn.hip), once, for both walks.
//  (ii)  default radii only: k_iss_nn is k_outlier_mean's walk (sorted_cloud.hpp: query_wave_collect) at k = 2 and keeps entry 1 of the row, k_iss_partial sums the
//        valid ones per workgroup of 256 points in ORIGINAL index order (fixed_tree.hpp).
//  (iii) k_iss_state: one workgroup adds the partials in the fixed tree and one lane writes the call's state block: the resolution, the two
//        radii, their squares and the shift of rule 3.  Every later kernel reads them from there.
//  (iv)  k_iss_scatter: one wave per query in curve order through walk_in_order at salient_radius.  Each lane takes one point of a passing
//        leaf and adds its quantised differences into nine per-lane 64-bit integer accumulators and a count; the wave sums the ten
//        integers with DPP adds (in pieces of 22 bits: no cross-lane 64-bit traffic).  A wave takes ISS_QPW queries in turn and parks the
//        totals of query q in lane q, so that the f64 part (covariance, Jacobi sweeps, the saliency test) runs once per wave with ISS_QPW
//        lanes busy instead of once per query with one.  No atomics, and no n x neighbours list.
//  (v)   k_iss_nms: the same walk at non_max_radius for the points with saliency > 0; it stops at the first neighbour of larger saliency.
//  (vi)  k_iss_count (the three counts, integer atomics of workgroup totals), exclusive_scan_dev, k_gather_flagged (flag_gather.hpp).
// Everything a kernel reads from the workspace is written by this call first: the state block by (iii), saliency and support for every
// point by (iv), flag by (v).
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "sorted_cloud.hpp"
#include "fixed_tree.hpp"
#include "flag_gather.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <algorithm>

namespace tdv {

namespace {

constexpr int ISS_WAVES = 4;    // waves per workgroup of k_iss_scatter and k_iss_nms, as k_cluster_count
constexpr int ISS_QPW = 16;     // queries a wave of k_iss_scatter takes in turn: the lanes that share the f64 part
constexpr int ISS_NN_WAVES = 1; // as k_outlier_mean

// device state of one call (workspace), read back at the end
struct IssState {
    int n_finite, n_supported, n_salient, n_keypoints;
    float salient_radius, non_max_radius;
    double resolution;
    float r2_salient, r2_nms;   // rule 1: r * r, FLT_MAX where that overflows (a NaN radius stays NaN: nothing passes)
    int sh, pad;                // rule 3: 20 - E
};

// E of rule 3: r = m * 2^E with m in [0.5, 1) (frexpf), from the bits; 0 for r = 0
__device__ __forceinline__ int iss_frexp_exponent(float r) {
    const unsigned b = __float_as_uint(r) & 0x7fffffffu;
    if (b == 0) return 0;
    const int e = (int)(b >> 23);
    return e ? e - 126 : (31 - __clz((int)b)) - 148;     // a subnormal is mant * 2^-149
}

__device__ __forceinline__ float iss_r2(float r) {
    const float r2 = r * r;
    return r2 > FLT_MAX ? FLT_MAX : r2;
}

// rule 8: nn[original index] = sqrt of the d2 of entry 1 of the query's kNN list at k = 2; NaN where the list has fewer than two entries
__global__ __launch_bounds__(64 * ISS_NN_WAVES)
void k_iss_nn(SortedCloud c, int k, double* __restrict__ nn) {
    __shared__ unsigned long long rows[ISS_NN_WAVES][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sp = xcd_contiguous_block(blockIdx.x, gridDim.x) * ISS_NN_WAVES + wave;
    if (sp >= c.n) return;                                                                // wave-uniform
    unsigned long long key[2];
    const int wcnt = query_wave_collect<2, QW_SEED_SPAN, QW_BEST_FIRST, false>(c, sp, INFINITY, 1, k, rows[wave], lane, key);
    const unsigned d2 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key[0] >> 32), 1);   // lane order is list order
    if (lane == 0) nn[c.orig[sp]] = min(k, wcnt) >= 2 ? sqrt((double)__uint_as_float(d2)) : tree_nan();
}

// part[b], cnt[b] = the sum and the number of the valid nn over points [256 b, 256 b + 256)
__global__ __launch_bounds__(256) void k_iss_partial(const double* __restrict__ nn, int n, double* __restrict__ part, int* __restrict__ cnt) {
    __shared__ double lds4[4];
    __shared__ int ldc4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double v = i < n ? nn[i] : tree_nan();
    const bool valid = v < (double)INFINITY;                                              // finite: a square root is never negative; NaN fails
    const double s = tree_block_sum(valid ? v : 0.0, lds4);
    const int c = tree_block_count(valid ? 1 : 0, ldc4);
    if (threadIdx.x == 0) { part[blockIdx.x] = s; cnt[blockIdx.x] = c; }
}

// One workgroup: the fixed tree over the nb partials (default radii; nb = 0 otherwise), then one lane writes the whole state block
__global__ __launch_bounds__(256) void k_iss_state(IssState* st, const double* __restrict__ part, const int* __restrict__ cnt, int nb,
                                                   int defaults, float salient_radius, float non_max_radius) {
    __shared__ double lds4[4];
    __shared__ int ldc4[4];
    const double s = tree_partials_sum(part, nb, lds4);
    const int c = tree_partials_count(cnt, nb, ldc4);
    if (threadIdx.x != 0) return;
    IssState z{};
    z.resolution = tree_nan();
    z.salient_radius = salient_radius; z.non_max_radius = non_max_radius;
    if (defaults) {
        z.resolution = c > 0 ? s / (double)c : tree_nan();
        z.salient_radius = (float)(6.0 * z.resolution);
        z.non_max_radius = (float)(4.0 * z.resolution);
    }
    z.r2_salient = iss_r2(z.salient_radius); z.r2_nms = iss_r2(z.non_max_radius);
    z.sh = 20 - iss_frexp_exponent(z.salient_radius);
    *st = z;
}

// Sum of a 64-bit integer over the wave, modulo 2^64, wave-uniform: three pieces of at most 22 bits, each summed with DPP adds
__device__ __forceinline__ unsigned long long iss_wave_sum_u64(unsigned long long v) {
    const unsigned s0 = (unsigned)wave_sum_i32((int)(v & 0x3fffffu)), s1 = (unsigned)wave_sum_i32((int)((v >> 22) & 0x3fffffu)),
                   s2 = (unsigned)wave_sum_i32((int)(v >> 44));
    return (unsigned long long)s0 + ((unsigned long long)s1 << 22) + ((unsigned long long)s2 << 44);
}

// rule 3: u = rintf(ldexpf(d, sh)) as an integer, saturated to what an int holds (it is within 2^20 + 1 wherever r * r is a normal f32)
__device__ __forceinline__ int iss_quantise(float d, int sh) {
    return (int)fminf(fmaxf(rintf(ldexpf(d, sh)), -2147483648.f), 2147483520.f);
}

// rule 5: one rotation of the pair (p, q); r is the third index, arp = a[r][p], arq = a[r][q]
__device__ __forceinline__ void iss_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app -= h; aqq += h;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq; apq = 0.0;
}

__device__ __forceinline__ void iss_order(double& a, double& b) {      // a >= b afterwards
    if (a < b) { const double t = a; a = b; b = t; }
}

// saliency[original index] (rules 2-6) for every point; support and the three eigenvalues where asked for
__global__ __launch_bounds__(64 * ISS_WAVES)
void k_iss_scatter(SortedCloud c, const IssState* __restrict__ st, int min_neighbors, double gamma_21, double gamma_32,
                   double* __restrict__ saliency, double* __restrict__ eig, int* __restrict__ support) {
    const int lane = threadIdx.x & 63;
    const int base = (xcd_contiguous_block(blockIdx.x, gridDim.x) * ISS_WAVES + (threadIdx.x >> 6)) * ISS_QPW;   // curve order
    if (base >= c.n) return;                                 // wave-uniform
    const float r2 = st->r2_salient;
    const int sh = st->sh;
    const int nq = min(ISS_QPW, c.n - base);
    unsigned long long mine[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // lane q: S_x, S_y, S_z, S_xx, S_xy, S_xz, S_yy, S_yz, S_zz of query base + q
    int mine_cnt = 0;
    for (int q = 0; q < nq; ++q) {
        const int sp = base + q;
        const float qx = c.sx[sp], qy = c.sy[sp], qz = c.sz[sp];
        unsigned long long a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int cnt = 0;
        // a query that is not its own neighbour (a NaN or infinite coordinate, a NaN radius) has none: as in k_cluster_count
        if (d2_point<D2::DBSCAN>(qx, qy, qz, qx, qy, qz) <= r2) walk_in_order<D2::DBSCAN>(c, qx, qy, qz, r2, lane, [&](int leaf) {
            const int p = leaf * 64 + lane;                  // the arrays are padded to a multiple of 256
            const float dx = c.sx[p] - qx, dy = c.sy[p] - qy, dz = c.sz[p] - qz;
            if (p < c.n && (dx * dx + dy * dy) + dz * dz <= r2) {
                const int ux = iss_quantise(dx, sh), uy = iss_quantise(dy, sh), uz = iss_quantise(dz, sh);
                a[0] += (unsigned long long)(long long)ux; a[1] += (unsigned long long)(long long)uy; a[2] += (unsigned long long)(long long)uz;
                a[3] += (unsigned long long)((long long)ux * ux); a[4] += (unsigned long long)((long long)ux * uy);
                a[5] += (unsigned long long)((long long)ux * uz); a[6] += (unsigned long long)((long long)uy * uy);
                a[7] += (unsigned long long)((long long)uy * uz); a[8] += (unsigned long long)((long long)uz * uz);
                ++cnt;
            }
            return false;
        });
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const unsigned long long tot = iss_wave_sum_u64(a[k]);
            if (lane == q) mine[k] = tot;
        }
        const int tc = wave_sum_i32(cnt);
        if (lane == q) mine_cnt = tc;
    }
    if (lane >= nq) return;
    const int i = c.orig[base + lane];
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, sal = 0.0;
    if (mine_cnt >= min_neighbors) {                         // rule 2 (min_neighbors >= 1: the count is not 0)
        const double n = (double)mine_cnt;
        double S[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = (double)(long long)mine[k];
        // rule 4
        double a00 = (S[3] - (S[0] * S[0]) / n) / n, a01 = (S[4] - (S[0] * S[1]) / n) / n, a02 = (S[5] - (S[0] * S[2]) / n) / n;
        double a11 = (S[6] - (S[1] * S[1]) / n) / n, a12 = (S[7] - (S[1] * S[2]) / n) / n, a22 = (S[8] - (S[2] * S[2]) / n) / n;
        // rule 5
        for (int sweep = 0; sweep < TDV_ISS_JACOBI_SWEEPS; ++sweep) {
            iss_rotate(a00, a11, a01, a02, a12);
            iss_rotate(a00, a22, a02, a01, a12);
            iss_rotate(a11, a22, a12, a01, a02);
        }
        l0 = a00; l1 = a11; l2 = a22;
        iss_order(l0, l1); iss_order(l1, l2); iss_order(l0, l1);
        l0 = ldexp(l0, -2 * sh); l1 = ldexp(l1, -2 * sh); l2 = ldexp(l2, -2 * sh);
        // rule 6
        if (l1 / l0 < gamma_21 && l2 / l1 < gamma_32 && l2 > 0.0) sal = l2;
    }
    saliency[i] = sal;
    if (support) support[i] = mine_cnt;
    if (eig) { eig[3 * (size_t)i] = l0; eig[3 * (size_t)i + 1] = l1; eig[3 * (size_t)i + 2] = l2; }
}

// rule 7: flag / mask[original index] = keypoint
__global__ __launch_bounds__(64 * ISS_WAVES)
void k_iss_nms(SortedCloud c, const IssState* __restrict__ st, int min_neighbors, const double* __restrict__ saliency, int* __restrict__ flag,
               uint8_t* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const int sp = xcd_contiguous_block(blockIdx.x, gridDim.x) * ISS_WAVES + (threadIdx.x >> 6);
    if (sp >= c.n) return;                                   // wave-uniform
    const int i = c.orig[sp];
    const double s = saliency[i];
    int key = 0;
    if (s > 0.0) {                                           // wave-uniform
        const float r2 = st->r2_nms;
        const float qx = c.sx[sp], qy = c.sy[sp], qz = c.sz[sp];
        int cnt = 0;
        bool beaten = false;
        if (d2_point<D2::DBSCAN>(qx, qy, qz, qx, qy, qz) <= r2) walk_in_order<D2::DBSCAN>(c, qx, qy, qz, r2, lane, [&](int leaf) {
            const int p = leaf * 64 + lane;
            const bool nb = p < c.n && d2_point<D2::DBSCAN>(c.sx[p], c.sy[p], c.sz[p], qx, qy, qz) <= r2;
            const double sj = nb ? saliency[c.orig[p]] : 0.0;
            cnt += __popcll(__ballot(nb));
            beaten = __ballot(sj > s) != 0;
            return beaten;                                   // one larger neighbour decides
        });
        key = (!beaten && cnt >= min_neighbors) ? 1 : 0;
    }
    if (lane == 0) {
        flag[i] = key;
        if (mask) mask[i] = (uint8_t)key;
    }
}

// n_finite, n_supported, n_salient: integers, any order.  The three flags of a point share one word (10 bits each: a workgroup counts at
// most 256), so one workgroup sum serves all three.
__global__ __launch_bounds__(256) void k_iss_count(const int* __restrict__ support, const double* __restrict__ saliency, int n, int min_neighbors,
                                                   IssState* st) {
    __shared__ int ldc4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    int v = 0;
    if (i < n) {
        const int sup = support[i];
        v = (sup >= 1 ? 1 : 0) | (sup >= min_neighbors ? 1 << 10 : 0) | (saliency[i] > 0.0 ? 1 << 20 : 0);
    }
    const int c = tree_block_count(v, ldc4);
    if (threadIdx.x == 0) {
        if (c & 1023) atomicAdd(&st->n_finite, c & 1023);
        if ((c >> 10) & 1023) atomicAdd(&st->n_supported, (c >> 10) & 1023);
        if (c >> 20) atomicAdd(&st->n_salient, c >> 20);
    }
}

bool iss_radius_ok(float r) { return std::isfinite(r) && r >= 0.f; }

// the outputs of a call (each optional)
struct IssOut {
    uint8_t* mask = nullptr; double* saliency = nullptr; double* eig = nullptr; int* support = nullptr; int* index = nullptr;
    float* xyz = nullptr; float* attr = nullptr;
};

// every argument, before anything is enqueued (include/tdv_hip.h)
bool iss_args_ok(const tdv_ctx* ctx, const float* xyz, int n, const tdv_iss_params* p, const float* attr, int attr_width,
                 const tdv_iss_result* result, const float* out_attr) {
    if (!ctx || !p || !result || n < 0 || n > TDV_ISS_MAX_POINTS || (n > 0 && !xyz)) return false;
    if (!iss_radius_ok(p->salient_radius) || !iss_radius_ok(p->non_max_radius) || ((p->salient_radius == 0.f) != (p->non_max_radius == 0.f))) return false;
    if (!(p->gamma_21 > 0.0) || !(p->gamma_32 > 0.0) || p->min_neighbors < 1) return false;
    return attr_width >= 0 && !(attr_width > 0 && !attr) && !(out_attr && !attr);
}

// The whole call on device memory.  h (host entry point): where the device outputs go.
int iss_run_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_iss_params& prm, const float* d_attr, int attr_width, tdv_iss_result* result,
                IssOut d, const IssOut* h) {
    std::memset(result, 0, sizeof(*result));
    const bool defaults = prm.salient_radius == 0.f;
    if (n == 0) {                                            // the mean of no distance: NaN, and so are the radii made from it
        result->resolution = std::nan("");
        result->salient_radius = defaults ? std::nanf("") : prm.salient_radius;
        result->non_max_radius = defaults ? std::nanf("") : prm.non_max_radius;
        return TDV_OK;
    }
    hipStream_t s = ctx->stream;
    const int nb = (n + 255) / 256;
    if (!d_attr || attr_width == 0) d.attr = nullptr;
    IssState* st;
    int *flag, *pos;
    double* part = nullptr; int* cnt = nullptr;
    TDV_TRY(ws_alloc(ctx, 1, &st));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &flag));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &pos));
    if (!d.saliency) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.saliency));
    if (!d.support) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.support));
    TDV_TRY(pin_reserve(ctx, sizeof(IssState)));
    SortedCloud sc;
    TDV_TRY(spatial_sort_cloud(ctx, d_xyz, n, sc));
    if (defaults) {
        double* nn;
        TDV_TRY(ws_alloc(ctx, (size_t)n, &nn));
        TDV_TRY(ws_alloc(ctx, (size_t)nb, &part));
        TDV_TRY(ws_alloc(ctx, (size_t)nb, &cnt));
        k_iss_nn<<<(n + ISS_NN_WAVES - 1) / ISS_NN_WAVES, 64 * ISS_NN_WAVES, 0, s>>>(sc, std::min(2, n), nn);
        k_iss_partial<<<nb, 256, 0, s>>>(nn, n, part, cnt);
    }
    k_iss_state<<<1, 256, 0, s>>>(st, part, cnt, defaults ? nb : 0, defaults ? 1 : 0, prm.salient_radius, prm.non_max_radius);
    const int per_wg = ISS_WAVES * ISS_QPW;
    k_iss_scatter<<<(n + per_wg - 1) / per_wg, 64 * ISS_WAVES, 0, s>>>(sc, st, prm.min_neighbors, prm.gamma_21, prm.gamma_32, d.saliency, d.eig, d.support);
    k_iss_nms<<<(n + ISS_WAVES - 1) / ISS_WAVES, 64 * ISS_WAVES, 0, s>>>(sc, st, prm.min_neighbors, d.saliency, flag, d.mask);
    k_iss_count<<<nb, 256, 0, s>>>(d.support, d.saliency, n, prm.min_neighbors, st);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(compact_flagged(ctx, flag, n, pos, &st->n_keypoints, d_xyz, d_attr, attr_width, d.index, d.xyz, d.attr));
    if (h) {
        TDV_TRY(download(ctx, h->mask, d.mask, (size_t)n));
        TDV_TRY(download(ctx, h->saliency, d.saliency, (size_t)n));
        TDV_TRY(download(ctx, h->eig, d.eig, (size_t)n * 3));
        TDV_TRY(download(ctx, h->support, d.support, (size_t)n));
    }
    IssState hs;
    TDV_TRY(fetch_state(ctx, st, &hs));
    result->n_finite = hs.n_finite; result->n_supported = hs.n_supported; result->n_salient = hs.n_salient; result->n_keypoints = hs.n_keypoints;
    result->salient_radius = hs.salient_radius; result->non_max_radius = hs.non_max_radius; result->resolution = hs.resolution;
    // host entry point: the keypoints' rows, n_keypoints of them
    if (!h) return TDV_OK;
    return download_rows(ctx, (size_t)hs.n_keypoints, {{h->index, d.index, sizeof(int)}, {h->xyz, d.xyz, 3 * sizeof(float)},
                                                       {h->attr, d.attr, (size_t)attr_width * sizeof(float)}});
}

// host arrays: upload, device outputs for what is asked for, iss_run_dev
int iss_run_host(tdv_ctx* ctx, const float* xyz, int n, const tdv_iss_params& prm, const float* attr, int attr_width, tdv_iss_result* result,
                 const IssOut& h) {
    TDV_TRY(call_begin(ctx));
    float *d_xyz, *d_attr = nullptr;
    IssOut d;
    const size_t n3 = (size_t)n * 3, na = (size_t)n * (size_t)attr_width;
    TDV_TRY(upload(ctx, xyz, n3, &d_xyz));
    if (n > 0) {
        if (h.attr) {                                        // the rows are only ever gathered
            TDV_TRY(upload(ctx, attr, na, &d_attr));
            if (d_attr) TDV_TRY(ws_alloc(ctx, na, &d.attr));
        }
        if (h.mask) TDV_TRY(ws_alloc(ctx, align_up((size_t)n, 16), &d.mask));
        if (h.saliency) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.saliency));
        if (h.eig) TDV_TRY(ws_alloc(ctx, n3, &d.eig));
        if (h.support) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.support));
        if (h.index) TDV_TRY(ws_alloc(ctx, (size_t)n, &d.index));
        if (h.xyz) TDV_TRY(ws_alloc(ctx, n3, &d.xyz));
    }
    return iss_run_dev(ctx, d_xyz, n, prm, d_attr, attr_width, result, d, &h);
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_iss_default_params(tdv_iss_params* p) {
    if (!p) return;
    p->salient_radius = 0.f; p->non_max_radius = 0.f; p->gamma_21 = 0.975; p->gamma_32 = 0.975; p->min_neighbors = 5;
}

int tdv_iss_keypoints(tdv_ctx* ctx, const float* xyz, int n, const tdv_iss_params* params, const float* attr, int attr_width, tdv_iss_result* result,
                      uint8_t* mask, double* saliency, double* eigenvalues, int* support, int* index, float* out_xyz, float* out_attr) {
    if (!iss_args_ok(ctx, xyz, n, params, attr, attr_width, result, out_attr)) return TDV_ERR_BAD_ARG;
    IssOut h; h.mask = mask; h.saliency = saliency; h.eig = eigenvalues; h.support = support; h.index = index; h.xyz = out_xyz; h.attr = out_attr;
    return iss_run_host(ctx, xyz, n, *params, attr, attr_width, result, h);
}

int tdv_iss_keypoints_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_iss_params* params, const float* d_attr, int attr_width,
                          tdv_iss_result* result, uint8_t* d_mask, double* d_saliency, double* d_eigenvalues, int* d_support, int* d_index,
                          float* d_out_xyz, float* d_out_attr) {
    if (!iss_args_ok(ctx, d_xyz, n, params, d_attr, attr_width, result, d_out_attr)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    IssOut d; d.mask = d_mask; d.saliency = d_saliency; d.eig = d_eigenvalues; d.support = d_support; d.index = d_index; d.xyz = d_out_xyz;
    d.attr = d_out_attr;
    return iss_run_dev(ctx, d_xyz, n, *params, d_attr, attr_width, result, d, nullptr);
}

}  // extern "C"
