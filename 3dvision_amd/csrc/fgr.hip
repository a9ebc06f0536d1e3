// Fast Global Registration (Zhou, Park, Koltun, ECCV 2016) on gfx950: include/tdv_hip.h (tdv_fgr) states every step and its order.
//
//  (i)   matches: feature_match_dev twice (source -> target, target -> source), into buffers allocated before both calls (the match's
//        own scratch is rewound inside it, never below what the caller holds).
//  (ii)  k_fgr_mutual_flags + exclusive_scan_dev + k_fgr_mutual_scatter: the mutual pairs in ascending source index; the count stays
//        on the device, where the tuple kernels read it.
//  (iii) tuple test: k_fgr_tuple_flags runs one trial per thread (a Philox draw, six gathered points, three ratio tests in f64) and
//        keeps one 64-bit pass mask per wave; k_fgr_tuple_compact (one workgroup) scans the masks of the chunk, adds the passes kept so
//        far and writes the pairs of the first maximum_tuple_count passes in trial order.  The first chunk is enqueued before the mutual
//        count is read back, so a typical call reads back once before the optimisation.
//  (iv)  k_fgr_mean_partial / k_fgr_mean_final and k_fgr_scale_partial / k_fgr_scale_final: the means (f64 fixed-order tree) and the
//        scale (max; order-free) of both clouds.
//  (v)   k_fgr_optimize: ONE workgroup runs every iteration: per-thread f64 partial sums of the 21 + 6 slots over pairs tid, tid + 256,
//        ..., a fixed wave and LDS tree, one lane does the f64 LDL^T, the Rz Ry Rx update and T = delta T; T goes back through LDS.
//        At the end that lane returns to the original scale and writes the f32 pose in the layout of RANSAC's winner.
//  (vi)  ransac_score_pose_dev: RANSAC's own winner scoring of that pose (k_gather_pq, k_ransac_rmse_partial, k_ransac_rmse_final).
#include "tdv_internal.hpp"
#include "philox.hpp"
#include "fixed_tree.hpp"
#include <cmath>
#include <cstring>
#include <algorithm>

namespace tdv {

namespace {

constexpr int FGR_OPT_THREADS = 256;
constexpr int FGR_CHUNK_MAX_SHIFT = 5;       // chunk k holds TDV_FGR_TRIAL_CHUNK << min(k, 5) trials
constexpr int FGR_COMPACT_THREADS = 1024;
static_assert(TDV_FGR_TRIAL_CHUNK % (64 * FGR_COMPACT_THREADS) == 0, "a chunk's waves split evenly over the compaction threads");

__global__ void k_fgr_mutual_flags(const int* __restrict__ cst, const int* __restrict__ cts, int ns, int nt, int* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const int j = cst[i];
    flags[i] = ((unsigned)j < (unsigned)nt && cts[j] == i) ? 1 : 0;
}

__global__ void k_fgr_mutual_scatter(const int* __restrict__ cst, const int* __restrict__ flags, const int* __restrict__ offs, int ns,
                                     int2* __restrict__ mutual) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns && flags[i]) mutual[offs[i]] = make_int2(i, cst[i]);
}

__device__ __forceinline__ double fgr_len(const float* __restrict__ x, int u, int v) {
    const double dx = (double)x[3 * u] - (double)x[3 * v], dy = (double)x[3 * u + 1] - (double)x[3 * v + 1],
                 dz = (double)x[3 * u + 2] - (double)x[3 * v + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ void fgr_trial_indices(unsigned long long t, unsigned n_mutual, uint32_t seed, unsigned idx[3]) {
    uint32_t x[4];
    philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), 0u, 0u, seed, 0u, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) idx[k] = (unsigned)(((unsigned long long)x[k] * n_mutual) >> 32);
}

// one trial per thread; masks[w] = pass bits of wave w of the chunk (bit = lane)
__global__ __launch_bounds__(256) void k_fgr_tuple_flags(const int2* __restrict__ mutual, const int* __restrict__ d_n_mutual,
                                                         const float* __restrict__ src, const float* __restrict__ tgt,
                                                         unsigned long long t0, uint32_t seed, double s,
                                                         unsigned long long* __restrict__ masks) {
    const unsigned n = (unsigned)*d_n_mutual;
    const unsigned long long t = t0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool pass = false;
    if (t < 100ull * n) {
        unsigned idx[3];
        fgr_trial_indices(t, n, seed, idx);
        const int2 m0 = mutual[idx[0]], m1 = mutual[idx[1]], m2 = mutual[idx[2]];
        const double la0 = fgr_len(src, m0.x, m1.x), la1 = fgr_len(src, m1.x, m2.x), la2 = fgr_len(src, m2.x, m0.x);
        const double lb0 = fgr_len(tgt, m0.y, m1.y), lb1 = fgr_len(tgt, m1.y, m2.y), lb2 = fgr_len(tgt, m2.y, m0.y);
        pass = (la0 * s < lb0 && lb0 < la0 / s) && (la1 * s < lb1 && lb1 < la1 / s) && (la2 * s < lb2 && lb2 < la2 / s);
    }
    const unsigned long long m = __ballot(pass);
    if ((threadIdx.x & 63) == 0) masks[((size_t)blockIdx.x * 256 + threadIdx.x) >> 6] = m;
}

// One workgroup: the passes of the chunk in trial order, appended after the `state[0]` kept so far, up to max_count trials.
// Thread i owns waves [i * per, (i + 1) * per) of the chunk.
__global__ __launch_bounds__(FGR_COMPACT_THREADS) void k_fgr_tuple_compact(const unsigned long long* __restrict__ masks, int per,
                                                                           unsigned long long t0, const int2* __restrict__ mutual,
                                                                           const int* __restrict__ d_n_mutual, uint32_t seed,
                                                                           int max_count, int* __restrict__ state,
                                                                           int2* __restrict__ tuples) {
    __shared__ long long wave_tot[FGR_COMPACT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned n = (unsigned)*d_n_mutual;
    const long long base = state[0];
    long long cnt = 0;
    for (int w = tid * per; w < (tid + 1) * per; ++w) cnt += __popcll(masks[w]);
    long long incl = cnt;                                                          // inclusive scan in the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    long long before = 0, total = 0;
    for (int k = 0; k < FGR_COMPACT_THREADS / 64; ++k) { if (k < wv) before += wave_tot[k]; total += wave_tot[k]; }
    long long rank = base + before + (incl - cnt);
    for (int w = tid * per; w < (tid + 1) * per && rank < max_count; ++w) {
        unsigned long long m = masks[w];
        while (m && rank < max_count) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            unsigned idx[3];
            fgr_trial_indices(t0 + (unsigned long long)w * 64 + bit, n, seed, idx);
#pragma unroll
            for (int k = 0; k < 3; ++k) tuples[3 * rank + k] = mutual[idx[k]];
            ++rank;
        }
    }
    __syncthreads();                                   // every thread has read state[0]
    if (tid == 0) state[0] = (int)std::min(base + total, (long long)max_count);
}

// blocks [0, bs) sum 256 source points each, blocks [bs, bs + bt) target points: slabs[3 b + a]
__global__ __launch_bounds__(256) void k_fgr_mean_partial(const float* __restrict__ src, int ns, const float* __restrict__ tgt, int nt,
                                                          int bs, double* __restrict__ slabs) {
    __shared__ double lds4[4];
    const bool is_s = (int)blockIdx.x < bs;
    const float* x = is_s ? src : tgt;
    const int n = is_s ? ns : nt, i = (is_s ? blockIdx.x : blockIdx.x - bs) * 256 + threadIdx.x;
    for (int a = 0; a < 3; ++a) {
        const double v = tree_block_sum(i < n ? (double)x[3 * i + a] : 0.0, lds4);
        if (threadIdx.x == 0) slabs[3 * (size_t)blockIdx.x + a] = v;
    }
}
// norm[0..2] = mu_s, norm[3..5] = mu_t
__global__ __launch_bounds__(256) void k_fgr_mean_final(const double* __restrict__ slabs, int bs, int bt, int ns, int nt,
                                                        double* __restrict__ norm) {
    __shared__ double part[256];
    for (int c = 0; c < 2; ++c) {
        const int b0 = c ? bs : 0, nb = c ? bt : bs;
        for (int a = 0; a < 3; ++a) {
            double v = 0.0;
            for (int b = threadIdx.x; b < nb; b += 256) v += slabs[3 * (size_t)(b0 + b) + a];
            part[threadIdx.x] = v;
            __syncthreads();
            for (int off = 128; off > 0; off >>= 1) {
                if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
                __syncthreads();
            }
            if (threadIdx.x == 0) norm[3 * c + a] = part[0] / (double)(c ? nt : ns);
            __syncthreads();
        }
    }
}
// slabs[b] = the largest |x - mu| of block b's points (fmax: a NaN never wins)
__global__ __launch_bounds__(256) void k_fgr_scale_partial(const float* __restrict__ src, int ns, const float* __restrict__ tgt, int nt,
                                                           int bs, const double* __restrict__ norm, double* __restrict__ slabs) {
    __shared__ double lds4[4];
    const bool is_s = (int)blockIdx.x < bs;
    const float* x = is_s ? src : tgt;
    const double* mu = norm + (is_s ? 0 : 3);
    const int n = is_s ? ns : nt, i = (is_s ? blockIdx.x : blockIdx.x - bs) * 256 + threadIdx.x;
    double r = 0.0;
    if (i < n) {
        const double dx = (double)x[3 * i] - mu[0], dy = (double)x[3 * i + 1] - mu[1], dz = (double)x[3 * i + 2] - mu[2];
        r = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    const double m = tree_block_max(r, lds4);
    if (threadIdx.x == 0) slabs[blockIdx.x] = m;
}
// norm[6] = sigma (1 with use_absolute_scale), norm[7] = mu's start value (1, or the scale with use_absolute_scale)
__global__ __launch_bounds__(256) void k_fgr_scale_final(const double* __restrict__ slabs, int nb, int absolute, double* __restrict__ norm) {
    __shared__ double lds4[4];
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) v = fmax(v, slabs[b]);
    const double scale = tree_block_max(v, lds4);
    if (threadIdx.x == 0) { norm[6] = absolute ? 1.0 : scale; norm[7] = absolute ? scale : 1.0; }
}

// A x = b for symmetric 6x6 A (slots of the upper triangle, row by row: (0,0), (0,1), ..., (5,5)) by unpivoted LDL^T in the header's
// order; false (x untouched) when a pivot is not > 0 or not finite.  Compile-time indices only: registers, no scratch.
__device__ __forceinline__ bool ldlt6_f64(const double* A21, const double* b, double* x) {
    double L[6][6], d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int i = j; i < 6; ++i) {
            const int slot = j * 6 - j * (j - 1) / 2 + (i - j);   // (j, i) of the upper triangle = (i, j) of the lower
            double s = A21[slot];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - (L[i][k] * d[k]) * L[j][k];
            if (i == j) {
                if (!(s > 0.0) || !isfinite(s)) return false;
                d[j] = s;
            } else {
                L[i][j] = s / d[j];
            }
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s;
    }
    return true;
}

// One workgroup, every iteration.  PQ: scratch of 6 doubles per pair (p, q normalised), written and read by the same thread.
// hyp12: the f32 pose, column-major R then t (k_ransac_rmse_partial's layout).
__global__ __launch_bounds__(FGR_OPT_THREADS) void k_fgr_optimize(const int2* __restrict__ pairs, int n, const float* __restrict__ src,
                                                                  const float* __restrict__ tgt, const double* __restrict__ norm,
                                                                  double* __restrict__ PQ, int iters, int decrease_mu, double mcd,
                                                                  double div, float* __restrict__ hyp12) {
    constexpr int NW = FGR_OPT_THREADS / 64;
    __shared__ double red[NW][27];
    __shared__ double sT[12];                          // rows 0..2 of T, row-major 3x4
    const int tid = threadIdx.x;
    if (n < 10) {                                      // Open3D's rule: the identity
        if (tid < 12) hyp12[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.f : 0.f;
        return;
    }
    const double mus[3] = {norm[0], norm[1], norm[2]}, mut[3] = {norm[3], norm[4], norm[5]};
    const double sigma = norm[6];
    for (int c = tid; c < n; c += FGR_OPT_THREADS) {
        const int2 pr = pairs[c];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            PQ[6 * (size_t)c + a] = ((double)src[3 * pr.x + a] - mus[a]) / sigma;
            PQ[6 * (size_t)c + 3 + a] = ((double)tgt[3 * pr.y + a] - mut[a]) / sigma;
        }
    }
    if (tid < 12) sT[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    __syncthreads();
    double mu = norm[7];
    for (int itr = 0; itr < iters; ++itr) {
        if (decrease_mu && itr % 4 == 0 && mu > mcd) mu = mu / div;
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = sT[k];
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.0;
        for (int c = tid; c < n; c += FGR_OPT_THREADS) {
            const double* g = PQ + 6 * (size_t)c;
            const double px = g[0], py = g[1], pz = g[2], qx = g[3], qy = g[4], qz = g[5];
            double q[3], r[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = ((T[4 * a] * qx + T[4 * a + 1] * qy) + T[4 * a + 2] * qz) + T[4 * a + 3];
            r[0] = px - q[0]; r[1] = py - q[1]; r[2] = pz - q[2];
            const double rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            double w = mu / (rr + mu);
            w = w * w;
            const double J[3][6] = {{0.0, -q[2], q[1], -1.0, 0.0, 0.0}, {q[2], 0.0, -q[0], 0.0, -1.0, 0.0}, {-q[1], q[0], 0.0, 0.0, 0.0, -1.0}};
            int slot = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b, ++slot)
                    acc[slot] += (w * (J[0][a] * J[0][b]) + w * (J[1][a] * J[1][b])) + w * (J[2][a] * J[2][b]);
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] += (w * (J[0][a] * r[0]) + w * (J[1][a] * r[1])) + w * (J[2][a] * r[2]);
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            double v = acc[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            acc[k] = v;
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 27; ++k) red[tid >> 6][k] = acc[k];
        }
        __syncthreads();
        if (tid == 0) {
            double H[27];
#pragma unroll
            for (int k = 0; k < 27; ++k) H[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
            double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (ldlt6_f64(H, H + 21, x)) {
#pragma unroll
                for (int k = 0; k < 6; ++k) x[k] = -x[k];
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k) x[k] = 0.0;
            }
            const double c0 = cos(x[0]), s0 = sin(x[0]), c1 = cos(x[1]), s1 = sin(x[1]), c2 = cos(x[2]), s2 = sin(x[2]);
            const double D[12] = {c2 * c1, (c2 * s1) * s0 - s2 * c0, (c2 * s1) * c0 + s2 * s0, x[3],
                                  s2 * c1, (s2 * s1) * s0 + c2 * c0, (s2 * s1) * c0 - c2 * s0, x[4],
                                  -s1, c1 * s0, c1 * c0, x[5]};
            double Tn[12];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    Tn[4 * a + b] = ((D[4 * a] * T[b] + D[4 * a + 1] * T[4 + b]) + D[4 * a + 2] * T[8 + b]) + D[4 * a + 3] * (b == 3 ? 1.0 : 0.0);
#pragma unroll
            for (int k = 0; k < 12; ++k) sT[k] = Tn[k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        // Open3D's GetInvTransformationOriginalScale: R' = R^T, t' = -R^T ((mu_s + sigma t) - R mu_t)
        double u[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = (mus[a] + sigma * sT[4 * a + 3]) - ((sT[4 * a] * mut[0] + sT[4 * a + 1] * mut[1]) + sT[4 * a + 2] * mut[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) hyp12[3 * c + r] = (float)sT[4 * c + r];            // R'[r][c] = R[c][r]
#pragma unroll
        for (int a = 0; a < 3; ++a) hyp12[9 + a] = (float)-((sT[a] * u[0] + sT[4 + a] * u[1]) + sT[8 + a] * u[2]);
    }
}

// want_pairs (tdv_fgr_correspondences): stop after the tuple test and leave the device pair lists in *pairs
struct FgrPairs { const int2* mutual = nullptr; const int2* tuple = nullptr; int n_mutual = 0, n_tuple = 0; long long trials_run = 0; };

int fgr_run_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* d_fs, const float* d_ft, float voxel,
                const tdv_fgr_params& prm, tdv_fgr_result* out, FgrPairs* pairs) {
    hipStream_t s = ctx->stream;
    // device block: [0] mutual count, [1] tuple trials kept; then f64 norm[8] (mu_s, mu_t, sigma, mu0), error sum + count, hyp12
    int* blk = nullptr;
    TDV_TRY(ws_alloc(ctx, 64, &blk));
    double* d_norm = reinterpret_cast<double*>(blk + 4);
    double* d_out2 = d_norm + 8;
    float* d_hyp12 = reinterpret_cast<float*>(d_out2 + 2);
    TDV_HIP(ctx, hipMemsetAsync(blk, 0, 256, s));
    int *cst, *cts, *flags, *offs; int2* mutual;
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &cst));
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &cts));
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &flags));
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &offs));
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &mutual));
    // pairs of at most max_tuple_count trials, and never more than 100 trials per possible mutual pair
    const long long max_trials_bound = 100LL * std::min(ns, nt);
    const long long tuple_cap = prm.tuple_test ? 3 * std::min((long long)prm.maximum_tuple_count, max_trials_bound) : 0;
    int2* tuples = nullptr;
    unsigned long long* masks = nullptr;
    if (prm.tuple_test) {
        TDV_TRY(ws_alloc(ctx, (size_t)tuple_cap, &tuples));
        TDV_TRY(ws_alloc(ctx, ((size_t)TDV_FGR_TRIAL_CHUNK << FGR_CHUNK_MAX_SHIFT) / 64, &masks));
    }
    const int bs = (ns + 255) / 256, bt = (nt + 255) / 256;
    double* slabs = nullptr;
    TDV_TRY(ws_alloc(ctx, (size_t)3 * (bs + bt), &slabs));
    TDV_TRY(pin_reserve(ctx, 256));

    // (i) matches, both ways (the two outputs were allocated above: neither call's scratch reaches them)
    TDV_TRY(feature_match_dev(ctx, d_fs, ns, d_ft, nt, cst));
    TDV_TRY(feature_match_dev(ctx, d_ft, nt, d_fs, ns, cts));
    // (ii) mutual pairs
    k_fgr_mutual_flags<<<bs, 256, 0, s>>>(cst, cts, ns, nt, flags);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(exclusive_scan_dev(ctx, flags, ns, offs, blk));
    k_fgr_mutual_scatter<<<bs, 256, 0, s>>>(cst, flags, offs, ns, mutual);
    // (iv) means and scale (independent of the pairs)
    k_fgr_mean_partial<<<bs + bt, 256, 0, s>>>(d_src, ns, d_tgt, nt, bs, slabs);
    k_fgr_mean_final<<<1, 256, 0, s>>>(slabs, bs, bt, ns, nt, d_norm);
    k_fgr_scale_partial<<<bs + bt, 256, 0, s>>>(d_src, ns, d_tgt, nt, bs, d_norm, slabs);
    k_fgr_scale_final<<<1, 256, 0, s>>>(slabs, bs + bt, prm.use_absolute_scale, d_norm);
    TDV_CHECK_LAUNCH(ctx);

    // (iii) tuple test, chunk by chunk; the first chunk goes out before the mutual count is known (the kernels read it on the device)
    const int* h_blk = reinterpret_cast<const int*>(ctx->pin);
    const double s_tuple = (double)prm.tuple_scale;
    long long trials_run = 0;
    int n_mutual = -1, kept = 0;
    for (int k = 0;; ++k) {
        const long long chunk = (long long)TDV_FGR_TRIAL_CHUNK << std::min(k, FGR_CHUNK_MAX_SHIFT);
        if (prm.tuple_test && (n_mutual < 0 || trials_run < 100LL * n_mutual)) {
            k_fgr_tuple_flags<<<(unsigned)(chunk / 256), 256, 0, s>>>(mutual, blk, d_src, d_tgt, (unsigned long long)trials_run, prm.seed,
                                                                     s_tuple, masks);
            k_fgr_tuple_compact<<<1, FGR_COMPACT_THREADS, 0, s>>>(masks, (int)(chunk / 64 / FGR_COMPACT_THREADS), (unsigned long long)trials_run,
                                                                  mutual, blk, prm.seed, prm.maximum_tuple_count, blk + 1, tuples);
            TDV_CHECK_LAUNCH(ctx);
            trials_run += chunk;
        } else if (n_mutual >= 0) {
            break;
        }
        TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, blk, 8, hipMemcpyDeviceToHost, s));
        TDV_HIP(ctx, hipStreamSynchronize(s));
        n_mutual = h_blk[0]; kept = h_blk[1];
        if (!prm.tuple_test || kept >= prm.maximum_tuple_count || trials_run >= 100LL * n_mutual) break;
    }
    trials_run = prm.tuple_test ? std::min(trials_run, 100LL * n_mutual) : 0;
    const int n_tuple = 3 * kept;
    if (pairs) {
        pairs->mutual = mutual; pairs->tuple = tuples; pairs->n_mutual = n_mutual; pairs->n_tuple = n_tuple; pairs->trials_run = trials_run;
        return TDV_OK;
    }
    const int n_corr = prm.tuple_test ? n_tuple : n_mutual;
    const int2* corr = prm.tuple_test ? tuples : mutual;

    // (v) optimisation, (vi) score
    double* PQ = nullptr;
    TDV_TRY(ws_alloc(ctx, (size_t)6 * std::max(n_corr, 1), &PQ));
    k_fgr_optimize<<<1, FGR_OPT_THREADS, 0, s>>>(corr, n_corr, d_src, d_tgt, d_norm, PQ, prm.iteration_number, prm.decrease_mu,
                                                 (double)prm.maximum_correspondence_distance, (double)prm.division_factor, d_hyp12);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(ransac_score_pose_dev(ctx, d_src, ns, d_tgt, nt, cst, d_hyp12, voxel, d_out2));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, d_out2, 2 * sizeof(double) + 12 * sizeof(float), hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    const double* h_o2 = reinterpret_cast<const double*>(ctx->pin);
    const float* h_hyp = reinterpret_cast<const float*>(h_o2 + 2);
    tdv_fgr_result r{};
    for (int c = 0; c < 3; ++c) for (int q = 0; q < 3; ++q) r.T[4 * c + q] = h_hyp[3 * c + q];
    r.T[12] = h_hyp[9]; r.T[13] = h_hyp[10]; r.T[14] = h_hyp[11]; r.T[15] = 1.f;
    r.inliers = (int)(h_o2[1] + 0.5);
    r.fitness = (float)r.inliers / (float)ns;
    r.rmse = r.inliers > 0 ? std::sqrt((float)h_o2[0] / (float)r.inliers) : 999.0f;   // as ransac_run_dev (registration.cpp:282)
    r.n_mutual = n_mutual; r.n_tuple = n_tuple; r.degenerate = n_corr < 10 ? 1 : 0; r.trials_run = trials_run;
    *out = r;
    return TDV_OK;
}

// every argument, before anything is enqueued (include/tdv_hip.h: tdv_fgr)
bool fgr_args_ok(const tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft,
                 float voxel_size, const tdv_fgr_params* p) {
    if (!ctx || !p || ns < 0 || nt < 0) return false;
    if (ns > 0 && (!src || !fs)) return false;
    if (nt > 0 && (!tgt || !ft)) return false;
    if (!std::isfinite(voxel_size) || !(voxel_size > 0.f)) return false;
    if (!std::isfinite(p->division_factor) || !(p->division_factor > 1.f)) return false;
    if (!std::isfinite(p->tuple_scale) || !(p->tuple_scale > 0.f && p->tuple_scale <= 1.f)) return false;
    if (!std::isfinite(p->maximum_correspondence_distance) || !(p->maximum_correspondence_distance > 0.f)) return false;
    return p->iteration_number >= 0 && p->maximum_tuple_count >= 1;
}

void fgr_empty(tdv_fgr_result* out) {
    std::memset(out, 0, sizeof(*out));
    for (int i = 0; i < 16; ++i) out->T[i] = (i % 5 == 0) ? 1.f : 0.f;
    out->degenerate = 1;
}

// host arrays: both clouds and their descriptors into the workspace
struct FgrClouds { float *src, *tgt, *fs, *ft; };
int fgr_upload(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft, FgrClouds* d) {
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d->src));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d->tgt));
    TDV_TRY(upload(ctx, fs, (size_t)ns * 33, &d->fs));
    return upload(ctx, ft, (size_t)nt * 33, &d->ft);
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_fgr_default_params(tdv_fgr_params* p) {
    if (!p) return;
    p->division_factor = 1.4f; p->maximum_correspondence_distance = 0.025f; p->tuple_scale = 0.95f; p->iteration_number = 64;
    p->maximum_tuple_count = 1000; p->use_absolute_scale = 0; p->decrease_mu = 1; p->tuple_test = 1; p->seed = 42u;
}

int tdv_fgr(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft, float voxel_size,
            const tdv_fgr_params* params, tdv_fgr_result* out) {
    if (!out || !fgr_args_ok(ctx, src, ns, tgt, nt, fs, ft, voxel_size, params)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (ns == 0 || nt == 0) { fgr_empty(out); return TDV_OK; }
    FgrClouds d;
    TDV_TRY(fgr_upload(ctx, src, ns, tgt, nt, fs, ft, &d));
    return fgr_run_dev(ctx, d.src, ns, d.tgt, nt, d.fs, d.ft, voxel_size, *params, out, nullptr);
}

int tdv_fgr_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* d_fs, const float* d_ft, float voxel_size,
                const tdv_fgr_params* params, tdv_fgr_result* out) {
    if (!out || !fgr_args_ok(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, voxel_size, params)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (ns == 0 || nt == 0) { fgr_empty(out); return TDV_OK; }
    return fgr_run_dev(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, voxel_size, *params, out, nullptr);
}

int tdv_fgr_correspondences(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft,
                            const tdv_fgr_params* params, int* out_mutual, int cap_mutual, int* out_tuple, int cap_tuple,
                            int* n_mutual, int* n_tuple, long long* trials_run) {
    if (!n_mutual || !n_tuple || !trials_run || cap_mutual < 0 || cap_tuple < 0 || (cap_mutual > 0 && !out_mutual) ||
        (cap_tuple > 0 && !out_tuple) || !fgr_args_ok(ctx, src, ns, tgt, nt, fs, ft, 1.f, params))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    *n_mutual = 0; *n_tuple = 0; *trials_run = 0;
    if (ns == 0 || nt == 0) return TDV_OK;
    FgrClouds d;
    TDV_TRY(fgr_upload(ctx, src, ns, tgt, nt, fs, ft, &d));
    FgrPairs pr;
    TDV_TRY(fgr_run_dev(ctx, d.src, ns, d.tgt, nt, d.fs, d.ft, 1.f, *params, nullptr, &pr));
    *n_mutual = pr.n_mutual; *n_tuple = pr.n_tuple; *trials_run = pr.trials_run;
    if (pr.n_mutual > cap_mutual || pr.n_tuple > cap_tuple) return TDV_ERR_BAD_ARG;
    TDV_TRY(download(ctx, reinterpret_cast<int2*>(out_mutual), pr.mutual, (size_t)pr.n_mutual));
    TDV_TRY(download(ctx, reinterpret_cast<int2*>(out_tuple), pr.tuple, (size_t)pr.n_tuple));
    return finish(ctx);
}

}  // extern "C"
