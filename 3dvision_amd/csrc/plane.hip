// Plane segmentation by RANSAC on gfx950: include/tdv_hip.h (tdv_segment_planes) states every step and its order.
//
// The host enqueues every round and every chunk up front; the rounds and the early stop are decided on the device, and the call reads
// back once, at the end.  Round k (candidates = the input for k = 0, then the previous round's compaction):
//  (i)   k_plane_begin: m_k = the previous compaction's total; the search ends below 3 candidates.
//  (ii)  per chunk of TDV_PLANE_CHUNK hypotheses: k_plane_hyp (one thread per hypothesis: the Philox draw, three gathered points, the f64
//        plane; an invalid one gets a NaN offset, so that it scores nothing), k_plane_score (the chunk's planes in LDS, the candidates
//        streamed PLANE_PPT per thread, a ballot per test, exact integer counts per wave in LDS, one integer atomic per hypothesis and
//        workgroup) and k_plane_select (one workgroup: the arg-max with the lowest t on ties, the early-stop rule).  Once a round has
//        stopped, the later chunks of that round exit at once.
//  (iii) k_plane_accept (one lane): the winner's plane, drawn again from its t (the same bits), and the acceptance rule.
//  (iv)  k_plane_label: labels, the candidates that stay, per-workgroup f64 sums of dist^2 and p over the inliers; k_plane_mean: their
//        fixed tree; k_plane_cov: the centred products per workgroup (refit only); k_plane_finish: their tree, the 3x3 eigen step in one
//        lane, the result record.
//  (v)   exclusive_scan_dev + k_plane_compact: the next round's candidates (points and original indices); the count stays on the device.
// Everything is f64 from the f32 inputs without contraction (the library is built with -ffp-contract=off; the pragma states it here).
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "philox.hpp"
#include "fixed_tree.hpp"
#include <cmath>
#include <cstring>
#include <algorithm>

namespace tdv {

namespace {

constexpr int PLANE_PPT = 8;                 // candidates per thread and pass of k_plane_score
constexpr int PLANE_SCORE_BLOCKS_MAX = 1024;
constexpr int PLANE_HYP_THREADS = 256;
static_assert(TDV_PLANE_CHUNK % PLANE_HYP_THREADS == 0, "a chunk's hypotheses split evenly over the workgroups");

// device state of one call (workspace)
struct PlaneState {
    int m;             // candidates of the current round
    int m_next;        // the last compaction's total
    int active;        // the search goes on
    int done;          // the current round has stopped (or never started)
    int best_count, best_t, run;
    int accepted;      // the current round's plane is kept
    int n_planes;
    int pad;
    double plane[4];   // the current round's winner (f64)
    double mean[3];    // inlier mean
    double sd2;        // sum of dist^2 over the inliers
};

// Steps 1-2 for hypothesis t of round k over m candidates; false: invalid.
__device__ __forceinline__ bool plane_hypothesis(const float* __restrict__ cand, unsigned m, unsigned t, unsigned k, uint32_t seed,
                                                 double pl[4]) {
    uint32_t x[4];
    philox4x32_10(t, k, 0u, 0u, seed, 1u, x);
    const unsigned i0 = (unsigned)(((unsigned long long)x[0] * m) >> 32), i1 = (unsigned)(((unsigned long long)x[1] * m) >> 32),
                   i2 = (unsigned)(((unsigned long long)x[2] * m) >> 32);
    if (i0 == i1 || i0 == i2 || i1 == i2) return false;
    const double p0x = cand[3 * (size_t)i0], p0y = cand[3 * (size_t)i0 + 1], p0z = cand[3 * (size_t)i0 + 2];
    const double ux = (double)cand[3 * (size_t)i1] - p0x, uy = (double)cand[3 * (size_t)i1 + 1] - p0y, uz = (double)cand[3 * (size_t)i1 + 2] - p0z;
    const double vx = (double)cand[3 * (size_t)i2] - p0x, vy = (double)cand[3 * (size_t)i2 + 1] - p0y, vz = (double)cand[3 * (size_t)i2 + 2] - p0z;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double s = (nx * nx + ny * ny) + nz * nz;
    if (!(s > 0.0) || !isfinite(s)) return false;
    const double r = sqrt(s);
    pl[0] = nx / r; pl[1] = ny / r; pl[2] = nz / r;
    pl[3] = -((pl[0] * p0x + pl[1] * p0y) + pl[2] * p0z);
    return true;
}

__device__ __forceinline__ double plane_dist(double a, double b, double c, double d, double px, double py, double pz) {
    return fabs(((a * px + b * py) + c * pz) + d);
}

__global__ void k_plane_init(PlaneState* st, int n) {
    if (threadIdx.x != 0) return;
    PlaneState z{};
    z.m_next = n; z.active = 1; z.done = 1;
    *st = z;
}

__global__ void k_plane_begin(PlaneState* st) {
    if (threadIdx.x != 0) return;
    st->m = st->m_next;
    if (st->active && st->m < 3) st->active = 0;
    st->done = !st->active;
    st->best_count = -1; st->best_t = 0; st->run = 0; st->accepted = 0;
}

// one thread per hypothesis t0 + i, i < h
__global__ __launch_bounds__(PLANE_HYP_THREADS) void k_plane_hyp(const float* __restrict__ cand, const PlaneState* __restrict__ st,
                                                                 unsigned k, unsigned t0, int h, uint32_t seed, double4* __restrict__ planes) {
    if (st->done) return;
    const int i = blockIdx.x * PLANE_HYP_THREADS + threadIdx.x;
    if (i >= h) return;
    double pl[4];
    planes[i] = plane_hypothesis(cand, (unsigned)st->m, t0 + (unsigned)i, k, seed, pl) ? make_double4(pl[0], pl[1], pl[2], pl[3])
                                                                                       : make_double4(0.0, 0.0, 0.0, __builtin_nan(""));
}

// counts[i] += inlier candidates of hypothesis i (exact integers)
__global__ __launch_bounds__(256) void k_plane_score(const float* __restrict__ cand, const PlaneState* __restrict__ st,
                                                     const double4* __restrict__ planes, int h, double thr, int* __restrict__ counts) {
    __shared__ double4 sp[TDV_PLANE_CHUNK];
    __shared__ int sc[4][TDV_PLANE_CHUNK];
    if (st->done) return;
    const int m = st->m;
    constexpr int PER_BLOCK = 256 * PLANE_PPT;
    if ((long long)blockIdx.x * PER_BLOCK >= m) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < h; i += 256) {
        sp[i] = planes[i];
        sc[0][i] = 0; sc[1][i] = 0; sc[2][i] = 0; sc[3][i] = 0;
    }
    __syncthreads();
    for (long long base = (long long)blockIdx.x * PER_BLOCK; base < m; base += (long long)gridDim.x * PER_BLOCK) {
        double px[PLANE_PPT], py[PLANE_PPT], pz[PLANE_PPT];
#pragma unroll
        for (int e = 0; e < PLANE_PPT; ++e) {
            const long long j = base + e * 256 + tid;
            if (j < m) {
                px[e] = cand[3 * j]; py[e] = cand[3 * j + 1]; pz[e] = cand[3 * j + 2];
            } else {
                px[e] = py[e] = pz[e] = __builtin_nan("");
            }
        }
        for (int i = 0; i < h; ++i) {
            const double4 q = sp[i];
            int c = 0;
#pragma unroll
            for (int e = 0; e < PLANE_PPT; ++e) c += __popcll(__ballot(plane_dist(q.x, q.y, q.z, q.w, px[e], py[e], pz[e]) < thr));
            if (lane == 0) sc[wv][i] += c;
        }
    }
    __syncthreads();
    for (int i = tid; i < h; i += 256) {
        const int c = (sc[0][i] + sc[1][i]) + (sc[2][i] + sc[3][i]);
        if (c) atomicAdd(counts + i, c);
    }
}

// One workgroup: the chunk's arg-max (lowest t on ties) against the best so far, then the stop rule.  Leaves counts zeroed.
__global__ __launch_bounds__(1024) void k_plane_select(PlaneState* st, int* __restrict__ counts, unsigned t0, int h, int num_iterations,
                                                       double probability) {
    __shared__ unsigned long long wbest[16];
    if (st->done) return;
    const int tid = threadIdx.x;
    unsigned long long key = 0;                         // (count + 1) << 32 | ~t: the largest key is the largest count, lowest t
    if (tid < h) {
        const int c = counts[tid];
        counts[tid] = 0;
        key = ((unsigned long long)(unsigned)(c + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (t0 + (unsigned)tid));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) wbest[tid >> 6] = key;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < 16; ++w) key = wbest[w] > key ? wbest[w] : key;
    const int bc = (int)(key >> 32) - 1;
    const int bt = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    if (bc > st->best_count) { st->best_count = bc; st->best_t = bt; }     // an earlier chunk keeps its (lower) t on a tie
    st->run += h;
    if ((long long)t0 + h >= num_iterations) { st->done = 1; return; }
    const int b = st->best_count;
    if (probability < 1.0 && b > 0) {
        const double f = (double)b / (double)st->m;
        if (f >= 1.0) { st->done = 1; return; }
        const double L = log(1.0 - (f * f) * f);
        if (L < 0.0 && (double)st->run >= log(1.0 - probability) / L) st->done = 1;
    }
}

__global__ void k_plane_accept(const float* __restrict__ cand, PlaneState* st, unsigned k, uint32_t seed, int min_inliers) {
    if (threadIdx.x != 0) return;
    st->accepted = 0;
    if (!st->active) return;
    double pl[4];
    const bool ok = plane_hypothesis(cand, (unsigned)st->m, (unsigned)st->best_t, k, seed, pl);
    if (!ok || st->best_count < min_inliers) { st->active = 0; return; }
    st->accepted = 1;
    for (int a = 0; a < 4; ++a) st->plane[a] = pl[a];
}

// over j < n_up: keep[j] = candidate j stays; labels of the inliers; per workgroup the f64 sums of dist^2, x, y, z over the inliers
__global__ __launch_bounds__(256) void k_plane_label(const float* __restrict__ cand, const int* __restrict__ cand_idx,
                                                     const PlaneState* __restrict__ st, int k, double thr, int n_up,
                                                     int* __restrict__ labels, int* __restrict__ keep, double* __restrict__ part) {
    __shared__ double lds4[4];
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int m = st->m;
    const bool acc = st->accepted != 0;
    double px = 0.0, py = 0.0, pz = 0.0, dist = 0.0;
    bool in = false;
    if (j < m) {
        px = cand[3 * (size_t)j]; py = cand[3 * (size_t)j + 1]; pz = cand[3 * (size_t)j + 2];
        if (acc) {
            dist = plane_dist(st->plane[0], st->plane[1], st->plane[2], st->plane[3], px, py, pz);
            in = dist < thr;
        }
    }
    if (j < n_up) keep[j] = (j < m && !in) ? 1 : 0;
    if (in && labels) labels[cand_idx ? cand_idx[j] : j] = k;
    if (!acc) return;                                   // uniform over the launch
    const double v[4] = {in ? dist * dist : 0.0, in ? px : 0.0, in ? py : 0.0, in ? pz : 0.0};
    for (int a = 0; a < 4; ++a) {
        const double s = tree_block_sum(v[a], lds4);
        if (threadIdx.x == 0) part[4 * (size_t)blockIdx.x + a] = s;
    }
}

__global__ __launch_bounds__(256) void k_plane_mean(PlaneState* st, const double* __restrict__ part, int nb) {
    __shared__ double lds4[4];
    if (!st->accepted) return;
    const double cnt = (double)st->best_count;
    for (int a = 0; a < 4; ++a) {
        const double s = tree_partials_sum(part, nb, lds4, 4, a);
        if (threadIdx.x == 0) { if (a == 0) st->sd2 = s; else st->mean[a - 1] = s / cnt; }
        __syncthreads();
    }
}

// per workgroup the six centred products (xx, xy, xz, yy, yz, zz) over the inliers
__global__ __launch_bounds__(256) void k_plane_cov(const float* __restrict__ cand, const PlaneState* __restrict__ st, double thr,
                                                   double* __restrict__ part) {
    __shared__ double lds4[4];
    if (!st->accepted) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (j < st->m) {
        const double px = cand[3 * (size_t)j], py = cand[3 * (size_t)j + 1], pz = cand[3 * (size_t)j + 2];
        if (plane_dist(st->plane[0], st->plane[1], st->plane[2], st->plane[3], px, py, pz) < thr) {
            dx = px - st->mean[0]; dy = py - st->mean[1]; dz = pz - st->mean[2];
        }
    }
    const double v[6] = {dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
    for (int a = 0; a < 6; ++a) {
        const double s = tree_block_sum(v[a], lds4);
        if (threadIdx.x == 0) part[6 * (size_t)blockIdx.x + a] = s;
    }
}

}  // namespace

// Cyclic Jacobi on a symmetric 3x3 matrix (f64): the unit eigenvector of the smallest eigenvalue (lowest index on ties) into e.
// Rotations in the order (0,1), (0,2), (1,2), at most 32 sweeps; a rotation is skipped when its off-diagonal entry is 0.  Compile-time
// indices only (the rotation loop is unrolled): registers, no scratch and no LDS.
__host__ __device__ inline void plane_smallest_eigvec(const double A[6], double e[3]) {
    double a[3][3] = {{A[0], A[1], A[2]}, {A[1], A[3], A[4]}, {A[2], A[4], A[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 32; ++sweep) {
        if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double arp = a[r][p], arq = a[r][q];
                a[r][p] = c * arp - s * arq; a[r][q] = s * arp + c * arq;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double apr = a[p][r], aqr = a[q][r];
                a[p][r] = c * apr - s * aqr; a[q][r] = s * apr + c * aqr;
            }
            a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double vrp = v[r][p], vrq = v[r][q];
                v[r][p] = c * vrp - s * vrq; v[r][q] = s * vrp + c * vrq;
            }
        }
    }
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    const int lo = (l1 < l0) ? ((l2 < l1) ? 2 : 1) : ((l2 < l0) ? 2 : 0);   // the smallest, lowest index on ties
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = lo == 0 ? v[i][0] : (lo == 1 ? v[i][1] : v[i][2]);
    const double nrm = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = w[i] / nrm;
}

namespace {

__global__ __launch_bounds__(256) void k_plane_finish(PlaneState* st, const double* __restrict__ part, int nb, int refit,
                                                      tdv_plane_result* __restrict__ res) {
    __shared__ double lds4[4];
    if (!st->accepted) return;
    double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (refit) {
        for (int a = 0; a < 6; ++a) {
            const double s = tree_partials_sum(part, nb, lds4, 6, a);
            if (threadIdx.x == 0) C[a] = s;
            __syncthreads();
        }
    }
    if (threadIdx.x != 0) return;
    const double* pl = st->plane;
    const double sg = pl[3] < 0.0 ? -1.0 : 1.0;
    tdv_plane_result r;
    for (int a = 0; a < 4; ++a) r.hypothesis[a] = pl[3] < 0.0 ? -(float)pl[a] : (float)pl[a];
    for (int a = 0; a < 4; ++a) r.plane[a] = r.hypothesis[a];
    if (refit) {
        double e[3];
        plane_smallest_eigvec(C, e);
        const double dot = (e[0] * (sg * pl[0]) + e[1] * (sg * pl[1])) + e[2] * (sg * pl[2]);
        if (dot < 0.0) { e[0] = -e[0]; e[1] = -e[1]; e[2] = -e[2]; }
        const double d = -((e[0] * st->mean[0] + e[1] * st->mean[1]) + e[2] * st->mean[2]);
        if (isfinite(e[0]) && isfinite(e[1]) && isfinite(e[2]) && isfinite(d)) {
            r.plane[0] = (float)e[0]; r.plane[1] = (float)e[1]; r.plane[2] = (float)e[2]; r.plane[3] = (float)d;
        }
    }
    const int cnt = st->best_count;
    r.fitness = (float)((double)cnt / (double)st->m);
    r.rmse = (float)sqrt(st->sd2 / (double)cnt);
    r.inliers = cnt; r.candidates = st->m; r.best_iteration = st->best_t; r.iterations_run = st->run;
    res[st->n_planes] = r;
    st->n_planes += 1;
}

// out[offs[j]] = in[j] for the candidates that stay (out_idx: their original indices, optional)
__global__ __launch_bounds__(256) void k_plane_compact(const int* __restrict__ keep, const int* __restrict__ offs, int n_up,
                                                       const float* __restrict__ in_xyz, const int* __restrict__ in_idx,
                                                       float* __restrict__ out_xyz, int* __restrict__ out_idx) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_up || !keep[j]) return;
    const int o = offs[j];
    out_xyz[3 * (size_t)o] = in_xyz[3 * (size_t)j];
    out_xyz[3 * (size_t)o + 1] = in_xyz[3 * (size_t)j + 1];
    out_xyz[3 * (size_t)o + 2] = in_xyz[3 * (size_t)j + 2];
    if (out_idx) out_idx[o] = in_idx ? in_idx[j] : j;
}

// every argument, before anything is enqueued (include/tdv_hip.h: tdv_segment_planes)
bool plane_args_ok(const tdv_ctx* ctx, const float* xyz, int n, const tdv_plane_params* p, const tdv_plane_result* out, const int* n_planes) {
    if (!ctx || !p || !out || !n_planes || n < 0 || (n > 0 && !xyz)) return false;
    if (!std::isfinite(p->distance_threshold) || !(p->distance_threshold > 0.f)) return false;
    if (!(p->probability > 0.0 && p->probability <= 1.0)) return false;
    return p->num_iterations >= 1 && p->max_planes >= 1 && p->max_planes <= TDV_PLANE_MAX && p->min_inliers >= 3;
}

// the whole call on device memory; h_labels (host, optional) receives the labels through d_labels
int plane_run_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_plane_params& prm, tdv_plane_result* out, int* n_planes,
                  int* d_labels, float* d_rest, int* n_rest, int* h_labels) {
    hipStream_t s = ctx->stream;
    if (d_labels && n > 0) TDV_HIP(ctx, hipMemsetAsync(d_labels, 0xFF, (size_t)n * sizeof(int), s));   // -1
    if (n < 3) {
        if (d_rest && n > 0) TDV_HIP(ctx, hipMemcpyAsync(d_rest, d_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
        TDV_TRY(download(ctx, h_labels, d_labels, (size_t)n));
        TDV_TRY(finish(ctx));
        *n_planes = 0;
        if (n_rest) *n_rest = n;
        return TDV_OK;
    }
    const int max_planes = prm.max_planes;
    const size_t rec_bytes = sizeof(PlaneState) + (size_t)max_planes * sizeof(tdv_plane_result);
    char* blk = nullptr;
    TDV_TRY(ws_alloc(ctx, rec_bytes, &blk));
    PlaneState* st = reinterpret_cast<PlaneState*>(blk);
    tdv_plane_result* d_res = reinterpret_cast<tdv_plane_result*>(blk + sizeof(PlaneState));
    double4* planes; int *counts, *keep, *offs;
    float* cxyz[2] = {nullptr, nullptr}; int* cidx[2] = {nullptr, nullptr};
    TDV_TRY(ws_alloc(ctx, (size_t)TDV_PLANE_CHUNK, &planes));
    TDV_TRY(ws_alloc(ctx, (size_t)TDV_PLANE_CHUNK, &counts));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &keep));
    TDV_TRY(ws_alloc(ctx, (size_t)n, &offs));
    const int rounds_with_output = max_planes > 1 ? 2 : 1;          // a single round compacts straight into d_rest (or nowhere)
    for (int b = 0; b < rounds_with_output; ++b) {
        TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &cxyz[b]));
        TDV_TRY(ws_alloc(ctx, (size_t)n, &cidx[b]));
    }
    const int nb = (n + 255) / 256;
    double* part;
    TDV_TRY(ws_alloc(ctx, (size_t)6 * nb, &part));
    TDV_TRY(pin_reserve(ctx, rec_bytes));
    TDV_HIP(ctx, hipMemsetAsync(counts, 0, TDV_PLANE_CHUNK * sizeof(int), s));
    k_plane_init<<<1, 64, 0, s>>>(st, n);
    TDV_CHECK_LAUNCH(ctx);

    const double thr = (double)prm.distance_threshold;
    const int score_blocks = std::min((n + 256 * PLANE_PPT - 1) / (256 * PLANE_PPT), PLANE_SCORE_BLOCKS_MAX);
    const int n_chunks = (prm.num_iterations + TDV_PLANE_CHUNK - 1) / TDV_PLANE_CHUNK;
    for (int k = 0; k < max_planes; ++k) {
        const float* in_xyz = k == 0 ? d_xyz : cxyz[(k - 1) & 1];
        const int* in_idx = k == 0 ? nullptr : cidx[(k - 1) & 1];
        k_plane_begin<<<1, 64, 0, s>>>(st);
        for (int c = 0; c < n_chunks; ++c) {
            const unsigned t0 = (unsigned)c * TDV_PLANE_CHUNK;
            const int h = std::min(TDV_PLANE_CHUNK, prm.num_iterations - (int)t0);
            k_plane_hyp<<<(h + PLANE_HYP_THREADS - 1) / PLANE_HYP_THREADS, PLANE_HYP_THREADS, 0, s>>>(in_xyz, st, (unsigned)k, t0, h, prm.seed, planes);
            k_plane_score<<<score_blocks, 256, 0, s>>>(in_xyz, st, planes, h, thr, counts);
            k_plane_select<<<1, 1024, 0, s>>>(st, counts, t0, h, prm.num_iterations, prm.probability);
        }
        k_plane_accept<<<1, 64, 0, s>>>(in_xyz, st, (unsigned)k, prm.seed, prm.min_inliers);
        k_plane_label<<<nb, 256, 0, s>>>(in_xyz, in_idx, st, k, thr, n, d_labels, keep, part);
        k_plane_mean<<<1, 256, 0, s>>>(st, part, nb);
        if (prm.refit) k_plane_cov<<<nb, 256, 0, s>>>(in_xyz, st, thr, part);
        k_plane_finish<<<1, 256, 0, s>>>(st, part, nb, prm.refit, d_res);
        TDV_CHECK_LAUNCH(ctx);
        const bool last = k == max_planes - 1;
        if (last && !d_rest) break;
        TDV_TRY(exclusive_scan_dev(ctx, keep, n, offs, &st->m_next));
        k_plane_compact<<<nb, 256, 0, s>>>(keep, offs, n, in_xyz, in_idx, last ? d_rest : cxyz[k & 1], last ? nullptr : cidx[k & 1]);
        TDV_CHECK_LAUNCH(ctx);
    }
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, blk, rec_bytes, hipMemcpyDeviceToHost, s));
    TDV_TRY(download(ctx, h_labels, d_labels, (size_t)n));
    TDV_TRY(finish(ctx));
    PlaneState hs;
    std::memcpy(&hs, ctx->pin, sizeof(hs));
    std::memcpy(out, ctx->pin + sizeof(PlaneState), (size_t)hs.n_planes * sizeof(tdv_plane_result));
    *n_planes = hs.n_planes;
    if (n_rest) {
        int rest = n;
        for (int i = 0; i < hs.n_planes; ++i) rest -= out[i].inliers;
        *n_rest = rest;
    }
    return TDV_OK;
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_plane_default_params(tdv_plane_params* p) {
    if (!p) return;
    p->probability = 0.99999999; p->distance_threshold = 0.01f; p->num_iterations = 100; p->max_planes = 1; p->min_inliers = 3;
    p->refit = 1; p->seed = 42u;
}

int tdv_segment_planes(tdv_ctx* ctx, const float* xyz, int n, const tdv_plane_params* params, tdv_plane_result* out, int* n_planes,
                       int* labels) {
    if (!plane_args_ok(ctx, xyz, n, params, out, n_planes)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float* d_xyz;
    int* d_labels = nullptr;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    if (labels && n > 0) TDV_TRY(ws_alloc(ctx, (size_t)n, &d_labels));
    return plane_run_dev(ctx, d_xyz, n, *params, out, n_planes, d_labels, nullptr, nullptr, labels);
}

int tdv_segment_planes_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_plane_params* params, tdv_plane_result* out, int* n_planes,
                           int* d_labels, float* d_rest_xyz, int* n_rest) {
    if (!plane_args_ok(ctx, d_xyz, n, params, out, n_planes)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return plane_run_dev(ctx, d_xyz, n, *params, out, n_planes, d_labels, d_rest_xyz, n_rest, nullptr);
}

}  // extern "C"
