// PPF matching (point-pair-feature voting) on gfx950: include/tdv_hip.h (tdv_ppf_match) states every rule.
//
// Model table (ppf_model_run), nothing returns to the host before the end:
//  (i)   k_ppf_diameter: one workgroup, min / max of the finite points (order-free), writes the state block (diameter, distance_step).
//  (ii)  k_ppf_model_keys: one thread per ordered pair p = i * nt + j: its key, or the sentinel n_keys (no key; the diagonal included).
//  (iii) radix_sort_pairs_dev on the keys with value p: stable, and the input is in ascending p, so the order is (key, p).
//  (iv)  k_ppf_offsets: offsets[k] = the lower bound of k in the sorted keys (one binary search per key; offsets[n_keys] = n_pairs, the
//        first sentinel); k_ppf_model_fill: pair and alpha bits of every keyed entry (alpha is formed again from the pair).
// Match (ppf_match_run):
//  (v)   k_ppf_vote: one workgroup per work item = (instance, reference point), items numbered in instance order (grid-stride where there
//        are more; a single cloud is the batch of one, without the offset arrays).  The counters are LDS (static: CELLS) or a slab
//        of the workspace (CELLS = 0).  A tile of PPF_THREADS scene points: each lane forms one pair's key, alpha and bucket; a block scan
//        of the bucket lengths numbers the tile's table entries 0 .. total - 1, and the lanes take them round robin, finding an entry's
//        pair by a binary search of the scanned lengths - so a long bucket is shared by the whole workgroup instead of stalling one lane.
//        One integer atomic add per entry.  Then one packed-key maximum over the counters; lane 0 writes the peak and, beside it, the
//        two points of the peak (12 floats) for the host's pose stage.  No ticket words, no spinning, no cooperative launch.
//  (vi)  host, f64: poses of the peaks, clustering (rule 7: ppf_rank); then icp_correspondences_dev per returned pose.
// Batch (ppf_match_batch_run): (v) once over every instance's reference points, one read-back of all peaks, (vi)'s ppf_rank per instance,
//        then k_ppf_score: every returned pose of every instance against the model in LDS (lds_scan.hpp: the scan k_icp_small runs), one
//        lane per source point, d2 and the accepted flag of every (pose, point) read back in one copy and summed as (vi) sums them.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "libm_f32.hpp"
#include "lds_scan.hpp"
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>

namespace tdv {

namespace {

constexpr int PPF_THREADS = 512;
constexpr int PPF_WAVES = PPF_THREADS / 64;
constexpr int PPF_LDS_SMALL = 10000;      // the smaller LDS variant: 46 KiB with the staging, so that three workgroups fit a CU's LDS (occupancy not measured)
constexpr int PPF_GRID_LDS = 2048;        // workgroups of a voting launch at most: a few per CU (256 CUs); chosen, not tuned by measurement
constexpr int PPF_GRID_SLAB = 512;        // ... with slabs (two per CU; chosen, not tuned), and no more than fit PPF_SLAB_BYTES (at least one)
constexpr size_t PPF_SLAB_BYTES = (size_t)128 << 20;   // what a match may take of the arena for slabs: 64 workgroups at 2048 x 256 counters
constexpr float PPF_PI = 3.14159274f, PPF_TWO_PI = 6.28318548f;
static_assert(TDV_PPF_LDS_CELLS * 4 + PPF_THREADS * 12 + 256 <= 160 * 1024, "counters + tile staging within one CU's LDS");

// what the kernels need of the parameters; step is the model's distance_step
struct PpfQuant { float step, astep, rstep; int A, R, n_dist, n_keys, flip; };
// device state of a model build, read back at the end
struct PpfState { float diameter, step; };
// a point with (frame = true) the frame of rule 3
struct PpfPoint { float px, py, pz, nx, ny, nz, wx, wy, wz, ca, cb; bool neg, ok; };

__device__ __forceinline__ bool ppf_finite(float v) { return fabsf(v) < INFINITY; }      // false for NaN

// rule 0 (and the frame of rule 3)
__device__ __forceinline__ PpfPoint ppf_point(const float* __restrict__ xyz, const float* __restrict__ nrm, int i, bool flip, bool frame) {
    PpfPoint a;
    a.px = xyz[3 * (size_t)i]; a.py = xyz[3 * (size_t)i + 1]; a.pz = xyz[3 * (size_t)i + 2];
    a.nx = nrm[3 * (size_t)i]; a.ny = nrm[3 * (size_t)i + 1]; a.nz = nrm[3 * (size_t)i + 2];
    if (flip) { a.nx = -a.nx; a.ny = -a.ny; a.nz = -a.nz; }
    const float nn = (a.nx * a.nx + a.ny * a.ny) + a.nz * a.nz;
    a.ok = ppf_finite(a.px) && ppf_finite(a.py) && ppf_finite(a.pz) && ppf_finite(a.nx) && ppf_finite(a.ny) && ppf_finite(a.nz) && nn > 0.f &&
           nn < INFINITY;
    a.neg = a.nx < 0.f;
    a.wx = a.wy = a.wz = a.ca = a.cb = 0.f;
    if (a.ok && frame) {
        const float norm = sqrtf(nn);
        const float ux = a.nx / norm, uy = a.ny / norm, uz = a.nz / norm;
        a.wx = a.neg ? -ux : ux; a.wy = a.neg ? -uy : uy; a.wz = a.neg ? -uz : uz;
        const float k = 1.0f + a.wx;
        a.ca = a.wy / k; a.cb = a.wz / k;
    }
    return a;
}

__device__ __forceinline__ float ppf_ang(float ux, float uy, float uz, float vx, float vy, float vz) {
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return lm::atan2f_glibc(sqrtf((cx * cx + cy * cy) + cz * cz), (ux * vx + uy * vy) + uz * vz);
}

// rules 2 and 3 for the ordered pair (a, b) of usable points, a with its frame; false: no key
__device__ __forceinline__ bool ppf_pair(const PpfPoint& a, const PpfPoint& b, const PpfQuant& q, int* key, float* alpha) {
    const float dx = b.px - a.px, dy = b.py - a.py, dz = b.pz - a.pz;
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (!(len > 0.f) || !(len < INFINITY)) return false;
    const float q0f = floorf(len / q.step);
    if (!(q0f < (float)q.n_dist)) return false;                      // before the angles: most far pairs end here
    const float f1 = ppf_ang(a.nx, a.ny, a.nz, dx, dy, dz), f2 = ppf_ang(b.nx, b.ny, b.nz, dx, dy, dz),
                f3 = ppf_ang(a.nx, a.ny, a.nz, b.nx, b.ny, b.nz);
    if (f1 != f1 || f2 != f2 || f3 != f3) return false;
    const float t = a.wy * dy + a.wz * dz;
    const float y = (dy - a.ca * t) - a.wy * dx;
    float z = (dz - a.cb * t) - a.wz * dx;
    if (a.neg) z = -z;
    const float al = lm::atan2f_glibc(-z, y);
    if (al != al) return false;
    const int q1 = min((int)floorf(f1 / q.astep), q.A - 1), q2 = min((int)floorf(f2 / q.astep), q.A - 1), q3 = min((int)floorf(f3 / q.astep), q.A - 1);
    *key = (((int)q0f * q.A + q1) * q.A + q2) * q.A + q3;
    *alpha = al;
    return true;
}

// rule 5: the bin of alpha_m - alpha_s
__device__ __forceinline__ int ppf_bin(float am, float as, const PpfQuant& q) {
    float x = am - as;
    if (x < -PPF_PI) x = x + PPF_TWO_PI;
    else if (x >= PPF_PI) x = x - PPF_TWO_PI;
    return min(max((int)floorf((x + PPF_PI) / q.rstep), 0), q.R - 1);
}

// rule 1: one workgroup
__global__ __launch_bounds__(256) void k_ppf_diameter(const float* __restrict__ tgt, int nt, float rel, PpfState* st) {
    __shared__ float red[4][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < nt; i += 256) {
        const float x = tgt[3 * (size_t)i], y = tgt[3 * (size_t)i + 1], z = tgt[3 * (size_t)i + 2];
        if (ppf_finite(x) && ppf_finite(y) && ppf_finite(z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64)); }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float e[3];
    for (int a = 0; a < 3; ++a) {
        const float l = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
        const float h = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
        e[a] = h >= l ? h - l : 0.f;                                  // no finite point: 0
    }
    PpfState z;
    z.diameter = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    z.step = rel * z.diameter;
    *st = z;
}

// the key of ordered pair p = i * nt + j, or the sentinel n_keys
__global__ __launch_bounds__(256) void k_ppf_model_keys(const float* __restrict__ tgt, const float* __restrict__ tnrm, int nt,
                                                        const PpfState* __restrict__ st, PpfQuant q, unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ vals) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)nt * (unsigned)nt) return;
    const int i = (int)(p / (unsigned)nt), j = (int)(p - (unsigned)i * (unsigned)nt);
    q.step = st->step;
    int key = q.n_keys;
    if (i != j) {
        const PpfPoint a = ppf_point(tgt, tnrm, i, q.flip != 0, true), b = ppf_point(tgt, tnrm, j, q.flip != 0, false);
        int k; float al;
        if (a.ok && b.ok && ppf_pair(a, b, q, &k, &al)) key = k;
    }
    keys[p] = (unsigned long long)key;
    vals[p] = p;
}

// offsets[k] = the number of sorted keys below k, k = 0 .. n_keys
__global__ __launch_bounds__(256) void k_ppf_offsets(const unsigned long long* __restrict__ skeys, unsigned n, int n_keys, int* __restrict__ offsets) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > n_keys) return;
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (skeys[mid] < (unsigned long long)k) lo = mid + 1; else hi = mid;
    }
    offsets[k] = (int)lo;
}

// the keyed entries of the sorted list (they come first): pair, alpha bits.  cap = nt * (nt - 1) >= their number.
__global__ __launch_bounds__(256) void k_ppf_model_fill(const float* __restrict__ tgt, const float* __restrict__ tnrm, int nt,
                                                        const PpfState* __restrict__ st, PpfQuant q, const unsigned long long* __restrict__ skeys,
                                                        const unsigned* __restrict__ svals, unsigned n, unsigned cap, unsigned* __restrict__ pair,
                                                        unsigned* __restrict__ alpha) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n || t >= cap) return;
    const unsigned long long key = skeys[t];
    if (key >= (unsigned long long)q.n_keys) return;
    q.step = st->step;
    const unsigned p = svals[t];
    const int i = (int)(p / (unsigned)nt), j = (int)(p - (unsigned)i * (unsigned)nt);
    const PpfPoint a = ppf_point(tgt, tnrm, i, q.flip != 0, true), b = ppf_point(tgt, tnrm, j, q.flip != 0, false);
    int k = 0; float al = 0.f;
    ppf_pair(a, b, q, &k, &al);
    pair[t] = p; alpha[t] = __float_as_uint(al);
}

// What the host's pose stage needs of a peak: the scene point and the model point (normal as voted with: flipped where asked for)
struct PpfPeakPoints { float ps[3], ns[3], pm[3], nm[3]; };

// The clouds of a voting launch.  A batch: instance b is rows [src_off[b], src_off[b + 1]) of src and nrm and owns the work items
// [ref_off[b], ref_off[b + 1]) (device arrays of n_inst + 1 ints).  ref_off == nullptr: one cloud of ns rows, item = reference point.
struct PpfClouds { const float* src; const float* nrm; int ns; const int* src_off; const int* ref_off; int n_inst; };

// rules 5 and 6 for work items blockIdx.x, + gridDim.x, ...  CELLS > 0: the counters are LDS (nt * R <= CELLS); CELLS == 0: slabs +
// blockIdx.x * nt * R.  peaks[item] and pts[item]; a peak's ref counts inside its instance.
template <int CELLS>
__global__ __launch_bounds__(PPF_THREADS)
void k_ppf_vote(PpfClouds cl, const float* __restrict__ tgt, const float* __restrict__ tnrm,
                int nt, const int* __restrict__ offsets, const unsigned* __restrict__ pair, const unsigned* __restrict__ alpha, PpfQuant q,
                int ref_stride, int n_items, unsigned* __restrict__ slabs, tdv_ppf_peak* __restrict__ peaks, PpfPeakPoints* __restrict__ pts) {
    __shared__ unsigned lds_acc[CELLS > 0 ? CELLS : 1];
    __shared__ unsigned s_start[PPF_THREADS], s_pref[PPF_THREADS];
    __shared__ float s_alpha[PPF_THREADS];
    __shared__ unsigned s_wave[PPF_WAVES];
    __shared__ unsigned long long s_best[PPF_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cells = nt * q.R;
    unsigned* acc = CELLS > 0 ? lds_acc : slabs + (size_t)blockIdx.x * (size_t)cells;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const float* __restrict__ src = cl.src; const float* __restrict__ snrm = cl.nrm;
        int ns = cl.ns, r = item;
        if (cl.ref_off) {                                            // the last instance b with ref_off[b] <= item: the one that has it
            int lo = 0, hi = cl.n_inst;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (cl.ref_off[mid] <= item) lo = mid; else hi = mid;
            }
            const int row = cl.src_off[lo];
            r = item - cl.ref_off[lo]; ns = cl.src_off[lo + 1] - row;
            src += 3 * (size_t)row; snrm += 3 * (size_t)row;
        }
        const int sr = r * ref_stride;
        const PpfPoint a = ppf_point(src, snrm, sr, false, true);    // workgroup-uniform
        unsigned long long best = 0;
        if (a.ok) {
            for (int c = tid; c < cells; c += PPF_THREADS) {
                if (CELLS > 0) acc[c] = 0u;
                else __hip_atomic_store(&acc[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (CELLS == 0) __threadfence();
            __syncthreads();
            for (int base = 0; base < ns; base += PPF_THREADS) {
                const int i = base + tid;
                unsigned start = 0, cnt = 0;
                float as = 0.f;
                if (i < ns && i != sr) {
                    const PpfPoint b = ppf_point(src, snrm, i, false, false);
                    int key;
                    if (b.ok && ppf_pair(a, b, q, &key, &as)) {
                        start = (unsigned)offsets[key];
                        cnt = (unsigned)offsets[key + 1] - start;
                    }
                }
                // exclusive scan of cnt over the workgroup
                unsigned incl = cnt;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned v = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += v;
                }
                if (lane == 63) s_wave[wave] = incl;
                s_start[tid] = start; s_alpha[tid] = as;
                __syncthreads();
                unsigned before = 0, total = 0;
#pragma unroll
                for (int k = 0; k < PPF_WAVES; ++k) { if (k < wave) before += s_wave[k]; total += s_wave[k]; }
                s_pref[tid] = before + (incl - cnt);
                __syncthreads();
                for (unsigned e = tid; e < total; e += PPF_THREADS) {
                    int lo = 0, hi = PPF_THREADS;                     // the last t with s_pref[t] <= e: its bucket is not empty
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_pref[mid] <= e) lo = mid; else hi = mid;
                    }
                    const unsigned idx = s_start[lo] + (e - s_pref[lo]);
                    const unsigned im = pair[idx] / (unsigned)nt;
                    const int bin = ppf_bin(__uint_as_float(alpha[idx]), s_alpha[lo], q);
                    atomicAdd(&acc[im * (unsigned)q.R + (unsigned)bin], 1u);
                }
                __syncthreads();                                     // the staging is free again
            }
            if (CELLS == 0) { __threadfence(); __syncthreads(); }
            for (int c = tid; c < cells; c += PPF_THREADS) {
                const unsigned v = CELLS > 0 ? acc[c] : __hip_atomic_load(&acc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v) best = max(best, ((unsigned long long)v << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c));
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off, 64));
            if (lane == 0) s_best[wave] = best;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PPF_WAVES; ++k) best = max(best, s_best[k]);
            __syncthreads();                                         // s_best and the counters are free again
        }
        if (tid == 0) {
            tdv_ppf_peak pk{sr, 0, 0, 0};
            PpfPeakPoints pp{};
            if (best) {
                const unsigned c = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu);
                pk.votes = (int)(best >> 32); pk.model_index = (int)(c / (unsigned)q.R); pk.bin = (int)(c - (unsigned)pk.model_index * (unsigned)q.R);
                const PpfPoint m = ppf_point(tgt, tnrm, pk.model_index, q.flip != 0, false);
                pp.ps[0] = a.px; pp.ps[1] = a.py; pp.ps[2] = a.pz; pp.ns[0] = a.nx; pp.ns[1] = a.ny; pp.ns[2] = a.nz;
                pp.pm[0] = m.px; pp.pm[1] = m.py; pp.pm[2] = m.pz; pp.nm[0] = m.nx; pp.nm[1] = m.ny; pp.nm[2] = m.nz;
            }
            peaks[item] = pk; pts[item] = pp;
        }
    }
}

// A returned pose of a batch: T (column-major), its instance, and where its rows start in d2 / accepted
struct PpfSlot { float T[16]; int inst, pad; unsigned long long out; };
constexpr int PPF_SCORE_THREADS = 256;
static_assert(TDV_PPF_MODEL_MAX % 4 == 0, "the staged model is padded to fours");

// rule 7's score pass for every pose slot of a batch: workgroup (x = slot, y) takes the slot's source points y * 256 + lane, + gridDim.y
// * 256, ...; the model sits in LDS (lds_scan.hpp).  d2[out + i] is the nearest model point's squared distance (FLT_MAX: none) and
// accepted[out + i] = d2 <= tau: per accepted row the bits of tdv_icp_correspondences at (T, thr), whichever search that call runs.
__global__ __launch_bounds__(PPF_SCORE_THREADS)
void k_ppf_score(const float* __restrict__ src0, const int* __restrict__ src_off, const float* __restrict__ tgt, int nt,
                 const PpfSlot* __restrict__ slots, float tau, float* __restrict__ d2, uint8_t* __restrict__ accepted) {
    __shared__ __attribute__((aligned(16))) float tx[TDV_PPF_MODEL_MAX], ty[TDV_PPF_MODEL_MAX], tz[TDV_PPF_MODEL_MAX];
    const PpfSlot* __restrict__ sl = slots + blockIdx.x;
    const int row = src_off[sl->inst], ns = src_off[sl->inst + 1] - row;
    if ((long long)blockIdx.y * PPF_SCORE_THREADS >= (long long)ns) return;       // workgroup-uniform
    lds_stage_targets(tgt, nt, tx, ty, tz, PPF_SCORE_THREADS);
    __syncthreads();
    float T[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = sl->T[k];
    const float* __restrict__ src = src0 + 3 * (size_t)row;
    const size_t out = (size_t)sl->out;
    const int nt4 = (nt + 3) / 4;
    for (long long i = (long long)blockIdx.y * PPF_SCORE_THREADS + threadIdx.x; i < (long long)ns; i += (long long)gridDim.y * PPF_SCORE_THREADS) {
        float px, py, pz, best; int idx;
        transform_point(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], px, py, pz);
        lds_nearest(px, py, pz, tx, ty, tz, nt4, best, idx);
        d2[out + (size_t)i] = best; accepted[out + (size_t)i] = best <= tau ? 1 : 0;
    }
}

// ---- rule 7 on the host, f64
struct Pose64 { double R[3][3], t[3]; };

void ppf_frame64(const float* n, double R[3][3]) {
    const double nx = n[0], ny = n[1], nz = n[2];
    const double norm = std::sqrt((nx * nx + ny * ny) + nz * nz);
    const bool neg = nx < 0.0;
    const double ux = nx / norm, uy = ny / norm, uz = nz / norm;
    const double wx = neg ? -ux : ux, wy = neg ? -uy : uy, wz = neg ? -uz : uz;
    const double k = 1.0 + wx, ca = wy / k, cb = wz / k;
    R[0][0] = wx; R[0][1] = wy; R[0][2] = wz;
    R[1][0] = -wy; R[1][1] = 1.0 - wy * ca; R[1][2] = -wy * cb;
    R[2][0] = -wz; R[2][1] = -wz * ca; R[2][2] = 1.0 - wz * cb;
    if (neg)
        for (int j = 0; j < 3; ++j) { R[0][j] = -R[0][j]; R[2][j] = -R[2][j]; }
}

Pose64 ppf_pose64(const PpfPeakPoints& pp, int bin, int rotation_bins) {
    const double pi = 3.141592653589793;
    const float alpha_c = (float)(-pi + ((double)bin + 0.5) * ((2.0 * pi) / (double)rotation_bins));
    const double c = std::cos((double)alpha_c), sn = std::sin((double)alpha_c);
    double Rs[3][3], Rm[3][3], M[3][3];
    ppf_frame64(pp.ns, Rs);
    ppf_frame64(pp.nm, Rm);
    for (int j = 0; j < 3; ++j) { M[0][j] = Rs[0][j]; M[1][j] = c * Rs[1][j] + sn * Rs[2][j]; M[2][j] = c * Rs[2][j] - sn * Rs[1][j]; }
    Pose64 P;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) P.R[i][j] = (Rm[0][i] * M[0][j] + Rm[1][i] * M[1][j]) + Rm[2][i] * M[2][j];
    for (int i = 0; i < 3; ++i) P.t[i] = (double)pp.pm[i] - ((P.R[i][0] * (double)pp.ps[0] + P.R[i][1] * (double)pp.ps[1]) + P.R[i][2] * (double)pp.ps[2]);
    return P;
}

bool ppf_within(const Pose64& a, const Pose64& b, double max_t, double min_c) {
    const double dx = a.t[0] - b.t[0], dy = a.t[1] - b.t[1], dz = a.t[2] - b.t[2];
    if (!(std::sqrt((dx * dx + dy * dy) + dz * dz) <= max_t)) return false;
    double tr = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) tr += a.R[i][j] * b.R[i][j];
    return (tr - 1.0) / 2.0 >= min_c;
}

struct PpfCluster { int founder; long long votes; int members; };

// what the parameters alone fix (ppf_plan): n_dist, n_keys and the table's layout for nt points
struct PpfPlan { int n_dist, n_keys; size_t off_words, cap, bytes; };

PpfQuant ppf_quant(const tdv_ppf_params& prm, const PpfPlan& plan, float step) {
    PpfQuant q;
    q.step = step; q.astep = PPF_PI / (float)prm.angle_bins; q.rstep = PPF_TWO_PI / (float)prm.rotation_bins;
    q.A = prm.angle_bins; q.R = prm.rotation_bins; q.n_dist = plan.n_dist; q.n_keys = plan.n_keys; q.flip = prm.flip_model_normals;
    return q;
}

// the table, as the kernels take it
struct PpfTable { const int* offsets; const unsigned* pair; const unsigned* alpha; };
PpfTable ppf_table(const void* d_model, const PpfPlan& plan) {
    PpfTable t;
    t.offsets = static_cast<const int*>(d_model);
    t.pair = reinterpret_cast<const unsigned*>(t.offsets) + plan.off_words;
    t.alpha = t.pair + plan.cap;
    return t;
}

// the voting launch over n_items work items (a single cloud or a batch: PpfClouds): the counter variant and its grid cap (rule 5)
int ppf_vote_launch(tdv_ctx* ctx, const PpfClouds& cl, int n_items, const float* d_tgt, const float* d_tgt_normals, int nt, const PpfTable& tb,
                    const PpfQuant& q, int ref_stride, tdv_ppf_peak* peaks, PpfPeakPoints* pts) {
    hipStream_t s = ctx->stream;
    const int cells = nt * q.R;
    if (cells <= PPF_LDS_SMALL) {
        k_ppf_vote<PPF_LDS_SMALL><<<std::min(n_items, PPF_GRID_LDS), PPF_THREADS, 0, s>>>(cl, d_tgt, d_tgt_normals, nt, tb.offsets, tb.pair, tb.alpha, q,
                                                                                         ref_stride, n_items, nullptr, peaks, pts);
    } else if (cells <= TDV_PPF_LDS_CELLS) {
        k_ppf_vote<TDV_PPF_LDS_CELLS><<<std::min(n_items, PPF_GRID_LDS), PPF_THREADS, 0, s>>>(cl, d_tgt, d_tgt_normals, nt, tb.offsets, tb.pair, tb.alpha,
                                                                                             q, ref_stride, n_items, nullptr, peaks, pts);
    } else {
        const int grid = std::max(1, std::min(std::min(n_items, PPF_GRID_SLAB), (int)(PPF_SLAB_BYTES / ((size_t)cells * 4))));
        unsigned* slabs;
        TDV_TRY(ws_alloc(ctx, (size_t)grid * (size_t)cells, &slabs));
        k_ppf_vote<0><<<grid, PPF_THREADS, 0, s>>>(cl, d_tgt, d_tgt_normals, nt, tb.offsets, tb.pair, tb.alpha, q, ref_stride, n_items, slabs, peaks, pts);
    }
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// rule 7 up to the score: the returned poses of one cloud's n_ref peaks, ranked, with T, votes, members and the founder's peak
std::vector<tdv_ppf_pose> ppf_rank(const tdv_ppf_peak* pk, const PpfPeakPoints* pp, int n_ref, const tdv_ppf_params& prm, const tdv_ppf_model_info& info) {
    std::vector<int> order;
    for (int r = 0; r < n_ref; ++r) if (pk[r].votes > 0) order.push_back(r);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pk[a].votes > pk[b].votes; });     // stable: ref ascending among equals
    std::vector<Pose64> pose((size_t)n_ref);
    for (int r : order) pose[r] = ppf_pose64(pp[r], pk[r].bin, prm.rotation_bins);
    const double max_t = (double)prm.cluster_translation_relative * (double)info.diameter, min_c = std::cos((double)prm.cluster_rotation);
    std::vector<PpfCluster> cl;
    for (int r : order) {
        size_t c = 0;
        while (c < cl.size() && !ppf_within(pose[r], pose[cl[c].founder], max_t, min_c)) ++c;
        if (c == cl.size()) cl.push_back({r, 0, 0});
        cl[c].votes += pk[r].votes; cl[c].members += 1;
    }
    std::vector<int> top(cl.size());
    for (size_t c = 0; c < cl.size(); ++c) top[c] = (int)c;
    std::stable_sort(top.begin(), top.end(), [&](int a, int b) { return cl[a].votes > cl[b].votes; });
    std::vector<tdv_ppf_pose> out(std::min(top.size(), (size_t)prm.max_poses));
    for (size_t k = 0; k < out.size(); ++k) {
        const PpfCluster& c = cl[top[k]];
        const Pose64& P = pose[c.founder];
        tdv_ppf_pose o{};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) o.T[4 * j + i] = (float)P.R[i][j];
            o.T[12 + i] = (float)P.t[i];
        }
        o.T[15] = 1.f;
        o.votes = (int)std::min(c.votes, (long long)INT_MAX); o.members = c.members;
        o.ref = pk[c.founder].ref; o.model_index = pk[c.founder].model_index; o.bin = pk[c.founder].bin;
        out[k] = o;
    }
    return out;
}

// rule 7's score of a pose from its correspondence pass read back (d2: ns floats, unaligned; accepted: ns bytes) and the pass's count
void ppf_score(tdv_ppf_pose* o, const char* d2, const uint8_t* accepted, int ns, int n_corr) {
    double S = 0.0;
    for (int i = 0; i < ns; ++i) {
        float v;
        std::memcpy(&v, d2 + (size_t)i * 4, 4);
        if (accepted[i]) S += (double)v;
    }
    o->n_corr = n_corr;
    o->fitness = (float)n_corr / (float)ns;
    o->rmse = n_corr > 0 ? (float)std::sqrt(S / (double)n_corr) : 0.f;
}

// every parameter (include/tdv_hip.h), and what they fix: the parameter check of every entry point
bool ppf_plan(const tdv_ppf_params* p, int nt, PpfPlan* plan) {
    if (!p || nt < 0 || nt > TDV_PPF_MODEL_MAX) return false;
    if (!(p->distance_step_relative > 0.f) || !(p->distance_step_relative <= 1.f)) return false;
    if (p->angle_bins < 1 || p->angle_bins > 64 || p->rotation_bins < 1 || p->rotation_bins > 256) return false;
    if (p->ref_stride < 1 || p->max_poses < 1 || p->max_poses > TDV_PPF_POSES_MAX) return false;
    if (!std::isfinite(p->cluster_translation_relative) || p->cluster_translation_relative < 0.f) return false;
    if (!(p->cluster_rotation >= 0.f) || !(p->cluster_rotation <= PPF_PI)) return false;
    if (p->flip_model_normals != 0 && p->flip_model_normals != 1) return false;
    const float inv = floorf(1.0f / p->distance_step_relative);
    if (!(inv <= (float)TDV_PPF_KEYS_MAX)) return false;
    const long long n_dist = (long long)inv + 1, n_keys = n_dist * p->angle_bins * p->angle_bins * p->angle_bins;
    if (n_keys > TDV_PPF_KEYS_MAX) return false;
    plan->n_dist = (int)n_dist; plan->n_keys = (int)n_keys;
    plan->off_words = align_up((size_t)n_keys + 1, 4);
    plan->cap = nt >= 2 ? (size_t)nt * (size_t)(nt - 1) : 0;
    plan->bytes = 4 * (plan->off_words + 2 * plan->cap);
    return true;
}

int ppf_model_run(tdv_ctx* ctx, const float* d_tgt, const float* d_tgt_normals, int nt, const tdv_ppf_params& prm, const PpfPlan& plan,
                  void* d_model, tdv_ppf_model_info* info) {
    hipStream_t s = ctx->stream;
    int* offsets = static_cast<int*>(d_model);
    tdv_ppf_model_info out{0.f, 0.f, 0, plan.n_keys, nt};
    if (nt < 2) {                                                    // no pair: an empty table (the diameter of one point is 0)
        TDV_HIP(ctx, hipMemsetAsync(offsets, 0, ((size_t)plan.n_keys + 1) * 4, s));
        TDV_HIP(ctx, hipStreamSynchronize(s));
        *info = out;
        return TDV_OK;
    }
    unsigned* pair = reinterpret_cast<unsigned*>(offsets) + plan.off_words;
    unsigned* alpha = pair + plan.cap;
    const size_t n = (size_t)nt * (size_t)nt;
    PpfState* st;
    unsigned long long *keys, *skeys; unsigned *vals, *svals;
    TDV_TRY(ws_alloc(ctx, 1, &st));
    TDV_TRY(ws_alloc(ctx, n, &keys));
    TDV_TRY(ws_alloc(ctx, n, &skeys));
    TDV_TRY(ws_alloc(ctx, n, &vals));
    TDV_TRY(ws_alloc(ctx, n, &svals));
    TDV_TRY(pin_reserve(ctx, 64));
    const PpfQuant q = ppf_quant(prm, plan, 0.f);
    const unsigned nb = (unsigned)((n + 255) / 256);
    k_ppf_diameter<<<1, 256, 0, s>>>(d_tgt, nt, prm.distance_step_relative, st);
    k_ppf_model_keys<<<nb, 256, 0, s>>>(d_tgt, d_tgt_normals, nt, st, q, keys, vals);
    TDV_CHECK_LAUNCH(ctx);
    int end_bit = 1;
    while (((long long)1 << end_bit) <= (long long)plan.n_keys) ++end_bit;       // the sentinel n_keys itself is a key value
    TDV_TRY(radix_sort_pairs_dev(ctx, keys, skeys, vals, svals, n, end_bit));
    k_ppf_offsets<<<(plan.n_keys + 1 + 255) / 256, 256, 0, s>>>(skeys, (unsigned)n, plan.n_keys, offsets);
    k_ppf_model_fill<<<nb, 256, 0, s>>>(d_tgt, d_tgt_normals, nt, st, q, skeys, svals, (unsigned)n, (unsigned)plan.cap, pair, alpha);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, st, sizeof(PpfState), hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin + 16, offsets + plan.n_keys, 4, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    PpfState hs;
    std::memcpy(&hs, ctx->pin, sizeof(hs));
    std::memcpy(&out.n_pairs, ctx->pin + 16, 4);
    out.diameter = hs.diameter; out.distance_step = hs.step;
    *info = out;
    return TDV_OK;
}

int ppf_match_run(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                  const void* d_model, const tdv_ppf_model_info& info, float thr, const tdv_ppf_params& prm, const PpfPlan& plan,
                  tdv_ppf_pose* out_poses, int* n_poses, tdv_ppf_peak* d_peaks, tdv_ppf_peak* h_peaks, int* n_ref_out) {
    *n_poses = 0;
    if (n_ref_out) *n_ref_out = 0;
    if (ns == 0 || nt < 2 || info.n_pairs == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    const int n_ref = (ns + prm.ref_stride - 1) / prm.ref_stride;
    const size_t peak_bytes = (size_t)n_ref * sizeof(tdv_ppf_peak), pts_bytes = (size_t)n_ref * sizeof(PpfPeakPoints);
    tdv_ppf_peak* peaks = d_peaks;
    PpfPeakPoints* pts;
    if (!peaks) TDV_TRY(ws_alloc(ctx, (size_t)n_ref, &peaks));
    TDV_TRY(ws_alloc(ctx, (size_t)n_ref, &pts));
    TDV_TRY(pin_reserve(ctx, std::max(peak_bytes + pts_bytes, (size_t)ns * 5 + 64)));
    const PpfClouds one{d_src, d_src_normals, ns, nullptr, nullptr, 1};          // the batch of one
    TDV_TRY(ppf_vote_launch(ctx, one, n_ref, d_tgt, d_tgt_normals, nt, ppf_table(d_model, plan), ppf_quant(prm, plan, info.distance_step),
                            prm.ref_stride, peaks, pts));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, peaks, peak_bytes, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin + peak_bytes, pts, pts_bytes, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    std::vector<tdv_ppf_peak> pk((size_t)n_ref);
    std::vector<PpfPeakPoints> pp((size_t)n_ref);
    std::memcpy(pk.data(), ctx->pin, peak_bytes);
    std::memcpy(pp.data(), ctx->pin + peak_bytes, pts_bytes);
    if (h_peaks) std::memcpy(h_peaks, pk.data(), peak_bytes);
    if (n_ref_out) *n_ref_out = n_ref;
    std::vector<tdv_ppf_pose> poses = ppf_rank(pk.data(), pp.data(), n_ref, prm, info);

    // score: tdv_icp_correspondences at each returned pose
    const WsMark mark = ws_mark(ctx);
    for (size_t k = 0; k < poses.size(); ++k) {
        tdv_ppf_pose& o = poses[k];
        ws_rewind(ctx, mark);
        IcpOutputs io;
        TDV_TRY(ws_alloc(ctx, (size_t)ns, &io.d2));
        TDV_TRY(ws_alloc(ctx, align_up((size_t)ns, 16), &io.accepted));
        int n_corr = 0;
        TDV_TRY(icp_correspondences_dev(ctx, d_src, ns, d_tgt, nt, o.T, thr, io, &n_corr));
        char* h = ctx->pin;                                          // (the pass is done with the staging: it has read its state back)
        TDV_HIP(ctx, hipMemcpyAsync(h, io.d2, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
        TDV_HIP(ctx, hipMemcpyAsync(h + (size_t)ns * 4, io.accepted, (size_t)ns, hipMemcpyDeviceToHost, s));
        TDV_HIP(ctx, hipStreamSynchronize(s));
        ppf_score(&o, h, reinterpret_cast<const uint8_t*>(h + (size_t)ns * 4), ns, n_corr);
        out_poses[k] = o;
    }
    *n_poses = (int)poses.size();
    return TDV_OK;
}

// Per instance, ppf_match_run: one voting launch over every instance's reference points, one read-back of all peaks, ppf_rank per instance,
// one scoring launch over every returned pose, one read-back of their d2 / accepted rows.  h_ref_off[b]: the instances' reference offsets
// (the entry point formed and checked them); out_poses, n_poses and h_peak_off as include/tdv_hip.h has them.
int ppf_match_batch_run(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_off, const int* h_ref_off, int n_inst,
                        const float* d_tgt, const float* d_tgt_normals, int nt, const void* d_model, const tdv_ppf_model_info& info, float thr,
                        const tdv_ppf_params& prm, const PpfPlan& plan, tdv_ppf_pose* out_poses, int* n_poses, tdv_ppf_peak* d_peaks,
                        int* h_peak_off) {
    for (int b = 0; b < n_inst; ++b) n_poses[b] = 0;
    if (h_peak_off) for (int b = 0; b <= n_inst; ++b) h_peak_off[b] = 0;
    const int n_items = n_inst > 0 ? h_ref_off[n_inst] : 0;
    if (n_items == 0 || nt < 2 || info.n_pairs == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    const size_t n_off = (size_t)n_inst + 1;
    const size_t off_bytes = align_up(2 * n_off * sizeof(int), 64);
    const size_t peak_bytes = (size_t)n_items * sizeof(tdv_ppf_peak), pts_bytes = (size_t)n_items * sizeof(PpfPeakPoints);
    int* d_off;                                                      // src_off[n_off], then ref_off[n_off]
    tdv_ppf_peak* peaks = d_peaks;
    PpfPeakPoints* pts;
    TDV_TRY(ws_alloc(ctx, 2 * n_off, &d_off));
    if (!peaks) TDV_TRY(ws_alloc(ctx, (size_t)n_items, &peaks));
    TDV_TRY(ws_alloc(ctx, (size_t)n_items, &pts));
    TDV_TRY(pin_reserve(ctx, off_bytes + peak_bytes + pts_bytes));
    std::memcpy(ctx->pin, h_src_off, n_off * sizeof(int));
    std::memcpy(ctx->pin + n_off * sizeof(int), h_ref_off, n_off * sizeof(int));
    TDV_HIP(ctx, hipMemcpyAsync(d_off, ctx->pin, 2 * n_off * sizeof(int), hipMemcpyHostToDevice, s));
    const PpfClouds cl{d_src, d_src_normals, 0, d_off, d_off + n_off, n_inst};
    TDV_TRY(ppf_vote_launch(ctx, cl, n_items, d_tgt, d_tgt_normals, nt, ppf_table(d_model, plan), ppf_quant(prm, plan, info.distance_step),
                            prm.ref_stride, peaks, pts));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin + off_bytes, peaks, peak_bytes, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin + off_bytes + peak_bytes, pts, pts_bytes, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));                           // read-back 1 of 2
    std::vector<tdv_ppf_peak> pk((size_t)n_items);
    std::vector<PpfPeakPoints> pp((size_t)n_items);
    std::memcpy(pk.data(), ctx->pin + off_bytes, peak_bytes);
    std::memcpy(pp.data(), ctx->pin + off_bytes + peak_bytes, pts_bytes);

    // rule 7 per instance; a slot per returned pose, its rows of d2 / accepted one after the other
    std::vector<tdv_ppf_pose> poses;
    std::vector<PpfSlot> slots;
    size_t rows = 0;
    int ns_max = 0;
    for (int b = 0; b < n_inst; ++b) {
        const int r0 = h_ref_off[b], n_ref = h_ref_off[b + 1] - r0, ns = h_src_off[b + 1] - h_src_off[b];
        const std::vector<tdv_ppf_pose> got = ppf_rank(pk.data() + r0, pp.data() + r0, n_ref, prm, info);
        n_poses[b] = (int)got.size();
        for (const tdv_ppf_pose& o : got) {
            PpfSlot sl{};
            std::memcpy(sl.T, o.T, sizeof(sl.T));
            sl.inst = b; sl.out = rows;
            rows += (size_t)ns;
            slots.push_back(sl); poses.push_back(o);
        }
        if (!got.empty()) ns_max = std::max(ns_max, ns);
    }
    if (!slots.empty()) {
        const size_t slot_bytes = align_up(slots.size() * sizeof(PpfSlot), 64);
        PpfSlot* d_slots; float* d_d2; uint8_t* d_acc;
        TDV_TRY(ws_alloc(ctx, slots.size(), &d_slots));
        TDV_TRY(ws_alloc(ctx, rows, &d_d2));
        TDV_TRY(ws_alloc(ctx, rows, &d_acc));
        TDV_TRY(pin_reserve(ctx, slot_bytes + rows * 5));            // (the stream is idle: the staging may move)
        std::memcpy(ctx->pin, slots.data(), slots.size() * sizeof(PpfSlot));
        TDV_HIP(ctx, hipMemcpyAsync(d_slots, ctx->pin, slots.size() * sizeof(PpfSlot), hipMemcpyHostToDevice, s));
        const unsigned gy = (unsigned)std::min<long long>(((long long)ns_max + PPF_SCORE_THREADS - 1) / PPF_SCORE_THREADS, 65535);
        k_ppf_score<<<dim3((unsigned)slots.size(), gy), PPF_SCORE_THREADS, 0, s>>>(d_src, d_off, d_tgt, nt, d_slots, tau_le(thr), d_d2, d_acc);
        TDV_CHECK_LAUNCH(ctx);
        char* h_d2 = ctx->pin + slot_bytes;
        const uint8_t* h_acc = reinterpret_cast<const uint8_t*>(h_d2 + rows * 4);
        TDV_HIP(ctx, hipMemcpyAsync(h_d2, d_d2, rows * 4, hipMemcpyDeviceToHost, s));
        TDV_HIP(ctx, hipMemcpyAsync(h_d2 + rows * 4, d_acc, rows, hipMemcpyDeviceToHost, s));
        TDV_HIP(ctx, hipStreamSynchronize(s));                       // read-back 2 of 2
        ctx->last_icp_search = TDV_ICP_SEARCH_BRUTE;
        for (size_t k = 0; k < slots.size(); ++k) {
            const int ns = h_src_off[slots[k].inst + 1] - h_src_off[slots[k].inst];
            const uint8_t* acc = h_acc + slots[k].out;
            int n_corr = 0;
            for (int i = 0; i < ns; ++i) n_corr += acc[i] ? 1 : 0;
            ppf_score(&poses[k], h_d2 + slots[k].out * 4, acc, ns, n_corr);
        }
    }
    size_t k = 0;
    for (int b = 0; b < n_inst; ++b)
        for (int j = 0; j < n_poses[b]; ++j) out_poses[(size_t)b * (size_t)prm.max_poses + (size_t)j] = poses[k++];
    if (h_peak_off) std::memcpy(h_peak_off, h_ref_off, n_off * sizeof(int));
    return TDV_OK;
}

// every argument of a match, before anything is enqueued (include/tdv_hip.h: tdv_ppf_match)
bool ppf_match_args_ok(const tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt,
                       float thr, const tdv_ppf_params* params, const tdv_ppf_pose* out_poses, const int* n_poses, PpfPlan* plan) {
    if (!ctx || !out_poses || !n_poses || ns < 0 || !ppf_plan(params, nt, plan)) return false;
    if (ns > 0 && (!src || !src_normals)) return false;
    if (nt > 0 && (!tgt || !tgt_normals)) return false;
    return std::isfinite(thr) && thr > 0.f;
}
bool ppf_model_ptr_ok(const void* d_model) { return d_model && (reinterpret_cast<uintptr_t>(d_model) & 3) == 0; }
// ... and the table with its info (tdv_ppf_match_dev, tdv_ppf_match_batch_dev)
bool ppf_model_info_ok(const void* d_model, const tdv_ppf_model_info* info, int nt, const PpfPlan& plan) {
    return info && ppf_model_ptr_ok(d_model) && info->nt == nt && info->n_keys == plan.n_keys && info->n_pairs >= 0 &&
           (size_t)info->n_pairs <= plan.cap && std::isfinite(info->diameter) && info->diameter >= 0.f && std::isfinite(info->distance_step) &&
           info->distance_step >= 0.f;
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_ppf_default_params(tdv_ppf_params* p) {
    if (!p) return;
    p->distance_step_relative = 0.05f; p->angle_bins = 30; p->rotation_bins = 30; p->ref_stride = 5; p->max_poses = 8;
    p->cluster_translation_relative = 0.1f; p->cluster_rotation = (float)(2.0 * 3.141592653589793 / 30.0); p->flip_model_normals = 0;
}

int tdv_ppf_model_bytes(int nt, const tdv_ppf_params* params, size_t* bytes) {
    PpfPlan plan;
    if (!bytes || !ppf_plan(params, nt, &plan)) return TDV_ERR_BAD_ARG;
    *bytes = plan.bytes;
    return TDV_OK;
}

int tdv_ppf_model_dev(tdv_ctx* ctx, const float* d_tgt, const float* d_tgt_normals, int nt, const tdv_ppf_params* params, void* d_model,
                      size_t model_bytes, tdv_ppf_model_info* info) {
    PpfPlan plan;
    if (!ctx || !info || !ppf_plan(params, nt, &plan) || (nt > 0 && (!d_tgt || !d_tgt_normals)) || !ppf_model_ptr_ok(d_model) ||
        model_bytes < plan.bytes)
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return ppf_model_run(ctx, d_tgt, d_tgt_normals, nt, *params, plan, d_model, info);
}

int tdv_ppf_match_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                      const void* d_model, const tdv_ppf_model_info* info, float thr, const tdv_ppf_params* params, tdv_ppf_pose* out_poses,
                      int* n_poses, tdv_ppf_peak* d_peaks, int* n_ref) {
    PpfPlan plan;
    if (!ppf_match_args_ok(ctx, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, thr, params, out_poses, n_poses, &plan)) return TDV_ERR_BAD_ARG;
    if (!ppf_model_info_ok(d_model, info, nt, plan)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return ppf_match_run(ctx, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, d_model, *info, thr, *params, plan, out_poses, n_poses, d_peaks,
                         nullptr, n_ref);
}

int tdv_ppf_match_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_offsets, int n_instances, const float* d_tgt,
                            const float* d_tgt_normals, int nt, const void* d_model, const tdv_ppf_model_info* info, float thr,
                            const tdv_ppf_params* params, tdv_ppf_pose* out_poses, int* n_poses, tdv_ppf_peak* d_peaks, int* h_peak_offsets) {
    PpfPlan plan;
    if (n_instances < 0 || (n_instances > 0 && !h_src_offsets)) return TDV_ERR_BAD_ARG;
    if (n_instances > 0 && h_src_offsets[0] != 0) return TDV_ERR_BAD_ARG;
    for (int b = 0; b < n_instances; ++b)
        if (h_src_offsets[b + 1] < h_src_offsets[b]) return TDV_ERR_BAD_ARG;
    const int ns = n_instances > 0 ? h_src_offsets[n_instances] : 0;
    if (!ppf_match_args_ok(ctx, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, thr, params, out_poses, n_poses, &plan)) return TDV_ERR_BAD_ARG;
    if (!ppf_model_info_ok(d_model, info, nt, plan)) return TDV_ERR_BAD_ARG;
    if ((long long)n_instances * params->max_poses > INT_MAX) return TDV_ERR_BAD_ARG;
    std::vector<int> ref_off((size_t)n_instances + 1, 0);            // rule 5's n_ref per instance, summed
    long long sum = 0;
    for (int b = 0; b < n_instances; ++b) {
        const long long n = h_src_offsets[b + 1] - h_src_offsets[b];
        sum += (n + params->ref_stride - 1) / params->ref_stride;
        if (sum > INT_MAX) return TDV_ERR_BAD_ARG;
        ref_off[(size_t)b + 1] = (int)sum;
    }
    TDV_TRY(call_begin(ctx));
    return ppf_match_batch_run(ctx, d_src, d_src_normals, h_src_offsets, ref_off.data(), n_instances, d_tgt, d_tgt_normals, nt, d_model, *info, thr,
                               *params, plan, out_poses, n_poses, d_peaks, h_peak_offsets);
}

int tdv_ppf_match(tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt, float thr,
                  const tdv_ppf_params* params, tdv_ppf_pose* out_poses, int* n_poses, tdv_ppf_peak* peaks, int* n_ref) {
    PpfPlan plan;
    if (!ppf_match_args_ok(ctx, src, src_normals, ns, tgt, tgt_normals, nt, thr, params, out_poses, n_poses, &plan)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float *d_src, *d_sn, *d_tgt, *d_tn;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, src_normals, (size_t)ns * 3, &d_sn));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    TDV_TRY(upload(ctx, tgt_normals, (size_t)nt * 3, &d_tn));
    void* d_model;
    TDV_TRY(ws_alloc_bytes(ctx, plan.bytes, &d_model));
    tdv_ppf_model_info info;
    TDV_TRY(ppf_model_run(ctx, d_tgt, d_tn, nt, *params, plan, d_model, &info));
    return ppf_match_run(ctx, d_src, d_sn, ns, d_tgt, d_tn, nt, d_model, info, thr, *params, plan, out_poses, n_poses, nullptr, peaks, n_ref);
}

}  // extern "C"
