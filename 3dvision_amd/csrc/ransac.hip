// RANSAC coarse alignment on gfx950.
//
// Replaces Registration::ransacRegistration (/root/reference/src/registration.cpp:204-295), which
// has no GPU entry point in the reference (src/pipeline.cpp:97-102 calls the CPU static directly).
// Sub-steps and their kernels:
//  (i)   feature correspondences (registration.cpp:216-232): csrc/fmatch.hip.
//  (ii)  index triples (registration.cpp:235-239): host, mt19937 + Lemire (ctx.hip), one batch at
//        a time in bulk (whole twist blocks, Lemire's test per word); a batch is uploaded as one 64-bit word per triple
//        (three 21-bit indices and the valid bit: triple_pack, tdv_internal.hpp) for clouds of at most 2^21 points,
//        as int4 (i0,i1,i2,valid) above that; the kernels read either through a TriView.
//  (iii) k_ransac_hypotheses: one lane per hypothesis — centroids, H = S_c T_c^T, Jacobi SVD,
//        R = V U^T with reflection fix, t = c_t - R c_s (registration.cpp:242-268).
//  (iv)  k_ransac_score: one hypothesis per lane (R,t in VGPRs); points (source p and its
//        pre-gathered match q, two points per component-interleaved record) are broadcast through
//        the scalar data path and processed two at a time with packed f32 ops;
//        28 VALU ops per (hypothesis, point); the inlier test sqrt(d2) < thr is evaluated as
//        d2 < tau with tau = min{f : sqrtf(f) >= thr} (exactly equivalent, no sqrt in the loop).
//        Inlier counts are integers: partial counts per point-split are added with integer
//        atomics, which are order-independent, so counts are bit-exact and reproducible.
//  (v)   selection (registration.cpp:281-290) on the device, k_ransac_finish at the end of every batch: the first
//        iteration whose fitness passes the confidence, then the first largest fitness up to it - strict > on
//        float(inliers)/ns against the running best, which stays on the device with the winner's 12 floats; the host
//        reads one four-int record per batch.  A traced call downloads every count and runs the loop on the host.
//  (iv') k_order_flags / k_order_scatter: once per call with bail-out, after the first batch, the scoring pass' pair array again with
//        the running best's outliers first (RansacPointOrder): counts are order-free, the bail-out drops far more.  The outliers
//        come in two classes, the far ones first: a live hypothesis close to that best skips them in phase 1 under a bound on how
//        many of them it can hold (RansacFarBound: rf_near, with the bound kernels).
//  (vi)  k_ransac_rmse_partial / k_ransac_rmse_final: error sum of the winning hypothesis only, fixed-order reduction (per-workgroup
//        slabs, then one workgroup over the slabs).
#include "tdv_internal.hpp"
#include "host_wait.hpp"
#include "device_linalg.hpp"
#include "ransac_cut.hpp"
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <algorithm>
#include <type_traits>
#include <vector>

namespace tdv {

// The band unit: E = band_u (A + s) in RansacBand (ransac_hypothesis_lane), u = 2^-24.
constexpr float kUnitRoundoff = 5.9604644775390625e-08f;
constexpr float kBandUnit = 16.f * kUnitRoundoff;            // the FMA pass
constexpr float kBandUnitMatrix = 24.f * kUnitRoundoff;      // the study build's matrix-core pass

// ------------------------------------------------------------------ hypotheses
// pq layout: 8 floats per point: px py pz qx qy qz 0 0  (q = tgt[corr[i]]); padding points have
// p = 0 and q = +inf so that d2 = +inf and they are never inliers.
// A correspondence outside [0, nt) (caller-supplied lists are not trusted) raises *bad and reads target 0 instead of
// faulting; the host turns the flag into TDV_ERR_BAD_ARG at its first synchronisation.
// *pmax receives (integer atomic max on the bits of a non-negative float) the largest |source coordinate|, +inf for a
// non-finite one or a NaN in a matched target: it scales the rounding band of the fast scoring pass (k_ransac_score_fast).
// One pair record (a = px py pz qx, b = qy qz 0 0) of source point i and its match; returns the record's am, the pmax term.
template <class I>
__device__ __forceinline__ float pair_record(const float* __restrict__ src, const float* __restrict__ tgt, const int* __restrict__ corr, I i, int nt,
                                             int* __restrict__ bad, float4& a, float4& b) {
    int c = corr[i];
    if ((unsigned)c >= (unsigned)nt) { *bad = 1; c = 0; }
    a = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], tgt[3 * c]);
    b = make_float4(tgt[3 * c + 1], tgt[3 * c + 2], 0.f, 0.f);
    float am = fmaxf(fabsf(a.x), fmaxf(fabsf(a.y), fabsf(a.z)));
    if (!(am <= FLT_MAX)) am = INFINITY;      // inf (fmaxf drops a NaN: checked below)
    // a NaN coordinate - source or target - makes d2 NaN, whose sign bit the fast pass would read as "inlier" where it is
    // set: such a cloud is scored with the reference arithmetic throughout (an infinite target gives d2 = +inf in both)
    if (a.x != a.x || a.y != a.y || a.z != a.z || a.w != a.w || b.x != b.x || b.y != b.y) am = INFINITY;
    return am;
}
__device__ __forceinline__ void pair_record_padding(float4& a, float4& b) {
    a = make_float4(0.f, 0.f, 0.f, INFINITY);
    b = make_float4(INFINITY, INFINITY, 0.f, 0.f);
}
__global__ void k_gather_pq(const float* __restrict__ src, const float* __restrict__ tgt, const int* __restrict__ corr,
                            int ns, int ns_pad, int nt, float* __restrict__ pq, int* __restrict__ bad, unsigned* __restrict__ pmax) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    float am = 0.f;
    if (i < ns_pad) {
        float4 a, b;
        if (i < ns) am = pair_record(src, tgt, corr, i, nt, bad, a, b);
        else pair_record_padding(a, b);
        reinterpret_cast<float4*>(pq)[2 * (size_t)i] = a;
        reinterpret_cast<float4*>(pq)[2 * (size_t)i + 1] = b;
    }
    // one atomic per workgroup: thousands of them on one address would cost more than the gather itself
    __shared__ unsigned s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) am = fmaxf(am, __shfl_xor(am, off, 64));
    if ((threadIdx.x & 63) == 0 && am > 0.f) atomicMax(&s_max, __float_as_uint(am));
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(pmax, s_max);
}

__device__ __forceinline__ float tau_mid_default(float sqrt_tau) { return sqrt_tau * sqrt_tau; }

// A of the band (RansacBand below) for the hypothesis o[12] (column-major R, t): max over rows of (|r0| + |r1| + |r2|) P + |t|.
// A row that is NaN makes A NaN (fmaxf would drop it).  A NaN hypothesis - sampled from a pair with an infinite target or a NaN
// source - then gets no band: with a small one, the fast pass would read the sign bits of its NaN d2_fma as inliers wherever they
// are set.  Without a band the reference arithmetic scores it: no inliers.
__device__ __forceinline__ float ransac_band_reach(const float* o, float P) {
    float A = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (fabsf(o[c]) + fabsf(o[3 + c]) + fabsf(o[6 + c])) * P + fabsf(o[9 + c]);
        A = (a > A || a != a) ? a : A;
    }
    return A;
}

// hyp layout: SoA [14][h_pad]: r00 r10 r20 r01 r11 r21 r02 r12 r22 t0 t1 t2 (column-major R).
// Invalid (skipped) iterations get NaN so that no comparison is ever true -> 0 inliers.
// Rows 12, 13 of hyp: the band of the fast scoring pass for this hypothesis (RansacBand below): mid and half-width of
// the d2 interval inside which the FMA arithmetic and the reference's arithmetic might disagree on `d2 < tau`.
__device__ __forceinline__ void ransac_hypothesis_lane(const float* __restrict__ pq, const int4 tr, const bool valid, const int h, const int h_pad,
                                                       float* __restrict__ hyp, const unsigned* __restrict__ pmax, const float sqrt_tau, const float band_u,
                                                       float* o_out = nullptr) {
    float o[12];
    if (valid) {
        const int id[3] = {tr.x, tr.y, tr.z};
        float sp[3][3], tp[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* r = pq + (size_t)id[k] * 8;
            sp[k][0] = r[0]; sp[k][1] = r[1]; sp[k][2] = r[2];
            tp[k][0] = r[3]; tp[k][1] = r[4]; tp[k][2] = r[5];
        }
        float sc[3], tc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            sc[r] = dl::s3(sp[0][r], sp[1][r], sp[2][r]) / 3.0f;
            tc[r] = dl::s3(tp[0][r], tp[1][r], tp[2][r]) / 3.0f;
        }
        dl::Mat3 S, Tt;  // S(r,c) = centred source column c ; Tt = (centred target)^T
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) { dl::el(S, r, c) = sp[c][r] - sc[r]; dl::el(Tt, c, r) = tp[c][r] - tc[r]; }
        dl::Mat3 H = dl::mul3(S, Tt);
        dl::Mat3 R = dl::kabsch_rotation(H);
        float rx, ry, rz;
        dl::mulv3(R, sc[0], sc[1], sc[2], rx, ry, rz);
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = R.a[k];
        o[9] = tc[0] - rx; o[10] = tc[1] - ry; o[11] = tc[2] - rz;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = __builtin_nanf("");
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) hyp[(size_t)k * h_pad + h] = o[k];
    // RansacBand.  x_ref = fl((r0 px + (r1 py + r2 pz)) + t) and x_fma = fma(r0, px, fma(r1, py, fma(r2, pz, t))) are both
    // within gamma_4 resp. gamma_3 of the real value relative to A = |r0||px| + |r1||py| + |r2||pz| + |t| (u = 2^-24), so
    // they differ by at most 7.1 u A per component; the subtraction of q, the squared norm (three terms, either order)
    // and the square root add relative errors of a few u.  In distance: |sqrt(d2_ref) - sqrt(d2_fma)| <= 12.3 u A + 12 u s
    // for distances up to 2 s, s = sqrt(tau).  E = 16 u (A + s) with A bounded over all points by the largest |source
    // coordinate|; outside [(s - E)^2, (s + E)^2] (widened by 1e-6) both arithmetics give the same side of `d2 < tau`.
    // A band that is not small against s (coordinates far from the origin, non-finite data, an invalid hypothesis) is
    // stored as NaN: every chunk of such a lane's wave is then scored with the reference arithmetic.
    // (a skipped iteration or a padding lane has no band at all - half = 0 - so that it never makes its wave score a chunk
    // twice; its count is garbage and the host never reads it)
    float mid = tau_mid_default(sqrt_tau), half = valid ? __builtin_nanf("") : 0.f;
    if (valid) {
        const float A = ransac_band_reach(o, __uint_as_float(*pmax));
        const float E = (band_u * A + band_u * sqrt_tau) * 1.0001f;
        if (E < 0.25f * sqrt_tau) {
            const float lo = sqrt_tau - E, hi = sqrt_tau + E;
            const float tlo = lo * lo * (1.0f - 1e-6f), thi = hi * hi * (1.0f + 1e-6f);
            mid = 0.5f * (tlo + thi);
            half = 0.5f * (thi - tlo) * (1.0f + 1e-5f) + mid * 1e-6f;
        }
    }
    hyp[(size_t)12 * h_pad + h] = mid;
    hyp[(size_t)13 * h_pad + h] = half;
    if (o_out)
#pragma unroll
        for (int k = 0; k < 12; ++k) o_out[k] = o[k];
}
// RansacPlan's set-up of a batch (see k_ransac_score_fast and k_ransac_select below), done by one thread of k_ransac_hypotheses:
// stream order puts the previous batch's final state[0] in front of that kernel, and the bound and scoring kernels that read the
// plan and append to the zeroed counters come after it.  plan == nullptr: a batch without bail-out.
struct RansacFar;
struct PlanJob { int* state; int* plan; int ns, n_pchunks, drop_permille; int* n_live; int* units; int n_units;   // units: the batch's ticket words (k_ransac_score_fast, job B)
                 const RansacFar* far; int a_permille; };                                                  // RansacFarBound: the classes, and the near lists' share of I in phase 1
__device__ __forceinline__ void ransac_plan(const PlanJob& j);
// What a bounded batch's hypotheses are judged by before the leaf walk (ransac_prejudge, beside k_ransac_bound): flags == nullptr in a batch without bound
struct PreJob { int* flags; int* ubf; const RansacFar* far; const unsigned* enc; const float* best12; float live_radius; int u_cut_permille; };
__device__ __forceinline__ void ransac_prejudge(const PreJob& j, const float* o, bool valid, int h, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u,
                                                const int* __restrict__ state, int ns);
// up != nullptr: the batch's triples as the host drew them, in pinned host memory, which the device reads as it is (it writes a
// batch's record there).  Lane h loads its triple from there and stores it to `triples` for the batch's later kernels (the bound, the
// select kernels and k_ransac_finish ask triples.valid(h)): the batch needs no copy in front of this kernel.
// up == nullptr: `triples` holds them already - carried there by the coarse bound level of the batch before (RansacStage, the
// default from a call's third batch on), or by a copy (study build, TDV_RANSAC_UPLOAD=inline).
// h_end: the hypothesis slots this batch covers (whole scoring blocks, the padding behind `count` as invalid lanes); h_pad is the stride.
__global__ void k_ransac_hypotheses(const float* __restrict__ pq, const TriView triples, const void* __restrict__ up, int count, int h_end, int h_pad,
                                    float* __restrict__ hyp, const unsigned* __restrict__ pmax, float sqrt_tau, int* __restrict__ counts,
                                    float band_u /* E = band_u (A + s): kBandUnit or kBandUnitMatrix */, const PlanJob plan, const PreJob pre) {
    int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h == 0 && plan.plan) ransac_plan(plan);
    if (h < plan.n_units) plan.units[h] = 0;     // job B of this batch's two scoring dispatches draws its units from them (n_units <= h_end)
    if (h >= h_end) return;
    counts[h] = 0;                       // the scoring kernel adds its point-splits' counts here (one memset launch less per batch)
    bool valid = false;
    int4 tr = make_int4(0, 0, 0, 0);
    if (h < count) {
        if (up) {
            if (triples.packed) {
                const uint64_t w = static_cast<const uint64_t*>(up)[h];
                const_cast<uint64_t*>(static_cast<const uint64_t*>(triples.p))[h] = w;
                tr = TriView::unpack(w);
            } else {
                tr = static_cast<const int4*>(up)[h];
                const_cast<int4*>(static_cast<const int4*>(triples.p))[h] = tr;
            }
        } else tr = triples.load(h);
        valid = tr.w != 0;
    }
    float o[12];
    ransac_hypothesis_lane(pq, tr, valid, h, h_pad, hyp, pmax, sqrt_tau, band_u, o);
    if (pre.flags) ransac_prejudge(pre, o, valid, h, pmax, sqrt_tau, band_u, plan.state, plan.ns);      // (uniform)
}

__device__ __forceinline__ unsigned long long shfl_u64_down(unsigned long long v, int o) {
    const unsigned lo = __shfl_down((unsigned)v, o, 64), hi = __shfl_down((unsigned)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// "The first largest fitness" as one maximum (k_ransac_finish, k_rb_select): key = fitness bits (positive floats order as their
// bits), then `earlier`, which is larger for the EARLIER iteration; 0 = none.  first_best_wave: lane 0 gets the wave's largest key.
__device__ __forceinline__ unsigned long long first_best_key(float fit, int earlier) { return ((unsigned long long)__float_as_uint(fit) << 32) | (unsigned)earlier; }
__device__ __forceinline__ unsigned long long first_best_wave(unsigned long long best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long x = shfl_u64_down(best, o); best = x > best ? x : best; }
    return best;
}

// ------------------------------------------------------------------ scoring
#ifndef RS_BLOCK_VALUE
#define RS_BLOCK_VALUE 1024
#endif
#ifndef RS_XCD_R
#define RS_XCD_R 8           // XCD groups over the point ranges (1, 2, 4 or 8); 8 / RS_XCD_R groups over the hypothesis blocks
#endif
constexpr int RS_BLOCK = RS_BLOCK_VALUE;   // 16 waves per workgroup walk the same points together (measured at 200k x 57k hyps: 128 threads 74 %,
                                           // 256 82 %, 512 85 %, 1024 87 % of the VALU peak; 3-12k workgroups make no difference)
constexpr int RS_HYP_PER_BLOCK = RS_BLOCK;   // one hypothesis per lane (measured best: R,t in 24 VGPRs, highest occupancy)
#ifndef RS_PCH_VALUE
#define RS_PCH_VALUE 8
#endif
constexpr int RS_PCH = RS_PCH_VALUE;   // points per scalar chunk: 4 records of 12 floats (8 measured 81 % of peak, 4: 80 %)
// (The cuts of a scoring dispatch - point_ranges for job A, score_unit for job B - are in ransac_cut.hpp.)

// The scoring loop reads a second pair array that holds TWO points per record, component-interleaved
// [px0 px1 | py0 py1 | pz0 pz1 | qx0 qx1 | qy0 qy1 | qz0 qz1] (48 B per 2 points), so that every arithmetic op is one
// v_pk_*_f32 on an aligned SGPR pair — the same per-element IEEE operations as a scalar loop, half the
// instructions, no SGPR shuffling (measured 81 % of the VALU peak against 79 % for the loop vectoriser's packing of
// the 8-float layout and 71 % for scalar code).
typedef float v2f __attribute__((ext_vector_type(2)));
struct Pair2 { v2f px, py, pz, qx, qy, qz; };
__device__ __forceinline__ Pair2 pair2(const float* v, int p) {      // record p of a chunk held in v
    return Pair2{{v[12 * p + 0], v[12 * p + 1]}, {v[12 * p + 2], v[12 * p + 3]}, {v[12 * p + 4], v[12 * p + 5]},
                 {v[12 * p + 6], v[12 * p + 7]}, {v[12 * p + 8], v[12 * p + 9]}, {v[12 * p + 10], v[12 * p + 11]}};
}
// The pair test in the reference's arithmetic (registration.cpp:270-279, no contraction) for a record's two points under the
// hypothesis r (each of the 12 values in both halves): the two d2, and their test.
__device__ __forceinline__ v2f ref_pair_d2(const v2f* r, const Pair2& a) {
    const v2f x = (r[0] * a.px + (r[3] * a.py + r[6] * a.pz)) + r[9];
    const v2f y = (r[1] * a.px + (r[4] * a.py + r[7] * a.pz)) + r[10];
    const v2f z = (r[2] * a.px + (r[5] * a.py + r[8] * a.pz)) + r[11];
    const v2f dx = x - a.qx, dy = y - a.qy, dz = z - a.qz;
    return dx * dx + (dy * dy + dz * dz);
}
__device__ __forceinline__ void count_inliers(v2f d2, float tau, int& cnt) { cnt += (d2.x < tau) ? 1 : 0; cnt += (d2.y < tau) ? 1 : 0; }
__global__ void k_pack_pq2(const float* __restrict__ pq, int ns_pad, float* __restrict__ pq2) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;   // pair index
    if (2 * i >= ns_pad) return;
    const float* a = pq + (size_t)(2 * i) * 8; const float* b = a + 8;
    float* o = pq2 + (size_t)i * 12;
#pragma unroll
    for (int c = 0; c < 6; ++c) { o[2 * c] = a[c]; o[2 * c + 1] = b[c]; }
}
__global__ __launch_bounds__(RS_BLOCK)
void k_ransac_score(const float* __restrict__ hyp, int h_pad, const float* __restrict__ pq2,
                       int n_pchunks, int pchunks_per_split, float tau, int* __restrict__ counts) {
    const int split = blockIdx.y;
    const int c0 = split * pchunks_per_split;
    const int c1 = min(n_pchunks, c0 + pchunks_per_split);
    const int base = blockIdx.x * RS_BLOCK + threadIdx.x;
    v2f r[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) { const float t = hyp[(size_t)e * h_pad + base]; r[e] = (v2f){t, t}; }
    int cnt = 0;
    for (int c = c0; c < c1; ++c) {
        const float* __restrict__ g = pq2 + (size_t)c * (6 * RS_PCH);  // RS_PCH points = RS_PCH/2 records of 12 floats, wave-uniform
        float v[6 * RS_PCH];
#pragma unroll
        for (int e = 0; e < 6 * RS_PCH; ++e) v[e] = g[e];
#pragma unroll
        for (int p = 0; p < RS_PCH / 2; ++p) {
            count_inliers(ref_pair_d2(r, pair2(v, p)), tau, cnt);
        }
    }
    atomicAdd(&counts[base], cnt);
}

// The same counts from half the arithmetic.  Parity forbids FMA contraction in the reference's expression, but only
// its RESULT - which side of tau each d2 falls on - has to be reproduced.  This pass evaluates every (hypothesis, point)
// with fused multiply-adds (15 packed instructions per two points instead of 26) and classifies by the sign of
// d2_fma - mid; a test whose d2_fma lies inside the hypothesis' rounding band (RansacBand in k_ransac_hypotheses: the
// two arithmetics provably agree outside it) makes its wave score that chunk of 8 points again with the reference
// arithmetic.  The band is about 1e-3 of the threshold wide at metre-scale coordinates, so this happens for a percent or
// so of the chunks; counts are identical to k_ransac_score's (tests/test_gpu_ransac.py holds the two against each other
// and against the oracle).
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
// Exact bail-out (RansacPlan, below).  One dispatch carries up to two JOBS, decoded from the workgroup id:
//   job A (ids below g1): a batch's hypotheses, one block of RS_BLOCK per id, over the first plan[0] chunks of the points
//                         (plan == nullptr: over all of them) cut EVENLY into a.ps ranges - every workgroup of the job has the
//                         same amount of work, whatever the prefix (the first version cut the whole point range and let the
//                         workgroups past the prefix exit: 3,648 busy workgroups on 512 slots, an eighth of the last round idle);
//   job B (the ids after): phase 2 of the PREVIOUS batch - the hypotheses its selection listed (plan[1] of them: those that
//                         can still beat the best count known) over the chunks its phase 1 left out.
// By default the two jobs are dispatched one after the other (job B alone, see RansacRun::enqueue); with TDV_RANSAC_MERGE=1 job B
// rides behind the NEXT batch's job A.
//   job B also scores phase 1 of a batch whose dead hypotheses k_ransac_bound has taken out (RansacLeafBound, below): n_live set,
//                         the live list (*n_live of them) over the chunks [0, plan[0]).
// Job B's workgroups are RESIDENT and pull their work (round 10; until then one (range of 30-155 chunks, block) item each, and per
// item a gather through the list, 14 strided loads, 1,024 scattered atomics and the statistics' two barriers - which a job-A
// workgroup of a full batch pays once per 260 chunks): a workgroup holds one hypothesis block in registers and draws units of
// RS_UNIT chunks of its XCD's share for that block from the block's ticket word (score_unit), the next ticket travelling while a unit
// is scored; the counts stay in registers until the block's units are drained - one atomicAdd per lane - and the workgroup moves to
// the next block (score_unit_block), so the tail balances itself.  Tickets only: no workgroup waits for another, any grid of at
// least 8 workgroups drains any list.  The words are zeroed by the batch's k_ransac_hypotheses.
struct ScoreJob {
    const float* hyp; int* counts; const int* plan; const int* list;
    int hb;      // hypothesis blocks (A: of the batch; B: upper bound - the real number comes from plan[1] or *n_live)
    int ps;      // A: point ranges
    const int* n_live;   // B: phase 1 over the live list (nullptr: phase 2)
    int* units;          // B: this dispatch's ticket words, [8 XCDs][hb]
    const int* c_far;    // B: a NEAR list (RansacFarBound): the chunks wholly inside F, which its phase 1 skips (nullptr: a far list)
};
// One block of hypotheses (lane = hypothesis `base`, -1: none) over the chunks [c0, c1) of the point pairs; returns the lane's
// inlier count, adds the point PAIRS the wave scored twice to n_rescored (wave-uniform; RS_PCH / 2 per chunk that was re-scored whole).
// (A finer band test - per PAIR of points instead of per chunk of eight - was built for the batch's small clouds, half of whose
// hypotheses are decent, so that some of a wave's 512 tests per chunk nearly always sit at the threshold and 49 % of the chunks are
// re-scored (k_rb_score, C5): the share stayed at 49 % and the pass got slower, 2.52 against 2.30 ms.  Removed in round 4.)
// ADAPT: a wave that had to re-score three of its first eight chunks stops trying the FMA pass and scores the rest of its range with
// the reference arithmetic alone (28 ops per test instead of 16.6 + 28: cheaper from a re-scoring share of 0.4 on).  Measured on C5:
// per-chunk band test 2.30 ms, per-pair band test 2.52 ms (the share stays at 49 % even for 128 tests), adaptive exact: see k_rb_score.
// A lane's hypothesis in registers: each of the 12 values in both halves of a packed operand, and its band.
struct HypLane { v2f r[12]; float mid, half; };
__device__ __forceinline__ HypLane load_hyp(const float* __restrict__ hyp, const int h_pad, const int base, const float tau) {
    HypLane l;
#pragma unroll
    for (int e = 0; e < 12; ++e) { const float t = base >= 0 ? hyp[(size_t)e * h_pad + base] : __builtin_nanf(""); l.r[e] = (v2f){t, t}; }
    l.mid = base >= 0 ? hyp[(size_t)12 * h_pad + base] : tau; l.half = base >= 0 ? hyp[(size_t)13 * h_pad + base] : 0.f;   // a lane without a hypothesis has no band
    return l;
}
// WRAP: [c0, c1) is a VIRTUAL chunk range that may run past the array's `wrap` chunks and goes on at chunk 0 (phase 2 of a near list:
// the tail, then the F chunks its phase 1 skipped).
template <bool ADAPT = false, bool WRAP = false>
__device__ __forceinline__ int score_chunks(const HypLane& l, const float* __restrict__ pq2, const int c0, const int c1, const float tau, unsigned& n_rescored, const int wrap = 0) {
    const v2f* const r = l.r;
    const float mid = l.mid, half = l.half;
    const v2f nmid = {-mid, -mid};
    int cnt = 0;
    int c_fast_end = c1;         // ADAPT: where the FMA pass gives up (wave-uniform)
    for (int c = c0; c < c_fast_end; ++c) {
        if (ADAPT && c == c0 + 8 && n_rescored >= 3u * (RS_PCH / 2)) { c_fast_end = c; break; }      // (n_rescored counts pairs: three whole chunks)
        const int pc = (WRAP && c >= wrap) ? c - wrap : c;
        const float* __restrict__ g = pq2 + (size_t)pc * (6 * RS_PCH);  // RS_PCH points = RS_PCH/2 records of 12 floats, wave-uniform
        float v[6 * RS_PCH];
#pragma unroll
        for (int e = 0; e < 6 * RS_PCH; ++e) v[e] = g[e];
        float m = INFINITY;      // smallest |d2_fma - mid| of this lane in the chunk
        unsigned sgn = 0u;       // the signs of d2_fma - mid, shifted in one per test (1 = below mid = inlier)
        int cf = 0;
        v2f tt[RS_PCH / 2];      // d2_fma - mid of every test, kept for the re-scoring branch (which pairs are inside a band)
#pragma unroll
        for (int p = 0; p < RS_PCH / 2; ++p) {
            const Pair2 a = pair2(v, p);
            const v2f dx = fma2(r[0], a.px, fma2(r[3], a.py, fma2(r[6], a.pz, r[9]))) - a.qx;
            const v2f dy = fma2(r[1], a.px, fma2(r[4], a.py, fma2(r[7], a.pz, r[10]))) - a.qy;
            const v2f dz = fma2(r[2], a.px, fma2(r[5], a.py, fma2(r[8], a.pz, r[11]))) - a.qz;
            // d2_fma - mid as one chain ending in -mid: its own rounding, at most 3 u mid = 1.5 u s in distance, sits inside
            // the 3.7 u A + 4 u s that the band's E keeps in reserve over the proven bound
            const v2f t = fma2(dx, dx, fma2(dy, dy, fma2(dz, dz, nmid)));
            tt[p] = t;
            m = fminf(fminf(m, fabsf(t.x)), fabsf(t.y));            // one v_min3_f32; a NaN (invalid hypothesis) leaves m alone: half is NaN there
            sgn = __builtin_amdgcn_alignbit(sgn, __float_as_uint(t.x), 31);      // sgn = sgn << 1 | sign(t.x)
            sgn = __builtin_amdgcn_alignbit(sgn, __float_as_uint(t.y), 31);
        }
        cf = __popc(sgn);
        if (__any(!(m >= half))) {      // some lane of the wave is inside its band (or has none): the reference arithmetic decides
            // ... the PAIRS of points that some lane has inside its band (round 4; until then the whole chunk: a hit is nearly always one
            // (lane, point), so three quarters of the second scoring were spent on pairs nobody doubted).  n_rescored counts pairs.
#pragma unroll
            for (int p = 0; p < RS_PCH / 2; ++p) {
                const float mp = fminf(fminf(INFINITY, fabsf(tt[p].x)), fabsf(tt[p].y));       // (NaN - an invalid hypothesis - leaves INFINITY)
                if (!ADAPT && !__any(!(mp >= half))) continue;                                 // (the small-cloud pass keeps re-scoring whole chunks: its ADAPT rule counts them)
                ++n_rescored;
                const v2f d2 = ref_pair_d2(r, pair2(v, p));
                // the pair's two sign bits in sgn: test 2p at bit RS_PCH - 1 - 2p, test 2p + 1 right below it
                cf -= __popc((sgn >> (RS_PCH - 2 - 2 * p)) & 3u);
                count_inliers(d2, tau, cf);
            }
        }
        cnt += cf;
    }
    if (ADAPT) {
        for (int c = c_fast_end; c < c1; ++c) {          // the reference arithmetic alone (k_ransac_score's loop)
            const float* __restrict__ g = pq2 + (size_t)c * (6 * RS_PCH);
            float v[6 * RS_PCH];
#pragma unroll
            for (int e = 0; e < 6 * RS_PCH; ++e) v[e] = g[e];
#pragma unroll
            for (int p = 0; p < RS_PCH / 2; ++p) {
                count_inliers(ref_pair_d2(r, pair2(v, p)), tau, cnt);
            }
        }
    }
    return cnt;
}
template <bool ADAPT = false>
__device__ __forceinline__ int score_range_fast(const float* __restrict__ hyp, const int h_pad, const int base, const float* __restrict__ pq2,
                                                const int c0, const int c1, const float tau, unsigned& n_rescored) {
    return score_chunks<ADAPT>(load_hyp(hyp, h_pad, base, tau), pq2, c0, c1, tau, n_rescored);
}
// One value from thread 0 to its whole workgroup, as a wave-uniform scalar (job B's tickets).  One barrier per call: s[2] is used in
// turns (`flip`), and a wave can be at most one call behind thread 0, which writes the other word then.
__device__ __forceinline__ int workgroup_value(int mine, int* s, int& flip) {
    if (threadIdx.x == 0) s[flip] = mine;
    __syncthreads();
    const int v = __builtin_amdgcn_readfirstlane(s[flip]);
    flip ^= 1;
    return v;
}

// A lane's returning atomicAdd(word, 1) whose result is awaited where it is USED.  The compiler's atomic optimizer turns an add to an
// address it can prove wave-uniform into a wave reduction and waits for the result right there; behind an offset it cannot see
// through, the add stays one plain atomic of the calling lane and travels while the lane goes on.
__device__ __forceinline__ int draw_ticket(int* word) {
    int zero = 0;
    asm volatile("" : "+v"(zero));
    return atomicAdd(word + zero, 1);
}

// statistics only (tdv_ctx_last_ransac_rescore / _scored): two atomics per workgroup - point pairs scored twice (n_rescored, wave-uniform),
// and (wave, chunk) pairs scored: `waves` x `chunks`, both workgroup-uniform; every thread of the workgroup calls it.
// The scored share counts the 16 waves of a block for every chunk the block walks - job A and the small-cloud pass, where every wave
// scores (padding lanes included), and phase 1 over a live list, so that a bounded batch whose hypotheses are all live reports job A's
// share.  Phase 2 alone counts, per block, the waves that hold a listed hypothesis (the caller passes waves = 1 and their sum in
// `chunks`): its list may fill a fraction of one block, whose other waves skip the arithmetic.  DESIGN.md 4 states the definition.
template <class C>
__device__ __forceinline__ void score_stats(unsigned n_rescored, C chunks, unsigned long long* __restrict__ rescored, unsigned waves = RS_BLOCK / 64) {
    __shared__ unsigned s_rescored;
    if (threadIdx.x == 0) s_rescored = 0u;
    __syncthreads();
    if (n_rescored && (threadIdx.x & 63) == 0) atomicAdd(&s_rescored, n_rescored);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_rescored) atomicAdd(rescored, (unsigned long long)s_rescored);
        atomicAdd(rescored + 1, (unsigned long long)waves * (unsigned long long)chunks);
    }
}

// TDV_TIMER_RANSAC_SCORE without events (an event on either side of the dispatch cost the batch 5.7 us each,
// profiles/r18/ransac_no_events.md): with timing on the dispatch gets a {t0, t1} pair (all the t0 words of a call, then all its t1
// words: two memsets set them to all ones and 0), and thread 0 of a workgroup stamps the constant-rate clock into it - a minimum into
// t0 as its first action, a maximum into t1 as its last, on every way out (behind score_stats' barriers, where thread 0 is the
// workgroup's last word).  Atomics without a return: nothing waits for them.  t0 is stamped by the first eight workgroups only, one per
// XCD: workgroups are dispatched in order, so the first to start is among them, and the other workgroups do not begin by waiting for
// the clock.  t1 - t0 is the first workgroup's start to the last workgroup's end, inside the dispatch.  The kernel is a template
// over STAMP: with timing off the instance that runs is the kernel without any of this (measured: the stamps' code alone, never
// executed, cost phase 2 1.5 us of 46).
struct ScoreStamp { unsigned long long *t0, *t1; };
template <bool STAMP> __device__ __forceinline__ void score_stamp_begin(const ScoreStamp& stamp) { if (STAMP && threadIdx.x == 0 && blockIdx.x < 8) atomicMin(stamp.t0, wall_clock64()); }
template <bool STAMP> __device__ __forceinline__ void score_stamp_end(const ScoreStamp& stamp) { if (STAMP && threadIdx.x == 0) atomicMax(stamp.t1, wall_clock64()); }

// Occupancy (round 4).  The loop keeps a chunk's 48 floats in SGPRs and the compiler took 106 of them: 7 waves per SIMD on paper, but a
// workgroup is 16 waves (4 per SIMD), so ONE workgroup per CU - 4 waves per SIMD to hide the scalar loads of a loop whose waves walk the
// same chunks nearly in step.  Capped at the 8-wave budget (80 SGPRs; 43 values spilled to VGPR lanes, all outside the chunk loop) two
// workgroups share a CU: 1,098 -> 1,211 steps/s of bench.py on the same box, `frac` 0.70 -> 0.78.  Also measured: chunks of 4 points
// with it (16 spills: 1,209-1,223, within a point of this), chunks of 2 (1,140), 512-thread workgroups (1,177), chunks of 4 without it (1,034);
// and, at 8 waves, a loop that loads the NEXT pair of points while it computes one (12 SGPRs in flight instead of 48, two waits per chunk
// instead of one wait on everything): 1,196-1,210 against 1,213-1,221 on one box - with two workgroups per CU the scalar loads are hidden already.
template <bool STAMP>
__global__ __launch_bounds__(RS_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_ransac_score_fast(const ScoreJob a, const ScoreJob b, const int g1, const int h_pad, const float* __restrict__ pq2,
                         const int n_pchunks, const float tau, unsigned long long* __restrict__ rescored, const ScoreStamp stamp) {
    const int id = blockIdx.x;
    score_stamp_begin<STAMP>(stamp);
    unsigned n_rescored = 0;     // wave-uniform
    unsigned chunks = 0;         // chunks this workgroup walked (workgroup-uniform)
    if (id < g1) {
        // XCD-aware deal (round 4).  An XCD (workgroup id mod 8) has its own L2.  Round 3 gave every XCD an eighth of the hypothesis blocks
        // and ALL point ranges: every L2 pulled the whole pair array (PMC: 38.4 MB of HBM traffic per dispatch for 4.8 MB of pairs).  Now
        // the eight XCDs form RS_XCD_R groups over the point ranges x 8 / RS_XCD_R groups over the hypothesis blocks: an L2 holds
        // 1 / RS_XCD_R of the pairs and 1 / (8 / RS_XCD_R) of the hypotheses (52 B each).
        const int xcd = id & 7, k = id >> 3;
        constexpr int XR = RS_XCD_R, XH = 8 / RS_XCD_R;
        const int hbl = (a.hb + XH - 1) / XH;
        const int hblock = (k % hbl) * XH + xcd / XR, split = (k / hbl) * XR + xcd % XR;
        if (hblock >= a.hb || split >= a.ps) { score_stamp_end<STAMP>(stamp); return; }   // (counts that are not multiples of the group sizes: the last groups are short)
        const int c_split = a.plan ? a.plan[0] : n_pchunks;
        const int per = (c_split + a.ps - 1) / a.ps;
        const int c0 = split * per, c1 = min(c_split, c0 + per);
        if (c0 >= c1) { score_stamp_end<STAMP>(stamp); return; }        // workgroup-uniform (ids past hb * ps, a prefix shorter than ps chunks)
        const int base = hblock * RS_BLOCK + threadIdx.x;
        const int cnt = score_range_fast(a.hyp, h_pad, base, pq2, c0, c1, tau, n_rescored);
        atomicAdd(&a.counts[base], cnt);
        chunks = (unsigned)(c1 - c0);
    } else {
        // Few hypothesis blocks are left, and the points reach the scalar cache through the XCD's L2: an XCD (workgroup id mod 8)
        // walks its own eighth of the chunks for ALL surviving blocks, its workgroups spread over the blocks and advancing through
        // the share at the same pace (a workgroup that walked a point range alone missed on every chunk: 1.2 ms for 5 % of the work).
        // One dispatch drains up to two lists, b's and then (g1 == 0 and other ticket words) a's: a bounded batch's far and near list.
        // A far list's phase 1 is the chunks [0, plan[0]), its phase 2 [plan[0], n_pchunks); a near list's phase 1 is [c_far, plan[3]),
        // its phase 2 the rest as one virtual range [plan[3], n_pchunks + c_far) that wraps to chunk 0.
        const int j0 = id - g1, xcd = j0 & 7, wg = j0 >> 3;
        __shared__ int s_ticket[2];
        int flip = 0;
        unsigned long long wave_chunks = 0ull;       // statistics: (wave, chunk) pairs this workgroup counts (score_stats)
        for (int pass = 0; pass < 2; ++pass) {
            if (pass && (g1 != 0 || a.units == b.units)) break;
            const ScoreJob& j = pass ? a : b;
            const bool phase1 = j.n_live != nullptr;
            const int n_list = phase1 ? *j.n_live : j.plan[j.c_far ? 4 : 1];
            const int n_blk = (n_list + RS_BLOCK - 1) / RS_BLOCK;
            if (n_blk == 0) continue;
            const int skip = j.c_far ? *j.c_far : 0, cut = j.plan[j.c_far ? 3 : 0];
            const int r0 = phase1 ? skip : cut, r1 = phase1 ? cut : n_pchunks + skip;
            for (int visit = 0; visit < n_blk; ++visit) {
                const int hblock = score_unit_block(wg, visit, n_blk);
                int* const word = j.units + (size_t)xcd * j.hb + hblock;
                int next = 0, c0 = 0, c1 = 0;
                if (threadIdx.x == 0) next = draw_ticket(word);
                if (!score_unit(workgroup_value(next, s_ticket, flip), r0, r1, xcd, c0, c1)) continue;   // drained (workgroup-uniform)
                const int slot = hblock * RS_BLOCK + threadIdx.x;
                const int base = slot < n_list ? j.list[slot] : -1;
                // a wave whose 64 slots are all past the end of the list has nothing to count: it keeps out of the issue slots of
                // the waves that do, and only joins the barriers
                const bool wave_scores = __builtin_amdgcn_readfirstlane(slot - (int)(threadIdx.x & 63)) < n_list;
                const HypLane l = load_hyp(j.hyp, h_pad, base, tau);
                const int stat_waves = phase1 ? RS_BLOCK / 64 : min(RS_BLOCK / 64, (n_list - hblock * RS_BLOCK + 63) / 64);   // (see score_stats)
                int cnt = 0;
                do {
                    if (threadIdx.x == 0) next = draw_ticket(word);       // in flight while this unit is scored
                    if (wave_scores) cnt += score_chunks<false, true>(l, pq2, c0, c1, tau, n_rescored, n_pchunks);
                    wave_chunks += (unsigned long long)stat_waves * (unsigned)(c1 - c0);
                } while (score_unit(workgroup_value(next, s_ticket, flip), r0, r1, xcd, c0, c1));
                if (base >= 0) atomicAdd(&j.counts[base], cnt);
            }
        }
        if (!wave_chunks) { score_stamp_end<STAMP>(stamp); return; }
        score_stats(n_rescored, wave_chunks, rescored, 1u);
        score_stamp_end<STAMP>(stamp);
        return;
    }
    score_stats(n_rescored, chunks, rescored);
    score_stamp_end<STAMP>(stamp);
}

// RansacFarBound's per-call state (the rules are with the bound kernels below).  The pairs are ordered [F | M | I] by the ORDERING
// pose B - the running best when k_order_flags ran, kept here because the running best may change later in the call:
//   F  finite pairs with d2_B >= rF2, d2_B the reference arithmetic's squared distance under B (ref_pair_d2);
//   M  the other outliers of B - every pair with a non-finite coordinate or a NaN d2_B among them;
//   I  B's inliers.
// cum is a count table over d2_B of the F pairs: bin = the leading bits of the non-negative float (monotone in its value), so
// cum[bin(t)] counts every F pair whose bin is at most t's, which holds all of them with d2_B < t: the lookup errs upward only.
constexpr int RF_SHIFT = 20, RF_BINS = 2048;                      // sign (0), exponent and three mantissa bits
struct RansacFar {
    float ord12[12];            // B
    int n_far, n_mid;           // |F|, |M|
    int c_far;                  // chunks wholly inside F: what a near hypothesis' phase 1 skips
    int pad;
    unsigned hist[RF_BINS];     // F pairs per bin (zeroed with the call's block, added up by k_order_flags)
    unsigned cum[RF_BINS];      // ... and in the bins up to and including this one (k_order_scatter)
};
__device__ __forceinline__ int rf_bin(float t) { return (int)(__float_as_uint(t) >> RF_SHIFT); }      // t >= 0, no NaN
// Where phase 1 of the near lists ends: behind M and the first a_permille of I (at least at F's end, at most at the array's).
__device__ __forceinline__ int ransac_near_end(const RansacFar& f, int ns, int n_pchunks, int a_permille) {
    const int out = f.n_far + f.n_mid, a = (int)((long long)(ns - out) * a_permille / 1000);
    return min(n_pchunks, (out + a + RS_PCH - 1) / RS_PCH);
}
// RansacPlan — exact bail-out.  The loop of ransacRegistration (registration.cpp:284-290) uses an iteration's inlier count only
// to ask whether it beats the best so far (strictly) — the early exit `fitness > confidence` can fire only on such a new best,
// the loop having stopped otherwise when the earlier best passed it.  So a hypothesis whose count over the first chunks plus
// ALL the remaining points cannot exceed the best count of the EARLIER batches needs no exact count: it is scored over the
// prefix only, and whatever partial count the host reads for it compares as the true one would.  The best hypothesis itself
// always survives, so the returned transform, inlier count, fitness, rmse and iteration are the reference's.  The running best
// stays on the device (no host round trip between batches): plan = { chunks in phase 1, survivors, best count so far }.
// Used only when the caller asked for no per-iteration trace.
// state[0] = best count known so far (a lower bound of the best count of every batch already enqueued: full counts of the
// batches that are complete, prefix counts of the one whose phase 2 is still to run).  plan = { chunks in phase 1, survivors,
// largest PREFIX count of this batch } - one plan per batch buffer, the state shared.
// (One thread of k_ransac_hypotheses makes the plan: a launch of its own - one thread behind a stream barrier - cost as much as k_ransac_best.)
__device__ __forceinline__ void ransac_plan(const PlanJob& j) {
    const int best = j.state[0], ns = j.ns, n_pchunks = j.n_pchunks;
    if (j.n_live) { j.n_live[0] = 0; j.n_live[2] = 0; j.n_live[4] = 0; j.n_live[6] = 0; }      // (RansacLeafBound: k_ransac_bound appends to them next: live, undecided, near; its close count)
    int c_split = n_pchunks;
    const int rest = best - max((int)((long long)best * j.drop_permille / 1000), 1);   // points left to phase 2: a hypothesis with under that share of the best count in the prefix is dropped
    if (rest >= ns / 8)                                      // (below an eighth of the points a second phase costs more than it saves)
        c_split = min(n_pchunks, (ns - rest + RS_PCH - 1) / RS_PCH);
    j.plan[0] = c_split; j.plan[1] = 0; j.plan[2] = 0;
    j.plan[3] = j.far ? ransac_near_end(*j.far, ns, n_pchunks, j.a_permille) : 0; j.plan[4] = 0;     // near lists: where phase 1 ends, survivors
}
// largest count of a batch (prefix counts after phase 1, full counts after phase 2) -> *dst by atomic max, one atomic per
// workgroup (one per wave on the same address cost 12 us for a 65,536-hypothesis batch)
__global__ __launch_bounds__(1024)
void k_ransac_best(const TriView triples, int count, const int* __restrict__ counts, int* __restrict__ dst) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    int c = (h < count && triples.valid(h)) ? counts[h] : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c = max(c, __shfl_xor(c, off, 64));
    __shared__ int s_max[16];
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) c = max(c, s_max[w]);
        if (c > 0) atomicMax(dst, c);
    }
}
// Which hypotheses of a batch go on to phase 2.  With rest = the points phase 1 left out, ub = count + rest bounds a
// hypothesis' full count from above.  It is dropped when it provably is neither the result nor the iteration the loop of
// registration.cpp:284-290 stops at:
//   (a) ub <= best of the EARLIER batches.  It cannot be a new best at its iteration (strict >, :284), and the early exit
//       (:290) can only fire on a new best: had an earlier iteration reached `fitness > confidence` the loop would have ended
//       there.  Ties with the earlier best lose by the strict comparison, so <= is enough.  [round 2]
//   (b) ub < L, L = the largest PREFIX count inside this very batch, and float(ub)/ns is not > confidence.  Some hypothesis
//       h* of the batch has a full count >= L > ub, so this one is not the final result whatever the order of the two (strict
//       <: with ub == L and h* LATER than it, a tie would go to the earlier iteration, i.e. to the dropped one).  It could
//       still be a new best at its own iteration when h* comes later, and an exit firing there would return it - hence the
//       second condition: with no count up to ub passing the confidence test, the exit cannot fire on it.  Conversely an exit
//       that fires at a kept iteration e returns e itself: anything earlier with at least its count would have ended the loop
//       before, and every dropped iteration has a count below the confidence bar that e passed.  [round 3]
// Either way the counts of the dropped hypotheses stay partial and compare as the true ones would: below the result's.
// Appends h to list (*n entries so far) for the lanes that `take`, one atomic per wave; returns the lane's slot.
__device__ __forceinline__ int rb_append(bool take, int lane, int h, int* __restrict__ list, int* __restrict__ n) {
    const unsigned long long m = __ballot(take);
    if (!m) return 0;
    const int lead = (int)__builtin_ctzll(m);
    int at = 0;
    if (lane == lead) at = atomicAdd(n, __popcll(m));
    at = __shfl(at, lead, 64) + __popcll(m & ((1ull << lane) - 1ull));
    if (take) list[at] = h;
    return at;
}
// `prefix` = the hypothesis' count over phase 1, `best` = rule (a)'s, `in_batch` = rule (b)'s L.
__device__ __forceinline__ bool ransac_keep(int prefix, int rest, int best, int in_batch, int ns, float confidence) {
    const int ub = prefix + rest;
    const bool passes = static_cast<float>(ub) / static_cast<float>((size_t)ns) > confidence;   // registration.cpp:281,290 on the bound
    return ub > best && (ub >= in_batch || passes);
}
__device__ __forceinline__ int ransac_rest(int ns, int c_split) { return max(0, ns - min(ns, c_split * RS_PCH)); }   // points phase 1 left out (the padding past ns is never an inlier)
__global__ void k_ransac_select(const TriView triples, int count, const int* __restrict__ counts, int ns, float confidence,
                                const int* __restrict__ state, int* __restrict__ plan, int* __restrict__ list) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    const int best = state[0], in_batch = plan[2], rest = ransac_rest(ns, plan[0]);
    bool keep = h < count && triples.valid(h) && rest > 0;
    if (keep) keep = ransac_keep(counts[h], rest, best, in_batch, ns, confidence);
    rb_append(keep, threadIdx.x & 63, h, list, &plan[1]);
}
// The two kernels above for a BOUNDED batch, in one launch over its live list (`live`, *n_live entries, in no order).  A dead
// hypothesis was never scored: its count is 0, which leaves the prefix maximum alone, and its leaf-box bound <= best drops it by
// rule (a).  So the largest prefix count of the live ones is the batch's (plan[2]), and the list is built from them under the same
// rules.  Phase 2's list holds the same hypotheses as k_ransac_select's,
// in another order: counts are integer atomics, the order does not matter.  One workgroup: the live list is an eighth of a batch.
// A NEAR hypothesis (RansacFarBound: `near`, *n_near entries, phase 1 over [c_far, plan[3])) has rest = the points behind its phase 1
// plus ubf[h], which bounds its inliers in the F chunks it skipped: prefix + rest still bounds its full count from above and the
// prefix is still a lower bound of it, so rules (a) and (b) hold as written.  Its survivors go to list2 (plan[4] of them).
// The register form of the two one-workgroup kernels (k_ransac_select_live, k_ransac_finish).  Both walk the live lists twice, and a
// trip of the loops is a chain of two dependent loads - live[i], then counts[live[i]] - that ends in a reduction, which keeps the
// trips apart: 7 trips x 2 round trips x 2 passes with the headline's 7,100 live hypotheses, on one workgroup.  So where the far and
// the near list together hold at most LIVE_MAX x 1,024 entries, thread t takes entries t, t + 1024, ... into registers at once: all the
// list loads back to back, then all the gathers, and both passes work from the registers.  Every load is unconditional - one under
// `if (i < n)` is an exec-masked block of its own with a full wait in front of it (icp.hip: acc_fetch): an entry past the end reads
// live[0], whatever it holds, and gathers counts[0]; `on` says which entries count.  Longer lists keep the loops.
// The fetch goes in rounds of LIVE_REG entries per thread, a round's loads in flight together; a round the lists do not reach
// (workgroup-uniform) is not fetched, so a batch of kRansacBatch - whose lists end inside the first - pays for one round as ever, and a
// grown batch's lists (14k entries at 131,072 hypotheses) take two.
#ifndef RS_LIVE_ROUNDS
#define RS_LIVE_ROUNDS 2     // tuning builds: 1 is the form of one round, 8,192 entries
#endif
constexpr int LIVE_REG = 8, LIVE_ROUNDS = RS_LIVE_ROUNDS, LIVE_MAX = LIVE_REG * LIVE_ROUNDS;
struct LiveRegs { int h[LIVE_MAX], c[LIVE_MAX], u[LIVE_MAX]; };     // hypothesis, its count, its UB_F (near entries; else not looked at)
__device__ __forceinline__ bool live_on(int e, int tot) { return (int)threadIdx.x + e * 1024 < tot; }
__device__ __forceinline__ bool live_is_near(int e, int n, int tot) { const int i = (int)threadIdx.x + e * 1024; return i >= n && i < tot; }
// far list `live` (n entries), near list `near` behind it (n2 entries; nullptr with n2 == 0); ubf == nullptr: no u[]
__device__ __forceinline__ void live_fetch(LiveRegs& L, const int* __restrict__ live, int n, const int* __restrict__ near, int n2,
                                           const int* __restrict__ counts, const int* __restrict__ ubf) {
    const int tot = n + n2;
#pragma unroll
    for (int r = 0; r < LIVE_ROUNDS; ++r) {
        const int e0 = r * LIVE_REG;
        if (r && e0 * 1024 >= tot) {                                 // (workgroup-uniform) nothing reaches this round: its entries are off
#pragma unroll
            for (int e = e0; e < e0 + LIVE_REG; ++e) { L.h[e] = 0; L.c[e] = 0; L.u[e] = 0; }
            continue;
        }
#pragma unroll
        for (int e = e0; e < e0 + LIVE_REG; ++e) {
            const int i = (int)threadIdx.x + e * 1024;
            L.h[e] = *(live_is_near(e, n, tot) ? near + (i - n) : live + (i < n ? i : 0));
        }
#pragma unroll
        for (int e = e0; e < e0 + LIVE_REG; ++e) L.c[e] = counts[live_on(e, tot) ? L.h[e] : 0];
        if (ubf) {
#pragma unroll
            for (int e = e0; e < e0 + LIVE_REG; ++e) L.u[e] = *(live_is_near(e, n, tot) ? ubf + L.h[e] : counts);
        }
    }
}
__global__ __launch_bounds__(1024)
void k_ransac_select_live(const int* __restrict__ live, const int* __restrict__ n_live, const int* __restrict__ near, const int* __restrict__ n_near,
                          const int* __restrict__ ubf, const int* __restrict__ counts, int ns, float confidence,
                          const int* __restrict__ state, int* __restrict__ plan, int* __restrict__ list, int* __restrict__ list2) {
    const int n = *n_live, n2 = near ? *n_near : 0, best = state[0], rest = ransac_rest(ns, plan[0]), rest2 = ransac_rest(ns, plan[3]);
    const int tot = n + n2;
    const bool in_regs = tot <= LIVE_MAX * 1024;                     // (workgroup-uniform)
    __shared__ int s_max, s_n[2];
    if (threadIdx.x == 0) { s_max = 0; s_n[0] = 0; s_n[1] = 0; }
    __syncthreads();
    int c = 0;
    LiveRegs L;
    if (in_regs) {
        live_fetch(L, live, n, near, n2, counts, near ? ubf : nullptr);
#pragma unroll
        for (int e = 0; e < LIVE_MAX; ++e) c = max(c, live_on(e, tot) ? L.c[e] : 0);
    } else
        for (int i = threadIdx.x; i < tot; i += 1024) c = max(c, counts[i < n ? live[i] : near[i - n]]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c = max(c, __shfl_xor(c, off, 64));
    if ((threadIdx.x & 63) == 0 && c > 0) atomicMax(&s_max, c);
    __syncthreads();
    const int in_batch = s_max, lane = threadIdx.x & 63;
    if (in_regs) {
        // no load from here on.  A wave's 64 entries may hold the far list's end and the near list's start: one ballot per list.
#pragma unroll
        for (int e = 0; e < LIVE_MAX; ++e) {
            // (workgroup-uniform: every lane reaches the ballots.  `continue`, not `break`: with a way out of it the compiler does
            // not unroll this loop, and L, indexed by a loop variable then, goes to scratch)
            if (e * 1024 >= tot) continue;
            const bool is_near = live_is_near(e, n, tot);
            const int r = is_near ? rest2 + L.u[e] : rest;
            const bool keep = live_on(e, tot) && r > 0 && ransac_keep(L.c[e], r, best, in_batch, ns, confidence);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const bool mine = keep && is_near == (k == 1);
                const unsigned long long m = __ballot(mine);
                if (m) {
                    int at = 0;
                    if (lane == 0) at = atomicAdd(&s_n[k], __popcll(m));
                    at = __shfl(at, 0, 64);
                    if (mine) (k ? list2 : list)[at + __popcll(m & ((1ull << lane) - 1ull))] = L.h[e];
                }
            }
        }
    } else
    for (int k = 0; k < 2; ++k) {                                    // the far list, then the near one
        const int* const from = k ? near : live; int* const to = k ? list2 : list;
        const int nk = k ? n2 : n;
        for (int i0 = 0; i0 < nk; i0 += 1024) {                      // (workgroup-uniform trip count: every lane reaches the ballot)
            const int i = i0 + threadIdx.x;
            bool keep = i < nk;
            int h = 0;
            if (keep) {
                h = from[i];
                const int r = k ? rest2 + ubf[h] : rest;
                keep = r > 0 && ransac_keep(counts[h], r, best, in_batch, ns, confidence);
            }
            const unsigned long long m = __ballot(keep);
            if (!m) continue;
            int at = 0;
            if (lane == 0) at = atomicAdd(&s_n[k], __popcll(m));
            at = __shfl(at, 0, 64);
            if (keep) to[at + __popcll(m & ((1ull << lane) - 1ull))] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { plan[1] = s_n[0]; plan[2] = in_batch; plan[4] = s_n[1]; }
}

// RansacPointOrder - the order of the scored points.  An inlier count does not depend on the order its points are scored in, and pq2
// alone fixes that order (the triples index pq, the rmse pass sums over pq, the leaf summary has its Morton order).  The bail-out
// drops a hypothesis whose count over the prefix plus ALL the remaining points cannot exceed the best; in the natural order a
// good-but-not-best pose (an eighth of the triples where half of the correspondences are true) collects a third of the prefix and
// is scored to the end.  So once per call, after the first batch has set a best, pq2 is written again from pq: the points the
// running best (d->best12) calls outliers first, its inliers behind them, both in their original relative order; the padding
// [ns, ns_pad) stays where k_pack_pq2 put it.  Those outliers are mostly the false correspondences, outliers of every good pose: a
// good pose collects next to nothing over the first N - best points and has to match the best inlier for inlier from there on.
// The plan, the lists, the rules of k_ransac_select and the scoring kernels see positions only and keep their shape.
// A stable partition without atomics on positions, so that two calls give the same pq2 and the same scored share:
//   k_order_flags    per block of RO_BLOCK points the ballot words of "outlier of the best" and their count.  The reference's test
//                    (ref_pair_d2, as the exact kernel), negated: a NaN is an outlier.  No best yet (state[0] == 0): all are.
//   k_order_scatter  a block adds up the counts in front of it and all of them (integers: any order), then every point goes to its
//                    slot of pq2's pair-interleaved layout.
// (Two launches, not the flags / scan / scatter of icp.hip: every block of the scatter re-reads all block counts, blocks^2 / 256 loads per
// thread in total - 782 blocks at 200k points, 11 us for both launches; 7,800 blocks and 6e7 cached loads at 2M points, where a
// call's batches take milliseconds each.  A scan launch of its own pays from some 10M points on, which no caller has.)
// Stream order puts the first batch's dispatches, which read pq2, in front of the two launches, and the second batch's behind.
// Three classes (RansacFarBound, far != nullptr): the outliers split into F and M (see RansacFar), in the order [F | M | I], each class
// in its original relative order, by the same scan over two ballot words per wave.  k_order_flags also keeps the ordering pose and
// adds the F pairs to the count table's bins (one LDS histogram per block, its non-empty bins added to the table by integer atomics:
// any order gives the same table); block 0 of k_order_scatter writes the class sizes and the table's running sums.
// far == nullptr (TDV_RANSAC_ORDER=1): the two-way order, no F.
constexpr int RO_BLOCK = 256;
__global__ __launch_bounds__(RO_BLOCK)
void k_order_flags(const float* __restrict__ pq, int ns, const int* __restrict__ state, const float* __restrict__ best12, float tau,
                   unsigned long long* __restrict__ mask, int* __restrict__ cnt, RansacFar* __restrict__ far, float rF2) {
    const int i = blockIdx.x * RO_BLOCK + threadIdx.x, n_words = (int)gridDim.x * (RO_BLOCK / 64);
    __shared__ int s_w[2][RO_BLOCK / 64];
    __shared__ unsigned s_hist[RF_BINS];
    if (far) {
        for (int b = threadIdx.x; b < RF_BINS; b += RO_BLOCK) s_hist[b] = 0u;
        if (blockIdx.x == 0 && threadIdx.x < 12) far->ord12[threadIdx.x] = best12[threadIdx.x];
        __syncthreads();
    }
    bool out = false, is_far = false;
    if (i < ns) {
        out = true;
        if (state[0] != 0) {
            const float* g = pq + (size_t)i * 8;
            v2f r[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) r[e] = (v2f){best12[e], best12[e]};
            const Pair2 a{{g[0], g[0]}, {g[1], g[1]}, {g[2], g[2]}, {g[3], g[3]}, {g[4], g[4]}, {g[5], g[5]}};
            const float d2 = ref_pair_d2(r, a).x;
            out = !(d2 < tau);
            if (far) {
                bool finite = true;
#pragma unroll
                for (int c = 0; c < 6; ++c) finite &= fabsf(g[c]) <= FLT_MAX;
                is_far = out && finite && d2 >= rF2;               // (a NaN d2 compares false: M)
                if (is_far) atomicAdd(&s_hist[rf_bin(d2)], 1u);
            }
        }
    }
    const unsigned long long m = __ballot(out), mf = __ballot(is_far);
    if ((threadIdx.x & 63) == 0) {      // (mask: RO_BLOCK / 64 words per block of the grid, the F words behind the outlier words)
        mask[i >> 6] = m; s_w[0][threadIdx.x >> 6] = __popcll(m);
        if (far) { mask[n_words + (i >> 6)] = mf; s_w[1][threadIdx.x >> 6] = __popcll(mf); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0, cf = 0;
        for (int w = 0; w < RO_BLOCK / 64; ++w) { c += s_w[0][w]; if (far) cf += s_w[1][w]; }
        cnt[blockIdx.x] = c;
        if (far) cnt[gridDim.x + blockIdx.x] = cf;
    }
    if (far)
        for (int b = threadIdx.x; b < RF_BINS; b += RO_BLOCK) { const unsigned v = s_hist[b]; if (v) atomicAdd(&far->hist[b], v); }
}
__global__ __launch_bounds__(RO_BLOCK)
void k_order_scatter(const float* __restrict__ pq, int ns, const unsigned long long* __restrict__ mask, const int* __restrict__ cnt,
                     float* __restrict__ pq2, RansacFar* __restrict__ far) {
    const int i = blockIdx.x * RO_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_words = (int)gridDim.x * (RO_BLOCK / 64);
    __shared__ int s_before[2][RO_BLOCK / 64], s_all[2][RO_BLOCK / 64], s_w[2][RO_BLOCK / 64];
    int before = 0, all = 0, fbefore = 0, fall = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += RO_BLOCK) {
        const int c = cnt[b]; all += c; if (b < (int)blockIdx.x) before += c;
        if (far) { const int f = cnt[gridDim.x + b]; fall += f; if (b < (int)blockIdx.x) fbefore += f; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        before += __shfl_xor(before, off, 64); all += __shfl_xor(all, off, 64);
        fbefore += __shfl_xor(fbefore, off, 64); fall += __shfl_xor(fall, off, 64);
    }
    const unsigned long long m = mask[i >> 6], mf = far ? mask[n_words + (i >> 6)] : 0ull;
    if (lane == 0) {
        s_before[0][wave] = before; s_all[0][wave] = all; s_w[0][wave] = __popcll(m);
        s_before[1][wave] = fbefore; s_all[1][wave] = fall; s_w[1][wave] = __popcll(mf);
    }
    __syncthreads();
    int out_before = 0, out_all = 0, rank = __popcll(m & ((1ull << lane) - 1ull));      // rank: the block's outliers in front of this point
    int far_before = 0, far_all = 0, frank = __popcll(mf & ((1ull << lane) - 1ull));    // ... and its F pairs
    for (int w = 0; w < RO_BLOCK / 64; ++w) {
        out_before += s_before[0][w]; out_all += s_all[0][w]; if (w < wave) rank += s_w[0][w];
        far_before += s_before[1][w]; far_all += s_all[1][w]; if (w < wave) frank += s_w[1][w];
    }
    if (far && blockIdx.x == 0) {        // the class sizes and the count table's running sums (workgroup-uniform branch)
        __shared__ unsigned s_part[RO_BLOCK];
        constexpr int PER = RF_BINS / RO_BLOCK;
        unsigned v[PER], sum = 0u;
#pragma unroll
        for (int e = 0; e < PER; ++e) { v[e] = far->hist[threadIdx.x * PER + e]; sum += v[e]; }
        s_part[threadIdx.x] = sum;
        __syncthreads();
        unsigned run = 0u;
        for (int t = 0; t < (int)threadIdx.x; ++t) run += s_part[t];
#pragma unroll
        for (int e = 0; e < PER; ++e) { run += v[e]; far->cum[threadIdx.x * PER + e] = run; }
        if (threadIdx.x == 0) { far->n_far = far_all; far->n_mid = out_all - far_all; far->c_far = far_all / RS_PCH; }
    }
    if (i >= ns) return;
    const bool out = (m >> lane) & 1ull, is_far = (mf >> lane) & 1ull;
    // F: [0, far_all) ; M: [far_all, out_all) ; inliers behind them: the points in front of this one that are no outliers
    const int pos = is_far ? far_before + frank
                  : out    ? far_all + (out_before + rank) - (far_before + frank)
                           : out_all + (i - out_before - rank);
    const float4 a = reinterpret_cast<const float4*>(pq)[2 * (size_t)i], b = reinterpret_cast<const float4*>(pq)[2 * (size_t)i + 1];
    float* o = pq2 + (size_t)(pos >> 1) * 12 + (pos & 1);
    o[0] = a.x; o[2] = a.y; o[4] = a.z; o[6] = a.w; o[8] = b.x; o[10] = b.y;
}

// RansacFinish - the end of a batch: the loop of registration.cpp:281-290 over the batch's counts in iteration order, on the device,
// as k_rb_select's two reductions: the first iteration whose fitness passes the confidence ends the loop (:290), and the first
// largest fitness up to it is the batch's candidate, a new best if it beats - strictly, in the float expression of :281 itself -
// the best of the earlier batches.  sel = { best fitness (bits), its count, its iteration, stopped } carries the loop's state from
// batch to batch on the device; once `stopped` is set the batches still in flight change nothing (the host discards them too).
// The winning hypothesis' 12 floats go to best12, and the host gets ONE record per batch - { best local index or -1, its count,
// local stop index or -1, bad correspondence flag } - where it used to download every count and walk them.  The same launch
// raises state[0] to the batch's largest full count, as k_ransac_best did (state == nullptr: a batch without bail-out), and
// adds a bounded batch's list lengths to the call's counters (lists != nullptr; a batch behind the loop's stop adds nothing).
// live != nullptr (a bounded batch, confidence >= 0): only the live lists - far and near - are read.  A dead hypothesis has count 0: no new best
// (strict > on a best fitness >= 0), no exit (0 > confidence is false), nothing to raise.
// One workgroup; the first batch and the live lists are a few thousand entries (a whole batch is walked only with the bound off).
// LISTS == false (live_in == nullptr: no lists) is the kernel without the register form - what a call without bail-out runs, whose
// path through the instance with it, 48 more registers' worth of code, measured 17 us per call longer (C4, profiles/r27 section 6).
template <bool LISTS>
__global__ __launch_bounds__(1024)
void k_ransac_finish(const TriView triples, int count, const int* __restrict__ counts, const int* __restrict__ live_in, const int* __restrict__ n_live,
                     const int* __restrict__ near, const int* __restrict__ n_near, const float* __restrict__ hyp, int h_pad, int ns, float confidence, int it0,
                     int* __restrict__ state, int* __restrict__ sel, float* __restrict__ best12, const int* __restrict__ bad, int* __restrict__ rec,
                     const int* __restrict__ lists, long long* __restrict__ bound, const int seq) {
    const int* const live = LISTS ? live_in : nullptr;
    const int n1 = live ? *n_live : count, n = n1 + (live && near ? *n_near : 0);      // (the near list behind the far one)
    const float fn = static_cast<float>((size_t)ns);
    __shared__ int s_stop, s_max;
    __shared__ unsigned long long s_best[16];
    if (threadIdx.x == 0) { s_stop = INT_MAX; s_max = 0; }
    __syncthreads();
    int stop = INT_MAX, cmax = 0;
    const bool in_regs = live && n <= LIVE_MAX * 1024;           // the register form (see live_fetch); workgroup-uniform
    LiveRegs L;
    if (in_regs) {
        live_fetch(L, live, n1, near, n - n1, counts, nullptr);
#pragma unroll
        for (int e = 0; e < LIVE_MAX; ++e) {
            if (!live_on(e, n)) continue;
            cmax = max(cmax, L.c[e]);
            if (static_cast<float>(L.c[e]) / fn > confidence) stop = min(stop, L.h[e]);
        }
    } else
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int h = live ? (i < n1 ? live[i] : near[i - n1]) : i;
        if (!live && !triples.valid(h)) continue;                // a skipped iteration (registration.cpp:240)
        const int c = counts[h];
        cmax = max(cmax, c);
        if (static_cast<float>(c) / fn > confidence) stop = min(stop, h);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { stop = min(stop, __shfl_xor(stop, off, 64)); cmax = max(cmax, __shfl_xor(cmax, off, 64)); }
    if ((threadIdx.x & 63) == 0) {
        if (stop != INT_MAX) atomicMin(&s_stop, stop);
        if (cmax > 0) atomicMax(&s_max, cmax);
    }
    __syncthreads();
    const int k_stop = s_stop;
    // the first largest fitness among the iterations up to k_stop (earlier = INT_MAX - h)
    unsigned long long best = 0ull;
    if (in_regs) {
#pragma unroll
        for (int e = 0; e < LIVE_MAX; ++e) {                     // from the registers: no load
            if (!live_on(e, n) || L.h[e] > k_stop) continue;
            const float fit = static_cast<float>(L.c[e]) / fn;   // registration.cpp:281
            if (!(fit > 0.f)) continue;
            const unsigned long long key = first_best_key(fit, INT_MAX - L.h[e]);
            best = key > best ? key : best;
        }
    } else
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int h = live ? (i < n1 ? live[i] : near[i - n1]) : i;
        if (h > k_stop || (!live && !triples.valid(h))) continue;
        const float fit = static_cast<float>(counts[h]) / fn;    // registration.cpp:281
        if (!(fit > 0.f)) continue;
        const unsigned long long key = first_best_key(fit, INT_MAX - h);
        best = key > best ? key : best;
    }
    best = first_best_wave(best);
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 16; ++w) best = s_best[w] > best ? s_best[w] : best;
    if (state && s_max > 0) atomicMax(state, s_max);
    int best_local = -1, best_count = 0, stop_local = -1;
    if (!sel[3]) {
        // RansacBoundLists' counters (lists: the bounded batch's words of RansacLive): hypotheses bounded, close, on the fine list, live
        if (lists) { bound[0] += count; bound[1] += lists[6]; bound[2] += lists[2]; bound[3] += lists[0] + lists[4]; }
        if (best != 0ull) {
            const int h = INT_MAX - (int)(unsigned)(best & 0xffffffffull);
            const float fit = __uint_as_float((unsigned)(best >> 32));
            if (fit > __int_as_float(sel[0])) {                  // registration.cpp:284
                best_local = h; best_count = counts[h];
                sel[0] = __float_as_int(fit); sel[1] = best_count; sel[2] = it0 + h;
                for (int e = 0; e < 12; ++e) best12[e] = hyp[(size_t)e * h_pad + h];
            }
        }
        if (k_stop != INT_MAX) { stop_local = k_stop; sel[3] = 1; }
    }
    rec[0] = best_local; rec[1] = best_count; rec[2] = stop_local; rec[3] = *bad;
    __threadfence_system();                                      // (the record may live in pinned host memory)
    // the batch's sequence number behind the record, the launch's last store: the host waits for this word instead of an event
    // (RansacRun::wait_batch; seq == 0: the batch ends with an event)
    // (relaxed: the fence above is the release, and a release store would write the L2 back a second time)
    if (seq) __hip_atomic_store(rec + 4, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------ RansacLeafBound
// Rule (a) above needs only an UPPER bound of a hypothesis' count.  The bail-out's bound is "every unscored point is an
// inlier"; this one is far tighter and costs a few percent of a full scoring.  Once per call the point pairs (p, q) are
// ordered along a 6-D Morton curve (5 bits per coordinate, the curve over the pairs' own bounding box) and cut into leaves
// of RL_LEAF pairs; a leaf keeps its p box (centre, half-extent), its q box (lo, hi) and its number of pairs.  Per batch,
// k_ransac_bound adds up, for each hypothesis, the sizes of the leaves whose boxes could hold an inlier: UB(h).  A hypothesis
// with UB(h) <= best count of the EARLIER batches is dead: it is not scored at all, its count stays 0, and k_ransac_select
// drops it like any other hypothesis of rule (a).  Only the summary is reordered: pq / pq2, the hypotheses, the scoring and
// the rmse pass keep the original order, so every count and every sum keeps its bits.
//
// Exactness.  A leaf fails only if g2 > Tb, g2 the squared length of the per-axis gaps between the interval R [pc - pe,
// pc + pe] + t and [qlo, qhi] evaluated in f32, Tb = (s + 3E)^2 (1 + 1e-6), s = sqrt(tau) rounded up, E = 16 u (A + s) the
// band of k_ransac_hypotheses (A = max over rows of (|r0| + |r1| + |r2|) P + |t|, P = the largest |source coordinate|).
//   (1) f32 evaluation of the bound.  xc = R pc + t and xe = |R| pe as FMA chains are within gamma_3 A of their real values
//       (|pc|, pe <= P), xc -+ xe one more rounding (<= 2 u A), the subtraction of qlo/qhi one relative rounding: each f32 gap
//       exceeds (1 + u) times (real gap + 8.1 u A), and |gap_f32| <= (1 + u) |gap| + 14.1 u A; the squared norm (three
//       roundings) adds a factor (1 + 2 u) in length.  So sqrt(g2) <= (1 + 3 u) G + 14.2 u A, G the real gap length - a lower
//       bound of |R p + t - q| for every pair of the leaf.  (Even with every operation unfused - were the compiler to split
//       the FMAs - the chains stay within gamma_4 and the total within 18 u A.)
//   (2) the reference's rounding.  d2_ref = fl((x_ref - qx)^2 + ...) with x_ref within gamma_4 A of the real value: in
//       distance sqrt(d2_ref) >= D (1 - 3 u) - 7 u A, D = |R p + t - q| (real).  D >= s + E therefore gives d2_ref >= s^2 >= tau.
// g2 > Tb gives sqrt(g2) > s + 3E, so G > (s + 3E - 18 u A) / (1 + 3 u) >= s + E (E >= 16 u A + 16 u s, E < s / 4): every
// pair of the leaf has D >= s + E and is no inlier in the reference arithmetic.  The margin (3E against the band's E) is at
// least as conservative as the band; tests/test_ransac_leaf_bound_margin.py checks (1) and (2) in emulated f32 on leaves
// whose boxes touch the threshold shell.  Where the band is off (non-finite data, coordinates far from the origin: E not
// below s / 4) the bound is off too: the hypothesis is live.  A leaf with any non-finite coordinate always passes.
constexpr int RL_LEAF = 32;          // pairs per leaf (the study: 32 prunes 11.7 % -> 15 % survivors at 64)
constexpr int RL_COARSE = 128;       // pairs per coarse leaf (4 fine leaves): the first of the bound's two levels, see k_ransac_bound
constexpr int RL_BITS = 5;           // Morton bits per coordinate (30-bit key)
__device__ __forceinline__ unsigned rl_enc(float f) { const unsigned b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }   // order-preserving
__device__ __forceinline__ float rl_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
// per-axis bounds of the finite coordinates of p and q: enc[0..5] = min (memset to 0xff), enc[6..11] = max (memset to 0)
__global__ __launch_bounds__(256)
void k_leaf_bounds(const float* __restrict__ pq, int ns, unsigned* __restrict__ enc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    __shared__ unsigned s_enc[12];
    if (threadIdx.x < 12) s_enc[threadIdx.x] = threadIdx.x < 6 ? 0xffffffffu : 0u;
    __syncthreads();
    unsigned lo[6], hi[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        lo[c] = 0xffffffffu; hi[c] = 0u;
        if (i < ns) {
            const float v = pq[(size_t)i * 8 + c];
            if (fabsf(v) <= FLT_MAX) { lo[c] = rl_enc(v); hi[c] = lo[c]; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo[c] = min(lo[c], (unsigned)__shfl_xor((int)lo[c], off, 64)); hi[c] = max(hi[c], (unsigned)__shfl_xor((int)hi[c], off, 64)); }
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < 6; ++c) { atomicMin(&s_enc[c], lo[c]); atomicMax(&s_enc[6 + c], hi[c]); }
    __syncthreads();
    if (threadIdx.x < 12) {
        const unsigned v = s_enc[threadIdx.x];
        if (threadIdx.x < 6) { if (v != 0xffffffffu) atomicMin(&enc[threadIdx.x], v); }
        else if (v != 0u) atomicMax(&enc[threadIdx.x], v);
    }
}
// 6-D Morton key of every pair (bit 6 b + c = bit b of coordinate c's cell); a non-finite coordinate takes cell 0.
// Class-major leaves (RansacBoundLists): bit RL_CLASS_BIT, above every Morton bit, is set for a pair that is no outlier of the
// ordering pose (`outlier`: k_order_flags' ballot words, indexed by the original pair), so the sorted order is the pose's outliers
// first and its inliers behind them, as k_order_scatter orders pq2, each class along its own Morton curve.  The inliers are true
// pairs on a 3-D sheet of the 6-D space, the outliers mostly random pairs: leaves cut class by class have tighter boxes than leaves
// that mix the two.  In the product library `outlier` is nullptr: the classes are off, and only the study build's
// TDV_RANSAC_LEAF_CLASSES=1 passes the words (see ransac_knobs).  nullptr, TDV_RANSAC_ORDER=0 and a call without a best (every
// word all ones) give class 0 everywhere: the plain Morton order.  Exactness needs no new argument: RansacLeafBound's proof is per leaf - a leaf's boxes hold its pairs,
// whatever the grouping, and a leaf that straddles the class boundary is merely loose - and a coarse leaf is still the union of 4
// consecutive fine leaves of the same sorted order, so "coarse-dead implies fine-dead" holds with its 5 E margin unchanged.
constexpr int RL_CLASS_BIT = 6 * RL_BITS;
__global__ __launch_bounds__(256)
void k_leaf_keys(const float* __restrict__ pq, int ns, const unsigned* __restrict__ enc, const unsigned long long* __restrict__ outlier,
                 unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    unsigned key = (outlier && !((outlier[i >> 6] >> (i & 63)) & 1ull)) ? 1u << RL_CLASS_BIT : 0u;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const float lo = rl_dec(enc[c]), hi = rl_dec(enc[6 + c]);
        const float v = pq[(size_t)i * 8 + c];
        int cell = 0;
        if (fabsf(v) <= FLT_MAX && hi > lo) cell = min(max((int)((v - lo) * ((float)(1 << RL_BITS) / (hi - lo))), 0), (1 << RL_BITS) - 1);
#pragma unroll
        for (int b = 0; b < RL_BITS; ++b) key |= (unsigned)((cell >> b) & 1) << (6 * b + c);
    }
    keys[i] = key; vals[i] = (unsigned)i;
}
// One leaf per RL_LEAF sorted pairs, 16 values {pc, n, pe, 0, qlo, 0, qhi, 0}, stored in PAIRS of leaves with the two leaves'
// values interleaved (value v of leaf 2k + j at [32 k + 2 v + j]) so that k_ransac_bound reads aligned SGPR pairs for its packed
// instructions; the buffer is zeroed first, so an odd last leaf is paired with an empty one (n = 0).  A leaf with a non-finite
// coordinate gets pc = pe = 0 and the q box (-inf, inf): it passes for every finite hypothesis.
// The same launch writes the COARSE leaves (RL_COARSE pairs each: the RL_COARSE / RL_LEAF consecutive fine leaves of one coarse
// leaf, same sorted order) to `coarse`, in the same layout and by the same rules: the min / max over its pairs are the min / max
// of its fine leaves' (exact), pc and pe follow from them as for a fine leaf.
__device__ __forceinline__ void rl_leaf_store(float* o, int n, bool bad, const float* lo, const float* hi) {
    o[6] = (float)n;
    if (bad) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[2 * c] = 0.f; o[8 + 2 * c] = 0.f; o[16 + 2 * c] = -INFINITY; o[24 + 2 * c] = INFINITY; }
        return;
    }
    float pc[3], pe[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pc[c] = 0.5f * lo[c] + 0.5f * hi[c];
        // half-extent rounded up past the exact max(hi - pc, pc - lo): every p of the leaf lies in [pc - pe, pc + pe]
        const double d = fmax((double)hi[c] - (double)pc[c], (double)pc[c] - (double)lo[c]);
        pe[c] = nextafterf((float)d, INFINITY);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[2 * c] = pc[c]; o[8 + 2 * c] = pe[c]; o[16 + 2 * c] = lo[3 + c]; o[24 + 2 * c] = hi[3 + c]; }
}
__global__ __launch_bounds__(256)
void k_leaf_build(const float* __restrict__ pq, int ns, const unsigned* __restrict__ order, float* __restrict__ leaves, float* __restrict__ coarse) {
    const int i = blockIdx.x * 256 + threadIdx.x;     // sorted position; the grid covers whole leaves (and so whole coarse leaves)
    float lo[6], hi[6];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
    if (i < ns) {
        const float* g = pq + (size_t)order[i] * 8;
#pragma unroll
        for (int c = 0; c < 6; ++c) { const float v = g[c]; lo[c] = v; hi[c] = v; bad |= !(fabsf(v) <= FLT_MAX); }
    }
#pragma unroll
    for (int off = RL_LEAF / 2; off > 0; off >>= 1) {        // within the leaf's 32 lanes (half a wave)
#pragma unroll
        for (int c = 0; c < 6; ++c) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], off, 64)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off, 64)); }
        bad |= __shfl_xor((int)bad, off, 64) != 0;
    }
    constexpr int FINE = 256 / RL_LEAF, PER = RL_COARSE / RL_LEAF;          // fine leaves per workgroup, per coarse leaf
    __shared__ float s_lo[FINE][6], s_hi[FINE][6];
    __shared__ int s_bad[FINE];
    const int f = threadIdx.x / RL_LEAF;
    if (!(threadIdx.x & (RL_LEAF - 1))) {
#pragma unroll
        for (int c = 0; c < 6; ++c) { s_lo[f][c] = lo[c]; s_hi[f][c] = hi[c]; }
        s_bad[f] = bad;
        if (i < ns) {
            const int leaf = i / RL_LEAF;
            rl_leaf_store(leaves + (size_t)(leaf >> 1) * 32 + (leaf & 1), min(RL_LEAF, ns - i), bad, lo, hi);
        }
    }
    __syncthreads();
    const int k = threadIdx.x;                                             // coarse leaf of this workgroup
    const int i0 = blockIdx.x * 256 + k * RL_COARSE;
    if (k >= 256 / RL_COARSE || i0 >= ns) return;
    float clo[6], chi[6];
    bool cbad = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) { clo[c] = INFINITY; chi[c] = -INFINITY; }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
#pragma unroll
        for (int c = 0; c < 6; ++c) { clo[c] = fminf(clo[c], s_lo[k * PER + j][c]); chi[c] = fmaxf(chi[c], s_hi[k * PER + j][c]); }
        cbad |= s_bad[k * PER + j] != 0;
    }
    const int leaf = i0 / RL_COARSE;
    rl_leaf_store(coarse + (size_t)(leaf >> 1) * 32 + (leaf & 1), min(RL_COARSE, ns - i0), cbad, clo, chi);
}
// A workgroup per 64 hypotheses (lane = hypothesis), its RB_SPLIT waves walking RB_SPLIT ranges of the leaf pairs; leaf values are
// wave-uniform (scalar loads), two leaves per packed instruction.  A lane stops adding once its partial bound exceeds the best count
// of the earlier batches (the hypothesis cannot be proven dead on these leaves then: the whole bound can only be larger); a wave
// stops when every lane has, so where nothing can be pruned the pass ends early by itself.  The partial bounds meet in LDS.
// (One lane per hypothesis walking all the leaves alone gives one wave per SIMD for a 65,536-hypothesis batch, every scalar load's
// latency exposed.)
// Two levels (round 6).  88 % of the hypotheses are dead, and a dead one walks every leaf.  The coarse leaves (RL_COARSE pairs,
// each the union of 4 fine leaves) already prove 81 % of them dead at a quarter of the leaf tests, so the bound runs twice:
//   RB_COARSE   every hypothesis of the batch over the coarse leaves.  Coarse sum <= best: dead.  No band or the gate closed: live.
//               The rest is undecided and appended to `und` (*n_und of them, zeroed by ransac_plan).
//   k_ransac_bound_fine   the undecided hypotheses over the fine leaves: the one-level walk, early stop included; dead or live.
// A fine leaf's pairs lie inside its coarse leaf's boxes, so in real arithmetic a coarse leaf that fails has children that all
// fail, the coarse sum is >= the fine sum and coarse-dead implies fine-dead.  In f32 the two tests round differently (other pc,
// pe; a fine box's rounded-up pe may poke an ulp past its parent's): so the coarse test fails a leaf only on g2 > (s + 5 E)^2,
// not 3 E.  By (1) below, run both ways, a coarse f32 gap above s + 5 E puts every child's f32 gap above s + 5 E - 2 (14.2 u A +
// 3 u (s + 5 E)) - 2 u A > s + 3 E (E >= 16 u (A + s)): every child fails its own test too.  Each coarse level verdict is thus
// the fine walk's, and the live list is exactly the one-level walk's (RB_ONE, kept for the study build's A/B:
// TDV_RANSAC_BOUND_LEVELS=1; tests/test_ransac_leaf_bound_two_levels.py checks the implication in emulated f32).
// Live hypotheses are appended to `live` (*n_live of them, zeroed by ransac_plan); a dead one leaves no trace: it is on no list.
constexpr int RB_SPLIT = 16;
enum { RB_ONE = 0, RB_COARSE = 1 };
// One wave's share [k0, k1) of the leaf pairs for its lane's hypothesis (r: column-major R, t): the sizes of the leaves that
// may hold an inlier, added until the sum exceeds `best` (done).  tb = (s + margin E)^2 (1 + 1e-6).
// LeafPtr: const float*, or - k_ransac_bound_fine - the same address in the constant address space (RbConstLeaves).
typedef const float __attribute__((address_space(4)))* RbConstLeaves;
template <typename LeafPtr>
__device__ __forceinline__ int rb_walk(const float* r, const LeafPtr leaves, int k0, int k1, float tb, int best, bool done) {
    int ub = 0;
    v2f rr[12], ar[9];
#pragma unroll
    for (int e = 0; e < 12; ++e) rr[e] = (v2f){r[e], r[e]};
#pragma unroll
    for (int e = 0; e < 9; ++e) ar[e] = (v2f){fabsf(r[e]), fabsf(r[e])};
    for (int k = k0; k < k1; ++k) {
        if (((k - k0) & 7) == 0 && !__any(!done)) break;
        const LeafPtr g = leaves + (size_t)k * 32;
        float v[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = g[e];
        const v2f pcx = {v[0], v[1]}, pcy = {v[2], v[3]}, pcz = {v[4], v[5]};
        const v2f pex = {v[8], v[9]}, pey = {v[10], v[11]}, pez = {v[12], v[13]};
        v2f g2 = {0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const v2f xc = fma2(rr[c], pcx, fma2(rr[3 + c], pcy, fma2(rr[6 + c], pcz, rr[9 + c])));
            const v2f xe = fma2(ar[c], pex, fma2(ar[3 + c], pey, ar[6 + c] * pez));
            const v2f qlo = {v[16 + 2 * c], v[17 + 2 * c]}, qhi = {v[24 + 2 * c], v[25 + 2 * c]};
            const v2f lo_gap = (xc - xe) - qhi, hi_gap = qlo - (xc + xe);
            const v2f gp = {fmaxf(fmaxf(lo_gap.x, hi_gap.x), 0.f), fmaxf(fmaxf(lo_gap.y, hi_gap.y), 0.f)};
            g2 = fma2(gp, gp, g2);
        }
        // a leaf fails only on g2 > tb; NaN passes
        const int n2 = (!(g2.x > tb) ? (int)v[6] : 0) + (!(g2.y > tb) ? (int)v[7] : 0);
        if (!done) { ub += n2; done = ub > best; }
    }
    return ub;
}
// The hypothesis' band test and its bound threshold (k_ransac_hypotheses' E, from the same f32 operations)
struct RbHyp { float r[12]; float tb, E; bool bounded; };
__device__ __forceinline__ float rb_band(const float* r, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u) {
    return (band_u * ransac_band_reach(r, __uint_as_float(*pmax)) + band_u * sqrt_tau) * 1.0001f;
}
__device__ __forceinline__ void rb_make(RbHyp& o, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u, float margin);
__device__ __forceinline__ RbHyp rb_load(const float* __restrict__ hyp, int h_pad, int h, bool valid, const unsigned* __restrict__ pmax,
                                         float sqrt_tau, float band_u, float margin) {
    RbHyp o;
#pragma unroll
    for (int e = 0; e < 12; ++e) o.r[e] = valid ? hyp[(size_t)e * h_pad + h] : 0.f;
    rb_make(o, pmax, sqrt_tau, band_u, margin);
    return o;
}
__device__ __forceinline__ void rb_make(RbHyp& o, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u, float margin) {      // o.r is set
    const float E = rb_band(o.r, pmax, sqrt_tau, band_u);
    o.bounded = E < 0.25f * sqrt_tau;                             // false for NaN (non-finite data or hypothesis)
    o.E = E;
    const float sb = sqrt_tau + margin * E;
    o.tb = sb * sb * (1.0f + 1e-6f);
}
// ------------------------------------------------------------------ RansacFarBound
// Almost every hypothesis the leaf bound leaves alive is a near-perfect pose, and almost none of the ordering pose B's far outliers
// (F of RansacFar) lies near its match under any such pose.  With Delta_h = max over the 8 corners c of the finite sources' bounding
// box of |(R_h - R_B) c + (t_h - t_B)| - the displacement between the two poses is affine in the point and its norm convex, so the
// corner maximum is the maximum over the box, which holds the source of every F pair - the triangle inequality gives
// D_h(i) >= D_B(i) - Delta_h for D = |R p + t - q| in real arithmetic.  So only the F pairs with D_B < s + Delta_h can be inliers of
// h, and the count table bounds their number: UB_F(h).  A live hypothesis whose UB_F is small goes on the batch's NEAR list: its
// phase 1 skips the chunks wholly inside F (a chunk that straddles F's end is scored; its F pairs may be counted in UB_F as well,
// which only loosens a valid bound), k_ransac_select_live adds UB_F(h) to its rest, and if it survives phase 2 scores the skipped
// chunks too: a survivor's count is exact, a dropped one's partial, as for every other hypothesis of RansacPlan.
//
// Exactness, with u = 2^-24, A_h, A_B the poses' reaches (ransac_band_reach) and E = 16 u (A + s) their bands, both below s / 4 - with
// either band off the hypothesis is far.  An F pair that UB_F(h) does not count has d2_B >= T in the reference arithmetic (the table
// errs upward), T = ((s + Delta_f + 3 (E_h + E_B)) (1 + 4e-6))^2 (1 + 1e-6) in f32, Delta_f the f32 value of Delta_h.
//   (1) Delta_f.  R_h - R_B and t_h - t_B round once each (<= u (|R_h| + |R_B|) per entry), the FMA chain over |c| <= P is within
//       gamma_3 of its real value: per component within 5 u (A_h + A_B), in length 8.7 u (A_h + A_B); the squared norm and the
//       square root add a factor (1 + 3 u).  Delta_h <= (1 + 3 u) Delta_f + 9 u (A_h + A_B).
//   (2) the reference's rounding (RansacLeafBound's (2), both ways): sqrt(d2_ref) <= (1 + 3 u) D + 7 u A and, for h,
//       D_h >= s + E_h gives d2_ref >= tau.
//   sqrt(T) in real arithmetic is at least (s + Delta_f + 3 (E_h + E_B)) (1 + 4e-6) (1 - 4 u) (the sum's and the products' roundings),
//   so D_B >= (sqrt(T) - 7 u A_B) / (1 + 3 u) >= (s + Delta_f + 3 (E_h + E_B)) (1 + 4e-6 - 8 u) - 7 u A_B, and with
//   4e-6 > 11 u, 16 u A <= E:  D_B >= s + (1 + 3 u) Delta_f + 3 (E_h + E_B) - 0.5 E_B >= s + Delta_h + 2.4 E_h + 1.9 E_B
//   > s + Delta_h + E_h.  Hence D_h >= s + E_h: the pair is no inlier of h in the reference arithmetic.  The margin 3 (E_h + E_B) is
//   RansacLeafBound's 3 E for two poses; tests/test_ransac_far_bound_margin.py checks the chain in emulated f32 on the shell.
// A box with no finite source decodes to NaN corners, a non-finite pose gives a NaN Delta: T is then no finite number and the
// hypothesis is far.
// Delta^2 between the poses r and ref (column-major R, then t): the largest squared displacement |(R - R_ref) c + (t - t_ref)|^2 over
// the 8 corners c of the finite sources' bounding box (enc).  A NaN stays.
__device__ __forceinline__ float rf_corner_max2(const float* r, const float* ref, const unsigned* __restrict__ enc) {
    float d[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) d[e] = r[e] - ref[e];
    float lo[3], hi[3], m2 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = rl_dec(enc[c]); hi[c] = rl_dec(enc[6 + c]); }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float x = (k & 1) ? hi[0] : lo[0], y = (k & 2) ? hi[1] : lo[1], z = (k & 4) ? hi[2] : lo[2];
        float n2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = fmaf(d[c], x, fmaf(d[3 + c], y, fmaf(d[6 + c], z, d[9 + c]))); n2 = fmaf(v, v, n2); }
        m2 = (n2 > m2 || n2 != n2) ? n2 : m2;                                // (a NaN stays)
    }
    return m2;
}
// Whether the hypothesis o, if live, goes on the near list; ub_f = UB_F(h) then.  best = the best count of the earlier batches.
// f.far == nullptr: every live hypothesis is far.
__device__ __forceinline__ bool rf_near(const RbHyp& o, const PreJob& f, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u, int best, int& ub_f) {
    if (!f.far || !o.bounded || f.far->c_far < 1) return false;              // (no band; skipping F saves less than a chunk)
    float b[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) b[e] = f.far->ord12[e];
    const float E_B = rb_band(b, pmax, sqrt_tau, band_u);
    if (!(E_B < 0.25f * sqrt_tau)) return false;                             // the ordering pose's band is off
    const float m2 = rf_corner_max2(o.r, b, f.enc);
    const float sb = (sqrt_tau + sqrtf(m2) + 3.f * (o.E + E_B)) * (1.0f + 4e-6f), T = sb * sb * (1.0f + 1e-6f);
    if (!(T <= FLT_MAX)) return false;
    ub_f = (int)f.far->cum[rf_bin(T)];
    return ub_f <= (int)((long long)best * f.u_cut_permille / 1000);
}
// ------------------------------------------------------------------ RansacBoundLists
// More than half of the hypotheses the coarse level leaves undecided end up live anyway: they are near-copies of the running best B
// (d->best12), a few thresholds from it everywhere on the cloud, and the fine level walks every leaf for each of them only to say
// so.  Putting a hypothesis on a live list needs no proof - only a dead verdict does: a live hypothesis is scored, and
// k_ransac_select_live drops it by its count like any other.  So a hypothesis that is CLOSE to B goes live without a verdict of the
// walk: live = close OR the walk's verdict, in the one-level walk and in the coarse level alike; a close hypothesis is never put on
// the undecided list, whatever its coarse sum.  Close: valid, its band on, the gate open, B's own band on (E_B < s / 4, as in
// rf_near), and Delta_h = rf_corner_max2 against B finite with sqrtf(Delta_h^2) <= radius * s (radius in thresholds: 20, measured
// above 13 and 9 in every run - a wrongly live hypothesis costs about three fine walks, profiles/r14/ransac_bound_lists.md).  The rule reads
// the running best, which every batch's k_ransac_finish writes in stream order: it depends neither on the point order nor on the
// far bound nor on the number of levels, and two calls give the same lists.
// Both judgements - close to B, near under the ordering pose - need the pose and a few words that are fixed once the batch is
// enqueued (best12, state[0], the ordering pose, the box, the count table), not the walk: k_ransac_hypotheses makes them for every
// hypothesis where it has the pose in registers (ransac_prejudge: flags[h], ubf[h]), and the bound kernels' tails read one word.
// (Made in wave 0's tail behind the walk they cost the coarse level 28 us per batch: four dependent trips to memory during which
// the workgroup's other 15 waves are gone and its slots cannot be given away.)
enum { RB_CLOSE = 1, RB_NEAR = 2 };
__device__ __forceinline__ bool rb_gate(int best, int ns) { return best >= ns / 32; }      // the walk's gate, see k_ransac_bound
__device__ __forceinline__ bool rb_close(const RbHyp& o, const PreJob& j, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u) {
    if (!(j.live_radius > 0.f)) return false;
    float b[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) b[e] = j.best12[e];
    if (!(rb_band(b, pmax, sqrt_tau, band_u) < 0.25f * sqrt_tau)) return false;      // the best pose's band is off
    const float m2 = rf_corner_max2(o.r, b, j.enc);
    return m2 <= FLT_MAX && sqrtf(m2) <= j.live_radius * sqrt_tau;                   // (false for NaN)
}
__device__ __forceinline__ void ransac_prejudge(const PreJob& j, const float* r, bool valid, int h, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u,
                                                const int* __restrict__ state, int ns) {
    RbHyp o;
#pragma unroll
    for (int e = 0; e < 12; ++e) o.r[e] = valid ? r[e] : 0.f;
    rb_make(o, pmax, sqrt_tau, band_u, 3.f);
    const int best = state[0];
    int ub_f = 0;
    const bool close = valid && o.bounded && rb_gate(best, ns) && rb_close(o, j, pmax, sqrt_tau, band_u);
    const bool near = valid && rf_near(o, j, pmax, sqrt_tau, band_u, best, ub_f);
    j.flags[h] = (close ? RB_CLOSE : 0) | (near ? RB_NEAR : 0);
    if (near) j.ubf[h] = ub_f;
}
// A tail's appends - the far list, the near list, the undecided list - reserved by ONE vector atomic (lane k for list k: one trip to
// memory, not three); returns the lane's slot on the undecided list.  near / und are false where their list is nullptr.
struct ListJob { const int* flags; int* near; int* n_near; int* n_close; };      // near == nullptr: every live hypothesis is far
__device__ __forceinline__ int rb_append3(bool far, bool near, bool und, int lane, int h, int* __restrict__ live, int* __restrict__ n_live,
                                          int* __restrict__ nearl, int* __restrict__ n_near, int* __restrict__ undl, int* __restrict__ n_und) {
    const unsigned long long m0 = __ballot(far), m1 = __ballot(near), m2 = __ballot(und);
    if (!(m0 | m1 | m2)) return 0;
    int at = 0;
    if (lane < 3) {
        const unsigned long long m = lane == 0 ? m0 : lane == 1 ? m1 : m2;
        int* const n = lane == 0 ? n_live : lane == 1 ? n_near : n_und;
        if (m) at = atomicAdd(n, __popcll(m));
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const int a0 = __shfl(at, 0, 64) + __popcll(m0 & below), a1 = __shfl(at, 1, 64) + __popcll(m1 & below), a2 = __shfl(at, 2, 64) + __popcll(m2 & below);
    if (far) live[a0] = h;
    if (near) nearl[a1] = h;
    if (und) undl[a2] = h;
    return a2;
}
// RansacStage (round 30).  A batch's triples are drawn by the host into pinned memory, and k_ransac_hypotheses - every lane's pose
// hangs behind its triple - read them from there at the link's rate.  They depend on nothing the device computes, so the host
// draws a batch further ahead and the coarse level of batch n, which is bound by its arithmetic, carries batch n + 1's triples
// across: thread i of its grid loads word i of the pinned slot in front of the walk and stores it to batch n + 1's device buffer
// behind it, and batch n + 1's k_ransac_hypotheses reads the device copy (up == nullptr).  The carrier is an instance of its own
// (STAGE, cnt >= 1): a coarse level with nothing to carry - the last batch's, a call that does not stage - runs the kernel as it was.
// Packed triples only (one word each); see RansacRun::loop for who stages and for the hazards.
struct StageJob { const uint64_t* src; uint64_t* dst; int cnt; };
// RB_ONE / RB_COARSE: a workgroup per 64 hypotheses of the batch.  RB_COARSE also zeroes the fine level's per-slot sums (acc) of
// the hypotheses it leaves undecided and the ticket of its slot block.
template <int MODE, bool STAGE = false>
__global__ __launch_bounds__(64 * RB_SPLIT)
void k_ransac_bound(const float* __restrict__ hyp, int h_pad, const TriView triples, int count, const float* __restrict__ leaves, int n_lpairs,
                    const unsigned* __restrict__ pmax, float sqrt_tau, float band_u, const int* __restrict__ state, int ns,
                    int* __restrict__ live, int* __restrict__ n_live, int* __restrict__ und, int* __restrict__ n_und,
                    int* __restrict__ acc, int* __restrict__ ticket, const ListJob lj, const StageJob stage) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x * 64 + lane;
    __shared__ int s_ub[64];
    if (wave == 0) s_ub[lane] = 0;
    if (MODE == RB_COARSE && threadIdx.x == 0) ticket[blockIdx.x] = 0;
    const bool valid = h < count && triples.valid(h);
    const RbHyp o = rb_load(hyp, h_pad, h, valid, pmax, sqrt_tau, band_u, MODE == RB_COARSE ? 5.f : 3.f);   // (coarse margin 5 E: see above)
    const int best = state[0];
    // Gate: with the best under a 32nd of the points nothing is pruned (true share 0.02: best 0.017 N), and the walk - whose RB_SPLIT
    // partial sums each have to pass the best before a wave stops - cost 8.5 % there: every hypothesis is live without it.  At a true
    // share of 0.1 (best 0.09 N) it still prunes 14 % of the tests and gains a point.
    const bool walk = rb_gate(best, ns);
    int fl = 0;                                                   // ransac_prejudge's word, asked for in front of the walk: the tail does not wait for it
    if (wave == 0 && valid) fl = lj.flags[h];
    // RansacStage: this thread's word of the next batch's triples, asked of the host's memory behind the pose's loads (loads return in
    // order: in front of them it would hold the pose back for the link's latency) and stored behind the walk, which needs no vector
    // load - the link's latency lies under the walk.  The load is every thread's, its index clamped (a thread past the count loads the
    // last word and stores nothing): behind a branch the compiler waits for it where the branch joins, in front of the walk.
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t sw = 0;
    if (STAGE) sw = stage.src[min(gid, stage.cnt - 1)];
    const int per = (n_lpairs + RB_SPLIT - 1) / RB_SPLIT, k0 = __builtin_amdgcn_readfirstlane(wave) * per, k1 = min(n_lpairs, k0 + per);   // (uniform: scalar loads)
    const int ub = rb_walk(o.r, leaves, k0, k1, o.tb, best, !valid || !o.bounded || !walk);
    if (STAGE) {
        if (gid < stage.cnt) stage.dst[gid] = sw;
        const int all = gridDim.x * blockDim.x;      // (a next batch larger than this one's threads: the rest of it, word by word)
        for (int i = gid + all; i < stage.cnt; i += all) stage.dst[i] = stage.src[i];
    }
    __syncthreads();                                 // (s_ub zeroed)
    if (ub) atomicAdd(&s_ub[lane], ub);
    __syncthreads();
    if (wave != 0) return;
    const int total = s_ub[lane];
    const bool gated = valid && (!o.bounded || !walk);            // live without a walk
    const bool close = (fl & RB_CLOSE) != 0;                      // live whatever the walk said (RansacBoundLists)
    const bool undecided = MODE == RB_COARSE && valid && !gated && !close && total > best;
    const bool is_live = gated || close || (MODE == RB_ONE && valid && total > best);
    const bool near = is_live && lj.near && (fl & RB_NEAR);
    const unsigned long long mc = __ballot(close);
    if (mc && lane == 0) atomicAdd(lj.n_close, __popcll(mc));
    const int slot = rb_append3(is_live && !near, near, undecided, lane, h, live, n_live, lj.near, lj.n_near, und, n_und);
    if (MODE == RB_COARSE && undecided) acc[slot] = 0;
}
// k_ransac_bound_fine: the undecided hypotheses over the fine leaves.  They are a tenth of the batch with Morton leaves, a
// twenty-fifth with class-major ones - too few workgroups to fill the chip with one per 64 of them, and how few the host does not
// know.  So the grid is the chip's (fine_grid: the workgroups it holds at once, whatever the batch), and every workgroup reads the
// list's length and cuts the work alike (ransac_cut.hpp: fine_ranges): a unit is a slot block of 64 hypotheses over one of R ranges
// of the leaf pairs, unit u is range u / nb of slot block u mod nb, and workgroup w takes the units w, w + gridDim.x, ...  (Until round 29 the grid was the batch's slot blocks times a
// fixed 4 ranges: the kernel took two rounds of a 49-pair walk for any list from a third of the chip up, and a shorter list gained
// nothing - profiles/r14/ransac_bound_lists.md, profiles/r29/ransac_leaf_classes.md.)  force_y > 0 (study build,
// TDV_RANSAC_FINE_Y): R = force_y whatever the list, the A/B.
// A workgroup adds its 64 partial sums to acc[slot], and the last of a slot block's R arrivals (ticket) decides: live on a
// total > best, dead otherwise.  A partial sum that stopped early exceeds best alone, so a stop anywhere makes the total exceed it
// too; without one the total is the full fine sum - the one-level walk's verdict, whatever the cut.  A unit whose range is empty
// (fewer leaf pairs than ranges) still arrives.  No workgroup waits for another.
// The kernel's one argument.  A unit reads what it needs from the kernel-argument segment itself (FineJobArg, the segment's address
// made anew per unit): held in scalar registers from the kernel's start across every unit's walk, the pointers of the tail took the
// kernel to 94 SGPRs, and above 80 a CU admits one workgroup of 16 waves, not two (measured: a list of 276 units took two rounds).
struct FineJob {
    const float* hyp; const float* leaves; const unsigned* pmax; const int* state; const int* und; const int* n_und;
    int *live, *n_live, *acc, *ticket; ListJob lj;
    int h_pad, n_lpairs, force_y; float sqrt_tau, band_u;
};
typedef const FineJob __attribute__((address_space(4)))* FineJobArg;
__global__ __launch_bounds__(64 * RB_SPLIT)
void k_ransac_bound_fine(const FineJob job) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = *job.n_und, best = job.state[0], n_lpairs = job.n_lpairs;
    const int nb = (n + 63) / 64;                    // slot blocks on the list
    int ranges = job.force_y > 0 ? job.force_y : 1;
    if (job.force_y <= 0 && nb > 0) {               // fine_ranges, lane r - 1 asking for r ranges
        unsigned long long key = fine_cut_key(lane + 1, nb, n_lpairs, (int)gridDim.x, RB_SPLIT);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(key, off, 64); key = o < key ? o : key; }
        ranges = __builtin_amdgcn_readfirstlane((int)(key & 127ull));
    }
    const int per_y = (n_lpairs + ranges - 1) / ranges, units = nb * ranges;      // (nb <= 2^25 / 64, ranges <= 64)
    // (the leaves through the constant address space: nothing writes them while a batch's kernels run, and behind a unit's fence and
    // atomics the compiler would not take that from the pointer itself - the walk's wave-uniform loads must stay scalar)
    const RbConstLeaves leaves = (RbConstLeaves)job.leaves;
    __shared__ int s_ub[64];
#pragma unroll 1
    for (int u = blockIdx.x; u < units; u += (int)gridDim.x) {        // workgroup-uniform
        FineJobArg j = (FineJobArg)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(j));                  // (made anew: what is read through it is read per unit and dies with the unit)
        // (slot block fastest, as the old grid's x: the workgroups that start side by side walk the same range of the leaves)
        const int y = u / nb, xb = u - y * nb;
        const int y0 = min(n_lpairs, y * per_y), y1 = min(n_lpairs, y0 + per_y);
        const int per = (y1 - y0 + RB_SPLIT - 1) / RB_SPLIT;
        const int k0 = min(y1, y0 + wave * per), k1 = min(y1, k0 + per);
        const int slot = xb * 64 + lane;
        const int h = slot < n ? j->und[slot] : -1;
        if (wave == 0) s_ub[lane] = 0;               // (behind wave 0's read of the unit before; the others add behind the barrier)
        const RbHyp o = rb_load(j->hyp, j->h_pad, h, h >= 0, j->pmax, j->sqrt_tau, j->band_u, 3.f);
        const int ub = rb_walk(o.r, leaves, k0, k1, o.tb, best, h < 0);
        __syncthreads();                             // (s_ub zeroed)
        if (ub) atomicAdd(&s_ub[lane], ub);
        __syncthreads();
        if (wave != 0) continue;
        int tl = lane;                               // the tail's lane, made anew per unit as well: nothing the tail derives from it
        asm volatile("" : "+v"(tl));                 // stays in registers across the walk (the kernel has 64 VGPRs at 8 waves per SIMD)
        FineJobArg t = (FineJobArg)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(t));
        const int tslot = xb * 64 + tl;
        const int part = s_ub[tl];
        int* const acc = t->acc;
        if (h >= 0 && part) atomicAdd(&acc[tslot], part);
        __threadfence();
        int arrived = 0;
        if (tl == 0) arrived = atomicAdd(&t->ticket[xb], 1);
        if (__shfl(arrived, 0, 64) != ranges - 1) continue;           // not the last unit of this slot block
        const int total = h >= 0 ? atomicAdd(&acc[tslot], 0) : 0;
        const bool is_live = h >= 0 && total > best;
        int* const nearl = t->lj.near;
        const bool near = is_live && nearl && (t->lj.flags[h] & RB_NEAR);
        rb_append3(is_live && !near, near, false, tl, h, t->live, t->n_live, nearl, t->lj.n_near, nullptr, nullptr);
    }
}

#ifdef TDV_STUDY
#include "ransac_study.hpp"     // the matrix-core scoring variant and the hypothesis probe
#endif

// error sum of one hypothesis (column-major R in hyp12[0..8], t in hyp12[9..11]) over all points: a slab of (sum, count) per workgroup
__global__ __launch_bounds__(256)
void k_ransac_rmse_partial(const float* __restrict__ pq, int ns, const float* __restrict__ hyp12, float tau,
                           double* __restrict__ slabs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double e = 0.0, n = 0.0;
    if (i < ns) {
        const float* g = pq + (size_t)i * 8;
        float px = g[0], py = g[1], pz = g[2];
        float x = (hyp12[0] * px + (hyp12[3] * py + hyp12[6] * pz)) + hyp12[9];
        float y = (hyp12[1] * px + (hyp12[4] * py + hyp12[7] * pz)) + hyp12[10];
        float z = (hyp12[2] * px + (hyp12[5] * py + hyp12[8] * pz)) + hyp12[11];
        float dx = x - g[3], dy = y - g[4], dz = z - g[5];
        float d2 = dx * dx + (dy * dy + dz * dz);
        if (d2 < tau) { float err = sqrtf(d2); e = (double)(err * err); n = 1.0; }  // d2 < tau <=> sqrtf(d2) < thr
    }
    __shared__ double red[2][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { e += __shfl_down(e, off, 64); n += __shfl_down(n, off, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = e; red[1][threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        slabs[2 * (size_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        slabs[2 * (size_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}
__global__ void k_ransac_rmse_final(const double* __restrict__ slabs, int nblocks, double* __restrict__ out2) {
    __shared__ double pe[256], pn[256];
    double e = 0.0, n = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) { e += slabs[2 * (size_t)b]; n += slabs[2 * (size_t)b + 1]; }
    pe[threadIdx.x] = e; pn[threadIdx.x] = n;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) { pe[threadIdx.x] += pe[threadIdx.x + off]; pn[threadIdx.x] += pn[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out2[0] = pe[0]; out2[1] = pn[0]; }
}

int ransac_score_pose_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const int* d_corr, const float* d_hyp12,
                          float voxel, double* d_out2) {
    if (ns <= 0 || nt <= 0) return TDV_ERR_BAD_ARG;
    hipStream_t s = ctx->stream;
    const int ns_pad = (int)align_up((size_t)ns, 256), rblocks = (ns + 255) / 256;
    float* pq = nullptr; double* slabs = nullptr; int* flags = nullptr;
    TDV_TRY(ws_alloc(ctx, (size_t)ns_pad * 8, &pq));
    TDV_TRY(ws_alloc(ctx, (size_t)2 * rblocks, &slabs));
    TDV_TRY(ws_alloc(ctx, 2, &flags));
    TDV_HIP(ctx, hipMemsetAsync(flags, 0, 8, s));
    k_gather_pq<<<ns_pad / 256, 256, 0, s>>>(d_src, d_tgt, d_corr, ns, ns_pad, nt, pq, flags, reinterpret_cast<unsigned*>(flags + 1));
    k_ransac_rmse_partial<<<rblocks, 256, 0, s>>>(pq, ns, d_hyp12, tau_lt(voxel * 1.5f), slabs);
    k_ransac_rmse_final<<<1, 256, 0, s>>>(slabs, rblocks, d_out2);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// ------------------------------------------------------------------ the driver
// RegistrationResult defaults (include/registration.hpp:26-30)
static void result_defaults(tdv_ransac_result* out) {
    for (int i = 0; i < 16; ++i) out->T[i] = (i % 5 == 0) ? 1.f : 0.f;
    out->fitness = 0.f; out->rmse = 0.f; out->inliers = 0; out->best_iteration = -1; out->iterations_run = 0;
}
// a hypothesis' 12 floats (column-major R, then t) into the column-major 4x4 T, whose last row keeps its defaults
static void pose_to_T16(const float* h12, float* T) {
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) T[c * 4 + r] = h12[c * 3 + r];
    T[12] = h12[9]; T[13] = h12[10]; T[14] = h12[11];
}

// A call's device block: one memset at the start, and the part in front of `sel` comes back in one copy at the end.  The pinned
// host block that copy lands in has the same type; its `bad` (traced calls) and `rec` also receive what a batch reports.
struct RansacBlock {
    int bad;                                 // a correspondence index outside [0, nt) was met
    unsigned pmax;                           // the largest |source coordinate| (bits of a non-negative float)
    unsigned long long rescored, scored;     // the fast pass' statistics: point pairs scored twice, (wave, chunk) pairs scored
    long long bound[4];                      // RansacBoundLists, over the call's bounded batches: hypotheses bounded, close, put on the fine list, live (far + near)
    int state[2];                            // [0] the best count known so far (RansacPlan)
    int plan[2][8];                          // per batch buffer: phase-1 chunks, survivors, largest prefix count; near lists: phase 1's end, survivors (three words unused)
    float best12[12];                        // the winning hypothesis
    double out2[2];                          // its error sum and inlier count
    int sel[4];                              // RansacFinish's loop state: best fitness (bits), its count, its iteration, stopped
    int rec[2][8];                           // per batch buffer: RansacFinish's record (4 ints; moved as 32 bytes under TDV_RANSAC_RECORD=copy)
    RansacFar far;                           // RansacFarBound: the ordering pose, the class sizes, the count table
};
constexpr size_t kRansacReadBack = offsetof(RansacBlock, sel);
static_assert(std::is_trivially_copyable<RansacBlock>::value, "memset, copied back");
static_assert(offsetof(RansacBlock, rescored) % 8 == 0 && offsetof(RansacBlock, scored) == offsetof(RansacBlock, rescored) + 8, "the kernels index the two as one u64[2]");
static_assert(offsetof(RansacBlock, out2) % 8 == 0 && offsetof(RansacBlock, out2) + sizeof(double[2]) == kRansacReadBack, "the part read back is a prefix that ends with out2");
// RansacLeafBound's and RansacFarBound's list lengths and RansacBoundLists' count of close hypotheses per batch buffer; ransac_plan zeroes
// a buffer's four through &n_live[q]: [0], [2], [4] and [6], and k_ransac_finish reads them the same way
struct RansacLive { int n_live[2], n_und[2], n_near[2], n_close[2]; };
static_assert(offsetof(RansacLive, n_und) == offsetof(RansacLive, n_live) + 2 * sizeof(int) && offsetof(RansacLive, n_near) == offsetof(RansacLive, n_live) + 4 * sizeof(int) &&
              offsetof(RansacLive, n_close) == offsetof(RansacLive, n_live) + 6 * sizeof(int), "ransac_plan's n_live[2], n_live[4], n_live[6]");

// Every switch of a call, read in one place.  TDV_RANSAC_SCORE=exact and TDV_RANSAC_BAILOUT are read once per process, the rest per
// call (the tests switch them); study_env() is a constant nullptr in the product library.
struct RansacKnobs { bool score_fast, score_mfma, bailout, bound, one_level, leaf_classes, merge, record_copy, upload_inline, order, far, end_event, timer_events; int drop_permille, a_permille, u_cut_permille, fine_y, grown, triples; float far_radius, live_radius; };
static RansacKnobs ransac_knobs(const tdv_ctx* ctx, bool traced, int max_iterations, int ns) {
    RansacKnobs k;
    static const bool score_exact_env = getenv("TDV_RANSAC_SCORE") && !strcmp(getenv("TDV_RANSAC_SCORE"), "exact");
    k.score_fast = !score_exact_env && ctx->ransac_score_mode != TDV_RANSAC_SCORE_EXACT;
    const bool score_mfma_env = study_env("TDV_RANSAC_SCORE") && !strcmp(study_env("TDV_RANSAC_SCORE"), "mfma");
    k.score_mfma = kStudyBuild && k.score_fast && (score_mfma_env || ctx->ransac_score_mode == TDV_RANSAC_SCORE_MATRIX);   // study build only
    static const bool bailout_env_off = getenv("TDV_RANSAC_BAILOUT") && atoi(getenv("TDV_RANSAC_BAILOUT")) == 0;   // A/B knob
    // RansacPlan; short calls run as one batch without it (C4's 10,000 iterations: a short first batch lost 2 % - best fitness 0.1-0.2)
    k.bailout = k.score_fast && !k.score_mfma && !traced && !bailout_env_off && max_iterations > 16384;
    k.merge = study_env("TDV_RANSAC_MERGE") && atoi(study_env("TDV_RANSAC_MERGE")) == 1;     // phase 2 rides behind the next batch's phase 1
    // RansacLeafBound: the leaf summary once per call, the bound in front of phase 1 of every batch after the first (whose best is 0)
    const bool bound_env_off = getenv("TDV_RANSAC_BOUND") && atoi(getenv("TDV_RANSAC_BOUND")) == 0;   // A/B knob
    k.bound = k.bailout && !k.merge && !bound_env_off;
    // RansacPointOrder: the best's outliers first, once per call after the first batch (the merged dispatch has no best12 by then)
    // TDV_RANSAC_ORDER: 0 the natural order, 1 the two-way order without skipping, unset (or anything else) the three classes of
    // RansacFarBound, whose near lists need the bound's lists and box
    const char* const order_env = getenv("TDV_RANSAC_ORDER");   // A/B knob
    k.order = k.bailout && !k.merge && !(order_env && atoi(order_env) == 0);
    k.far = k.order && k.bound && !(order_env && atoi(order_env) == 1);
    // tuning knobs: F from far_radius thresholds on; a near list's phase 1 takes a_permille of I; near means UB_F <= u_cut_permille of the
    // best count (profiles/r13/ransac_far_outliers.md)
    k.far_radius = study_env("TDV_RANSAC_FAR_RADIUS") ? (float)atof(study_env("TDV_RANSAC_FAR_RADIUS")) : 4.f;
    k.a_permille = study_env("TDV_RANSAC_FAR_A_PERMILLE") ? atoi(study_env("TDV_RANSAC_FAR_A_PERMILLE")) : 110;
    k.u_cut_permille = study_env("TDV_RANSAC_FAR_UCUT_PERMILLE") ? atoi(study_env("TDV_RANSAC_FAR_UCUT_PERMILLE")) : 22;
    // RansacBoundLists: a hypothesis within live_radius thresholds of the running best is live unwalked (0: off); the fine level
    // cuts the leaf pairs into as many ranges as its list's length asks for (fine_ranges) - fine_y > 0: into fine_y, whatever the list
    k.live_radius = study_env("TDV_RANSAC_LIVE_RADIUS") ? (float)atof(study_env("TDV_RANSAC_LIVE_RADIUS")) : 20.f;
    k.fine_y = study_env("TDV_RANSAC_FINE_Y") ? std::min(std::max(atoi(study_env("TDV_RANSAC_FINE_Y")), 1), kFineMaxRanges) : 0;
    // the batch schedule (ransac_cut.hpp: ransac_batch_size): the grown batch's size - kRansacBatch: no growth, the A/B.  (The fine
    // level cuts by its list, not by the batch.)
    k.grown = study_env("TDV_RANSAC_GROWN") ? (int)align_up((size_t)std::min(std::max(atoi(study_env("TDV_RANSAC_GROWN")), kRansacBatch), 4 * kRansacBatch), RS_HYP_PER_BLOCK) : kRansacGrown;
    // class-major leaves (k_leaf_keys): the context's mode (tdv_ctx_set_ransac_leaf_order), AUTO by the call's size
    // (ransac_cut.hpp: kRansacLeafClassesMin - on a 9,999-point cloud they take the live list from 4,317 to 4,063 hypotheses, one block
    // of 1,024 fewer for the two-way order but not for the far and near lists together, and tests/test_gpu_ransac_far_bound.py holds
    // the far bound strictly under the two-way order there).  The study build's TDV_RANSAC_LEAF_CLASSES overrides: 1 on, else off.
    k.leaf_classes = ctx->ransac_leaf_order == TDV_RANSAC_LEAVES_CLASSES || (ctx->ransac_leaf_order == TDV_RANSAC_LEAVES_AUTO && ns >= kRansacLeafClassesMin);
    if (study_env("TDV_RANSAC_LEAF_CLASSES")) k.leaf_classes = atoi(study_env("TDV_RANSAC_LEAF_CLASSES")) == 1;
    k.one_level = study_env("TDV_RANSAC_BOUND_LEVELS") && atoi(study_env("TDV_RANSAC_BOUND_LEVELS")) == 1;   // A/B knob: the fine walk alone
    k.record_copy = study_env("TDV_RANSAC_RECORD") && !strcmp(study_env("TDV_RANSAC_RECORD"), "copy");   // the record by a 32-byte copy, not by the kernel's own stores into pinned memory
    // A/B knobs (profiles/r18/ransac_no_events.md): the batch's end by an event as it was; the fast kernel's score timer by events as it was
    k.end_event = traced || k.record_copy || (study_env("TDV_RANSAC_END") && !strcmp(study_env("TDV_RANSAC_END"), "event"));   // (a traced call's counts come by a copy: it keeps the event)
    k.timer_events = study_env("TDV_RANSAC_TIMER") && !strcmp(study_env("TDV_RANSAC_TIMER"), "events");
    k.upload_inline = study_env("TDV_RANSAC_UPLOAD") && !strcmp(study_env("TDV_RANSAC_UPLOAD"), "inline");   // A/B knob: the triples by a copy on the compute stream in front of k_ransac_hypotheses, not by the kernel's own loads from pinned memory
    // RansacStage: the context's mode (tdv_ctx_set_ransac_triples; AUTO stages wherever a call can: RansacRun::setup); the study
    // build's TDV_RANSAC_UPLOAD=staged / =direct overrides
    k.triples = ctx->ransac_triples;
    if (study_env("TDV_RANSAC_UPLOAD") && !strcmp(study_env("TDV_RANSAC_UPLOAD"), "staged")) k.triples = TDV_RANSAC_TRIPLES_STAGED;
    if (study_env("TDV_RANSAC_UPLOAD") && !strcmp(study_env("TDV_RANSAC_UPLOAD"), "direct")) k.triples = TDV_RANSAC_TRIPLES_DIRECT;
    k.drop_permille = study_env("TDV_RANSAC_DROP_PERMILLE") ? atoi(study_env("TDV_RANSAC_DROP_PERMILLE")) : 50;   // tuning knob: phase 1 over the first N - 0.95 best points (natural order: 5 to 100 measured equal;
                                                                                                                     // best's outliers first, round 12: 25, 50 and 75 above 100, profiles/r12/ransac_point_order.md)
    return k;
}

// One of the two sets of batch buffers: batch k+1 is drawn on the host and enqueued while the GPU scores batch k; results are
// consumed in iteration order, so the outcome is that of the sequential loop.
struct RansacBuf {
    float* hyp; int* counts; void* tri; int* list;    // [14][h_pad] hypotheses (h_pad: the call's largest batch, the stride; a batch fills its own slots()), their counts, the triples on the device (k_ransac_hypotheses stores them); bail-out: phase 2's list
    int *live, *und, *acc, *ticket;                   // RansacLeafBound: live list, undecided list, its fine sums and tickets
    int *near, *list2, *ubf;                          // RansacFarBound: near list, its phase 2's list, UB_F per hypothesis
    int* flags;                                       // RansacBoundLists: ransac_prejudge's word per hypothesis (RB_CLOSE, RB_NEAR)
    int* units;                                       // bail-out: job B's ticket words, [far, near][2 phases][8 XCDs][slots(cnt) / RS_BLOCK] of the batch in it - unit_words(cnt) words, which its k_ransac_hypotheses zeroes (room for unit_words(cap))
    int *plan, *rec, *n_live, *n_und, *n_near;        // this buffer's fields of the RansacBlock and of RansacLive
    void* h_tri; int* h_cnt; volatile int* h_rec;     // pinned: the slot that holds the triples of the batch in this buffer (RansacRun::slot_ptr), counts (traced calls), the record
    bool staged;                                      // RansacStage: the batch in this buffer found its triples on the device
    hipEvent_t ev;                                    // the batch's end where an event marks it (traced calls; study build: TDV_RANSAC_RECORD=copy, TDV_RANSAC_END=event)
    int seq;                                          // ... and everywhere else the sequence number that k_ransac_finish stores behind the record (h_rec[4])
};
struct RansacBatch { int q, cnt, it0; bool bounded, staged; };        // buffer q holds cnt hypotheses from iteration it0 on; staged: their triples are on the device already
struct RansacDrawn { int it0, cnt, slot; };           // a batch as the host drew it: cnt triples from iteration it0 on in pinned slot `slot`
struct RangeCut { int per, ranges; };                 // chunks per point range, point ranges
static RangeCut range_cut(int hb, int n_pchunks) {    // of a dispatch with hb hypothesis blocks (counts are added by atomics: the cut may differ per dispatch)
    const int per = (n_pchunks + point_ranges(hb, n_pchunks) - 1) / point_ranges(hb, n_pchunks);
    return RangeCut{per, (n_pchunks + per - 1) / per};
}
static int hyp_blocks(int cnt) { return (int)(align_up((size_t)cnt, RS_HYP_PER_BLOCK) / RS_HYP_PER_BLOCK); }
static int score_grid(int hb, int ps) { return 8 * ((hb + 8 / RS_XCD_R - 1) / (8 / RS_XCD_R)) * ((ps + RS_XCD_R - 1) / RS_XCD_R); }   // k_ransac_score_fast's job-A workgroups
// ... and its job-B workgroups: as many as the device holds at once (two of 16 waves per CU at the kernel's 8 waves per SIMD), a
// multiple of 8.  Only speed depends on it: the host knows neither how many hypotheses are listed nor how long phase 1 was, and
// the workgroups pull their units, so any grid of at least 8 drains any list.
static int unit_grid(int cus) { return std::max(8, (2 * cus + 7) / 8 * 8); }
// k_ransac_bound_fine's workgroups: the same count - its workgroups have 16 waves too, two per CU at 8 waves per SIMD - and for the
// same reason: they take their units by the list's length, which the host does not know.
static int fine_grid(int cus) { return unit_grid(cus); }

// One call of ransac_run_dev: what its steps share, and the steps in the order a batch takes them.
struct RansacRun {
    tdv_ctx* ctx; hipStream_t s; RansacKnobs k;
    int ns, nt, max_iterations; float confidence; int* trace;
    float tau, sqrt_tau, band_u;
    int ns_pad, n_pchunks, batch, cap, h_pad, packed, rblocks, n_lpairs = 0, n_cpairs = 0, cus = 0;
    size_t tri_bytes;                                 // per triple: one packed word or an int4
    float *pq = nullptr, *pq2 = nullptr, *pq3 = nullptr, *leaves = nullptr, *cleaves = nullptr; double* slabs = nullptr;
    RansacBlock *d = nullptr, *h = nullptr; RansacLive* lv = nullptr;
    unsigned long long* leaf_keys = nullptr; unsigned* leaf_vals = nullptr; bool leaves_built = false;   // RansacLeafBound: the sort's keys and values; built for this call
    unsigned long long* ord_mask = nullptr; int* ord_cnt = nullptr; bool ordered = false;     // RansacPointOrder: ballot words, block counts (outliers, then F); done for this call
    unsigned* enc = nullptr;                          // RansacLeafBound: the finite coordinates' bounds per axis
    RansacBuf buf[2] = {};
    // RansacStage: the pinned triple slots (two; three in rotation where the call stages), whether it does, the batches drawn so
    // far and where the next one starts, and the batches the loop reached that ran from staged triples
    char* h_slots = nullptr; size_t sz_slot = 0; int n_slots = 2; bool stage = false;
    int n_drawn = 0, it_drawn = 0, n_staged = 0;
    void* slot_ptr(int slot) const { return h_slots + (size_t)slot * sz_slot; }
    // TDV_TIMER_RANSAC_SCORE's stamps (score_stamp_begin): a {t0, t1} pair per dispatch of k_ransac_score_fast, nullptr with timing off
    unsigned long long *stamps = nullptr, *h_stamps = nullptr; int n_stamps = 0, stamps_used = 0;
    RansacBatch pending = {}; bool has_pending = false;       // merged dispatch (study build): the batch whose phase 2 is not enqueued yet
    double wave_chunks = 0.0;                         // wave x chunk pairs the call would score without bail-out
    float best_fitness = 0.f; int best_iter = -1, best_inliers = 0, done_iters = 0; bool stop = false;   // the reference loop's state

    TriView tri(const RansacBuf& B) const { return TriView{B.tri, packed}; }
    // ---- set-up: pair gather, optional leaf summary, pair packing, the batch buffers
    int setup(const float* d_src, const float* d_tgt, const int* d_corr) {
        ns_pad = (int)align_up((size_t)ns, (size_t)RS_PCH * 64);
        TDV_TRY(ws_alloc(ctx, (size_t)ns_pad * 8, &pq)); TDV_TRY(ws_alloc(ctx, 1, &d));
        TDV_HIP(ctx, hipMemsetAsync(d, 0, sizeof(RansacBlock), s));
        k_gather_pq<<<(ns_pad + 255) / 256, 256, 0, s>>>(d_src, d_tgt, d_corr, ns, ns_pad, nt, pq, &d->bad, &d->pmax);
        if (k.bound) TDV_TRY(leaf_alloc());
#ifdef TDV_STUDY
        if (k.score_mfma) TDV_TRY(mfma_pack(ctx, pq, ns, ns_pad, &pq3));
        else
#endif
        {
            TDV_TRY(ws_alloc(ctx, (size_t)ns_pad * 6, &pq2));
            k_pack_pq2<<<(ns_pad / 2 + 255) / 256, 256, 0, s>>>(pq, ns_pad, pq2);
        }
        TDV_CHECK_LAUNCH(ctx);
        // batch size: enough hypotheses to fill the chip, bounded for early exit granularity
        batch = std::min(std::max(max_iterations, 1), kRansacBatch);  // per-batch host sync is ~0.3 ms: amortise it
        // With the bail-out the sizes are the schedule's (ransac_cut.hpp: ransac_batch_size, the one statement of it): a shorter first
        // batch establishes a best count for the rest, batches of kRansacBatch follow, and from iteration kRansacGrowAt on they grow.
        // Here: how many batches the call has, and the largest of them (cap) - what the per-batch buffers hold.  A call that never
        // reaches a grown batch allocates what it did before there was one; h_pad is the layout's stride, a batch's kernels cover
        // its own slots().
        int n_batches = 0; cap = batch;
        for (int it = 0; it < max_iterations; ++n_batches) { const int c = std::min(batch_size(it), max_iterations - it); cap = std::max(cap, c); it += c; }
        h_pad = (int)align_up((size_t)cap, RS_HYP_PER_BLOCK); n_pchunks = ns_pad / RS_PCH;
        packed = (uint64_t)ns <= kTriplePackMaxN;      // triples as one 64-bit word each (tdv_internal.hpp: triple_pack)
        tri_bytes = packed ? 8 : 16;
        for (RansacBuf& B : buf) { TDV_TRY(ws_alloc(ctx, (size_t)14 * h_pad, &B.hyp)); TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.counts)); TDV_TRY(ws_alloc_bytes(ctx, (size_t)cap * tri_bytes, &B.tri)); }
        if (k.bailout) {
            for (RansacBuf& B : buf) { TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.list)); TDV_TRY(ws_alloc(ctx, (size_t)unit_words(cap), &B.units)); }
            TDV_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        }
        if (k.order) { TDV_TRY(ws_alloc(ctx, (size_t)2 * order_blocks() * (RO_BLOCK / 64), &ord_mask)); TDV_TRY(ws_alloc(ctx, (size_t)2 * order_blocks(), &ord_cnt)); }
        if (k.bound) {
            for (RansacBuf& B : buf) {
                TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.live)); TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.und));
                TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.acc)); TDV_TRY(ws_alloc(ctx, (size_t)h_pad / 64, &B.ticket));
                TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.flags));
            }
            TDV_TRY(ws_alloc(ctx, 1, &lv));
        }
        if (k.far) for (RansacBuf& B : buf) { TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.near)); TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.list2)); TDV_TRY(ws_alloc(ctx, (size_t)h_pad, &B.ubf)); }
        rblocks = (ns + 255) / 256; TDV_TRY(ws_alloc(ctx, (size_t)2 * rblocks, &slabs));
        // the score timer's stamps: two dispatches per batch and one to spare, {all ones, 0} each
        if (ctx->timing && k.score_fast && !k.score_mfma && !k.timer_events) {
            n_stamps = 2 * n_batches + 1;
            TDV_TRY(ws_alloc(ctx, (size_t)2 * n_stamps, &stamps));
            TDV_HIP(ctx, hipMemsetAsync(stamps, 0xff, (size_t)n_stamps * 8, s));              // [n_stamps] t0, then [n_stamps] t1
            TDV_HIP(ctx, hipMemsetAsync(stamps + n_stamps, 0, (size_t)n_stamps * 8, s));
        }
        // pinned: the block | 2 x triples | 2 x counts (traced calls only) | the stamps (timing on)
        const size_t sz_blk = align_up(sizeof(RansacBlock), 64), sz_tri = align_up((size_t)cap * tri_bytes, 64), sz_cnt = trace ? align_up((size_t)cap * 4, 64) : 0;
        // A call with bail-out reserves what the grown schedule needs (int4 triples), whatever its own length: pin_reserve grows by a
        // free and an allocation behind a stream synchronise, and the block then moves once per context - in its first such call - and
        // not at the start of a long call that follows shorter ones.
        const size_t sz_grown = k.bailout ? 2 * align_up((size_t)k.grown * 16, 64) : 0;
        const size_t tri_room = std::max(2 * sz_tri, sz_grown);
        TDV_TRY(pin_reserve(ctx, sz_blk + tri_room + 2 * sz_cnt + (size_t)n_stamps * 16));
        // RansacStage: who stages.  A call with the bound's coarse level (its carrier: so not traced, not short, no merged dispatch,
        // not the one-level walk), packed triples (one word per thread; int4 triples keep the direct read), and three slots inside
        // the room reserved above - the reservation's size is what it was: three packed slots of a grown batch are 3 MB of the
        // 4 MB a call with bail-out asks for.  Its first batch and the batch behind an unbounded one read directly all the same.
        stage = k.triples != TDV_RANSAC_TRIPLES_DIRECT && k.bound && !k.one_level && !k.upload_inline && !trace && packed && 3 * sz_tri <= tri_room;
        n_slots = stage ? 3 : 2; sz_slot = sz_tri; h_slots = ctx->pin + sz_blk;
        h = reinterpret_cast<RansacBlock*>(ctx->pin); h->bad = 0;
        h->rec[0][4] = h->rec[1][4] = 0;              // the sequence words: nothing of an earlier call (the stream is idle: ransac_run_dev)
        h_stamps = reinterpret_cast<unsigned long long*>(ctx->pin + sz_blk + tri_room + 2 * sz_cnt);      // (behind the whole room: the third slot lies past 2 x sz_tri)
        if (trace) TDV_HIP(ctx, hipMemcpyAsync(&h->bad, &d->bad, 4, hipMemcpyDeviceToHost, s));   // lands before the first batch's counts (RansacFinish: the flag comes in the record)
        for (int q = 0; q < 2; ++q) {
            RansacBuf& B = buf[q];
            B.plan = d->plan[q]; B.rec = d->rec[q]; B.n_live = lv ? &lv->n_live[q] : nullptr; B.n_und = lv ? &lv->n_und[q] : nullptr; B.n_near = lv ? &lv->n_near[q] : nullptr;
            B.h_tri = slot_ptr(q); B.staged = false; B.h_cnt = reinterpret_cast<int*>(ctx->pin + sz_blk + 2 * sz_tri + q * sz_cnt); B.h_rec = h->rec[q];
        }
        if (k.end_event) {
            buf[0].ev = event_acquire(ctx); buf[1].ev = event_acquire(ctx);   // from the ctx's pool: no create/destroy per call
            if (!buf[0].ev || !buf[1].ev) { release_events(); return TDV_ERR_OOM; }
        }
        return TDV_OK;
    }
    // the next dispatch's stamp pair (nullptr: timing off, or - cannot happen - more dispatches than setup counted), and the
    // slot its ScopedTimer gets: none where the stamps time it
    ScoreStamp next_stamp() { if (!stamps || stamps_used >= n_stamps) return ScoreStamp{nullptr, nullptr}; const int e = stamps_used++; return ScoreStamp{stamps + e, stamps + n_stamps + e}; }
    int score_slot() const { return stamps ? -1 : TDV_TIMER_RANSAC_SCORE; }
    // a dispatch of k_ransac_score_fast: with timing on the instance that stamps, and the dispatch's pair
    void launch_score(int grid, const ScoreJob& a, const ScoreJob& b, int g1) {
        const ScoreStamp st = next_stamp();
        if (st.t0) k_ransac_score_fast<true><<<grid, RS_BLOCK, 0, s>>>(a, b, g1, h_pad, pq2, n_pchunks, tau, &d->rescored, st);
        else k_ransac_score_fast<false><<<grid, RS_BLOCK, 0, s>>>(a, b, g1, h_pad, pq2, n_pchunks, tau, &d->rescored, st);
    }
    // The schedule: the size of the batch that starts at iteration it0 (its count is at most what is left of max_iterations) ...
    int batch_size(int it0) const { return k.bailout ? ransac_batch_size(it0, k.grown) : batch; }
    // ... and the hypothesis slots that a batch of cnt covers - its hypothesis kernel's grid, its blocks of ticket words: those of a
    // batch of `batch` as ever, a grown batch's own.  h_pad, the largest batch's, is only the stride of the layout.
    int slots(int cnt) const { return (int)align_up((size_t)std::max(cnt, batch), RS_HYP_PER_BLOCK); }
    int unit_words(int cnt) const { return 4 * 8 * (slots(cnt) / RS_BLOCK); }     // per buffer: phase 1's and phase 2's, then the near lists' two
    int order_blocks() const { return (ns + RO_BLOCK - 1) / RO_BLOCK; }
    void release_events() { for (RansacBuf& B : buf) { event_release(ctx, B.ev); B.ev = nullptr; } }
    // RansacLeafBound's summary of the pairs: fine and coarse leaves along the class-major Morton order.  Its buffers ...
    int leaf_alloc() {
        const int n_leaves = (ns + RL_LEAF - 1) / RL_LEAF, n_cleaves = (ns + RL_COARSE - 1) / RL_COARSE;
        n_lpairs = (n_leaves + 1) / 2; n_cpairs = (n_cleaves + 1) / 2;
        TDV_TRY(ws_alloc(ctx, 12, &enc)); TDV_TRY(ws_alloc(ctx, (size_t)2 * ns, &leaf_keys)); TDV_TRY(ws_alloc(ctx, (size_t)2 * ns, &leaf_vals));
        TDV_TRY(ws_alloc(ctx, (size_t)n_lpairs * 32, &leaves)); TDV_TRY(ws_alloc(ctx, (size_t)n_cpairs * 32, &cleaves));
        return TDV_OK;
    }
    // ... and its build, once per call in front of the first bounded batch - nothing reads the leaves before - and behind
    // point_order(), whose outlier words class the pairs (k_leaf_keys).  The sort takes its scratch (a table and one more set of
    // keys and values, 12 ns bytes) from the workspace here, not in setup: on a context's first call that can reach hipMalloc with
    // the first batch in flight - once per context, no effect on a result.
    int leaf_build() {
        const int n_leaves = (ns + RL_LEAF - 1) / RL_LEAF;
        unsigned long long* const keys = leaf_keys; unsigned* const vals = leaf_vals;
        TDV_HIP(ctx, hipMemsetAsync(leaves, 0, (size_t)n_lpairs * 32 * sizeof(float), s));
        TDV_HIP(ctx, hipMemsetAsync(cleaves, 0, (size_t)n_cpairs * 32 * sizeof(float), s));
        TDV_HIP(ctx, hipMemsetAsync(enc, 0xff, 24, s)); TDV_HIP(ctx, hipMemsetAsync(enc + 6, 0, 24, s));
        k_leaf_bounds<<<(ns + 255) / 256, 256, 0, s>>>(pq, ns, enc);
        k_leaf_keys<<<(ns + 255) / 256, 256, 0, s>>>(pq, ns, enc, k.leaf_classes && ordered ? ord_mask : nullptr, keys, vals);
        TDV_TRY(radix_sort_pairs_dev(ctx, keys, keys + ns, vals, vals + ns, (size_t)ns, RL_CLASS_BIT + (k.leaf_classes ? 1 : 0)));
        k_leaf_build<<<(n_leaves * RL_LEAF + 255) / 256, 256, 0, s>>>(pq, ns, vals + ns, leaves, cleaves);
        leaves_built = true;
        TDV_CHECK_LAUNCH(ctx); return TDV_OK;
    }

    // ---- a batch's steps.  TDV_TIMER_RANSAC_SCORE times every dispatch of a scoring kernel on its own: k_ransac_score_fast by its
    // stamps, the others between two events.
    // host: the next cnt triples of the index stream into buffer q (i0, i1, i2, valid: registration.cpp:240)
    // The batches are drawn in the call's order, each into the next slot of the rotation; the caller has seen to it that the slot's
    // last readers are done (loop()).
    RansacDrawn draw(TripleStream& idx) {
        const RansacDrawn dn{it_drawn, std::min(batch_size(it_drawn), max_iterations - it_drawn), n_drawn % n_slots};
        if (packed) idx.next_batch_packed(dn.cnt, static_cast<uint64_t*>(slot_ptr(dn.slot)));
        else idx.next_batch(dn.cnt, static_cast<int*>(slot_ptr(dn.slot)));
        ++n_drawn; it_drawn += dn.cnt;
        return dn;
    }
    // hypotheses, reading the triples where draw() put them.  The batch used to begin with a 512 KB copy of the triples on the compute
    // stream: 17 us of copy with an engine switch on either side, 36 us in which no kernel ran (profiles/r17/ransac_batch_path.md).
    // The host draws the triples into pinned memory, which the device can read, so k_ransac_hypotheses loads them from there and
    // leaves the device copy behind for the batch's later kernels.
    //  - A batch's slot is written by draw() and must hold still until the batch's k_ransac_hypotheses has run.  The next draw into it is
    //    for the batch after the next, and loop() waits for this batch's end (wait_batch) before that.  A traced call's consume_trace
    //    reads it on the host, behind the batch's event.
    //  - After an early exit a batch that was drawn and enqueued may still read its slot: ransac_run_dev synchronises the compute stream
    //    on every way out of loop(), before the next entry point draws into the pinned block or lets pin_reserve move it.
    //  - Traced calls and the merged dispatch (study build) read the same way; TDV_RANSAC_UPLOAD=inline (study build) is the copy on the
    //    compute stream as it was.
    //  - A staged batch (RansacStage) does not read its slot here at all: the coarse level of the batch before it has put the triples
    //    into B.tri, in stream order in front of this kernel, which takes them from there (up == nullptr).
    // One thread makes the batch's plan from the best count known now: full counts of the batches whose
    // phase 2 has run, the prefix counts of a pending one (a lower bound of its full counts - a bound is all the rule needs)
    int hypotheses(const RansacBatch& b) {
        const RansacBuf& B = buf[b.q];
        if (k.upload_inline) TDV_HIP(ctx, hipMemcpyAsync(B.tri, B.h_tri, (size_t)b.cnt * tri_bytes, hipMemcpyHostToDevice, s));
        const PlanJob plan{d->state, k.bailout ? B.plan : nullptr, ns, n_pchunks, k.drop_permille, b.bounded ? B.n_live : nullptr, B.units, k.bailout ? unit_words(b.cnt) : 0,
                           k.far && b.bounded ? &d->far : nullptr, k.a_permille};
        const PreJob pre{b.bounded ? B.flags : nullptr, B.ubf, k.far ? &d->far : nullptr, enc, d->best12, k.live_radius, k.u_cut_permille};
        k_ransac_hypotheses<<<(slots(b.cnt) + 255) / 256, 256, 0, s>>>(pq, tri(B), k.upload_inline || b.staged ? nullptr : B.h_tri, b.cnt, slots(b.cnt), h_pad, B.hyp, &d->pmax, sqrt_tau, B.counts, band_u, plan, pre);
        return TDV_OK;
    }
    // every test of the batch, no plan: the exact kernel, the fast one, or (study build) the matrix cores
    int score_all(const RansacBatch& b) {
        const RansacBuf& B = buf[b.q]; const int hb = hyp_blocks(b.cnt);
        ScopedTimer tm(ctx, k.score_fast && !k.score_mfma ? score_slot() : TDV_TIMER_RANSAC_SCORE);
#ifdef TDV_STUDY
        if (k.score_mfma) wave_chunks += mfma_score(s, B.hyp, h_pad, pq3, ns, b.cnt, tau, B.counts, &d->rescored);
        else
#endif
        if (k.score_fast) {
            const ScoreJob ja{B.hyp, B.counts, nullptr, nullptr, hb, range_cut(hb, n_pchunks).ranges, nullptr, nullptr, nullptr};
            const int gA = score_grid(hb, ja.ps);
            launch_score(gA, ja, ja, gA);
            wave_chunks += (double)hb * (RS_BLOCK / 64) * (double)n_pchunks;
        } else {
            const RangeCut c = range_cut(h_pad / RS_HYP_PER_BLOCK, n_pchunks);
            k_ransac_score<<<dim3(hb, c.ranges), RS_BLOCK, 0, s>>>(B.hyp, h_pad, pq2, n_pchunks, c.per, tau, B.counts);
        }
        return TDV_OK;
    }
    // RansacLeafBound: the dead hypotheses out - the batch's live list
    // next != nullptr (RansacStage): the batch behind b, drawn already; the coarse level carries its triples from their pinned slot
    // into the other buffer's tri.  That buffer held the batch before b, whose kernels - the last readers of its tri - stand in
    // front of this one in stream order.
    void bound(const RansacBatch& b, const RansacDrawn* next) {
        const RansacBuf& B = buf[b.q]; const int bgrid = (b.cnt + 63) / 64;
        const ListJob lj{B.flags, k.far ? B.near : nullptr, B.n_near, B.n_live + 6};
        if (k.one_level)
            k_ransac_bound<RB_ONE><<<bgrid, 64 * RB_SPLIT, 0, s>>>(B.hyp, h_pad, tri(B), b.cnt, leaves, n_lpairs, &d->pmax, sqrt_tau, band_u,
                                                                   d->state, ns, B.live, B.n_live, nullptr, nullptr, nullptr, nullptr, lj, StageJob{nullptr, nullptr, 0});
        else {
            const StageJob sj = next ? StageJob{static_cast<const uint64_t*>(slot_ptr(next->slot)), static_cast<uint64_t*>(buf[b.q ^ 1].tri), next->cnt} : StageJob{nullptr, nullptr, 0};
            const auto kernel = next && next->cnt > 0 ? k_ransac_bound<RB_COARSE, true> : k_ransac_bound<RB_COARSE, false>;
            kernel<<<bgrid, 64 * RB_SPLIT, 0, s>>>(B.hyp, h_pad, tri(B), b.cnt, cleaves, n_cpairs, &d->pmax, sqrt_tau, band_u,
                                                   d->state, ns, B.live, B.n_live, B.und, B.n_und, B.acc, B.ticket, lj, sj);
            const FineJob fj{B.hyp, leaves, &d->pmax, d->state, B.und, B.n_und, B.live, B.n_live, B.acc, B.ticket, lj, h_pad, n_lpairs, k.fine_y, sqrt_tau, band_u};
            k_ransac_bound_fine<<<fine_grid(cus), 64 * RB_SPLIT, 0, s>>>(fj);
        }
    }
    // RansacPointOrder: pq2 again from pq, the outliers of the best so far (best12, state[0]: the batches enqueued before) first
    void point_order() {
        RansacFar* const far = k.far ? &d->far : nullptr;
        k_order_flags<<<order_blocks(), RO_BLOCK, 0, s>>>(pq, ns, d->state, d->best12, tau, ord_mask, ord_cnt, far, std::max(tau, k.far_radius * k.far_radius * tau));
        k_order_scatter<<<order_blocks(), RO_BLOCK, 0, s>>>(pq, ns, ord_mask, ord_cnt, pq2, far);
        ordered = true;
    }
    ScoreJob job_a(const RansacBatch& b) const { return ScoreJob{buf[b.q].hyp, buf[b.q].counts, buf[b.q].plan, nullptr, hyp_blocks(b.cnt), range_cut(hyp_blocks(b.cnt), n_pchunks).ranges, nullptr, nullptr, nullptr}; }
    // phase 1: the batch's hypotheses (job A) - or, bounded, its live list as a job B (resident workgroups that pull units) - over
    // the chunks its plan sets
    void phase1(const RansacBatch& b) {
        const RansacBuf& B = buf[b.q];
        const int hbw = slots(b.cnt) / RS_BLOCK;
        const ScoreJob ja = job_a(b), jl{B.hyp, B.counts, B.plan, B.live, hbw, 0, B.n_live, B.units, nullptr};
        const ScoreJob jn = k.far ? ScoreJob{B.hyp, B.counts, B.plan, B.near, hbw, 0, B.n_near, B.units + 16 * hbw, &d->far.c_far} : jl;   // the near list rides behind the far one
        const int g1 = score_grid(ja.hb, ja.ps);          // (a multiple of 8: job B's XCD numbering starts there)
        ScopedTimer tm(ctx, score_slot());
        if (b.bounded) launch_score(unit_grid(cus), jn, jl, 0);
        else launch_score(g1, ja, ja, g1);
    }
    // survivors of the batch: the in-batch bound first (largest prefix count), then the list (bounded: both in one launch over its live list)
    int select(const RansacBatch& b) {
        const RansacBuf& B = buf[b.q];
        if (b.bounded) k_ransac_select_live<<<1, 1024, 0, s>>>(B.live, B.n_live, k.far ? B.near : nullptr, B.n_near, B.ubf, B.counts, ns, confidence, d->state, B.plan, B.list, B.list2);
        else {
            k_ransac_best<<<(b.cnt + 1023) / 1024, 1024, 0, s>>>(tri(B), b.cnt, B.counts, B.plan + 2);
            k_ransac_select<<<(b.cnt + 255) / 256, 256, 0, s>>>(tri(B), b.cnt, B.counts, ns, confidence, d->state, B.plan, B.list);
        }
        // (merged dispatch only: phase 2 comes a dispatch later, so the prefix counts raise the best for the batch in between)
        if (k.merge) k_ransac_best<<<(b.cnt + 1023) / 1024, 1024, 0, s>>>(tri(B), b.cnt, B.counts, d->state);
        wave_chunks += (double)hyp_blocks(b.cnt) * (RS_BLOCK / 64) * (double)n_pchunks;
        TDV_CHECK_LAUNCH(ctx); return TDV_OK;
    }
    // phase 2 of batch b: the hypotheses on its list over the chunks its phase 1 left out - alone, or (merged dispatch) riding as
    // job B behind the phase 1 `a` of the next batch, g1 workgroups
    int phase2(const RansacBatch& b, const ScoreJob* a = nullptr, int g1 = 0) {
        const RansacBuf& B = buf[b.q]; const int hbw = slots(b.cnt) / RS_BLOCK;
        const ScoreJob jb{B.hyp, B.counts, B.plan, B.list, hbw, 0, nullptr, B.units + 8 * hbw, nullptr};
        const ScoreJob jn = k.far && b.bounded ? ScoreJob{B.hyp, B.counts, B.plan, B.list2, hbw, 0, nullptr, B.units + 24 * hbw, &d->far.c_far} : jb;   // the near list's survivors behind the far one's
        const int g2 = unit_grid(cus);
        { ScopedTimer tm(ctx, score_slot()); launch_score(g1 + g2, a ? *a : jn, jb, g1); }
        TDV_CHECK_LAUNCH(ctx); return TDV_OK;
    }
    // the batch's end: RansacFinish and its record, or - traced - every count to the host.  with_state: the batch's
    // largest full count raises state[0] (a batch with bail-out).
    // No event stands behind the batch: an event record kept the next batch's k_ransac_hypotheses 5.8 us away
    // (profiles/r18/ransac_no_events.md).  k_ransac_finish stores the batch's sequence number - the ctx's counter, never 0, one more
    // per batch, so no word an earlier batch or call left can match - behind its record, and loop() waits for that word.
    int finish(const RansacBatch& b, bool with_state) {
        RansacBuf& B = buf[b.q];
        TDV_CHECK_LAUNCH(ctx);
        B.seq = 0;
        if (!k.end_event) { if (++ctx->ransac_seq <= 0) ctx->ransac_seq = 1; B.seq = ctx->ransac_seq; }
        if (!trace) {
            const bool live_only = b.bounded && confidence >= 0.f;      // (see k_ransac_finish)
            int* rec = k.record_copy ? B.rec : const_cast<int*>(B.h_rec);
            const auto kernel = live_only ? k_ransac_finish<true> : k_ransac_finish<false>;
            kernel<<<1, 1024, 0, s>>>(tri(B), b.cnt, B.counts, live_only ? B.live : nullptr, live_only ? B.n_live : nullptr,
                                      k.far ? B.near : nullptr, B.n_near, B.hyp, h_pad, ns, confidence, b.it0, with_state ? d->state : nullptr, d->sel, d->best12, &d->bad, rec,
                                      b.bounded ? B.n_live : nullptr, d->bound, B.seq);
            TDV_CHECK_LAUNCH(ctx);
            if (k.record_copy) TDV_HIP(ctx, hipMemcpyAsync(const_cast<int*>(B.h_rec), B.rec, sizeof(d->rec[0]), hipMemcpyDeviceToHost, s));
        } else TDV_HIP(ctx, hipMemcpyAsync(B.h_cnt, B.counts, (size_t)b.cnt * 4, hipMemcpyDeviceToHost, s));
        if (k.end_event) TDV_HIP(ctx, hipEventRecord(B.ev, s));
        return TDV_OK;
    }
    // The host's wait for the batch in buffer B.  With a sequence word: an acquire load in a spin (host_wait.hpp) until
    // k_ransac_finish's last store - at system scope, behind its record and its system fence - has landed in the
    // fine-grained pinned block; what the event gave is what this gives: every kernel of the batch has done its work (they run in
    // stream order in front of that store), so the record is whole and the batch's h_tri may be drawn over.  The spin cannot hang:
    // at intervals by the host's clock it asks the stream, and a stream that failed, or that ran dry without the word, ends the call.
    // (The question is not free: asked about a stream that is still running, the runtime puts a marker behind the last command
    // enqueued - the next batch's k_ransac_finish - and the kernel behind a marker starts 5.8 us late, which is the very gap the
    // event left.  So it is asked rarely: a batch of 65,536 hypotheses over 200k pairs takes a third of a millisecond and ends before
    // the first question; a longer one meets a marker per kRecordPollUs, a part in a thousand of its time.)
    static constexpr int kRecordPollUs = 5000;
    int wait_batch(const RansacBuf& B) {
        if (k.end_event) return hipEventSynchronize(B.ev) == hipSuccess ? TDV_OK : TDV_ERR_LAUNCH;
        hipError_t err = hipSuccess;
        const int st = wait_for_word(B.h_rec + 4, B.seq, [&] {
            err = hipStreamQuery(s);
            if (err == hipErrorNotReady) { (void)hipGetLastError(); return 1; }     // (not an error: it must not meet the next TDV_CHECK_LAUNCH)
            return err == hipSuccess ? 0 : -1;
        }, kRecordPollUs);
        if (st == HOST_WAIT_OK) return TDV_OK;
        if (st == HOST_WAIT_FAILED) return set_err(ctx, err, "ransac: the stream, while waiting for a batch's record,", __LINE__);
        std::snprintf(ctx->err, sizeof(ctx->err), "ransac: the stream ran dry and batch %d's record never came", B.seq);
        return TDV_ERR_LAUNCH;
    }
    // Study build, TDV_RANSAC_MERGE=1: one scoring dispatch per batch - its phase 1 and, behind it, phase 2 of the batch before, whose
    // end follows.  Measured: a point of lane-op utilisation gained, but the counts reach the host a dispatch later and the call loses
    // 11 % (profiles/r3/history/ransac_merged_dispatch.md); two batches in flight (three buffer sets) would hide that - not built.
    int enqueue_merged(const RansacBatch& b) {
        if (has_pending) {
            const ScoreJob ja = job_a(b);
            TDV_TRY(phase2(pending, &ja, score_grid(ja.hb, ja.ps)));
            TDV_TRY(finish(pending, true));
        } else phase1(b);
        TDV_TRY(select(b));
        pending = b; has_pending = true;
        return TDV_OK;                           // counts and event follow with this batch's phase 2
    }
    int finish_pending() { has_pending = false; TDV_TRY(phase2(pending)); return finish(pending, true); }

    // ---- the device side of one batch: the four paths
    // dn: the batch, drawn; staged: the batch before it has carried its triples to the device; next: the batch behind it, drawn
    // already, for this batch's coarse level to carry (nullptr: none, or not staged)
    int enqueue(int q, const RansacDrawn& dn, bool staged, const RansacDrawn* next) {
        const int cnt = dn.cnt, it0 = dn.it0;
        buf[q].h_tri = slot_ptr(dn.slot); buf[q].staged = staged;
        const RansacBatch b{q, cnt, it0, k.bound && it0 != 0, staged};
        // RansacPointOrder, once per call: the first batch has set a best, nothing reads pq2 in between (in front of the batch's
        // k_ransac_hypotheses, whose plan reads the class sizes)
        if (k.order && it0 != 0 && !ordered) point_order();
        if (b.bounded && !leaves_built) TDV_TRY(leaf_build());
        TDV_TRY(hypotheses(b));
        if (!k.bailout) { TDV_TRY(score_all(b)); return finish(b, false); }   // exact, traced, short or matrix-core calls: every test is scored
        if (k.merge) return enqueue_merged(b);
        if (b.bounded) bound(b, next);                       // bail-out with bound: phase 1 over the live list only
        phase1(b);
        TDV_TRY(select(b));
        TDV_TRY(phase2(b));
        return finish(b, true);
    }

    // ---- the host side of one batch, after its end (wait_batch)
    // RansacFinish ran the loop of registration.cpp:281-290 on the device: its record
    void consume_record(const RansacBuf& B, int it0, int cnt) {
        const int k_best = B.h_rec[0], k_stop = B.h_rec[2];
        if (k_best >= 0) {
            best_inliers = B.h_rec[1]; best_iter = it0 + k_best;
            best_fitness = static_cast<float>(best_inliers) / static_cast<float>((size_t)ns);  // registration.cpp:281
        }
        stop = k_stop >= 0; done_iters = it0 + (stop ? k_stop + 1 : cnt);
    }
    // a traced call: the loop itself over the downloaded counts
    int consume_trace(const RansacBuf& B, int it0, int cnt) {
        const TriView t{B.h_tri, packed};
        int batch_best = -1;
        for (int j = 0; j < cnt; ++j) {
            done_iters = it0 + j + 1;
            if (!t.valid(j)) { trace[it0 + j] = -1; continue; }
            const int inl = trace[it0 + j] = B.h_cnt[j];
            const float fitness = static_cast<float>(inl) / static_cast<float>((size_t)ns);  // registration.cpp:281
            if (fitness > best_fitness) { best_fitness = fitness; best_iter = it0 + j; best_inliers = inl; batch_best = j; }
            if (fitness > confidence) { stop = true; break; }
        }
        if (batch_best >= 0)    // keep the winning (R,t) of this batch (its hyp is not overwritten before the batch after the next is enqueued)
            TDV_HIP(ctx, hipMemcpy2DAsync(d->best12, 4, B.hyp + batch_best, (size_t)h_pad * 4, 4, 12, hipMemcpyDeviceToDevice, s));
        return TDV_OK;
    }
    // RansacStage, the host's side.  Where the call stages, the coarse level of a bounded batch n carries batch n + 1's triples to
    // the device, so batch n + 1 is drawn before batch n is enqueued: the host draws two batches ahead of the one it waits for,
    // into three pinned slots in rotation.
    //  - The slot is fully drawn before the kernel that reads it is enqueued: draw() is host code that has returned.
    //  - Batch m is drawn into slot m mod 3 in front of enqueue(m - 1), which follows wait_batch(m - 3).  The slot's last readers
    //    - batch m - 3's own k_ransac_hypotheses, or batch m - 4's coarse level - ran in front of batch m - 3's record.
    //  - The device buffer that batch n's coarse level writes was batch n - 1's: stream order protects it (bound()).
    //  - An early stop leaves a batch drawn and perhaps staged that never runs: the staging kernel may still be reading the slot
    //    when loop() returns, and ransac_run_dev's synchronise on every way out covers it as it covers a speculative batch.
    //  - Nothing of this survives the call: slots, counters and flags are RansacRun's, a call's first batch is never staged.
    // A batch is staged iff the call stages and the batch before it is bounded: not the first (it0 == 0), and not the second, which
    // stands behind the unbounded first.
    int enqueue_next(TripleStream& idx, int q, const RansacDrawn& dn, bool staged, RansacDrawn& ahead, bool& has_ahead) {
        has_ahead = stage && k.bound && dn.it0 != 0 && dn.it0 + dn.cnt < max_iterations;
        if (has_ahead) ahead = draw(idx);
        return enqueue(q, dn, staged, has_ahead ? &ahead : nullptr);
    }
    int loop(uint32_t seed) {
        TripleStream idx(seed, (uint64_t)ns);   // sequential over the whole run (registration.cpp:235-239)
        int cur = 0;
        RansacDrawn dc = draw(idx), ahead = {}; bool has_ahead = false;
        TDV_TRY(enqueue_next(idx, cur, dc, false, ahead, has_ahead));
        while (dc.cnt > 0 && !stop) {
            const int nxt = cur ^ 1, it_next = dc.it0 + dc.cnt; RansacDrawn dn = {it_next, 0, 0};
            if (it_next < max_iterations) {             // overlap: draw and enqueue the next batch behind the current one
                const bool staged = has_ahead;          // (drawn when the current batch was enqueued, and carried by its coarse level)
                dn = staged ? ahead : draw(idx);
                TDV_TRY(enqueue_next(idx, nxt, dn, staged, ahead, has_ahead));
            } else if (has_pending) TDV_TRY(finish_pending());      // (merged dispatch) the last batch's phase 2 runs alone
            const RansacBuf& B = buf[cur];
            TDV_TRY(wait_batch(B));
            if (trace ? h->bad : B.h_rec[3]) { std::snprintf(ctx->err, sizeof(ctx->err), "ransac: a correspondence index lies outside [0, %d)", nt); return TDV_ERR_BAD_ARG; }
            if (trace) TDV_TRY(consume_trace(B, dc.it0, dc.cnt));
            else consume_record(B, dc.it0, dc.cnt);
            n_staged += B.staged ? 1 : 0;
            cur = nxt; dc = dn;
        }
        return TDV_OK;
    }

    // TDV_TIMER_RANSAC_SCORE from the stamps: every dispatch of k_ransac_score_fast the call enqueued counts as a launch, and adds its
    // last workgroup's end minus its first workgroup's start, in ticks of the constant-rate clock
    int read_stamps() {
        if (!ctx->wall_clock_khz) TDV_HIP(ctx, hipDeviceGetAttribute(&ctx->wall_clock_khz, hipDeviceAttributeWallClockRate, ctx->device));
        unsigned long long ticks = 0ull;
        for (int e = 0; e < stamps_used; ++e) if (h_stamps[n_stamps + e] > h_stamps[e]) ticks += h_stamps[n_stamps + e] - h_stamps[e];
        TimerSlot& t = ctx->timers[TDV_TIMER_RANSAC_SCORE];
        if (ctx->wall_clock_khz > 0) t.total_ms += (double)ticks / (double)ctx->wall_clock_khz;
        t.launches += stamps_used;
        return TDV_OK;
    }

    // ---- the result: the winner's rmse, then the block comes back in one copy - winning hypothesis, its error sum and count, the
    // fast pass' statistics ((wave, chunk) pairs scored twice / scored - the FMA kernel counts the latter itself: the bail-out
    // leaves chunks out - and the scored share of all pairs)
    int result(tdv_ransac_result* out) {
        out->iterations_run = done_iters;
        const bool want_stats = k.score_fast && wave_chunks > 0.0;
        if (best_iter >= 0) {
            k_ransac_rmse_partial<<<rblocks, 256, 0, s>>>(pq, ns, d->best12, tau, slabs);
            k_ransac_rmse_final<<<1, 256, 0, s>>>(slabs, rblocks, d->out2);
            TDV_CHECK_LAUNCH(ctx);
        }
        if (best_iter >= 0 || want_stats) {
            if (stamps_used) TDV_HIP(ctx, hipMemcpyAsync(h_stamps, stamps, (size_t)n_stamps * 16, hipMemcpyDeviceToHost, s));
            TDV_HIP(ctx, hipMemcpyAsync(h, d, kRansacReadBack, hipMemcpyDeviceToHost, s)); TDV_HIP(ctx, hipStreamSynchronize(s));
            if (stamps_used) TDV_TRY(read_stamps());
        }
        if (want_stats) {
            const double scored = h->scored ? (double)h->scored : wave_chunks;
            ctx->last_ransac_rescore = (double)h->rescored / (scored * (k.score_mfma ? 1.0 : (double)(RS_PCH / 2)));      // the FMA kernel counts point pairs scored twice, the matrix-core study kernel chunks
            ctx->last_ransac_scored = scored / wave_chunks;
        }
        if (best_iter >= 0 || want_stats) for (int e = 0; e < 4; ++e) ctx->last_ransac_bound[e] = h->bound[e];
        if (best_iter < 0) return TDV_OK;
        pose_to_T16(h->best12, out->T);
        out->fitness = best_fitness; out->inliers = best_inliers; out->best_iteration = best_iter;
        // registration.cpp:282 (float total_error / int inliers)
        out->rmse = best_inliers > 0 ? std::sqrt((float)h->out2[0] / (float)best_inliers) : 999.0f;
        if ((int)(h->out2[1] + 0.5) != best_inliers) {
            snprintf(ctx->err, sizeof(ctx->err), "ransac: rmse pass counted %d inliers, scoring pass %d", (int)(h->out2[1] + 0.5), best_inliers);
            return TDV_ERR_INTERNAL;
        }
        return TDV_OK;
    }
};

int ransac_run_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* d_fs, const float* d_ft, const int* d_corr_in,
                   float voxel, int max_iterations, float confidence, uint32_t seed, tdv_ransac_result* out, int* trace_inliers) {
    if (!ctx || !out || ns < 0 || nt < 0 || max_iterations < 0) return TDV_ERR_BAD_ARG;
    if (ns > 0 && (!d_src || !d_tgt)) return TDV_ERR_BAD_ARG;
    if (!d_corr_in && ns > 0 && nt > 0 && (!d_fs || !d_ft)) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipSetDevice(ctx->device));
    result_defaults(out);
    if (ns == 0 || nt == 0 || max_iterations == 0) return TDV_OK;  // uniform_int over an empty range is UB in the reference
    int* d_match = nullptr;
    if (!d_corr_in) { TDV_TRY(ws_alloc(ctx, (size_t)ns, &d_match)); TDV_TRY(feature_match_dev(ctx, d_fs, ns, d_ft, nt, d_match)); }
    const int* d_corr = d_corr_in ? d_corr_in : d_match;
    RansacRun r;
    r.ctx = ctx; r.s = ctx->stream; r.k = ransac_knobs(ctx, trace_inliers != nullptr, max_iterations, ns);
    r.ns = ns; r.nt = nt; r.max_iterations = max_iterations; r.confidence = confidence; r.trace = trace_inliers;
    r.tau = tau_lt(voxel * 1.5f);  // registration.cpp:213
    // sqrt(tau) rounded up: the boundary of `d2 < tau` in distance, for the band of the fast scoring pass
    r.sqrt_tau = std::nextafter((float)std::sqrt((double)r.tau), INFINITY);
    r.band_u = r.k.score_mfma ? kBandUnitMatrix : kBandUnit;
    TDV_TRY(r.setup(d_src, d_tgt, d_corr));
    const int status = r.loop(seed);
    (void)hipStreamSynchronize(r.s);   // a speculative batch may still be in flight after an early exit
    ctx->last_ransac_rescore = -1.0; ctx->last_ransac_scored = 1.0;
    for (long long& v : ctx->last_ransac_bound) v = 0;
    ctx->last_ransac_staged = r.n_staged;
    r.release_events();
    return status != TDV_OK ? status : r.result(out);
}


// ---- many small clouds against one target: the whole coarse alignment in a handful of launches (round 3) ---------------------
// A batch of small instances (config C5: 1,024 clouds of ~400 voxels, 10,000 hypotheses each) is bound by what ransac_run_dev
// does on the HOST per call - 30,000 index draws, a dozen launches, two synchronisations - not by its kernels.  Here:
//   k_rb_sample      the reference's index stream on the device.  mt19937(42)'s raw outputs are the same for every cloud (the host
//                    draws them once per call); only libstdc++'s Lemire mapping to [0, n) depends on the cloud.  A workgroup per
//                    cloud maps the raw draws 1,024 at a time and compacts away the rejected ones (probability n / 2^32 each) with
//                    a workgroup scan, so a rejection shifts everything after it exactly as the sequential loop does.
//   k_rb_gather_pq   the (point, matched target) pairs of all clouds, each cloud padded to whole scoring chunks; k_pack_pq2 as usual
//   k_rb_hypotheses  one lane per (cloud, iteration): the lane function of k_ransac_hypotheses
//   k_rb_score       one workgroup per (cloud, 1,024 hypotheses): score_range_fast over all the cloud's chunks
//   k_rb_select      one workgroup per cloud: the loop of registration.cpp:281-290 as two reductions - the first iteration
//                    whose fitness passes the confidence bounds the prefix, then the first largest fitness inside it.
// Index stream, transforms, counts and the winner are ransac_run_dev's (tests/test_gpu_c5.py and test_gpu_chain.py hold the batch
// against the operator chain bit for bit).  The winner's rmse is not evaluated: the batch does not report it.
struct RbResult { float T[12]; int best_iter, inliers, iterations_run, pad; };

__global__ __launch_bounds__(1024)
void k_rb_sample(const unsigned* __restrict__ raw, int n_raw, const int* __restrict__ off, int H, int* __restrict__ idx_out /* [clouds][3 H] */, int* __restrict__ fail) {
    const int b = blockIdx.x, n = off[b + 1] - off[b];
    if (n <= 0) return;
    const unsigned range = (unsigned)n, thr = (0u - range) % range;        // libstdc++ 11 uniform_int_distribution (Lemire), see ctx.hip
    int* out = idx_out + (size_t)b * 3 * H;
    __shared__ int s_wave[16];
    __shared__ int s_produced;
    if (threadIdx.x == 0) s_produced = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r0 = 0; r0 < n_raw; r0 += 1024) {
        const int produced = s_produced;
        if (produced >= 3 * H) break;                                      // workgroup-uniform
        const int r = r0 + threadIdx.x;
        unsigned long long prod = 0ull; bool acc = false;
        if (r < n_raw) { prod = (unsigned long long)raw[r] * (unsigned long long)range; acc = !((unsigned)prod < thr); }
        const unsigned long long m = __ballot(acc);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 16; ++w) { if (w < wave) before += s_wave[w]; total += s_wave[w]; }
        const int q = produced + before + __popcll(m & ((1ull << lane) - 1ull));
        if (acc && q < 3 * H) out[q] = (int)(prod >> 32);
        __syncthreads();
        if (threadIdx.x == 0) s_produced = produced + total;
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_produced < 3 * H) *fail = 1;                  // ran out of raw draws (cannot happen with the slack the host adds)
}

// pos_off[b]: first padded pair slot of cloud b (multiples of 2 RS_PCH); grid over all padded slots
__global__ void k_rb_gather_pq(const float* __restrict__ src, const float* __restrict__ tgt, const int* __restrict__ corr, const int* __restrict__ off,
                               const int* __restrict__ pos_off, int n_clouds, int total_pos, int nt, float* __restrict__ pq, int* __restrict__ bad,
                               unsigned* __restrict__ pmax /* [clouds] */) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= total_pos) return;
    int a = 0, z = n_clouds;
    while (z - a > 1) { const int m = (a + z) >> 1; if (pos_off[m] <= pos) a = m; else z = m; }
    const int i = pos - pos_off[a], n = off[a + 1] - off[a];
    float4 A, Bq;
    if (i < n) {
        const float am = pair_record(src, tgt, corr, (size_t)off[a] + i, nt, bad, A, Bq);
        if (am > 0.f) atomicMax(&pmax[a], __float_as_uint(am));
    } else pair_record_padding(A, Bq);
    reinterpret_cast<float4*>(pq)[2 * (size_t)pos] = A;
    reinterpret_cast<float4*>(pq)[2 * (size_t)pos + 1] = Bq;
}

__global__ void k_rb_hypotheses(const float* __restrict__ pq, const int* __restrict__ pos_off, const int* __restrict__ off, const int* __restrict__ idx /* [clouds][3 H] */,
                                int H, int h_pad, float* __restrict__ hyp /* [clouds][14][h_pad] */, const unsigned* __restrict__ pmax, float sqrt_tau, float band_u) {
    const int b = blockIdx.y, h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= h_pad || off[b + 1] == off[b]) return;
    bool valid = false;
    int4 tr = make_int4(0, 0, 0, 0);
    if (h < H) {
        const int* t = idx + (size_t)b * 3 * H + 3 * (size_t)h;
        tr = make_int4(t[0], t[1], t[2], 0);
        valid = !(tr.x == tr.y || tr.y == tr.z || tr.x == tr.z);           // registration.cpp:240
    }
    ransac_hypothesis_lane(pq + (size_t)pos_off[b] * 8, tr, valid, h, h_pad, hyp + (size_t)b * 14 * h_pad, pmax + b, sqrt_tau, band_u);
}

__global__ __launch_bounds__(RS_BLOCK)
void k_rb_score(const float* __restrict__ hyp, int h_pad, const float* __restrict__ pq2, const int* __restrict__ pos_off, const int* __restrict__ off, float tau,
                int* __restrict__ counts /* [clouds][h_pad] */, unsigned long long* __restrict__ rescored /* [0] chunks scored twice, [1] chunks scored (per wave) */) {
    // consecutive workgroup ids = consecutive clouds of ONE hypothesis block: a cloud's 10 blocks land on the same XCD (id mod 8 =
    // cloud mod 8), so its pair records are pulled into one L2 only, and stay there for the next block
    const int b = blockIdx.x;
    if (off[b + 1] == off[b]) return;
    const int base = blockIdx.y * RS_BLOCK + threadIdx.x;
    const int chunks = (pos_off[b + 1] - pos_off[b]) / RS_PCH;
    unsigned n_rescored = 0;
    const int cnt = score_range_fast<true>(hyp + (size_t)b * 14 * h_pad, h_pad, base, pq2 + (size_t)pos_off[b] * 6, 0, chunks, tau, n_rescored);
    counts[(size_t)b * h_pad + base] = cnt;
    score_stats(n_rescored, chunks, rescored);
}

__global__ __launch_bounds__(256)
void k_rb_select(const int* __restrict__ idx, const int* __restrict__ counts, const float* __restrict__ hyp, const int* __restrict__ off, int H, int h_pad,
                 float confidence, RbResult* __restrict__ res) {
    const int b = blockIdx.x, n = off[b + 1] - off[b];
    RbResult* r = res + b;
    if (n <= 0) { if (threadIdx.x == 0) { r->best_iter = -1; r->inliers = 0; r->iterations_run = 0; } return; }
    const int* t = idx + (size_t)b * 3 * H;
    const int* c = counts + (size_t)b * h_pad;
    const float fn = static_cast<float>((size_t)n);
    __shared__ int s_stop;
    __shared__ unsigned long long s_best[4];
    if (threadIdx.x == 0) s_stop = H;
    __syncthreads();
    // the first iteration whose fitness passes the confidence ends the loop (registration.cpp:290)
    int stop = H;
    for (int h = threadIdx.x; h < H; h += 256) {
        const bool valid = !(t[3 * h] == t[3 * h + 1] || t[3 * h + 1] == t[3 * h + 2] || t[3 * h] == t[3 * h + 2]);
        if (valid && static_cast<float>(c[h]) / fn > confidence) { stop = h; break; }
    }
    atomicMin(&s_stop, stop);
    __syncthreads();
    const int k_end = s_stop < H ? s_stop + 1 : H;
    // the first largest fitness among iterations [0, k_end) (earlier = H - h)
    unsigned long long best = 0ull;
    for (int h = threadIdx.x; h < k_end; h += 256) {
        const bool valid = !(t[3 * h] == t[3 * h + 1] || t[3 * h + 1] == t[3 * h + 2] || t[3 * h] == t[3 * h + 2]);
        if (!valid) continue;
        const float fit = static_cast<float>(c[h]) / fn;                     // registration.cpp:281
        if (!(fit > 0.f)) continue;                                          // has to beat the initial best fitness 0 (:284)
        const unsigned long long key = first_best_key(fit, H - h);
        best = key > best ? key : best;
    }
    best = first_best_wave(best);
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = s_best[w] > best ? s_best[w] : best;
        r->iterations_run = k_end;
        if (best == 0ull) { r->best_iter = -1; r->inliers = 0; }
        else {
            const int h = H - (int)(unsigned)(best & 0xffffffffull);
            r->best_iter = h; r->inliers = c[h];
            const float* hp = hyp + (size_t)b * 14 * h_pad;
            for (int e = 0; e < 12; ++e) r->T[e] = hp[(size_t)e * h_pad + h];
        }
    }
}

int ransac_small_batch_dev(tdv_ctx* ctx, const float* d_src, const int* h_off, const int* d_off, int n_clouds, const float* d_tgt, int nt, const int* d_corr,
                           float voxel, int max_iterations, float confidence, uint32_t seed, tdv_ransac_result* out, int* fell_back) {
    if (!ctx || !h_off || !d_off || !out || !fell_back || n_clouds < 0 || nt < 0 || max_iterations < 0) return TDV_ERR_BAD_ARG;
    *fell_back = 0;
    for (int b = 0; b < n_clouds; ++b) result_defaults(&out[b]);
    const int total = n_clouds ? h_off[n_clouds] : 0;
    if (total == 0 || nt == 0 || max_iterations == 0) return TDV_OK;
    if (!d_src || !d_tgt || !d_corr) return TDV_ERR_BAD_ARG;
    const bool off_env = getenv("TDV_RANSAC_BATCH") && atoi(getenv("TDV_RANSAC_BATCH")) == 0;   // A/B knob (read per call: the tests switch it)
    const bool fast_mode = ctx->ransac_score_mode == TDV_RANSAC_SCORE_FAST && !(getenv("TDV_RANSAC_SCORE") && strcmp(getenv("TDV_RANSAC_SCORE"), "fast"));
    int v_max = 0;
    for (int b = 0; b < n_clouds; ++b) v_max = std::max(v_max, h_off[b + 1] - h_off[b]);
    if (off_env || !fast_mode || v_max > 4096 || max_iterations > 32768) { *fell_back = 1; return TDV_OK; }
    hipStream_t s = ctx->stream;
    const float thr = voxel * 1.5f;  // registration.cpp:213
    const float tau = tau_lt(thr);
    const float sqrt_tau = std::nextafter((float)std::sqrt((double)tau), INFINITY);
    const int H = max_iterations, h_pad = (int)align_up((size_t)H, RS_HYP_PER_BLOCK), hb = h_pad / RS_HYP_PER_BLOCK;
    // padded pair slots per cloud
    std::vector<int> pos_off((size_t)n_clouds + 1, 0);
    for (int b = 0; b < n_clouds; ++b) pos_off[b + 1] = pos_off[b] + (int)align_up((size_t)(h_off[b + 1] - h_off[b]), (size_t)RS_PCH * 2);   // whole chunks of RS_PCH pairs, 64-B aligned records
    const int total_pos = pos_off[n_clouds];
    const int n_raw = 3 * H + 4096;                                            // slack for rejected draws (each has probability n / 2^32)
    int* d_pos_off; unsigned* d_raw; int* d_idx; float *pq, *pq2, *hyp; int* counts; unsigned* d_pmax; int* d_flags; RbResult* d_res;
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds + 1, &d_pos_off));
    TDV_TRY(ws_alloc(ctx, (size_t)n_raw, &d_raw));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds * 3 * H, &d_idx));
    TDV_TRY(ws_alloc(ctx, (size_t)total_pos * 8, &pq));
    TDV_TRY(ws_alloc(ctx, (size_t)total_pos * 6, &pq2));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds * 14 * h_pad, &hyp));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds * h_pad, &counts));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds + 2, &d_pmax));                     // pmax[clouds] | bad | fail
    d_flags = reinterpret_cast<int*>(d_pmax + n_clouds);
    unsigned long long* d_stats;                                               // rescored, scored (their own allocation: 8-byte aligned whatever n_clouds is)
    TDV_TRY(ws_alloc(ctx, 2, &d_stats));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds, &d_res));
    const size_t pin_raw = align_up((size_t)n_raw * 4, 64), pin_res = align_up((size_t)n_clouds * sizeof(RbResult), 64);
    TDV_TRY(pin_reserve(ctx, pin_raw + pin_res + 64 + ((size_t)n_clouds + 1) * 4));
    unsigned* h_raw = reinterpret_cast<unsigned*>(ctx->pin);
    RbResult* h_res = reinterpret_cast<RbResult*>(ctx->pin + pin_raw);
    int* h_flags = reinterpret_cast<int*>(ctx->pin + pin_raw + pin_res);
    int* h_pos = h_flags + 16;
    mt19937_raw(seed, (size_t)n_raw, h_raw);
    std::memcpy(h_pos, pos_off.data(), ((size_t)n_clouds + 1) * 4);
    TDV_HIP(ctx, hipMemcpyAsync(d_raw, h_raw, (size_t)n_raw * 4, hipMemcpyHostToDevice, s));
    TDV_HIP(ctx, hipMemcpyAsync(d_pos_off, h_pos, ((size_t)n_clouds + 1) * 4, hipMemcpyHostToDevice, s));
    TDV_HIP(ctx, hipMemsetAsync(d_pmax, 0, ((size_t)n_clouds + 2) * 4, s));
    TDV_HIP(ctx, hipMemsetAsync(d_stats, 0, 2 * sizeof(unsigned long long), s));
    k_rb_sample<<<n_clouds, 1024, 0, s>>>(d_raw, n_raw, d_off, H, d_idx, d_flags + 1);
    k_rb_gather_pq<<<(total_pos + 255) / 256, 256, 0, s>>>(d_src, d_tgt, d_corr, d_off, d_pos_off, n_clouds, total_pos, nt, pq, d_flags, d_pmax);
    k_pack_pq2<<<(total_pos / 2 + 255) / 256, 256, 0, s>>>(pq, total_pos, pq2);
    k_rb_hypotheses<<<dim3((h_pad + 255) / 256, n_clouds), 256, 0, s>>>(pq, d_pos_off, d_off, d_idx, H, h_pad, hyp, d_pmax, sqrt_tau, kBandUnit);
    {
        ScopedTimer tm(ctx, TDV_TIMER_RANSAC_SCORE);
        k_rb_score<<<dim3(n_clouds, hb), RS_BLOCK, 0, s>>>(hyp, h_pad, pq2, d_pos_off, d_off, tau, counts, d_stats);
    }
    k_rb_select<<<n_clouds, 256, 0, s>>>(d_idx, counts, hyp, d_off, H, h_pad, confidence, d_res);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipMemcpyAsync(h_res, d_res, (size_t)n_clouds * sizeof(RbResult), hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipMemcpyAsync(h_flags, d_flags, 8, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipMemcpyAsync(h_flags + 4, d_stats, 16, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    {
        const unsigned long long* st = reinterpret_cast<const unsigned long long*>(h_flags + 4);
        ctx->last_ransac_rescore = st[1] ? (double)st[0] / ((double)st[1] * (RS_PCH / 2)) : 0.0; ctx->last_ransac_scored = 1.0;      // (pairs scored twice / pairs scored)
    }
    if (h_flags[0]) { std::snprintf(ctx->err, sizeof(ctx->err), "ransac: a correspondence index lies outside [0, %d)", nt); return TDV_ERR_BAD_ARG; }
    if (h_flags[1]) { *fell_back = 1; return TDV_OK; }
    for (int b = 0; b < n_clouds; ++b) {
        const int n = h_off[b + 1] - h_off[b];
        if (n == 0) continue;
        const RbResult& r = h_res[b];
        out[b].iterations_run = r.iterations_run;
        if (r.best_iter < 0) continue;
        pose_to_T16(r.T, out[b].T);
        out[b].inliers = r.inliers; out[b].best_iteration = r.best_iter;
        out[b].fitness = static_cast<float>(r.inliers) / static_cast<float>((size_t)n);
    }
    return TDV_OK;
}

}  // namespace tdv
