// Study-only probe into the per-lane solvers (device_linalg.hpp), the libm restatement (libm_f32.hpp) and RANSAC's hypothesis lane
// (ransac.hip), for tests/test_gpu_solver_probe.py: one problem per lane, inputs read from global memory - nothing folds at compile
// time -, outputs written to global memory, and every kernel calls the very inline function the product kernels call.  The whole file
// is empty in the product library.
//
// A second entry point, tdv_study_primitive, reaches the shared device primitives underneath the stages for
// tests/test_gpu_primitives_probe.py: the exclusive scan and the bitonic record sorts (sort.hip), the gather tail of outlier and ISS
// (flag_gather.hpp) and the fixed f64 tree (fixed_tree.hpp).  Each op calls the very function the product paths call and adds no logic
// of its own - but for the tree ops' term-to-thread assignment, which is the header's: term i belongs to workgroup i / 256, thread i % 256.
#ifdef TDV_STUDY
#include <vector>
#include "tdv_internal.hpp"
#include "device_linalg.hpp"
#include "fixed_tree.hpp"
#include "flag_gather.hpp"

// Not part of include/tdv_hip.h: the study library alone exports it.  d_in / d_out are device pointers, n problems back to back:
//   op                      floats in                                    floats out
//   0  dl::svd3             9   A, column-major                          21  U, V (column-major), s0 s1 s2
//   1  dl::kabsch_rotation  9   H, column-major                          9   R, column-major
//   2  dl::smallest_eigvec3 6   a00 a10 a20 a11 a21 a22                  4   vx vy vz, ok (1.0 / 0.0)
//   3  dl::ldlt6_solve      42  A row-major (36), b (6)                  6   x
//   4  dl::euler_xyz        3   a b g                                    9   R, column-major
//   5  dl::mul44            32  A, B column-major                        16  A * B
//   6  lm::sinf_glibc       1                                            1
//   7  lm::cosf_glibc       1                                            1
//   8  lm::atanf_glibc      1                                            1
//   9  lm::atan2f_glibc     2   y x                                      1
//   10 ransac_hypothesis_lane   24: three records px py pz qx qy qz 0 0  12  rows 0-11 of hyp: R column-major, t
// Runs on the ctx stream and returns once the results are there.  TDV_ERR_BAD_ARG for an unknown op, n < 0 or a NULL pointer with
// n > 0; n == 0 does nothing.
extern "C" int tdv_study_probe(tdv_ctx* ctx, int op, long long n, const float* d_in, float* d_out);

// The primitives.  Every pointer is a device pointer; nb = ceil(n / 256):
//   op                  what runs                                      in0               in1          in2             out0              out1             out2                 out3
//   0 exclusive_scan    exclusive_scan_dev(in0, n, out0, out1)         int[n], any int   -            -               int[n]            int[1] total     -                    -
//                                                                      offset
//   1 sort_records      sort_records_dev(out0, n), in place            -                 -            -               uint4[n]          -                -                    -
//   2 segment_sort      segment_sort_records_dev(out0, in0, n)         int[n + 1] starts -            -               uint4[width]      -                -                    -
//                       n segments of a buffer of `width` records
//   3 compact           compact_flagged: exclusive_scan_dev(in0, n,    int[n] flags      float[3n]    float[width n]  int[n] index      float[3n] rows   float[width n] rows  int[1] kept
//                       pos, out3), k_gather_flagged: outlier, ISS     (0 / 1)           xyz, opt.    attr, optional  optional          opt., needs in1  opt., needs in2      optional
//   4 tree_sum          part[width b + a] = tree_block_sum of terms    double[n, width]  -            -               double[nb, width] double[width]    -                    -
//                       [256 b .. 256 b + 255][a]; then out1[a] =                                                     part
//                       tree_partials_sum(part, nb, lds4, width, a)
//   5 tree_count        tree_block_count / tree_partials_count         int[n]            -            -               int[nb]           int[1]           -                    -
//   6 tree_block_max    tree_block_max per workgroup; a thread         double[n]         -            -               double[nb]        -                -                    -
//                       without a term holds NaN (never wins)
// Runs on the ctx stream and returns once the results are there.  TDV_ERR_BAD_ARG before anything is launched: an unknown op; n < 0; a
// required pointer NULL with n > 0 (out1 needs in1 and out2 needs in2 for compact); n not a power of two >= 2,048 (or above 2^26) for
// sort_records; segment starts that are negative, descend, pass `width` or span more than segment_sort_max_len() records (the starts are
// read back to check them: a copy, no launch) or more than 2^22 segments; more than 2^30 items; width outside [1, 64] for compact and tree_sum.  n == 0 does nothing.
extern "C" int tdv_study_primitive(tdv_ctx* ctx, int op, long long n, long long width, const void* in0, const void* in1, const void* in2,
                                   void* out0, void* out1, void* out2, void* out3);

namespace tdv {

int probe_hypotheses_dev(tdv_ctx* ctx, int n, const float* d_in, float* d_out);   // ransac.hip

namespace {

template <int OP>
__global__ void k_probe(const float* __restrict__ in, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (OP == 0) {
        dl::Mat3 A, U, V; float s0, s1, s2;
        for (int k = 0; k < 9; ++k) A.a[k] = in[i * 9 + k];
        dl::svd3(A, U, V, s0, s1, s2);
        float* o = out + i * 21;
        for (int k = 0; k < 9; ++k) { o[k] = U.a[k]; o[9 + k] = V.a[k]; }
        o[18] = s0; o[19] = s1; o[20] = s2;
    } else if constexpr (OP == 1) {
        dl::Mat3 H;
        for (int k = 0; k < 9; ++k) H.a[k] = in[i * 9 + k];
        const dl::Mat3 R = dl::kabsch_rotation(H);
        for (int k = 0; k < 9; ++k) out[i * 9 + k] = R.a[k];
    } else if constexpr (OP == 2) {
        const float* a = in + i * 6;
        float vx, vy, vz;
        const bool ok = dl::smallest_eigvec3(a[0], a[1], a[2], a[3], a[4], a[5], vx, vy, vz);
        float* o = out + i * 4;
        o[0] = vx; o[1] = vy; o[2] = vz; o[3] = ok ? 1.f : 0.f;
    } else if constexpr (OP == 3) {
        float A[36], b[6], x[6];
        for (int k = 0; k < 36; ++k) A[k] = in[i * 42 + k];
        for (int k = 0; k < 6; ++k) b[k] = in[i * 42 + 36 + k];
        dl::ldlt6_solve(A, b, x);
        for (int k = 0; k < 6; ++k) out[i * 6 + k] = x[k];
    } else if constexpr (OP == 4) {
        const dl::Mat3 R = dl::euler_xyz(in[i * 3], in[i * 3 + 1], in[i * 3 + 2]);
        for (int k = 0; k < 9; ++k) out[i * 9 + k] = R.a[k];
    } else if constexpr (OP == 5) {
        float A[16], B[16], Cm[16];
        for (int k = 0; k < 16; ++k) { A[k] = in[i * 32 + k]; B[k] = in[i * 32 + 16 + k]; }
        dl::mul44(A, B, Cm);
        for (int k = 0; k < 16; ++k) out[i * 16 + k] = Cm[k];
    } else if constexpr (OP == 6) {
        out[i] = lm::sinf_glibc(in[i]);
    } else if constexpr (OP == 7) {
        out[i] = lm::cosf_glibc(in[i]);
    } else if constexpr (OP == 8) {
        out[i] = lm::atanf_glibc(in[i]);
    } else {
        out[i] = lm::atan2f_glibc(in[i * 2], in[i * 2 + 1]);
    }
}

template <int OP>
int launch(tdv_ctx* ctx, long long n, const float* d_in, float* d_out) {
    k_probe<OP><<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_in, d_out, n);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// ---- the primitives: the header's term-to-thread assignment (term i: workgroup i / 256, thread i % 256) around fixed_tree.hpp's functions
__global__ __launch_bounds__(256) void k_prim_tree_block(const double* __restrict__ terms, int n, int width, double* __restrict__ part) {
    __shared__ double lds4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    for (int a = 0; a < width; ++a) {
        const double s = tree_block_sum(i < n ? terms[(size_t)width * i + a] : 0.0, lds4);
        if (threadIdx.x == 0) part[(size_t)width * blockIdx.x + a] = s;
    }
}

__global__ __launch_bounds__(256) void k_prim_tree_partials(const double* __restrict__ part, int nb, int width, double* __restrict__ out) {
    __shared__ double lds4[4];
    for (int a = 0; a < width; ++a) {
        const double s = tree_partials_sum(part, nb, lds4, width, a);
        if (threadIdx.x == 0) out[a] = s;
    }
}

__global__ __launch_bounds__(256) void k_prim_count_block(const int* __restrict__ v, int n, int* __restrict__ cnt) {
    __shared__ int ldc4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int c = tree_block_count(i < n ? v[i] : 0, ldc4);
    if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(256) void k_prim_count_partials(const int* __restrict__ cnt, int nb, int* __restrict__ out) {
    __shared__ int ldc4[4];
    const int c = tree_partials_count(cnt, nb, ldc4);
    if (threadIdx.x == 0) out[0] = c;
}

__global__ __launch_bounds__(256) void k_prim_max_block(const double* __restrict__ v, int n, double* __restrict__ out) {
    __shared__ double lds4[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double m = tree_block_max(i < n ? v[i] : tree_nan(), lds4);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// the starts of n segments of a buffer of `records` records, read back and checked before the sort is launched
int segments_ok(tdv_ctx* ctx, const int* d_seg_start, int nseg, long long records, bool* ok) {
    std::vector<int> h((size_t)nseg + 1);
    TDV_HIP(ctx, hipMemcpyAsync(h.data(), d_seg_start, h.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *ok = h[0] >= 0 && (long long)h[nseg] <= records;
    for (int c = 0; c < nseg && *ok; ++c) *ok = h[c + 1] >= h[c] && h[c + 1] - h[c] <= segment_sort_max_len();
    return TDV_OK;
}

}  // namespace
}  // namespace tdv

extern "C" int tdv_study_primitive(tdv_ctx* ctx, int op, long long n, long long width, const void* in0, const void* in1, const void* in2,
                                   void* out0, void* out1, void* out2, void* out3) {
    using namespace tdv;
    if (!ctx || op < 0 || op > 6 || n < 0 || n > (1ll << 30)) return TDV_ERR_BAD_ARG;
    if (n == 0) return TDV_OK;
    const bool pow2 = (n & (n - 1)) == 0;
    switch (op) {                                                     // every refusal before anything is launched
        case 0: if (!in0 || !out0 || !out1) return TDV_ERR_BAD_ARG; break;
        case 1: if (!out0 || !pow2 || n < 2048 || n > (1ll << 26)) return TDV_ERR_BAD_ARG; break;
        case 2: if (!in0 || !out0 || n > (1ll << 22) || width < 0 || width > (1ll << 30)) return TDV_ERR_BAD_ARG; break;
        case 3: if (!in0 || width < 1 || width > 64 || (out1 && !in1) || (out2 && !in2)) return TDV_ERR_BAD_ARG; break;
        case 4: if (!in0 || !out0 || !out1 || width < 1 || width > 64) return TDV_ERR_BAD_ARG; break;
        case 5: if (!in0 || !out0 || !out1) return TDV_ERR_BAD_ARG; break;
        default: if (!in0 || !out0) return TDV_ERR_BAD_ARG;
    }
    TDV_TRY(call_begin(ctx));
    hipStream_t s = ctx->stream;
    const int ni = (int)n, nb = (ni + 255) / 256;
    switch (op) {
        case 0:
            TDV_TRY(exclusive_scan_dev(ctx, static_cast<const int*>(in0), ni, static_cast<int*>(out0), static_cast<int*>(out1)));
            break;
        case 1:
            TDV_TRY(sort_records_dev(ctx, static_cast<uint4*>(out0), (size_t)n));
            break;
        case 2: {
            bool ok = false;
            TDV_TRY(segments_ok(ctx, static_cast<const int*>(in0), ni, width, &ok));
            if (!ok) return TDV_ERR_BAD_ARG;
            TDV_TRY(segment_sort_records_dev(ctx, static_cast<uint4*>(out0), static_cast<const int*>(in0), ni));
            break;
        }
        case 3: {
            int *pos, *kept = static_cast<int*>(out3);
            TDV_TRY(ws_alloc(ctx, (size_t)n, &pos));
            if (!kept) TDV_TRY(ws_alloc(ctx, 1, &kept));
            TDV_TRY(compact_flagged(ctx, static_cast<const int*>(in0), ni, pos, kept, static_cast<const float*>(in1), static_cast<const float*>(in2),
                                    (int)width, static_cast<int*>(out0), static_cast<float*>(out1), static_cast<float*>(out2)));
            break;
        }
        case 4:
            k_prim_tree_block<<<nb, 256, 0, s>>>(static_cast<const double*>(in0), ni, (int)width, static_cast<double*>(out0));
            k_prim_tree_partials<<<1, 256, 0, s>>>(static_cast<const double*>(out0), nb, (int)width, static_cast<double*>(out1));
            TDV_CHECK_LAUNCH(ctx);
            break;
        case 5:
            k_prim_count_block<<<nb, 256, 0, s>>>(static_cast<const int*>(in0), ni, static_cast<int*>(out0));
            k_prim_count_partials<<<1, 256, 0, s>>>(static_cast<const int*>(out0), nb, static_cast<int*>(out1));
            TDV_CHECK_LAUNCH(ctx);
            break;
        default:
            k_prim_max_block<<<nb, 256, 0, s>>>(static_cast<const double*>(in0), ni, static_cast<double*>(out0));
            TDV_CHECK_LAUNCH(ctx);
    }
    TDV_HIP(ctx, hipStreamSynchronize(s));
    return TDV_OK;
}

extern "C" int tdv_study_probe(tdv_ctx* ctx, int op, long long n, const float* d_in, float* d_out) {
    using namespace tdv;
    if (!ctx || op < 0 || op > 10 || n < 0 || n > (1ll << 31) - 256) return TDV_ERR_BAD_ARG;
    if (n == 0) return TDV_OK;
    if (!d_in || !d_out) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    switch (op) {
        case 0: TDV_TRY(launch<0>(ctx, n, d_in, d_out)); break;
        case 1: TDV_TRY(launch<1>(ctx, n, d_in, d_out)); break;
        case 2: TDV_TRY(launch<2>(ctx, n, d_in, d_out)); break;
        case 3: TDV_TRY(launch<3>(ctx, n, d_in, d_out)); break;
        case 4: TDV_TRY(launch<4>(ctx, n, d_in, d_out)); break;
        case 5: TDV_TRY(launch<5>(ctx, n, d_in, d_out)); break;
        case 6: TDV_TRY(launch<6>(ctx, n, d_in, d_out)); break;
        case 7: TDV_TRY(launch<7>(ctx, n, d_in, d_out)); break;
        case 8: TDV_TRY(launch<8>(ctx, n, d_in, d_out)); break;
        case 9: TDV_TRY(launch<9>(ctx, n, d_in, d_out)); break;
        default:
            if (n > (1 << 24)) return TDV_ERR_BAD_ARG;         // its workspace is 14 floats per problem; the tests use 1e5
            TDV_TRY(probe_hypotheses_dev(ctx, (int)n, d_in, d_out));
    }
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TDV_OK;
}
#endif  // TDV_STUDY
