// Study-only probe into the per-lane solvers (device_linalg.hpp), the libm restatement (libm_f32.hpp) and RANSAC's hypothesis lane
// (ransac.hip), for tests/test_gpu_solver_probe.py: one problem per lane, inputs read from global memory - nothing folds at compile
// time -, outputs written to global memory, and every kernel calls the very inline function the product kernels call.  The whole file
// is empty in the product library.
#ifdef TDV_STUDY
#include "tdv_internal.hpp"
#include "device_linalg.hpp"

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

}  // namespace
}  // namespace tdv

extern "C" int tdv_study_probe(tdv_ctx* ctx, int op, long long n, const float* d_in, float* d_out) {
    using namespace tdv;
    if (!ctx || op < 0 || op > 10 || n < 0 || n > (1ll << 31) - 256) return TDV_ERR_BAD_ARG;
    if (n == 0) return TDV_OK;
    if (!d_in || !d_out) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipSetDevice(ctx->device));
    ctx->err[0] = 0;
    TDV_TRY(ws_reset(ctx));
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
