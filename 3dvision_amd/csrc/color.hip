// Colour gradients of a cloud for colored ICP (include/tdv_hip.h: tdv_color_gradients; Park, Zhou, Koltun, ICCV 2017, as Open3D's
// registration_colored_icp forms them): per point the intensity I and the gradient d of I on the point's tangent plane, fitted by
// least squares to its kNN neighbours' intensity differences.  One thread per point walks its neighbour list in list order and sums
// the 3x3 normal equations in f64, so the result does not depend on the launch shape.
#include "tdv_internal.hpp"
#include <cmath>

namespace tdv {

namespace {

constexpr int CG_BLOCK = 256;

__device__ __forceinline__ float intensity(const float* __restrict__ rgb, size_t i) {
    return ((rgb[3 * i] + rgb[3 * i + 1]) + rgb[3 * i + 2]) / 3.0f;
}

// out[4 i .. 4 i + 3] = (I_i, d_i) for every point i; knn: int[n * k], point i's list at i * k, -1 padded (self and pads are skipped)
__global__ __launch_bounds__(CG_BLOCK)
void k_color_gradients(const float* __restrict__ xyz, const float* __restrict__ rgb, const float* __restrict__ normals, int n,
                       const int* __restrict__ knn, int k, float* __restrict__ out) {
    const int i = blockIdx.x * CG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float Ii = intensity(rgb, (size_t)i);
    const float qx = xyz[3 * (size_t)i], qy = xyz[3 * (size_t)i + 1], qz = xyz[3 * (size_t)i + 2];
    const float nx = normals[3 * (size_t)i], ny = normals[3 * (size_t)i + 1], nz = normals[3 * (size_t)i + 2];
    double S00 = 0.0, S01 = 0.0, S02 = 0.0, S11 = 0.0, S12 = 0.0, S22 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
    int m = 0;
    const int* __restrict__ L = knn + (size_t)i * k;
#pragma unroll 1
    for (int r = 0; r < k; ++r) {
        const int j = L[r];
        if (j < 0 || j == i) continue;
        // u = (q_j - q) - ((q_j - q) . n) n, b = I_j - I_i in f32; their products summed in f64 (exact: products of two f32)
        const float dx = xyz[3 * (size_t)j] - qx, dy = xyz[3 * (size_t)j + 1] - qy, dz = xyz[3 * (size_t)j + 2] - qz;
        const float t = dx * nx + (dy * ny + dz * nz);
        const double u0 = dx - t * nx, u1 = dy - t * ny, u2 = dz - t * nz;
        const double b = intensity(rgb, (size_t)j) - Ii;
        S00 += u0 * u0; S01 += u0 * u1; S02 += u0 * u2; S11 += u1 * u1; S12 += u1 * u2; S22 += u2 * u2;
        c0 += u0 * b; c1 += u1 * b; c2 += u2 * b;
        ++m;
    }
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (m >= 3) {
        // A = S + m^2 n n^T (Open3D's tangent row m n), solved by cofactors in f64
        const double mm = (double)m * (double)m, N0 = nx, N1 = ny, N2 = nz;
        const double A00 = S00 + (mm * N0) * N0, A01 = S01 + (mm * N0) * N1, A02 = S02 + (mm * N0) * N2;
        const double A11 = S11 + (mm * N1) * N1, A12 = S12 + (mm * N1) * N2, A22 = S22 + (mm * N2) * N2;
        const double C00 = A11 * A22 - A12 * A12, C11 = A00 * A22 - A02 * A02, C22 = A00 * A11 - A01 * A01;
        const double C01 = A02 * A12 - A01 * A22, C02 = A01 * A12 - A02 * A11, C12 = A01 * A02 - A00 * A12;
        const double det = A00 * C00 + (A01 * C01 + A02 * C02);
        if (det > 0.0 && det < INFINITY) {
            d0 = (float)((C00 * c0 + (C01 * c1 + C02 * c2)) / det);
            d1 = (float)((C01 * c0 + (C11 * c1 + C12 * c2)) / det);
            d2 = (float)((C02 * c0 + (C12 * c1 + C22 * c2)) / det);
        }
    }
    float* __restrict__ o = out + 4 * (size_t)i;
    o[0] = Ii; o[1] = d0; o[2] = d1; o[3] = d2;
}

}  // namespace

int color_gradients_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, const float* d_normals, int n, int k, const int* d_knn,
                        float* d_color) {
    if (!ctx || n < 0 || k <= 0 || k > 255 || (n > 0 && (!d_xyz || !d_rgb || !d_normals || !d_color))) return TDV_ERR_BAD_ARG;
    if (n == 0) return TDV_OK;
    if (!d_knn) {   // the exact kNN lists of tdv_estimate_normals (its normals are discarded: the caller's are used)
        float* scratch_normals; int* lists;
        TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &scratch_normals));
        TDV_TRY(ws_alloc(ctx, (size_t)n * k, &lists));
        TDV_TRY(estimate_normals_dev(ctx, d_xyz, n, k, scratch_normals, lists));
        d_knn = lists;
    }
    k_color_gradients<<<(n + CG_BLOCK - 1) / CG_BLOCK, CG_BLOCK, 0, ctx->stream>>>(d_xyz, d_rgb, d_normals, n, d_knn, k, d_color);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

}  // namespace tdv
