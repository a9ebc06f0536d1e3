// The tail of the calls that keep a subset of a cloud's rows (outlier.hip, iss.hip): after flag[i] (1 = kept) and its exclusive scan pos
// (exclusive_scan_dev), the kept rows in ascending original index.  The kernel and the host function that runs scan and gather.
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

namespace {   // per translation unit, as the kernels that use it

// index, xyz and the rows of one companion array of `width` floats per point (each optional)
__global__ __launch_bounds__(256) void k_gather_flagged(const int* __restrict__ flag, const int* __restrict__ pos, const float* __restrict__ xyz,
                                                        const float* __restrict__ attr, int width, int n, int* __restrict__ index,
                                                        float* __restrict__ out_xyz, float* __restrict__ out_attr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const size_t o = (size_t)pos[i], j = (size_t)i;
    if (index) index[o] = i;
    if (out_xyz) { out_xyz[3 * o] = xyz[3 * j]; out_xyz[3 * o + 1] = xyz[3 * j + 1]; out_xyz[3 * o + 2] = xyz[3 * j + 2]; }
    if (out_attr) for (int w = 0; w < width; ++w) out_attr[(size_t)width * o + w] = attr[(size_t)width * j + w];
}

// The tail itself: pos = exclusive scan of flag and *d_total = the number kept (both on the device), then the kept rows into whichever
// of index, out_xyz and out_attr is asked for.
int compact_flagged(tdv_ctx* ctx, const int* flag, int n, int* pos, int* d_total, const float* xyz, const float* attr, int width, int* index,
                    float* out_xyz, float* out_attr) {
    TDV_TRY(exclusive_scan_dev(ctx, flag, n, pos, d_total));
    if (index || out_xyz || out_attr)
        k_gather_flagged<<<(n + 255) / 256, 256, 0, ctx->stream>>>(flag, pos, xyz, attr, width, n, index, out_xyz, out_attr);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

}  // namespace

}  // namespace tdv
