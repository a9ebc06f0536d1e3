// Depth scale + mask and depth -> point-cloud unprojection on gfx950 (HBM-bound scans).
//
// Replaces GPUDepth::preprocess (/root/reference/src/gpu_impl.cpp:28-66, kernel
// cuda/depth_processing.cu:10-30) and GPUPointCloud::generate (gpu_impl.cpp:69-128, kernel
// cuda/pointcloud.cu:11-51); results follow the CPU branches src/pipeline.cpp:46-54 and :61-84:
//   depth  = float(raw) * float(1.0/scale), zero where the mask rejects the pixel
//   keep 0 < z <= zmax ; x = (u - cx) * z / fx ; y = (v - cy) * z / fy ; colour = BGR->RGB / 255
// This file: the depth image itself (scale + mask, the bilateral filter, the mask resize).  depth_cloud.hip: one frame -> cloud;
// depth_batch.hip: all instances of a frame; depth_rules.hpp: the per-pixel rules.
#include "depth_rules.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

namespace tdv {

__global__ __launch_bounds__(DP_BLOCK)
void k_depth_preprocess(const uint16_t* __restrict__ raw, const uint8_t* __restrict__ mask, size_t n,
                        float inv_scale, int mask_mode, float* __restrict__ out) {
    // 4 consecutive pixels per lane: 8 B of depth, 4 B of mask in, 16 B out
    size_t i4 = ((size_t)blockIdx.x * DP_BLOCK + threadIdx.x) * 4;
    if (i4 + 3 < n) {
        ushort4 r = *reinterpret_cast<const ushort4*>(raw + i4);
        float4 o = make_float4(scaled_depth(r.x, inv_scale), scaled_depth(r.y, inv_scale), scaled_depth(r.z, inv_scale), scaled_depth(r.w, inv_scale));
        if (mask) {
            uchar4 m = *reinterpret_cast<const uchar4*>(mask + i4);
            if (!mask_keeps(m.x, mask_mode)) o.x = 0.f;
            if (!mask_keeps(m.y, mask_mode)) o.y = 0.f;
            if (!mask_keeps(m.z, mask_mode)) o.z = 0.f;
            if (!mask_keeps(m.w, mask_mode)) o.w = 0.f;
        }
        *reinterpret_cast<float4*>(out + i4) = o;
    } else {
        for (size_t i = i4; i < n; ++i) out[i] = masked_depth(raw, mask, i, inv_scale, mask_mode);
    }
}

// ------------------------------------------------------------------ bilateral depth filter
// Semantics of the reference's (never-called) filter, cuda/depth_processing.cu:62-155: window radius
// int(2 sigma_s + 0.5) clamped to 5; weight expf(d2 * (-0.5/sigma_s^2) + dr^2 * (-0.5/sigma_r^2)); zero depths are
// skipped and stay zero; taps outside the image count as zero; sums run row-major over the window (so results equal the
// CPU restatement's within expf's last bit).
// Design for gfx950 — no LDS tile, no barriers: one wave owns 64 consecutive pixels of ONE image row and streams the
// 2r + 1 rows of its window through registers.  A row of the window is two coalesced loads (the 64 pixels shifted by
// -r, and the 2r pixels that follow); the tap at offset dx is then a lane rotation of that register pair
// (ds_bpermute through the LDS crossbar, no LDS storage).  The spatial term of a tap is wave-uniform (a scalar
// operand); only the range term and the exponential are per lane.
constexpr int BF_MAXR = 5;

__global__ __launch_bounds__(256)
void k_bilateral_rows(const float* __restrict__ depth, float* __restrict__ filtered, int width, int height, int radius,
                      float spatial_scale, float range_scale) {
    const int lane = threadIdx.x & 63;
    const int segments = (width + 63) / 64;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);             // wave-uniform: (row, 64-pixel segment)
    if (seg >= segments * height) return;
    const int row = seg / segments, col0 = (seg - row * segments) * 64;
    const int col = col0 + lane;
    const float mine = col < width ? depth[(size_t)row * width + col] : 0.f;
    float weight_sum = 0.f, value_sum = 0.f;
    for (int oy = -radius; oy <= radius; ++oy) {
        const int r = row + oy;
        const bool row_inside = r >= 0 && r < height;                 // wave-uniform
        // window of this row: pixels col0 - radius ... col0 + 63 + radius as (lo: first 64, hi: the rest)
        const int c_lo = col0 - radius + lane, c_hi = c_lo + 64;
        const float lo = (row_inside && c_lo >= 0 && c_lo < width) ? depth[(size_t)r * width + c_lo] : 0.f;
        const float hi = (row_inside && lane < 2 * radius && c_hi < width) ? depth[(size_t)r * width + c_hi] : 0.f;
        for (int ox = -radius; ox <= radius; ++ox) {
            const int k = lane + ox + radius;                          // position of this lane's tap inside the window
            const float a = __shfl(lo, k & 63, 64), b = __shfl(hi, k & 63, 64);
            const float tap = k < 64 ? a : b;
            if (tap <= 0.f) continue;                                  // missing depth (or outside the image)
            const float dr = tap - mine;
            const float w = expf((float)(ox * ox + oy * oy) * spatial_scale + dr * dr * range_scale);
            weight_sum += w;
            value_sum += w * tap;
        }
    }
    if (col < width) filtered[(size_t)row * width + col] = mine <= 0.f ? 0.f : (weight_sum > 0.f ? value_sum / weight_sum : mine);
}

int bilateral_filter_dev(tdv_ctx* ctx, const float* d_in, float* d_out, int w, int h, float sigma_spatial, float sigma_range) {
    if (!ctx || !d_in || !d_out || w < 0 || h < 0 || !(sigma_spatial > 0.f) || !(sigma_range > 0.f)) return TDV_ERR_BAD_ARG;
    if ((size_t)w * h == 0) return TDV_OK;
    const int radius = std::min(BF_MAXR, static_cast<int>(2.0f * sigma_spatial + 0.5f));   // depth_processing.cu:131-136
    const float spatial_scale = -0.5f / (sigma_spatial * sigma_spatial);
    const float range_scale = -0.5f / (sigma_range * sigma_range);
    const long long waves = (long long)((w + 63) / 64) * h;
    ScopedTimer tm(ctx, TDV_TIMER_DEPTH);
    k_bilateral_rows<<<(unsigned)((waves + 3) / 4), 256, 0, ctx->stream>>>(d_in, d_out, w, h, radius, spatial_scale, range_scale);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// cv::resize(mask, resized, depth.size(), 0, 0, cv::INTER_NEAREST) of src/pipeline.cpp:38-41 for B stacked masks: a gather
// through the two index tables of OpenCV's resizeNN (imgproc/src/resize.cpp: x_ofs[x] = min(cvFloor(x * ifx), sw - 1) with
// ifx = 1. / ((double)dw / sw), likewise for rows), which the host computes in double exactly as OpenCV does.
__global__ __launch_bounds__(256)
void k_mask_resize_nn(const uint8_t* __restrict__ src, int sw, int sh, const int* __restrict__ x_ofs, const int* __restrict__ y_ofs,
                      int dw, int dh, uint8_t* __restrict__ dst) {
    const size_t b = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)dw * dh) return;
    const int y = (int)(i / dw), x = (int)(i - (size_t)y * dw);
    dst[b * (size_t)dw * dh + i] = src[b * (size_t)sw * sh + (size_t)y_ofs[y] * sw + x_ofs[x]];
}

static void resize_nn_tables(int sw, int sh, int dw, int dh, int* x_ofs, int* y_ofs) {
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double ifx = 1. / inv_scale_x, ify = 1. / inv_scale_y;
    for (int x = 0; x < dw; ++x) x_ofs[x] = std::min((int)std::floor(x * ifx), sw - 1);
    for (int y = 0; y < dh; ++y) y_ofs[y] = std::min((int)std::floor(y * ify), sh - 1);
}

int mask_resize_nearest_dev(tdv_ctx* ctx, const uint8_t* d_src, int n_masks, int sw, int sh, int dw, int dh, uint8_t* d_dst) {
    if (!ctx || n_masks < 0 || sw <= 0 || sh <= 0 || dw < 0 || dh < 0) return TDV_ERR_BAD_ARG;
    if (n_masks == 0 || (size_t)dw * dh == 0) return TDV_OK;
    if (!d_src || !d_dst) return TDV_ERR_BAD_ARG;
    std::vector<int> tab((size_t)dw + dh);
    resize_nn_tables(sw, sh, dw, dh, tab.data(), tab.data() + dw);
    int* d_tab;
    TDV_TRY(ws_alloc(ctx, tab.size(), &d_tab));
    TDV_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const size_t npx = (size_t)dw * dh;
    k_mask_resize_nn<<<dim3((unsigned)((npx + 255) / 256), n_masks), 256, 0, ctx->stream>>>(d_src, sw, sh, d_tab, d_tab + dw, dw, dh, d_dst);
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));   // tab is a host temporary
    return TDV_OK;
}

int depth_preprocess_dev(tdv_ctx* ctx, const DepthFrames& f, float* d_out) {
    if (!ctx || !f.raw || !d_out || f.w < 0 || f.h < 0) return TDV_ERR_BAD_ARG;
    if (f.n == 0) return TDV_OK;
    const int blocks = (int)((f.n + DP_PX_PER_BLOCK - 1) / DP_PX_PER_BLOCK);
    ScopedTimer tm(ctx, TDV_TIMER_DEPTH);
    k_depth_preprocess<<<blocks, DP_BLOCK, 0, ctx->stream>>>(f.raw, f.masks, f.n, f.inv_scale, f.mask_mode, d_out);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

}  // namespace tdv
