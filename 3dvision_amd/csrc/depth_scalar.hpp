// The scalar count / emit pair of the depth -> cloud stage: one pixel per lane and step, any frame size and alignment.  Grid =
// (blocks of 1,024 pixels, instances); count leaves one number per (instance, block), the caller scans them, emit writes the points
// in row-major pixel order.  A pixel source tells where a pixel's depth comes from:
//   OneFrameSrc    the study build's three-launch path of one frame (depth_cloud.hip, TDV_DEPTH_THREE_PASS=1)
//   BatchSrc       the batched path for frames the tiled kernels do not take (depth_batch.hip)
#pragma once
#include "depth_rules.hpp"

namespace tdv {

// one frame: u16 (+ optional mask) or an f32 depth image; points past `capacity` are counted and not written
struct OneFrameSrc {
    const uint16_t* raw; const float* depth; const uint8_t* mask; const uint8_t* bgr;
    size_t n; float inv_scale; int mask_mode; float zmax; int capacity;
    __device__ __forceinline__ size_t frame(int) const { return 0; }
    __device__ __forceinline__ float z(size_t, int, size_t i) const {
        return raw ? masked_depth(raw, mask, i, inv_scale, mask_mode) : depth[i];
    }
    __device__ __forceinline__ const uint8_t* colours(size_t) const { return bgr; }
    __device__ __forceinline__ bool fits(size_t slot) const { return slot < (size_t)capacity; }
};

// instance b = blockIdx.y of a batch: its frame through frame_of, its mask by the layout; the buffers were sized from the count
struct BatchSrc {
    const uint16_t* raw0; const int* frame_of; const uint8_t* masks; const uint8_t* bgr0;
    size_t n; MaskLayout layout; float inv_scale; int mask_mode; float zmax;
    __device__ __forceinline__ size_t frame(int b) const { return frame_of ? (size_t)frame_of[b] : 0; }
    __device__ __forceinline__ float z(size_t frame, int b, size_t i) const {
        return masked_depth(raw0 + frame * n, masks, n, b, layout, i, inv_scale, mask_mode);
    }
    __device__ __forceinline__ const uint8_t* colours(size_t frame) const { return bgr0 ? bgr0 + frame * n * 3 : nullptr; }
    __device__ __forceinline__ bool fits(size_t) const { return true; }
};

template <class Src>
__global__ __launch_bounds__(DP_BLOCK)
void k_count(const Src src, int* __restrict__ block_counts) {
    // pixel p of the block = threadIdx.x + k*256 (coalesced), k = 0..3
    const int b = blockIdx.y;
    const size_t frame = src.frame(b);
    const size_t base = (size_t)blockIdx.x * DP_PX_PER_BLOCK;
    int c = 0;
#pragma unroll
    for (int k = 0; k < DP_PX_PER_THREAD; ++k) {
        const size_t i = base + k * DP_BLOCK + threadIdx.x;
        if (i < src.n) c += z_valid(src.z(frame, b, i), src.zmax);
    }
    __shared__ int red[DP_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[(size_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <class Src>
__global__ __launch_bounds__(DP_BLOCK)
void k_emit(const Src src, int width, const Pinhole cam, const int* __restrict__ offsets, float* __restrict__ xyz, float* __restrict__ rgb) {
    const int b = blockIdx.y;
    const size_t frame = src.frame(b);
    const uint8_t* __restrict__ bgr = src.colours(frame);
    const size_t base = (size_t)blockIdx.x * DP_PX_PER_BLOCK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int wcnt[DP_PX_PER_THREAD][DP_BLOCK / 64];
    float zs[DP_PX_PER_THREAD]; bool ok[DP_PX_PER_THREAD]; int rank[DP_PX_PER_THREAD];
#pragma unroll
    for (int k = 0; k < DP_PX_PER_THREAD; ++k) {
        const size_t i = base + k * DP_BLOCK + threadIdx.x;
        float z = 0.f;
        if (i < src.n) z = src.z(frame, b, i);
        ok[k] = (i < src.n) && z_valid(z, src.zmax);
        zs[k] = z;
        const unsigned long long bal = __ballot(ok[k]);
        rank[k] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[k][wave] = __popcll(bal);
    }
    __syncthreads();
    size_t run = (size_t)offsets[(size_t)b * gridDim.x + blockIdx.x];
#pragma unroll
    for (int k = 0; k < DP_PX_PER_THREAD; ++k) {
        int before = 0;
#pragma unroll
        for (int w = 0; w < DP_BLOCK / 64; ++w) before += (w < wave) ? wcnt[k][w] : 0;
        const size_t slot = run + before + rank[k];
        if (ok[k] && src.fits(slot)) {
            const size_t i = base + k * DP_BLOCK + threadIdx.x;
            const int v = (int)(i / width), u = (int)(i - (size_t)v * width);
            emit_point((float)u, (float)v, zs[k], cam.cx, cam.cy, PlainDiv{cam.fx, cam.fy}, xyz, rgb, rgb ? bgr : nullptr, slot, i);
        }
        run += (wcnt[k][0] + wcnt[k][1]) + (wcnt[k][2] + wcnt[k][3]);
    }
}

}  // namespace tdv
