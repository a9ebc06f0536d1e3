// The five per-pixel rules of the reference's depth -> cloud stage (src/pipeline.cpp:46-84), each stated once; every depth kernel calls
// these.  The fast forms that restate a rule for many pixels at once (range_bits16, MaskRule / keep_bits16, div_by_uniform:
// depth_batch.hip) name the rule they restate.
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

constexpr int DP_BLOCK = 256;
constexpr int DP_PX_PER_THREAD = 4;
constexpr int DP_PX_PER_BLOCK = DP_BLOCK * DP_PX_PER_THREAD;

// 1. depth in metres
__device__ __forceinline__ float scaled_depth(uint16_t raw, float inv_scale) { return (float)raw * inv_scale; }   // pipeline.cpp:47

// 2. mask rule: reference CPU (> 10, src/pipeline.cpp:51), reference CUDA (!= 0, cuda/depth_processing.cu:22), or
// label image (pixel value == instance label; SURVEY.md 8f N2: one u8 image instead of B full-frame masks)
__device__ __forceinline__ bool mask_keeps(uint8_t m, int mask_mode) {
    if (mask_mode == TDV_MASK_THRESHOLD10) return m > 10;
    if (mask_mode == TDV_MASK_NONZERO) return m != 0;
    return (int)m == mask_mode - TDV_MASK_LABEL_BASE;
}
// ... for instance b of a batch, whose masks come in one of three layouts (depth_frames.hpp)
__device__ __forceinline__ bool instance_mask_keeps(const uint8_t* __restrict__ masks, size_t n, int b, MaskLayout layout, size_t i, int mask_mode) {
    if (layout == MaskLayout::Stacked) return mask_keeps(masks[(size_t)b * n + i], mask_mode);
    if (layout == MaskLayout::LabelU8) return (int)masks[i] == b + 1;
    return (int)reinterpret_cast<const uint16_t*>(masks)[i] == b + 1;
}
// 1 + 2: pixel i of the depth image after masking (pipeline.cpp:46-54), for one frame with an optional mask ...
__device__ __forceinline__ float masked_depth(const uint16_t* __restrict__ raw, const uint8_t* __restrict__ mask, size_t i, float inv_scale, int mask_mode) {
    float v = scaled_depth(raw[i], inv_scale);
    if (mask && !mask_keeps(mask[i], mask_mode)) v = 0.f;
    return v;
}
// ... and for instance b of a batch (raw: the instance's frame)
__device__ __forceinline__ float masked_depth(const uint16_t* __restrict__ raw, const uint8_t* __restrict__ masks, size_t n, int b, MaskLayout layout,
                                              size_t i, float inv_scale, int mask_mode) {
    float v = scaled_depth(raw[i], inv_scale);
    if (!instance_mask_keeps(masks, n, b, layout, i, mask_mode)) v = 0.f;
    return v;
}

// 3. the z clip
__device__ __forceinline__ bool z_valid(float z, float zmax) { return !(z <= 0.f || z > zmax); }   // pipeline.cpp:71

// 4 + 5. the point of pixel (u, v) = pixel i of its frame, at depth z -> xyz[3 slot ...], and, when the frame has colours (bgr not
// null), its colour -> rgb[3 slot ...].
// `div` performs the two divisions by the focal lengths: PlainDiv, or a form proven to give the same quotient (depth_batch.hip).
__device__ __forceinline__ float unit_colour(uint8_t byte) { return (float)byte / 255.0f; }   // pipeline.cpp:78-80
struct PlainDiv {
    float fx, fy;
    __device__ __forceinline__ float by_fx(float a) const { return a / fx; }
    __device__ __forceinline__ float by_fy(float a) const { return a / fy; }
};
template <class Div, class Slot>
__device__ __forceinline__ void emit_point(float u, float v, float z, float cx, float cy, const Div div, float* __restrict__ xyz, float* __restrict__ rgb,
                                           const uint8_t* __restrict__ bgr, Slot slot, size_t i) {
    const float ax = (u - cx) * z, ay = (v - cy) * z;
    const float x = div.by_fx(ax);   // pipeline.cpp:73
    const float y = div.by_fy(ay);   // pipeline.cpp:74
    xyz[3 * slot] = x; xyz[3 * slot + 1] = y; xyz[3 * slot + 2] = z;
    if (bgr) {
        const uint8_t* p = bgr + i * 3;
        rgb[3 * slot] = unit_colour(p[2]); rgb[3 * slot + 1] = unit_colour(p[1]); rgb[3 * slot + 2] = unit_colour(p[0]);   // BGR -> RGB
    }
}

}  // namespace tdv
