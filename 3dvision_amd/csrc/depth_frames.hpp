// What the host functions of every stage that reads depth frames are called with: the pinhole and the camera of a frame with its one
// check (verify*.hip, tsdf*.hip, odometry.hip), and for the depth stage (depth.hip, depth_cloud.hip, depth_batch.hip) the frames and
// their masks as one descriptor and the plan the batched count pass hands to the emit pass.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "tdv_hip.h"

struct tdv_ctx;

namespace tdv {

// How the masks of a batch are laid out; the values are the ABI's mask_format (include/tdv_hip.h, checked by the entry points).
enum class MaskLayout : int {
    Stacked = 0,    // one u8 mask per instance (mask_mode applies)
    LabelU8 = 1,    // ONE u8 label image: instance b keeps the pixels equal to b + 1
    LabelU16 = 2,   // ONE u16 label image (the same rule, for more than 255 instances)
};
inline MaskLayout mask_layout_of(int mask_format) { return static_cast<MaskLayout>(mask_format); }

struct Pinhole { float fx, fy, cx, cy; };

inline bool positive_finite(float v) { return std::isfinite(v) && v > 0.f; }
// raw depth units -> metres, as cv::Mat::convertTo(CV_32F, 1.0/scale) forms the factor: the one place it is formed
inline float depth_inv_scale(float scale) { return (float)(1.0 / (double)scale); }

// The camera of a W x H depth frame as the entry points receive it; scale is 1 where a call has none (a rendering, a ray cast).
struct FrameCamera {
    int w, h;
    float scale;
    Pinhole k;
    size_t npx() const { return (size_t)w * h; }
    float inv_scale() const { return depth_inv_scale(scale); }
};
// what every entry point that takes a frame's camera asks of it: sides in [0, TDV_VERIFY_MAX_SIDE], fx, fy and - where the call has
// one - scale finite and > 0 (cx and cy are free)
inline bool frame_camera_ok(const FrameCamera& c, bool has_scale) {
    if (c.w < 0 || c.w > TDV_VERIFY_MAX_SIDE || c.h < 0 || c.h > TDV_VERIFY_MAX_SIDE) return false;
    return positive_finite(c.k.fx) && positive_finite(c.k.fy) && (!has_scale || positive_finite(c.scale));
}

// n_inst masks (or one label image) over one or several W x H depth frames stored back to back; one frame with an optional mask
// is n_inst = 1, Stacked, frame_of = nullptr.  All pointers are device pointers.
struct DepthFrames {
    const uint16_t* raw;      // frame f starts at raw + f * n
    const int* frame_of;      // instance -> frame (frame_map_dev), nullptr: every instance reads frame 0
    const uint8_t* masks;
    MaskLayout layout;
    int n_inst, w, h;
    size_t n;                 // pixels of a frame
    float inv_scale;
    int mask_mode;
    float zmax;
    DepthFrames(const uint16_t* raw_, const int* frame_of_, const uint8_t* masks_, MaskLayout layout_, int n_inst_, int w_, int h_, float scale, int mask_mode_, float zmax_)
        : raw(raw_), frame_of(frame_of_), masks(masks_), layout(layout_), n_inst(n_inst_), w(w_), h(h_), n((size_t)w_ * h_),
          inv_scale(depth_inv_scale(scale)), mask_mode(mask_mode_), zmax(zmax_) {}
    static DepthFrames one(const uint16_t* raw, const uint8_t* mask, int w, int h, float scale, int mask_mode, float zmax) {
        return DepthFrames(raw, nullptr, mask, MaskLayout::Stacked, 1, w, h, scale, mask_mode, zmax);
    }
};

// What the batched count pass did, for the emit pass to continue: nothing is decided twice.  The pointers are workspace memory of the
// current call.
struct DepthBatchPlan {
    enum Family { TiledBitmap, Scalar, LabelImage } family;
    int blocks;               // tiles (TiledBitmap, LabelImage) resp. workgroups (Scalar) per instance: 1,024 pixels either way
    int* offsets;             // exclusive scan of the (instance, block) counts; the label emit advances them as cursors
    const uint16_t* bits;     // TiledBitmap: the validity bitmap, n / 16 words per instance; else nullptr
};

int depth_preprocess_dev(tdv_ctx* ctx, const DepthFrames& f, float* d_out);
int bilateral_filter_dev(tdv_ctx* ctx, const float* d_in, float* d_out, int w, int h, float sigma_spatial, float sigma_range);
int mask_resize_nearest_dev(tdv_ctx* ctx, const uint8_t* d_src, int n_masks, int sw, int sh, int dw, int dh, uint8_t* d_dst);
// one frame: f.raw (+ mask), or d_depth_f32 when f.raw is null
int depth_to_cloud_dev(tdv_ctx* ctx, const DepthFrames& f, const float* d_depth_f32, const uint8_t* d_bgr, const Pinhole& cam,
                       float* d_xyz, float* d_rgb, int capacity, int* n_out);
int frame_map_dev(tdv_ctx* ctx, int n_inst, int n_frames, const int* h_frame_of, const int** d_frame_of);
// pass 1 (counts + scan): the per-instance start offsets (host, n_inst + 1 entries) and the plan for pass 2
int depth_to_cloud_batch_count(tdv_ctx* ctx, const DepthFrames& f, DepthBatchPlan* plan, int* h_offsets);
// pass 2 (emit) into buffers sized from pass 1
int depth_to_cloud_batch_emit(tdv_ctx* ctx, const DepthFrames& f, const uint8_t* d_bgr, const Pinhole& cam, const DepthBatchPlan& plan,
                              float* d_xyz, float* d_rgb);
int depth_batch_nonzero_any(tdv_ctx* ctx, const DepthFrames& f, const int* h_inst, int n_list, int* h_flags);

}  // namespace tdv
