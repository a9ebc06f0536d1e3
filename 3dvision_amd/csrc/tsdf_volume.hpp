// The TSDF volume as tsdf.hip (T1 to T12, T19 to T23) and tsdf_raycast.hip (T13 to T18, T24, K1 to K3) share it: a voxel, its colour quad, an
// output row, the checks every TSDF entry point makes, the default truncation, the voxel centre beside its inverse, the running mean of
// T5 and T21, and the unit vector of a gradient.
#pragma once
#include "tdv_internal.hpp"
#include "frame_pose.hpp"

namespace tdv {

struct alignas(8) TsdfVoxel { float f, w; };               // (tsdf, weight): 8 bytes, loaded and stored whole
struct alignas(16) TsdfColour { float r, g, b, w; };       // T19 (r, g, b, wc): 16 bytes, loaded and stored whole
struct Row3 { float x, y, z; };                            // a row of a 3-wide output

// the voxels of a volume the checks accept, 0 for one they refuse
inline size_t tsdf_voxels(const tdv_tsdf_volume* v) {
    if (!v || !positive_finite(v->voxel_length)) return 0;
    if (v->nx < 1 || v->nx > TDV_TSDF_MAX_SIDE || v->ny < 1 || v->ny > TDV_TSDF_MAX_SIDE || v->nz < 1 || v->nz > TDV_TSDF_MAX_SIDE) return 0;
    const size_t n = (size_t)v->nx * v->ny * v->nz;
    return n <= (size_t)TDV_TSDF_MAX_VOXELS ? n : 0;
}
inline bool tsdf_params_ok(const tdv_tsdf_params* p) {
    if (!p || !(std::isfinite(p->trunc) && p->trunc >= 0.f) || !(std::isfinite(p->max_weight) && p->max_weight >= 1.f)) return false;
    return positive_finite(p->min_weight) && pose_direction_ok(p->pose_direction);
}
inline bool tsdf_frames_ok(const void* raw, int n_frames, const FrameCamera& cam, const float* poses) {
    if (n_frames < 0 || n_frames > TDV_TSDF_MAX_FRAMES || (n_frames > 0 && (!raw || !poses))) return false;
    return frame_camera_ok(cam, true);
}
// T19: the colour volume of a call that takes one - present and aligned for 16-byte accesses
inline bool tsdf_colour_ok(const float* color) { return color && (reinterpret_cast<uintptr_t>(color) & 15u) == 0; }
// the truncation distance: params.trunc, or by default four voxels
inline float tsdf_trunc(const tdv_tsdf_params& p, const tdv_tsdf_volume& V) { return p.trunc == 0.f ? 4.0f * V.voxel_length : p.trunc; }

// tsdf.hip: tdv_tsdf_integrate_dev after its checks - every frame of the call in one launch, and one read-back only where h_n_updated
// is asked for.  It does not begin a call (call_begin is the entry point's): the tracker calls it per frame.
int tsdf_integrate_frames(tdv_ctx* ctx, const tdv_tsdf_volume& vol, float* d_volume, const uint16_t* d_raw, int n_frames, const FrameCamera& cam,
                          const float* h_poses, const tdv_tsdf_params& params, long long* h_n_updated);

#ifdef __HIPCC__
// T1: the centre of voxel i along an axis; and T14's way back, the grid coordinate of p along that axis (voxel i's centre is at i)
__device__ __forceinline__ float tsdf_centre(float origin, int i, float L) { return origin + ((float)i + 0.5f) * L; }
__device__ __forceinline__ float tsdf_grid_coord(float origin, float p, float L) { return (p - origin) / L - 0.5f; }

// T5 and T21: the mean of `weight` samples, `mean`, with one more sample t
__device__ __forceinline__ float tsdf_running_mean(float mean, float weight, float t) { return (mean * weight + t) / (weight + 1.0f); }
// T22
__device__ __forceinline__ bool tsdf_coloured(const TsdfColour& c) { return c.w > 0.f; }
// one quad: a single 16-byte load (the buffer is 16-byte aligned: tsdf_colour_ok)
__device__ __forceinline__ TsdfColour tsdf_quad(const TsdfColour* __restrict__ a) {
    const float4 q = *reinterpret_cast<const float4*>(a);
    return TsdfColour{q.x, q.y, q.z, q.w};
}

// T8, T18, O3: n / |n|, or zeros when the length is 0, infinite or NaN; unit (optional): which of the two it was
__device__ __forceinline__ Row3 normalized_or_zero(float n0, float n1, float n2, bool* unit = nullptr) {
    const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    const bool ok = len > 0.f && len < INFINITY;           // (false for NaN)
    if (unit) *unit = ok;
    return ok ? Row3{n0 / len, n1 / len, n2 / len} : Row3{0.f, 0.f, 0.f};
}
#endif

}  // namespace tdv
