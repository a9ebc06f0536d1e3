// What frame-to-model tracking (tsdf_raycast.hip: tdv_tsdf_track_dev, tdv_tsdf_track_sequence_dev) calls of odometry.hip: its parameter
// check, the result of a pair without work, and the pair itself.  Each is defined once, in odometry.hip, and called there under the same
// name; none of them begins a call (call_begin is the entry point's).  What tracking calls of tsdf.hip is in tsdf_volume.hpp.
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

bool odometry_params_ok(const tdv_odometry_params* params, int w, int h);
// the start pose (NULL: the identity) with zeros: what a pair without work returns
void odometry_empty_result(const float* h_T0, tdv_odometry_result* out);

// A pair's target frame on the device: raw u16 (O1) or, raw == nullptr, an f32 depth image (O10).
struct OdTarget { const uint16_t* raw; const float* depth; };
// A few bytes of the caller's that come down with a pair's records: the read-back places them behind its records in the pinned block,
// copies them in the same enqueue, and writes them to h_dst after its one wait.
struct OdRider { const void* d_src; size_t bytes; void* h_dst; };

// One pair after its checks (cam.npx() > 0): the raw source frame onto the target, one read-back
int odometry_pair(tdv_ctx* ctx, const uint16_t* d_raw_src, const OdTarget& tgt, const FrameCamera& cam, const float* h_T0,
                  const tdv_odometry_params& params, tdv_odometry_result* out, const OdRider* rider = nullptr);

}  // namespace tdv
