// What frame-to-model tracking (tsdf_raycast.hip: tdv_tsdf_track_dev, tdv_tsdf_track_sequence_dev) takes from the two stages it joins:
// tsdf.hip's argument checks and its integrate pass, odometry.hip's checks and its pair against an f32 target depth (O10).  Each is the
// stage's own code behind a name another file can call; none of them begins a call (call_begin is the entry point's).
#pragma once
#include "tdv_internal.hpp"

namespace tdv {

// tsdf.hip: the voxels of a volume the checks accept (0 for one they refuse); the params and the frames as every TSDF entry point checks them
size_t tsdf_voxels(const tdv_tsdf_volume* vol);
bool tsdf_params_ok(const tdv_tsdf_params* params);
bool tsdf_frames_ok(const void* raw, int n_frames, int w, int h, float scale, float fx, float fy, const float* poses);
// tdv_tsdf_integrate_dev after its checks: enqueued, and one read-back only where h_n_updated is asked for
int tsdf_integrate_frames(tdv_ctx* ctx, const tdv_tsdf_volume& vol, float* d_volume, const uint16_t* d_raw, int n_frames, int w, int h,
                          float scale, float fx, float fy, float cx, float cy, const float* h_poses, const tdv_tsdf_params& params,
                          long long* h_n_updated);

// odometry.hip: the camera and the params as every odometry entry point checks them
bool odometry_camera_ok(int w, int h, float scale, float fx, float fy);
bool odometry_params_ok(const tdv_odometry_params* params, int w, int h);
// the start pose (NULL: the identity) with zeros: what a pair without work returns
void odometry_empty_result(const float* h_T0, tdv_odometry_result* out);
// tdv_depth_odometry_to_depth_dev after its checks (width*height > 0): the raw source frame against the f32 target depth, one read-back
int odometry_pair_to_depth(tdv_ctx* ctx, const uint16_t* d_raw_src, const float* d_depth_tgt, int w, int h, float scale, float fx, float fy,
                           float cx, float cy, const float* h_T0, const tdv_odometry_params& params, tdv_odometry_result* out);

// O9's product C = A * B of two column-major poses: each entry the f64 sum of four f64 products in index order, rounded once to f32
inline void pose_chain_product(const float* A, const float* B, float* Cm) {
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            double acc = (double)A[i] * (double)B[4 * j];
            for (int q = 1; q < 4; ++q) acc = acc + (double)A[4 * q + i] * (double)B[4 * j + q];
            Cm[4 * j + i] = (float)acc;
        }
}

}  // namespace tdv
