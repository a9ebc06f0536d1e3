// What the two renderers of the pose verification share (include/tdv_hip.h: tdv_verify_poses, tdv_verify_poses_mesh): the per-pose record,
// the kernels' camera, rules 1 to 3 (frame_pose.hpp's pose and projection), the tile list and the tail of a tile - rules 5 to 7, the
// classification of the tile's pixels against the raw frame and their reduction into the record.  verify.hip splats points into the
// tile, verify_mesh.hip rasterises triangles; everything around the tile's z-buffer is here, once.  The host part (the poses up, init, plan, the one read-back and wait, the order,
// the render's clear and count) is defined in verify.hip.
#pragma once
#include "tdv_internal.hpp"
#include "frame_pose.hpp"

namespace tdv {

constexpr int VERIFY_VT = TDV_VERIFY_LANES, VERIFY_TW = TDV_VERIFY_TILE_W, VERIFY_TH = TDV_VERIFY_TILE_H, VERIFY_TILE = VERIFY_TW * VERIFY_TH;
constexpr unsigned VERIFY_EMPTY = 0xFFFFFFFFu;              // above the bits of every positive finite f32
constexpr int VERIFY_GRID = 512;                            // 256 CUs x the two workgroups a CU's LDS holds
static_assert(VERIFY_TILE % (4 * VERIFY_VT) == 0 && (VERIFY_TW & (VERIFY_TW - 1)) == 0, "the clear and the pixel walk assume it");

struct VerifyRec {                                          // one per pose (device)
    int n_projected;
    int u0, v0, u1, v1;                                     // the covered pixels' box inside the frame; u0 > u1: none
    int cls[4];                                             // consistent, occluded, violating, unknown (render: cls[0] = rendered)
    int pad;
    unsigned long long err;
};
struct VerifyCam { Pinhole k; float zmax, tau, inv_scale; int w, h, splat, direction; };

// what a call holds on the device and in the pinned staging: the poses, a record per pose, the tile offsets; down: where the records land
struct VerifyStage { float* d_poses; VerifyRec* rec; int* off; char* down; };

// the kernels' camera from the entry point's (tau, splat: 0 where a renderer has none)
inline VerifyCam verify_cam(const FrameCamera& c, float zmax, float tau, int splat, int direction) {
    return VerifyCam{c.k, zmax, tau, c.inv_scale(), c.w, c.h, splat, direction};
}
// the poses up and a fresh record per pose, enqueued (pin: poses up at [0], records down at st->down)
int verify_stage(tdv_ctx* ctx, const float* h_poses, int n_poses, VerifyStage* st);
// k_verify_plan: the tile list of the records' boxes, enqueued
void verify_plan(tdv_ctx* ctx, const VerifyStage& st, int n_poses);
// the records down, enqueued; then the stream is to be synchronised
int verify_fetch(tdv_ctx* ctx, const VerifyStage& st, int n_poses);
// after either renderer's enqueue: the one wait, then records -> results and the order by n_consistent - n_violating descending, ties
// to the lower index (order: optional)
int verify_finish(tdv_ctx* ctx, const VerifyStage& st, int n_poses, tdv_verify_result* results, int* order);
// tdv_render_depth*: zeros for the pixels outside the pose's tiles, enqueued before the renderer; and after it the one wait and the
// record's count
int render_clear(tdv_ctx* ctx, const FrameCamera& cam, float* d_out);
int render_finish(tdv_ctx* ctx, const VerifyStage& st, int* n_rendered);
// the arguments both renderers check alike: ctx, the pose and frame pointers and counts, the camera, tau, the direction
bool verify_common_args_ok(const tdv_ctx* ctx, const float* poses, int n_poses, const void* frame, const FrameCamera& cam, bool has_scale,
                           float tau, int pose_direction, const void* results);

#ifdef __HIPCC__
// rules 1 to 3 of include/tdv_hip.h: the model point into the camera (frame_pose.hpp: pose_into_camera), then pinhole_project
template <int SUB>
__device__ __forceinline__ bool verify_project(const Pose16& P, const VerifyCam& c, float m0, float m1, float m2, int& u, int& v, float& zc) {
    float xc, yc;
    pose_into_camera(P, c.direction, m0, m1, m2, xc, yc, zc);
    return pinhole_project<SUB>(c.k, c.zmax, xc, yc, zc, u, v);
}

// tile t of the list: its pose and the tile's pixels inside the frame, [x0, xe] x [y0, ye] (every lane alike)
__device__ __forceinline__ int verify_tile_of(const int* __restrict__ off, int n_poses, const VerifyRec* rec, const VerifyCam& c, int t, int& x0,
                                              int& y0, int& xe, int& ye) {
    int lo = 0, hi = n_poses;                                // off[lo] <= t < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= t) lo = mid; else hi = mid;
    }
    const int pose = __builtin_amdgcn_readfirstlane(lo);
    const int bu0 = rec[pose].u0, bu1 = rec[pose].u1, bv0 = rec[pose].v0;
    const int tiles_x = bu1 / VERIFY_TW - bu0 / VERIFY_TW + 1, k = t - off[pose];
    x0 = (bu0 / VERIFY_TW + k % tiles_x) * VERIFY_TW;
    y0 = (bv0 / VERIFY_TH + k / tiles_x) * VERIFY_TH;
    xe = min(x0 + VERIFY_TW, c.w) - 1;
    ye = min(y0 + VERIFY_TH, c.h) - 1;
    return pose;
}

// the tail of a tile, after the barrier that completes its z-buffer: rules 5 to 7 and the counts into the pose's record; RENDER: the tile
// out as f32 into `out` in place of the classification
template <bool RENDER>
__device__ __forceinline__ void verify_tile_tail(const unsigned* tile, int x0, int y0, int xe, int ye, const VerifyCam& c,
                                                 const uint16_t* __restrict__ raw, VerifyRec* rec, int pose, float* __restrict__ out) {
    const int tid = threadIdx.x;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    unsigned long long err = 0;
    for (int i = tid; i < VERIFY_TILE; i += VERIFY_VT) {
        const unsigned b = tile[i];
        const int x = x0 + (i & (VERIFY_TW - 1)), y = y0 + i / VERIFY_TW;
        if (RENDER) {
            if (x <= xe && y <= ye) out[(size_t)y * c.w + x] = b == VERIFY_EMPTY ? 0.f : __uint_as_float(b);
            n0 += b != VERIFY_EMPTY;
            continue;
        }
        if (b == VERIFY_EMPTY) continue;                     // (never set outside the frame)
        const unsigned r = raw[(size_t)y * c.w + x];
        const float zr = __uint_as_float(b), zo = (float)r * c.inv_scale;
        if (!(r != 0 && zo <= c.zmax)) { ++n3; continue; }
        const float diff = zo - zr;
        if (fabsf(diff) <= c.tau) {
            const float q = fabsf(diff) * 1048576.0f;
            err += q >= 4294967296.0f ? 0xFFFFFFFFu : (unsigned)q;
            ++n0;
        } else if (diff < -c.tau) ++n1;
        else ++n2;
    }
    // per lane at most 16 pixels: err < 2^36.  Its low 20 bits and the rest sum over the wave without leaving 32 bits.
    n0 = wave_sum_i32(n0);
    if (!RENDER) {
        n1 = wave_sum_i32(n1); n2 = wave_sum_i32(n2); n3 = wave_sum_i32(n3);
        const unsigned elo = (unsigned)wave_sum_i32((int)(err & 0xFFFFFu)), ehi = (unsigned)wave_sum_i32((int)(err >> 20));
        err = (unsigned long long)elo + ((unsigned long long)ehi << 20);
    }
    if ((tid & 63) == 0) {
        if (n0) atomicAdd(&rec[pose].cls[0], n0);
        if (n1) atomicAdd(&rec[pose].cls[1], n1);
        if (n2) atomicAdd(&rec[pose].cls[2], n2);
        if (n3) atomicAdd(&rec[pose].cls[3], n3);
        if (err) atomicAdd(&rec[pose].err, err);
    }
}
#endif

}  // namespace tdv
