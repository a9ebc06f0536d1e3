// Pose verification (include/tdv_hip.h: tdv_verify_poses): the model splatted at every candidate pose into a z-buffer and each rendered
// pixel classified against the observed depth.  Candidates x model points is the hot loop; the z-buffer of a tile lives in LDS and is
// built with LDS integer minimum atomics - no global atomic touches a depth, and no kernel waits for another workgroup.
//   k_verify_init    the per-pose record: zero counts, an empty box
//   k_verify_bounds  per pose n_projected and the box of the covered pixels, clipped to the frame: the exact min / max over the same u, v
//                    the render computes (LDS atomics per workgroup, then integer atomics on the record - integers, the order is free)
//   k_verify_plan    tiles per pose = the frame-aligned TDV_VERIFY_TILE_W x TDV_VERIFY_TILE_H tiles its box touches, and their exclusive
//                    scan over the poses: the tile list, on the device
//   k_verify_tiles   a fixed grid of workgroups walks the tile list (tile t of the list belongs to the pose p with off[p] <= t < off[p + 1]:
//                    a search over the offsets); per tile: clear the LDS tile, project the model with the pose in uniform registers, apply
//                    the covers that fall inside the tile (ds_min_u32), barrier, then classify the tile's pixels against the raw frame,
//                    reduce the counts over the wave with DPP and add them to the pose's record; or, for tdv_render_depth, write the tile
//                    out as f32.  The grid never needs the tile total on the host: the call reads back once, the records.
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 7, "Pose verification".
// The record, the projection (frame_pose.hpp's pose and pinhole), the tile list and the classify-and-reduce tail are verify_common.hpp's,
// shared with the mesh renderer (verify_mesh.hip); the host side of a call that both renderers use - stage, plan, fetch, the wait with
// results and order, the render's clear and count - is defined at the end.  The camera arrives as depth_frames.hpp's FrameCamera.
#include "verify_common.hpp"
#include <algorithm>
#include <numeric>

namespace tdv {
namespace {

constexpr int VT = VERIFY_VT, TW = VERIFY_TW, TH = VERIFY_TH, TILE = VERIFY_TILE;
constexpr unsigned EMPTY = VERIFY_EMPTY;

__global__ void k_verify_init(VerifyRec* rec, int n_poses) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_poses) return;
    VerifyRec r{};
    r.u0 = INT_MAX; r.v0 = INT_MAX; r.u1 = -1; r.v1 = -1;
    rec[p] = r;
}

// workgroup (pose, chunk): the points chunk * 256 + lane, + chunks * 256, ...
__global__ __launch_bounds__(256) void k_verify_bounds(const float* __restrict__ xyz, int n, const float* __restrict__ poses, int chunks, VerifyCam c,
                                                       VerifyRec* rec) {
    __shared__ int s[5];
    const int pose = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (threadIdx.x < 5) s[threadIdx.x] = threadIdx.x == 0 ? 0 : threadIdx.x <= 2 ? INT_MAX : -1;
    __syncthreads();
    const Pose16 P = load_pose(poses, pose);
    int cnt = 0, u0 = INT_MAX, v0 = INT_MAX, u1 = -1, v1 = -1;
    for (int i = chunk * 256 + (int)threadIdx.x; i < n; i += chunks * 256) {
        int u, v; float zc;
        if (!verify_project<1>(P, c, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], u, v, zc)) continue;
        ++cnt;
        const int a0 = max(u - c.splat, 0), a1 = min(u + c.splat, c.w - 1), b0 = max(v - c.splat, 0), b1 = min(v + c.splat, c.h - 1);
        if (a0 > a1 || b0 > b1) continue;                    // the square reaches nothing inside the frame
        u0 = min(u0, a0); u1 = max(u1, a1); v0 = min(v0, b0); v1 = max(v1, b1);
    }
    cnt = wave_sum_i32(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s[0], cnt);
    if (u0 <= u1) { atomicMin(&s[1], u0); atomicMin(&s[2], v0); atomicMax(&s[3], u1); atomicMax(&s[4], v1); }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s[0]) atomicAdd(&rec[pose].n_projected, s[0]);
        if (s[1] <= s[3]) {
            atomicMin(&rec[pose].u0, s[1]); atomicMin(&rec[pose].v0, s[2]); atomicMax(&rec[pose].u1, s[3]); atomicMax(&rec[pose].v1, s[4]);
        }
    }
}

// off[p] = tiles of the poses before p, off[n_poses] = all tiles (at most 65536 poses x 64 x 64 tiles: an int)
__global__ __launch_bounds__(1024) void k_verify_plan(const VerifyRec* rec, int n_poses, int* off) {
    __shared__ int s[1024];
    int carry = 0;
    for (int base = 0; base < n_poses; base += 1024) {
        const int p = base + (int)threadIdx.x;
        int t = 0;
        if (p < n_poses && rec[p].u0 <= rec[p].u1) t = (rec[p].u1 / TW - rec[p].u0 / TW + 1) * (rec[p].v1 / TH - rec[p].v0 / TH + 1);
        s[threadIdx.x] = t;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int a = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += a;
            __syncthreads();
        }
        if (p < n_poses) off[p] = carry + s[threadIdx.x] - t;
        carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n_poses] = carry;
}

// RENDER: the tile out as f32 into `out` (one pose) in place of the classification
// (8 waves per SIMD asked for: two workgroups of 16 waves share a CU only while the SGPR count stays within 80)
template <bool RENDER>
__global__ __launch_bounds__(VT, 8) void k_verify_tiles(const float* __restrict__ xyz, int n, const float* __restrict__ poses, int n_poses,
                                                     const int* __restrict__ off, VerifyCam c, const uint16_t* __restrict__ raw, VerifyRec* rec,
                                                     float* __restrict__ out) {
    __shared__ unsigned tile[TILE];
    const int tid = threadIdx.x;
    const int total = off[n_poses];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        int x0, y0, xe, ye;                                  // the tile inside the frame: [x0, xe] x [y0, ye]
        const int pose = verify_tile_of(off, n_poses, rec, c, t, x0, y0, xe, ye);
        for (int i = tid; i < TILE / 4; i += VT) reinterpret_cast<uint4*>(tile)[i] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
        __syncthreads();
        const Pose16 P = load_pose(poses, pose);
        for (int i = tid; i < n; i += VT) {
            int u, v; float zc;
            if (!verify_project<1>(P, c, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], u, v, zc)) continue;
            const int a0 = max(u - c.splat, x0), a1 = min(u + c.splat, xe), b0 = max(v - c.splat, y0), b1 = min(v + c.splat, ye);
            const unsigned bits = __float_as_uint(zc);
            for (int y = b0; y <= b1; ++y)
                for (int x = a0; x <= a1; ++x) atomicMin(&tile[(y - y0) * TW + (x - x0)], bits);
        }
        __syncthreads();
        verify_tile_tail<RENDER>(tile, x0, y0, xe, ye, c, raw, rec, pose, out);
        __syncthreads();                                     // the next tile's clear
    }
}

// the records of every pose on the device, everything enqueued: init, bounds, plan, tiles, the records down
int verify_enqueue(tdv_ctx* ctx, const float* d_model, int n_model, const float* h_poses, int n_poses, const uint16_t* d_raw, float* d_out,
                   const VerifyCam& cam, VerifyStage* st) {
    hipStream_t s = ctx->stream;
    TDV_TRY(verify_stage(ctx, h_poses, n_poses, st));
    const long long frame_tiles = (long long)((cam.w + TW - 1) / TW) * ((cam.h + TH - 1) / TH);
    if (n_model > 0) {
        const int chunks = std::max(1, std::min(64, (n_model + 2047) / 2048));
        k_verify_bounds<<<n_poses * chunks, 256, 0, s>>>(d_model, n_model, st->d_poses, chunks, cam, st->rec);
    }
    if (n_model > 0 && frame_tiles > 0) {
        verify_plan(ctx, *st, n_poses);
        const int grid = (int)std::min<long long>(VERIFY_GRID, frame_tiles * n_poses);
        if (d_out) k_verify_tiles<true><<<grid, VT, 0, s>>>(d_model, n_model, st->d_poses, n_poses, st->off, cam, d_raw, st->rec, d_out);
        else k_verify_tiles<false><<<grid, VT, 0, s>>>(d_model, n_model, st->d_poses, n_poses, st->off, cam, d_raw, st->rec, d_out);
    }
    return verify_fetch(ctx, *st, n_poses);
}

}  // namespace

// ---- what verify_mesh.hip shares (verify_common.hpp)
int verify_stage(tdv_ctx* ctx, const float* h_poses, int n_poses, VerifyStage* st) {
    hipStream_t s = ctx->stream;
    const size_t up_bytes = align_up((size_t)n_poses * 16 * sizeof(float), 256), down_bytes = (size_t)n_poses * sizeof(VerifyRec);
    TDV_TRY(pin_reserve(ctx, up_bytes + down_bytes));
    std::memcpy(ctx->pin, h_poses, (size_t)n_poses * 16 * sizeof(float));
    TDV_TRY(ws_alloc(ctx, (size_t)n_poses * 16, &st->d_poses));
    TDV_TRY(ws_alloc(ctx, (size_t)n_poses, &st->rec));
    TDV_TRY(ws_alloc(ctx, (size_t)n_poses + 1, &st->off));
    TDV_HIP(ctx, hipMemcpyAsync(st->d_poses, ctx->pin, (size_t)n_poses * 16 * sizeof(float), hipMemcpyHostToDevice, s));
    k_verify_init<<<(n_poses + 255) / 256, 256, 0, s>>>(st->rec, n_poses);
    st->down = ctx->pin + up_bytes;
    return TDV_OK;
}

void verify_plan(tdv_ctx* ctx, const VerifyStage& st, int n_poses) { k_verify_plan<<<1, 1024, 0, ctx->stream>>>(st.rec, n_poses, st.off); }

int verify_fetch(tdv_ctx* ctx, const VerifyStage& st, int n_poses) {
    TDV_CHECK_LAUNCH(ctx);
    TDV_HIP(ctx, hipMemcpyAsync(st.down, st.rec, (size_t)n_poses * sizeof(VerifyRec), hipMemcpyDeviceToHost, ctx->stream));
    return TDV_OK;
}

namespace {

// records -> results, and the order
void verify_results(const char* down, int n_poses, tdv_verify_result* results, int* order) {
    for (int p = 0; p < n_poses; ++p) {
        VerifyRec r;
        std::memcpy(&r, down + (size_t)p * sizeof(VerifyRec), sizeof(r));
        tdv_verify_result& o = results[p];
        o.n_projected = r.n_projected;
        o.n_consistent = r.cls[0]; o.n_occluded = r.cls[1]; o.n_violating = r.cls[2]; o.n_unknown = r.cls[3];
        o.n_rendered = r.cls[0] + r.cls[1] + r.cls[2] + r.cls[3];
        o.err_q20 = r.err;
    }
    if (order) {
        std::iota(order, order + n_poses, 0);
        std::stable_sort(order, order + n_poses, [&](int a, int b) {
            return results[a].n_consistent - results[a].n_violating > results[b].n_consistent - results[b].n_violating;
        });
    }
}

}  // namespace

int verify_finish(tdv_ctx* ctx, const VerifyStage& st, int n_poses, tdv_verify_result* results, int* order) {
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    verify_results(st.down, n_poses, results, order);
    return TDV_OK;
}

int render_clear(tdv_ctx* ctx, const FrameCamera& cam, float* d_out) {
    if (cam.npx() > 0) TDV_HIP(ctx, hipMemsetAsync(d_out, 0, cam.npx() * sizeof(float), ctx->stream));
    return TDV_OK;
}

int render_finish(tdv_ctx* ctx, const VerifyStage& st, int* n_rendered) {
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VerifyRec r;
    std::memcpy(&r, st.down, sizeof(r));
    if (n_rendered) *n_rendered = r.cls[0];
    return TDV_OK;
}

bool verify_common_args_ok(const tdv_ctx* ctx, const float* poses, int n_poses, const void* frame, const FrameCamera& cam, bool has_scale,
                           float tau, int pose_direction, const void* results) {
    if (!ctx || n_poses < 0 || n_poses > TDV_VERIFY_MAX_POSES || !frame_camera_ok(cam, has_scale)) return false;
    if ((n_poses > 0 && (!poses || !results)) || (cam.npx() > 0 && !frame)) return false;
    return positive_finite(tau) && pose_direction_ok(pose_direction);
}

namespace {

// every argument of the four entry points, before anything is enqueued (include/tdv_hip.h).  frame: the raw frame resp. the depth
// output; results: what receives the per-pose output
bool verify_args_ok(const tdv_ctx* ctx, const float* model, int n_model, const float* poses, int n_poses, const void* frame,
                    const FrameCamera& cam, bool has_scale, const tdv_verify_params* p, const void* results) {
    if (!p || n_model < 0 || n_model > TDV_VERIFY_MAX_MODEL || (n_model > 0 && !model)) return false;
    if (p->splat < 0 || p->splat > TDV_VERIFY_MAX_SPLAT) return false;
    return verify_common_args_ok(ctx, poses, n_poses, frame, cam, has_scale, p->tau, p->pose_direction, results);
}

int verify_run_dev(tdv_ctx* ctx, const float* d_model, int n_model, const float* h_poses, int n_poses, const uint16_t* d_raw,
                   const FrameCamera& cam, const tdv_verify_params& prm, tdv_verify_result* results, int* order) {
    if (n_poses == 0) return TDV_OK;
    VerifyStage st;
    TDV_TRY(verify_enqueue(ctx, d_model, n_model, h_poses, n_poses, d_raw, nullptr,
                           verify_cam(cam, prm.zmax, prm.tau, prm.splat, prm.pose_direction), &st));
    return verify_finish(ctx, st, n_poses, results, order);
}

int render_depth_run_dev(tdv_ctx* ctx, const float* d_model, int n_model, const float* h_pose, const FrameCamera& cam,
                         const tdv_verify_params& prm, float* d_out, int* n_rendered) {
    TDV_TRY(render_clear(ctx, cam, d_out));
    VerifyStage st;
    TDV_TRY(verify_enqueue(ctx, d_model, n_model, h_pose, 1, nullptr, d_out, verify_cam(cam, prm.zmax, prm.tau, prm.splat, prm.pose_direction),
                           &st));
    return render_finish(ctx, st, n_rendered);
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_verify_default_params(tdv_verify_params* p) {
    if (!p) return;
    p->pose_direction = TDV_POSE_SOURCE_ONTO_TARGET; p->splat = 1; p->tau = 0.002f; p->zmax = 10.f;
}

int tdv_verify_poses_dev(tdv_ctx* ctx, const float* d_model_xyz, int n_model, const float* h_poses, int n_poses, const uint16_t* d_raw_depth, int width,
                         int height, float scale, float fx, float fy, float cx, float cy, const tdv_verify_params* params,
                         tdv_verify_result* h_results, int* h_order) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!verify_args_ok(ctx, d_model_xyz, n_model, h_poses, n_poses, d_raw_depth, cam, true, params, h_results)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return verify_run_dev(ctx, d_model_xyz, n_model, h_poses, n_poses, d_raw_depth, cam, *params, h_results, h_order);
}

int tdv_verify_poses(tdv_ctx* ctx, const float* model_xyz, int n_model, const float* poses, int n_poses, const uint16_t* raw_depth, int width,
                     int height, float scale, float fx, float fy, float cx, float cy, const tdv_verify_params* params, tdv_verify_result* results,
                     int* order) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!verify_args_ok(ctx, model_xyz, n_model, poses, n_poses, raw_depth, cam, true, params, results)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float* d_model; uint16_t* d_raw;
    TDV_TRY(upload(ctx, model_xyz, (size_t)n_model * 3, &d_model));
    TDV_TRY(upload(ctx, raw_depth, cam.npx(), &d_raw));
    return verify_run_dev(ctx, d_model, n_model, poses, n_poses, d_raw, cam, *params, results, order);
}

int tdv_render_depth_dev(tdv_ctx* ctx, const float* d_model_xyz, int n_model, const float* h_pose, int width, int height, float fx, float fy, float cx,
                         float cy, const tdv_verify_params* params, float* d_out_depth, int* n_rendered) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!verify_args_ok(ctx, d_model_xyz, n_model, h_pose, 1, d_out_depth, cam, false, params, h_pose)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return render_depth_run_dev(ctx, d_model_xyz, n_model, h_pose, cam, *params, d_out_depth, n_rendered);
}

int tdv_render_depth(tdv_ctx* ctx, const float* model_xyz, int n_model, const float* pose, int width, int height, float fx, float fy, float cx, float cy,
                     const tdv_verify_params* params, float* out_depth, int* n_rendered) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!verify_args_ok(ctx, model_xyz, n_model, pose, 1, out_depth, cam, false, params, pose)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float *d_model, *d_out;
    TDV_TRY(upload(ctx, model_xyz, (size_t)n_model * 3, &d_model));
    TDV_TRY(ws_alloc(ctx, cam.npx(), &d_out));
    TDV_TRY(render_depth_run_dev(ctx, d_model, n_model, pose, cam, *params, d_out, n_rendered));
    TDV_TRY(download(ctx, out_depth, d_out, cam.npx()));
    return finish(ctx);
}

}  // extern "C"
