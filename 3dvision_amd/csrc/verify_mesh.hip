// Pose verification from a triangle mesh (include/tdv_hip.h: tdv_verify_poses_mesh): the model's faces rasterised at every candidate pose
// into the z-buffer that verify.hip fills with point squares, and the same classification after it (verify_common.hpp).  The shape is
// verify.hip's: init, bounds, plan, tiles, one read-back, and the host's ends around the enqueue are verify.hip's own functions; a tile's
// z-buffer lives in LDS and is built with LDS integer minimum atomics.
//   k_mesh_bounds  per pose n_projected (the usable triangles, rules M2 and M3) and a box of the pixels the usable triangles can cover,
//                  clipped to the frame: the union of their pixel boxes - conservative, no result depends on it
//   k_mesh_tiles   the fixed grid walks the tile list.  Per tile and per block of TDV_VERIFY_LANES triangles a lane sets its triangle up
//                  (three projections, the snapped positions, the signed area, the facing), clips its pixel box to the tile and
//                    - rasterises it itself where the box holds at most TDV_MESH_COOP_PIXELS pixels (a scanned mesh: thousands of faces
//                      of a few pixels), or
//                    - puts a 64-byte setup record onto an LDS queue of TDV_MESH_QUEUE entries (a CAD mesh: a dozen faces of thousands of
//                      pixels).  The workgroup drains the queue together, one pixel per lane over each record's box, when the queue is
//                      full and after the last block; a lane that found it full sets its triangle up again and queues it in the next round.
//                  The queue's order is the order the lanes arrive in and shows in no result: every write is a minimum.
// The edge functions are integers (int32 differences, int64 products: exact), the depth is f64 with the order of rule M5 and no contraction.
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 7, "Pose verification from a mesh".
#include "verify_common.hpp"
#include <algorithm>

namespace tdv {
namespace {

constexpr int VT = VERIFY_VT, TW = VERIFY_TW, TH = VERIFY_TH, TILE = VERIFY_TILE;
constexpr unsigned EMPTY = VERIFY_EMPTY;
constexpr int COOP = TDV_MESH_COOP_PIXELS, QUEUE = TDV_MESH_QUEUE;

// a usable triangle after rule M2 (A > 0) and its pixel box inside a tile or the frame: what a lane rasterises from, and the queue's record
struct MeshRec {
    int xa, ya, xb, yb, xc, yc;                              // snapped positions, 1/TDV_MESH_SUBPIXEL px
    int bx0, by0;                                            // the box's first pixel
    double iza, izb, izc;                                    // 1.0 / (double)zc of a, b, c
    int bw, npix;                                            // the box's width and its pixels
};
static_assert(sizeof(MeshRec) == 64, "the queue's LDS is sized by it");
static_assert(TILE * 4 + QUEUE * (int)sizeof(MeshRec) + 64 <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS");
static_assert(COOP >= 1 && COOP < TILE && QUEUE >= 1, "a box inside a tile can be of either kind");

// rule M1 for vertex i: the snapped position and zc
__device__ __forceinline__ bool mesh_vertex(const Pose16& P, const VerifyCam& c, const float* __restrict__ vtx, int i, int& X, int& Y, float& zc) {
    return verify_project<TDV_MESH_SUBPIXEL>(P, c, vtx[3 * (size_t)i], vtx[3 * (size_t)i + 1], vtx[3 * (size_t)i + 2], X, Y, zc);
}

// rule M2 for triangle i: usable, and then m's positions (b and c swapped where A < 0) and its box of pixel centres, unclipped, in px0..py1
__device__ __forceinline__ bool mesh_setup(const Pose16& P, const VerifyCam& c, int cull, const float* __restrict__ vtx, int nv,
                                           const int* __restrict__ tri, int i, MeshRec& m, float (&z)[3], int& px0, int& py0, int& px1, int& py1) {
    const int ia = tri[3 * (size_t)i], ib = tri[3 * (size_t)i + 1], ic = tri[3 * (size_t)i + 2];
    if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) return false;   // before any read
    if (!mesh_vertex(P, c, vtx, ia, m.xa, m.ya, z[0]) || !mesh_vertex(P, c, vtx, ib, m.xb, m.yb, z[1]) ||
        !mesh_vertex(P, c, vtx, ic, m.xc, m.yc, z[2]))
        return false;
    const long long A = (long long)(m.xb - m.xa) * (m.yc - m.ya) - (long long)(m.yb - m.ya) * (m.xc - m.xa);
    if (A == 0 || (A > 0 && cull == TDV_MESH_CULL_BACK)) return false;
    if (A < 0) {
        int t = m.xb; m.xb = m.xc; m.xc = t;
        t = m.yb; m.yb = m.yc; m.yc = t;
        const float f = z[1]; z[1] = z[2]; z[2] = f;
    }
    const int s = TDV_MESH_SUBPIXEL;                          // pixel x has its centre at s * x: ceil and floor of the extremes / s
    px0 = (min(m.xa, min(m.xb, m.xc)) + s - 1) >> 4; px1 = max(m.xa, max(m.xb, m.xc)) >> 4;
    py0 = (min(m.ya, min(m.yb, m.yc)) + s - 1) >> 4; py1 = max(m.ya, max(m.yb, m.yc)) >> 4;
    return true;
}
static_assert(TDV_MESH_SUBPIXEL == 16, "the shifts by 4 above");

// whether the directed edge (dx, dy) owns the centres on it (rule M4): 0 where it does, 1 where E has to be positive
__device__ __forceinline__ int mesh_edge_bias(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// rules M5 and M6 for a covered pixel: the weights, the tile's word
__device__ __forceinline__ void mesh_depth(const MeshRec& m, long long w0, long long w1, long long w2, unsigned* word) {
    const double s = ((double)w0 * m.iza + (double)w1 * m.izb) + (double)w2 * m.izc;
    const float zr = (float)((double)(w0 + w1 + w2) / s);
    atomicMin(word, __float_as_uint(zr));
}

// rules M4 to M6 for the pixel (x, y) of the tile at (x0, y0).  The positions pass through an empty asm: the compiler otherwise lifts the
// six differences, the three biases and the row's three products out of the pixel loops and holds them in 20 more registers than the
// kernel has at two workgroups per CU; formed anew they cost a pixel nine integer operations beside its f64 division.
__device__ __forceinline__ void mesh_pixel(const MeshRec& m, int x, int y, unsigned* tile, int x0, int y0) {
    int xa = m.xa, ya = m.ya, xb = m.xb, yb = m.yb, xc = m.xc, yc = m.yc;
    asm volatile("" : "+v"(xa), "+v"(ya), "+v"(xb), "+v"(yb), "+v"(xc), "+v"(yc));
    const int px = TDV_MESH_SUBPIXEL * x, py = TDV_MESH_SUBPIXEL * y;
    const int dx0 = xc - xb, dy0 = yc - yb, dx1 = xa - xc, dy1 = ya - yc, dx2 = xb - xa, dy2 = yb - ya;
    const long long w0 = (long long)dx0 * (py - yb) - (long long)dy0 * (px - xb);
    const long long w1 = (long long)dx1 * (py - yc) - (long long)dy1 * (px - xc);
    const long long w2 = (long long)dx2 * (py - ya) - (long long)dy2 * (px - xa);
    if (w0 < mesh_edge_bias(dx0, dy0) || w1 < mesh_edge_bias(dx1, dy1) || w2 < mesh_edge_bias(dx2, dy2)) return;
    mesh_depth(m, w0, w1, w2, &tile[(y - y0) * TW + (x - x0)]);
}

// workgroup (pose, chunk): the triangles chunk * 256 + lane, + chunks * 256, ...
__global__ __launch_bounds__(256) void k_mesh_bounds(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int nt,
                                                     const float* __restrict__ poses, int chunks, VerifyCam c, int cull, VerifyRec* rec) {
    __shared__ int s[5];
    const int pose = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (threadIdx.x < 5) s[threadIdx.x] = threadIdx.x == 0 ? 0 : threadIdx.x <= 2 ? INT_MAX : -1;
    __syncthreads();
    const Pose16 P = load_pose(poses, pose);
    int cnt = 0, u0 = INT_MAX, v0 = INT_MAX, u1 = -1, v1 = -1;
    for (int i = chunk * 256 + (int)threadIdx.x; i < nt; i += chunks * 256) {
        MeshRec m; float z[3]; int a0, b0, a1, b1;
        if (!mesh_setup(P, c, cull, vtx, nv, tri, i, m, z, a0, b0, a1, b1)) continue;
        ++cnt;
        a0 = max(a0, 0); a1 = min(a1, c.w - 1); b0 = max(b0, 0); b1 = min(b1, c.h - 1);
        if (a0 > a1 || b0 > b1) continue;                    // no pixel centre of the frame inside the triangle's box
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

// RENDER: the tile out as f32 into `out` (one pose) in place of the classification
// (8 waves per SIMD asked for: two workgroups of 16 waves share a CU, as in verify.hip)
template <bool RENDER>
__global__ __launch_bounds__(VT, 8) void k_mesh_tiles(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int nt,
                                                   const float* __restrict__ poses, int n_poses, const int* __restrict__ off, VerifyCam c, int cull,
                                                   const uint16_t* __restrict__ raw, VerifyRec* rec, float* __restrict__ out) {
    __shared__ unsigned tile[TILE];
    __shared__ MeshRec queue[QUEUE];
    __shared__ int qn;
    const int tid = threadIdx.x;
    const int total = off[n_poses];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        int x0, y0, xe, ye;                                  // the tile inside the frame: [x0, xe] x [y0, ye]
        const int pose = verify_tile_of(off, n_poses, rec, c, t, x0, y0, xe, ye);
        for (int i = tid; i < TILE / 4; i += VT) reinterpret_cast<uint4*>(tile)[i] = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
        if (tid == 0) qn = 0;
        __syncthreads();
        const Pose16 P = load_pose(poses, pose);
        for (int base = 0; base < nt; base += VT) {          // every lane of the workgroup takes every turn of this loop and the next
            const int i = base + tid;
            const bool last = base + VT >= nt;
            bool pending = i < nt;                           // the lane's triangle is not dealt with yet
            for (;;) {
                if (pending) {                               // (again after a round that turned it away: a setup costs less than its registers)
                    MeshRec m; float z[3]; int a0, b0, a1, b1;
                    pending = false;
                    if (mesh_setup(P, c, cull, vtx, nv, tri, i, m, z, a0, b0, a1, b1)) {
                        a0 = max(a0, x0); a1 = min(a1, xe); b0 = max(b0, y0); b1 = min(b1, ye);
                        if (a0 <= a1 && b0 <= b1) {
                            m.iza = 1.0 / (double)z[0]; m.izb = 1.0 / (double)z[1]; m.izc = 1.0 / (double)z[2];
                            m.bx0 = a0; m.by0 = b0; m.bw = a1 - a0 + 1; m.npix = m.bw * (b1 - b0 + 1);
                            if (m.npix <= COOP) {
                                for (int y = b0; y <= b1; ++y)
                                    for (int x = a0; x <= a1; ++x) mesh_pixel(m, x, y, tile, x0, y0);
                            } else {
                                const int slot = atomicAdd(&qn, 1);       // (at most VT adds between two resets)
                                if (slot < QUEUE) queue[slot] = m; else pending = true;
                            }
                        }
                    }
                }
                __syncthreads();
                const int asked = qn;                        // the same in every lane: nothing adds between these two barriers
                __syncthreads();
                if (asked < QUEUE && !last) break;           // room left and more triangles to come: every asker has its slot
                const int nq = min(asked, QUEUE);
                for (int k = 0; k < nq; ++k) {
                    const MeshRec q = queue[k];
                    for (int idx = tid; idx < q.npix; idx += VT) mesh_pixel(q, q.bx0 + idx % q.bw, q.by0 + idx / q.bw, tile, x0, y0);
                }
                __syncthreads();                             // the records are read
                if (tid == 0) qn = 0;
                __syncthreads();
                if (asked <= QUEUE) break;                   // nobody was turned away
            }
        }
        __syncthreads();
        verify_tile_tail<RENDER>(tile, x0, y0, xe, ye, c, raw, rec, pose, out);
        __syncthreads();                                     // the next tile's clear
    }
}

// the records of every pose on the device, everything enqueued: init, bounds, plan, tiles, the records down
int mesh_enqueue(tdv_ctx* ctx, const float* d_vtx, int nv, const int* d_tri, int nt, const float* h_poses, int n_poses, const uint16_t* d_raw,
                 float* d_out, const VerifyCam& cam, int cull, VerifyStage* st) {
    hipStream_t s = ctx->stream;
    TDV_TRY(verify_stage(ctx, h_poses, n_poses, st));
    const long long frame_tiles = (long long)((cam.w + TW - 1) / TW) * ((cam.h + TH - 1) / TH);
    if (nt > 0 && nv > 0) {
        const int chunks = std::max(1, std::min(64, (nt + 2047) / 2048));
        k_mesh_bounds<<<n_poses * chunks, 256, 0, s>>>(d_vtx, nv, d_tri, nt, st->d_poses, chunks, cam, cull, st->rec);
        if (frame_tiles > 0) {
            verify_plan(ctx, *st, n_poses);
            const int grid = (int)std::min<long long>(VERIFY_GRID, frame_tiles * n_poses);
            if (d_out) k_mesh_tiles<true><<<grid, VT, 0, s>>>(d_vtx, nv, d_tri, nt, st->d_poses, n_poses, st->off, cam, cull, d_raw, st->rec, d_out);
            else k_mesh_tiles<false><<<grid, VT, 0, s>>>(d_vtx, nv, d_tri, nt, st->d_poses, n_poses, st->off, cam, cull, d_raw, st->rec, d_out);
        }
    }
    return verify_fetch(ctx, *st, n_poses);
}

// every argument of the four entry points, before anything is enqueued (include/tdv_hip.h).  frame: the raw frame resp. the depth
// output; results: what receives the per-pose output
bool mesh_verify_args_ok(const tdv_ctx* ctx, const float* vtx, int nv, const int* tri, int nt, const float* poses, int n_poses, const void* frame,
                         const FrameCamera& cam, bool has_scale, const tdv_mesh_verify_params* p, const void* results) {
    if (!p || nv < 0 || nv > TDV_MESH_MAX_VERTICES || nt < 0 || nt > TDV_MESH_MAX_TRIANGLES) return false;
    if ((nv > 0 && !vtx) || (nt > 0 && !tri)) return false;
    if (p->cull != TDV_MESH_CULL_NONE && p->cull != TDV_MESH_CULL_BACK) return false;
    return verify_common_args_ok(ctx, poses, n_poses, frame, cam, has_scale, p->tau, p->pose_direction, results);
}

// verify.hip's verify_run_dev and render_depth_run_dev with the mesh's enqueue between the shared ends (verify_common.hpp)
int mesh_verify_run_dev(tdv_ctx* ctx, const float* d_vtx, int nv, const int* d_tri, int nt, const float* h_poses, int n_poses,
                        const uint16_t* d_raw, const FrameCamera& cam, const tdv_mesh_verify_params& prm, tdv_verify_result* results, int* order) {
    if (n_poses == 0) return TDV_OK;
    VerifyStage st;
    TDV_TRY(mesh_enqueue(ctx, d_vtx, nv, d_tri, nt, h_poses, n_poses, d_raw, nullptr, verify_cam(cam, prm.zmax, prm.tau, 0, prm.pose_direction),
                         prm.cull, &st));
    return verify_finish(ctx, st, n_poses, results, order);
}

int mesh_render_run_dev(tdv_ctx* ctx, const float* d_vtx, int nv, const int* d_tri, int nt, const float* h_pose, const FrameCamera& cam,
                        const tdv_mesh_verify_params& prm, float* d_out, int* n_rendered) {
    TDV_TRY(render_clear(ctx, cam, d_out));
    VerifyStage st;
    TDV_TRY(mesh_enqueue(ctx, d_vtx, nv, d_tri, nt, h_pose, 1, nullptr, d_out, verify_cam(cam, prm.zmax, prm.tau, 0, prm.pose_direction), prm.cull,
                         &st));
    return render_finish(ctx, st, n_rendered);
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_mesh_verify_default_params(tdv_mesh_verify_params* p) {
    if (!p) return;
    p->pose_direction = TDV_POSE_SOURCE_ONTO_TARGET; p->cull = TDV_MESH_CULL_NONE; p->tau = 0.002f; p->zmax = 10.f;
}

int tdv_verify_poses_mesh_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles, const float* h_poses,
                              int n_poses, const uint16_t* d_raw_depth, int width, int height, float scale, float fx, float fy, float cx, float cy,
                              const tdv_mesh_verify_params* params, tdv_verify_result* h_results, int* h_order) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!mesh_verify_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_poses, n_poses, d_raw_depth, cam, true, params, h_results))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return mesh_verify_run_dev(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_poses, n_poses, d_raw_depth, cam, *params, h_results,
                               h_order);
}

int tdv_verify_poses_mesh(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* poses, int n_poses,
                          const uint16_t* raw_depth, int width, int height, float scale, float fx, float fy, float cx, float cy,
                          const tdv_mesh_verify_params* params, tdv_verify_result* results, int* order) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!mesh_verify_args_ok(ctx, vertices, n_vertices, triangles, n_triangles, poses, n_poses, raw_depth, cam, true, params, results))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float* d_vtx; int* d_tri; uint16_t* d_raw;
    TDV_TRY(upload(ctx, vertices, (size_t)n_vertices * 3, &d_vtx));
    TDV_TRY(upload(ctx, triangles, (size_t)n_triangles * 3, &d_tri));
    TDV_TRY(upload(ctx, raw_depth, cam.npx(), &d_raw));
    return mesh_verify_run_dev(ctx, d_vtx, n_vertices, d_tri, n_triangles, poses, n_poses, d_raw, cam, *params, results, order);
}

int tdv_render_depth_mesh_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles, const float* h_pose,
                              int width, int height, float fx, float fy, float cx, float cy, const tdv_mesh_verify_params* params,
                              float* d_out_depth, int* n_rendered) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!mesh_verify_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_pose, 1, d_out_depth, cam, false, params, h_pose))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return mesh_render_run_dev(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_pose, cam, *params, d_out_depth, n_rendered);
}

int tdv_render_depth_mesh(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* pose, int width,
                          int height, float fx, float fy, float cx, float cy, const tdv_mesh_verify_params* params, float* out_depth,
                          int* n_rendered) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!mesh_verify_args_ok(ctx, vertices, n_vertices, triangles, n_triangles, pose, 1, out_depth, cam, false, params, pose))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float *d_vtx, *d_out; int* d_tri;
    TDV_TRY(upload(ctx, vertices, (size_t)n_vertices * 3, &d_vtx));
    TDV_TRY(upload(ctx, triangles, (size_t)n_triangles * 3, &d_tri));
    TDV_TRY(ws_alloc(ctx, cam.npx(), &d_out));
    TDV_TRY(mesh_render_run_dev(ctx, d_vtx, n_vertices, d_tri, n_triangles, pose, cam, *params, d_out, n_rendered));
    TDV_TRY(download(ctx, out_depth, d_out, cam.npx()));
    return finish(ctx);
}

}  // extern "C"
