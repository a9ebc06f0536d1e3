// TSDF ray casting and frame-to-model tracking on gfx950: include/tdv_hip.h (tdv_tsdf_raycast_dev) states every rule, T13 to T18 and
// K1 to K3; tdv_tsdf_raycast_color_dev adds T24.
//
// A pixel's march depends on that pixel, the pose and the volume only, every loop is bounded by the step cap, and every float below is
// evaluated as the header writes it: nothing depends on the order the device works in.  The only atomic is the optional hit count.
//   k_tsdf_raycast   a lane per pixel, a wave per 8 x 8 pixel tile, so the eight pair loads of neighbouring rays fall into the same
//                    lines; a pair (tsdf, weight) is loaded whole, as a 64-bit word, and hipcc joins a voxel's with its +x neighbour's:
//                    four 16-byte loads per sample, all in flight before the one test of the eight weights.  The volume, the camera and the pose are kernel arguments: the
//                    pose reaches the lanes through scalar loads.  T15's march in z, T16's one interpolation, then T17 and T18 for the
//                    maps that were asked for (MAPS) - six more samples, only on lanes that hit.  COUNT: the workgroup's hits by
//                    fixed_tree.hpp's block count, one atomic per workgroup.  No LDS beyond that count's four ints.  COL (T24): the
//                    hit's colour from the colour volume - eight 16-byte loads once per ray, after T16, on lanes that hit - by the
//                    sample's own cell (rc_cell) and lerps (rc_trilerp).
// The voxel, T14's grid coordinate, the default truncation and the normalisation are tsdf_volume.hpp's; T13's pose, T17's vertex and
// T18's rotation are frame_pose.hpp's.
// Tracking (K1 to K3) is this kernel into a workspace image, odometry.hip's pair against that image (O10, tsdf_track.hpp) with the hit
// count as the rider of its read-back, and O9's product on the host; the sequence adds tsdf.hip's integrate pass per frame.  Everything a kernel reads from the workspace is written by the call first.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "tsdf_volume.hpp"
#include "fixed_tree.hpp"
#include "tsdf_track.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace tdv {

namespace {

constexpr int RC_T = 256;                                  // lanes of a workgroup: four waves, an 8 x 8 pixel tile each
constexpr int RC_TILE = 8;
static_assert(RC_TILE * RC_TILE == 64, "a wave owns one tile");
static_assert(sizeof(tdv_tsdf_raycast_params) == 8 && sizeof(tdv_tsdf_track_result) == 184, "include/tdv_hip.h: the structs' layout");

struct RcCam { Pinhole k; int w, h; };
struct RcMarch { float zmin, zmax, trunc, min_weight; int max_steps, direction; };

// T13: the volume-frame point of pixel (u, v) at camera depth z
__device__ __forceinline__ void rc_point(int u, int v, float z, const RcCam& c, const Pose16& P, int direction, float* p) {
    float C[3];
    pinhole_vertex(u, v, z, c.k, C);                                               // O2
    pose_out_of_camera(P, direction, C, p);
}

// one voxel: a single 8-byte load
__device__ __forceinline__ TsdfVoxel rc_pair(const TsdfVoxel* __restrict__ a) {
    const unsigned long long q = *reinterpret_cast<const unsigned long long*>(a);                       // (two floats would be loaded apart)
    return TsdfVoxel{__uint_as_float((unsigned)q), __uint_as_float((unsigned)(q >> 32))};
}

__device__ __forceinline__ float rc_lerp(float a, float b, float t) { return a + t * (b - a); }

// T14's cell of p: false where a grid coordinate fails its condition; otherwise the voxel index of corner (i0, i1, i2) and t.  The grid
// coordinates are checked as floats, so every index of the cell's eight voxels is inside the volume: 0 <= i <= n - 2 on each axis.
__device__ __forceinline__ bool rc_cell(const tdv_tsdf_volume& V, const float* p, size_t& corner, float& t0, float& t1, float& t2) {
    const float g0 = tsdf_grid_coord(V.origin[0], p[0], V.voxel_length), g1 = tsdf_grid_coord(V.origin[1], p[1], V.voxel_length),
                g2 = tsdf_grid_coord(V.origin[2], p[2], V.voxel_length);
    if (!(g0 >= 0.f && g0 < (float)(V.nx - 1) && g1 >= 0.f && g1 < (float)(V.ny - 1) && g2 >= 0.f && g2 < (float)(V.nz - 1))) return false;
    const float i0 = floorf(g0), i1 = floorf(g1), i2 = floorf(g2);
    t0 = g0 - i0; t1 = g1 - i1; t2 = g2 - i2;
    corner = ((size_t)(int)i2 * V.ny + (size_t)(int)i1) * V.nx + (size_t)(int)i0;
    return true;
}

// T14's seven lerps over the eight values f[dx + 2 dy + 4 dz]
__device__ __forceinline__ float rc_trilerp(const float* f, float t0, float t1, float t2) {
    const float x00 = rc_lerp(f[0], f[1], t0), x10 = rc_lerp(f[2], f[3], t0), x01 = rc_lerp(f[4], f[5], t0), x11 = rc_lerp(f[6], f[7], t0);
    const float y0 = rc_lerp(x00, x10, t1), y1 = rc_lerp(x01, x11, t1);
    return rc_lerp(y0, y1, t2);
}

// T14: the field at p; false where the sample is unknown.
__device__ __forceinline__ bool rc_sample(const tdv_tsdf_volume& V, float min_weight, const TsdfVoxel* __restrict__ vol, const float* p, float& s) {
    size_t corner;
    float t0, t1, t2;
    if (!rc_cell(V, p, corner, t0, t1, t2)) return false;
    const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * V.ny;
    const TsdfVoxel* a = vol + corner;
    const TsdfVoxel q000 = rc_pair(a), q100 = rc_pair(a + 1), q010 = rc_pair(a + sy), q110 = rc_pair(a + sy + 1), q001 = rc_pair(a + sz),
                 q101 = rc_pair(a + sz + 1), q011 = rc_pair(a + sz + sy), q111 = rc_pair(a + sz + sy + 1);
    const float mw = min_weight;
    if (!((q000.w >= mw) & (q100.w >= mw) & (q010.w >= mw) & (q110.w >= mw) & (q001.w >= mw) & (q101.w >= mw) & (q011.w >= mw) & (q111.w >= mw)))
        return false;                                                              // T6: eight loads in flight, one test
    const float f[8] = {q000.f, q100.f, q010.f, q110.f, q001.f, q101.f, q011.f, q111.f};
    s = rc_trilerp(f, t0, t1, t2);
    return s == s;                                                                 // a NaN is not a sample
}

// T24: the colour at the hit's point p - T14's lerps per channel where the cell's eight voxels are coloured (T22), zeros otherwise.
// Eight 16-byte loads, all in flight before the one test of the eight weights.
__device__ __forceinline__ Row3 rc_colour(const tdv_tsdf_volume& V, const TsdfColour* __restrict__ col, const float* p) {
    size_t corner;
    float t0, t1, t2;
    if (!rc_cell(V, p, corner, t0, t1, t2)) return Row3{0.f, 0.f, 0.f};
    const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * V.ny;
    const TsdfColour* a = col + corner;
    const TsdfColour q[8] = {tsdf_quad(a), tsdf_quad(a + 1), tsdf_quad(a + sy), tsdf_quad(a + sy + 1), tsdf_quad(a + sz), tsdf_quad(a + sz + 1),
                             tsdf_quad(a + sz + sy), tsdf_quad(a + sz + sy + 1)};
    bool all = true;
    float r[8], g[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { all = all & tsdf_coloured(q[k]); r[k] = q[k].r; g[k] = q[k].g; b[k] = q[k].b; }
    if (!all) return Row3{0.f, 0.f, 0.f};
    return Row3{rc_trilerp(r, t0, t1, t2), rc_trilerp(g, t0, t1, t2), rc_trilerp(b, t0, t1, t2)};
}

// blockIdx.x * 4 + wave = the tile, x fastest; lane = (v & 7) * 8 + (u & 7).  COL (T24): rgb_map (not null) gets the colour of every
// pixel from `col`, read once per ray and only at a hit; without COL both are unused and the kernel is the geometry-only one.
template <bool MAPS, bool COUNT, bool COL>
__global__ __launch_bounds__(RC_T)
void k_tsdf_raycast(tdv_tsdf_volume V, RcCam c, Pose16 P, RcMarch m, const TsdfVoxel* __restrict__ vol, float* __restrict__ depth,
                    float* __restrict__ vertex_map, float* __restrict__ normal_map, unsigned long long* __restrict__ n_hit,
                    const TsdfColour* __restrict__ col, float* __restrict__ rgb_map) {
    __shared__ int s_cnt[4];
    const int lane = threadIdx.x & 63, tiles_x = (c.w + RC_TILE - 1) / RC_TILE;
    const int tile = (int)blockIdx.x * (RC_T / 64) + ((int)threadIdx.x >> 6);
    const int u = (tile % tiles_x) * RC_TILE + (lane & 7), v = (tile / tiles_x) * RC_TILE + (lane >> 3);
    const bool in = u < c.w && v < c.h;
    bool hit = false;
    float zh = 0.f;
    if (in) {
        // T15: the k == max_steps test stands in the loop's own condition, so the march is finite whatever the arguments
        float z = m.zmin, zp = 0.f, sp = 0.f;
        bool prev = false;
        for (int k = 0; k < m.max_steps && z <= m.zmax; ++k) {
            float p[3], s = 0.f;
            rc_point(u, v, z, c, P, m.direction, p);
            const bool known = rc_sample(V, m.min_weight, vol, p, s);
            if (known && s < 0.f) {
                if (prev) { hit = true; zh = fminf(zp + ((z - zp) * sp) / (sp - s), z); }      // T16
                break;
            }
            zp = z; sp = s; prev = known;
            z = z + (known ? fmaxf(s * m.trunc, V.voxel_length) : m.trunc);
        }
        const size_t i = (size_t)v * c.w + u;
        if (depth) depth[i] = hit ? zh : 0.0f;
        if (MAPS) {
            Row3 vr{0.f, 0.f, 0.f}, nr{0.f, 0.f, 0.f};
            if (hit) {
                float C[3], p[3], G[3];
                pinhole_vertex(u, v, zh, c.k, C);                                  // T17
                vr = Row3{C[0], C[1], C[2]};
                if (normal_map) {                                                  // T18
                    rc_point(u, v, zh, c, P, m.direction, p);
                    bool all = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        float q[3] = {p[0], p[1], p[2]}, sf = 0.f, sb = 0.f;
                        q[a] = p[a] + V.voxel_length;
                        const bool kf = rc_sample(V, m.min_weight, vol, q, sf);
                        q[a] = p[a] - V.voxel_length;
                        const bool kb = rc_sample(V, m.min_weight, vol, q, sb);
                        all = all && kf && kb;
                        G[a] = sf - sb;
                    }
                    if (all) {
                        float n0, n1, n2;
                        rotate_into_camera(P, m.direction, G, n0, n1, n2);
                        nr = normalized_or_zero(n0, n1, n2);
                    }
                }
            }
            if (vertex_map) reinterpret_cast<Row3*>(vertex_map)[i] = vr;
            if (normal_map) reinterpret_cast<Row3*>(normal_map)[i] = nr;
        }
        if (COL) {
            Row3 cr{0.f, 0.f, 0.f};
            if (hit) {
                float p[3];
                rc_point(u, v, zh, c, P, m.direction, p);
                cr = rc_colour(V, col, p);
            }
            reinterpret_cast<Row3*>(rgb_map)[i] = cr;
        }
    }
    if (COUNT) {
        const int n = tree_block_count(hit ? 1 : 0, s_cnt);
        if (threadIdx.x == 0 && n) atomicAdd(n_hit, (unsigned long long)n);
    }
}


bool rc_params_ok(const tdv_tsdf_raycast_params* r) { return r && positive_finite(r->zmin) && r->max_steps >= 1 && r->max_steps <= TDV_TSDF_RAYCAST_MAX_STEPS; }
bool rc_args_ok(const tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* volume, const FrameCamera& cam, const float* pose,
                const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray) {
    return ctx && tsdf_voxels(vol) && volume && frame_camera_ok(cam, false) && pose && tsdf_params_ok(params) && rc_params_ok(ray);
}

// The launch (cam.npx() > 0).  d_n_hit: nullptr, or where to leave a fresh workspace counter that the launch counts the hits into.
// d_color and d_rgb (both or neither): the colour volume and the map of T24.
int rc_launch(tdv_ctx* ctx, const tdv_tsdf_volume& V, const float* d_volume, const FrameCamera& fc, const float* h_pose, const tdv_tsdf_params& prm,
              const tdv_tsdf_raycast_params& ray, float* d_depth, float* d_vm, float* d_nm, unsigned long long** d_n_hit,
              const float* d_color = nullptr, float* d_rgb = nullptr) {
    hipStream_t s = ctx->stream;
    unsigned long long* d_cnt = nullptr;
    if (d_n_hit) {
        TDV_TRY(ws_alloc(ctx, 1, &d_cnt));
        TDV_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
        *d_n_hit = d_cnt;
    }
    const RcCam cam{fc.k, fc.w, fc.h};
    Pose16 P;
    std::memcpy(P.T, h_pose, sizeof(P.T));
    const RcMarch m{ray.zmin, prm.zmax, tsdf_trunc(prm, V), prm.min_weight, ray.max_steps, prm.pose_direction};
    const unsigned tiles = (unsigned)((fc.w + RC_TILE - 1) / RC_TILE) * (unsigned)((fc.h + RC_TILE - 1) / RC_TILE);      // at most 2^20
    const unsigned blocks = (tiles + RC_T / 64 - 1) / (RC_T / 64);
    const TsdfVoxel* vol = reinterpret_cast<const TsdfVoxel*>(d_volume);
    const TsdfColour* col = reinterpret_cast<const TsdfColour*>(d_color);
    const bool maps = d_vm || d_nm;
    if (d_rgb) {
        if (maps && d_cnt) k_tsdf_raycast<true, true, true><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, d_vm, d_nm, d_cnt, col, d_rgb);
        else if (maps) k_tsdf_raycast<true, false, true><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, d_vm, d_nm, nullptr, col, d_rgb);
        else if (d_cnt) k_tsdf_raycast<false, true, true><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, nullptr, nullptr, d_cnt, col, d_rgb);
        else k_tsdf_raycast<false, false, true><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, nullptr, nullptr, nullptr, col, d_rgb);
    }
    else if (maps && d_cnt) k_tsdf_raycast<true, true, false><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, d_vm, d_nm, d_cnt, nullptr, nullptr);
    else if (maps) k_tsdf_raycast<true, false, false><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, d_vm, d_nm, nullptr, nullptr, nullptr);
    else if (d_cnt) k_tsdf_raycast<false, true, false><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, nullptr, nullptr, d_cnt, nullptr, nullptr);
    else k_tsdf_raycast<false, false, false><<<blocks, RC_T, 0, s>>>(V, cam, P, m, vol, d_depth, nullptr, nullptr, nullptr, nullptr, nullptr);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// after the launch, where the hit count was asked for: the count down (one wait, which the downloads enqueued before it ride)
int rc_hits(tdv_ctx* ctx, const unsigned long long* d_cnt, long long* h_n_hit) {
    unsigned long long n = 0;
    TDV_TRY(pin_reserve(ctx, sizeof(n)));
    TDV_TRY(fetch_state(ctx, d_cnt, &n));
    *h_n_hit = (long long)n;
    return TDV_OK;
}

bool track_args_ok(const tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* volume, const FrameCamera& cam, const tdv_tsdf_params* params,
                   const tdv_tsdf_raycast_params* ray, const tdv_odometry_params* odom) {
    return ctx && tsdf_voxels(vol) && volume && frame_camera_ok(cam, true) && tsdf_params_ok(params) &&
           params->pose_direction == TDV_POSE_SOURCE_ONTO_TARGET && rc_params_ok(ray) && odometry_params_ok(odom, cam.w, cam.h);
}

// K1 to K3 for one frame (cam.npx() > 0): the hit count rides the odometry's read-back, so a tracked frame waits once
int track_frame(tdv_ctx* ctx, const tdv_tsdf_volume& V, const float* d_volume, const uint16_t* d_raw, const FrameCamera& cam, const float* h_guess,
                const tdv_tsdf_params& prm, const tdv_tsdf_raycast_params& ray, const tdv_odometry_params& odom, tdv_tsdf_track_result* out) {
    float* d_depth;
    unsigned long long *d_cnt, n_hit = 0;
    TDV_TRY(ws_alloc(ctx, cam.npx(), &d_depth));
    TDV_TRY(rc_launch(ctx, V, d_volume, cam, h_guess, prm, ray, d_depth, nullptr, nullptr, &d_cnt));                              // K1
    const OdRider hits{d_cnt, sizeof(n_hit), &n_hit};
    TDV_TRY(odometry_pair(ctx, d_raw, OdTarget{nullptr, d_depth}, cam, nullptr, odom, &out->odom, &hits));                        // K2
    out->n_hit = (long long)n_hit;
    pose_chain_product(h_guess, out->odom.T, out->pose);                                                                             // K3
    return TDV_OK;
}

void track_empty(const float* h_guess, tdv_tsdf_track_result* out) {
    std::memset(out, 0, sizeof(*out));
    odometry_empty_result(nullptr, &out->odom);
    pose_chain_product(h_guess, out->odom.T, out->pose);
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_tsdf_raycast_default_params(tdv_tsdf_raycast_params* p) {
    if (!p) return;
    p->zmin = 0.05f; p->max_steps = 4096;
}

int tdv_tsdf_raycast_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, int width, int height, float fx, float fy, float cx,
                         float cy, const float* h_pose, const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray, float* d_depth,
                         float* d_vertex_map, float* d_normal_map, long long* h_n_hit) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!rc_args_ok(ctx, vol, d_volume, cam, h_pose, params, ray)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (h_n_hit) *h_n_hit = 0;
    if (cam.npx() == 0 || (!d_depth && !d_vertex_map && !d_normal_map && !h_n_hit)) return TDV_OK;
    unsigned long long* d_cnt;
    TDV_TRY(rc_launch(ctx, *vol, d_volume, cam, h_pose, *params, *ray, d_depth, d_vertex_map, d_normal_map, h_n_hit ? &d_cnt : nullptr));
    return h_n_hit ? rc_hits(ctx, d_cnt, h_n_hit) : TDV_OK;
}

int tdv_tsdf_raycast_color_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const float* d_color, int width, int height, float fx,
                               float fy, float cx, float cy, const float* h_pose, const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray,
                               float* d_depth, float* d_vertex_map, float* d_normal_map, float* d_rgb_map, long long* h_n_hit) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!rc_args_ok(ctx, vol, d_volume, cam, h_pose, params, ray) || !tsdf_colour_ok(d_color)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (h_n_hit) *h_n_hit = 0;
    if (cam.npx() == 0 || (!d_depth && !d_vertex_map && !d_normal_map && !d_rgb_map && !h_n_hit)) return TDV_OK;
    unsigned long long* d_cnt;
    TDV_TRY(rc_launch(ctx, *vol, d_volume, cam, h_pose, *params, *ray, d_depth, d_vertex_map, d_normal_map, h_n_hit ? &d_cnt : nullptr, d_color, d_rgb_map));
    return h_n_hit ? rc_hits(ctx, d_cnt, h_n_hit) : TDV_OK;
}

int tdv_tsdf_raycast(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* volume, int width, int height, float fx, float fy, float cx, float cy,
                     const float* pose, const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray, float* depth, float* vertex_map,
                     float* normal_map, long long* n_hit) {
    const FrameCamera cam{width, height, 1.f, {fx, fy, cx, cy}};
    if (!rc_args_ok(ctx, vol, volume, cam, pose, params, ray) || tsdf_voxels(vol) > (size_t)TDV_TSDF_HOST_MAX_VOXELS) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (n_hit) *n_hit = 0;
    const size_t npx = cam.npx();
    if (npx == 0 || (!depth && !vertex_map && !normal_map && !n_hit)) return TDV_OK;
    float *d_volume, *d_depth = nullptr, *d_vm = nullptr, *d_nm = nullptr;
    unsigned long long* d_cnt;
    TDV_TRY(upload(ctx, volume, tsdf_voxels(vol) * 2, &d_volume));
    if (depth) TDV_TRY(ws_alloc(ctx, npx, &d_depth));
    if (vertex_map) TDV_TRY(ws_alloc(ctx, npx * 3, &d_vm));
    if (normal_map) TDV_TRY(ws_alloc(ctx, npx * 3, &d_nm));
    TDV_TRY(rc_launch(ctx, *vol, d_volume, cam, pose, *params, *ray, d_depth, d_vm, d_nm, n_hit ? &d_cnt : nullptr));
    TDV_TRY(download(ctx, depth, d_depth, npx));
    TDV_TRY(download(ctx, vertex_map, d_vm, npx * 3));
    TDV_TRY(download(ctx, normal_map, d_nm, npx * 3));
    return n_hit ? rc_hits(ctx, d_cnt, n_hit) : finish(ctx);
}

int tdv_tsdf_track_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const uint16_t* d_raw, int width, int height,
                       float scale, float fx, float fy, float cx, float cy, const float* h_guess, const tdv_tsdf_params* params,
                       const tdv_tsdf_raycast_params* ray, const tdv_odometry_params* odom, tdv_tsdf_track_result* out) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!track_args_ok(ctx, vol, d_volume, cam, params, ray, odom) || !h_guess || !out) return TDV_ERR_BAD_ARG;
    if (cam.npx() != 0 && !d_raw) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    track_empty(h_guess, out);
    if (cam.npx() == 0) return TDV_OK;
    return track_frame(ctx, *vol, d_volume, d_raw, cam, h_guess, *params, *ray, *odom, out);
}

int tdv_tsdf_track_sequence_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume, const uint16_t* d_raw, int n_frames, int width,
                                int height, float scale, float fx, float fy, float cx, float cy, const float* h_pose0,
                                const tdv_tsdf_params* params, const tdv_tsdf_raycast_params* ray, const tdv_odometry_params* odom,
                                float* h_poses, tdv_tsdf_track_result* h_results) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!track_args_ok(ctx, vol, d_volume, cam, params, ray, odom) || n_frames < 0 || n_frames > TDV_TSDF_MAX_FRAMES ||
        (n_frames > 0 && (!h_poses || !d_raw)))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (n_frames == 0) return TDV_OK;
    const size_t npx = cam.npx();
    std::vector<tdv_tsdf_track_result> res((size_t)n_frames);
    std::memset(&res[0], 0, sizeof(res[0]));
    if (h_pose0) std::memcpy(res[0].pose, h_pose0, 64); else pose_identity(res[0].pose);
    std::memcpy(h_poses, res[0].pose, 64);
    const WsMark mark = ws_mark(ctx);
    for (int k = 0; k < n_frames; ++k) {
        const uint16_t* frame = d_raw + (size_t)k * npx;
        float* pose = h_poses + 16 * (size_t)k;
        ws_rewind(ctx, mark);                                // a frame's workspace is the last one's again: the stream orders the reuse
        if (k > 0) {
            track_empty(pose - 16, &res[k]);
            if (npx != 0) TDV_TRY(track_frame(ctx, *vol, d_volume, frame, cam, pose - 16, *params, *ray, *odom, &res[k]));
            std::memcpy(pose, res[k].pose, 64);
        }
        TDV_TRY(tsdf_integrate_frames(ctx, *vol, d_volume, frame, 1, cam, pose, *params, nullptr));
    }
    if (h_results) std::memcpy(h_results, res.data(), (size_t)n_frames * sizeof(tdv_tsdf_track_result));
    return TDV_OK;
}

}  // extern "C"
