// TSDF fusion on gfx950: include/tdv_hip.h (tdv_tsdf_integrate_dev) states every rule, T1 to T8.
//
// A voxel's update depends on that voxel and one pixel per frame, and a crossing on a voxel's 2 x 6 neighbourhood: every float below is
// evaluated as the header writes it, in the frame order it names, so nothing depends on the order the device works in.  The only atomics
// are integer counts (h_n_updated); no output position comes from one.
//   k_tsdf_reset      one lane per voxel: the pair (1, 0).
//   k_tsdf_integrate  every frame of the call in one pass: a wave owns TS_RPW rows of one run of 64 voxels along x, a lane one voxel of
//                     each.  T1 once, then per frame T2 and T3 (verify_common.hpp's verify_project, the verifier's rules as written),
//                     T4 and T5 in registers.  A pair is loaded (8 bytes) when the first frame updates it and stored once after the
//                     last; a voxel no frame updates is neither loaded nor stored.  The pose of a frame is read at a wave-uniform
//                     address: scalar loads, not per-lane ones.  The per-frame counts go through one LDS atomic per wave and frame,
//                     then one global atomic per workgroup.  One row per wave (93,750 workgroups on 24 M voxels) lost its measurement
//                     and lives on in the study build: DESIGN.md 7, "TSDF fusion".
//   k_tsdf_extract    a workgroup per tile of TDV_TSDF_TILE_X x _Y x _Z voxels staged in LDS with its halo (one voxel below and two above
//                     per axis with normals: the 6-neighbourhood of both ends of a crossing; one above without).  A wave owns a run of 64
//                     voxels along x: three ballots (one per axis) place a lane's crossings inside the run in T7's order.  It runs twice:
//                     the count per run (<false, false>), exclusive_scan_dev over the runs in voxel order, one read-back of the total -
//                     where a capacity that is too small ends the call before any row is written -, then the rows (<true, NRM>).
// Everything a kernel reads from the workspace is written by the call first: the poses by an upload, the counts by a memset, the run
// counts by the first pass (every run of the volume is owned by exactly one wave), their prefix sums by the scan.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "verify_common.hpp"
#include <cmath>
#include <cstring>

namespace tdv {

namespace {

constexpr int TS_T = 256;                                  // lanes of a workgroup: four waves, a run of 64 voxels along x each
constexpr int TS_RPW = 8;                                  // k_tsdf_integrate: voxel rows of a wave
constexpr int TS_TX = TDV_TSDF_TILE_X, TS_TY = TDV_TSDF_TILE_Y, TS_TZ = TDV_TSDF_TILE_Z;
static_assert(TS_TX == 64, "a wave owns a run of TDV_TSDF_TILE_X voxels");
static_assert(sizeof(tdv_tsdf_volume) == 28 && sizeof(tdv_tsdf_params) == 20, "include/tdv_hip.h: the structs' layout");
static_assert(TDV_TSDF_MAX_FRAMES <= TS_T, "k_tsdf_integrate: one lane per frame count");

struct TsPair { float f, w; };                             // a voxel of the volume: 8 bytes, loaded and stored whole
struct TsRow3 { float x, y, z; };

// T1: the centre of voxel i along an axis
__device__ __forceinline__ float ts_centre(float origin, int i, float L) { return origin + ((float)i + 0.5f) * L; }

__global__ __launch_bounds__(TS_T)
void k_tsdf_reset(TsPair* __restrict__ vol, size_t n) {
    const size_t i = (size_t)blockIdx.x * TS_T + threadIdx.x;
    if (i < n) vol[i] = TsPair{1.0f, 0.0f};
}

// A wave owns RPW rows (row = k * ny + j) of one run of 64 voxels along x, a workgroup 4 RPW consecutive rows: blockIdx.x = (row group)
// x (runs along x).  The frames are the outer loop, so a frame's pose is read once per wave and its count leaves through one LDS atomic;
// the RPW pairs live in registers across the frames.  c: the camera as verify_project takes it (tau unused).
template <int RPW>
__global__ __launch_bounds__(TS_T)
void k_tsdf_integrate(tdv_tsdf_volume V, VerifyCam c, float trunc, float max_weight, int n_frames, TsPair* __restrict__ vol,
                      const uint16_t* __restrict__ raw, const float* __restrict__ poses, unsigned long long* __restrict__ n_updated) {
    __shared__ int s_cnt[TDV_TSDF_MAX_FRAMES];
    if (threadIdx.x < TDV_TSDF_MAX_FRAMES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int nrun = (V.nx + TS_TX - 1) / TS_TX, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = V.ny * V.nz;
    const int i = (int)(blockIdx.x % nrun) * TS_TX + lane, row0 = ((int)(blockIdx.x / nrun) * (TS_T / 64) + wave) * RPW;
    const float xw = ts_centre(V.origin[0], i, V.voxel_length);
    const size_t frame = (size_t)c.w * c.h;
    float yw[RPW], zw[RPW], f[RPW], w[RPW];
    bool in[RPW], loaded[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int row = row0 + r;
        in[r] = i < V.nx && row < rows;
        yw[r] = ts_centre(V.origin[1], row % V.ny, V.voxel_length);
        zw[r] = ts_centre(V.origin[2], row / V.ny, V.voxel_length);
        f[r] = 0.f; w[r] = 0.f; loaded[r] = false;
    }
    for (int fr = 0; fr < n_frames; ++fr) {
        const Pose16 P = load_pose(poses, fr);                                    // wave-uniform
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            bool upd = false;
            float t = 0.f;
            int u, v;
            float zc;
            if (in[r] && verify_project<1>(P, c, xw, yw[r], zw[r], u, v, zc) && u >= 0 && u < c.w && v >= 0 && v < c.h) {      // T2, T3
                const unsigned d = raw[fr * frame + (size_t)v * c.w + u];
                const float zo = (float)d * c.inv_scale;                         // T4
                if (d != 0 && zo <= c.zmax) {
                    const float sdf = zo - zc;                                   // T5
                    if (!(sdf < -trunc)) { upd = true; t = fminf(1.0f, sdf / trunc); }
                }
            }
            if (upd) {
                if (!loaded[r]) { const TsPair p = vol[(size_t)(row0 + r) * V.nx + i]; f[r] = p.f; w[r] = p.w; loaded[r] = true; }
                f[r] = (f[r] * w[r] + t) / (w[r] + 1.0f);
                w[r] = fminf(w[r] + 1.0f, max_weight);
            }
            cnt += __popcll(__ballot(upd));
        }
        if (lane == 0 && cnt) atomicAdd(&s_cnt[fr], cnt);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r)
        if (loaded[r]) vol[(size_t)(row0 + r) * V.nx + i] = TsPair{f[r], w[r]};
    __syncthreads();
    if ((int)threadIdx.x < n_frames && s_cnt[threadIdx.x]) atomicAdd(&n_updated[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// T8: the gradient at the staged voxel `cell` along the axis of `stride`; s_o is 0 outside the volume as for an unobserved voxel
__device__ __forceinline__ float ts_gradient(const float* s_f, const unsigned char* s_o, int cell, int stride) {
    const bool of = s_o[cell + stride] != 0, ob = s_o[cell - stride] != 0;
    if (!of && !ob) return 0.f;
    const float d = (of ? s_f[cell + stride] : s_f[cell]) - (ob ? s_f[cell - stride] : s_f[cell]);
    return of != ob ? d * 2.0f : d;
}

// blockIdx.x = tile (x fastest).  EMIT false: run_cnt[run] = the crossings of every run of 64 voxels of the tile; true: the rows of
// every run from run_off[run] on.  run = (k * ny + j) * nrun + the run's number along x: ascending with T7's order.
template <bool EMIT, bool NRM>
__global__ __launch_bounds__(TS_T)
void k_tsdf_extract(tdv_tsdf_volume V, float min_weight, const TsPair* __restrict__ vol, int* __restrict__ run_cnt,
                    const int* __restrict__ run_off, float* __restrict__ out_xyz, float* __restrict__ out_nrm) {
    constexpr int LO = NRM ? 1 : 0, HI = NRM ? 2 : 1;
    constexpr int LX = TS_TX + LO + HI, LY = TS_TY + LO + HI, LZ = TS_TZ + LO + HI, CELLS = LX * LY * LZ;
    __shared__ float s_f[CELLS];
    __shared__ unsigned char s_o[CELLS];                                           // T6, and 0 outside the volume
    const int nrun = (V.nx + TS_TX - 1) / TS_TX, nty = (V.ny + TS_TY - 1) / TS_TY;
    const int sx = (int)(blockIdx.x % nrun), ty = (int)((blockIdx.x / nrun) % nty), tz = (int)((blockIdx.x / nrun) / nty);
    const int x0 = sx * TS_TX, y0 = ty * TS_TY, z0 = tz * TS_TZ;
    for (int cell = threadIdx.x; cell < CELLS; cell += TS_T) {
        const int gx = x0 - LO + cell % LX, gy = y0 - LO + (cell / LX) % LY, gz = z0 - LO + cell / (LX * LY);
        const bool inside = (unsigned)gx < (unsigned)V.nx && (unsigned)gy < (unsigned)V.ny && (unsigned)gz < (unsigned)V.nz;
        TsPair p{0.f, 0.f};
        if (inside) p = vol[((size_t)gz * V.ny + gy) * V.nx + gx];
        s_f[cell] = p.f;
        s_o[cell] = inside && p.w >= min_weight;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int STRIDE[3] = {1, LX, LX * LY};
    for (int r = wave; r < TS_TY * TS_TZ; r += TS_T / 64) {
        const int ry = r % TS_TY, rz = r / TS_TY, g[3] = {x0 + lane, y0 + ry, z0 + rz};
        if (g[1] >= V.ny || g[2] >= V.nz) continue;                                // wave-uniform
        const int a = ((rz + LO) * LY + (ry + LO)) * LX + (lane + LO);
        const float fa = s_f[a];
        const bool oa = g[0] < V.nx && s_o[a] != 0;
        bool has[3];
        unsigned long long m[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {                                           // T7
            const int b = a + STRIDE[ax];
            has[ax] = oa && s_o[b] != 0 && ((fa < 0.f) != (s_f[b] < 0.f));
            m[ax] = __ballot(has[ax]);
        }
        const size_t run = ((size_t)g[2] * V.ny + g[1]) * nrun + sx;
        if (!EMIT) {
            if (lane == 0) run_cnt[run] = __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]);
            continue;
        }
        if ((m[0] | m[1] | m[2]) == 0ull) continue;
        const unsigned long long below = (1ull << lane) - 1ull;
        size_t out = (size_t)run_off[run] + (size_t)(__popcll(m[0] & below) + __popcll(m[1] & below) + __popcll(m[2] & below));
        const float ca[3] = {ts_centre(V.origin[0], g[0], V.voxel_length), ts_centre(V.origin[1], g[1], V.voxel_length),
                             ts_centre(V.origin[2], g[2], V.voxel_length)};
        float ga[3] = {0.f, 0.f, 0.f};
        if (NRM && (has[0] || has[1] || has[2])) {
#pragma unroll
            for (int d = 0; d < 3; ++d) ga[d] = ts_gradient(s_f, s_o, a, STRIDE[d]);
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!has[ax]) continue;
            const int b = a + STRIDE[ax];
            const float ra = fabsf(fa), rb = fabsf(s_f[b]);
            float p[3] = {ca[0], ca[1], ca[2]};
            const float cb = ts_centre(V.origin[ax], g[ax] + 1, V.voxel_length);
            p[ax] = (ca[ax] * rb + cb * ra) / (ra + rb);
            reinterpret_cast<TsRow3*>(out_xyz)[out] = TsRow3{p[0], p[1], p[2]};
            if (NRM) {                                                             // T8
                float n[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) n[d] = ga[d] * rb + ts_gradient(s_f, s_o, b, STRIDE[d]) * ra;
                const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                const bool ok = len > 0.f && len < INFINITY;                       // (false for NaN)
                reinterpret_cast<TsRow3*>(out_nrm)[out] = ok ? TsRow3{n[0] / len, n[1] / len, n[2] / len} : TsRow3{0.f, 0.f, 0.f};
            }
            ++out;
        }
    }
}

bool ts_positive_finite(float v) { return std::isfinite(v) && v > 0.f; }

// the voxels of a volume the checks accept, 0 for one they refuse
size_t ts_voxels(const tdv_tsdf_volume* v) {
    if (!v || !ts_positive_finite(v->voxel_length)) return 0;
    if (v->nx < 1 || v->nx > TDV_TSDF_MAX_SIDE || v->ny < 1 || v->ny > TDV_TSDF_MAX_SIDE || v->nz < 1 || v->nz > TDV_TSDF_MAX_SIDE) return 0;
    const size_t n = (size_t)v->nx * v->ny * v->nz;
    return n <= (size_t)TDV_TSDF_MAX_VOXELS ? n : 0;
}

bool ts_params_ok(const tdv_tsdf_params* p) {
    if (!p || !(std::isfinite(p->trunc) && p->trunc >= 0.f) || !(std::isfinite(p->max_weight) && p->max_weight >= 1.f)) return false;
    if (!ts_positive_finite(p->min_weight)) return false;
    return p->pose_direction == TDV_POSE_SOURCE_ONTO_TARGET || p->pose_direction == TDV_POSE_MODEL_TO_CAMERA;
}

bool ts_frames_ok(const void* raw, int n_frames, int w, int h, float scale, float fx, float fy, const float* poses) {
    if (n_frames < 0 || n_frames > TDV_TSDF_MAX_FRAMES || w < 0 || w > TDV_VERIFY_MAX_SIDE || h < 0 || h > TDV_VERIFY_MAX_SIDE) return false;
    if (n_frames > 0 && (!raw || !poses)) return false;
    return ts_positive_finite(scale) && ts_positive_finite(fx) && ts_positive_finite(fy);
}

int ts_reset(tdv_ctx* ctx, size_t nvox, float* d_volume) {
    k_tsdf_reset<<<(unsigned)((nvox + TS_T - 1) / TS_T), TS_T, 0, ctx->stream>>>(reinterpret_cast<TsPair*>(d_volume), nvox);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// every frame of the call in one launch; h_n_updated (optional): one read-back
int ts_integrate(tdv_ctx* ctx, const tdv_tsdf_volume& V, float* d_volume, const uint16_t* d_raw, int n_frames, int w, int h, float scale,
                 float fx, float fy, float cx, float cy, const float* h_poses, const tdv_tsdf_params& prm, long long* h_n_updated) {
    if (n_frames == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    float* d_poses;
    unsigned long long* d_cnt;
    TDV_TRY(upload(ctx, h_poses, (size_t)n_frames * 16, &d_poses));
    TDV_TRY(ws_alloc(ctx, (size_t)TDV_TSDF_MAX_FRAMES, &d_cnt));
    TDV_TRY(pin_reserve(ctx, sizeof(unsigned long long) * TDV_TSDF_MAX_FRAMES));
    TDV_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * TDV_TSDF_MAX_FRAMES, s));
    const VerifyCam cam{fx, fy, cx, cy, prm.zmax, 0.f, (float)(1.0 / (double)scale), w, h, 0, prm.pose_direction};
    const float trunc = prm.trunc == 0.f ? 4.0f * V.voxel_length : prm.trunc;
    const size_t rows = (size_t)V.ny * V.nz, nrun = (size_t)(V.nx + TS_TX - 1) / TS_TX;
    auto blocks = [&](int rpw) { return (unsigned)(nrun * ((rows + rpw * (TS_T / 64) - 1) / (rpw * (TS_T / 64)))); };      // at most 16 x 2^18
    TsPair* vol = reinterpret_cast<TsPair*>(d_volume);
#ifdef TDV_STUDY
    // The A/B that lost ("TSDF fusion"): one row per wave, a workgroup of four voxel rows
    if (study_env("TDV_TSDF_ONE_ROW")) k_tsdf_integrate<1><<<blocks(1), TS_T, 0, s>>>(V, cam, trunc, prm.max_weight, n_frames, vol, d_raw, d_poses, d_cnt);
    else
#endif
    k_tsdf_integrate<TS_RPW><<<blocks(TS_RPW), TS_T, 0, s>>>(V, cam, trunc, prm.max_weight, n_frames, vol, d_raw, d_poses, d_cnt);
    TDV_CHECK_LAUNCH(ctx);
    if (!h_n_updated) return TDV_OK;
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, d_cnt, sizeof(unsigned long long) * n_frames, hipMemcpyDeviceToHost, s));
    TDV_TRY(finish(ctx));
    std::memcpy(h_n_updated, ctx->pin, sizeof(long long) * n_frames);
    return TDV_OK;
}

// count, scan, the total down, then the rows.  Device form: d_xyz / d_nrm are the caller's.  Host form (h_xyz != nullptr): the rows go
// through workspace memory of the size the count names.
int ts_extract(tdv_ctx* ctx, const tdv_tsdf_volume& V, const float* d_volume, const tdv_tsdf_params& prm, float* d_xyz, float* d_nrm,
               int capacity, int* n_out, float* h_xyz, float* h_nrm) {
    hipStream_t s = ctx->stream;
    const TsPair* vol = reinterpret_cast<const TsPair*>(d_volume);
    const size_t nrun = (size_t)(V.nx + TS_TX - 1) / TS_TX, runs = nrun * V.ny * V.nz;            // at most 2^24
    const unsigned tiles = (unsigned)(nrun * ((V.ny + TS_TY - 1) / TS_TY) * ((V.nz + TS_TZ - 1) / TS_TZ));
    int *cnt, *off, *d_total, total = 0;
    TDV_TRY(ws_alloc(ctx, runs, &cnt));
    TDV_TRY(ws_alloc(ctx, runs, &off));
    TDV_TRY(ws_alloc(ctx, 1, &d_total));
    TDV_TRY(pin_reserve(ctx, sizeof(int)));
    k_tsdf_extract<false, false><<<tiles, TS_T, 0, s>>>(V, prm.min_weight, vol, cnt, nullptr, nullptr, nullptr);
    TDV_TRY(exclusive_scan_dev(ctx, cnt, (int)runs, off, d_total));
    TDV_TRY(fetch_state(ctx, d_total, &total));
    *n_out = total;
    if (total > capacity) return TDV_ERR_BAD_ARG;
    if (total == 0) return TDV_OK;
    if (h_xyz) {
        TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &d_xyz));
        if (h_nrm) TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &d_nrm));
    }
    if (d_nrm) k_tsdf_extract<true, true><<<tiles, TS_T, 0, s>>>(V, prm.min_weight, vol, nullptr, off, d_xyz, d_nrm);
    else k_tsdf_extract<true, false><<<tiles, TS_T, 0, s>>>(V, prm.min_weight, vol, nullptr, off, d_xyz, nullptr);
    TDV_CHECK_LAUNCH(ctx);
    if (!h_xyz) return TDV_OK;
    return download_rows(ctx, (size_t)total, {{h_xyz, d_xyz, 3 * sizeof(float)}, {h_nrm, d_nrm, 3 * sizeof(float)}});
}

bool ts_extract_args_ok(const float* out_xyz, int capacity, const int* n_out) { return capacity >= 0 && n_out && (out_xyz || capacity == 0); }

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_tsdf_default_params(tdv_tsdf_params* p) {
    if (!p) return;
    p->trunc = 0.f; p->max_weight = 255.f; p->zmax = 10.f; p->min_weight = 1.f; p->pose_direction = TDV_POSE_MODEL_TO_CAMERA;
}

unsigned long long tdv_tsdf_volume_bytes(const tdv_tsdf_volume* vol) { return (unsigned long long)ts_voxels(vol) * sizeof(TsPair); }

int tdv_tsdf_reset_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume) {
    const size_t nvox = ts_voxels(vol);
    if (!ctx || !nvox || !d_volume) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return ts_reset(ctx, nvox, d_volume);
}

int tdv_tsdf_integrate_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, float* d_volume, const uint16_t* d_raw, int n_frames, int width, int height,
                           float scale, float fx, float fy, float cx, float cy, const float* h_poses, const tdv_tsdf_params* params,
                           long long* h_n_updated) {
    if (!ctx || !ts_voxels(vol) || !d_volume || !ts_params_ok(params) || !ts_frames_ok(d_raw, n_frames, width, height, scale, fx, fy, h_poses))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return ts_integrate(ctx, *vol, d_volume, d_raw, n_frames, width, height, scale, fx, fy, cx, cy, h_poses, *params, h_n_updated);
}

int tdv_tsdf_extract_dev(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const float* d_volume, const tdv_tsdf_params* params, float* d_out_xyz,
                         float* d_out_normals, int capacity, int* n_out) {
    if (!ctx || !ts_voxels(vol) || !d_volume || !ts_params_ok(params) || !ts_extract_args_ok(d_out_xyz, capacity, n_out)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    return ts_extract(ctx, *vol, d_volume, *params, d_out_xyz, d_out_normals, capacity, n_out, nullptr, nullptr);
}

int tdv_tsdf_fuse(tdv_ctx* ctx, const tdv_tsdf_volume* vol, const uint16_t* raw, int n_frames, int width, int height, float scale, float fx,
                  float fy, float cx, float cy, const float* poses, const tdv_tsdf_params* params, float* out_xyz, float* out_normals,
                  int capacity, int* n_out) {
    const size_t nvox = ts_voxels(vol);
    if (!ctx || !nvox || nvox > (size_t)TDV_TSDF_HOST_MAX_VOXELS || !ts_params_ok(params) ||
        !ts_frames_ok(raw, n_frames, width, height, scale, fx, fy, poses) || !ts_extract_args_ok(out_xyz, capacity, n_out))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float* d_volume;
    uint16_t* d_raw;
    TDV_TRY(ws_alloc(ctx, nvox * 2, &d_volume));
    TDV_TRY(upload(ctx, raw, (size_t)n_frames * width * height, &d_raw));
    TDV_TRY(ts_reset(ctx, nvox, d_volume));
    TDV_TRY(ts_integrate(ctx, *vol, d_volume, d_raw, n_frames, width, height, scale, fx, fy, cx, cy, poses, *params, nullptr));
    float dummy;                                             // capacity 0 with a NULL out_xyz is a query: ts_extract writes no row then
    return ts_extract(ctx, *vol, d_volume, *params, nullptr, nullptr, capacity, n_out, out_xyz ? out_xyz : &dummy, out_normals);
}

}  // extern "C"
