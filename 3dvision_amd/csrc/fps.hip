// Farthest point sampling on gfx950: include/tdv_hip.h (tdv_farthest_point_down_sample) states every rule.
//
// A sample is one maximum over 64-bit keys (rule 6), so the two kernel families below give the same bytes whatever order they work in.
// Both keep m_j < 0 as the mark of a row that is out (unusable, selected, or past the end of the cloud): a usable row's m is never
// negative and never -0 (rule 3).  The first sample is a maximum too: every usable row starts with the bits of +inf, and the start row,
// if usable, with those bits + 1 - above every real key, so that rule 5 needs no case of its own.
//
// Workgroup path, k_fps_workgroup<R>: one workgroup of FPS_T = 1,024 lanes per cloud, lane t owns rows t, t + FPS_T, ... (R of them: x, y,
//   z and m in 4 R registers for the whole call).  Per sample: every lane updates its rows and takes its best key; the wave reduces the
//   key with DPP row operations (no LDS); the winner's coordinates come from its owner lane (a chain of selects on the wave-uniform
//   row-in-lane number, then v_readlane); each wave's lane 0 writes (key, x, y, z) into one of two LDS slots; after ONE barrier every
//   wave reduces the 16 candidates itself.  The slot that iteration i + 2 overwrites was last read before the barrier of iteration i + 1.
//   The owner thread writes the sample's outputs.  The last maximum is cover_d2 (rule 9).
//   Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage, R = 16): see DESIGN.md 7; 1,024 lanes leave 128 VGPRs per lane,
//   R = 16 takes 64 of them for the rows: TDV_FPS_WORKGROUP_MAX = 16 x 1,024.
// Grid path, for larger clouds: k_fps_grid_init packs (x, y, z, m) per row and takes sample 0's maximum into slot 0; launch i of
//   k_fps_grid_step reads sample i - 1 from slot i - 1 - final, the launch before has completed -, writes its outputs, updates every
//   row's m and sends one 64-bit atomicMax per workgroup into slot i.  A slot is FPS_SUB words, workgroup b's maximum goes to word
//   b % FPS_SUB and the reader takes the maximum of the words (with one word per slot a sample at 200 k rows took 11.4 us, most of it
//   the 782 atomics on that word).  No kernel waits for another workgroup; the host enqueues
//   min(num_samples, n) launches back to back and never looks in between (a launch whose slot is 0 - fewer usable rows than samples -
//   returns at once).  k_fps_grid_finish writes the counts and cover_d2.
// Everything a kernel reads from the workspace is written by the call first: the records and the slots by a memset, the packed rows by
// k_fps_grid_init, the batch's plan by k_fps_count and k_fps_plan.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace tdv {

namespace {

constexpr int FPS_T = TDV_FPS_WORKGROUP_LANES;
constexpr int FPS_WAVES = FPS_T / 64;
constexpr int FPS_RMAX = TDV_FPS_WORKGROUP_MAX / FPS_T;
constexpr unsigned FPS_INF = 0x7f800000u;
constexpr int FPS_SUB = 16;                   // words of a grid-path slot: workgroup b sends its maximum to word b % FPS_SUB (one word takes ~90 atomics per microsecond)
constexpr int FPS_GRID_BLOCKS = 1024;         // most workgroups of 256 a grid-path launch uses; rows beyond are taken in turns
static_assert(FPS_T == 1024 && FPS_RMAX == 16, "the owner arithmetic below (j & 1023, j >> 10) and the dispatch on R assume these");

// device record of one cloud (workspace), read back at the end
struct FpsRec { int n_usable, n_selected; float cover_d2; int out_off; };
// one cloud of a call: rows [in_off, in_off + n) of the arrays, start row, its record
struct FpsCloud { int in_off, n, start, id; };
// the outputs of a call (each optional)
struct FpsOut { int* index = nullptr; float* d2 = nullptr; float* xyz = nullptr; float* attr = nullptr; };

__device__ __forceinline__ bool fps_usable(float x, float y, float z) {       // rule 1 (NaN fails every comparison)
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

__device__ __forceinline__ float fps_d2(float x, float y, float z, float sx, float sy, float sz) {   // rule 3
    const float dx = x - sx, dy = y - sy, dz = z - sz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ unsigned long long fps_key(float m, int j) {      // rule 6, for a row that is in
    return ((unsigned long long)__float_as_uint(m) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
}

// sample 0 (rule 5): +inf for every usable row, one more for the start row
__device__ __forceinline__ unsigned long long fps_first_key(bool usable, int j, int start) {
    if (!usable) return 0;
    return ((unsigned long long)(j == start ? FPS_INF + 1u : FPS_INF) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
}

__device__ __forceinline__ float fps_key_d2(unsigned long long key) {         // the m in a key (the start row's extra bit taken off)
    return __uint_as_float(min((unsigned)(key >> 32), FPS_INF));
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long fps_dpp_max(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xF, false);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;     // 0, the maximum's identity, in the rows a broadcast leaves out
    return o > v ? o : v;
}

// every lane of a 16-lane row holds the row's maximum
__device__ __forceinline__ unsigned long long fps_row_max(unsigned long long v) {
    v = fps_dpp_max<0xB1, 0xF>(v);     // quad_perm [1,0,3,2]
    v = fps_dpp_max<0x4E, 0xF>(v);     // quad_perm [2,3,0,1]
    v = fps_dpp_max<0x141, 0xF>(v);    // row_half_mirror
    return fps_dpp_max<0x140, 0xF>(v); // row_mirror
}

// maximum over the 64 lanes, wave-uniform (as wave_sum_i32: valid in lane 63)
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long v) {
    v = fps_row_max(v);
    v = fps_dpp_max<0x142, 0xA>(v);    // row_bcast15 into rows 1 and 3
    v = fps_dpp_max<0x143, 0xC>(v);    // row_bcast31 into rows 2 and 3
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// maximum of the first 16 lanes' values, wave-uniform; every lane of the wave is active
__device__ __forceinline__ unsigned long long fps_row0_max(unsigned long long v) {
    v = fps_row_max(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ float fps_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <int R>
__global__ __launch_bounds__(FPS_T)
void k_fps_workgroup(const float* __restrict__ xyz, FpsCloud one, const FpsCloud* __restrict__ many, const int* __restrict__ list, int k,
                     FpsRec* __restrict__ rec, int* __restrict__ index, float* __restrict__ out_d2, float* __restrict__ out_xyz) {
    __shared__ unsigned long long s_key[2][FPS_WAVES];
    __shared__ float s_x[2][FPS_WAVES], s_y[2][FPS_WAVES], s_z[2][FPS_WAVES];
    __shared__ int s_cnt[FPS_WAVES];
    const FpsCloud c = many ? many[list[blockIdx.x]] : one;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* __restrict__ p = xyz + 3 * (size_t)c.in_off;
    float x[R], y[R], z[R], m[R];
    unsigned long long best = 0;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = t + r * FPS_T;
        const bool in = j < c.n;
        x[r] = in ? p[3 * (size_t)j] : 0.f; y[r] = in ? p[3 * (size_t)j + 1] : 0.f; z[r] = in ? p[3 * (size_t)j + 2] : 0.f;
        const bool usable = in && fps_usable(x[r], y[r], z[r]);
        m[r] = usable ? INFINITY : -1.f;
        cnt += usable ? 1 : 0;
        const unsigned long long key = fps_first_key(usable, j, c.start);
        best = key > best ? key : best;
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    int n_usable = 0;
#pragma unroll
    for (int w = 0; w < FPS_WAVES; ++w) n_usable += s_cnt[w];
    n_usable = __builtin_amdgcn_readfirstlane(n_usable);
    const int n_sel = min(k, n_usable);
    const int out_off = rec[c.id].out_off;
    for (int i = 0; i < n_sel; ++i) {
        const int b = i & 1;
        {   // this wave's candidate, with its coordinates from the owner lane
            const unsigned long long wkey = fps_wave_max(best);
            const unsigned wj = 0xFFFFFFFFu - (unsigned)wkey;
            const unsigned rs = wj >> 10;                    // wave-uniform; past R for a wave without a candidate (key 0 never wins)
            float wx = x[0], wy = y[0], wz = z[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                wx = rs == (unsigned)r ? x[r] : wx; wy = rs == (unsigned)r ? y[r] : wy; wz = rs == (unsigned)r ? z[r] : wz;
            }
            const int src = (int)(wj & 63u);
            wx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wx), src));
            wy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wy), src));
            wz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wz), src));
            if (lane == 0) { s_key[b][wave] = wkey; s_x[b][wave] = wx; s_y[b][wave] = wy; s_z[b][wave] = wz; }
        }
        __syncthreads();
        const unsigned long long g = fps_row0_max(lane < FPS_WAVES ? s_key[b][lane] : 0ull);
        const int gj = (int)(0xFFFFFFFFu - (unsigned)g);
        const int gw = (gj & (FPS_T - 1)) >> 6;
        const float sx = fps_uniform(s_x[b][gw]), sy = fps_uniform(s_y[b][gw]), sz = fps_uniform(s_z[b][gw]);
        if (t == (gj & (FPS_T - 1))) {                       // rule 8, from the owner
            const size_t o = (size_t)out_off + (size_t)i;
            if (index) index[o] = gj;
            if (out_d2) out_d2[o] = fps_key_d2(g);
            if (out_xyz) { out_xyz[3 * o] = sx; out_xyz[3 * o + 1] = sy; out_xyz[3 * o + 2] = sz; }
        }
        best = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {                        // rules 4, 6 and 7
            const int j = t + r * FPS_T;
            float mr = j == gj ? -1.f : m[r];
            const float d = fps_d2(x[r], y[r], z[r], sx, sy, sz);
            const bool alive = mr >= 0.f;
            mr = (alive && d < mr) ? d : mr;
            m[r] = mr;
            const unsigned long long key = alive ? fps_key(mr, j) : 0ull;
            best = key > best ? key : best;
        }
    }
    // rule 9: the maximum that would choose the next sample
    const int b = n_sel & 1;
    const unsigned long long wkey = fps_wave_max(best);
    if (lane == 0) s_key[b][wave] = wkey;
    __syncthreads();
    const unsigned long long g = fps_row0_max(lane < FPS_WAVES ? s_key[b][lane] : 0ull);
    if (t == 0) { rec[c.id].n_usable = n_usable; rec[c.id].n_selected = n_sel; rec[c.id].cover_d2 = fps_key_d2(g); }
}

// maximum over a workgroup of 256, valid in thread 0
__device__ __forceinline__ unsigned long long fps_block256_max(unsigned long long v, unsigned long long* lds4) {
    v = fps_wave_max(v);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned long long a = lds4[0] > lds4[1] ? lds4[0] : lds4[1], b = lds4[2] > lds4[3] ? lds4[2] : lds4[3];
    return a > b ? a : b;
}

__global__ __launch_bounds__(256)
void k_fps_grid_init(const float* __restrict__ xyz, FpsCloud c, float4* __restrict__ P, unsigned long long* __restrict__ slot, FpsRec* __restrict__ rec) {
    __shared__ unsigned long long lds4[4];
    __shared__ int ldc4[4];
    const float* __restrict__ p = xyz + 3 * (size_t)c.in_off;
    unsigned long long best = 0;
    int cnt = 0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < c.n; j += gridDim.x * 256) {
        const float x = p[3 * (size_t)j], y = p[3 * (size_t)j + 1], z = p[3 * (size_t)j + 2];
        const bool usable = fps_usable(x, y, z);
        P[j] = make_float4(x, y, z, usable ? INFINITY : -1.f);
        cnt += usable ? 1 : 0;
        const unsigned long long key = fps_first_key(usable, j, c.start);
        best = key > best ? key : best;
    }
    cnt = wave_sum_i32(cnt);
    if ((threadIdx.x & 63) == 0) ldc4[threadIdx.x >> 6] = cnt;
    best = fps_block256_max(best, lds4);                    // (its barrier covers ldc4 too)
    if (threadIdx.x == 0) {
        const int total = (ldc4[0] + ldc4[1]) + (ldc4[2] + ldc4[3]);
        if (total) atomicAdd(&rec[c.id].n_usable, total);
        if (best) atomicMax(&slot[blockIdx.x & (FPS_SUB - 1)], best);
    }
}

// launch i = 1, 2, ...: sample i - 1 is slot[i - 1]; slot[i] receives the maximum after it
__global__ __launch_bounds__(256)
void k_fps_grid_step(const float* __restrict__ xyz, FpsCloud c, float4* __restrict__ P, unsigned long long* __restrict__ slot, int i,
                     const FpsRec* __restrict__ rec, int* __restrict__ index, float* __restrict__ out_d2, float* __restrict__ out_xyz) {
    __shared__ unsigned long long lds4[4];
    const unsigned long long g = fps_row0_max((threadIdx.x & 63) < FPS_SUB ? slot[(size_t)(i - 1) * FPS_SUB + (threadIdx.x & 63)] : 0ull);
    if (g == 0) return;                                     // every usable row is taken: the same in every workgroup
    const int gj = (int)(0xFFFFFFFFu - (unsigned)g);
    const float* __restrict__ p = xyz + 3 * ((size_t)c.in_off + (size_t)gj);
    const float sx = p[0], sy = p[1], sz = p[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) {              // rule 8
        const size_t o = (size_t)rec[c.id].out_off + (size_t)(i - 1);
        if (index) index[o] = gj;
        if (out_d2) out_d2[o] = fps_key_d2(g);
        if (out_xyz) { out_xyz[3 * o] = sx; out_xyz[3 * o + 1] = sy; out_xyz[3 * o + 2] = sz; }
    }
    unsigned long long best = 0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < c.n; j += gridDim.x * 256) {
        const float4 q = P[j];
        if (j == gj) { P[j].w = -1.f; continue; }           // rule 7
        if (!(q.w >= 0.f)) continue;
        const float d = fps_d2(q.x, q.y, q.z, sx, sy, sz);
        float mr = q.w;
        if (d < mr) { mr = d; P[j].w = d; }                 // rule 4
        const unsigned long long key = fps_key(mr, j);
        best = key > best ? key : best;
    }
    best = fps_block256_max(best, lds4);
    if (threadIdx.x == 0 && best) atomicMax(&slot[(size_t)i * FPS_SUB + (blockIdx.x & (FPS_SUB - 1))], best);
}

__global__ void k_fps_grid_finish(const unsigned long long* __restrict__ slot, int k, FpsCloud c, FpsRec* __restrict__ rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int n_sel = min(k, rec[c.id].n_usable);
    rec[c.id].n_selected = n_sel;
    unsigned long long g = 0;                               // rule 9: slot n_sel is the maximum after the last sample (0: none left)
    for (int w = 0; w < FPS_SUB; ++w) g = slot[(size_t)n_sel * FPS_SUB + w] > g ? slot[(size_t)n_sel * FPS_SUB + w] : g;
    rec[c.id].cover_d2 = fps_key_d2(g);
}

// the companion rows of the selected ones: blockIdx.x = cloud (of `many`, or `one`), blockIdx.y strides over its elements
__global__ __launch_bounds__(256)
void k_fps_gather_attr(FpsCloud one, const FpsCloud* __restrict__ many, const FpsRec* __restrict__ rec, const int* __restrict__ index,
                       const float* __restrict__ attr, int width, float* __restrict__ out_attr) {
    const FpsCloud c = many ? many[blockIdx.x] : one;
    const FpsRec r = rec[c.id];
    const size_t total = (size_t)r.n_selected * (size_t)width;
    for (size_t e = (size_t)blockIdx.y * 256 + threadIdx.x; e < total; e += (size_t)gridDim.y * 256) {
        const size_t row = e / (size_t)width, col = e - row * (size_t)width;
        const size_t src = (size_t)c.in_off + (size_t)index[(size_t)r.out_off + row];
        out_attr[(size_t)r.out_off * (size_t)width + e] = attr[src * (size_t)width + col];
    }
}

// batch: usable[b] = the usable rows of cloud b, for the output offsets.  off: the clouds' offsets, [n_clouds + 1]
__global__ __launch_bounds__(256)
void k_fps_count(const float* __restrict__ xyz, const int* __restrict__ off, int n_clouds, int* __restrict__ usable) {
    const int g = blockIdx.x * 256 + threadIdx.x, total = off[n_clouds];
    const bool in = g < total;
    int lo = 0, hi = n_clouds;                               // the last b with off[b] <= g
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
    const bool u = in && fps_usable(xyz[3 * (size_t)(in ? g : 0)], xyz[3 * (size_t)(in ? g : 0) + 1], xyz[3 * (size_t)(in ? g : 0) + 2]);
    const int b0 = __builtin_amdgcn_readfirstlane(lo);
    if (__all(!in || lo == b0)) {                            // the wave lies in one cloud: one add
        const int c = __popcll(__ballot(u));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&usable[b0], c);
    } else if (u) atomicAdd(&usable[lo], 1);
}

// batch: rec[b].out_off = the sum over a < b of min(k, usable[a]); one workgroup
__global__ __launch_bounds__(1024)
void k_fps_plan(const int* __restrict__ usable, int n_clouds, int k, FpsRec* __restrict__ rec) {
    __shared__ int s[1024];
    int carry = 0;
    for (int base = 0; base < n_clouds; base += 1024) {
        const int b = base + (int)threadIdx.x;
        const int v = b < n_clouds ? min(k, usable[b]) : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int a = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += a;
            __syncthreads();
        }
        if (b < n_clouds) rec[b].out_off = carry + s[threadIdx.x] - v;
        carry += s[1023];
        __syncthreads();
    }
}

int fps_choose(const tdv_ctx* ctx, int n) {
    return ctx->fps_path != TDV_FPS_AUTO ? ctx->fps_path : (n <= TDV_FPS_WORKGROUP_MAX ? TDV_FPS_WORKGROUP : TDV_FPS_GRID);
}

bool fps_attr_ok(const float* attr, int attr_width, const float* out_attr) {
    return attr_width >= 0 && !(attr_width > 0 && !attr) && !(out_attr && !attr);
}

// smallest rows-per-lane count of the dispatch that holds n rows
int fps_rows_class(int n) {
    int cls = 0;
    while ((FPS_T << cls) < n) ++cls;
    return cls;                                              // R = 1 << cls, cls in [0, 4]
}

int fps_launch_workgroup(tdv_ctx* ctx, int cls, int blocks, const float* d_xyz, FpsCloud one, const FpsCloud* many, const int* list, int k, FpsRec* rec,
                         const FpsOut& d) {
    hipStream_t s = ctx->stream;
    switch (cls) {
        case 0: k_fps_workgroup<1><<<blocks, FPS_T, 0, s>>>(d_xyz, one, many, list, k, rec, d.index, d.d2, d.xyz); break;
        case 1: k_fps_workgroup<2><<<blocks, FPS_T, 0, s>>>(d_xyz, one, many, list, k, rec, d.index, d.d2, d.xyz); break;
        case 2: k_fps_workgroup<4><<<blocks, FPS_T, 0, s>>>(d_xyz, one, many, list, k, rec, d.index, d.d2, d.xyz); break;
        case 3: k_fps_workgroup<8><<<blocks, FPS_T, 0, s>>>(d_xyz, one, many, list, k, rec, d.index, d.d2, d.xyz); break;
        default: k_fps_workgroup<16><<<blocks, FPS_T, 0, s>>>(d_xyz, one, many, list, k, rec, d.index, d.d2, d.xyz); break;
    }
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// one cloud through the grid path; P ([c.n]) and slot ([(min(k, c.n) + 1) * FPS_SUB]) are the caller's workspace
int fps_launch_grid(tdv_ctx* ctx, const float* d_xyz, FpsCloud c, int k, float4* P, unsigned long long* slot, FpsRec* rec, const FpsOut& d) {
    hipStream_t s = ctx->stream;
    const int launches = std::min(k, c.n);
    const int blocks = std::min((c.n + 255) / 256, FPS_GRID_BLOCKS);
    TDV_HIP(ctx, hipMemsetAsync(slot, 0, ((size_t)launches + 1) * FPS_SUB * sizeof(unsigned long long), s));
    k_fps_grid_init<<<blocks, 256, 0, s>>>(d_xyz, c, P, slot, rec);
    for (int i = 1; i <= launches; ++i) k_fps_grid_step<<<blocks, 256, 0, s>>>(d_xyz, c, P, slot, i, rec, d.index, d.d2, d.xyz);
    k_fps_grid_finish<<<1, 64, 0, s>>>(slot, k, c, rec);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

int fps_gather_blocks(long long elements) { return (int)std::max(1LL, std::min(64LL, (elements + 255) / 256)); }

// every argument, before anything is enqueued (include/tdv_hip.h)
bool fps_args_ok(const tdv_ctx* ctx, const float* xyz, int n, int num_samples, int start_index, const float* attr, int attr_width,
                 const tdv_fps_result* result, const float* out_attr) {
    if (!ctx || !result || n < 0 || n > TDV_FPS_MAX_POINTS || (n > 0 && !xyz) || num_samples < 0) return false;
    if (n > 0 && (start_index < 0 || start_index >= n)) return false;
    if (ctx->fps_path == TDV_FPS_WORKGROUP && n > TDV_FPS_WORKGROUP_MAX) return false;
    return fps_attr_ok(attr, attr_width, out_attr);
}

bool fps_batch_args_ok(const tdv_ctx* ctx, const float* d_xyz, const float* d_attr, int attr_width, const int* h_off, int n_clouds,
                       int num_samples, const tdv_fps_result* results, const int* h_out_off, const float* d_out_attr) {
    if (!ctx || n_clouds < 0 || !h_off || !h_out_off || (n_clouds > 0 && !results) || num_samples < 0) return false;
    if (h_off[0] != 0) return false;
    for (int b = 0; b < n_clouds; ++b) {
        if (h_off[b + 1] < h_off[b]) return false;
        const int n = h_off[b + 1] - h_off[b];
        if (n > TDV_FPS_MAX_POINTS || (ctx->fps_path == TDV_FPS_WORKGROUP && n > TDV_FPS_WORKGROUP_MAX)) return false;
    }
    if (h_off[n_clouds] > 0 && !d_xyz) return false;
    return fps_attr_ok(d_attr, attr_width, d_out_attr);
}

// The whole call on device memory.  h (host entry point): where the device outputs go.
int fps_run_dev(tdv_ctx* ctx, const float* d_xyz, int n, int num_samples, int start_index, const float* d_attr, int attr_width,
                tdv_fps_result* result, FpsOut d, const FpsOut* h) {
    std::memset(result, 0, sizeof(*result));
    const int path = fps_choose(ctx, n);
    ctx->last_fps_path = path;
    result->path = path;
    if (n == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    const int cap = std::min(num_samples, n);
    if (!d_attr || attr_width == 0) d.attr = nullptr;
    if (d.attr && !d.index) TDV_TRY(ws_alloc(ctx, (size_t)std::max(cap, 1), &d.index));
    FpsRec* rec;
    TDV_TRY(ws_alloc(ctx, 1, &rec));
    TDV_TRY(pin_reserve(ctx, sizeof(FpsRec)));
    TDV_HIP(ctx, hipMemsetAsync(rec, 0, sizeof(FpsRec), s));
    const FpsCloud c{0, n, start_index, 0};
    if (path == TDV_FPS_WORKGROUP) {
        TDV_TRY(fps_launch_workgroup(ctx, fps_rows_class(n), 1, d_xyz, c, nullptr, nullptr, num_samples, rec, d));
    } else {
        float4* P; unsigned long long* slot;
        TDV_TRY(ws_alloc(ctx, (size_t)n, &P));
        TDV_TRY(ws_alloc(ctx, ((size_t)cap + 1) * FPS_SUB, &slot));
        TDV_TRY(fps_launch_grid(ctx, d_xyz, c, num_samples, P, slot, rec, d));
    }
    if (d.attr && cap > 0) {
        k_fps_gather_attr<<<dim3(1, fps_gather_blocks((long long)cap * attr_width)), 256, 0, s>>>(c, nullptr, rec, d.index, d_attr, attr_width, d.attr);
        TDV_CHECK_LAUNCH(ctx);
    }
    FpsRec hr;
    TDV_TRY(fetch_state(ctx, rec, &hr));
    result->n_usable = hr.n_usable; result->n_selected = hr.n_selected; result->cover_d2 = hr.cover_d2;
    // host entry point: the selected rows, n_selected of them
    if (!h) return TDV_OK;
    return download_rows(ctx, (size_t)hr.n_selected, {{h->index, d.index, sizeof(int)}, {h->d2, d.d2, sizeof(float)},
                                                      {h->xyz, d.xyz, 3 * sizeof(float)}, {h->attr, d.attr, (size_t)attr_width * sizeof(float)}});
}

// host arrays: upload, device outputs for what is asked for, fps_run_dev
int fps_run_host(tdv_ctx* ctx, const float* xyz, int n, int num_samples, int start_index, const float* attr, int attr_width,
                 tdv_fps_result* result, const FpsOut& h) {
    TDV_TRY(call_begin(ctx));
    float *d_xyz, *d_attr = nullptr;
    FpsOut d;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    if (n > 0) {
        const size_t cap = (size_t)std::max(std::min(num_samples, n), 1);
        if (h.attr) {                                        // the rows are only ever gathered
            TDV_TRY(upload(ctx, attr, (size_t)n * (size_t)attr_width, &d_attr));
            if (d_attr) TDV_TRY(ws_alloc(ctx, cap * (size_t)attr_width, &d.attr));
        }
        if (h.index) TDV_TRY(ws_alloc(ctx, cap, &d.index));
        if (h.d2) TDV_TRY(ws_alloc(ctx, cap, &d.d2));
        if (h.xyz) TDV_TRY(ws_alloc(ctx, cap * 3, &d.xyz));
    }
    return fps_run_dev(ctx, d_xyz, n, num_samples, start_index, d_attr, attr_width, result, d, &h);
}

int fps_batch_run_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_attr, int attr_width, const int* h_off, int n_clouds, int num_samples,
                      tdv_fps_result* results, int* h_out_off, FpsOut d) {
    h_out_off[0] = 0;
    int last = TDV_FPS_WORKGROUP, n_max_grid = 0, n_run = 0;
    long long cap_total = 0;
    for (int b = 0; b < n_clouds; ++b) {
        const int n = h_off[b + 1] - h_off[b];
        std::memset(&results[b], 0, sizeof(results[b]));
        results[b].path = fps_choose(ctx, n);
        h_out_off[b + 1] = 0;
        if (results[b].path == TDV_FPS_GRID) { last = TDV_FPS_GRID; n_max_grid = std::max(n_max_grid, n); }
        cap_total += std::min(num_samples, n);
        n_run += n > 0 ? 1 : 0;
    }
    if (n_clouds > 0 && ctx->fps_path != TDV_FPS_AUTO) last = ctx->fps_path;
    ctx->last_fps_path = last;
    if (n_run == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    if (!d_attr || attr_width == 0) d.attr = nullptr;
    if (d.attr && !d.index) TDV_TRY(ws_alloc(ctx, (size_t)std::max(cap_total, 1LL), &d.index));
    // one upload: the clouds, the offsets, and per rows-per-lane class the list of its clouds
    const size_t up_ints = (size_t)n_clouds * 4 + ((size_t)n_clouds + 1) + (size_t)n_clouds;
    const size_t up_bytes = align_up(up_ints * sizeof(int), 256), down_bytes = (size_t)n_clouds * sizeof(FpsRec);
    TDV_TRY(pin_reserve(ctx, up_bytes + down_bytes));
    int* up = reinterpret_cast<int*>(ctx->pin);
    FpsCloud* hc = reinterpret_cast<FpsCloud*>(up);
    int* hoff = up + (size_t)n_clouds * 4;
    int* hlist = hoff + n_clouds + 1;
    int cls_begin[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < n_clouds; ++b) hc[b] = FpsCloud{h_off[b], h_off[b + 1] - h_off[b], 0, b};
    std::memcpy(hoff, h_off, ((size_t)n_clouds + 1) * sizeof(int));
    int filled = 0;
    for (int cls = 0; cls < 5; ++cls) {
        cls_begin[cls] = filled;
        for (int b = 0; b < n_clouds; ++b)
            if (hc[b].n > 0 && results[b].path == TDV_FPS_WORKGROUP && fps_rows_class(hc[b].n) == cls) hlist[filled++] = b;
    }
    cls_begin[5] = filled;
    int *d_up, *usable;
    FpsRec* rec;
    TDV_TRY(ws_alloc(ctx, up_ints, &d_up));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds, &usable));
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds, &rec));
    float4* P = nullptr; unsigned long long* slot = nullptr;
    if (n_max_grid > 0) {
        TDV_TRY(ws_alloc(ctx, (size_t)n_max_grid, &P));
        TDV_TRY(ws_alloc(ctx, ((size_t)std::min(num_samples, n_max_grid) + 1) * FPS_SUB, &slot));
    }
    TDV_HIP(ctx, hipMemcpyAsync(d_up, up, up_ints * sizeof(int), hipMemcpyHostToDevice, s));
    TDV_HIP(ctx, hipMemsetAsync(usable, 0, (size_t)n_clouds * sizeof(int), s));
    TDV_HIP(ctx, hipMemsetAsync(rec, 0, (size_t)n_clouds * sizeof(FpsRec), s));
    const FpsCloud* d_clouds = reinterpret_cast<const FpsCloud*>(d_up);
    const int* d_off = d_up + (size_t)n_clouds * 4;
    const int* d_list = d_off + n_clouds + 1;
    const int total = h_off[n_clouds];
    k_fps_count<<<(total + 255) / 256, 256, 0, s>>>(d_xyz, d_off, n_clouds, usable);
    k_fps_plan<<<1, 1024, 0, s>>>(usable, n_clouds, num_samples, rec);
    TDV_CHECK_LAUNCH(ctx);
    for (int cls = 0; cls < 5; ++cls)
        if (cls_begin[cls + 1] > cls_begin[cls])
            TDV_TRY(fps_launch_workgroup(ctx, cls, cls_begin[cls + 1] - cls_begin[cls], d_xyz, FpsCloud{}, d_clouds, d_list + cls_begin[cls], num_samples, rec, d));
    for (int b = 0; b < n_clouds; ++b)
        if (hc[b].n > 0 && results[b].path == TDV_FPS_GRID) TDV_TRY(fps_launch_grid(ctx, d_xyz, hc[b], num_samples, P, slot, rec, d));
    if (d.attr && cap_total > 0) {
        int cap_max = 0;
        for (int b = 0; b < n_clouds; ++b) cap_max = std::max(cap_max, std::min(num_samples, hc[b].n));
        k_fps_gather_attr<<<dim3(n_clouds, fps_gather_blocks((long long)cap_max * attr_width)), 256, 0, s>>>(FpsCloud{}, d_clouds, rec, d.index, d_attr, attr_width, d.attr);
        TDV_CHECK_LAUNCH(ctx);
    }
    char* down = ctx->pin + up_bytes;
    TDV_HIP(ctx, hipMemcpyAsync(down, rec, down_bytes, hipMemcpyDeviceToHost, s));
    TDV_HIP(ctx, hipStreamSynchronize(s));
    for (int b = 0; b < n_clouds; ++b) {
        FpsRec hr;
        std::memcpy(&hr, down + (size_t)b * sizeof(FpsRec), sizeof(hr));
        results[b].n_usable = hr.n_usable; results[b].n_selected = hr.n_selected; results[b].cover_d2 = hr.cover_d2;
        h_out_off[b + 1] = h_out_off[b] + hr.n_selected;
    }
    return TDV_OK;
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

int tdv_farthest_point_down_sample(tdv_ctx* ctx, const float* xyz, int n, int num_samples, int start_index, const float* attr, int attr_width,
                                   tdv_fps_result* result, int* index, float* out_d2, float* out_xyz, float* out_attr) {
    if (!fps_args_ok(ctx, xyz, n, num_samples, start_index, attr, attr_width, result, out_attr)) return TDV_ERR_BAD_ARG;
    FpsOut h; h.index = index; h.d2 = out_d2; h.xyz = out_xyz; h.attr = out_attr;
    return fps_run_host(ctx, xyz, n, num_samples, start_index, attr, attr_width, result, h);
}

int tdv_farthest_point_down_sample_dev(tdv_ctx* ctx, const float* d_xyz, int n, int num_samples, int start_index, const float* d_attr,
                                       int attr_width, tdv_fps_result* result, int* d_index, float* d_out_d2, float* d_out_xyz,
                                       float* d_out_attr) {
    if (!fps_args_ok(ctx, d_xyz, n, num_samples, start_index, d_attr, attr_width, result, d_out_attr)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    FpsOut d; d.index = d_index; d.d2 = d_out_d2; d.xyz = d_out_xyz; d.attr = d_out_attr;
    return fps_run_dev(ctx, d_xyz, n, num_samples, start_index, d_attr, attr_width, result, d, nullptr);
}

int tdv_farthest_point_down_sample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_attr, int attr_width, const int* h_offsets,
                                             int n_clouds, int num_samples, tdv_fps_result* results, int* h_out_offsets, int* d_index,
                                             float* d_out_d2, float* d_out_xyz, float* d_out_attr) {
    if (!fps_batch_args_ok(ctx, d_xyz, d_attr, attr_width, h_offsets, n_clouds, num_samples, results, h_out_offsets, d_out_attr)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    FpsOut d; d.index = d_index; d.d2 = d_out_d2; d.xyz = d_out_xyz; d.attr = d_out_attr;
    return fps_batch_run_dev(ctx, d_xyz, d_attr, attr_width, h_offsets, n_clouds, num_samples, results, h_out_offsets, d);
}

}  // extern "C"
