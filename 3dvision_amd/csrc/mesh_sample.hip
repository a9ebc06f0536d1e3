// Mesh sampling on gfx950: include/tdv_hip.h (tdv_mesh_sample_points) states every rule, S1 to S7.
//
// A sample is a function of the mesh, the seed and its global index alone (S7): its triangle comes from an integer search over the
// inclusive prefix sums C of integer weights (S3, S4), its barycentric coordinates are integers (S5), and the f32 expressions of S2 and
// S6 are evaluated as written.  Nothing below depends on the order the device works in: the maximum is over u32 bits, the counts and the
// sums are integers.
//   k_ms_area      one lane per triangle: S1 and S2.  area[t] = the bits of the area, MS_BAD for a bad triangle; n_bad and area_max go
//                  to the record through at most one atomic each per workgroup (the maximum over the u32 bits of a non-negative f32;
//                  none where the workgroup has no bad triangle, or a maximum the record already holds).
//   k_ms_sums      the weights (S3) of MS_T triangles per workgroup: their sum and how many are usable and degenerate, one record each.
//   k_ms_scan_sums one workgroup: the exclusive prefix sums of the workgroup sums in place, MS_SCAN_T at a time with a carry; W, n_sampled
//                  and the counts' sums.
//   k_ms_prefix    the weights again (two conversions cost less than 16 bytes of traffic per triangle), the workgroup's inclusive scan plus
//                  its sum's prefix: C.  2^22 triangles are 16,384 workgroup sums, 16 turns of k_ms_scan_sums: no third level.
//   k_ms_sample    one lane per sample: Philox, the high product, a branch-free upper-bound search over C - its coarse levels over a table
//                  of at most 4,096 entries that the workgroup stages in LDS (all of C up to 4,096 triangles), the rest, at most ten steps
//                  of one 8-byte load, in global memory -, three vertex fetches, the row stores.  The normal is formed again from the
//                  vertices the lane has fetched anyway.  It reads W from the record: with W == 0 it writes nothing, and the host learns
//                  n_sampled from the one read-back.
// The launches follow each other on the ctx's stream; no kernel waits on another workgroup.  Everything a kernel reads from the workspace
// is written by the call first: the record by a memset, area by k_ms_area, the sums by k_ms_sums, C by k_ms_prefix.
// The search with every step in global memory lost its measurement and lives on in the study build: DESIGN.md 7, "Mesh sampling".
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "philox.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace tdv {

namespace {

constexpr int MS_T = 256;                      // triangles of a workgroup in the three per-triangle kernels
constexpr int MS_LDS_N = 4096;                 // entries of C's coarse table in k_ms_sample's LDS: 32 KiB
constexpr int MS_LDS_T = 1024, MS_PER = 4;     // k_ms_sample: lanes of a workgroup and samples per lane - one staging serves 4,096 samples
constexpr int MS_SCAN_T = 1024;                // workgroup sums k_ms_scan_sums takes per turn
constexpr unsigned MS_BAD = 0xFFFFFFFFu;       // area[t] of a bad triangle: above the bits of every finite non-negative f32
constexpr unsigned MS_ONE = 1u << 24;          // S5's 2^24
constexpr unsigned MS_KEY_TAG = 2u;            // S4: Philox key word 1 of this stage

typedef tdv_mesh_sample_result MsRec;          // the device record is the result itself (area_max through its u32 bits)
static_assert(sizeof(MsRec) == 32 && sizeof(tdv_mesh_sample_params) == 16, "include/tdv_hip.h: the structs' layout");

// the outputs of a call (each optional)
struct MsOut { float* xyz = nullptr; float* normals = nullptr; int* triangle = nullptr; float* bary = nullptr; float* attr = nullptr; };
// a row of out_xyz / out_normals and of out_bary: 4-byte aligned like the float arrays they lie in, stored whole
struct MsRow3 { float x, y, z; };
struct MsRow2 { float u, v; };
// what k_ms_sums leaves per workgroup: the sum of its weights (k_ms_scan_sums turns it into the sum of the workgroups before) and its counts
struct MsSum { unsigned long long w; int usable, degenerate; };

__device__ __forceinline__ bool ms_finite(float x) { return fabsf(x) < INFINITY; }     // (NaN fails every comparison)

// S1 and S2 for triangle t: false for a bad index or a non-finite coordinate - the indices are tested before any vertex is read.
// a, b, c: the vertices; n, L: the normal before its division and its length (the caller tests the area)
__device__ __forceinline__ bool ms_triangle(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int t, float (&a)[3],
                                            float (&b)[3], float (&c)[3], float (&n)[3], float& L) {
    const int ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
    if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = vtx[3 * (size_t)ia + k]; b[k] = vtx[3 * (size_t)ib + k]; c[k] = vtx[3 * (size_t)ic + k];
        ok = ok && ms_finite(a[k]) && ms_finite(b[k]) && ms_finite(c[k]);
    }
    if (!ok) return false;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2], e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    n[0] = e1y * e2z - e1z * e2y; n[1] = e1z * e2x - e1x * e2z; n[2] = e1x * e2y - e1y * e2x;
    L = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    return true;
}

// S3: what a weight is scaled by, and e.  area_max == 0: e = 0, and the caller's weights are 0
struct MsScale { double scale; int e; bool any; };
__device__ __forceinline__ MsScale ms_scale(unsigned area_max_bits) {
    MsScale s{0.0, 0, area_max_bits != 0u};
    if (!s.any) return s;
    const double m = (double)__uint_as_float(area_max_bits);                          // exact, and normal in f64 whatever the f32 was
    s.e = (int)((__double_as_longlong(m) >> 52) & 0x7FF) - 1023;
    s.scale = __longlong_as_double((long long)(1023 + 31 - s.e) << 52);               // 2^(31 - e), 31 - e in [-96, 180]
    return s;
}
__device__ __forceinline__ unsigned long long ms_weight(unsigned area_bits, const MsScale& s) {
    if (area_bits == MS_BAD || !s.any) return 0ull;
    return (unsigned long long)((double)__uint_as_float(area_bits) * s.scale);        // exact product, truncated; below 2^32
}

// inclusive prefix sums over a workgroup of T lanes in LDS (s[T]); the workgroup's sum is s[T - 1] afterwards
template <int T>
__device__ __forceinline__ unsigned long long ms_block_scan(unsigned long long v, unsigned long long* s) {
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < T; d <<= 1) {
        const unsigned long long a = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0ull;
        __syncthreads();
        s[threadIdx.x] += a;
        __syncthreads();
    }
    return s[threadIdx.x];
}

__global__ __launch_bounds__(MS_T)
void k_ms_area(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int nt, unsigned* __restrict__ area, MsRec* rec) {
    __shared__ unsigned s_max;
    __shared__ int s_bad;
    if (threadIdx.x == 0) { s_max = 0u; s_bad = 0; }
    __syncthreads();
    const int t = blockIdx.x * MS_T + (int)threadIdx.x;
    unsigned bits = MS_BAD;
    if (t < nt) {
        float a[3], b[3], c[3], n[3], L;
        if (ms_triangle(vtx, nv, tri, t, a, b, c, n, L)) {
            const float ar = 0.5f * L;
            if (ms_finite(ar)) bits = __float_as_uint(ar);
        }
        area[t] = bits;
    }
    const int bad = wave_sum_i32((t < nt && bits == MS_BAD) ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&s_bad, bad);
    if (bits != MS_BAD && bits != 0u) atomicMax(&s_max, bits);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad) atomicAdd(&rec->n_bad, s_bad);
        // a maximum the word already holds needs no atomic (a stale read only costs one): 4,096 workgroups on one word took 45 us
        unsigned* m = reinterpret_cast<unsigned*>(&rec->area_max);
        if (s_max > __atomic_load_n(m, __ATOMIC_RELAXED)) atomicMax(m, s_max);
    }
}

__global__ __launch_bounds__(MS_T)
void k_ms_sums(const unsigned* __restrict__ area, int nt, MsRec* rec, MsSum* __restrict__ sums) {
    __shared__ unsigned long long s[MS_T];
    __shared__ int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    const MsScale sc = ms_scale(__float_as_uint(rec->area_max));                       // final: k_ms_area has completed
    const int t = blockIdx.x * MS_T + (int)threadIdx.x;
    const unsigned bits = t < nt ? area[t] : MS_BAD;
    const unsigned long long w = ms_weight(bits, sc);
    ms_block_scan<MS_T>(w, s);                                                         // (its barriers cover s_cnt's reset)
    const int usable = wave_sum_i32(w != 0ull ? 1 : 0), degenerate = wave_sum_i32((bits != MS_BAD && w == 0ull) ? 1 : 0);
    if ((threadIdx.x & 63) == 0) {
        if (usable) atomicAdd(&s_cnt[0], usable);
        if (degenerate) atomicAdd(&s_cnt[1], degenerate);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = MsSum{s[MS_T - 1], s_cnt[0], s_cnt[1]};
        if (blockIdx.x == 0) rec->weight_exponent = sc.e;
    }
}

// one workgroup: sums[b].w becomes the sum of the workgroups before b; W, n_sampled and the two counts into the record (the counts
// summed here, not by an atomic per workgroup of k_ms_sums on one word)
__global__ __launch_bounds__(MS_SCAN_T)
void k_ms_scan_sums(MsSum* __restrict__ sums, int nb, int n_samples, MsRec* rec) {
    __shared__ unsigned long long s[MS_SCAN_T];
    unsigned long long carry = 0, counts = 0;                                          // counts: (usable << 32) | degenerate, each at most 2^22
    for (int base = 0; base < nb; base += MS_SCAN_T) {
        const int b = base + (int)threadIdx.x;
        const MsSum r = b < nb ? sums[b] : MsSum{0ull, 0, 0};
        counts += ((unsigned long long)(unsigned)r.usable << 32) | (unsigned)r.degenerate;
        const unsigned long long inc = ms_block_scan<MS_SCAN_T>(r.w, s);
        if (b < nb) sums[b].w = carry + (inc - r.w);
        carry += s[MS_SCAN_T - 1];
        __syncthreads();                                                               // the next turn overwrites s
    }
    ms_block_scan<MS_SCAN_T>(counts, s);
    if (threadIdx.x == 0) {
        rec->total_weight = carry; rec->n_sampled = carry != 0ull ? n_samples : 0;
        rec->n_usable = (int)(s[MS_SCAN_T - 1] >> 32); rec->n_degenerate = (int)(unsigned)s[MS_SCAN_T - 1];
    }
}

__global__ __launch_bounds__(MS_T)
void k_ms_prefix(const unsigned* __restrict__ area, int nt, const MsRec* __restrict__ rec, const MsSum* __restrict__ sums,
                 unsigned long long* __restrict__ C) {
    __shared__ unsigned long long s[MS_T];
    const MsScale sc = ms_scale(__float_as_uint(rec->area_max));
    const int t = blockIdx.x * MS_T + (int)threadIdx.x;
    const unsigned long long inc = ms_block_scan<MS_T>(ms_weight(t < nt ? area[t] : MS_BAD, sc), s);
    if (t < nt) C[t] = sums[blockIdx.x].w + inc;
}

// S4's draw for sample k: the target in [0, W) and the Philox words S5 takes
__device__ __forceinline__ unsigned long long ms_draw(unsigned long long g, unsigned seed, unsigned long long W, uint32_t (&x)[4]) {
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, seed, MS_KEY_TAG, x);
    return __umul64hi(((unsigned long long)x[0] << 32) | x[1], W);
}

// the number of entries <= target among c[t0 .. end), added to t0, in steps of `top`, top / 2, ..., 1 - every probe inside [t0, end)
__device__ __forceinline__ int ms_upper_bound(const unsigned long long* __restrict__ c, int t0, int end, int top, unsigned long long target) {
    int t = t0;
    for (int step = top; step > 0; step >>= 1) {
        const int probe = t + step;
        const unsigned long long v = c[min(probe, end) - 1];
        t = (probe <= end && v <= target) ? probe : t;
    }
    return t;
}

// S5 and S6 for sample k in triangle t
__device__ __forceinline__ void ms_emit(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int t, const uint32_t (&x)[4],
                                        const float* __restrict__ attr, int width, int k, const MsOut& out) {
    unsigned i1 = x[2] >> 8, i2 = x[3] >> 8;                                           // S5
    if (i1 + i2 > MS_ONE) { i1 = MS_ONE - i1; i2 = MS_ONE - i2; }
    const float u = (float)i1 * 0x1p-24f, v = (float)i2 * 0x1p-24f, w = (float)(MS_ONE - i1 - i2) * 0x1p-24f;
    float a[3], b[3], c[3], n[3], L;
    ms_triangle(vtx, nv, tri, t, a, b, c, n, L);                                       // w_t > 0: not bad, and L > 0
    if (out.xyz)
        reinterpret_cast<MsRow3*>(out.xyz)[k] = MsRow3{(w * a[0] + u * b[0]) + v * c[0], (w * a[1] + u * b[1]) + v * c[1], (w * a[2] + u * b[2]) + v * c[2]};
    if (out.normals) reinterpret_cast<MsRow3*>(out.normals)[k] = MsRow3{n[0] / L, n[1] / L, n[2] / L};
    if (out.triangle) out.triangle[k] = t;
    if (out.bary) reinterpret_cast<MsRow2*>(out.bary)[k] = MsRow2{u, v};
    if (out.attr) {
        const size_t ia = (size_t)tri[3 * (size_t)t] * width, ib = (size_t)tri[3 * (size_t)t + 1] * width, ic = (size_t)tri[3 * (size_t)t + 2] * width;
        float* __restrict__ o = out.attr + (size_t)k * width;
        for (int col = 0; col < width; ++col) o[col] = (w * attr[ia + col] + u * attr[ib + col]) + v * attr[ic + col];
    }
}

// One lane per sample, MS_PER samples per lane.  The workgroup first stages the coarse levels of the search in LDS: s[i] = the last entry of
// segment i of C, segments of `stride` entries (a power of two, the smallest with at most MS_LDS_N whole segments: 1 up to 4,096
// triangles, where s is all of C).  A lane counts the segments that lie wholly at or below its target in LDS, then searches the stride
// entries of the next one in global memory.  ctop: the largest power of two <= the number of whole segments.
__global__ __launch_bounds__(MS_LDS_T)
void k_ms_sample(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int nt, int stride, int ctop,
                 const unsigned long long* __restrict__ C, const float* __restrict__ attr, int width, unsigned seed,
                 unsigned long long first, int n_samples, const MsRec* __restrict__ rec, MsOut out) {
    __shared__ unsigned long long s[MS_LDS_N];
    const unsigned long long W = rec->total_weight;
    if (W == 0ull) return;
    const int nc = nt / stride;                                                        // whole segments, 1 <= nc <= MS_LDS_N
    for (int i = threadIdx.x; i < nc; i += MS_LDS_T) s[i] = C[(size_t)(i + 1) * stride - 1];
    __syncthreads();
    for (int r = 0; r < MS_PER; ++r) {
        const int k = (blockIdx.x * MS_PER + r) * MS_LDS_T + (int)threadIdx.x;
        if (k >= n_samples) return;
        uint32_t x[4];
        const unsigned long long target = ms_draw(first + (unsigned long long)k, seed, W, x);
        // the smallest t with C_t > target = the number of C_t <= target.  q segments lie wholly at or below the target, so the answer is
        // in [q stride, (q + 1) stride): the last entry of segment q is above the target - or segment q is the short tail, whose last
        // entry is C[nt - 1] = W > target.  Either way t < nt; the min never binds and is stated for the reader of the fetches.
        const int t0 = ms_upper_bound(s, 0, nc, ctop, target) * stride;
        const int t = min(stride > 1 ? ms_upper_bound(C, t0, min(t0 + stride, nt), stride >> 1, target) : t0, nt - 1);
        ms_emit(vtx, nv, tri, t, x, attr, width, k, out);
    }
}

#ifdef TDV_STUDY
// The A/B that lost ("Mesh sampling"): every step of the search in global memory, 256 lanes, one sample per lane.
// top: the largest power of two <= nt
__global__ __launch_bounds__(MS_T)
void k_ms_sample_global(const float* __restrict__ vtx, int nv, const int* __restrict__ tri, int nt, int top, const unsigned long long* __restrict__ C,
                        const float* __restrict__ attr, int width, unsigned seed, unsigned long long first, int n_samples,
                        const MsRec* __restrict__ rec, MsOut out) {
    const unsigned long long W = rec->total_weight;
    const int k = blockIdx.x * MS_T + (int)threadIdx.x;
    if (W == 0ull || k >= n_samples) return;
    uint32_t x[4];
    const unsigned long long target = ms_draw(first + (unsigned long long)k, seed, W, x);
    ms_emit(vtx, nv, tri, min(ms_upper_bound(C, 0, nt, top, target), nt - 1), x, attr, width, k, out);
}
#endif

// every argument, before anything is enqueued (include/tdv_hip.h)
bool ms_args_ok(const tdv_ctx* ctx, const float* vtx, int nv, const int* tri, int nt, const float* attr, int attr_width, int n_samples,
                const tdv_mesh_sample_params* p, const tdv_mesh_sample_result* result, const float* out_attr) {
    if (!ctx || !p || !result) return false;
    if (nv < 0 || nv > TDV_MESH_MAX_VERTICES || nt < 0 || nt > TDV_MESH_MAX_TRIANGLES || (nv > 0 && !vtx) || (nt > 0 && !tri)) return false;
    if (n_samples < 0 || n_samples > TDV_MESH_SAMPLE_MAX || p->first_sample + (uint64_t)n_samples < p->first_sample) return false;
    return attr_width >= 0 && !(attr_width > 0 && !attr) && !(out_attr && !attr);
}

// The whole call on device memory.  h (host entry point): where the device outputs go.
int ms_run_dev(tdv_ctx* ctx, const float* d_vtx, int nv, const int* d_tri, int nt, const float* d_attr, int attr_width, int n_samples,
               const tdv_mesh_sample_params& prm, tdv_mesh_sample_result* result, MsOut d, const MsOut* h) {
    std::memset(result, 0, sizeof(*result));
    if (nt == 0) return TDV_OK;
    hipStream_t s = ctx->stream;
    if (!d_attr || attr_width == 0) d.attr = nullptr;
    const int nb = (nt + MS_T - 1) / MS_T;
    unsigned* area; MsSum* sums; unsigned long long* C = nullptr; MsRec* rec;
    TDV_TRY(ws_alloc(ctx, (size_t)nt, &area));
    TDV_TRY(ws_alloc(ctx, (size_t)nb, &sums));
    if (n_samples > 0) TDV_TRY(ws_alloc(ctx, (size_t)nt, &C));
    TDV_TRY(ws_alloc(ctx, 1, &rec));
    TDV_TRY(pin_reserve(ctx, sizeof(MsRec)));
    TDV_HIP(ctx, hipMemsetAsync(rec, 0, sizeof(MsRec), s));
    k_ms_area<<<nb, MS_T, 0, s>>>(d_vtx, nv, d_tri, nt, area, rec);
    k_ms_sums<<<nb, MS_T, 0, s>>>(area, nt, rec, sums);
    k_ms_scan_sums<<<1, MS_SCAN_T, 0, s>>>(sums, nb, n_samples, rec);
    if (n_samples > 0) {
        k_ms_prefix<<<nb, MS_T, 0, s>>>(area, nt, rec, sums, C);
#ifdef TDV_STUDY
        if (study_env("TDV_MESH_SAMPLE_GLOBAL")) {
            int top = 1;
            while (top <= nt / 2) top <<= 1;
            k_ms_sample_global<<<(n_samples + MS_T - 1) / MS_T, MS_T, 0, s>>>(d_vtx, nv, d_tri, nt, top, C, d_attr, attr_width, prm.seed,
                                                                              prm.first_sample, n_samples, rec, d);
        } else
#endif
        {
            int stride = 1, ctop = 1;
            while (nt / stride > MS_LDS_N) stride <<= 1;
            while (ctop <= nt / stride / 2) ctop <<= 1;
            const int per = MS_LDS_T * MS_PER;
            k_ms_sample<<<(n_samples + per - 1) / per, MS_LDS_T, 0, s>>>(d_vtx, nv, d_tri, nt, stride, ctop, C, d_attr, attr_width, prm.seed,
                                                                        prm.first_sample, n_samples, rec, d);
        }
    }
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(fetch_state(ctx, rec, result));
    // host entry point: the sampled rows, n_sampled of them
    if (!h) return TDV_OK;
    return download_rows(ctx, (size_t)result->n_sampled, {{h->xyz, d.xyz, 3 * sizeof(float)}, {h->normals, d.normals, 3 * sizeof(float)},
                                                         {h->triangle, d.triangle, sizeof(int)}, {h->bary, d.bary, 2 * sizeof(float)},
                                                         {h->attr, d.attr, (size_t)attr_width * sizeof(float)}});
}

}  // namespace

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_mesh_sample_default_params(tdv_mesh_sample_params* p) {
    if (!p) return;
    p->seed = 0u; p->first_sample = 0ull;
}

int tdv_mesh_sample_points_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles, const float* d_attr,
                               int attr_width, int n_samples, const tdv_mesh_sample_params* params, tdv_mesh_sample_result* result,
                               float* d_out_xyz, float* d_out_normals, int* d_out_triangle, float* d_out_bary, float* d_out_attr) {
    if (!ms_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, d_attr, attr_width, n_samples, params, result, d_out_attr))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    MsOut d; d.xyz = d_out_xyz; d.normals = d_out_normals; d.triangle = d_out_triangle; d.bary = d_out_bary; d.attr = d_out_attr;
    return ms_run_dev(ctx, d_vertices, n_vertices, d_triangles, n_triangles, d_attr, attr_width, n_samples, *params, result, d, nullptr);
}

int tdv_mesh_sample_points(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* attr,
                           int attr_width, int n_samples, const tdv_mesh_sample_params* params, tdv_mesh_sample_result* result, float* out_xyz,
                           float* out_normals, int* out_triangle, float* out_bary, float* out_attr) {
    if (!ms_args_ok(ctx, vertices, n_vertices, triangles, n_triangles, attr, attr_width, n_samples, params, result, out_attr))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    float *d_vtx, *d_attr = nullptr; int* d_tri;
    MsOut h, d; h.xyz = out_xyz; h.normals = out_normals; h.triangle = out_triangle; h.bary = out_bary; h.attr = out_attr;
    TDV_TRY(upload(ctx, vertices, (size_t)n_vertices * 3, &d_vtx));
    TDV_TRY(upload(ctx, triangles, (size_t)n_triangles * 3, &d_tri));
    if (n_triangles > 0 && n_samples > 0) {
        const size_t m = (size_t)n_samples;
        if (out_attr) {                                      // the rows are only ever interpolated into out_attr
            TDV_TRY(upload(ctx, attr, (size_t)n_vertices * (size_t)attr_width, &d_attr));
            if (d_attr) TDV_TRY(ws_alloc(ctx, m * (size_t)attr_width, &d.attr));
        }
        if (out_xyz) TDV_TRY(ws_alloc(ctx, m * 3, &d.xyz));
        if (out_normals) TDV_TRY(ws_alloc(ctx, m * 3, &d.normals));
        if (out_triangle) TDV_TRY(ws_alloc(ctx, m, &d.triangle));
        if (out_bary) TDV_TRY(ws_alloc(ctx, m * 2, &d.bary));
    }
    return ms_run_dev(ctx, d_vtx, n_vertices, d_tri, n_triangles, d_attr, attr_width, n_samples, *params, result, d, &h);
}

}  // extern "C"
