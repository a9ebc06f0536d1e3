// Internal definitions of the MI355X registration backend (not part of the C ABI).
// One tdv_ctx = one HIP stream + a grow-only device workspace + pinned staging + optional
// per-kernel HIP-event timers.  Steady state performs no hipMalloc.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tdv_hip.h"
#include "depth_frames.hpp"

namespace tdv {

struct TimerSlot {
    double total_ms = 0.0;
    int launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace tdv

struct tdv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // device workspace: a list of blocks; coalesced into one block at the next reset when it grew
    struct Block { char* p; size_t cap; };
    std::vector<Block> blocks;
    size_t cur_block = 0, cur_off = 0, high_water = 0, used_total = 0;
    // pinned host staging
    char* pin = nullptr;
    size_t pin_cap = 0;
    char err[512] = {0};
    bool timing = false;
    int icp_search = 0;      // TDV_ICP_SEARCH_AUTO / _BRUTE / _PRUNED / _GRID (tdv_ctx_set_icp_search)
    int icp_accumulate = 0;  // TDV_ICP_ACCUMULATE_TREE (f64 fixed tree) / _REFERENCE (f32, ascending source index: the CPU path's sums bit for bit)
    int icp_loss = 0;        // TDV_ICP_LOSS_L2 / _HUBER / _TUKEY / _CAUCHY (tdv_ctx_set_icp_loss)
    float icp_loss_scale = 0.f;   // its scale k (0 with L2)
    int ransac_leaf_order = 0;    // TDV_RANSAC_LEAVES_AUTO (class-major from kRansacLeafClassesMin pairs on) / _MORTON / _CLASSES (tdv_ctx_set_ransac_leaf_order)
    int ransac_triples = 0;       // TDV_RANSAC_TRIPLES_AUTO (staged wherever a call can: ransac.hip, RansacStage) / _DIRECT / _STAGED (tdv_ctx_set_ransac_triples)
    int last_ransac_staged = 0;   // batches of the last RANSAC call that ran from staged triples (tdv_ctx_last_ransac_staged)
    int ransac_score_mode = 0;   // TDV_RANSAC_SCORE_FAST (FMA pass + exact band) / _EXACT (the reference arithmetic only) / _MATRIX (tdv_ctx_set_ransac_score)
    double last_ransac_rescore = -1.0;   // fraction of (wave, 8-point chunk) pairs of the last RANSAC call that the fast pass scored again exactly (-1: exact mode)
    long long last_ransac_bound[4] = {0, 0, 0, 0};   // the leaf-box bound's lists in the last RANSAC call: hypotheses bounded, close, on the fine list, live
    double last_ransac_scored = 1.0;     // share of the (hypothesis, point) tests the last RANSAC call evaluated (< 1: the exact bail-out left the rest out)
    int last_voxel_grouping = 0;   // 1: the table (k_vh_insert), 2: pixel windows (k_vs_group) - the last batched voxel call (tdv_ctx_last_voxel_grouping)
    int last_voxel_batch_redone = -1;   // whether the caller of the last batched voxel pass (voxel_downsample_batch_dev) redid it cloud by cloud: 0 kept, 1 redone (tdv_ctx_last_voxel_batch_redone)
    int last_fm_path = 0;      // TDV_FM_PATH_* of the last descriptor match on this ctx (tdv_ctx_last_feature_match_path)
    int last_batch_lanes = 0;  // host lanes the last tdv_register_batch_dev call on this ctx spread its instances over (tdv_ctx_last_batch_lanes)
    int fps_path = 0;          // TDV_FPS_AUTO / _WORKGROUP / _GRID (tdv_ctx_set_fps_path)
    int last_fps_path = 0;     // the family the last farthest-point call on this ctx chose (tdv_ctx_last_fps_path)
    int icp_launches = 0;      // TDV_ICP_LAUNCHES_AUTO / _TWO / _ONE (tdv_ctx_set_icp_launches)
    int last_icp_launches = 0; // whether the last ICP call on this ctx ran the one-launch iteration (tdv_ctx_last_icp_launches)
    int icp_probe_cache = 0;   // TDV_ICP_PROBE_CACHE_AUTO / _OFF / _ON (tdv_ctx_set_icp_probe_cache)
    int last_icp_probe_misses = -1;   // lanes that probed the hash table in the last ICP call, -1 if it ran without the probe cache
    int last_icp_search = 0;// the search the last ICP / correspondence call on this ctx actually ran (tdv_ctx_last_icp_search)
    unsigned* scan_ticket = nullptr;  // persistent device words: [0] exclusive_scan_dev's last-workgroup ticket, [1..] ICP's, [8] the tile ticket of depth_cloud.hip's chained scan
    unsigned long long* chain_status = nullptr;   // depth_cloud.hip k_depth_cloud_chain: one status word per tile, persistent (told apart by chain_epoch)
    size_t chain_cap = 0;
    unsigned chain_epoch = 0, chain_ticket_base = 0;   // calls so far; tickets handed out so far (the kernel's tile = ticket - base)
    tdv_ctx* helper = nullptr;   // second stream + workspace of the batched pipeline's other lane (owned; created on first use)
    tdv::TimerSlot timers[TDV_TIMER_COUNT];
    std::vector<hipEvent_t> event_pool;
    int ransac_seq = 0;          // the sequence number of the last RANSAC batch enqueued on this ctx (ransac.hip: the record's word [4]); never 0
    int wall_clock_khz = 0;      // hipDeviceAttributeWallClockRate, read on first use (ransac.hip: the score timer's stamps)
};

namespace tdv {

inline int set_err(tdv_ctx* ctx, hipError_t e, const char* what, int line) {
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s failed at line %d: %s", what, line, hipGetErrorString(e));
    if (e == hipErrorOutOfMemory) return TDV_ERR_OOM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return TDV_ERR_NO_DEVICE;
    return TDV_ERR_LAUNCH;
}

#define TDV_HIP(ctx, call)                                              \
    do {                                                                \
        hipError_t e__ = (call);                                        \
        if (e__ != hipSuccess) return tdv::set_err((ctx), e__, #call, __LINE__); \
    } while (0)

#define TDV_TRY(expr)                    \
    do {                                 \
        int s__ = (expr);                \
        if (s__ != TDV_OK) return s__;   \
    } while (0)

#define TDV_CHECK_LAUNCH(ctx) TDV_HIP((ctx), hipGetLastError())

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// float -> int as x86's cvttss2si converts (include/tdv_hip.h, tdv_voxel_downsample): truncation inside int range, INT_MIN for NaN
// and for everything outside it.  The reference's static_cast<int>(std::floor(x * inv)) is undefined in C++ there and compiles to
// cvttss2si on x86; the device's own conversion (v_cvt_i32_f32) gives 0 for NaN and saturates.  Every voxel key goes through this.
__host__ __device__ __forceinline__ int cvt_i32_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }
// ... and double -> int as cvttsd2si converts (the FPFH theta bin is formed in double: include/tdv_hip.h, tdv_compute_fpfh).
__host__ __device__ __forceinline__ int cvt_i32_x86_f64(double f) { return (f > -2147483649.0 && f < 2147483648.0) ? (int)f : INT_MIN; }

// Study build (-DTDV_STUDY -> lib3dvision_hip_study.so, used by tools/studies/ and by the tests marked `study`): keeps the A/B
// variants that LOST their measurement (the matrix-core scoring pass, the merged scoring dispatch, round 1's key-ordered descriptor
// scan, one-point-per-wave SPFH / FPFH, the full bitonic voxel sort, ...) and the tuning knobs, all behind study_env().  In the
// product library study_env() is the constant nullptr: every branch behind it is dead code the compiler drops, and the kernels
// only those branches launch are not compiled at all (#ifdef TDV_STUDY).  What stays a real getenv() is what a deployer or a
// parity test of a LIVE path needs.
#ifdef TDV_STUDY
inline const char* study_env(const char* name) { return getenv(name); }
constexpr bool kStudyBuild = true;
#else
constexpr const char* study_env(const char*) { return nullptr; }
constexpr bool kStudyBuild = false;
#endif

#ifdef __HIPCC__
// ascending order of the 16-byte records that sort.hip sorts: (x, y, z, w) as unsigned words
__device__ __forceinline__ bool rec_less(const uint4& a, const uint4& b) {
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.z != b.z) return a.z < b.z;
    return a.w < b.w;
}
// Sum over the 64 lanes of a wave with DPP row operations (no LDS crossbar traffic, unlike __shfl_down): the result is
// valid in lane 63 and returned wave-uniform.
__device__ __forceinline__ int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);   // row_mirror: every lane of a 16-lane row holds the row sum
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}
#endif

// Workspace: reset at the start of every public entry point.
int ws_reset(tdv_ctx* ctx);
int ws_alloc_bytes(tdv_ctx* ctx, size_t bytes, void** out);
template <class T>
inline int ws_alloc(tdv_ctx* ctx, size_t count, T** out) {
    void* p = nullptr;
    int s = ws_alloc_bytes(ctx, count * sizeof(T), &p);
    *out = static_cast<T*>(p);
    return s;
}
int pin_reserve(tdv_ctx* ctx, size_t bytes);
// mark / rewind: a batched caller frees everything one instance allocated while keeping what came before
struct WsMark { size_t block, off, used; };
inline WsMark ws_mark(tdv_ctx* ctx) { return WsMark{ctx->cur_block, ctx->cur_off, ctx->used_total}; }
inline void ws_rewind(tdv_ctx* ctx, const WsMark& m) { ctx->cur_block = m.block; ctx->cur_off = m.off; ctx->used_total = m.used; }

// Events for stream synchronisation points come from (and go back to) the ctx's pool: no hipEventCreate in steady state.
hipEvent_t event_acquire(tdv_ctx* ctx);
void event_release(tdv_ctx* ctx, hipEvent_t e);

// Timing helpers: bracket a launch with events when ctx->timing is on.
struct ScopedTimer {
    tdv_ctx* ctx; int slot; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(tdv_ctx* c, int s);
    ~ScopedTimer();
};

// ------------------------------------------------------------------ device pipelines
struct IcpOutputs {  // optional per-source outputs of one correspondence pass (device pointers)
    int* corr = nullptr; float* d2 = nullptr; uint8_t* accepted = nullptr;
};
// What an ICP call minimises: the kind (its value is the kernels' MODE, icp.hip; point-to-plane without target normals runs as
// point-to-point: icp_dispatch) and what the kind needs beyond the clouds and the
// target's normals.  GICP (plane-to-plane, include/tdv_hip.h: tdv_gicp): the source normals and c = 1 - epsilon in f32.  Colored ICP
// (Park et al. 2017, tdv_colored_icp): the source colours, the target's colour table (float4 (I, d) per point, tdv_color_gradients),
// lg = sqrtf(lambda) and lc = sqrtf(1 - lambda).  Source normals and colours are laid out like the source points.
enum IcpKind { ICP_POINT_TO_PLANE = 0, ICP_POINT_TO_POINT = 1, ICP_GICP = 3, ICP_COLORED = 4 };
struct IcpObjective {
    IcpKind kind;
    const float* src_normals; float c;                            // GICP
    const float *src_rgb, *tgt_color; float lg, lc;               // colored ICP
    float param;                                                  // epsilon resp. lambda as the caller gave it (icp_objective_check)
    // when the loop stops (icp.hip: icp_update): |fitness change| < rel_fitness and |rmse change| < rel_rmse.  The defaults are the
    // reference's rule (registration.cpp:406) and what every entry point but the multi-scale ones passes.
    float rel_fitness = INFINITY, rel_rmse = 1e-6f;
    IcpObjective criteria(float fitness, float rmse) const { IcpObjective o = *this; o.rel_fitness = fitness; o.rel_rmse = rmse; return o; }
    static IcpObjective plain(int point_to_plane) { return {point_to_plane ? ICP_POINT_TO_PLANE : ICP_POINT_TO_POINT, nullptr, 0.f, nullptr, nullptr, 0.f, 0.f, 0.f}; }
    static IcpObjective gicp(const float* src_normals, float epsilon) { return {ICP_GICP, src_normals, 1.f - epsilon, nullptr, nullptr, 0.f, 0.f, epsilon}; }
    static IcpObjective colored(const float* src_rgb, const float* tgt_color, float lambda) {
        return {ICP_COLORED, nullptr, 0.f, src_rgb, tgt_color, sqrtf(lambda), sqrtf(1.f - lambda), lambda};
    }
    // the objective of an instance whose source points start at point `start` of the arrays
    IcpObjective at(int start) const {
        IcpObjective o = *this;
        if (o.src_normals) o.src_normals += (size_t)start * 3;
        if (o.src_rgb) o.src_rgb += (size_t)start * 3;
        return o;
    }
};
struct SortedCloud;
// Hash grid over a target cloud for ICP's correspondence search at one acceptance threshold (icp.hip): cells of 2.2 x
// the threshold, open-addressing table of (32-bit cell tag, list head), the points of a cell as a linked list of (x, y, z, next) nodes indexed like the cloud.  Lives
// in the workspace of the ctx that built it; read-only afterwards.  usable = 0: coordinates too large for the cell
// arithmetic or too many points per cell (the threshold is large against the spacing) - the caller takes another search.
struct CellGrid { const void* table; const void* node; unsigned mask; int shift; float inv_cell; float thr; int n; int usable; };
int cell_grid_build(tdv_ctx* ctx, const float* d_tgt, int nt, float thr, CellGrid* g);
// tgt_sorted / tgt_grid (optional): the target in Morton order with its boxes (spatial_sort_cloud) resp. its hash grid
// (cell_grid_build, for this thr), built once and reused across calls
int icp_run_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                const float* T0, float thr, int max_iterations, IcpObjective obj, int fixed_iterations,
                tdv_icp_result* out, const SortedCloud* tgt_sorted = nullptr, const CellGrid* tgt_grid = nullptr);
// many small problems against one target in one launch (icp.hip: k_icp_small), when icp_small_batch_fits(ctx, largest problem, nt)
bool icp_small_batch_fits(const tdv_ctx* ctx, int ns_max, int nt);
int icp_small_batch_dev(tdv_ctx* ctx, const float* d_src, const int* d_src_off, int n_prob, const float* d_tgt, const float* d_tgt_normals, int nt,
                        const float* T0s, float thr, int max_iterations, IcpObjective obj, tdv_icp_result* out);
// icp_run_dev for n instances against one target (icp.hip): instance b = h_count[b] points from point h_start[b] of d_src (host arrays), start
// pose T0s + 16 b, obj's source arrays laid out like d_src; per instance icp_run_dev's result bit for bit.  Arguments are not checked.
int icp_batch_run_dev(tdv_ctx* ctx, const float* d_src, const int* h_start, const int* h_count, int n, const float* d_tgt, const float* d_tgt_normals,
                      int nt, const float* T0s, float thr, int max_iterations, IcpObjective obj, int fixed_iterations, tdv_icp_result* out);
int icp_correspondences_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt,
                            const float* T, float thr, IcpOutputs outs, int* n_corr);
// TDV_ERR_BAD_ARG (reason in ctx->err) when the ctx's ICP loss cannot run with its accumulation mode (a robust loss with
// reference-order sums); the ICP entry points ask before they enqueue or write anything
int icp_loss_check(tdv_ctx* ctx);
// what an entry point asks of its objective before it enqueues or writes anything: TDV_ERR_BAD_ARG (reason in ctx->err where there is
// more to say than "bad argument").  Point-to-plane and point-to-point: icp_loss_check.  GICP: a NULL normal array, epsilon not finite or
// outside (0, 1], or a ctx in reference-order accumulation (the reference has no GICP).  Colored ICP: a NULL colour, colour table or
// normal array, lambda not finite or outside [0, 1], or reference-order accumulation; device: the colour table is a device pointer,
// which the kernels read as float4 - it must be 16-byte aligned.
int icp_objective_check(tdv_ctx* ctx, const IcpObjective& obj, const float* tgt_normals, bool device);
int ransac_run_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt,
                   const float* d_fs, const float* d_ft, const int* d_corr,
                   float voxel, int max_iterations, float confidence, uint32_t seed,
                   tdv_ransac_result* out, int* trace_inliers);
// the winner scoring of ransac_run_dev for one pose (ransac.hip): d_hyp12 = column-major R then t (device, f32); d_out2 (device) receives
// the f64 tree sum of (double)(err * err) over the inliers (sqrtf(d2) < 1.5 voxel) of the matches d_corr and the inlier count
int ransac_score_pose_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const int* d_corr, const float* d_hyp12,
                          float voxel, double* d_out2);
// ransac_run_dev for many small clouds against one target in a handful of launches (ransac.hip): cloud b = points
// [h_off[b], h_off[b+1]) of d_src with correspondences d_corr (same indexing); out[b].rmse is NOT evaluated (0).  *fell_back = 1:
// nothing was computed (a cloud too large, too many hypotheses, or the index sampler ran out of draws) - use ransac_run_dev.
int ransac_small_batch_dev(tdv_ctx* ctx, const float* d_src, const int* h_off, const int* d_off, int n_clouds, const float* d_tgt, int nt, const int* d_corr,
                           float voxel, int max_iterations, float confidence, uint32_t seed, tdv_ransac_result* out, int* fell_back);
// The descriptor match (fmatch.hip).  Which calls use the packed index, said once: a target set is indexed when fm_wants_index(nt)
// (at least 2,048 targets, and neither TDV_FM_BRUTE nor the study build's TDV_FM_KEYORDER asks for another search; read per call),
// and a call searches the index when it brings fm_indexes_sources(ns) (at least 4,096 sources); every other call is the plain scan.
bool fm_wants_index(int nt);
bool fm_indexes_sources(int ns);
int feature_match_dev(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr);
// Packed index of a target descriptor set (fmatch_index.hip; every array's layout: fmatch_layout.hpp): rows in sort-tile-recursive
// order along the set's principal directions, padded per column, with boxes of the 64-row leaves and the 64-leaf groups.  Lives in
// the workspace of the ctx that built it (valid until that ctx's next ws_reset / rewind below the build); read-only afterwards, so a
// batch builds it once for the model and every instance (on either lane) queries it.
struct FmIndex {
    const float* ft = nullptr;                                      // the caller's rows, [nt][33] (must outlive the index: the fallback scan reads them)
    float* T = nullptr; int* torig = nullptr;                       // the packed rows and their original indices
    float *lbox = nullptr, *gbox = nullptr;                         // 33-D boxes of the leaves and of the groups
    float *pbox = nullptr, *gpbox = nullptr;                        // ... and their boxes in the 3 principal coordinates
    float *sleaf = nullptr, *sgroup = nullptr;                      // the same boxes as the leaf-major search stages them
    unsigned* amax = nullptr; float pscale = 0.f;                   // largest |x_d - mean_d| of the targets (float bits); pscale 0 disables the 3-D boxes
    float *basis = nullptr, *b0 = nullptr, *b1 = nullptr, *leaf_p2 = nullptr; const int* col_leaf0 = nullptr;   // locating a source's cell
    int nt = 0, rows = 0, nleaf = 0, ngroup = 0, S0 = 1, S1 = 1;
};
int fm_index_build(tdv_ctx* ctx, const float* d_ft, int nt, FmIndex* out);
int feature_match_indexed_dev(tdv_ctx* ctx, const float* d_fs, int ns, const FmIndex& ix, int* d_corr);
int estimate_normals_dev(tdv_ctx* ctx, const float* d_xyz, int n, int k, float* d_normals, int* d_knn);
// colour gradients of a cloud (color.hip, include/tdv_hip.h: tdv_color_gradients): float4 (I, d) per point from the kNN lists d_knn
// (int[n * k], tdv_estimate_normals' for the same k) or, d_knn == nullptr, from estimate_normals_dev's search
int color_gradients_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, const float* d_normals, int n, int k, const int* d_knn,
                        float* d_color);
int compute_fpfh_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_normals, int n, float radius,
                     float* d_desc, int* d_nbr, int* d_nbr_cnt);
// With TDV_VOXEL_ORDER_REFERENCE, `both` (optional) also receives the cloud in first-occurrence order and the permutation
// between the two orders: out_xyz[p] == first_xyz[ref2first[p]], first2ref[ref2first[p]] == p (each of capacity entries).
struct VoxelBothOrders { float* first_xyz; int* ref2first; int* first2ref; };
// The second 3-wide companion of a cloud, its normals (include/tdv_hip.h: tdv_voxel_downsample_normals): the input rows and where a
// voxel's unit mean goes, each laid out like the points' array beside it.  Both pointers or neither; they ride the points' one
// grouping pass, as the colours do.
struct VoxelNormals { const float* in = nullptr; float* out = nullptr; };
int voxel_downsample_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, float voxel, int order,
                         float* d_out_xyz, float* d_out_rgb, int capacity, int* n_out, const VoxelBothOrders* both = nullptr,
                         VoxelNormals nrm = VoxelNormals{});

// The voxels of one or several clouds in first-occurrence order, and what the reference order needs of them (voxel.hip: what a rung
// of the grouping ladder leaves behind).  By value, like SortedCloud and DepthFrames.
struct VoxelFirst {
    float* xyz = nullptr; float* rgb = nullptr; float* nrm = nullptr;   // rows; rgb / nrm null for a cloud without that companion
    int capacity = 0;                                                   // rows that fit (a batch: its points)
    int* rank = nullptr;       // optional, per input point: the first-occurrence rank of a voxel's first point, counted through all clouds
    int4* leaders = nullptr;   // optional, per voxel: the cell and the index (within its cloud) of its first point
    int* d_voff = nullptr;     // optional, n_clouds + 2 device ints: the voxel offsets, then the rung's flag
};
// Every knob of the voxel stage, read in one place at the top of a call (voxel.hip: voxel_knobs).  LIVE knobs are real getenv()s, read
// per call because the tests switch them inside a process; STUDY knobs go through study_env() and are dead code in the product library.
struct VoxelKnobs {
    bool pixels;         // live   TDV_VOXEL_PIXELS=0: clouds with intrinsics go to the table at once (parity tests)
    int device_order;    // live   TDV_VOXEL_DEVICE_ORDER=0 / 1: the reference order by the host replay / the device periods; -1 (unset): by voxel count
    bool batch;          // live   TDV_BATCH_VOXEL=0: a registration batch groups instance by instance
    bool counting_sort;  // study  TDV_VOXEL_LEGACY: start the ladder at the counting sort
    bool full_sort;      // study  TDV_VOXEL_SORT: start it at the full bitonic sort
    bool real_map;       // study  TDV_VOXEL_REAL_MAP: a real std::unordered_map instead of the emulation
    int split_from;      // study  TDV_VOXEL_SPLIT_FROM: tiles from which k_vh_finalize runs as count + scan + emit (224)
};
VoxelKnobs voxel_knobs();
// Clouds stored back to back - cloud b = points [h_off[b], h_off[b + 1]) of d_xyz, d_off the same offsets on the device - all at once
// (voxel.hip: pixel windows when pinhole4 = fx, fy, cx, cy says they were unprojected with these intrinsics in row-major pixel order,
// else the table): cloud b's voxels at [h_voff[b], h_voff[b + 1]) of out.xyz (room for every point), in first-occurrence order;
// out.rank / leaders / d_voff for a caller that goes on to the reference order.  d_normals (optional, not with pinhole4): the clouds'
// normals, their voxels' unit means to out.nrm.  A voxel too full for the table: the clouds are redone one by one with
// voxel_downsample_dev and packed back to back the same way - here, or (overflowed not null: it is told, and nothing of `out` is
// valid) by a caller with lanes of its own.  batched = false: one by one at once (one cloud on its own; not recorded as a redone batch).
int voxel_downsample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_off, const int* d_off, int n_clouds, float voxel, const float* pinhole4,
                               const VoxelFirst& out, int* h_voff, const float* d_normals = nullptr, int* overflowed = nullptr, bool batched = true);
// voxel_order.hip.  The reference's container order of every cloud of a batch, computed on the device; h_failed[b] != 0: finish cloud b with voxel_reference_order
int voxel_reference_order_batch_dev(tdv_ctx* ctx, int n_clouds, const int* h_voff, const int* d_voff, const int4* d_leaders, const float* d_first_xyz,
                                    float* d_out_xyz, int* d_ref2first, int* d_first2ref, int* h_failed);
int voxel_reference_order(tdv_ctx* ctx, int v, int n, const int4* d_leaders, const float* tmp_xyz, const float* tmp_rgb, const int* d_rank, int rank_base,
                          float* d_out_xyz, float* d_out_rgb, const VoxelBothOrders* both, VoxelNormals nrm = VoxelNormals{});
int voxel_finish_reference(tdv_ctx* ctx, int n, int v, const VoxelFirst& first, float* d_out_xyz, float* d_out_rgb, float* d_out_nrm,
                           const VoxelBothOrders* both, const VoxelKnobs& knobs);

int sort_records_dev(tdv_ctx* ctx, uint4* rec, size_t n_pow2);  // sort.hip: ascending bitonic sort, n_pow2 >= 2048
// sort.hip: stable LSD radix sort (hand-written) of (key, value) pairs on the low end_bit bits of the 64-bit key; any n; scratch from the workspace
int radix_sort_pairs_dev(tdv_ctx* ctx, const unsigned long long* d_keys_in, unsigned long long* d_keys_out,
                         const unsigned* d_vals_in, unsigned* d_vals_out, size_t n, int end_bit);
// sort.hip: every segment [d_seg_start[c], d_seg_start[c + 1]) sorted on its own in one launch; segments of at most segment_sort_max_len() records
int segment_sort_records_dev(tdv_ctx* ctx, uint4* rec, const int* d_seg_start, int nseg);
int segment_sort_max_len();
size_t sort_pow2(size_t n);
int exclusive_scan_dev(tdv_ctx* ctx, const int* d_in, int n, int* d_out, int* d_total);  // sort.hip
// A cloud in search order with the bounding boxes of its 64-point leaves and of its 4096-point groups of 64 leaves (workspace memory):
// the one structure every neighbour search walks (sorted_cloud.hpp).  The kernels take it by value.  spatial_sort_cloud builds it in
// Morton order with positions n..pad filled with +inf; the batch of small clouds (knn.hip: normals_fpfh_batch_dev) lays its clouds out
// back to back, each padded to whole leaves with NaN, and names their leaf ranges in inst_leaf (there n == pad: every position is read).
struct SortedCloud {
    const float *sx, *sy, *sz;            // SoA coordinates of the `pad` positions (a multiple of 256)
    const int* orig;                      // original index of a position (INT_MAX at a padding position)
    const float *lbox, *tbox;             // leaf and group boxes, [6][n_leaf] and [6][n_top]: min x, y, z, then max x, y, z
    int n, n_leaf, n_top, pad;            // (the three a walk reads side by side: one scalar load)
    // optional: ties in (d2, id) order are broken by okey[position] instead of the original index, and the lists receive key2idx[id]
    const int *okey = nullptr, *key2idx = nullptr;
    // optional, several clouds in one array: cloud b owns leaves [inst_leaf[b], inst_leaf[b + 1]), and a query never leaves its cloud
    const int* inst_leaf = nullptr; int n_inst = 0;
};
int spatial_sort_cloud(tdv_ctx* ctx, const float* d_xyz, int n, SortedCloud& out);

// normals + FPFH in one go, sharing one spatial sort and one radius scan (batch path; identical results)
// d_tie_ids / d_tie_ids_inv (optional, both or neither): neighbour lists are ordered by (d2, d_tie_ids[index]) instead of
// (d2, index) — the results are those of the cloud permuted so that point i sits at position d_tie_ids[i]
int normals_fpfh_dev(tdv_ctx* ctx, const float* d_xyz, int n, int k, float radius, float* d_normals, float* d_desc,
                     const int* d_tie_ids = nullptr, const int* d_tie_ids_inv = nullptr);

// the same for many small clouds stored back to back, in one set of launches (knn.hip); tie ids / their inverse are GLOBAL here
int normals_fpfh_batch_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_voff, const int* d_voff, int n_clouds, int k, float radius,
                           float* d_normals, float* d_desc, const int* d_tie_ids = nullptr, const int* d_tie_ids_inv = nullptr);

// A RANSAC index triple in one 64-bit word, for clouds of at most 2^21 points: i0 in bits 0..20, i1 in 21..41, i2 in 42..62, bit 63 =
// valid (the three indices differ, registration.cpp:240).  A batch is uploaded in this form where the cloud allows it, as int4
// (i0, i1, i2, valid) above that; TriView gives the kernels either.
constexpr uint64_t kTriplePackMaxN = (uint64_t)1 << 21;
__host__ __device__ __forceinline__ uint64_t triple_pack(uint32_t a, uint32_t b, uint32_t c) {
    const uint64_t valid = !(a == b || b == c || a == c);
    return (uint64_t)a | ((uint64_t)b << 21) | ((uint64_t)c << 42) | (valid << 63);
}
struct TriView {
    const void* p; int packed;
    __host__ __device__ __forceinline__ bool valid(int h) const {
        return packed ? (static_cast<const uint64_t*>(p)[h] >> 63) != 0 : static_cast<const int4*>(p)[h].w != 0;
    }
    __host__ __device__ static __forceinline__ int4 unpack(uint64_t w) {
        return make_int4((int)(w & 0x1fffffu), (int)((w >> 21) & 0x1fffffu), (int)((w >> 42) & 0x1fffffu), (int)(w >> 63));
    }
    __host__ __device__ __forceinline__ int4 load(int h) const {
        if (!packed) return static_cast<const int4*>(p)[h];
        return unpack(static_cast<const uint64_t*>(p)[h]);
    }
};

// host helpers
void mt19937_raw(uint32_t seed, size_t count, uint32_t* out);
// the same index stream, drawn incrementally (one (i0, i1, i2) triple per call) so that it can be produced batch by
// batch while the GPU scores the previous batch
class TripleStream {
public:
    TripleStream(uint32_t seed, uint64_t n);
    ~TripleStream();
    void next(uint64_t* out3);
    // `count` triples at once, as int4 (i0, i1, i2, valid) with valid = the three indices differ (registration.cpp:240);
    // indices are below n <= 2^31 here (the batch loop's clouds)
    void next_batch(int count, int* out4);
    // the same triples as one 64-bit word each (triple_pack below): for n <= kTriplePackMaxN, half the bytes of a batch's upload
    void next_batch_packed(int count, uint64_t* out);
private:
    struct Impl; Impl* impl_; uint64_t n_;
    TripleStream(const TripleStream&) = delete;
};
// largest float f with sqrtf(f) <= thr  (accept  <=>  d2 <= f  <=>  !(sqrtf(d2) > thr))
float tau_le(float thr);
// smallest float f with sqrtf(f) >= thr (inlier <=>  d2 < f   <=>  sqrtf(d2) < thr)
float tau_lt(float thr);

}  // namespace tdv

#include "entry.hpp"   // the frame of a public call: call_begin, upload / download, fetch_state, download_rows
