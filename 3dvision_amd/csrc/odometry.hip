// Depth odometry on gfx950: include/tdv_hip.h (tdv_depth_odometry_dev) states every rule, O1 to O10.
//
// Two frames of one sensor need no search structure: the pixel grid gives a vertex its neighbours (a normal is one cross product, O3)
// and the projection gives a source pixel its partner (O5).  Every float below is evaluated as the header writes it; the sums go over
// the fixed f64 tree (fixed_tree.hpp) in pixel order, and the only atomics are integer counts and tickets, so nothing depends on the
// order the device works in.
//   k_od_depth0    O1: a lane per pixel, the raw u16 frame to f32 metres, 0 where invalid.  blockIdx.y = frame.
//   k_od_depth0_f32  O10: the same from an f32 depth image - the target of tdv_depth_odometry_to_depth_dev and of tracking.
//   k_od_down      O4: a lane per pixel of the coarser level, its block of four from the finer one.
//   k_od_normals   O2 + O3: a lane per pixel; the +1 column and +1 row neighbours come from two more coalesced loads of the depth rows.
//                  Counts the level's valid pixels (an integer atomic per workgroup).  MAPS: also the vertex map, the normal map and the
//                  flag compact_flagged (flag_gather.hpp) gathers the rows by - the maps call.
//   k_od_iterate   one launch per iteration, blockIdx.y = pair: O5 and O6 per source pixel (frame_pose.hpp's pose_apply and
//                  pinhole_project, icp_terms.hpp's corr_rec and rec_terms: the verifier's and point-to-plane ICP's own code), the
//                  workgroup's 29 sums by the tree, one row of partials per workgroup; the workgroup that takes the pair's last ticket (agent scope) folds the rows in the
//                  tree's order and applies icp_update in its tail.  The next launch reads the new pose: no host round trip.  A pair
//                  that is done leaves at once.  TERMS: the folded sums go out instead (tdv_depth_odometry_terms_dev).
//   k_od_level     between levels, a lane per pair: records what the level did and restarts the iteration state (O8).
// The workspace keeps, per frame and level, the depth (4 bytes per pixel) and the normal map (12): vertices are recomputed from the
// depth wherever they are needed, O2 gives the same bits.  Everything a kernel reads from the workspace is written by the call first:
// depths and normals by the kernels above (every pixel of every level), counts and tickets by a memset, states by an upload.
// On the host a pair is set up once (od_pair_setup) for the four pair entry points, the terms call and tracking; odometry_pair, its
// parameter check and its empty result are what tsdf_raycast.hip calls (tsdf_track.hpp), under the names they have here.
#pragma clang fp contract(off)
#include "tdv_internal.hpp"
#include "frame_pose.hpp"
#include "tsdf_volume.hpp"
#include "icp_terms.hpp"
#include "fixed_tree.hpp"
#include "flag_gather.hpp"
#include "tsdf_track.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace tdv {

namespace {

constexpr int OD_T = 256;                                  // lanes of a workgroup: O7's 256 pixels
constexpr int OD_NV = 29;                                  // point-to-plane's sums: 1, d2, 21 + 6
constexpr int OD_ROW = 32;                                 // doubles per row of partials
constexpr int OD_L = TDV_ODOM_MAX_LEVELS;
static_assert(sizeof(tdv_odometry_params) == 28 && sizeof(tdv_odometry_result) == 108, "include/tdv_hip.h: the structs' layout");
static_assert(OD_L == 4, "tdv_odometry_params.max_iterations, tdv_odometry_result.iterations");

// one level of every frame of a call: frame f's depth at z + f * npx, its normal map at nrm + 3 * f * npx, its valid count at
// nvalid[f * OD_L + level]
struct OdLevel { int w, h, npx, level; Pinhole k; float* z; float* nrm; int* nvalid; };
// a pair's state on the device: ICP's record, and what the levels so far have left for the result
struct OdState { IcpState s; float fitness, rmse; int n_corr; int iterations[OD_L]; int n_corr_level[OD_L]; };
struct OdTerms { double sums[OD_NV]; int n_valid; int pad; };

__global__ __launch_bounds__(OD_T)
void k_od_depth0(const uint16_t* __restrict__ raw, int npx, float inv_scale, float zmax, float* __restrict__ z) {
    const int i = blockIdx.x * OD_T + threadIdx.x;
    if (i >= npx) return;
    const size_t o = (size_t)blockIdx.y * npx + i;
    const uint16_t r = raw[o];
    const float d = scaled_depth(r, inv_scale);                                    // O1
    z[o] = (r != 0 && d <= zmax) ? d : 0.0f;
}

// O10: level 0 of one frame from an f32 depth image (a ray cast of the volume, a rendering), 0 where it holds no usable depth
__global__ __launch_bounds__(OD_T)
void k_od_depth0_f32(const float* __restrict__ depth, int npx, float zmax, float* __restrict__ z) {
    const int i = blockIdx.x * OD_T + threadIdx.x;
    if (i >= npx) return;
    const float d = depth[i];
    z[i] = (d > 0.f && d <= zmax) ? d : 0.0f;                                      // (false for NaN)
}

// fine: w x h pixels per frame, coarse: (w / 2) x (h / 2)
__global__ __launch_bounds__(OD_T)
void k_od_down(const float* __restrict__ fine, int w, int h, float depth_diff, float* __restrict__ coarse) {
    const int w2 = w / 2, h2 = h / 2, i = blockIdx.x * OD_T + threadIdx.x;
    if (i >= w2 * h2) return;
    const int u = i % w2, v = i / w2;
    const float* f = fine + (size_t)blockIdx.y * w * h;
    const size_t a = (size_t)(2 * v) * w + 2 * u;
    const float zz[4] = {f[a], f[a + 1], f[a + w], f[a + w + 1]};                   // 2u + 1 < w and 2v + 1 < h by the integer division
    float z0 = 0.f, sum = 0.f;
    int count = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(zz[k] > 0.f)) continue;
        if (count == 0 && z0 == 0.f) z0 = zz[k];
        if (fabsf(zz[k] - z0) <= depth_diff) { sum = count ? sum + zz[k] : zz[k]; ++count; }
    }
    coarse[(size_t)blockIdx.y * w2 * h2 + i] = count ? sum / (float)count : 0.0f;
}

template <bool MAPS>
__global__ __launch_bounds__(OD_T)
void k_od_normals(OdLevel L, float depth_diff, float* __restrict__ vertex_map, float* __restrict__ normal_map, int* __restrict__ flag) {
    __shared__ int s_cnt[4];
    const int i = blockIdx.x * OD_T + threadIdx.x, f = blockIdx.y;
    const bool in = i < L.npx;
    const float* z = L.z + (size_t)f * L.npx;
    float n[3] = {0.f, 0.f, 0.f}, V[3] = {0.f, 0.f, 0.f};
    bool valid = false, has = false;
    if (in) {
        const int u = i % L.w, v = i / L.w;
        const float z0 = z[i];
        valid = z0 > 0.f;
        if (valid) pinhole_vertex(u, v, z0, L.k, V);
        if (valid && u + 1 < L.w && v + 1 < L.h) {
            const float zu = z[i + 1], zv = z[i + L.w];
            if (zu > 0.f && zv > 0.f && fabsf(zu - z0) <= depth_diff && fabsf(zv - z0) <= depth_diff) {   // O3
                float A[3], B[3];
                pinhole_vertex(u + 1, v, zu, L.k, A);
                pinhole_vertex(u, v + 1, zv, L.k, B);
                const float a0 = A[0] - V[0], a1 = A[1] - V[1], a2 = A[2] - V[2];
                const float b0 = B[0] - V[0], b1 = B[1] - V[1], b2 = B[2] - V[2];
                const float n0 = b1 * a2 - b2 * a1, n1 = b2 * a0 - b0 * a2, n2 = b0 * a1 - b1 * a0;
                const Row3 unit = normalized_or_zero(n0, n1, n2, &has);
                n[0] = unit.x; n[1] = unit.y; n[2] = unit.z;
            }
        }
        float* nm = (MAPS ? normal_map : L.nrm + 3 * (size_t)f * L.npx);
        if (nm) { nm[3 * (size_t)i] = n[0]; nm[3 * (size_t)i + 1] = n[1]; nm[3 * (size_t)i + 2] = n[2]; }
        if (MAPS) {
            if (vertex_map) { vertex_map[3 * (size_t)i] = V[0]; vertex_map[3 * (size_t)i + 1] = V[1]; vertex_map[3 * (size_t)i + 2] = V[2]; }
            if (flag) flag[i] = has ? 1 : 0;
        }
    }
    if (MAPS) return;
    const int c = tree_block_count(valid ? 1 : 0, s_cnt);
    if (threadIdx.x == 0 && c) atomicAdd(&L.nvalid[f * OD_L + L.level], c);
}

// blockIdx.y = pair p: source frame p + 1, target frame p.  part: the pair's rows of partials at part + (p * gridDim.x + b) * OD_ROW.
template <bool TERMS>
__global__ __launch_bounds__(OD_T)
void k_od_iterate(OdLevel L, float zmax, float depth_diff, OdState* __restrict__ st_all, double* __restrict__ part,
                  unsigned* __restrict__ tickets, OdTerms* __restrict__ terms) {
    __shared__ double s_lds[4 * OD_NV];
    __shared__ double s_tot[OD_ROW];
    __shared__ float s_solve[56];
    __shared__ int s_last;
    const int p = blockIdx.y, nblk = gridDim.x;
    OdState* st = st_all + p;
    if (!TERMS && st->s.done) return;                       // (every workgroup of the pair alike: only the tail of a launch writes it)
    const Pose16 P = load_pose(st->s.T, 0);                 // wave-uniform
    const float* zs = L.z + (size_t)(p + 1) * L.npx;
    const float* zt = L.z + (size_t)p * L.npx;
    const float* nt = L.nrm + 3 * (size_t)p * L.npx;
    const int i = blockIdx.x * OD_T + threadIdx.x;
    double v[OD_NV];
#pragma unroll
    for (int k = 0; k < OD_NV; ++k) v[k] = 0.0;
    const float z0 = i < L.npx ? zs[i] : 0.f;
    if (z0 > 0.f) {
        float S[3], qx, qy, qz;
        int u, w;
        pinhole_vertex(i % L.w, i / L.w, z0, L.k, S);
        pose_apply(P, S[0], S[1], S[2], qx, qy, qz);                                   // O5: the source vertex in the target's camera
        if (pinhole_project<1>(L.k, zmax, qx, qy, qz, u, w) && u >= 0 && u < L.w && w >= 0 && w < L.h) {
            const size_t j = (size_t)w * L.w + u;
            CorrTgt G;
            G.n[0] = nt[3 * j]; G.n[1] = nt[3 * j + 1]; G.n[2] = nt[3 * j + 2];
            const float ztj = zt[j];
            if ((G.n[0] != 0.f || G.n[1] != 0.f || G.n[2] != 0.f) && fabsf(ztj - qz) <= depth_diff) {
                pinhole_vertex(u, w, ztj, L.k, G.q);
                const float ex = qx - G.q[0], ey = qy - G.q[1], ez = qz - G.q[2];
                CorrRec R;
                corr_rec<0>(qx, qy, qz, ex * ex + (ey * ey + ez * ez), G, R);     // O6
                rec_terms<0, false>(R, IcpLoss{TDV_ICP_LOSS_L2, 0.f}, [&v](int k, double t) { v[k] = t; });
            }
        }
    }
    // O7: the workgroup's sums, then its row
    const double s = tree_block_sums<OD_NV>(v, s_lds);
    double* row = part + ((size_t)p * nblk + blockIdx.x) * OD_ROW;
    if (threadIdx.x < OD_NV) row[threadIdx.x] = s;
    // release by the wave that wrote the row, acquire by the workgroup that folds (icp.hip: acc_ticket_fold)
    if (threadIdx.x < 64) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&tickets[p], 1u) == (unsigned)nblk - 1u;
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
    for (int k = 0; k < OD_NV; ++k) v[k] = 0.0;
    const double* rows = part + (size_t)p * nblk * OD_ROW;
    for (int b = threadIdx.x; b < nblk; b += OD_T)
#pragma unroll
        for (int k = 0; k < OD_NV; ++k) v[k] += rows[(size_t)b * OD_ROW + k];
    const double tot = tree_block_sums<OD_NV>(v, s_lds);
    const int n_valid = L.nvalid[(p + 1) * OD_L + L.level];
    if (TERMS) {
        if (threadIdx.x < OD_NV) terms->sums[threadIdx.x] = tot;
        if (threadIdx.x == 0) { terms->n_valid = n_valid; terms->pad = 0; tickets[p] = 0u; }
        return;
    }
    if (threadIdx.x < OD_NV) s_tot[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x != 0) return;
    tickets[p] = 0u;                                        // ready for the next launch (stream order)
    icp_update<0>(s_tot, n_valid, &st->s, 0, st->s.iter, st->s.rmse, P.T, s_solve);      // O8
}

// O8 between levels.  done >= 0: that level has finished - its iterations and correspondences go to the record, and fitness, rmse and
// n_corr too if it applied an iteration.  Then the iteration state restarts; T is carried.
__global__ void k_od_level(OdState* __restrict__ st_all, int n_pairs, int done_level) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    OdState& st = st_all[p];
    if (done_level >= 0) {
        st.iterations[done_level] = st.s.applied;
        st.n_corr_level[done_level] = st.s.last_n_corr_applied;
        if (st.s.applied > 0) { st.fitness = st.s.fitness; st.rmse = st.s.rmse; st.n_corr = st.s.last_n_corr_applied; }
    }
    st.s.fitness = 0.f; st.s.rmse = 0.f;
    st.s.n_corr = 0; st.s.applied = 0; st.s.done = 0; st.s.iter = 0; st.s.last_n_corr_applied = 0;
}

// ------------------------------------------------------------------------------------------------ host
struct OdPyramid { OdLevel lv[OD_L]; int n_levels, n_frames; int* nvalid; };

// Workspace for n_frames frames of the camera's size at n_levels levels; O4's intrinsics.  Nothing is enqueued but the counts' memset.
int od_alloc(tdv_ctx* ctx, int n_frames, const FrameCamera& cam, int n_levels, OdPyramid* py) {
    py->n_levels = n_levels; py->n_frames = n_frames;
    TDV_TRY(ws_alloc(ctx, (size_t)n_frames * OD_L, &py->nvalid));
    TDV_HIP(ctx, hipMemsetAsync(py->nvalid, 0, (size_t)n_frames * OD_L * sizeof(int), ctx->stream));
    int w = cam.w, h = cam.h;
    Pinhole k = cam.k;
    for (int l = 0; l < n_levels; ++l) {
        OdLevel& L = py->lv[l];
        L.w = w; L.h = h; L.npx = w * h; L.level = l; L.k = k; L.nvalid = py->nvalid;
        TDV_TRY(ws_alloc(ctx, (size_t)n_frames * L.npx, &L.z));
        TDV_TRY(ws_alloc(ctx, (size_t)n_frames * L.npx * 3, &L.nrm));
        w /= 2; h /= 2;
        k = Pinhole{k.fx * 0.5f, k.fy * 0.5f, (k.cx - 0.5f) * 0.5f, (k.cy - 0.5f) * 0.5f};
    }
    return TDV_OK;
}

unsigned od_blocks(int npx) { return (unsigned)((npx + OD_T - 1) / OD_T); }

// O1 for `count` frames stored back to back at d_raw, into the pyramid's slots from `slot` on
int od_depth0(tdv_ctx* ctx, const OdPyramid& py, const uint16_t* d_raw, int slot, int count, float inv_scale, float zmax) {
    const OdLevel& L = py.lv[0];
    k_od_depth0<<<dim3(od_blocks(L.npx), count), OD_T, 0, ctx->stream>>>(d_raw, L.npx, inv_scale, zmax, L.z + (size_t)slot * L.npx);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// O10 for one frame, into the pyramid's slot `slot`: the other way to fill level 0
int od_depth0(tdv_ctx* ctx, const OdPyramid& py, const float* d_depth, int slot, float zmax) {
    const OdLevel& L = py.lv[0];
    k_od_depth0_f32<<<od_blocks(L.npx), OD_T, 0, ctx->stream>>>(d_depth, L.npx, zmax, L.z + (size_t)slot * L.npx);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

// O4 and O3 for every frame and level, once level 0's depths stand
int od_build(tdv_ctx* ctx, const OdPyramid& py, float depth_diff) {
    hipStream_t s = ctx->stream;
    for (int l = 0; l + 1 < py.n_levels; ++l)
        k_od_down<<<dim3(od_blocks(py.lv[l + 1].npx), py.n_frames), OD_T, 0, s>>>(py.lv[l].z, py.lv[l].w, py.lv[l].h, depth_diff, py.lv[l + 1].z);
    for (int l = 0; l < py.n_levels; ++l)
        k_od_normals<false><<<dim3(od_blocks(py.lv[l].npx), py.n_frames), OD_T, 0, s>>>(py.lv[l], depth_diff, nullptr, nullptr, nullptr);
    TDV_CHECK_LAUNCH(ctx);
    return TDV_OK;
}

struct OdRun { OdState* st; double* part; unsigned* tickets; };

// states from the start poses (h_T0: n_pairs x 16, or nullptr for identities), partial rows for the finest level, tickets at 0
int od_run_alloc(tdv_ctx* ctx, const OdPyramid& py, int n_pairs, const float* h_T0, OdRun* run) {
    std::vector<OdState> init((size_t)n_pairs);
    std::memset(init.data(), 0, init.size() * sizeof(OdState));
    for (int p = 0; p < n_pairs; ++p) {
        if (h_T0) std::memcpy(init[p].s.T, h_T0 + (size_t)p * 16, 64); else pose_identity(init[p].s.T);
        std::memcpy(init[p].s.res_T, init[p].s.T, 64);
    }
    TDV_TRY(upload(ctx, init.data(), init.size(), &run->st));
    TDV_TRY(ws_alloc(ctx, (size_t)n_pairs * od_blocks(py.lv[0].npx) * OD_ROW, &run->part));
    TDV_TRY(ws_alloc(ctx, (size_t)n_pairs, &run->tickets));
    TDV_HIP(ctx, hipMemsetAsync(run->tickets, 0, (size_t)n_pairs * sizeof(unsigned), ctx->stream));
    return TDV_OK;
}

// O8 for n_pairs pairs together (pair p: frames p + 1 onto p), the results down in one read-back.  rider (optional, tsdf_track.hpp):
// the caller's bytes land behind the records in the pinned block - the offset is formed here, from the size reserved here - and come
// down in the same enqueue, before the one wait.
int od_iterate(tdv_ctx* ctx, const OdPyramid& py, const tdv_odometry_params& prm, int n_pairs, const OdRun& run, tdv_odometry_result* out,
               const OdRider* rider) {
    hipStream_t s = ctx->stream;
    const unsigned pb = (unsigned)((n_pairs + 63) / 64);
    int prev = -1;
    for (int l = py.n_levels - 1; l >= 0; --l) {
        if (prm.max_iterations[l] == 0) continue;
        k_od_level<<<pb, 64, 0, s>>>(run.st, n_pairs, prev);
        const OdLevel& L = py.lv[l];
        for (int it = 0; it < prm.max_iterations[l]; ++it)
            k_od_iterate<false><<<dim3(od_blocks(L.npx), n_pairs), OD_T, 0, s>>>(L, prm.zmax, prm.depth_diff, run.st, run.part, run.tickets, nullptr);
        prev = l;
    }
    k_od_level<<<pb, 64, 0, s>>>(run.st, n_pairs, prev);
    TDV_CHECK_LAUNCH(ctx);
    const size_t rec_bytes = align_up((size_t)n_pairs * sizeof(OdState), 16);
    TDV_TRY(pin_reserve(ctx, rec_bytes + (rider ? rider->bytes : 0)));
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, run.st, (size_t)n_pairs * sizeof(OdState), hipMemcpyDeviceToHost, s));
    if (rider) TDV_HIP(ctx, hipMemcpyAsync(ctx->pin + rec_bytes, rider->d_src, rider->bytes, hipMemcpyDeviceToHost, s));
    TDV_TRY(finish(ctx));
    if (rider) std::memcpy(rider->h_dst, ctx->pin + rec_bytes, rider->bytes);
    const OdState* h = reinterpret_cast<const OdState*>(ctx->pin);
    for (int p = 0; p < n_pairs; ++p) {
        std::memcpy(out[p].T, h[p].s.T, 64);
        out[p].fitness = h[p].fitness; out[p].rmse = h[p].rmse; out[p].n_corr = h[p].n_corr;
        for (int l = 0; l < OD_L; ++l) { out[p].iterations[l] = h[p].iterations[l]; out[p].n_corr_level[l] = h[p].n_corr_level[l]; }
    }
    return TDV_OK;
}

// A pair ready to iterate: the workspace, level 0 of the target (slot 0: O1 or O10, as the target comes) and of the source (slot 1), the
// pyramid, and the run state from the start pose
int od_pair_setup(tdv_ctx* ctx, const uint16_t* d_src, const OdTarget& tgt, const FrameCamera& cam, const float* h_T0,
                  const tdv_odometry_params& prm, OdPyramid* py, OdRun* run) {
    TDV_TRY(od_alloc(ctx, 2, cam, prm.n_levels, py));
    TDV_TRY(tgt.raw ? od_depth0(ctx, *py, tgt.raw, 0, 1, cam.inv_scale(), prm.zmax) : od_depth0(ctx, *py, tgt.depth, 0, prm.zmax));
    TDV_TRY(od_depth0(ctx, *py, d_src, 1, 1, cam.inv_scale(), prm.zmax));
    TDV_TRY(od_build(ctx, *py, prm.depth_diff));
    return od_run_alloc(ctx, *py, 1, h_T0, run);
}

// O2 and O3 of one frame (level 0): maps, rows and count.  host: every output is a host array and goes through the workspace.
int od_maps(tdv_ctx* ctx, const uint16_t* d_raw, const FrameCamera& cam, const tdv_odometry_params& prm, float* vertex_map, float* normal_map,
            float* out_xyz, float* out_normals, int capacity, int* n_out, bool host) {
    hipStream_t s = ctx->stream;
    OdLevel L{cam.w, cam.h, cam.w * cam.h, 0, cam.k, nullptr, nullptr, nullptr};
    const size_t npx = cam.npx();
    float *d_vm = host ? nullptr : vertex_map, *d_nm = host ? nullptr : normal_map, *d_xyz = host ? nullptr : out_xyz,
          *d_nrm = host ? nullptr : out_normals;
    int *flag = nullptr, *pos = nullptr, *d_total = nullptr, total = 0;
    TDV_TRY(ws_alloc(ctx, npx, &L.z));
    k_od_depth0<<<dim3(od_blocks(L.npx), 1), OD_T, 0, s>>>(d_raw, L.npx, cam.inv_scale(), prm.zmax, L.z);
    if (n_out) {
        // the count first, so that a capacity that is too small ends the call before anything is written
        TDV_TRY(ws_alloc(ctx, npx, &flag));
        TDV_TRY(ws_alloc(ctx, npx, &pos));
        TDV_TRY(ws_alloc(ctx, 1, &d_total));
        TDV_TRY(pin_reserve(ctx, sizeof(int)));
        k_od_normals<true><<<dim3(od_blocks(L.npx), 1), OD_T, 0, s>>>(L, prm.depth_diff, nullptr, nullptr, flag);
        TDV_TRY(exclusive_scan_dev(ctx, flag, L.npx, pos, d_total));
        TDV_TRY(fetch_state(ctx, d_total, &total));
        *n_out = total;
        if (total > capacity) return TDV_ERR_BAD_ARG;
    }
    const bool rows = n_out && total > 0 && (out_xyz || out_normals);
    if ((host && vertex_map) || (rows && out_xyz && !d_vm)) TDV_TRY(ws_alloc(ctx, npx * 3, &d_vm));
    if ((host && normal_map) || (rows && out_normals && !d_nm)) TDV_TRY(ws_alloc(ctx, npx * 3, &d_nm));
    if (!d_vm && !d_nm) return TDV_OK;
    k_od_normals<true><<<dim3(od_blocks(L.npx), 1), OD_T, 0, s>>>(L, prm.depth_diff, d_vm, d_nm, nullptr);
    if (rows) {
        if (host && out_xyz) TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &d_xyz));
        if (host && out_normals) TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &d_nrm));
        k_gather_flagged<<<od_blocks(L.npx), 256, 0, s>>>(flag, pos, d_vm, d_nm, 3, L.npx, nullptr, d_xyz, d_nrm);
    }
    TDV_CHECK_LAUNCH(ctx);
    if (!host) return TDV_OK;
    TDV_TRY(download(ctx, vertex_map, d_vm, npx * 3));
    TDV_TRY(download(ctx, normal_map, d_nm, npx * 3));
    if (rows) { TDV_TRY(download(ctx, out_xyz, d_xyz, (size_t)total * 3)); TDV_TRY(download(ctx, out_normals, d_nrm, (size_t)total * 3)); }
    return finish(ctx);
}

bool od_maps_args_ok(const tdv_ctx* ctx, const void* raw, const FrameCamera& cam, const tdv_odometry_params* prm, const float* out_xyz,
                     const float* out_normals, int capacity, const int* n_out) {
    if (!ctx || !frame_camera_ok(cam, true) || !prm || !odometry_params_ok(prm, 0, 0) || capacity < 0) return false;
    if (cam.npx() != 0 && !raw) return false;
    if (capacity > 0 && !out_xyz && !out_normals) return false;
    if ((out_xyz || out_normals) && !n_out) return false;   // rows need the count: it is what bounds them
    return true;
}

// what the entry points with two frames check alike, before the call begins
bool od_frames_args_ok(const tdv_ctx* ctx, const void* src, const OdTarget& tgt, const FrameCamera& cam, const tdv_odometry_params* prm) {
    if (!ctx || !frame_camera_ok(cam, true) || !odometry_params_ok(prm, cam.w, cam.h)) return false;
    return cam.npx() == 0 || (src && (tgt.raw || tgt.depth));
}

template <class T>
int od_upload_in_place(tdv_ctx* ctx, const T** p, size_t n) {
    T* d;
    TDV_TRY(upload(ctx, *p, n, &d));
    *p = d;
    return TDV_OK;
}

// The four pair entry points after they have named their camera and target.  host: the frames are host arrays and go up first.
int od_pair_call(tdv_ctx* ctx, const uint16_t* raw_src, OdTarget tgt, const FrameCamera& cam, const float* h_T0, const tdv_odometry_params* params,
                 tdv_odometry_result* out, bool host) {
    if (!od_frames_args_ok(ctx, raw_src, tgt, cam, params) || !out) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    odometry_empty_result(h_T0, out);
    if (cam.npx() == 0) return TDV_OK;
    if (host) {
        TDV_TRY(od_upload_in_place(ctx, &raw_src, cam.npx()));
        TDV_TRY(tgt.raw ? od_upload_in_place(ctx, &tgt.raw, cam.npx()) : od_upload_in_place(ctx, &tgt.depth, cam.npx()));
    }
    return odometry_pair(ctx, raw_src, tgt, cam, h_T0, *params, out);
}

}  // namespace

// ---- defined here once, and called under these names from here and from tsdf_raycast.hip (tsdf_track.hpp)
bool odometry_params_ok(const tdv_odometry_params* p, int w, int h) {
    if (!p || !positive_finite(p->depth_diff) || !positive_finite(p->zmax)) return false;
    if (p->n_levels < 1 || p->n_levels > OD_L) return false;
    for (int l = 0; l < OD_L; ++l) if (p->max_iterations[l] < 0) return false;
    if ((size_t)w * h != 0 && ((w >> (p->n_levels - 1)) < 1 || (h >> (p->n_levels - 1)) < 1)) return false;      // no level with a side of 0
    return true;
}

void odometry_empty_result(const float* T0, tdv_odometry_result* out) {
    std::memset(out, 0, sizeof(*out));
    if (T0) std::memcpy(out->T, T0, 64); else pose_identity(out->T);
}

int odometry_pair(tdv_ctx* ctx, const uint16_t* d_raw_src, const OdTarget& tgt, const FrameCamera& cam, const float* h_T0,
                  const tdv_odometry_params& prm, tdv_odometry_result* out, const OdRider* rider) {
    OdPyramid py;
    OdRun run;
    TDV_TRY(od_pair_setup(ctx, d_raw_src, tgt, cam, h_T0, prm, &py, &run));
    return od_iterate(ctx, py, prm, 1, run, out, rider);
}

}  // namespace tdv

using namespace tdv;

extern "C" {

void tdv_odometry_default_params(tdv_odometry_params* p) {
    if (!p) return;
    p->depth_diff = 0.03f; p->zmax = 10.f; p->n_levels = 3;
    p->max_iterations[0] = 20; p->max_iterations[1] = 10; p->max_iterations[2] = 5; p->max_iterations[3] = 0;
}

int tdv_depth_maps_dev(tdv_ctx* ctx, const uint16_t* d_raw, int width, int height, float scale, float fx, float fy, float cx, float cy,
                       const tdv_odometry_params* params, float* d_vertex_map, float* d_normal_map, float* d_out_xyz, float* d_out_normals,
                       int capacity, int* n_out) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!od_maps_args_ok(ctx, d_raw, cam, params, d_out_xyz, d_out_normals, capacity, n_out)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (n_out) *n_out = 0;
    if (cam.npx() == 0) return TDV_OK;
    return od_maps(ctx, d_raw, cam, *params, d_vertex_map, d_normal_map, d_out_xyz, d_out_normals, capacity, n_out, false);
}

int tdv_depth_maps(tdv_ctx* ctx, const uint16_t* raw, int width, int height, float scale, float fx, float fy, float cx, float cy,
                   const tdv_odometry_params* params, float* vertex_map, float* normal_map, float* out_xyz, float* out_normals, int capacity,
                   int* n_out) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!od_maps_args_ok(ctx, raw, cam, params, out_xyz, out_normals, capacity, n_out)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (n_out) *n_out = 0;
    if (cam.npx() == 0) return TDV_OK;
    uint16_t* d_raw;
    TDV_TRY(upload(ctx, raw, cam.npx(), &d_raw));
    return od_maps(ctx, d_raw, cam, *params, vertex_map, normal_map, out_xyz, out_normals, capacity, n_out, true);
}

int tdv_depth_odometry_terms_dev(tdv_ctx* ctx, const uint16_t* d_raw_src, const uint16_t* d_raw_tgt, int width, int height, float scale, float fx,
                                 float fy, float cx, float cy, const float* h_T, int level, const tdv_odometry_params* params, double* h_sums,
                                 int* n_valid_src) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    const OdTarget tgt{d_raw_tgt, nullptr};
    if (!od_frames_args_ok(ctx, d_raw_src, tgt, cam, params) || !h_T || !h_sums || level < 0 || level >= params->n_levels) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    for (int k = 0; k < OD_NV; ++k) h_sums[k] = 0.0;
    if (n_valid_src) *n_valid_src = 0;
    if (cam.npx() == 0) return TDV_OK;
    OdPyramid py;
    OdRun run;
    OdTerms *d_terms, terms;
    TDV_TRY(od_pair_setup(ctx, d_raw_src, tgt, cam, h_T, *params, &py, &run));
    TDV_TRY(ws_alloc(ctx, 1, &d_terms));
    TDV_TRY(pin_reserve(ctx, sizeof(OdTerms)));
    const OdLevel& L = py.lv[level];
    k_od_iterate<true><<<dim3(od_blocks(L.npx), 1), OD_T, 0, ctx->stream>>>(L, params->zmax, params->depth_diff, run.st, run.part, run.tickets, d_terms);
    TDV_CHECK_LAUNCH(ctx);
    TDV_TRY(fetch_state(ctx, d_terms, &terms));
    std::memcpy(h_sums, terms.sums, sizeof(terms.sums));
    if (n_valid_src) *n_valid_src = terms.n_valid;
    return TDV_OK;
}

int tdv_depth_odometry_dev(tdv_ctx* ctx, const uint16_t* d_raw_src, const uint16_t* d_raw_tgt, int width, int height, float scale, float fx,
                           float fy, float cx, float cy, const float* h_T0, const tdv_odometry_params* params, tdv_odometry_result* out) {
    return od_pair_call(ctx, d_raw_src, OdTarget{d_raw_tgt, nullptr}, FrameCamera{width, height, scale, {fx, fy, cx, cy}}, h_T0, params, out, false);
}

int tdv_depth_odometry(tdv_ctx* ctx, const uint16_t* raw_src, const uint16_t* raw_tgt, int width, int height, float scale, float fx, float fy,
                       float cx, float cy, const float* T0, const tdv_odometry_params* params, tdv_odometry_result* out) {
    return od_pair_call(ctx, raw_src, OdTarget{raw_tgt, nullptr}, FrameCamera{width, height, scale, {fx, fy, cx, cy}}, T0, params, out, true);
}

int tdv_depth_odometry_to_depth_dev(tdv_ctx* ctx, const uint16_t* d_raw_src, const float* d_depth_tgt, int width, int height, float scale,
                                    float fx, float fy, float cx, float cy, const float* h_T0, const tdv_odometry_params* params,
                                    tdv_odometry_result* out) {
    return od_pair_call(ctx, d_raw_src, OdTarget{nullptr, d_depth_tgt}, FrameCamera{width, height, scale, {fx, fy, cx, cy}}, h_T0, params, out, false);
}

int tdv_depth_odometry_to_depth(tdv_ctx* ctx, const uint16_t* raw_src, const float* depth_tgt, int width, int height, float scale, float fx,
                                float fy, float cx, float cy, const float* T0, const tdv_odometry_params* params, tdv_odometry_result* out) {
    return od_pair_call(ctx, raw_src, OdTarget{nullptr, depth_tgt}, FrameCamera{width, height, scale, {fx, fy, cx, cy}}, T0, params, out, true);
}

int tdv_depth_odometry_sequence_dev(tdv_ctx* ctx, const uint16_t* d_raw, int n_frames, int width, int height, float scale, float fx, float fy,
                                    float cx, float cy, const float* h_init, const tdv_odometry_params* params, float* h_poses,
                                    tdv_odometry_result* h_pairs) {
    const FrameCamera cam{width, height, scale, {fx, fy, cx, cy}};
    if (!ctx || !frame_camera_ok(cam, true) || !odometry_params_ok(params, width, height) || n_frames < 0 || n_frames > TDV_TSDF_MAX_FRAMES ||
        (n_frames > 0 && !h_poses))
        return TDV_ERR_BAD_ARG;
    const size_t npx = cam.npx();
    if (npx != 0 && n_frames > 0 && !d_raw) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    if (n_frames == 0) return TDV_OK;
    const int n_pairs = n_frames - 1;
    std::vector<tdv_odometry_result> res((size_t)n_frames);
    std::memset(&res[0], 0, sizeof(res[0]));
    for (int k = 1; k < n_frames; ++k) odometry_empty_result(h_init ? h_init + 16 * (size_t)k : nullptr, &res[k]);
    if (npx != 0 && n_pairs > 0) {
        OdPyramid py;
        OdRun run;
        TDV_TRY(od_alloc(ctx, n_frames, cam, params->n_levels, &py));
        TDV_TRY(od_depth0(ctx, py, d_raw, 0, n_frames, cam.inv_scale(), params->zmax));
        TDV_TRY(od_build(ctx, py, params->depth_diff));
        TDV_TRY(od_run_alloc(ctx, py, n_pairs, h_init ? h_init + 16 : nullptr, &run));
        TDV_TRY(od_iterate(ctx, py, *params, n_pairs, run, res.data() + 1, nullptr));
    }
    // O9: P_0 = I, P_k = P_(k-1) T_k, each entry the f64 sum of four f64 products in index order, rounded once
    pose_identity(h_poses);
    for (int k = 1; k < n_frames; ++k) pose_chain_product(h_poses + 16 * (size_t)(k - 1), res[k].T, h_poses + 16 * (size_t)k);
    if (h_pairs) std::memcpy(h_pairs, res.data(), (size_t)n_frames * sizeof(tdv_odometry_result));
    return TDV_OK;
}

}  // extern "C"
