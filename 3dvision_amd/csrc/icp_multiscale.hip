// Multi-scale ICP: coarse-to-fine refinement over a voxel pyramid (include/tdv_hip.h: tdv_icp_multiscale), Open3D's
// t.pipelines.registration.multi_scale_icp.  Nothing here computes: a level is the public stages in a row - the voxel grid with the
// normals riding along (voxel.hip), then the ICP loop of the level's objective and criteria (icp.hip) from the pose the level before
// left - so that level l of instance b is, bit for bit, what the stagewise public calls return on the same ctx.  What the one call
// saves is around the stages: the target's level is built once per level and call, all sources' levels come from the batched voxel
// path, the instances iterate together (icp_batch_run_dev), and the level clouds never leave the workspace.
#include "tdv_internal.hpp"
#include <cmath>
#include <cstring>
#include <vector>

using namespace tdv;

namespace {

// the result of a level that cannot iterate (no points on either side, or 0 iterations): what tdv_icp_dev reports for it
void level_defaults(const float* T0, tdv_icp_result& out) {
    std::memcpy(out.T, T0, 64);
    out.fitness = 0.f; out.rmse = 0.f; out.iterations = 0; out.n_corr = 0;
}

// Everything a call can refuse, before anything is enqueued or written (the pointers of the clouds are the caller's to check: they
// depend on the call shape).  The objective's own rules are icp_objective_check's.
int check_schedule(tdv_ctx* ctx, const tdv_icp_level* levels, int n_levels, int estimation, float epsilon, const float* src_normals,
                   const float* tgt_normals) {
    if (!levels || n_levels < 1 || n_levels > TDV_ICP_MAX_LEVELS) return TDV_ERR_BAD_ARG;
    if (estimation != TDV_ICP_POINT_TO_PLANE && estimation != TDV_ICP_POINT_TO_POINT && estimation != TDV_ICP_GICP) return TDV_ERR_BAD_ARG;
    for (int l = 0; l < n_levels; ++l) {
        const tdv_icp_level& lv = levels[l];
        const bool last = l + 1 == n_levels;
        if (std::isnan(lv.voxel_size) || (!last && !(lv.voxel_size > 0.f))) return TDV_ERR_BAD_ARG;
        if (l > 0 && lv.voxel_size > 0.f && !(lv.voxel_size < levels[l - 1].voxel_size)) return TDV_ERR_BAD_ARG;
        if (!(lv.max_correspondence_distance > 0.f) || !std::isfinite(lv.max_correspondence_distance)) return TDV_ERR_BAD_ARG;
        if (lv.max_iterations < 0) return TDV_ERR_BAD_ARG;
        if (!(lv.relative_fitness > 0.f) || !(lv.relative_rmse >= 0.f)) return TDV_ERR_BAD_ARG;      // (NaN fails both)
    }
    const IcpObjective obj = estimation == TDV_ICP_GICP ? IcpObjective::gicp(src_normals, epsilon) : IcpObjective::plain(estimation == TDV_ICP_POINT_TO_PLANE);
    return icp_objective_check(ctx, obj, tgt_normals, true);
}

// The schedule over n instances against one target.  Instance b = points [h_off[b], h_off[b + 1]) of d_src (and of d_src_normals, GICP),
// start pose h_T0 + 16 b; out[b * n_levels + l].  single: the one instance runs icp_run_dev and voxel_downsample_dev, as tdv_icp_dev and
// tdv_voxel_downsample_normals_dev do; otherwise the batched voxel path and icp_batch_run_dev, whose results are the same bits.
// Arguments have been checked.  Every level rewinds the workspace to where it began: a call needs the room of its largest level.
int multiscale_run(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_off, int n, const float* d_tgt, const float* d_tgt_normals,
                   int nt, const float* h_T0, const tdv_icp_level* levels, int n_levels, int estimation, float epsilon, tdv_icp_level_result* out, bool single) {
    const int total = h_off[n];
    const bool gicp = estimation == TDV_ICP_GICP;
    std::vector<float> T(h_T0, h_T0 + 16 * (size_t)n);
    std::vector<int> start((size_t)n + 1), count((size_t)n);
    std::vector<tdv_icp_result> res((size_t)n);
    int* d_off = nullptr;
    if (!single && total > 0) TDV_TRY(upload(ctx, h_off, (size_t)n + 1, &d_off));
    for (int l = 0; l < n_levels; ++l) {
        const tdv_icp_level& lv = levels[l];
        const WsMark level_mark = ws_mark(ctx);
        // the level's clouds: the caller's, or their voxel means in first-occurrence order with the unit mean normals
        const float *t_xyz = d_tgt, *t_nrm = d_tgt_normals, *s_xyz = d_src, *s_nrm = d_src_normals;
        int nt_l = nt;
        for (int b = 0; b <= n; ++b) start[b] = h_off[b];
        if (lv.voxel_size > 0.f) {
            if (nt > 0) {
                float *o_xyz, *o_nrm = nullptr;
                TDV_TRY(ws_alloc(ctx, (size_t)nt * 3, &o_xyz));
                if (d_tgt_normals) TDV_TRY(ws_alloc(ctx, (size_t)nt * 3, &o_nrm));
                const WsMark m = ws_mark(ctx);
                TDV_TRY(voxel_downsample_dev(ctx, d_tgt, nullptr, nt, lv.voxel_size, TDV_VOXEL_ORDER_FIRST, o_xyz, nullptr, nt, &nt_l, nullptr,
                                             VoxelNormals{d_tgt_normals, o_nrm}));
                ws_rewind(ctx, m);
                t_xyz = o_xyz; t_nrm = o_nrm;
            }
            if (total > 0) {
                float *o_xyz, *o_nrm = nullptr;
                TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &o_xyz));
                if (gicp) TDV_TRY(ws_alloc(ctx, (size_t)total * 3, &o_nrm));
                const WsMark m = ws_mark(ctx);
                // all instances at once; one instance, or a level too coarse for the table, cloud by cloud (voxel.hip) - packed the same way
                TDV_TRY(voxel_downsample_batch_dev(ctx, d_src, h_off, d_off, n, lv.voxel_size, nullptr, VoxelFirst{o_xyz, nullptr, o_nrm}, start.data(),
                                                   gicp ? d_src_normals : nullptr, nullptr, !single));
                ws_rewind(ctx, m);
                s_xyz = o_xyz; s_nrm = o_nrm;
            }
        }
        for (int b = 0; b < n; ++b) count[b] = start[b + 1] - start[b];
        const IcpObjective obj = (gicp ? IcpObjective::gicp(s_nrm, epsilon) : IcpObjective::plain(estimation == TDV_ICP_POINT_TO_PLANE))
                                     .criteria(lv.relative_fitness, lv.relative_rmse);
        if (single) {
            if (count[0] == 0 || nt_l == 0 || lv.max_iterations == 0) level_defaults(T.data(), res[0]);
            else TDV_TRY(icp_run_dev(ctx, s_xyz, count[0], t_xyz, t_nrm, nt_l, T.data(), lv.max_correspondence_distance, lv.max_iterations, obj, 0, &res[0]));
        } else {
            TDV_TRY(icp_batch_run_dev(ctx, s_xyz, start.data(), count.data(), n, t_xyz, t_nrm, nt_l, T.data(), lv.max_correspondence_distance, lv.max_iterations,
                                      obj, 0, res.data()));
        }
        for (int b = 0; b < n; ++b) {
            tdv_icp_level_result& o = out[(size_t)b * n_levels + l];
            o.icp = res[b]; o.ns = count[b]; o.nt = nt_l;
            std::memcpy(&T[16 * (size_t)b], res[b].T, 64);      // (a level that applied nothing reports its start pose: it is passed on unchanged)
        }
        TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));         // nothing of the level is in flight when its memory is handed to the next
        ws_rewind(ctx, level_mark);
    }
    return TDV_OK;
}

}  // namespace

extern "C" {

void tdv_icp_level_default(tdv_icp_level* level) {
    if (!level) return;
    level->voxel_size = -1.f;
    level->max_correspondence_distance = 0.f;
    level->max_iterations = 30;
    level->relative_fitness = INFINITY;
    level->relative_rmse = 1e-6f;
}

int tdv_icp_multiscale_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_offsets, int n_instances,
                                 const float* d_tgt, const float* d_tgt_normals, int nt, const float* h_T0, const tdv_icp_level* levels, int n_levels,
                                 int estimation, float epsilon, tdv_icp_level_result* out) {
    if (!ctx || n_instances < 0 || nt < 0) return TDV_ERR_BAD_ARG;
    if (n_instances > 0) {
        if (!h_src_offsets || !h_T0 || !out || h_src_offsets[0] != 0 || (nt > 0 && !d_tgt)) return TDV_ERR_BAD_ARG;
        for (int b = 0; b < n_instances; ++b) if (h_src_offsets[b + 1] < h_src_offsets[b]) return TDV_ERR_BAD_ARG;
        if (h_src_offsets[n_instances] > 0 && !d_src) return TDV_ERR_BAD_ARG;
    }
    TDV_TRY(call_begin(ctx));
    TDV_TRY(check_schedule(ctx, levels, n_levels, estimation, epsilon, d_src_normals, d_tgt_normals));
    if (n_instances == 0) return TDV_OK;
    TDV_TRY(multiscale_run(ctx, d_src, d_src_normals, h_src_offsets, n_instances, d_tgt, d_tgt_normals, nt, h_T0, levels, n_levels, estimation, epsilon, out, false));
    return finish(ctx);
}

int tdv_icp_multiscale_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                           const float* T0, const tdv_icp_level* levels, int n_levels, int estimation, float epsilon, tdv_icp_level_result* out) {
    if (!ctx || !T0 || !out || ns < 0 || nt < 0 || (ns > 0 && !d_src) || (nt > 0 && !d_tgt)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    TDV_TRY(check_schedule(ctx, levels, n_levels, estimation, epsilon, d_src_normals, d_tgt_normals));
    const int off[2] = {0, ns};
    TDV_TRY(multiscale_run(ctx, d_src, d_src_normals, off, 1, d_tgt, d_tgt_normals, nt, T0, levels, n_levels, estimation, epsilon, out, true));
    return finish(ctx);
}

int tdv_icp_multiscale(tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt,
                       const float* T0, const tdv_icp_level* levels, int n_levels, int estimation, float epsilon, tdv_icp_level_result* out) {
    if (!ctx || !T0 || !out || ns < 0 || nt < 0 || (ns > 0 && !src) || (nt > 0 && !tgt)) return TDV_ERR_BAD_ARG;
    TDV_TRY(call_begin(ctx));
    TDV_TRY(check_schedule(ctx, levels, n_levels, estimation, epsilon, src_normals, tgt_normals));
    float *d_src, *d_src_nrm, *d_tgt, *d_tgt_nrm;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, estimation == TDV_ICP_GICP ? src_normals : nullptr, (size_t)ns * 3, &d_src_nrm));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    TDV_TRY(upload(ctx, tgt_normals, (size_t)nt * 3, &d_tgt_nrm));
    const int off[2] = {0, ns};
    TDV_TRY(multiscale_run(ctx, d_src, d_src_nrm, off, 1, d_tgt, d_tgt_nrm, nt, T0, levels, n_levels, estimation, epsilon, out, true));
    return finish(ctx);
}

}  // extern "C"
