// extern "C" entry points of include/tdv_hip.h: argument checks, host<->device staging through the
// ctx workspace, dispatch to the device pipelines.  This TU replaces the reference's CUDA
// dispatch layer /root/reference/src/gpu_impl.cpp (per-call cudaMalloc/cudaMemcpy/launch/cudaFree)
// with arena-backed staging on one stream per ctx.
#include "tdv_internal.hpp"
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>

using namespace tdv;

namespace {

template <class T>
int upload(tdv_ctx* ctx, const T* host, size_t count, T** dev) {
    *dev = nullptr;
    if (!host || count == 0) return TDV_OK;
    TDV_TRY(ws_alloc(ctx, count, dev));
    TDV_HIP(ctx, hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return TDV_OK;
}
template <class T>
int download(tdv_ctx* ctx, T* host, const T* dev, size_t count) {
    if (!host || !dev || count == 0) return TDV_OK;
    TDV_HIP(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return TDV_OK;
}
int begin(tdv_ctx* ctx) {
    if (!ctx) return TDV_ERR_BAD_ARG;
    TDV_HIP(ctx, hipSetDevice(ctx->device));
    ctx->err[0] = 0;
    return ws_reset(ctx);
}
int finish(tdv_ctx* ctx) {
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TDV_OK;
}

}  // namespace

extern "C" {

int tdv_depth_preprocess(tdv_ctx* ctx, const uint16_t* raw, const uint8_t* mask, int width, int height,
                         float scale, int mask_mode, float* out_depth) {
    if (!raw || !out_depth || width < 0 || height < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    const size_t n = (size_t)width * height;
    if (n == 0) return TDV_OK;
    uint16_t* d_raw; uint8_t* d_mask; float* d_out;
    TDV_TRY(upload(ctx, raw, n, &d_raw));
    TDV_TRY(upload(ctx, mask, n, &d_mask));
    TDV_TRY(ws_alloc(ctx, n, &d_out));
    TDV_TRY(depth_preprocess_dev(ctx, d_raw, d_mask, width, height, scale, mask_mode, d_out));
    TDV_TRY(download(ctx, out_depth, d_out, n));
    return finish(ctx);
}

int tdv_bilateral_filter(tdv_ctx* ctx, const float* depth, int width, int height, float sigma_spatial, float sigma_range,
                         float* out_depth) {
    if (!depth || !out_depth || width < 0 || height < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    const size_t n = (size_t)width * height;
    if (n == 0) return TDV_OK;
    float *d_in, *d_out;
    TDV_TRY(upload(ctx, depth, n, &d_in));
    TDV_TRY(ws_alloc(ctx, n, &d_out));
    TDV_TRY(bilateral_filter_dev(ctx, d_in, d_out, width, height, sigma_spatial, sigma_range));
    TDV_TRY(download(ctx, out_depth, d_out, n));
    return finish(ctx);
}

static int voxel_batch_impl(tdv_ctx* ctx, const float* d_xyz, const int* h_cloud_offsets, int n_clouds, float voxel_size, const float* pinhole4,
                            float* d_out_xyz, int* h_voxel_offsets);
int tdv_voxel_downsample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_cloud_offsets, int n_clouds, float voxel_size,
                                   float* d_out_xyz, int* h_voxel_offsets) {
    return voxel_batch_impl(ctx, d_xyz, h_cloud_offsets, n_clouds, voxel_size, nullptr, d_out_xyz, h_voxel_offsets);
}
int tdv_voxel_downsample_batch_pinhole_dev(tdv_ctx* ctx, const float* d_xyz, const int* h_cloud_offsets, int n_clouds, float voxel_size,
                                           float fx, float fy, float cx, float cy, float* d_out_xyz, int* h_voxel_offsets) {
    if (!(fx > 0.f) || !(fy > 0.f)) return TDV_ERR_BAD_ARG;
    const float cam[4] = {fx, fy, cx, cy};
    return voxel_batch_impl(ctx, d_xyz, h_cloud_offsets, n_clouds, voxel_size, cam, d_out_xyz, h_voxel_offsets);
}
static int voxel_batch_impl(tdv_ctx* ctx, const float* d_xyz, const int* h_cloud_offsets, int n_clouds, float voxel_size, const float* pinhole4,
                            float* d_out_xyz, int* h_voxel_offsets) {
    if (!h_cloud_offsets || !h_voxel_offsets || n_clouds < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    h_voxel_offsets[0] = 0;
    if (n_clouds == 0) return TDV_OK;
    for (int b = 0; b < n_clouds; ++b) if (h_cloud_offsets[b] > h_cloud_offsets[b + 1] || h_cloud_offsets[b] < 0) return TDV_ERR_BAD_ARG;
    const int total = h_cloud_offsets[n_clouds];
    if (h_cloud_offsets[0] != 0 || (total > 0 && (!d_xyz || !d_out_xyz))) return TDV_ERR_BAD_ARG;
    int* d_off;
    TDV_TRY(ws_alloc(ctx, (size_t)n_clouds + 1, &d_off));
    TDV_HIP(ctx, hipMemcpyAsync(d_off, h_cloud_offsets, ((size_t)n_clouds + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    int overflowed = 0;
    TDV_TRY(voxel_downsample_batch_dev(ctx, d_xyz, total, d_off, n_clouds, voxel_size, d_out_xyz, nullptr, nullptr, h_voxel_offsets, &overflowed, nullptr,
                                       pinhole4, pinhole4 ? h_cloud_offsets : nullptr));
    if (!overflowed) return TDV_OK;
    // a voxel with more points than the table's member rows hold (a coarse grid): cloud by cloud on the path without that limit
    int at = 0;
    for (int b = 0; b < n_clouds; ++b) {
        const int n = h_cloud_offsets[b + 1] - h_cloud_offsets[b];
        int v = 0;
        h_voxel_offsets[b] = at;
        if (n > 0) TDV_TRY(voxel_downsample_dev(ctx, d_xyz + (size_t)h_cloud_offsets[b] * 3, nullptr, n, voxel_size, TDV_VOXEL_ORDER_FIRST, d_out_xyz + (size_t)at * 3, nullptr, n, &v));
        at += v;
    }
    h_voxel_offsets[n_clouds] = at;
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TDV_OK;
}

int tdv_mask_resize_nearest(tdv_ctx* ctx, const uint8_t* masks, int n_masks, int src_width, int src_height, int dst_width, int dst_height, uint8_t* out) {
    if (n_masks < 0 || src_width <= 0 || src_height <= 0 || dst_width < 0 || dst_height < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    const size_t ns = (size_t)src_width * src_height * n_masks, nd = (size_t)dst_width * dst_height * n_masks;
    if (nd == 0) return TDV_OK;
    if (!masks || !out) return TDV_ERR_BAD_ARG;
    uint8_t *d_in, *d_out;
    TDV_TRY(upload(ctx, masks, ns, &d_in));
    TDV_TRY(ws_alloc(ctx, nd, &d_out));
    TDV_TRY(mask_resize_nearest_dev(ctx, d_in, n_masks, src_width, src_height, dst_width, dst_height, d_out));
    TDV_TRY(download(ctx, out, d_out, nd));
    return finish(ctx);
}

int tdv_mask_resize_nearest_dev(tdv_ctx* ctx, const uint8_t* d_masks, int n_masks, int src_width, int src_height, int dst_width, int dst_height, uint8_t* d_out) {
    TDV_TRY(begin(ctx));
    return mask_resize_nearest_dev(ctx, d_masks, n_masks, src_width, src_height, dst_width, dst_height, d_out);
}

int tdv_deproject(tdv_ctx* ctx, const float* depth, const uint8_t* bgr, int width, int height,
                  float fx, float fy, float cx, float cy, float zmax,
                  float* out_xyz, float* out_rgb, int capacity, int* n_out) {
    if (!depth || !n_out || width < 0 || height < 0 || capacity < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    *n_out = 0;
    const size_t n = (size_t)width * height;
    if (n == 0) return TDV_OK;
    float* d_depth; uint8_t* d_bgr; float *d_xyz = nullptr, *d_rgb = nullptr;
    TDV_TRY(upload(ctx, depth, n, &d_depth));
    TDV_TRY(upload(ctx, bgr, n * 3, &d_bgr));
    const size_t cap = (size_t)std::min<size_t>((size_t)capacity, n);
    if (out_xyz && cap) TDV_TRY(ws_alloc(ctx, cap * 3, &d_xyz));
    if (out_rgb && bgr && cap) TDV_TRY(ws_alloc(ctx, cap * 3, &d_rgb));
    int st = depth_to_cloud_dev(ctx, nullptr, d_depth, nullptr, d_bgr, width, height, 1.f, 0, fx, fy, cx, cy, zmax,
                                d_xyz, d_rgb, (int)cap, n_out);
    if (st != TDV_OK) return st;
    TDV_TRY(download(ctx, out_xyz, d_xyz, (size_t)*n_out * 3));
    TDV_TRY(download(ctx, out_rgb, d_rgb, (size_t)*n_out * 3));
    return finish(ctx);
}

int tdv_depth_to_cloud(tdv_ctx* ctx, const uint16_t* raw, const uint8_t* mask, const uint8_t* bgr,
                       int width, int height, float scale, int mask_mode,
                       float fx, float fy, float cx, float cy, float zmax,
                       float* out_xyz, float* out_rgb, int capacity, int* n_out) {
    if (!raw || !n_out || width < 0 || height < 0 || capacity < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    *n_out = 0;
    const size_t n = (size_t)width * height;
    if (n == 0) return TDV_OK;
    uint16_t* d_raw; uint8_t *d_mask, *d_bgr; float *d_xyz = nullptr, *d_rgb = nullptr;
    TDV_TRY(upload(ctx, raw, n, &d_raw));
    TDV_TRY(upload(ctx, mask, n, &d_mask));
    TDV_TRY(upload(ctx, bgr, n * 3, &d_bgr));
    const size_t cap = (size_t)std::min<size_t>((size_t)capacity, n);
    if (out_xyz && cap) TDV_TRY(ws_alloc(ctx, cap * 3, &d_xyz));
    if (out_rgb && bgr && cap) TDV_TRY(ws_alloc(ctx, cap * 3, &d_rgb));
    int st = depth_to_cloud_dev(ctx, d_raw, nullptr, d_mask, d_bgr, width, height, scale, mask_mode, fx, fy, cx, cy, zmax,
                                d_xyz, d_rgb, (int)cap, n_out);
    if (st != TDV_OK) return st;
    TDV_TRY(download(ctx, out_xyz, d_xyz, (size_t)*n_out * 3));
    TDV_TRY(download(ctx, out_rgb, d_rgb, (size_t)*n_out * 3));
    return finish(ctx);
}

int tdv_voxel_downsample(tdv_ctx* ctx, const float* xyz, const float* rgb, int n, float voxel_size, int order,
                         float* out_xyz, float* out_rgb, int capacity, int* n_out) {
    if (!n_out || n < 0 || capacity < 0 || (n > 0 && (!xyz || !out_xyz)) || !(voxel_size > 0.f)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    *n_out = 0;
    if (n == 0) return TDV_OK;
    float *d_xyz, *d_rgb, *d_oxyz = nullptr, *d_orgb = nullptr;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    TDV_TRY(upload(ctx, rgb, (size_t)n * 3, &d_rgb));
    const int cap = std::min(capacity, n);
    if (cap) TDV_TRY(ws_alloc(ctx, (size_t)cap * 3, &d_oxyz));
    if (rgb && out_rgb && cap) TDV_TRY(ws_alloc(ctx, (size_t)cap * 3, &d_orgb));
    int st = voxel_downsample_dev(ctx, d_xyz, d_rgb, n, voxel_size, order, d_oxyz, d_orgb, cap, n_out);
    if (st != TDV_OK) return st;
    TDV_TRY(download(ctx, out_xyz, d_oxyz, (size_t)*n_out * 3));
    TDV_TRY(download(ctx, out_rgb, d_orgb, (size_t)*n_out * 3));
    return finish(ctx);
}

int tdv_estimate_normals(tdv_ctx* ctx, const float* xyz, int n, int k, float* out_normals, int* out_knn) {
    if (n < 0 || k <= 0 || (n > 0 && (!xyz || !out_normals))) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    if (n == 0) return TDV_OK;
    float *d_xyz, *d_nrm; int* d_knn = nullptr;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    TDV_TRY(ws_alloc(ctx, (size_t)n * 3, &d_nrm));
    if (out_knn) TDV_TRY(ws_alloc(ctx, (size_t)n * k, &d_knn));
    TDV_TRY(estimate_normals_dev(ctx, d_xyz, n, k, d_nrm, d_knn));
    TDV_TRY(download(ctx, out_normals, d_nrm, (size_t)n * 3));
    TDV_TRY(download(ctx, out_knn, d_knn, (size_t)n * k));
    return finish(ctx);
}

int tdv_compute_fpfh(tdv_ctx* ctx, const float* xyz, const float* normals, int n, float radius,
                     float* out_desc33, int* out_nbr, int* out_nbr_cnt) {
    if (n < 0 || (n > 0 && (!xyz || !normals || !out_desc33))) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    if (n == 0) return TDV_OK;
    float *d_xyz, *d_nrm, *d_desc; int *d_nbr = nullptr, *d_cnt = nullptr;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    TDV_TRY(upload(ctx, normals, (size_t)n * 3, &d_nrm));
    TDV_TRY(ws_alloc(ctx, (size_t)n * 33, &d_desc));
    if (out_nbr) TDV_TRY(ws_alloc(ctx, (size_t)n * 100, &d_nbr));
    if (out_nbr_cnt) TDV_TRY(ws_alloc(ctx, (size_t)n, &d_cnt));
    TDV_TRY(compute_fpfh_dev(ctx, d_xyz, d_nrm, n, radius, d_desc, d_nbr, d_cnt));
    TDV_TRY(download(ctx, out_desc33, d_desc, (size_t)n * 33));
    TDV_TRY(download(ctx, out_nbr, d_nbr, (size_t)n * 100));
    TDV_TRY(download(ctx, out_nbr_cnt, d_cnt, (size_t)n));
    return finish(ctx);
}

int tdv_feature_match(tdv_ctx* ctx, const float* fs, int ns, const float* ft, int nt, int* out_corr) {
    if (ns < 0 || nt < 0 || (ns > 0 && (!fs || !out_corr)) || (nt > 0 && !ft)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    if (ns == 0) return TDV_OK;
    if (nt == 0) { std::memset(out_corr, 0, (size_t)ns * 4); return TDV_OK; }
    float *d_fs, *d_ft; int* d_corr;
    TDV_TRY(upload(ctx, fs, (size_t)ns * 33, &d_fs));
    TDV_TRY(upload(ctx, ft, (size_t)nt * 33, &d_ft));
    TDV_TRY(ws_alloc(ctx, (size_t)ns, &d_corr));
    TDV_TRY(feature_match_dev(ctx, d_fs, ns, d_ft, nt, d_corr));
    TDV_TRY(download(ctx, out_corr, d_corr, (size_t)ns));
    return finish(ctx);
}

int tdv_ransac(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt,
               const float* fs, const float* ft, const int* corr,
               float voxel_size, int max_iterations, float confidence, uint32_t seed,
               tdv_ransac_result* out, int* trace_inliers) {
    if (!out || ns < 0 || nt < 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float *d_src, *d_tgt, *d_fs = nullptr, *d_ft = nullptr; int* d_corr = nullptr;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    if (corr) TDV_TRY(upload(ctx, corr, (size_t)ns, &d_corr));
    else { TDV_TRY(upload(ctx, fs, (size_t)ns * 33, &d_fs)); TDV_TRY(upload(ctx, ft, (size_t)nt * 33, &d_ft)); }
    return ransac_run_dev(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, d_corr, voxel_size, max_iterations, confidence, seed, out, trace_inliers);
}

// ---- ICP: each entry point builds its objective (tdv_internal.hpp: IcpObjective) and runs the body of its call shape
// host arrays: stage the clouds, the target's normals and the objective's own arrays (obj arrives with the caller's host pointers), run
static int icp_host(tdv_ctx* ctx, const float* src, int ns, const float* tgt, const float* tgt_normals, int nt, const float* T0,
                    float distance_threshold, int max_iterations, IcpObjective obj, tdv_icp_result* out) {
    if (!out || !T0 || ns < 0 || nt < 0 || (ns > 0 && !src) || (nt > 0 && !tgt)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    TDV_TRY(icp_objective_check(ctx, obj, tgt_normals, false));
    float *d_src, *d_tgt, *d_nrm, *d_own;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    if (obj.src_normals) { TDV_TRY(upload(ctx, obj.src_normals, (size_t)ns * 3, &d_own)); obj.src_normals = d_own; }
    if (obj.src_rgb) { TDV_TRY(upload(ctx, obj.src_rgb, (size_t)ns * 3, &d_own)); obj.src_rgb = d_own; }
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    TDV_TRY(upload(ctx, tgt_normals, (size_t)nt * 3, &d_nrm));
    if (obj.tgt_color) { TDV_TRY(upload(ctx, obj.tgt_color, (size_t)nt * 4, &d_own)); obj.tgt_color = d_own; }
    if (ns == 0 || nt == 0) {
        std::memcpy(out->T, T0, 64); out->fitness = 0.f; out->rmse = 0.f; out->iterations = 0; out->n_corr = 0;
        return TDV_OK;
    }
    return icp_run_dev(ctx, d_src, ns, d_tgt, d_nrm, nt, T0, distance_threshold, max_iterations, obj, 0, out);
}
// device pointers (pointer and size checks are icp_run_dev's)
static int icp_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, const float* d_tgt_normals, int nt, const float* T0,
                   float distance_threshold, int max_iterations, const IcpObjective& obj, int fixed_iterations, tdv_icp_result* out) {
    TDV_TRY(begin(ctx));
    TDV_TRY(icp_objective_check(ctx, obj, d_tgt_normals, true));
    return icp_run_dev(ctx, d_src, ns, d_tgt, d_tgt_normals, nt, T0, distance_threshold, max_iterations, obj, fixed_iterations, out);
}
// a batch: every argument before anything is enqueued or written
static int icp_batch_dev(tdv_ctx* ctx, const float* d_src, const int* h_src_offsets, int n_instances, const float* d_tgt, const float* d_tgt_normals,
                         int nt, const float* h_T0, float distance_threshold, int max_iterations, const IcpObjective& obj, int fixed_iterations,
                         tdv_icp_result* out) {
    if (!ctx || n_instances < 0 || nt < 0 || max_iterations < 0) return TDV_ERR_BAD_ARG;
    if (n_instances > 0) {
        if (!h_src_offsets || !h_T0 || !out || h_src_offsets[0] != 0 || (nt > 0 && !d_tgt)) return TDV_ERR_BAD_ARG;
        for (int b = 0; b < n_instances; ++b) if (h_src_offsets[b + 1] < h_src_offsets[b]) return TDV_ERR_BAD_ARG;
        if (h_src_offsets[n_instances] > 0 && !d_src) return TDV_ERR_BAD_ARG;
    }
    TDV_TRY(begin(ctx));
    if (n_instances == 0 && obj.kind < ICP_GICP) return TDV_OK;   // (an empty batch: GICP and colored ICP still check their own arguments, the loss is not looked at)
    TDV_TRY(icp_objective_check(ctx, obj, d_tgt_normals, true));
    if (n_instances == 0) return TDV_OK;
    std::vector<int> count((size_t)n_instances);
    for (int b = 0; b < n_instances; ++b) count[b] = h_src_offsets[b + 1] - h_src_offsets[b];
    TDV_TRY(icp_batch_run_dev(ctx, d_src, h_src_offsets, count.data(), n_instances, d_tgt, d_tgt_normals, nt, h_T0, distance_threshold, max_iterations,
                              obj, fixed_iterations, out));
    return finish(ctx);
}

int tdv_icp(tdv_ctx* ctx, const float* src, int ns, const float* tgt, const float* tgt_normals, int nt,
            const float* T0, float distance_threshold, int max_iterations, int point_to_plane,
            tdv_icp_result* out) {
    return icp_host(ctx, src, ns, tgt, tgt_normals, nt, T0, distance_threshold, max_iterations, IcpObjective::plain(point_to_plane), out);
}

int tdv_icp_correspondences(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt,
                            const float* T, float distance_threshold,
                            int* out_corr, float* out_d2, uint8_t* out_accepted, int* out_n_corr) {
    if (!src || !tgt || !T || ns <= 0 || nt <= 0) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float *d_src, *d_tgt;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    IcpOutputs o;
    if (out_corr) TDV_TRY(ws_alloc(ctx, (size_t)ns, &o.corr));
    if (out_d2) TDV_TRY(ws_alloc(ctx, (size_t)ns, &o.d2));
    if (out_accepted) TDV_TRY(ws_alloc(ctx, (size_t)ns, &o.accepted));
    TDV_TRY(icp_correspondences_dev(ctx, d_src, ns, d_tgt, nt, T, distance_threshold, o, out_n_corr));
    TDV_TRY(download(ctx, out_corr, o.corr, (size_t)ns));
    TDV_TRY(download(ctx, out_d2, o.d2, (size_t)ns));
    TDV_TRY(download(ctx, out_accepted, o.accepted, (size_t)ns));
    return finish(ctx);
}

// ---- device-resident entry points
int tdv_icp_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                const float* T0, float distance_threshold, int max_iterations, int point_to_plane,
                int fixed_iterations, tdv_icp_result* out) {
    return icp_dev(ctx, d_src, ns, d_tgt, d_tgt_normals, nt, T0, distance_threshold, max_iterations, IcpObjective::plain(point_to_plane), fixed_iterations, out);
}
int tdv_icp_batch_dev(tdv_ctx* ctx, const float* d_src, const int* h_src_offsets, int n_instances, const float* d_tgt, const float* d_tgt_normals,
                      int nt, const float* h_T0, float distance_threshold, int max_iterations, int point_to_plane, int fixed_iterations,
                      tdv_icp_result* out) {
    return icp_batch_dev(ctx, d_src, h_src_offsets, n_instances, d_tgt, d_tgt_normals, nt, h_T0, distance_threshold, max_iterations,
                         IcpObjective::plain(point_to_plane), fixed_iterations, out);
}
// ---- generalized ICP: tdv_icp / tdv_icp_dev / tdv_icp_batch_dev with the source normals, plane-to-plane terms (icp.hip, MODE 3)
int tdv_gicp(tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt,
             const float* T0, float distance_threshold, int max_iterations, float epsilon, tdv_icp_result* out) {
    return icp_host(ctx, src, ns, tgt, tgt_normals, nt, T0, distance_threshold, max_iterations, IcpObjective::gicp(src_normals, epsilon), out);
}
int tdv_gicp_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                 const float* T0, float distance_threshold, int max_iterations, float epsilon, int fixed_iterations, tdv_icp_result* out) {
    return icp_dev(ctx, d_src, ns, d_tgt, d_tgt_normals, nt, T0, distance_threshold, max_iterations, IcpObjective::gicp(d_src_normals, epsilon),
                   fixed_iterations, out);
}
int tdv_gicp_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_offsets, int n_instances,
                       const float* d_tgt, const float* d_tgt_normals, int nt, const float* h_T0, float distance_threshold,
                       int max_iterations, float epsilon, int fixed_iterations, tdv_icp_result* out) {
    return icp_batch_dev(ctx, d_src, h_src_offsets, n_instances, d_tgt, d_tgt_normals, nt, h_T0, distance_threshold, max_iterations,
                         IcpObjective::gicp(d_src_normals, epsilon), fixed_iterations, out);
}
// ---- colored ICP: the target's colour gradients (color.hip), then tdv_icp / tdv_icp_dev / tdv_icp_batch_dev with the source colours
// and the target's colour table, point-to-plane plus photometric terms (icp.hip, MODE 4)
int tdv_color_gradients(tdv_ctx* ctx, const float* xyz, const float* rgb, const float* normals, int n, int k, float* out_color) {
    if (n < 0 || k <= 0 || k > 255 || (n > 0 && (!xyz || !rgb || !normals || !out_color))) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    if (n == 0) return TDV_OK;
    float *d_xyz, *d_rgb, *d_nrm, *d_color;
    TDV_TRY(upload(ctx, xyz, (size_t)n * 3, &d_xyz));
    TDV_TRY(upload(ctx, rgb, (size_t)n * 3, &d_rgb));
    TDV_TRY(upload(ctx, normals, (size_t)n * 3, &d_nrm));
    TDV_TRY(ws_alloc(ctx, (size_t)n * 4, &d_color));
    TDV_TRY(color_gradients_dev(ctx, d_xyz, d_rgb, d_nrm, n, k, nullptr, d_color));
    TDV_TRY(download(ctx, out_color, d_color, (size_t)n * 4));
    return finish(ctx);
}
int tdv_color_gradients_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, const float* d_normals, int n, int k, const int* d_knn,
                            float* d_color) {
    if (n < 0 || k <= 0 || k > 255 || (n > 0 && (!d_xyz || !d_rgb || !d_normals || !d_color))) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    TDV_TRY(color_gradients_dev(ctx, d_xyz, d_rgb, d_normals, n, k, d_knn, d_color));
    return finish(ctx);
}
int tdv_colored_icp(tdv_ctx* ctx, const float* src, const float* src_rgb, int ns, const float* tgt, const float* tgt_normals,
                    const float* tgt_color, int nt, const float* T0, float distance_threshold, int max_iterations, float lambda_geometric,
                    tdv_icp_result* out) {
    return icp_host(ctx, src, ns, tgt, tgt_normals, nt, T0, distance_threshold, max_iterations,
                    IcpObjective::colored(src_rgb, tgt_color, lambda_geometric), out);
}
int tdv_colored_icp_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_rgb, int ns, const float* d_tgt, const float* d_tgt_normals,
                        const float* d_tgt_color, int nt, const float* T0, float distance_threshold, int max_iterations,
                        float lambda_geometric, int fixed_iterations, tdv_icp_result* out) {
    return icp_dev(ctx, d_src, ns, d_tgt, d_tgt_normals, nt, T0, distance_threshold, max_iterations,
                   IcpObjective::colored(d_src_rgb, d_tgt_color, lambda_geometric), fixed_iterations, out);
}
int tdv_colored_icp_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_rgb, const int* h_src_offsets, int n_instances,
                              const float* d_tgt, const float* d_tgt_normals, const float* d_tgt_color, int nt, const float* h_T0,
                              float distance_threshold, int max_iterations, float lambda_geometric, int fixed_iterations, tdv_icp_result* out) {
    return icp_batch_dev(ctx, d_src, h_src_offsets, n_instances, d_tgt, d_tgt_normals, nt, h_T0, distance_threshold, max_iterations,
                         IcpObjective::colored(d_src_rgb, d_tgt_color, lambda_geometric), fixed_iterations, out);
}
int tdv_ransac_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt,
                   const float* d_fs, const float* d_ft, const int* d_corr,
                   float voxel_size, int max_iterations, float confidence, uint32_t seed,
                   tdv_ransac_result* out, int* trace_inliers) {
    TDV_TRY(begin(ctx));
    return ransac_run_dev(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, d_corr, voxel_size, max_iterations, confidence, seed, out, trace_inliers);
}
int tdv_feature_match_dev(tdv_ctx* ctx, const float* d_fs, int ns, const float* d_ft, int nt, int* d_corr) {
    TDV_TRY(begin(ctx));
    TDV_TRY(feature_match_dev(ctx, d_fs, ns, d_ft, nt, d_corr));
    return finish(ctx);
}
int tdv_estimate_normals_dev(tdv_ctx* ctx, const float* d_xyz, int n, int k, float* d_normals, int* d_knn) {
    TDV_TRY(begin(ctx));
    TDV_TRY(estimate_normals_dev(ctx, d_xyz, n, k, d_normals, d_knn));
    return finish(ctx);
}
int tdv_compute_fpfh_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_normals, int n, float radius,
                         float* d_desc33, int* d_nbr, int* d_nbr_cnt) {
    TDV_TRY(begin(ctx));
    TDV_TRY(compute_fpfh_dev(ctx, d_xyz, d_normals, n, radius, d_desc33, d_nbr, d_nbr_cnt));
    return finish(ctx);
}
int tdv_normals_fpfh_dev(tdv_ctx* ctx, const float* d_xyz, int n, int k, float radius, float* d_normals, float* d_desc33) {
    TDV_TRY(begin(ctx));
    TDV_TRY(normals_fpfh_dev(ctx, d_xyz, n, k, radius, d_normals, d_desc33));
    return finish(ctx);
}
int tdv_radix_sort_pairs_dev(tdv_ctx* ctx, const unsigned long long* d_keys_in, unsigned long long* d_keys_out, const unsigned* d_vals_in,
                             unsigned* d_vals_out, size_t n, int end_bit) {
    TDV_TRY(begin(ctx));
    TDV_TRY(radix_sort_pairs_dev(ctx, d_keys_in, d_keys_out, d_vals_in, d_vals_out, n, end_bit));
    return finish(ctx);
}
int tdv_depth_to_cloud_dev(tdv_ctx* ctx, const uint16_t* d_raw, const uint8_t* d_mask, const uint8_t* d_bgr,
                           int width, int height, float scale, int mask_mode,
                           float fx, float fy, float cx, float cy, float zmax,
                           float* d_xyz, float* d_rgb, int capacity, int* n_out) {
    TDV_TRY(begin(ctx));
    return depth_to_cloud_dev(ctx, d_raw, nullptr, d_mask, d_bgr, width, height, scale, mask_mode, fx, fy, cx, cy, zmax,
                              d_xyz, d_rgb, capacity, n_out);
}
int tdv_voxel_downsample_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_rgb, int n, float voxel_size, int order,
                             float* d_out_xyz, float* d_out_rgb, int capacity, int* n_out) {
    TDV_TRY(begin(ctx));
    return voxel_downsample_dev(ctx, d_xyz, d_rgb, n, voxel_size, order, d_out_xyz, d_out_rgb, capacity, n_out);
}

// ---- Fast Global Registration (fgr.hip)
void tdv_fgr_default_params(tdv_fgr_params* p) {
    if (!p) return;
    p->division_factor = 1.4f; p->maximum_correspondence_distance = 0.025f; p->tuple_scale = 0.95f; p->iteration_number = 64;
    p->maximum_tuple_count = 1000; p->use_absolute_scale = 0; p->decrease_mu = 1; p->tuple_test = 1; p->seed = 42u;
}
// every argument, before anything is enqueued (include/tdv_hip.h: tdv_fgr)
static bool fgr_args_ok(const tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft,
                        float voxel_size, const tdv_fgr_params* p) {
    if (!ctx || !p || ns < 0 || nt < 0) return false;
    if (ns > 0 && (!src || !fs)) return false;
    if (nt > 0 && (!tgt || !ft)) return false;
    if (!std::isfinite(voxel_size) || !(voxel_size > 0.f)) return false;
    if (!std::isfinite(p->division_factor) || !(p->division_factor > 1.f)) return false;
    if (!std::isfinite(p->tuple_scale) || !(p->tuple_scale > 0.f && p->tuple_scale <= 1.f)) return false;
    if (!std::isfinite(p->maximum_correspondence_distance) || !(p->maximum_correspondence_distance > 0.f)) return false;
    return p->iteration_number >= 0 && p->maximum_tuple_count >= 1;
}
static void fgr_empty(tdv_fgr_result* out) {
    std::memset(out, 0, sizeof(*out));
    for (int i = 0; i < 16; ++i) out->T[i] = (i % 5 == 0) ? 1.f : 0.f;
    out->degenerate = 1;
}
int tdv_fgr(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft, float voxel_size,
            const tdv_fgr_params* params, tdv_fgr_result* out) {
    if (!out || !fgr_args_ok(ctx, src, ns, tgt, nt, fs, ft, voxel_size, params)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    if (ns == 0 || nt == 0) { fgr_empty(out); return TDV_OK; }
    float *d_src, *d_tgt, *d_fs, *d_ft;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    TDV_TRY(upload(ctx, fs, (size_t)ns * 33, &d_fs));
    TDV_TRY(upload(ctx, ft, (size_t)nt * 33, &d_ft));
    return fgr_run_dev(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, voxel_size, *params, out, nullptr);
}
int tdv_fgr_dev(tdv_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* d_fs, const float* d_ft, float voxel_size,
                const tdv_fgr_params* params, tdv_fgr_result* out) {
    if (!out || !fgr_args_ok(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, voxel_size, params)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    if (ns == 0 || nt == 0) { fgr_empty(out); return TDV_OK; }
    return fgr_run_dev(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, voxel_size, *params, out, nullptr);
}
int tdv_fgr_correspondences(tdv_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* fs, const float* ft,
                            const tdv_fgr_params* params, int* out_mutual, int cap_mutual, int* out_tuple, int cap_tuple,
                            int* n_mutual, int* n_tuple, long long* trials_run) {
    if (!n_mutual || !n_tuple || !trials_run || cap_mutual < 0 || cap_tuple < 0 || (cap_mutual > 0 && !out_mutual) ||
        (cap_tuple > 0 && !out_tuple) || !fgr_args_ok(ctx, src, ns, tgt, nt, fs, ft, 1.f, params))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    *n_mutual = 0; *n_tuple = 0; *trials_run = 0;
    if (ns == 0 || nt == 0) return TDV_OK;
    float *d_src, *d_tgt, *d_fs, *d_ft;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    TDV_TRY(upload(ctx, fs, (size_t)ns * 33, &d_fs));
    TDV_TRY(upload(ctx, ft, (size_t)nt * 33, &d_ft));
    FgrPairs pr;
    TDV_TRY(fgr_run_dev(ctx, d_src, ns, d_tgt, nt, d_fs, d_ft, 1.f, *params, nullptr, &pr));
    *n_mutual = pr.n_mutual; *n_tuple = pr.n_tuple; *trials_run = pr.trials_run;
    if (pr.n_mutual > cap_mutual || pr.n_tuple > cap_tuple) return TDV_ERR_BAD_ARG;
    TDV_TRY(download(ctx, reinterpret_cast<int2*>(out_mutual), pr.mutual, (size_t)pr.n_mutual));
    TDV_TRY(download(ctx, reinterpret_cast<int2*>(out_tuple), pr.tuple, (size_t)pr.n_tuple));
    return finish(ctx);
}

// ---- ISS keypoints (iss.hip)
void tdv_iss_default_params(tdv_iss_params* p) {
    if (!p) return;
    p->salient_radius = 0.f; p->non_max_radius = 0.f; p->gamma_21 = 0.975; p->gamma_32 = 0.975; p->min_neighbors = 5;
}

int tdv_iss_keypoints(tdv_ctx* ctx, const float* xyz, int n, const tdv_iss_params* params, const float* attr, int attr_width, tdv_iss_result* result,
                      uint8_t* mask, double* saliency, double* eigenvalues, int* support, int* index, float* out_xyz, float* out_attr) {
    if (!iss_args_ok(ctx, xyz, n, params, attr, attr_width, result, out_attr)) return TDV_ERR_BAD_ARG;
    IssOut h; h.mask = mask; h.saliency = saliency; h.eig = eigenvalues; h.support = support; h.index = index; h.xyz = out_xyz; h.attr = out_attr;
    return iss_run_host(ctx, xyz, n, *params, attr, attr_width, result, h);
}

int tdv_iss_keypoints_dev(tdv_ctx* ctx, const float* d_xyz, int n, const tdv_iss_params* params, const float* d_attr, int attr_width,
                          tdv_iss_result* result, uint8_t* d_mask, double* d_saliency, double* d_eigenvalues, int* d_support, int* d_index,
                          float* d_out_xyz, float* d_out_attr) {
    if (!iss_args_ok(ctx, d_xyz, n, params, d_attr, attr_width, result, d_out_attr)) return TDV_ERR_BAD_ARG;
    TDV_TRY(iss_begin(ctx));
    IssOut d; d.mask = d_mask; d.saliency = d_saliency; d.eig = d_eigenvalues; d.support = d_support; d.index = d_index; d.xyz = d_out_xyz;
    d.attr = d_out_attr;
    return iss_run_dev(ctx, d_xyz, n, *params, d_attr, attr_width, result, d, nullptr);
}

// ---- farthest point sampling (fps.hip)
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
    TDV_TRY(fps_begin(ctx));
    FpsOut d; d.index = d_index; d.d2 = d_out_d2; d.xyz = d_out_xyz; d.attr = d_out_attr;
    return fps_run_dev(ctx, d_xyz, n, num_samples, start_index, d_attr, attr_width, result, d, nullptr);
}

int tdv_farthest_point_down_sample_batch_dev(tdv_ctx* ctx, const float* d_xyz, const float* d_attr, int attr_width, const int* h_offsets,
                                             int n_clouds, int num_samples, tdv_fps_result* results, int* h_out_offsets, int* d_index,
                                             float* d_out_d2, float* d_out_xyz, float* d_out_attr) {
    if (!fps_batch_args_ok(ctx, d_xyz, d_attr, attr_width, h_offsets, n_clouds, num_samples, results, h_out_offsets, d_out_attr)) return TDV_ERR_BAD_ARG;
    TDV_TRY(fps_begin(ctx));
    FpsOut d; d.index = d_index; d.d2 = d_out_d2; d.xyz = d_out_xyz; d.attr = d_out_attr;
    return fps_batch_run_dev(ctx, d_xyz, d_attr, attr_width, h_offsets, n_clouds, num_samples, results, h_out_offsets, d);
}

// ---- pose verification (verify.hip)
void tdv_verify_default_params(tdv_verify_params* p) {
    if (!p) return;
    p->pose_direction = TDV_POSE_SOURCE_ONTO_TARGET; p->splat = 1; p->tau = 0.002f; p->zmax = 10.f;
}

int tdv_verify_poses_dev(tdv_ctx* ctx, const float* d_model_xyz, int n_model, const float* h_poses, int n_poses, const uint16_t* d_raw_depth, int width,
                         int height, float scale, float fx, float fy, float cx, float cy, const tdv_verify_params* params,
                         tdv_verify_result* h_results, int* h_order) {
    if (!verify_args_ok(ctx, d_model_xyz, n_model, h_poses, n_poses, d_raw_depth, width, height, scale, fx, fy, params, h_results)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    return verify_run_dev(ctx, d_model_xyz, n_model, h_poses, n_poses, d_raw_depth, width, height, scale, fx, fy, cx, cy, *params, h_results, h_order);
}

int tdv_verify_poses(tdv_ctx* ctx, const float* model_xyz, int n_model, const float* poses, int n_poses, const uint16_t* raw_depth, int width,
                     int height, float scale, float fx, float fy, float cx, float cy, const tdv_verify_params* params, tdv_verify_result* results,
                     int* order) {
    if (!verify_args_ok(ctx, model_xyz, n_model, poses, n_poses, raw_depth, width, height, scale, fx, fy, params, results)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float* d_model; uint16_t* d_raw;
    TDV_TRY(upload(ctx, model_xyz, (size_t)n_model * 3, &d_model));
    TDV_TRY(upload(ctx, raw_depth, (size_t)width * height, &d_raw));
    return verify_run_dev(ctx, d_model, n_model, poses, n_poses, d_raw, width, height, scale, fx, fy, cx, cy, *params, results, order);
}

int tdv_render_depth_dev(tdv_ctx* ctx, const float* d_model_xyz, int n_model, const float* h_pose, int width, int height, float fx, float fy, float cx,
                         float cy, const tdv_verify_params* params, float* d_out_depth, int* n_rendered) {
    if (!verify_args_ok(ctx, d_model_xyz, n_model, h_pose, 1, d_out_depth, width, height, 1.f, fx, fy, params, h_pose)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    return render_depth_run_dev(ctx, d_model_xyz, n_model, h_pose, width, height, fx, fy, cx, cy, *params, d_out_depth, n_rendered);
}

int tdv_render_depth(tdv_ctx* ctx, const float* model_xyz, int n_model, const float* pose, int width, int height, float fx, float fy, float cx, float cy,
                     const tdv_verify_params* params, float* out_depth, int* n_rendered) {
    if (!verify_args_ok(ctx, model_xyz, n_model, pose, 1, out_depth, width, height, 1.f, fx, fy, params, pose)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float *d_model, *d_out;
    TDV_TRY(upload(ctx, model_xyz, (size_t)n_model * 3, &d_model));
    TDV_TRY(ws_alloc(ctx, (size_t)width * height, &d_out));
    TDV_TRY(render_depth_run_dev(ctx, d_model, n_model, pose, width, height, fx, fy, cx, cy, *params, d_out, n_rendered));
    TDV_TRY(download(ctx, out_depth, d_out, (size_t)width * height));
    return finish(ctx);
}

// ---- pose verification from a mesh (verify_mesh.hip)
void tdv_mesh_verify_default_params(tdv_mesh_verify_params* p) {
    if (!p) return;
    p->pose_direction = TDV_POSE_SOURCE_ONTO_TARGET; p->cull = TDV_MESH_CULL_NONE; p->tau = 0.002f; p->zmax = 10.f;
}

int tdv_verify_poses_mesh_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles, const float* h_poses,
                              int n_poses, const uint16_t* d_raw_depth, int width, int height, float scale, float fx, float fy, float cx, float cy,
                              const tdv_mesh_verify_params* params, tdv_verify_result* h_results, int* h_order) {
    if (!mesh_verify_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_poses, n_poses, d_raw_depth, width, height, scale, fx, fy,
                             params, h_results))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    return mesh_verify_run_dev(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_poses, n_poses, d_raw_depth, width, height, scale, fx, fy, cx,
                               cy, *params, h_results, h_order);
}

int tdv_verify_poses_mesh(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* poses, int n_poses,
                          const uint16_t* raw_depth, int width, int height, float scale, float fx, float fy, float cx, float cy,
                          const tdv_mesh_verify_params* params, tdv_verify_result* results, int* order) {
    if (!mesh_verify_args_ok(ctx, vertices, n_vertices, triangles, n_triangles, poses, n_poses, raw_depth, width, height, scale, fx, fy, params,
                             results))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float* d_vtx; int* d_tri; uint16_t* d_raw;
    TDV_TRY(upload(ctx, vertices, (size_t)n_vertices * 3, &d_vtx));
    TDV_TRY(upload(ctx, triangles, (size_t)n_triangles * 3, &d_tri));
    TDV_TRY(upload(ctx, raw_depth, (size_t)width * height, &d_raw));
    return mesh_verify_run_dev(ctx, d_vtx, n_vertices, d_tri, n_triangles, poses, n_poses, d_raw, width, height, scale, fx, fy, cx, cy, *params,
                               results, order);
}

int tdv_render_depth_mesh_dev(tdv_ctx* ctx, const float* d_vertices, int n_vertices, const int* d_triangles, int n_triangles, const float* h_pose,
                              int width, int height, float fx, float fy, float cx, float cy, const tdv_mesh_verify_params* params,
                              float* d_out_depth, int* n_rendered) {
    if (!mesh_verify_args_ok(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_pose, 1, d_out_depth, width, height, 1.f, fx, fy, params,
                             h_pose))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    return mesh_render_run_dev(ctx, d_vertices, n_vertices, d_triangles, n_triangles, h_pose, width, height, fx, fy, cx, cy, *params, d_out_depth,
                               n_rendered);
}

int tdv_render_depth_mesh(tdv_ctx* ctx, const float* vertices, int n_vertices, const int* triangles, int n_triangles, const float* pose, int width,
                          int height, float fx, float fy, float cx, float cy, const tdv_mesh_verify_params* params, float* out_depth,
                          int* n_rendered) {
    if (!mesh_verify_args_ok(ctx, vertices, n_vertices, triangles, n_triangles, pose, 1, out_depth, width, height, 1.f, fx, fy, params, pose))
        return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float *d_vtx, *d_out; int* d_tri;
    TDV_TRY(upload(ctx, vertices, (size_t)n_vertices * 3, &d_vtx));
    TDV_TRY(upload(ctx, triangles, (size_t)n_triangles * 3, &d_tri));
    TDV_TRY(ws_alloc(ctx, (size_t)width * height, &d_out));
    TDV_TRY(mesh_render_run_dev(ctx, d_vtx, n_vertices, d_tri, n_triangles, pose, width, height, fx, fy, cx, cy, *params, d_out, n_rendered));
    TDV_TRY(download(ctx, out_depth, d_out, (size_t)width * height));
    return finish(ctx);
}

// ---- PPF matching (ppf.hip)
void tdv_ppf_default_params(tdv_ppf_params* p) {
    if (!p) return;
    p->distance_step_relative = 0.05f; p->angle_bins = 30; p->rotation_bins = 30; p->ref_stride = 5; p->max_poses = 8;
    p->cluster_translation_relative = 0.1f; p->cluster_rotation = (float)(2.0 * 3.141592653589793 / 30.0); p->flip_model_normals = 0;
}
int tdv_ppf_model_bytes(int nt, const tdv_ppf_params* params, size_t* bytes) {
    PpfPlan plan;
    if (!bytes || !ppf_plan(params, nt, &plan)) return TDV_ERR_BAD_ARG;
    *bytes = plan.bytes;
    return TDV_OK;
}
// every argument of a match, before anything is enqueued (include/tdv_hip.h: tdv_ppf_match)
static bool ppf_match_args_ok(const tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt,
                              float thr, const tdv_ppf_params* params, const tdv_ppf_pose* out_poses, const int* n_poses, PpfPlan* plan) {
    if (!ctx || !out_poses || !n_poses || ns < 0 || !ppf_plan(params, nt, plan)) return false;
    if (ns > 0 && (!src || !src_normals)) return false;
    if (nt > 0 && (!tgt || !tgt_normals)) return false;
    return std::isfinite(thr) && thr > 0.f;
}
static bool ppf_model_ptr_ok(const void* d_model) { return d_model && (reinterpret_cast<uintptr_t>(d_model) & 3) == 0; }
// ... and the table with its info (tdv_ppf_match_dev, tdv_ppf_match_batch_dev)
static bool ppf_model_info_ok(const void* d_model, const tdv_ppf_model_info* info, int nt, const PpfPlan& plan) {
    return info && ppf_model_ptr_ok(d_model) && info->nt == nt && info->n_keys == plan.n_keys && info->n_pairs >= 0 &&
           (size_t)info->n_pairs <= plan.cap && std::isfinite(info->diameter) && info->diameter >= 0.f && std::isfinite(info->distance_step) &&
           info->distance_step >= 0.f;
}
int tdv_ppf_model_dev(tdv_ctx* ctx, const float* d_tgt, const float* d_tgt_normals, int nt, const tdv_ppf_params* params, void* d_model,
                      size_t model_bytes, tdv_ppf_model_info* info) {
    PpfPlan plan;
    if (!ctx || !info || !ppf_plan(params, nt, &plan) || (nt > 0 && (!d_tgt || !d_tgt_normals)) || !ppf_model_ptr_ok(d_model) ||
        model_bytes < plan.bytes)
        return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    return ppf_model_run(ctx, d_tgt, d_tgt_normals, nt, *params, plan, d_model, info);
}
int tdv_ppf_match_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, int ns, const float* d_tgt, const float* d_tgt_normals, int nt,
                      const void* d_model, const tdv_ppf_model_info* info, float thr, const tdv_ppf_params* params, tdv_ppf_pose* out_poses,
                      int* n_poses, tdv_ppf_peak* d_peaks, int* n_ref) {
    PpfPlan plan;
    if (!ppf_match_args_ok(ctx, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, thr, params, out_poses, n_poses, &plan)) return TDV_ERR_BAD_ARG;
    if (!ppf_model_info_ok(d_model, info, nt, plan)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    return ppf_match_run(ctx, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, d_model, *info, thr, *params, plan, out_poses, n_poses, d_peaks,
                         nullptr, n_ref);
}
int tdv_ppf_match_batch_dev(tdv_ctx* ctx, const float* d_src, const float* d_src_normals, const int* h_src_offsets, int n_instances, const float* d_tgt,
                            const float* d_tgt_normals, int nt, const void* d_model, const tdv_ppf_model_info* info, float thr,
                            const tdv_ppf_params* params, tdv_ppf_pose* out_poses, int* n_poses, tdv_ppf_peak* d_peaks, int* h_peak_offsets) {
    PpfPlan plan;
    if (n_instances < 0 || (n_instances > 0 && !h_src_offsets)) return TDV_ERR_BAD_ARG;
    if (n_instances > 0 && h_src_offsets[0] != 0) return TDV_ERR_BAD_ARG;
    for (int b = 0; b < n_instances; ++b)
        if (h_src_offsets[b + 1] < h_src_offsets[b]) return TDV_ERR_BAD_ARG;
    const int ns = n_instances > 0 ? h_src_offsets[n_instances] : 0;
    if (!ppf_match_args_ok(ctx, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, thr, params, out_poses, n_poses, &plan)) return TDV_ERR_BAD_ARG;
    if (!ppf_model_info_ok(d_model, info, nt, plan)) return TDV_ERR_BAD_ARG;
    if ((long long)n_instances * params->max_poses > INT_MAX) return TDV_ERR_BAD_ARG;
    std::vector<int> ref_off((size_t)n_instances + 1, 0);            // rule 5's n_ref per instance, summed
    long long sum = 0;
    for (int b = 0; b < n_instances; ++b) {
        const long long n = h_src_offsets[b + 1] - h_src_offsets[b];
        sum += (n + params->ref_stride - 1) / params->ref_stride;
        if (sum > INT_MAX) return TDV_ERR_BAD_ARG;
        ref_off[(size_t)b + 1] = (int)sum;
    }
    TDV_TRY(begin(ctx));
    return ppf_match_batch_run(ctx, d_src, d_src_normals, h_src_offsets, ref_off.data(), n_instances, d_tgt, d_tgt_normals, nt, d_model, *info, thr,
                               *params, plan, out_poses, n_poses, d_peaks, h_peak_offsets);
}
int tdv_ppf_match(tdv_ctx* ctx, const float* src, const float* src_normals, int ns, const float* tgt, const float* tgt_normals, int nt, float thr,
                  const tdv_ppf_params* params, tdv_ppf_pose* out_poses, int* n_poses, tdv_ppf_peak* peaks, int* n_ref) {
    PpfPlan plan;
    if (!ppf_match_args_ok(ctx, src, src_normals, ns, tgt, tgt_normals, nt, thr, params, out_poses, n_poses, &plan)) return TDV_ERR_BAD_ARG;
    TDV_TRY(begin(ctx));
    float *d_src, *d_sn, *d_tgt, *d_tn;
    TDV_TRY(upload(ctx, src, (size_t)ns * 3, &d_src));
    TDV_TRY(upload(ctx, src_normals, (size_t)ns * 3, &d_sn));
    TDV_TRY(upload(ctx, tgt, (size_t)nt * 3, &d_tgt));
    TDV_TRY(upload(ctx, tgt_normals, (size_t)nt * 3, &d_tn));
    void* d_model;
    TDV_TRY(ws_alloc_bytes(ctx, plan.bytes, &d_model));
    tdv_ppf_model_info info;
    TDV_TRY(ppf_model_run(ctx, d_tgt, d_tn, nt, *params, plan, d_model, &info));
    return ppf_match_run(ctx, d_src, d_sn, ns, d_tgt, d_tn, nt, d_model, info, thr, *params, plan, out_poses, n_poses, nullptr, peaks, n_ref);
}

}  // extern "C"
