"""3dvision_amd — MI355X (gfx950) point-cloud registration backend.

Python front end over the C ABI of ``include/tdv_hip.h`` (``lib3dvision_hip.so``, hand-written
HIP).  It mirrors the reference's operator API so that tests read like calls into the reference:

    reference (C++, namespace industry_picking)           here
    ------------------------------------------------      -----------------------------------
    PointCloud / FPFHFeatures / RegistrationResult        PointCloud / ndarray[n,33] / RegistrationResult
    GPUDepth::preprocess, ::isCudaAvailable               GPUDepth.preprocess, .isCudaAvailable
    GPUPointCloud::generate                               GPUPointCloud.generate
    GPURegistration::icpRefine                            GPURegistration.icpRefine
    Registration::voxelDownsample / estimateNormals /     Registration.voxelDownsample / ...
      computeFPFH / ransacRegistration / icpRefine

(include/gpu_depth.hpp:9-22, include/gpu_registration.hpp:8-19, include/registration.hpp:10-60 of the
reference).  The package directory name starts with a digit, so import it with
``importlib.import_module("3dvision_amd")``.

There is NO CPU fallback: every operator calls the HIP library and raises if the library or a GPU
is missing (``isCudaAvailable()`` is the only call that answers without one).  4x4 transforms are
ordinary row-major ``[4,4]`` numpy arrays at this level; the column-major ``float[16]`` of
``Eigen::Matrix4f::data()`` is the ABI's layout and is converted here.
"""
import ctypes as C
import os
import sys
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TDV_LIB_VARIANT=study (tests marked `study`, tools/studies): the -DTDV_STUDY build, which keeps the A/B variants that lost their
# measurement and the tuning knobs (csrc/tdv_internal.hpp: study_env).  Anything else: the product library.
STUDY_BUILD = os.environ.get("TDV_LIB_VARIANT") == "study"
LIB_PATH = os.path.join(_HERE, "lib3dvision_hip_study.so" if STUDY_BUILD else "lib3dvision_hip.so")

TDV_MASK_THRESHOLD10 = 0
TDV_MASK_NONZERO = 1
TDV_MASK_LABEL_BASE = 256
TDV_VOXEL_ORDER_FIRST = 0
TDV_VOXEL_ORDER_REFERENCE = 1
TIMER_ICP_NN, TIMER_RANSAC_SCORE, TIMER_FEATURE_MATCH, TIMER_KNN, TIMER_RADIUS, TIMER_DEPTH, TIMER_VOXEL, TIMER_FM_INDEX = range(8)
DEPTH_BATCH_MASK_PASSES = 1   # the B masks cross HBM once in tdv_depth_to_cloud_batch_dev (SURVEY.md 8d's minimum): algorithmic bytes of that op

# every symbol include/tdv_hip.h declares (checked by the CPU test-suite against the built library)
ABI_SYMBOLS = [
    "tdv_device_count", "tdv_ctx_create", "tdv_ctx_set_stream", "tdv_ctx_set_icp_search", "tdv_ctx_set_icp_accumulation", "tdv_ctx_last_icp_search", "tdv_ctx_last_batch_lanes", "tdv_ctx_last_voxel_grouping", "tdv_ctx_last_voxel_batch_redone", "tdv_ctx_last_feature_match_path", "tdv_ctx_workspace_bytes", "tdv_ctx_workspace_fill", "tdv_ctx_set_ransac_score", "tdv_ctx_set_ransac_leaf_order", "tdv_ctx_set_ransac_triples", "tdv_ctx_last_ransac_staged", "tdv_ctx_last_ransac_rescore", "tdv_ctx_last_ransac_scored", "tdv_ctx_last_ransac_bound", "tdv_ctx_get_stream", "tdv_ctx_synchronize",
    "tdv_ctx_destroy", "tdv_status_string", "tdv_last_error", "tdv_version", "tdv_timing_enable", "tdv_timing_read",
    "tdv_depth_preprocess", "tdv_deproject", "tdv_depth_to_cloud", "tdv_voxel_downsample", "tdv_estimate_normals",
    "tdv_compute_fpfh", "tdv_feature_match", "tdv_ransac", "tdv_icp", "tdv_icp_correspondences",
    "tdv_icp_dev", "tdv_ransac_dev", "tdv_feature_match_dev", "tdv_estimate_normals_dev", "tdv_compute_fpfh_dev", "tdv_normals_fpfh_dev", "tdv_radix_sort_pairs_dev",
    "tdv_depth_to_cloud_dev", "tdv_voxel_downsample_dev", "tdv_sample_triples", "tdv_sample_triples_batch", "tdv_pose_compose",
    "tdv_register_batch_dev", "tdv_prepare_model_dev", "tdv_bilateral_filter", "tdv_filter_duplicates", "tdv_ransac_score_unit", "tdv_ransac_score_unit_block", "tdv_ransac_score_unit_chunks", "tdv_ransac_batch_size", "tdv_voxel_rules", "tdv_load_ply_ascii", "tdv_load_mask_png", "tdv_load_masks_from_dir",
    "tdv_depth_to_cloud_batch_dev", "tdv_broadcast_model", "tdv_gather_results", "tdv_mask_resize_nearest", "tdv_mask_resize_nearest_dev", "tdv_voxel_downsample_batch_dev", "tdv_voxel_downsample_batch_pinhole_dev",
    "tdv_icp_batch_dev", "tdv_refine_batch_dev", "tdv_ctx_set_icp_loss", "tdv_ctx_get_icp_loss",
    "tdv_gicp", "tdv_gicp_dev", "tdv_gicp_batch_dev",
    "tdv_color_gradients", "tdv_color_gradients_dev", "tdv_colored_icp", "tdv_colored_icp_dev", "tdv_colored_icp_batch_dev",
    "tdv_fgr_default_params", "tdv_fgr", "tdv_fgr_dev", "tdv_fgr_correspondences",
    "tdv_plane_default_params", "tdv_segment_planes", "tdv_segment_planes_dev",
    "tdv_cluster_default_params", "tdv_cluster_dbscan", "tdv_cluster_dbscan_dev",
    "tdv_remove_statistical_outlier", "tdv_remove_statistical_outlier_dev", "tdv_remove_radius_outlier", "tdv_remove_radius_outlier_dev",
    "tdv_iss_default_params", "tdv_iss_keypoints", "tdv_iss_keypoints_dev",
    "tdv_ppf_default_params", "tdv_ppf_model_bytes", "tdv_ppf_model_dev", "tdv_ppf_match_dev", "tdv_ppf_match",
    "tdv_ppf_match_batch_dev",
    "tdv_farthest_point_down_sample", "tdv_farthest_point_down_sample_dev", "tdv_farthest_point_down_sample_batch_dev",
    "tdv_ctx_set_fps_path", "tdv_ctx_last_fps_path", "tdv_ctx_set_icp_launches", "tdv_ctx_last_icp_launches",
    "tdv_ctx_set_icp_probe_cache", "tdv_ctx_last_icp_probe_misses",
    "tdv_verify_default_params", "tdv_verify_poses", "tdv_verify_poses_dev", "tdv_render_depth", "tdv_render_depth_dev",
    "tdv_mesh_verify_default_params", "tdv_verify_poses_mesh", "tdv_verify_poses_mesh_dev", "tdv_render_depth_mesh", "tdv_render_depth_mesh_dev",
    "tdv_mesh_sample_default_params", "tdv_mesh_sample_points", "tdv_mesh_sample_points_dev",
    "tdv_tsdf_default_params", "tdv_tsdf_volume_bytes", "tdv_tsdf_reset_dev", "tdv_tsdf_integrate_dev", "tdv_tsdf_extract_dev", "tdv_tsdf_fuse",
    "tdv_tsdf_extract_mesh_dev", "tdv_tsdf_fuse_mesh",
    "tdv_tsdf_color_bytes", "tdv_tsdf_color_reset_dev", "tdv_tsdf_integrate_color_dev", "tdv_tsdf_extract_color_dev",
    "tdv_tsdf_extract_mesh_color_dev", "tdv_tsdf_raycast_color_dev", "tdv_tsdf_fuse_color",
    "tdv_odometry_default_params", "tdv_depth_maps_dev", "tdv_depth_maps", "tdv_depth_odometry_terms_dev", "tdv_depth_odometry_dev",
    "tdv_depth_odometry", "tdv_depth_odometry_sequence_dev", "tdv_depth_odometry_to_depth_dev", "tdv_depth_odometry_to_depth",
    "tdv_tsdf_raycast_default_params", "tdv_tsdf_raycast_dev", "tdv_tsdf_raycast", "tdv_tsdf_track_dev", "tdv_tsdf_track_sequence_dev",
    "tdv_voxel_downsample_normals", "tdv_voxel_downsample_normals_dev",
    "tdv_icp_level_default", "tdv_icp_multiscale", "tdv_icp_multiscale_dev", "tdv_icp_multiscale_batch_dev",
]


class TdvError(RuntimeError):
    pass


class RansacResultC(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_float), ("rmse", C.c_float), ("inliers", C.c_int),
                ("best_iteration", C.c_int), ("iterations_run", C.c_int)]


class BatchParamsC(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("scale_to_meters", C.c_float), ("mask_mode", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("zmax", C.c_float),
                ("voxel_size", C.c_float), ("normals_k", C.c_int), ("fpfh_radius_factor", C.c_float),
                ("ransac_max_iterations", C.c_int), ("ransac_confidence", C.c_float), ("icp_distance_factor", C.c_float),
                ("icp_max_iterations", C.c_int), ("point_to_plane", C.c_int), ("seed", C.c_uint32),
                ("voxel_order", C.c_int), ("n_frames", C.c_int), ("frame_of_instance", C.c_void_p),
                ("mask_format", C.c_int), ("mask_width", C.c_int), ("mask_height", C.c_int)]


class InstanceResultC(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_float), ("rmse", C.c_float), ("coarse_fitness", C.c_float),
                ("coarse_inliers", C.c_int), ("icp_iterations", C.c_int), ("n_points", C.c_int), ("n_voxels", C.c_int),
                ("status", C.c_int)]


class IcpResultC(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_float), ("rmse", C.c_float), ("iterations", C.c_int),
                ("n_corr", C.c_int)]


class IcpLevelC(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("max_correspondence_distance", C.c_float), ("max_iterations", C.c_int),
                ("relative_fitness", C.c_float), ("relative_rmse", C.c_float)]


class IcpLevelResultC(C.Structure):
    _fields_ = [("icp", IcpResultC), ("ns", C.c_int), ("nt", C.c_int)]


TDV_ICP_MAX_LEVELS = 8
TDV_ICP_POINT_TO_PLANE, TDV_ICP_POINT_TO_POINT, TDV_ICP_GICP = 0, 1, 3
ICP_ESTIMATION = {"point_to_plane": TDV_ICP_POINT_TO_PLANE, "point_to_point": TDV_ICP_POINT_TO_POINT, "gicp": TDV_ICP_GICP}


def icp_levels(voxel_sizes, max_correspondence_distances, max_iterations=None, relative_fitness=None, relative_rmse=None):
    """The tdv_icp_level array of a multi-scale schedule (include/tdv_hip.h: tdv_icp_multiscale).  voxel_sizes sets the number of levels
    (a voxel size of None or <= 0, last level only: the clouds as given); the other arguments are one value per level or a scalar for
    all of them, None: the library's default (tdv_icp_level_default: 30 iterations, relative_fitness inf, relative_rmse 1e-6)."""
    voxels = [-1.0 if v is None else float(v) for v in (voxel_sizes if isinstance(voxel_sizes, (list, tuple, np.ndarray)) else [voxel_sizes])]
    n = len(voxels)

    def per_level(x, name):
        if x is None:
            return [None] * n
        x = list(np.atleast_1d(x))
        if len(x) == 1:
            x = x * n
        if len(x) != n:
            raise ValueError("icp_levels: %s has %d values for %d levels" % (name, len(x), n))
        return x
    dist = per_level(max_correspondence_distances, "max_correspondence_distances")
    its = per_level(max_iterations, "max_iterations")
    rf = per_level(relative_fitness, "relative_fitness")
    rr = per_level(relative_rmse, "relative_rmse")
    levels = (IcpLevelC * max(n, 1))()
    for l in range(n):
        lib().tdv_icp_level_default(C.byref(levels[l]))
        levels[l].voxel_size = voxels[l]
        if dist[l] is not None:
            levels[l].max_correspondence_distance = float(dist[l])
        if its[l] is not None:
            levels[l].max_iterations = int(its[l])
        if rf[l] is not None:
            levels[l].relative_fitness = float(rf[l])
        if rr[l] is not None:
            levels[l].relative_rmse = float(rr[l])
    levels.n_levels = n
    return levels


def _params(stage, kw):
    """The parameter struct of a stage (_PARAMS below), filled by the library's tdv_*_default_params, with the fields in kw replaced."""
    struct, default_fn_name, label, names = _PARAMS[stage]
    p = struct()
    getattr(lib(), default_fn_name)(C.byref(p))
    fields = dict(struct._fields_)
    for k, v in kw.items():
        if k not in fields:
            raise TypeError("unknown %s parameter %r" % (label, k))
        setattr(p, k, names[k][v] if names and k in names and isinstance(v, str) else v)
    return p


def _fields_dict(r):
    """A result struct as a dict of its fields."""
    return {k: getattr(r, k) for k, _ in r._fields_}


class FgrParamsC(C.Structure):
    _fields_ = [("division_factor", C.c_float), ("maximum_correspondence_distance", C.c_float), ("tuple_scale", C.c_float),
                ("iteration_number", C.c_int), ("maximum_tuple_count", C.c_int), ("use_absolute_scale", C.c_int),
                ("decrease_mu", C.c_int), ("tuple_test", C.c_int), ("seed", C.c_uint32)]


class FgrResultC(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_float), ("rmse", C.c_float), ("inliers", C.c_int), ("n_mutual", C.c_int),
                ("n_tuple", C.c_int), ("degenerate", C.c_int), ("trials_run", C.c_longlong)]


def fgr_params(**kw):
    """tdv_fgr_default_params with the given fields replaced (Open3D's FastGlobalRegistrationOption names)."""
    return _params("fgr", kw)


TDV_PLANE_CHUNK = 1024
TDV_PLANE_MAX = 16


class PlaneParamsC(C.Structure):
    _fields_ = [("probability", C.c_double), ("distance_threshold", C.c_float), ("num_iterations", C.c_int), ("max_planes", C.c_int),
                ("min_inliers", C.c_int), ("refit", C.c_int), ("seed", C.c_uint32)]


class PlaneResultC(C.Structure):
    _fields_ = [("plane", C.c_float * 4), ("hypothesis", C.c_float * 4), ("fitness", C.c_float), ("rmse", C.c_float),
                ("inliers", C.c_int), ("candidates", C.c_int), ("best_iteration", C.c_int), ("iterations_run", C.c_int)]


def plane_params(**kw):
    """tdv_plane_default_params with the given fields replaced (Open3D's segment_plane names, plus max_planes, min_inliers, refit, seed)."""
    return _params("plane", kw)


def _plane_results(res, n):
    return [dict(plane=np.array(r.plane[:], np.float32), hypothesis=np.array(r.hypothesis[:], np.float32), fitness=np.float32(r.fitness),
                 rmse=np.float32(r.rmse), inliers=r.inliers, candidates=r.candidates, best_iteration=r.best_iteration,
                 iterations_run=r.iterations_run) for r in res[:n]]


class ClusterParamsC(C.Structure):
    _fields_ = [("eps", C.c_float), ("min_points", C.c_int), ("min_cluster_size", C.c_int)]


class ClusterResultC(C.Structure):
    _fields_ = [("n_clusters", C.c_int), ("n_core", C.c_int), ("n_border", C.c_int), ("n_noise", C.c_int), ("n_dropped", C.c_int),
                ("largest", C.c_int)]


def cluster_params(**kw):
    """tdv_cluster_default_params (min_cluster_size = 1; eps and min_points have no default) with the given fields replaced."""
    return _params("cluster", kw)


class OutlierResultC(C.Structure):
    _fields_ = [("n_valid", C.c_int), ("n_kept", C.c_int), ("cloud_mean", C.c_double), ("std_dev", C.c_double), ("threshold", C.c_double)]


class IssParamsC(C.Structure):
    _fields_ = [("salient_radius", C.c_float), ("non_max_radius", C.c_float), ("gamma_21", C.c_double), ("gamma_32", C.c_double),
                ("min_neighbors", C.c_int)]


class IssResultC(C.Structure):
    _fields_ = [("n_finite", C.c_int), ("n_supported", C.c_int), ("n_salient", C.c_int), ("n_keypoints", C.c_int),
                ("salient_radius", C.c_float), ("non_max_radius", C.c_float), ("resolution", C.c_double)]


def iss_params(**kw):
    """tdv_iss_default_params (radii 0: from the cloud's resolution; gammas 0.975; min_neighbors 5) with the given fields replaced
    (Open3D's compute_iss_keypoints names)."""
    return _params("iss", kw)


TDV_FPS_MAX_POINTS = 1 << 22
TDV_FPS_WORKGROUP_LANES = 1024
TDV_FPS_WORKGROUP_MAX = 16384
TDV_FPS_AUTO, TDV_FPS_WORKGROUP, TDV_FPS_GRID = 0, 1, 2
FPS_PATH = {"auto": TDV_FPS_AUTO, "workgroup": TDV_FPS_WORKGROUP, "grid": TDV_FPS_GRID}


class FpsResultC(C.Structure):
    _fields_ = [("n_usable", C.c_int), ("n_selected", C.c_int), ("path", C.c_int), ("cover_d2", C.c_float)]


def _fps_result(r):
    return dict(n_usable=r.n_usable, n_selected=r.n_selected, path=r.path, cover_d2=np.float32(r.cover_d2))


TDV_POSE_SOURCE_ONTO_TARGET, TDV_POSE_MODEL_TO_CAMERA = 0, 1
TDV_VERIFY_MAX_SPLAT = 3
TDV_VERIFY_MAX_MODEL = 1 << 22
TDV_VERIFY_MAX_POSES = 65536
TDV_VERIFY_MAX_SIDE = 8192
TDV_VERIFY_TILE_W = 128
TDV_VERIFY_TILE_H = 128
TDV_VERIFY_LANES = 1024
POSE_DIRECTION = {"source_onto_target": TDV_POSE_SOURCE_ONTO_TARGET, "model_to_camera": TDV_POSE_MODEL_TO_CAMERA}


class VerifyParamsC(C.Structure):
    _fields_ = [("pose_direction", C.c_int), ("splat", C.c_int), ("tau", C.c_float), ("zmax", C.c_float)]


class VerifyResultC(C.Structure):
    _fields_ = [("n_projected", C.c_int), ("n_rendered", C.c_int), ("n_consistent", C.c_int), ("n_occluded", C.c_int),
                ("n_violating", C.c_int), ("n_unknown", C.c_int), ("err_q20", C.c_ulonglong)]


def verify_params(**kw):
    """tdv_verify_default_params (T moves the camera's cloud onto the model, splat 1, tau 0.002 m, zmax 10 m) with the given fields replaced;
    pose_direction also by name ('source_onto_target', 'model_to_camera')."""
    return _params("verify", kw)


def _verify_results(res, n):
    """One dict of ints per pose.  The names are taken once: a call converts hundreds of records, a third of a device call's time."""
    names = [k for k, _ in VerifyResultC._fields_]
    return [{k: int(getattr(r, k)) for k in names} for r in res[:n]]


TDV_MESH_CULL_NONE, TDV_MESH_CULL_BACK = 0, 1
TDV_MESH_MAX_VERTICES = 1 << 22
TDV_MESH_MAX_TRIANGLES = 1 << 22
TDV_MESH_SUBPIXEL = 16
TDV_MESH_COOP_PIXELS = 64
TDV_MESH_QUEUE = 128
MESH_CULL = {"none": TDV_MESH_CULL_NONE, "back": TDV_MESH_CULL_BACK}


class MeshVerifyParamsC(C.Structure):
    _fields_ = [("pose_direction", C.c_int), ("cull", C.c_int), ("tau", C.c_float), ("zmax", C.c_float)]


def mesh_verify_params(**kw):
    """tdv_mesh_verify_default_params (T moves the camera's cloud onto the model, no culling, tau 0.002 m, zmax 10 m) with the given fields
    replaced; pose_direction and cull also by name ('source_onto_target', 'model_to_camera'; 'none', 'back')."""
    return _params("mesh_verify", kw)


def _mesh(vertices, triangles):
    return _f32(vertices).reshape(-1, 3), np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)


TDV_MESH_SAMPLE_MAX = 1 << 24


class MeshSampleParamsC(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("first_sample", C.c_uint64)]


class MeshSampleResultC(C.Structure):
    _fields_ = [("n_usable", C.c_int), ("n_degenerate", C.c_int), ("n_bad", C.c_int), ("n_sampled", C.c_int), ("weight_exponent", C.c_int),
                ("area_max", C.c_float), ("total_weight", C.c_uint64)]


def mesh_sample_params(**kw):
    """tdv_mesh_sample_default_params (seed 0, first_sample 0) with the given fields replaced."""
    return _params("mesh_sample", kw)


def _mesh_sample_result(r):
    """The result as a dict, with surface_area = ldexp(total_weight, weight_exponent - 31) (include/tdv_hip.h: one rounding)."""
    import math
    return dict(n_usable=r.n_usable, n_degenerate=r.n_degenerate, n_bad=r.n_bad, n_sampled=r.n_sampled, weight_exponent=r.weight_exponent,
                area_max=np.float32(r.area_max), total_weight=int(r.total_weight),
                surface_area=math.ldexp(float(int(r.total_weight)), r.weight_exponent - 31))


TDV_TSDF_MAX_SIDE = 1024
TDV_TSDF_MAX_VOXELS = 1 << 27
TDV_TSDF_HOST_MAX_VOXELS = 1 << 25
TDV_TSDF_MAX_FRAMES = 64
TDV_TSDF_TILE_X, TDV_TSDF_TILE_Y, TDV_TSDF_TILE_Z = 64, 8, 8
TDV_TSDF_MC_MAX_TRIANGLES = 5


class TsdfVolumeC(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_length", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int)]


class TsdfParamsC(C.Structure):
    _fields_ = [("trunc", C.c_float), ("max_weight", C.c_float), ("zmax", C.c_float), ("min_weight", C.c_float), ("pose_direction", C.c_int)]


def tsdf_params(**kw):
    """tdv_tsdf_default_params (trunc 0: four voxel lengths, max_weight 255, zmax 10 m, min_weight 1, poses take the volume's frame to the
    camera's) with the given fields replaced; pose_direction also by name ('model_to_camera', 'source_onto_target')."""
    return _params("tsdf", kw)


def tsdf_volume_struct(origin, voxel_length, dims):
    """The tdv_tsdf_volume of a grid of dims = (nx, ny, nz) voxels of voxel_length metres whose corner (not first centre) is origin."""
    o = np.asarray(origin, np.float32).reshape(3)
    return TsdfVolumeC((C.c_float * 3)(*[float(x) for x in o]), float(np.float32(voxel_length)), int(dims[0]), int(dims[1]), int(dims[2]))


TDV_ODOM_MAX_LEVELS = 4
ODOM_TERMS = 29   # O7's sums: 1, d2, 21 + 6


class OdometryParamsC(C.Structure):
    _fields_ = [("depth_diff", C.c_float), ("zmax", C.c_float), ("n_levels", C.c_int), ("max_iterations", C.c_int * TDV_ODOM_MAX_LEVELS)]


class OdometryResultC(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_float), ("rmse", C.c_float), ("n_corr", C.c_int),
                ("iterations", C.c_int * TDV_ODOM_MAX_LEVELS), ("n_corr_level", C.c_int * TDV_ODOM_MAX_LEVELS)]


def odometry_params(**kw):
    """tdv_odometry_default_params (depth_diff 0.03 m, zmax 10 m, 3 levels, 20 / 10 / 5 / 0 iterations on levels 0 to 3) with the given
    fields replaced; max_iterations as a sequence of up to TDV_ODOM_MAX_LEVELS ints, level 0 first (the rest 0)."""
    kw = dict(kw)
    its = kw.pop("max_iterations", None)
    p = _params("odometry", kw)
    if its is not None:
        its = [int(x) for x in its]
        if len(its) > TDV_ODOM_MAX_LEVELS:
            raise ValueError("max_iterations: at most TDV_ODOM_MAX_LEVELS entries")
        p.max_iterations = (C.c_int * TDV_ODOM_MAX_LEVELS)(*(its + [0] * (TDV_ODOM_MAX_LEVELS - len(its))))
    return p


def _odometry_result(r):
    """A tdv_odometry_result as a dict: T row-major [4, 4], fitness and rmse as float32, the per-level lists."""
    return dict(T=from_colmajor16(r.T), fitness=np.float32(r.fitness), rmse=np.float32(r.rmse), n_corr=int(r.n_corr),
                iterations=list(r.iterations), n_corr_level=list(r.n_corr_level))


TDV_TSDF_RAYCAST_MAX_STEPS = 16384


class TsdfRaycastParamsC(C.Structure):
    _fields_ = [("zmin", C.c_float), ("max_steps", C.c_int)]


class TsdfTrackResultC(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("odom", OdometryResultC), ("n_hit", C.c_longlong)]


def raycast_params(**kw):
    """tdv_tsdf_raycast_default_params (zmin 0.05 m, max_steps 4096) with the given fields replaced."""
    return _params("raycast", kw)


def _track_result(r):
    """A tdv_tsdf_track_result as a dict: pose row-major [4, 4], odom as _odometry_result's dict, n_hit."""
    return dict(pose=from_colmajor16(r.pose), odom=_odometry_result(r.odom), n_hit=int(r.n_hit))


def _split_params(kw, *stages):
    """kw split by the parameter struct each name belongs to, in the order of `stages` (a name two stages share - zmax - goes to
    every one of them): one dict per stage.  An unknown name raises TypeError."""
    fields = [dict(_PARAMS[s][0]._fields_) for s in stages]
    out = [dict() for _ in stages]
    for k, v in kw.items():
        hit = [i for i, f in enumerate(fields) if k in f]
        if not hit:
            raise TypeError("unknown parameter %r (stages: %s)" % (k, ", ".join(stages)))
        for i in hit:
            out[i][k] = v
    return out


def mesh_compact(vertices, normals, triangles):
    """The mesh without the vertices no triangle refers to: the kept rows in their order, the triangles renumbered (numpy, on the host)."""
    triangles = np.asarray(triangles, np.int32).reshape(-1, 3)
    used = np.zeros(len(vertices), bool)
    used[triangles.reshape(-1)] = True
    new = (np.cumsum(used) - 1).astype(np.int32)
    return vertices[used], (None if normals is None else normals[used]), new[triangles].reshape(-1, 3)


def _colored_mesh(vertices, normals, triangles, rgb, compact):
    """(vertices, normals, triangles, rgb); compact: mesh_compact, the colours of the dropped vertices dropped with them."""
    if not compact:
        return vertices, normals, triangles, rgb
    used = np.zeros(len(vertices), bool)
    used[np.asarray(triangles, np.int32).reshape(-1)] = True
    return mesh_compact(vertices, normals, triangles) + (rgb[used],)


def _poses16(poses):
    """[n, 4, 4] row-major poses as the ABI's n x 16 column-major floats."""
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    return np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(-1), len(poses)


TDV_PPF_MODEL_MAX = 2048
TDV_PPF_POSES_MAX = 64
TDV_PPF_KEYS_MAX = 1 << 24
TDV_PPF_LDS_CELLS = 39000


class PpfParamsC(C.Structure):
    _fields_ = [("distance_step_relative", C.c_float), ("angle_bins", C.c_int), ("rotation_bins", C.c_int), ("ref_stride", C.c_int),
                ("max_poses", C.c_int), ("cluster_translation_relative", C.c_float), ("cluster_rotation", C.c_float),
                ("flip_model_normals", C.c_int)]


class PpfModelInfoC(C.Structure):
    _fields_ = [("diameter", C.c_float), ("distance_step", C.c_float), ("n_pairs", C.c_int), ("n_keys", C.c_int), ("nt", C.c_int)]


class PpfPoseC(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_float), ("rmse", C.c_float), ("n_corr", C.c_int), ("votes", C.c_int),
                ("members", C.c_int), ("ref", C.c_int), ("model_index", C.c_int), ("bin", C.c_int)]


PPF_PEAK_DTYPE = np.dtype([("ref", np.int32), ("model_index", np.int32), ("bin", np.int32), ("votes", np.int32)])


def ppf_params(**kw):
    """tdv_ppf_default_params (step 0.05 of the diameter, 30 angle and 30 rotation bins, ref_stride 5, 8 poses, clusters within 0.1 of the
    diameter and 2 pi / 30) with the given fields replaced."""
    return _params("ppf", kw)


def _ppf_poses(poses, n):
    """The poses of a PPF call: RegistrationResults, and one dict per pose with what they have no field for."""
    res = [RegistrationResult(transformation=from_colmajor16(q.T), fitness=np.float32(q.fitness), rmse=np.float32(q.rmse), n_corr=q.n_corr)
           for q in poses[:n]]
    return res, [dict(votes=q.votes, members=q.members, ref=q.ref, model_index=q.model_index, bin=q.bin) for q in poses[:n]]


# The stages with a parameter struct: the struct, the library's function that fills in its defaults, the stage's name in the TypeError
# of an unknown field, and per field the strings that stand for its values.  _params builds the struct from a row, and lib() declares
# every row's function as returning nothing: a new stage is one row here.
_PARAMS = {
    "fgr": (FgrParamsC, "tdv_fgr_default_params", "FGR", None),
    "plane": (PlaneParamsC, "tdv_plane_default_params", "plane", None),
    "cluster": (ClusterParamsC, "tdv_cluster_default_params", "cluster", None),
    "iss": (IssParamsC, "tdv_iss_default_params", "ISS", None),
    "verify": (VerifyParamsC, "tdv_verify_default_params", "verification", dict(pose_direction=POSE_DIRECTION)),
    "mesh_verify": (MeshVerifyParamsC, "tdv_mesh_verify_default_params", "mesh verification",
                    dict(pose_direction=POSE_DIRECTION, cull=MESH_CULL)),
    "mesh_sample": (MeshSampleParamsC, "tdv_mesh_sample_default_params", "mesh sampling", None),
    "ppf": (PpfParamsC, "tdv_ppf_default_params", "PPF", None),
    "tsdf": (TsdfParamsC, "tdv_tsdf_default_params", "TSDF", dict(pose_direction=POSE_DIRECTION)),
    "odometry": (OdometryParamsC, "tdv_odometry_default_params", "odometry", None),
    "raycast": (TsdfRaycastParamsC, "tdv_tsdf_raycast_default_params", "ray cast", None),
}

_lib = None
_lib_lock = threading.Lock()


def build():
    """Compile the HIP library in-tree (hipcc cross-compiles for gfx950 without a GPU)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tdv_build", os.path.join(_HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build()


def lib():
    """The loaded C-ABI library.  Raises (never falls back) when it has not been built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise TdvError("lib3dvision_hip.so is not built (%s). Run `python 3dvision_amd/build.py` or "
                               "__graft_entry__.build(); there is no CPU fallback." % LIB_PATH)
            # A process that will also use torch must load torch FIRST: its wheel brings its own copy of the HIP runtime, and once the system's
            # copy (this library's dependency) has initialised the device, torch's reports "No HIP GPUs are available".  The harness around
            # this package (tests, bench.py, tools) always uses torch for device buffers, so it is imported here when it is installed.
            if "torch" not in sys.modules:
                try:
                    import torch  # noqa: F401
                except ImportError:
                    pass
            l = C.CDLL(LIB_PATH)
            l.tdv_status_string.restype = C.c_char_p
            l.tdv_last_error.restype = C.c_char_p
            l.tdv_version.restype = C.c_char_p
            l.tdv_ctx_get_stream.restype = C.c_void_p
            l.tdv_ctx_workspace_bytes.restype = C.c_ulonglong
            l.tdv_tsdf_volume_bytes.restype = C.c_ulonglong
            l.tdv_tsdf_color_bytes.restype = C.c_ulonglong
            l.tdv_ctx_last_ransac_rescore.restype = C.c_double
            l.tdv_ctx_last_ransac_scored.restype = C.c_double
            l.tdv_ctx_last_ransac_bound.restype = None
            l.tdv_icp_level_default.restype = None
            for _, default_fn_name, _, _ in _PARAMS.values():
                getattr(l, default_fn_name).restype = None
            _lib = l
    return _lib


def _check(ctx, status, what):
    if status != 0:
        msg = lib().tdv_status_string(status).decode()
        detail = lib().tdv_last_error(ctx).decode() if ctx else ""
        raise TdvError("%s: %s (%d) %s" % (what, msg, status, detail))


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def to_colmajor16(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).T).reshape(16)


def from_colmajor16(t):
    return np.array(t, dtype=np.float32).reshape(4, 4).T.copy()


def device_count():
    n = C.c_int(0)
    _check(None, lib().tdv_device_count(C.byref(n)), "tdv_device_count")
    return n.value


@dataclass
class PointCloud:
    """include/registration.hpp:10-19."""
    points: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float32))
    normals: Optional[np.ndarray] = None
    colors: Optional[np.ndarray] = None

    def size(self):
        return len(self.points)

    def empty(self):
        return len(self.points) == 0

    def hasNormals(self):
        return self.normals is not None and len(self.normals) == len(self.points)

    def hasColors(self):
        return self.colors is not None and len(self.colors) == len(self.points)


@dataclass
class RegistrationResult:
    """include/registration.hpp:26-30 (+ diagnostics the ABI also returns)."""
    transformation: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    fitness: float = 0.0
    rmse: float = 0.0
    iterations: int = 0
    inliers: int = 0
    best_iteration: int = -1
    iterations_run: int = 0
    n_corr: int = 0
    trace_inliers: Optional[np.ndarray] = None
    levels: Optional[list] = None     # multi_scale_icp: one IcpLevelResult per level, coarse to fine


@dataclass
class IcpLevelResult(RegistrationResult):
    """One level of a multi-scale ICP call: the level's ICP result and the points of its two clouds."""
    ns: int = 0
    nt: int = 0


def _icp_level_results(res, n_levels, b=0):
    """The n_levels level results of instance b as the RegistrationResult of the last level, with all of them in .levels."""
    levels = []
    for l in range(n_levels):
        r = res[b * n_levels + l]
        levels.append(IcpLevelResult(transformation=from_colmajor16(r.icp.T), fitness=np.float32(r.icp.fitness), rmse=np.float32(r.icp.rmse),
                                     iterations=r.icp.iterations, n_corr=r.icp.n_corr, ns=r.ns, nt=r.nt))
    last = levels[-1]
    return RegistrationResult(transformation=last.transformation.copy(), fitness=last.fitness, rmse=last.rmse, iterations=last.iterations,
                              n_corr=last.n_corr, levels=levels)


def _icp_result(r):
    """An IcpResultC as the RegistrationResult every ICP call returns."""
    return RegistrationResult(transformation=from_colmajor16(r.T), fitness=np.float32(r.fitness), rmse=np.float32(r.rmse),
                              iterations=r.iterations, n_corr=r.n_corr)


def _icp_batch_args(offsets, T0s):
    """What a batch call passes for its instances: the offsets as int32, their count, the start poses column-major back to back and the result array."""
    off = np.ascontiguousarray(offsets, np.int32)
    n = len(off) - 1
    T0s = np.asarray(T0s, np.float32).reshape(-1, 4, 4)
    t0 = np.concatenate([to_colmajor16(T) for T in T0s]) if len(T0s) else np.zeros(0, np.float32)
    return off, n, t0, (IcpResultC * max(n, 1))()


def _instance_rows(arrays):
    """Per-instance host arrays as (n_b, 3) float32, and their offsets."""
    rows = [_f32(a).reshape(-1, 3) for a in arrays]
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a in rows])
    return rows, off


def _upload_rows(device, rows, width=3):
    """Host rows - one (n, width) array, or a list of per-instance arrays back to back - as a torch tensor on `device`; one dummy row
    where there are none, so that the call gets a valid pointer."""
    import torch
    if isinstance(rows, list):
        rows = np.concatenate(rows) if rows else np.zeros((0, width), np.float32)
    return torch.from_numpy(rows if len(rows) else np.zeros((1, width), np.float32)).to(torch.device("cuda", device))


class Context:
    """One tdv_ctx (stream + workspace).  Not thread-safe; one per host thread."""

    def __init__(self, device=0, stream=None):
        self.icp_search_name = "auto"
        self._h = C.c_void_p()
        _check(None, lib().tdv_ctx_create(int(device), C.byref(self._h)), "tdv_ctx_create")
        self.device = device
        if stream is not None:
            _check(self._h, lib().tdv_ctx_set_stream(self._h, C.c_void_p(stream)), "tdv_ctx_set_stream")

    ICP_SEARCH = {"auto": 0, "brute": 1, "pruned": 2, "grid": 3}

    def set_icp_search(self, mode):
        """'auto' (by size and cell occupancy), 'brute' (the reference's scan), 'pruned' (exact box-pruned walk) or 'grid' (hash grid
        with cells of 2.2 x the threshold; falls back to 'pruned' when the threshold is large against the spacing); same results."""
        _check(self._h, lib().tdv_ctx_set_icp_search(self._h, self.ICP_SEARCH[mode]), "tdv_ctx_set_icp_search")
        self.icp_search_name = mode

    def set_icp_accumulation(self, mode):
        """'tree' (default: f64 sums in a fixed tree, transform within tolerance of the CPU path) or 'reference' (f32 sums in
        ascending source index as registration.cpp:340-358,374-386: transform, rmse, fitness and iteration count equal the
        CPU path's bit for bit; a serial chain per iteration)."""
        _check(self._h, lib().tdv_ctx_set_icp_accumulation(self._h, {"tree": 0, "reference": 1}[mode]), "tdv_ctx_set_icp_accumulation")

    ICP_LOSS = {"l2": 0, "huber": 1, "tukey": 2, "cauchy": 3}

    def set_icp_loss(self, kind, scale=None):
        """ICP's robust loss on this context (include/tdv_hip.h: tdv_ctx_set_icp_loss): 'l2' (default: every accepted
        correspondence has weight 1), 'huber', 'tukey' or 'cauchy' with its scale k in metres (finite, > 0; 'l2' ignores it).
        Residuals: point-to-plane (p - q) . n, point-to-point |p - q|.  Refused with reference-order accumulation at call time."""
        if kind not in self.ICP_LOSS:
            raise ValueError("unknown ICP loss %r (one of %s)" % (kind, ", ".join(self.ICP_LOSS)))
        if kind != "l2" and scale is None:
            raise ValueError("the %s loss needs a scale" % kind)
        _check(self._h, lib().tdv_ctx_set_icp_loss(self._h, self.ICP_LOSS[kind], C.c_float(0.0 if scale is None else float(scale))),
               "tdv_ctx_set_icp_loss")

    def icp_loss(self):
        """(kind, scale) of this context's ICP loss; scale is 0.0 for 'l2'."""
        k = C.c_int(); sc = C.c_float()
        _check(self._h, lib().tdv_ctx_get_icp_loss(self._h, C.byref(k), C.byref(sc)), "tdv_ctx_get_icp_loss")
        return {v: n for n, v in self.ICP_LOSS.items()}[k.value], float(sc.value)

    def set_ransac_score(self, mode):
        """'fast' (default: FMA pass, chunks inside the rounding band re-scored with the reference arithmetic) or 'exact'
        (the reference arithmetic only); same inlier counts."""
        _check(self._h, lib().tdv_ctx_set_ransac_score(self._h, {"fast": 0, "exact": 1, "matrix": 2}[mode]), "tdv_ctx_set_ransac_score")

    def set_ransac_leaf_order(self, mode):
        """'auto' (default: class-major leaves for a call with at least 50,000 pairs), 'morton' or 'classes': the order of the
        leaves the leaf-box bound walks; same result, other list lengths."""
        _check(self._h, lib().tdv_ctx_set_ransac_leaf_order(self._h, {"auto": 0, "morton": 1, "classes": 2}[mode]), "tdv_ctx_set_ransac_leaf_order")

    def set_ransac_triples(self, mode):
        """'auto' (default: staged wherever a call can), 'direct' or 'staged': whether a batch's hypothesis kernel reads its index
        triples from the host's pinned memory or finds them on the device, carried there by the batch before; same results."""
        _check(self._h, lib().tdv_ctx_set_ransac_triples(self._h, {"auto": 0, "direct": 1, "staged": 2}[mode]), "tdv_ctx_set_ransac_triples")

    def last_ransac_staged(self):
        """Batches of the last RANSAC call on this context, of those its loop reached, that ran from staged triples."""
        return int(lib().tdv_ctx_last_ransac_staged(self._h))

    def last_ransac_rescore(self):
        """Fraction of the (hypothesis, point) tests the last RANSAC call scored a second time exactly (-1 in 'exact' mode)."""
        return float(lib().tdv_ctx_last_ransac_rescore(self._h))

    def last_ransac_scored(self):
        """Share of the (hypothesis, point) tests the last RANSAC call evaluated (< 1: calls without a trace stop scoring a
        hypothesis that can no longer beat the best count of the earlier batches; same result)."""
        return float(lib().tdv_ctx_last_ransac_scored(self._h))

    def last_ransac_bound(self):
        """(bounded, close, fine, live): over the last RANSAC call's bounded batches, the hypotheses the leaf-box bound saw, those close
        to the running best and live without a walk, those put on the fine level's list, and those live - scored at all."""
        out = (C.c_longlong * 4)()
        lib().tdv_ctx_last_ransac_bound(self._h, out)
        return tuple(int(v) for v in out)

    def last_feature_match_path(self):
        """'scan', 'leaf_major' or 'walk': the search the last feature_match call on this context ran."""
        return {0: "none", 1: "scan", 2: "leaf_major", 3: "walk"}[int(lib().tdv_ctx_last_feature_match_path(self._h))]

    def last_voxel_grouping(self):
        """'table' or 'pixels': how the last batched voxel stage on this context grouped its points."""
        return {0: "none", 1: "table", 2: "pixels"}[int(lib().tdv_ctx_last_voxel_grouping(self._h))]

    def last_voxel_batch_redone(self):
        """Whether the last batched voxel pass on this context (voxel_downsample_batch_dev, a voxelised level of multi_scale_icp_batch_dev)
        was redone cloud by cloud because a voxel held more points than the table's rows: 0 kept, 1 redone, -1 before any."""
        return int(lib().tdv_ctx_last_voxel_batch_redone(self._h))

    def last_batch_lanes(self):
        """Host lanes the last register_batch_dev call on this context used."""
        return int(lib().tdv_ctx_last_batch_lanes(self._h))

    def last_icp_search(self):
        """Name of the search the last ICP / correspondence call ran ('brute', 'pruned', 'grid'; 'auto' before any)."""
        v = lib().tdv_ctx_last_icp_search(self._h)
        return {n: k for k, n in self.ICP_SEARCH.items()}[v]

    ICP_LAUNCHES = {"auto": 0, "two": 1, "one": 2}

    def set_icp_launches(self, mode):
        """'auto' (default: one launch per iteration where it measured faster), 'two' (search, then accumulation) or 'one' (both in one
        kernel, where the path has it: hash grid, tree sums, point-to-plane or point-to-point); same bytes (tests and measurements)."""
        _check(self._h, lib().tdv_ctx_set_icp_launches(self._h, self.ICP_LAUNCHES[mode]), "tdv_ctx_set_icp_launches")

    def last_icp_launches(self):
        """'one' if the last ICP call on this context ran the one-launch iteration, else 'two' ('auto' before any)."""
        return {v: k for k, v in self.ICP_LAUNCHES.items()}[int(lib().tdv_ctx_last_icp_launches(self._h))]

    ICP_PROBE_CACHE = {"auto": 0, "off": 1, "on": 2}

    def set_icp_probe_cache(self, mode):
        """'auto' (default: with the one-launch iteration, when the call may run four iterations or more), 'off' or 'on' (the single
        call's grid search in either launch form, from two iterations on): whether the hash-grid search keeps each source point's probed
        list heads between a call's iterations; same bytes (tests and measurements)."""
        _check(self._h, lib().tdv_ctx_set_icp_probe_cache(self._h, self.ICP_PROBE_CACHE[mode]), "tdv_ctx_set_icp_probe_cache")

    def last_icp_probe_misses(self):
        """(point, iteration) pairs of the last ICP call on this context that probed the hash table; -1 if it ran without the probe cache."""
        return int(lib().tdv_ctx_last_icp_probe_misses(self._h))

    def set_fps_path(self, mode):
        """'auto' (default: the workgroup kernels up to TDV_FPS_WORKGROUP_MAX rows, the grid kernels above), 'workgroup' or 'grid': the
        kernel family of farthest point sampling on this context; same bytes either way (tests and measurements)."""
        _check(self._h, lib().tdv_ctx_set_fps_path(self._h, FPS_PATH[mode]), "tdv_ctx_set_fps_path")

    def last_fps_path(self):
        """'workgroup' or 'grid': the family the last farthest-point call on this context chose ('auto' before any)."""
        return {v: k for k, v in FPS_PATH.items()}[int(lib().tdv_ctx_last_fps_path(self._h))]

    def workspace_high_water(self):
        """Bytes of device memory held by this ctx's workspace arenas (its batch lanes' included): the high-water mark so far."""
        return int(lib().tdv_ctx_workspace_bytes(self._h))

    def workspace_fill(self, byte):
        """Test aid (include/tdv_hip.h: tdv_ctx_workspace_fill): every byte of this ctx's workspace arenas and pinned staging, its batch
        lanes' included, becomes `byte` (0..255).  The persistent ticket and status words are left alone."""
        _check(self._h, lib().tdv_ctx_workspace_fill(self._h, int(byte)), "tdv_ctx_workspace_fill")

    def set_stream(self, handle):
        """Run this ctx's work on the caller's stream `handle` from now on (0 = the null stream, torch.cuda.Stream().cuda_stream, ...);
        the ctx waits for and destroys the stream it made itself, and never destroys the caller's."""
        _check(self._h, lib().tdv_ctx_set_stream(self._h, C.c_void_p(int(handle))), "tdv_ctx_set_stream")

    def close(self):
        if self._h:
            lib().tdv_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().tdv_ctx_get_stream(self._h)

    def synchronize(self):
        _check(self._h, lib().tdv_ctx_synchronize(self._h), "tdv_ctx_synchronize")

    def timing_enable(self, on=True):
        _check(self._h, lib().tdv_timing_enable(self._h, int(on)), "tdv_timing_enable")

    def timing_read(self, slot):
        ms = C.c_double(); n = C.c_int()
        _check(self._h, lib().tdv_timing_read(self._h, slot, C.byref(ms), C.byref(n)), "tdv_timing_read")
        return ms.value, n.value

    # ---------------------------------------------------------------- R1 / R2
    def depth_preprocess(self, raw, mask, scale, mask_mode=TDV_MASK_THRESHOLD10):
        raw = np.ascontiguousarray(raw, np.uint16)
        h, w = raw.shape
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.empty((h, w), np.float32)
        _check(self._h, lib().tdv_depth_preprocess(self._h, _ptr(raw), _ptr(m), w, h, C.c_float(scale), mask_mode, _ptr(out)),
               "tdv_depth_preprocess")
        return out

    def bilateral_filter(self, depth, sigma_spatial, sigma_range):
        d = _f32(depth); h, w = d.shape
        out = np.empty_like(d)
        _check(self._h, lib().tdv_bilateral_filter(self._h, _ptr(d), w, h, C.c_float(sigma_spatial), C.c_float(sigma_range), _ptr(out)),
               "tdv_bilateral_filter")
        return out

    def mask_resize_nearest(self, masks, dst_width, dst_height):
        """cv::resize(mask, ..., INTER_NEAREST) of src/pipeline.cpp:38-41; masks: uint8 [h, w] or [B, h, w]."""
        m = np.ascontiguousarray(masks, np.uint8)
        single = m.ndim == 2
        if single:
            m = m[None]
        B, sh, sw = m.shape
        out = np.empty((B, dst_height, dst_width), np.uint8)
        _check(self._h, lib().tdv_mask_resize_nearest(self._h, _ptr(m), B, sw, sh, dst_width, dst_height, _ptr(out)), "tdv_mask_resize_nearest")
        return out[0] if single else out

    def deproject(self, depth, bgr, fx, fy, cx, cy, zmax, capacity=None):
        depth = _f32(depth)
        h, w = depth.shape
        b = None if bgr is None else np.ascontiguousarray(bgr, np.uint8)
        cap = h * w if capacity is None else capacity
        xyz = np.empty((cap, 3), np.float32)
        rgb = np.empty((cap, 3), np.float32) if b is not None else None
        n = C.c_int()
        _check(self._h, lib().tdv_deproject(self._h, _ptr(depth), _ptr(b), w, h, C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                            C.c_float(cy), C.c_float(zmax), _ptr(xyz), _ptr(rgb), cap, C.byref(n)), "tdv_deproject")
        return xyz[:n.value].copy(), (None if rgb is None else rgb[:n.value].copy())

    def depth_to_cloud(self, raw, mask, bgr, scale, fx, fy, cx, cy, zmax, mask_mode=TDV_MASK_THRESHOLD10):
        raw = np.ascontiguousarray(raw, np.uint16)
        h, w = raw.shape
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        b = None if bgr is None else np.ascontiguousarray(bgr, np.uint8)
        xyz = np.empty((h * w, 3), np.float32)
        rgb = np.empty((h * w, 3), np.float32) if b is not None else None
        n = C.c_int()
        _check(self._h, lib().tdv_depth_to_cloud(self._h, _ptr(raw), _ptr(m), _ptr(b), w, h, C.c_float(scale), mask_mode,
                                                 C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), C.c_float(zmax),
                                                 _ptr(xyz), _ptr(rgb), h * w, C.byref(n)), "tdv_depth_to_cloud")
        return xyz[:n.value].copy(), (None if rgb is None else rgb[:n.value].copy())

    # ---------------------------------------------------------------- R3
    def voxel_downsample(self, xyz, rgb, voxel, order=TDV_VOXEL_ORDER_REFERENCE):
        xyz = _f32(xyz); rgb = _f32(rgb)
        n = len(xyz)
        oxyz = np.empty((max(n, 1), 3), np.float32)
        orgb = np.empty((max(n, 1), 3), np.float32) if rgb is not None else None
        m = C.c_int()
        _check(self._h, lib().tdv_voxel_downsample(self._h, _ptr(xyz), _ptr(rgb), n, C.c_float(voxel), order, _ptr(oxyz), _ptr(orgb),
                                                   n, C.byref(m)), "tdv_voxel_downsample")
        return oxyz[:m.value].copy(), (None if orgb is None else orgb[:m.value].copy())

    def voxel_downsample_normals(self, xyz, normals, voxel, rgb=None, order=TDV_VOXEL_ORDER_REFERENCE):
        """voxel_downsample with the normals kept: (xyz, unit mean normals, rgb or None) per voxel (include/tdv_hip.h:
        tdv_voxel_downsample_normals)."""
        xyz = _f32(xyz); nrm = _f32(normals); rgb = _f32(rgb)
        n = len(xyz)
        oxyz = np.empty((max(n, 1), 3), np.float32)
        onrm = np.empty((max(n, 1), 3), np.float32) if nrm is not None else None
        orgb = np.empty((max(n, 1), 3), np.float32) if rgb is not None else None
        m = C.c_int()
        _check(self._h, lib().tdv_voxel_downsample_normals(self._h, _ptr(xyz), _ptr(nrm), _ptr(rgb), n, C.c_float(voxel), order, _ptr(oxyz),
                                                           _ptr(onrm), _ptr(orgb), n, C.byref(m)), "tdv_voxel_downsample_normals")
        return oxyz[:m.value].copy(), (None if onrm is None else onrm[:m.value].copy()), (None if orgb is None else orgb[:m.value].copy())

    # ---------------------------------------------------------------- R4
    def estimate_normals(self, xyz, k=30, want_knn=False):
        xyz = _f32(xyz); n = len(xyz)
        nrm = np.empty((n, 3), np.float32)
        knn = np.empty((n, k), np.int32) if want_knn else None
        _check(self._h, lib().tdv_estimate_normals(self._h, _ptr(xyz), n, k, _ptr(nrm), _ptr(knn)), "tdv_estimate_normals")
        return (nrm, knn) if want_knn else nrm

    def compute_fpfh(self, xyz, normals, radius, want_neighbors=False):
        xyz = _f32(xyz); normals = _f32(normals); n = len(xyz)
        desc = np.empty((n, 33), np.float32)
        nb = np.empty((n, 100), np.int32) if want_neighbors else None
        cnt = np.empty(n, np.int32) if want_neighbors else None
        _check(self._h, lib().tdv_compute_fpfh(self._h, _ptr(xyz), _ptr(normals), n, C.c_float(radius), _ptr(desc), _ptr(nb), _ptr(cnt)),
               "tdv_compute_fpfh")
        return (desc, nb, cnt) if want_neighbors else desc

    # ---------------------------------------------------------------- R5
    def feature_match(self, fs, ft):
        fs = _f32(fs); ft = _f32(ft)
        corr = np.empty(len(fs), np.int32)
        _check(self._h, lib().tdv_feature_match(self._h, _ptr(fs), len(fs), _ptr(ft), len(ft), _ptr(corr)), "tdv_feature_match")
        return corr

    def ransac(self, src, tgt, fs=None, ft=None, corr=None, voxel=0.001, max_iterations=100000, confidence=0.999,
               seed=42, trace=False):
        src = _f32(src); tgt = _f32(tgt); fs = _f32(fs); ft = _f32(ft)
        c = None if corr is None else np.ascontiguousarray(corr, np.int32)
        res = RansacResultC()
        tr = np.full(max(max_iterations, 1), -2, np.int32) if trace else None
        _check(self._h, lib().tdv_ransac(self._h, _ptr(src), len(src), _ptr(tgt), len(tgt), _ptr(fs), _ptr(ft), _ptr(c),
                                         C.c_float(voxel), max_iterations, C.c_float(confidence), C.c_uint32(seed),
                                         C.byref(res), _ptr(tr)), "tdv_ransac")
        return RegistrationResult(transformation=from_colmajor16(res.T), fitness=np.float32(res.fitness), rmse=np.float32(res.rmse),
                                  inliers=res.inliers, best_iteration=res.best_iteration, iterations_run=res.iterations_run,
                                  trace_inliers=tr)

    # ---------------------------------------------------------------- R6
    def icp(self, src, tgt, tgt_normals, T0, thr, max_iterations=200, point_to_plane=True):
        src = _f32(src); tgt = _f32(tgt); tn = _f32(tgt_normals)
        res = IcpResultC()
        t0 = to_colmajor16(T0)
        _check(self._h, lib().tdv_icp(self._h, _ptr(src), len(src), _ptr(tgt), _ptr(tn), len(tgt), _ptr(t0), C.c_float(thr),
                                      max_iterations, int(point_to_plane), C.byref(res)), "tdv_icp")
        return _icp_result(res)

    def icp_correspondences(self, src, tgt, T, thr):
        src = _f32(src); tgt = _f32(tgt)
        ns = len(src)
        corr = np.empty(ns, np.int32); d2 = np.empty(ns, np.float32); acc = np.empty(ns, np.uint8); nc = C.c_int()
        t = to_colmajor16(T)
        _check(self._h, lib().tdv_icp_correspondences(self._h, _ptr(src), ns, _ptr(tgt), len(tgt), _ptr(t), C.c_float(thr),
                                                      _ptr(corr), _ptr(d2), _ptr(acc), C.byref(nc)), "tdv_icp_correspondences")
        return dict(corr=corr, d2=d2, accepted=acc.astype(bool), n_corr=nc.value)

    # ---------------------------------------------------------------- device-resident (pointers are ints)
    def icp_dev(self, d_src, ns, d_tgt, d_tgt_normals, nt, T0, thr, max_iterations, point_to_plane=True, fixed_iterations=False):
        res = IcpResultC()
        t0 = to_colmajor16(T0)
        _check(self._h, lib().tdv_icp_dev(self._h, _ptr(d_src), ns, _ptr(d_tgt), _ptr(d_tgt_normals), nt, _ptr(t0), C.c_float(thr),
                                          max_iterations, int(point_to_plane), int(fixed_iterations), C.byref(res)), "tdv_icp_dev")
        return _icp_result(res)

    def icp_batch_dev(self, d_src, offsets, d_tgt, d_tgt_normals, nt, T0s, thr, max_iterations, point_to_plane=True, fixed_iterations=False):
        """ICP of many clouds against one target in one call (device pointers): cloud b = points [offsets[b], offsets[b + 1]) of d_src,
        start pose T0s[b] ((B, 4, 4)).  Per instance what icp_dev returns for that cloud, bit for bit."""
        off, n, t0, res = _icp_batch_args(offsets, T0s)
        _check(self._h, lib().tdv_icp_batch_dev(self._h, _ptr(d_src), _ptr(off), n, _ptr(d_tgt), _ptr(d_tgt_normals), nt, _ptr(t0), C.c_float(thr),
                                                max_iterations, int(point_to_plane), int(fixed_iterations), res), "tdv_icp_batch_dev")
        return [_icp_result(r) for r in res[:n]]

    def icp_batch(self, sources, tgt, tgt_normals, T0s, thr, max_iterations=200, point_to_plane=True):
        """icp_batch_dev on host clouds: a list of (n_b, 3) arrays against one target, uploaded with torch."""
        import torch
        srcs, off = _instance_rows(sources)
        tgt = _f32(tgt); tn = _f32(tgt_normals)
        d_src = _upload_rows(self.device, srcs); d_tgt = _upload_rows(self.device, tgt)
        d_tn = torch.from_numpy(tn).to(torch.device("cuda", self.device)) if tn is not None else None
        return self.icp_batch_dev(d_src.data_ptr(), off, d_tgt.data_ptr(), None if d_tn is None else d_tn.data_ptr(), len(tgt), T0s, thr,
                                  max_iterations, point_to_plane)

    # ---------------------------------------------------------------- generalized ICP (include/tdv_hip.h: tdv_gicp)
    def gicp(self, src, src_normals, tgt, tgt_normals, T0, thr, max_iterations=200, epsilon=1e-3):
        """Plane-to-plane ICP from both clouds' normals; the result as icp's."""
        src = _f32(src); sn = _f32(src_normals); tgt = _f32(tgt); tn = _f32(tgt_normals)
        res = IcpResultC()
        t0 = to_colmajor16(T0)
        _check(self._h, lib().tdv_gicp(self._h, _ptr(src), _ptr(sn), len(src), _ptr(tgt), _ptr(tn), len(tgt), _ptr(t0), C.c_float(thr),
                                       max_iterations, C.c_float(epsilon), C.byref(res)), "tdv_gicp")
        return _icp_result(res)

    def gicp_dev(self, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, T0, thr, max_iterations, epsilon=1e-3, fixed_iterations=False):
        res = IcpResultC()
        t0 = to_colmajor16(T0)
        _check(self._h, lib().tdv_gicp_dev(self._h, _ptr(d_src), _ptr(d_src_normals), ns, _ptr(d_tgt), _ptr(d_tgt_normals), nt, _ptr(t0),
                                           C.c_float(thr), max_iterations, C.c_float(epsilon), int(fixed_iterations), C.byref(res)), "tdv_gicp_dev")
        return _icp_result(res)

    def gicp_batch_dev(self, d_src, d_src_normals, offsets, d_tgt, d_tgt_normals, nt, T0s, thr, max_iterations, epsilon=1e-3, fixed_iterations=False):
        """GICP of many clouds against one target in one call (device pointers; the source normals laid out like d_src).  Per instance
        what gicp_dev returns for that cloud, bit for bit."""
        off, n, t0, res = _icp_batch_args(offsets, T0s)
        _check(self._h, lib().tdv_gicp_batch_dev(self._h, _ptr(d_src), _ptr(d_src_normals), _ptr(off), n, _ptr(d_tgt), _ptr(d_tgt_normals), nt,
                                                 _ptr(t0), C.c_float(thr), max_iterations, C.c_float(epsilon), int(fixed_iterations), res),
               "tdv_gicp_batch_dev")
        return [_icp_result(r) for r in res[:n]]

    def gicp_batch(self, sources, source_normals, tgt, tgt_normals, T0s, thr, max_iterations=200, epsilon=1e-3):
        """gicp_batch_dev on host clouds: lists of (n_b, 3) points and normals against one target, uploaded with torch."""
        srcs, off = _instance_rows(sources)
        sns, offn = _instance_rows(source_normals)
        if list(offn) != list(off):
            raise ValueError("gicp_batch: one normal per source point")
        tgt = _f32(tgt); tn = _f32(tgt_normals)
        d_src = _upload_rows(self.device, srcs); d_sn = _upload_rows(self.device, sns)
        d_tgt = _upload_rows(self.device, tgt); d_tn = _upload_rows(self.device, tn)
        return self.gicp_batch_dev(d_src.data_ptr(), d_sn.data_ptr(), off, d_tgt.data_ptr(), d_tn.data_ptr(), len(tgt), T0s, thr,
                                   max_iterations, epsilon)

    # ---------------------------------------------------------------- multi-scale ICP (include/tdv_hip.h: tdv_icp_multiscale)
    @staticmethod
    def _schedule(voxel_sizes, max_correspondence_distances, max_iterations, relative_fitness, relative_rmse, levels):
        if levels is None:
            levels = icp_levels(voxel_sizes, max_correspondence_distances, max_iterations, relative_fitness, relative_rmse)
        return levels, getattr(levels, "n_levels", len(levels))

    def multi_scale_icp(self, source, target, voxel_sizes, max_correspondence_distances, init, max_iterations=None,
                        estimation="point_to_plane", target_normals=None, source_normals=None, relative_fitness=float("inf"), relative_rmse=1e-6,
                        epsilon=1e-3, levels=None):
        """Coarse-to-fine ICP over a voxel pyramid (Open3D's multi_scale_icp): level l downsamples both clouds at voxel_sizes[l] (None or
        <= 0, last level only: as given) and refines the pose of the level before within max_correspondence_distances[l].  Scalars
        broadcast over the levels; `levels` (icp_levels) replaces the per-level arguments.  The result of the last level, every level's in
        .levels (with its point counts ns, nt)."""
        src = _f32(source); tgt = _f32(target); tn = _f32(target_normals); sn = _f32(source_normals)
        lv, n_levels = self._schedule(voxel_sizes, max_correspondence_distances, max_iterations, relative_fitness, relative_rmse, levels)
        res = (IcpLevelResultC * max(n_levels, 1))()
        t0 = to_colmajor16(init)
        _check(self._h, lib().tdv_icp_multiscale(self._h, _ptr(src), _ptr(sn), len(src), _ptr(tgt), _ptr(tn), len(tgt), _ptr(t0), lv, n_levels,
                                                 ICP_ESTIMATION[estimation], C.c_float(epsilon), res), "tdv_icp_multiscale")
        return _icp_level_results(res, n_levels)

    def multi_scale_icp_dev(self, d_src, ns, d_tgt, d_tgt_normals, nt, init, voxel_sizes=None, max_correspondence_distances=None, max_iterations=None,
                            estimation="point_to_plane", d_src_normals=None, relative_fitness=float("inf"), relative_rmse=1e-6, epsilon=1e-3,
                            levels=None):
        """multi_scale_icp on device pointers."""
        lv, n_levels = self._schedule(voxel_sizes, max_correspondence_distances, max_iterations, relative_fitness, relative_rmse, levels)
        res = (IcpLevelResultC * max(n_levels, 1))()
        t0 = to_colmajor16(init)
        _check(self._h, lib().tdv_icp_multiscale_dev(self._h, _ptr(d_src), _ptr(d_src_normals), ns, _ptr(d_tgt), _ptr(d_tgt_normals), nt, _ptr(t0),
                                                     lv, n_levels, ICP_ESTIMATION[estimation], C.c_float(epsilon), res), "tdv_icp_multiscale_dev")
        return _icp_level_results(res, n_levels)

    def multi_scale_icp_batch_dev(self, d_src, offsets, d_tgt, d_tgt_normals, nt, T0s, voxel_sizes=None, max_correspondence_distances=None,
                                  max_iterations=None, estimation="point_to_plane", d_src_normals=None, relative_fitness=float("inf"),
                                  relative_rmse=1e-6, epsilon=1e-3, levels=None):
        """multi_scale_icp of many clouds against one target in one call (device pointers, laid out as icp_batch_dev's).  Per instance
        what multi_scale_icp_dev returns for that cloud, bit for bit."""
        lv, n_levels = self._schedule(voxel_sizes, max_correspondence_distances, max_iterations, relative_fitness, relative_rmse, levels)
        off, n, t0, _ = _icp_batch_args(offsets, T0s)
        res = (IcpLevelResultC * max(n * n_levels, 1))()
        _check(self._h, lib().tdv_icp_multiscale_batch_dev(self._h, _ptr(d_src), _ptr(d_src_normals), _ptr(off), n, _ptr(d_tgt), _ptr(d_tgt_normals),
                                                           nt, _ptr(t0), lv, n_levels, ICP_ESTIMATION[estimation], C.c_float(epsilon), res),
               "tdv_icp_multiscale_batch_dev")
        return [_icp_level_results(res, n_levels, b) for b in range(n)]

    def multi_scale_icp_batch(self, sources, target, voxel_sizes, max_correspondence_distances, T0s, max_iterations=None,
                              estimation="point_to_plane", target_normals=None, source_normals=None, relative_fitness=float("inf"),
                              relative_rmse=1e-6, epsilon=1e-3, levels=None):
        """multi_scale_icp_batch_dev on host clouds: a list of (n_b, 3) arrays (and their normals, GICP) against one target, uploaded with
        torch; the offsets are made here."""
        srcs, off = _instance_rows(sources)
        d_sn = None
        if source_normals is not None:
            sns, offn = _instance_rows(source_normals)
            if list(offn) != list(off):
                raise ValueError("multi_scale_icp_batch: one normal per source point")
            d_sn = _upload_rows(self.device, sns)
        tgt = _f32(target); tn = _f32(target_normals)
        d_src = _upload_rows(self.device, srcs); d_tgt = _upload_rows(self.device, tgt)
        d_tn = _upload_rows(self.device, tn) if tn is not None else None
        return self.multi_scale_icp_batch_dev(d_src.data_ptr(), off, d_tgt.data_ptr(), None if d_tn is None else d_tn.data_ptr(), len(tgt), T0s,
                                              voxel_sizes, max_correspondence_distances, max_iterations, estimation,
                                              None if d_sn is None else d_sn.data_ptr(), relative_fitness, relative_rmse, epsilon, levels)

    # ---------------------------------------------------------------- colored ICP (include/tdv_hip.h: tdv_colored_icp)
    def color_gradients(self, xyz, rgb, normals, k=30):
        """(n, 4) float32 per point: intensity I and its gradient d on the tangent plane, from the k nearest neighbours."""
        xyz = _f32(xyz); rgb = _f32(rgb); nrm = _f32(normals); n = len(xyz)
        out = np.empty((n, 4), np.float32)
        _check(self._h, lib().tdv_color_gradients(self._h, _ptr(xyz), _ptr(rgb), _ptr(nrm), n, k, _ptr(out)), "tdv_color_gradients")
        return out

    def color_gradients_dev(self, d_xyz, d_rgb, d_normals, n, k, d_color, d_knn=None):
        """d_knn (optional): estimate_normals_dev's list for the same cloud and k; None runs that search."""
        _check(self._h, lib().tdv_color_gradients_dev(self._h, _ptr(d_xyz), _ptr(d_rgb), _ptr(d_normals), n, k, _ptr(d_knn), _ptr(d_color)),
               "tdv_color_gradients_dev")

    def colored_icp(self, src, src_rgb, tgt, tgt_normals, tgt_color, T0, thr, max_iterations=200, lambda_geometric=0.968):
        """Point-to-plane plus photometric ICP; tgt_color = color_gradients of the target.  The result as icp's."""
        src = _f32(src); rgb = _f32(src_rgb); tgt = _f32(tgt); tn = _f32(tgt_normals); tc = _f32(tgt_color)
        res = IcpResultC()
        t0 = to_colmajor16(T0)
        _check(self._h, lib().tdv_colored_icp(self._h, _ptr(src), _ptr(rgb), len(src), _ptr(tgt), _ptr(tn), _ptr(tc), len(tgt), _ptr(t0),
                                              C.c_float(thr), max_iterations, C.c_float(lambda_geometric), C.byref(res)), "tdv_colored_icp")
        return _icp_result(res)

    def colored_icp_dev(self, d_src, d_src_rgb, ns, d_tgt, d_tgt_normals, d_tgt_color, nt, T0, thr, max_iterations, lambda_geometric=0.968,
                        fixed_iterations=False):
        res = IcpResultC()
        t0 = to_colmajor16(T0)
        _check(self._h, lib().tdv_colored_icp_dev(self._h, _ptr(d_src), _ptr(d_src_rgb), ns, _ptr(d_tgt), _ptr(d_tgt_normals), _ptr(d_tgt_color), nt,
                                                  _ptr(t0), C.c_float(thr), max_iterations, C.c_float(lambda_geometric), int(fixed_iterations),
                                                  C.byref(res)), "tdv_colored_icp_dev")
        return _icp_result(res)

    def colored_icp_batch_dev(self, d_src, d_src_rgb, offsets, d_tgt, d_tgt_normals, d_tgt_color, nt, T0s, thr, max_iterations,
                              lambda_geometric=0.968, fixed_iterations=False):
        """Colored ICP of many clouds against one target in one call (device pointers; the source colours laid out like d_src).  Per
        instance what colored_icp_dev returns for that cloud, bit for bit."""
        off, n, t0, res = _icp_batch_args(offsets, T0s)
        _check(self._h, lib().tdv_colored_icp_batch_dev(self._h, _ptr(d_src), _ptr(d_src_rgb), _ptr(off), n, _ptr(d_tgt), _ptr(d_tgt_normals),
                                                        _ptr(d_tgt_color), nt, _ptr(t0), C.c_float(thr), max_iterations,
                                                        C.c_float(lambda_geometric), int(fixed_iterations), res), "tdv_colored_icp_batch_dev")
        return [_icp_result(r) for r in res[:n]]

    def colored_icp_batch(self, sources, source_rgbs, tgt, tgt_normals, tgt_color, T0s, thr, max_iterations=200, lambda_geometric=0.968):
        """colored_icp_batch_dev on host clouds: lists of (n_b, 3) points and colours against one target, uploaded with torch."""
        srcs, off = _instance_rows(sources)
        rgbs, offc = _instance_rows(source_rgbs)
        if list(offc) != list(off):
            raise ValueError("colored_icp_batch: one colour per source point")
        tgt = _f32(tgt); tn = _f32(tgt_normals); tc = _f32(tgt_color).reshape(-1, 4)
        d_src = _upload_rows(self.device, srcs); d_rgb = _upload_rows(self.device, rgbs)
        d_tgt = _upload_rows(self.device, tgt); d_tn = _upload_rows(self.device, tn); d_tc = _upload_rows(self.device, tc, 4)
        return self.colored_icp_batch_dev(d_src.data_ptr(), d_rgb.data_ptr(), off, d_tgt.data_ptr(), d_tn.data_ptr(), d_tc.data_ptr(), len(tgt),
                                          T0s, thr, max_iterations, lambda_geometric)

    # ---------------------------------------------------------------- Fast Global Registration
    @staticmethod
    def _fgr_result(res):
        return RegistrationResult(transformation=from_colmajor16(res.T), fitness=np.float32(res.fitness), rmse=np.float32(res.rmse),
                                  inliers=res.inliers), dict(n_mutual=res.n_mutual, n_tuple=res.n_tuple, degenerate=bool(res.degenerate),
                                                             trials_run=res.trials_run)

    def fgr(self, src, tgt, fs, ft, voxel, **params):
        """tdv_fgr: (RegistrationResult with transformation, fitness, rmse, inliers; dict n_mutual, n_tuple, degenerate, trials_run)."""
        src = _f32(src).reshape(-1, 3); tgt = _f32(tgt).reshape(-1, 3); fs = _f32(fs).reshape(-1, 33); ft = _f32(ft).reshape(-1, 33)
        res = FgrResultC(); p = fgr_params(**params)
        _check(self._h, lib().tdv_fgr(self._h, _ptr(src), len(src), _ptr(tgt), len(tgt), _ptr(fs), _ptr(ft), C.c_float(voxel), C.byref(p),
                                      C.byref(res)), "tdv_fgr")
        return self._fgr_result(res)

    def fgr_dev(self, d_src, ns, d_tgt, nt, d_fs, d_ft, voxel, **params):
        res = FgrResultC(); p = fgr_params(**params)
        _check(self._h, lib().tdv_fgr_dev(self._h, _ptr(d_src), ns, _ptr(d_tgt), nt, _ptr(d_fs), _ptr(d_ft), C.c_float(voxel), C.byref(p),
                                          C.byref(res)), "tdv_fgr_dev")
        return self._fgr_result(res)

    def fgr_correspondences(self, src, tgt, fs, ft, **params):
        """tdv_fgr_correspondences: dict(mutual (k, 2) int32 pairs, tuples (m, 2), n_mutual, n_tuple, trials_run)."""
        src = _f32(src).reshape(-1, 3); tgt = _f32(tgt).reshape(-1, 3); fs = _f32(fs).reshape(-1, 33); ft = _f32(ft).reshape(-1, 33)
        p = fgr_params(**params)
        nm = C.c_int(); nu = C.c_int(); tr = C.c_longlong()
        args = (self._h, _ptr(src), len(src), _ptr(tgt), len(tgt), _ptr(fs), _ptr(ft), C.byref(p))
        st = lib().tdv_fgr_correspondences(*args, None, 0, None, 0, C.byref(nm), C.byref(nu), C.byref(tr))   # size query
        if st not in (0, -2) or (st == -2 and nm.value == 0 and nu.value == 0):
            _check(self._h, st, "tdv_fgr_correspondences")
        mutual = np.zeros((nm.value, 2), np.int32); tuples = np.zeros((nu.value, 2), np.int32)
        _check(self._h, lib().tdv_fgr_correspondences(*args, _ptr(mutual), nm.value, _ptr(tuples), nu.value, C.byref(nm), C.byref(nu),
                                                      C.byref(tr)), "tdv_fgr_correspondences")
        return dict(mutual=mutual, tuples=tuples, n_mutual=nm.value, n_tuple=nu.value, trials_run=tr.value)

    # ---------------------------------------------------------------- plane segmentation (include/tdv_hip.h: tdv_segment_planes)
    def segment_planes(self, xyz, **params):
        """tdv_segment_planes: (list of one dict per plane kept - plane, hypothesis, fitness, rmse, inliers, candidates, best_iteration,
        iterations_run - and labels int32[n]: k for the points of plane k, -1 for the rest)."""
        xyz = _f32(xyz).reshape(-1, 3); n = len(xyz)
        p = plane_params(**params)
        res = (PlaneResultC * TDV_PLANE_MAX)(); npl = C.c_int()
        labels = np.empty(max(n, 1), np.int32)
        _check(self._h, lib().tdv_segment_planes(self._h, _ptr(xyz), n, C.byref(p), res, C.byref(npl), _ptr(labels)), "tdv_segment_planes")
        return _plane_results(res, npl.value), labels[:n]

    def segment_planes_dev(self, d_xyz, n, d_labels=None, d_rest=None, **params):
        """tdv_segment_planes_dev on device pointers: (list of plane dicts as segment_planes, n_rest).  d_labels (int32[n]) and d_rest
        (float[3n]: the unlabelled points in ascending index) are optional."""
        p = plane_params(**params)
        res = (PlaneResultC * TDV_PLANE_MAX)(); npl = C.c_int(); nr = C.c_int()
        _check(self._h, lib().tdv_segment_planes_dev(self._h, _ptr(d_xyz), n, C.byref(p), res, C.byref(npl), _ptr(d_labels), _ptr(d_rest),
                                                     C.byref(nr)), "tdv_segment_planes_dev")
        return _plane_results(res, npl.value), nr.value

    def segment_plane(self, xyz, distance_threshold=0.01, ransac_n=3, num_iterations=100, probability=0.99999999, seed=42):
        """Open3D's PointCloud.segment_plane: (plane_model float32[4], inlier indices int64, ascending).  One plane; a search
        that keeps none gives zeros and no index."""
        if ransac_n != 3:
            raise ValueError("segment_plane: only ransac_n = 3 is provided (got %r)" % (ransac_n,))
        planes, labels = self.segment_planes(xyz, distance_threshold=distance_threshold, num_iterations=num_iterations,
                                             probability=probability, seed=seed, max_planes=1)
        if not planes:
            return np.zeros(4, np.float32), np.zeros(0, np.int64)
        return planes[0]["plane"], np.nonzero(labels == 0)[0]

    # ---------------------------------------------------------------- clustering (include/tdv_hip.h: tdv_cluster_dbscan)
    def cluster(self, xyz, eps, min_points, min_cluster_size=1, grouped=False):
        """tdv_cluster_dbscan: (result dict - n_clusters, n_core, n_border, n_noise, n_dropped, largest, n_labelled -, labels int32[n],
        order int32[n]: the labelled points by (label, index), then the noise, offsets int32[n_clusters + 1] into order).
        grouped=True appends the cloud's rows in that order."""
        xyz = _f32(xyz).reshape(-1, 3); n = len(xyz)
        p = cluster_params(eps=eps, min_points=min_points, min_cluster_size=min_cluster_size)
        res = ClusterResultC(); nl = C.c_int()
        labels = np.empty(max(n, 1), np.int32); order = np.empty(max(n, 1), np.int32); offsets = np.empty(n + 1, np.int32)
        rows = np.empty((max(n, 1), 3), np.float32) if grouped else None
        _check(self._h, lib().tdv_cluster_dbscan(self._h, _ptr(xyz), n, C.byref(p), C.byref(res), _ptr(labels), _ptr(order), _ptr(rows),
                                                 _ptr(offsets), n, C.byref(nl)), "tdv_cluster_dbscan")
        out = (dict(_fields_dict(res), n_labelled=nl.value), labels[:n], order[:n], offsets[:res.n_clusters + 1].copy())
        return out + (rows[:n],) if grouped else out

    def cluster_dbscan(self, xyz, eps, min_points, min_cluster_size=1):
        """Open3D's PointCloud.cluster_dbscan: labels int32[n], -1 for noise."""
        return self.cluster(xyz, eps, min_points, min_cluster_size)[1]

    def cluster_dbscan_dev(self, d_xyz, n, eps, min_points, min_cluster_size=1, d_labels=None, d_order=None, d_grouped=None):
        """tdv_cluster_dbscan_dev on device pointers: (result dict as cluster's, offsets int32[n_clusters + 1] on the host).  d_labels
        (int32[n]), d_order (int32[n]) and d_grouped (float[3n]) are optional; (d_grouped, offsets) is what the batch calls take."""
        p = cluster_params(eps=eps, min_points=min_points, min_cluster_size=min_cluster_size)
        res = ClusterResultC(); nl = C.c_int()
        offsets = np.empty(n + 1, np.int32)
        _check(self._h, lib().tdv_cluster_dbscan_dev(self._h, _ptr(d_xyz), n, C.byref(p), C.byref(res), _ptr(d_labels), _ptr(d_order),
                                                     _ptr(d_grouped), _ptr(offsets), n, C.byref(nl)), "tdv_cluster_dbscan_dev")
        return dict(_fields_dict(res), n_labelled=nl.value), offsets[:res.n_clusters + 1].copy()

    # ---------------------------------------------------------------- outlier removal (include/tdv_hip.h: tdv_remove_statistical_outlier)
    def _outlier_host(self, fn, what, xyz, rgb, a, b, per_point_dtype):
        xyz = _f32(xyz).reshape(-1, 3); n = len(xyz)
        rgb = None if rgb is None else _f32(rgb).reshape(-1, 3)
        if rgb is not None and len(rgb) != n:
            raise ValueError("%s: one colour per point" % what)
        res = OutlierResultC()
        mask = np.zeros(max(n, 1), np.uint8); per = np.zeros(max(n, 1), per_point_dtype); index = np.zeros(max(n, 1), np.int32)
        rows = np.zeros((max(n, 1), 3), np.float32); cols = None if rgb is None else np.zeros((max(n, 1), 3), np.float32)
        _check(self._h, fn(self._h, _ptr(xyz), _ptr(rgb), n, a, b, C.byref(res), _ptr(mask), _ptr(per), _ptr(index), _ptr(rows), _ptr(cols)), what)
        m = res.n_kept
        return dict(_fields_dict(res), mask=mask[:n], per_point=per[:n], index=index[:m], xyz=rows[:m], rgb=None if cols is None else cols[:m])

    def statistical_outlier(self, xyz, nb_neighbors, std_ratio, rgb=None):
        """tdv_remove_statistical_outlier, every output: dict(n_valid, n_kept, cloud_mean, std_dev, threshold, mask uint8[n], mean float64[n],
        index int32[n_kept], xyz float32[n_kept, 3], rgb or None)."""
        r = self._outlier_host(lib().tdv_remove_statistical_outlier, "tdv_remove_statistical_outlier", xyz, rgb, int(nb_neighbors),
                               C.c_double(std_ratio), np.float64)
        r["mean"] = r.pop("per_point")
        return r

    def radius_outlier(self, xyz, nb_points, radius, rgb=None):
        """tdv_remove_radius_outlier, every output: as statistical_outlier, with count int32[n] (saturated at nb_points + 1) for mean."""
        r = self._outlier_host(lib().tdv_remove_radius_outlier, "tdv_remove_radius_outlier", xyz, rgb, int(nb_points), C.c_float(radius), np.int32)
        r["count"] = r.pop("per_point")
        return r

    def remove_statistical_outlier(self, xyz, nb_neighbors, std_ratio, rgb=None):
        """Open3D's PointCloud.remove_statistical_outlier: (the kept rows, ind - their indices, int64 ascending); with rgb, (rows, colours, ind)."""
        r = self.statistical_outlier(xyz, nb_neighbors, std_ratio, rgb)
        ind = r["index"].astype(np.int64)
        return (r["xyz"], ind) if rgb is None else (r["xyz"], r["rgb"], ind)

    def remove_radius_outlier(self, xyz, nb_points, radius, rgb=None):
        """Open3D's PointCloud.remove_radius_outlier: (the kept rows, ind); with rgb, (rows, colours, ind)."""
        r = self.radius_outlier(xyz, nb_points, radius, rgb)
        ind = r["index"].astype(np.int64)
        return (r["xyz"], ind) if rgb is None else (r["xyz"], r["rgb"], ind)

    def remove_statistical_outlier_dev(self, d_xyz, n, nb_neighbors, std_ratio, d_rgb=None, d_mask=None, d_mean=None, d_index=None,
                                       d_out_xyz=None, d_out_rgb=None):
        """tdv_remove_statistical_outlier_dev on device pointers: the result dict (n_valid, n_kept, cloud_mean, std_dev, threshold).  d_mask
        (uint8[n]), d_mean (float64[n]), d_index (int32[n]), d_out_xyz and d_out_rgb (float[3n]) are optional; n_kept rows are written."""
        res = OutlierResultC()
        _check(self._h, lib().tdv_remove_statistical_outlier_dev(self._h, _ptr(d_xyz), _ptr(d_rgb), n, int(nb_neighbors), C.c_double(std_ratio),
                                                                 C.byref(res), _ptr(d_mask), _ptr(d_mean), _ptr(d_index), _ptr(d_out_xyz),
                                                                 _ptr(d_out_rgb)), "tdv_remove_statistical_outlier_dev")
        return _fields_dict(res)

    def remove_radius_outlier_dev(self, d_xyz, n, nb_points, radius, d_rgb=None, d_mask=None, d_count=None, d_index=None, d_out_xyz=None,
                                  d_out_rgb=None):
        """tdv_remove_radius_outlier_dev on device pointers: the result dict; d_count (int32[n]) takes d_mean's place."""
        res = OutlierResultC()
        _check(self._h, lib().tdv_remove_radius_outlier_dev(self._h, _ptr(d_xyz), _ptr(d_rgb), n, int(nb_points), C.c_float(radius), C.byref(res),
                                                            _ptr(d_mask), _ptr(d_count), _ptr(d_index), _ptr(d_out_xyz), _ptr(d_out_rgb)),
               "tdv_remove_radius_outlier_dev")
        return _fields_dict(res)

    # ---------------------------------------------------------------- ISS keypoints (include/tdv_hip.h: tdv_iss_keypoints)
    def iss(self, xyz, attr=None, **params):
        """tdv_iss_keypoints, every output: dict(n_finite, n_supported, n_salient, n_keypoints, salient_radius, non_max_radius, resolution,
        mask uint8[n], saliency float64[n], eigenvalues float64[n, 3], support int32[n], index int32[n_keypoints], xyz
        float32[n_keypoints, 3], attr float32[n_keypoints, width] or None).  attr: one row of floats per point, gathered beside xyz."""
        xyz = _f32(xyz).reshape(-1, 3); n = len(xyz)
        width = 0
        if attr is not None:
            attr = _f32(attr)
            if attr.ndim != 2 or len(attr) != n:
                raise ValueError("tdv_iss_keypoints: one attr row per point")
            width = attr.shape[1]
        p = iss_params(**params)
        res = IssResultC()
        m1 = max(n, 1)
        mask = np.zeros(m1, np.uint8); sal = np.zeros(m1, np.float64); eig = np.zeros((m1, 3), np.float64); sup = np.zeros(m1, np.int32)
        index = np.zeros(m1, np.int32); rows = np.zeros((m1, 3), np.float32)
        cols = None if attr is None else np.zeros((m1, max(width, 1)), np.float32)
        _check(self._h, lib().tdv_iss_keypoints(self._h, _ptr(xyz), n, C.byref(p), _ptr(attr), width, C.byref(res), _ptr(mask), _ptr(sal), _ptr(eig),
                                                _ptr(sup), _ptr(index), _ptr(rows), _ptr(cols)), "tdv_iss_keypoints")
        m = res.n_keypoints
        return dict(_fields_dict(res), mask=mask[:n], saliency=sal[:n], eigenvalues=eig[:n], support=sup[:n], index=index[:m], xyz=rows[:m],
                    attr=None if cols is None else cols.reshape(-1)[:m * width].reshape(m, width))

    def compute_iss_keypoints(self, xyz, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
        """Open3D's geometry.keypoint.compute_iss_keypoints: (the keypoints' rows, ind - their indices, int64 ascending)."""
        r = self.iss(xyz, salient_radius=salient_radius, non_max_radius=non_max_radius, gamma_21=gamma_21, gamma_32=gamma_32,
                     min_neighbors=min_neighbors)
        return r["xyz"], r["index"].astype(np.int64)

    def iss_keypoints_dev(self, d_xyz, n, d_attr=None, attr_width=0, d_mask=None, d_saliency=None, d_eigenvalues=None, d_support=None,
                          d_index=None, d_out_xyz=None, d_out_attr=None, **params):
        """tdv_iss_keypoints_dev on device pointers: the result dict.  d_mask (uint8[n]), d_saliency (float64[n]), d_eigenvalues
        (float64[3n]), d_support (int32[n]), d_index (int32[n]), d_out_xyz (float[3n]) and d_out_attr (float[attr_width * n]) are optional;
        n_keypoints rows are written - (d_out_xyz, d_out_attr) are the (src, fs) of ransac_dev and fgr_dev."""
        p = iss_params(**params)
        res = IssResultC()
        _check(self._h, lib().tdv_iss_keypoints_dev(self._h, _ptr(d_xyz), n, C.byref(p), _ptr(d_attr), int(attr_width), C.byref(res), _ptr(d_mask),
                                                    _ptr(d_saliency), _ptr(d_eigenvalues), _ptr(d_support), _ptr(d_index), _ptr(d_out_xyz),
                                                    _ptr(d_out_attr)), "tdv_iss_keypoints_dev")
        return _fields_dict(res)

    # ---------------------------------------------------------------- farthest point sampling (include/tdv_hip.h: tdv_farthest_point_down_sample)
    def fps(self, xyz, num_samples, start_index=0, attr=None):
        """tdv_farthest_point_down_sample, every output: dict(n_usable, n_selected, path, cover_d2, index int32[n_selected] in selection
        order, d2 float32[n_selected], xyz float32[n_selected, 3], attr float32[n_selected, width] or None).  attr: one row of floats per
        point, gathered beside xyz."""
        xyz = _f32(xyz).reshape(-1, 3); n = len(xyz)
        width = 0
        if attr is not None:
            attr = _f32(attr)
            if attr.ndim != 2 or len(attr) != n:
                raise ValueError("tdv_farthest_point_down_sample: one attr row per point")
            width = attr.shape[1]
        res = FpsResultC()
        m1 = max(min(int(num_samples), n), 1)
        index = np.zeros(m1, np.int32); d2 = np.zeros(m1, np.float32); rows = np.zeros((m1, 3), np.float32)
        cols = None if attr is None else np.zeros((m1, max(width, 1)), np.float32)
        _check(self._h, lib().tdv_farthest_point_down_sample(self._h, _ptr(xyz), n, int(num_samples), int(start_index), _ptr(attr), width,
                                                             C.byref(res), _ptr(index), _ptr(d2), _ptr(rows), _ptr(cols)),
               "tdv_farthest_point_down_sample")
        m = res.n_selected
        return dict(_fps_result(res), index=index[:m], d2=d2[:m], xyz=rows[:m],
                    attr=None if cols is None else cols.reshape(-1)[:m * width].reshape(m, width))

    def farthest_point_down_sample(self, xyz, num_samples, start_index=0):
        """Open3D's PointCloud.farthest_point_down_sample: the selected rows, in selection order."""
        return self.fps(xyz, num_samples, start_index)["xyz"]

    def fps_dev(self, d_xyz, n, num_samples, start_index=0, d_attr=None, attr_width=0, d_index=None, d_out_d2=None, d_out_xyz=None,
                d_out_attr=None):
        """tdv_farthest_point_down_sample_dev on device pointers: the result dict.  d_index (int32), d_out_d2 (float), d_out_xyz (3 floats)
        and d_out_attr (attr_width floats) per sample, each of min(num_samples, n) entries, are optional; n_selected rows are written."""
        res = FpsResultC()
        _check(self._h, lib().tdv_farthest_point_down_sample_dev(self._h, _ptr(d_xyz), int(n), int(num_samples), int(start_index), _ptr(d_attr),
                                                                 int(attr_width), C.byref(res), _ptr(d_index), _ptr(d_out_d2), _ptr(d_out_xyz),
                                                                 _ptr(d_out_attr)), "tdv_farthest_point_down_sample_dev")
        return _fps_result(res)

    def fps_batch_dev(self, d_xyz, offsets, num_samples, d_attr=None, attr_width=0, d_index=None, d_out_d2=None, d_out_xyz=None, d_out_attr=None):
        """tdv_farthest_point_down_sample_batch_dev on device pointers: cloud b = rows [offsets[b], offsets[b + 1]) of d_xyz and d_attr, each
        sampled from its row 0.  Returns (one result dict per cloud, out offsets int32[n_clouds + 1]); cloud b's samples are rows
        [out offsets[b], out offsets[b + 1]) of the optional device outputs (each of sum over b of min(num_samples, n_b) entries)."""
        off = np.ascontiguousarray(offsets, np.int32)
        n = len(off) - 1
        res = (FpsResultC * max(n, 1))()
        out_off = np.zeros(n + 1, np.int32)
        _check(self._h, lib().tdv_farthest_point_down_sample_batch_dev(self._h, _ptr(d_xyz), _ptr(d_attr), int(attr_width), _ptr(off), n,
                                                                       int(num_samples), res, _ptr(out_off), _ptr(d_index), _ptr(d_out_d2),
                                                                       _ptr(d_out_xyz), _ptr(d_out_attr)),
               "tdv_farthest_point_down_sample_batch_dev")
        return [_fps_result(res[b]) for b in range(n)], out_off

    def fps_batch(self, xyz, offsets, num_samples, attr=None):
        """fps_batch_dev on host arrays (rows of all clouds back to back): one dict per cloud as fps() returns it, index inside the cloud."""
        import torch
        xyz = np.array(xyz, np.float32).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, np.int32)
        width = 0
        d_a = None
        if attr is not None:
            attr = np.array(attr, np.float32)
            if attr.ndim != 2 or len(attr) != len(xyz):
                raise ValueError("tdv_farthest_point_down_sample_batch_dev: one attr row per point")
            width = attr.shape[1]
            d_a = _upload_rows(self.device, attr, max(width, 1))
        d_x = _upload_rows(self.device, xyz)
        cap = max(int(np.minimum(np.diff(off), int(num_samples)).sum()) if len(off) > 1 else 0, 1)
        dev = torch.device("cuda", self.device)
        oi = torch.zeros(cap, dtype=torch.int32, device=dev); od = torch.zeros(cap, dtype=torch.float32, device=dev)
        ox = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
        oa = None if attr is None else torch.zeros((cap, max(width, 1)), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        res, out_off = self.fps_batch_dev(d_x.data_ptr(), off, num_samples, None if d_a is None else d_a.data_ptr(), width, oi.data_ptr(),
                                          od.data_ptr(), ox.data_ptr(), None if oa is None else oa.data_ptr())
        self.synchronize()
        hi, hd, hx = oi.cpu().numpy(), od.cpu().numpy(), ox.cpu().numpy()
        ha = None if oa is None else oa.cpu().numpy().reshape(-1)
        out = []
        for b, r in enumerate(res):
            a, e = int(out_off[b]), int(out_off[b + 1])
            out.append(dict(r, index=hi[a:e].copy(), d2=hd[a:e].copy(), xyz=hx[a:e].copy(),
                            attr=None if ha is None else ha[a * width:e * width].reshape(e - a, width).copy()))
        return out

    # ---------------------------------------------------------------- pose verification (include/tdv_hip.h: tdv_verify_poses)
    def verify_poses(self, model, poses, raw, scale, fx, fy, cx, cy, **params):
        """tdv_verify_poses: the model ([n, 3]) splatted at every pose ([n_poses, 4, 4], row-major as everywhere at this level) into the
        frame of the raw u16 depth image `raw` ([H, W]) and each rendered pixel classified against the observed depth
        float(raw) * float(1.0 / scale): (one dict per pose of n_projected, n_rendered, n_consistent, n_occluded, n_violating, n_unknown,
        err_q20 - all integers, n_rendered their sum over the four classes -, order int32[n_poses]: the pose indices by
        n_consistent - n_violating descending, ties to the lower index).  params: verify_params' fields (pose_direction, splat, tau, zmax)."""
        model = _f32(model).reshape(-1, 3)
        raw = np.ascontiguousarray(raw, np.uint16)
        h, w = raw.shape
        t, n = _poses16(poses)
        res = (VerifyResultC * max(n, 1))()
        order = np.zeros(n, np.int32)
        _check(self._h, lib().tdv_verify_poses(self._h, _ptr(model), len(model), _ptr(t), n, _ptr(raw), w, h, C.c_float(scale), C.c_float(fx),
                                               C.c_float(fy), C.c_float(cx), C.c_float(cy), C.byref(verify_params(**params)), res,
                                               _ptr(order)), "tdv_verify_poses")
        return _verify_results(res, n), order

    def verify_poses_dev(self, d_model, n_model, poses, d_raw, w, h, scale, fx, fy, cx, cy, **params):
        """tdv_verify_poses_dev: verify_poses with the model (float[3 n_model]) and the raw frame (uint16[w h]) as device pointers; the poses
        and the results stay on the host.  One read-back."""
        t, n = _poses16(poses)
        res = (VerifyResultC * max(n, 1))()
        order = np.zeros(n, np.int32)
        _check(self._h, lib().tdv_verify_poses_dev(self._h, _ptr(d_model), int(n_model), _ptr(t), n, _ptr(d_raw), int(w), int(h), C.c_float(scale),
                                                   C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), C.byref(verify_params(**params)),
                                                   res, _ptr(order)), "tdv_verify_poses_dev")
        return _verify_results(res, n), order

    def render_depth(self, model, pose, w, h, fx, fy, cx, cy, **params):
        """tdv_render_depth: the rendered depth of the model at one pose, float32 [h, w], 0 where nothing rendered - per pixel the minimum
        camera z over the model points whose splat square covers it (the z-buffer verify_poses classifies)."""
        model = _f32(model).reshape(-1, 3)
        out = np.zeros((int(h), int(w)), np.float32)
        n = C.c_int()
        _check(self._h, lib().tdv_render_depth(self._h, _ptr(model), len(model), _ptr(to_colmajor16(pose)), int(w), int(h), C.c_float(fx),
                                               C.c_float(fy), C.c_float(cx), C.c_float(cy), C.byref(verify_params(**params)), _ptr(out),
                                               C.byref(n)), "tdv_render_depth")
        return out

    def render_depth_dev(self, d_model, n_model, pose, w, h, fx, fy, cx, cy, d_out_depth, **params):
        """tdv_render_depth_dev: render_depth from a device model into the device image d_out_depth (float[w h]); returns n_rendered."""
        n = C.c_int()
        _check(self._h, lib().tdv_render_depth_dev(self._h, _ptr(d_model), int(n_model), _ptr(to_colmajor16(pose)), int(w), int(h), C.c_float(fx),
                                                   C.c_float(fy), C.c_float(cx), C.c_float(cy), C.byref(verify_params(**params)),
                                                   _ptr(d_out_depth), C.byref(n)), "tdv_render_depth_dev")
        return n.value

    # ---------------------------------------------------------------- pose verification from a mesh (include/tdv_hip.h: tdv_verify_poses_mesh)
    def verify_poses_mesh(self, vertices, triangles, poses, raw, scale, fx, fy, cx, cy, **params):
        """tdv_verify_poses_mesh: verify_poses with the model's faces rasterised - vertices [n, 3], triangles int [m, 3] - in place of a
        point splat.  Returns what verify_poses returns; n_projected counts the usable triangles.  params: mesh_verify_params' fields
        (pose_direction, cull, tau, zmax)."""
        vtx, tri = _mesh(vertices, triangles)
        raw = np.ascontiguousarray(raw, np.uint16)
        h, w = raw.shape
        t, n = _poses16(poses)
        res = (VerifyResultC * max(n, 1))()
        order = np.zeros(n, np.int32)
        _check(self._h, lib().tdv_verify_poses_mesh(self._h, _ptr(vtx), len(vtx), _ptr(tri), len(tri), _ptr(t), n, _ptr(raw), w, h, C.c_float(scale),
                                                    C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                                    C.byref(mesh_verify_params(**params)), res, _ptr(order)), "tdv_verify_poses_mesh")
        return _verify_results(res, n), order

    def verify_poses_mesh_dev(self, d_vertices, n_vertices, d_triangles, n_triangles, poses, d_raw, w, h, scale, fx, fy, cx, cy, **params):
        """tdv_verify_poses_mesh_dev: verify_poses_mesh with the vertices (float[3 n_vertices]), the triangles (int32[3 n_triangles]) and the
        raw frame (uint16[w h]) as device pointers; the poses and the results stay on the host.  One read-back."""
        t, n = _poses16(poses)
        res = (VerifyResultC * max(n, 1))()
        order = np.zeros(n, np.int32)
        _check(self._h, lib().tdv_verify_poses_mesh_dev(self._h, _ptr(d_vertices), int(n_vertices), _ptr(d_triangles), int(n_triangles), _ptr(t), n,
                                                        _ptr(d_raw), int(w), int(h), C.c_float(scale), C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                                        C.c_float(cy), C.byref(mesh_verify_params(**params)), res, _ptr(order)),
               "tdv_verify_poses_mesh_dev")
        return _verify_results(res, n), order

    def render_depth_mesh(self, vertices, triangles, pose, w, h, fx, fy, cx, cy, **params):
        """tdv_render_depth_mesh: the rendered depth of the mesh at one pose, float32 [h, w], 0 where nothing rendered - per pixel the
        minimum interpolated depth over the triangles that cover its centre (the z-buffer verify_poses_mesh classifies)."""
        vtx, tri = _mesh(vertices, triangles)
        out = np.zeros((int(h), int(w)), np.float32)
        n = C.c_int()
        _check(self._h, lib().tdv_render_depth_mesh(self._h, _ptr(vtx), len(vtx), _ptr(tri), len(tri), _ptr(to_colmajor16(pose)), int(w), int(h),
                                                    C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                                    C.byref(mesh_verify_params(**params)), _ptr(out), C.byref(n)), "tdv_render_depth_mesh")
        return out

    def render_depth_mesh_dev(self, d_vertices, n_vertices, d_triangles, n_triangles, pose, w, h, fx, fy, cx, cy, d_out_depth, **params):
        """tdv_render_depth_mesh_dev: render_depth_mesh from a device mesh into the device image d_out_depth (float[w h]); returns
        n_rendered."""
        n = C.c_int()
        _check(self._h, lib().tdv_render_depth_mesh_dev(self._h, _ptr(d_vertices), int(n_vertices), _ptr(d_triangles), int(n_triangles),
                                                        _ptr(to_colmajor16(pose)), int(w), int(h), C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                                        C.c_float(cy), C.byref(mesh_verify_params(**params)), _ptr(d_out_depth), C.byref(n)),
               "tdv_render_depth_mesh_dev")
        return n.value

    # ---------------------------------------------------------------- mesh sampling (include/tdv_hip.h: tdv_mesh_sample_points)
    def mesh_sample(self, vertices, triangles, n_samples, attr=None, seed=0, first_sample=0):
        """tdv_mesh_sample_points, every output: the result's fields and surface_area, xyz float32[n_sampled, 3], normals float32[n_sampled, 3]
        (the faces' outward unit normals), triangle int32[n_sampled], bary float32[n_sampled, 2] and attr float32[n_sampled, width] or None.
        attr: one row of floats per vertex (vertex normals, colours), interpolated at every sample."""
        vtx, tri = _mesh(vertices, triangles)
        width = 0
        if attr is not None:
            attr = _f32(attr)
            if attr.ndim != 2 or len(attr) != len(vtx):
                raise ValueError("tdv_mesh_sample_points: one attr row per vertex")
            width = attr.shape[1]
        res = MeshSampleResultC()
        m1 = max(int(n_samples), 1)
        xyz = np.zeros((m1, 3), np.float32); nrm = np.zeros((m1, 3), np.float32); idx = np.zeros(m1, np.int32); bary = np.zeros((m1, 2), np.float32)
        cols = None if attr is None else np.zeros((m1, max(width, 1)), np.float32)
        p = mesh_sample_params(seed=seed, first_sample=first_sample)
        _check(self._h, lib().tdv_mesh_sample_points(self._h, _ptr(vtx), len(vtx), _ptr(tri), len(tri), _ptr(attr), width, int(n_samples),
                                                     C.byref(p), C.byref(res), _ptr(xyz), _ptr(nrm), _ptr(idx), _ptr(bary), _ptr(cols)),
               "tdv_mesh_sample_points")
        m = res.n_sampled
        return dict(_mesh_sample_result(res), xyz=xyz[:m], normals=nrm[:m], triangle=idx[:m], bary=bary[:m],
                    attr=None if cols is None else cols.reshape(-1)[:m * width].reshape(m, width))

    def sample_points_uniformly(self, vertices, triangles, number_of_points, seed=0):
        """Open3D's TriangleMesh.sample_points_uniformly: (points, normals), the normals the faces' own."""
        r = self.mesh_sample(vertices, triangles, number_of_points, seed=seed)
        return r["xyz"], r["normals"]

    def mesh_sample_dev(self, d_vertices, n_vertices, d_triangles, n_triangles, n_samples, d_attr=None, attr_width=0, seed=0, first_sample=0,
                        d_out_xyz=None, d_out_normals=None, d_out_triangle=None, d_out_bary=None, d_out_attr=None):
        """tdv_mesh_sample_points_dev on device pointers: the result dict.  d_out_xyz and d_out_normals (3 floats), d_out_triangle (int32),
        d_out_bary (2 floats) and d_out_attr (attr_width floats) per sample, each of n_samples entries, are optional; n_sampled rows are
        written.  One read-back."""
        res = MeshSampleResultC()
        p = mesh_sample_params(seed=seed, first_sample=first_sample)
        _check(self._h, lib().tdv_mesh_sample_points_dev(self._h, _ptr(d_vertices), int(n_vertices), _ptr(d_triangles), int(n_triangles), _ptr(d_attr),
                                                         int(attr_width), int(n_samples), C.byref(p), C.byref(res), _ptr(d_out_xyz),
                                                         _ptr(d_out_normals), _ptr(d_out_triangle), _ptr(d_out_bary), _ptr(d_out_attr)),
               "tdv_mesh_sample_points_dev")
        return _mesh_sample_result(res)

    def mesh_model_dev(self, d_vertices, n_vertices, d_triangles, n_triangles, n_points, d_out_xyz, d_out_normals, oversample=8, seed=0):
        """The even-spread model of a mesh, on the device: oversample * n_points uniform samples (mesh_sample_dev) thinned to n_points by
        fps_dev from row 0, the face normals as the companion rows - sample_points_poisson_disk's oversample-and-eliminate with the
        exact-count sampler.  d_out_xyz and d_out_normals (3 n_points floats each) go into ppf_model_dev and the ICP entry points as they
        stand.  Returns the fps result dict (n_selected rows are written); the oversampled rows live in torch buffers for the call."""
        import torch
        n_over = int(oversample) * int(n_points)
        if oversample < 1 or n_points < 0 or n_over > TDV_FPS_MAX_POINTS:
            raise ValueError("mesh_model: oversample >= 1 and oversample * n_points <= TDV_FPS_MAX_POINTS")
        dev = torch.device("cuda", self.device)
        over = torch.empty((2, max(n_over, 1), 3), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()         # (a reused block: what torch last did with it is over before the ctx's stream writes it)
        s = self.mesh_sample_dev(d_vertices, n_vertices, d_triangles, n_triangles, n_over, seed=seed, d_out_xyz=over[0].data_ptr(),
                                 d_out_normals=over[1].data_ptr())
        return self.fps_dev(over[0].data_ptr(), s["n_sampled"], n_points, 0, over[1].data_ptr(), 3, None, None, d_out_xyz, d_out_normals)

    def mesh_model(self, vertices, triangles, n_points, oversample=8, seed=0):
        """mesh_model_dev on host arrays: (points float32[m, 3], normals float32[m, 3], fps result dict), m = n_points unless the mesh has
        no usable triangle."""
        import torch
        vtx, tri = _mesh(vertices, triangles)
        dev = torch.device("cuda", self.device)
        d_v = _upload_rows(self.device, vtx)
        d_t = torch.from_numpy(tri if len(tri) else np.zeros((1, 3), np.int32)).to(dev)
        out = torch.zeros((2, max(int(n_points), 1), 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        r = self.mesh_model_dev(d_v.data_ptr(), len(vtx), d_t.data_ptr(), len(tri), n_points, out[0].data_ptr(), out[1].data_ptr(), oversample, seed)
        self.synchronize()
        h = out.cpu().numpy()
        m = r["n_selected"]
        return h[0, :m].copy(), h[1, :m].copy(), r

    # ---------------------------------------------------------------- TSDF fusion (include/tdv_hip.h: tdv_tsdf_integrate_dev)
    tsdf_params = staticmethod(tsdf_params)

    def tsdf_volume(self, origin, voxel_length, dims):
        """A fresh volume: (the tdv_tsdf_volume struct, its device buffer - a torch float32 tensor [nx*ny*nz, 2] of (tsdf, weight) pairs, voxel
        (i, j, k) at row (k*ny + j)*nx + i, every pair (1, 0)).  The caller owns the tensor, as it owns tdv_ppf_model_dev's table."""
        import torch
        vol = tsdf_volume_struct(origin, voxel_length, dims)
        nbytes = int(lib().tdv_tsdf_volume_bytes(C.byref(vol)))
        if nbytes == 0:
            raise ValueError("tsdf_volume: sides in [1, TDV_TSDF_MAX_SIDE], at most TDV_TSDF_MAX_VOXELS voxels, voxel_length > 0")
        buf = torch.empty((nbytes // 8, 2), dtype=torch.float32, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(buf.device).synchronize()
        self.tsdf_reset_dev(vol, buf.data_ptr())
        self.synchronize()
        return vol, buf

    def tsdf_reset_dev(self, vol, d_volume):
        """tdv_tsdf_reset_dev: every pair of the volume becomes (1, 0)."""
        _check(self._h, lib().tdv_tsdf_reset_dev(self._h, C.byref(vol), _ptr(d_volume)), "tdv_tsdf_reset_dev")

    def tsdf_integrate_dev(self, vol, d_volume, d_raw, poses, w, h, scale, fx, fy, cx, cy, want_counts=True, **params):
        """tdv_tsdf_integrate_dev: the frames d_raw (uint16[n, h, w] on the device) taken at poses ([n, 4, 4], row-major) into the volume, in
        one pass.  Returns int64[n], the voxels each frame updated, or None with want_counts=False (no read-back)."""
        t, n = _poses16(poses)
        counts = np.zeros(n, np.int64) if want_counts else None
        _check(self._h, lib().tdv_tsdf_integrate_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_raw), n, int(w), int(h), C.c_float(scale),
                                                     C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), _ptr(t),
                                                     C.byref(tsdf_params(**params)), _ptr(counts)), "tdv_tsdf_integrate_dev")
        return counts

    def tsdf_extract_dev(self, vol, d_volume, d_out_xyz, d_out_normals, capacity, **params):
        """tdv_tsdf_extract_dev: the crossings of the volume into d_out_xyz and d_out_normals (optional), capacity rows each; returns
        (n, fits): n rows were written, or, fits False, n rows are needed and none was written."""
        n = C.c_int(-1)
        st = lib().tdv_tsdf_extract_dev(self._h, C.byref(vol), _ptr(d_volume), C.byref(tsdf_params(**params)), _ptr(d_out_xyz),
                                        _ptr(d_out_normals), int(capacity), C.byref(n))
        if st == -2 and n.value > int(capacity) >= 0:
            return n.value, False
        _check(self._h, st, "tdv_tsdf_extract_dev")
        return n.value, True

    def tsdf_integrate(self, volume, frames, poses, intrinsics, **params):
        """tsdf_integrate_dev on host frames (uint16[n, h, w]) into volume = tsdf_volume()'s pair; intrinsics = (scale, fx, fy, cx, cy)."""
        import torch
        frames = np.array(frames, np.uint16)                     # (a copy: torch wants a writable array)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        d_raw = torch.from_numpy(frames.view(np.int16) if frames.size else np.zeros((1, 1, 1), np.int16)).to(volume[1].device)
        torch.cuda.synchronize()
        counts = self.tsdf_integrate_dev(volume[0], volume[1].data_ptr(), d_raw.data_ptr(), poses, frames.shape[2], frames.shape[1], *intrinsics,
                                         **params)
        return counts

    def tsdf_extract(self, volume, normals=True, **params):
        """The crossings of volume = tsdf_volume()'s pair: (xyz float32[n, 3], normals float32[n, 3] or None)."""
        import torch
        n, _ = self.tsdf_extract_dev(volume[0], volume[1].data_ptr(), None, None, 0, **params)
        out = torch.zeros((2 if normals else 1, max(n, 1), 3), dtype=torch.float32, device=volume[1].device)
        torch.cuda.synchronize()
        self.tsdf_extract_dev(volume[0], volume[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr() if normals else None, n, **params)
        self.synchronize()
        h = out.cpu().numpy()
        return h[0, :n].copy(), (h[1, :n].copy() if normals else None)

    def tsdf_fuse(self, frames, poses, intrinsics, volume, normals=True, **params):
        """tdv_tsdf_fuse on host arrays: frames uint16[n, h, w] taken at poses [n, 4, 4] with intrinsics = (scale, fx, fy, cx, cy), fused in
        volume = (origin, voxel_length, dims) or a TsdfVolumeC: (xyz float32[m, 3], normals float32[m, 3] or None).  The first call asks for the
        count, the second brings the rows."""
        vol = volume if isinstance(volume, TsdfVolumeC) else tsdf_volume_struct(*volume)
        frames = np.ascontiguousarray(frames, np.uint16)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        t, n = _poses16(poses)
        if n != len(frames):
            raise ValueError("tdv_tsdf_fuse: one pose per frame")
        scale, fx, fy, cx, cy = intrinsics
        p = tsdf_params(**params)

        def call(xyz, nrm, capacity):
            m = C.c_int(-1)
            st = lib().tdv_tsdf_fuse(self._h, C.byref(vol), _ptr(frames), n, frames.shape[2], frames.shape[1], C.c_float(scale), C.c_float(fx),
                                     C.c_float(fy), C.c_float(cx), C.c_float(cy), _ptr(t), C.byref(p), _ptr(xyz), _ptr(nrm), capacity, C.byref(m))
            if not (st == -2 and m.value > capacity):
                _check(self._h, st, "tdv_tsdf_fuse")
            return m.value

        m = call(None, None, 0)
        xyz = np.zeros((m, 3), np.float32)
        nrm = np.zeros((m, 3), np.float32) if normals else None
        if m:
            call(xyz, nrm, m)
        return xyz, nrm

    def tsdf_extract_mesh_dev(self, vol, d_volume, d_out_vertices, d_out_normals, vertex_capacity, d_out_triangles, triangle_capacity, **params):
        """tdv_tsdf_extract_mesh_dev: the volume's surface as a triangle mesh whose vertices are tsdf_extract_dev's rows - vertices and
        normals (optional) into d_out_vertices / d_out_normals (vertex_capacity rows of 3 floats), the triangles into d_out_triangles
        (triangle_capacity rows of 3 int32).  Returns (n_vertices, n_triangles, fits): with fits False that many rows are needed and
        nothing was written."""
        nv, nt = C.c_int(-1), C.c_int(-1)
        st = lib().tdv_tsdf_extract_mesh_dev(self._h, C.byref(vol), _ptr(d_volume), C.byref(tsdf_params(**params)), _ptr(d_out_vertices),
                                             _ptr(d_out_normals), int(vertex_capacity), C.byref(nv), _ptr(d_out_triangles), int(triangle_capacity),
                                             C.byref(nt))
        if st == -2 and ((nv.value > int(vertex_capacity) >= 0) or (nt.value > int(triangle_capacity) >= 0)):
            return nv.value, nt.value, False
        _check(self._h, st, "tdv_tsdf_extract_mesh_dev")
        return nv.value, nt.value, True

    def tsdf_extract_mesh(self, volume, normals=True, compact=False, **params):
        """The mesh of volume = tsdf_volume()'s pair: (vertices float32[n, 3], normals float32[n, 3] or None, triangles int32[m, 3]).  The
        vertices are tsdf_extract's rows; compact=True drops those no triangle refers to (mesh_compact)."""
        import torch
        vol, buf = volume
        nv, nt, _ = self.tsdf_extract_mesh_dev(vol, buf.data_ptr(), None, None, 0, None, 0, **params)
        out = torch.zeros((2 if normals else 1, max(nv, 1), 3), dtype=torch.float32, device=buf.device)
        tri = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device=buf.device)
        torch.cuda.synchronize()
        self.tsdf_extract_mesh_dev(vol, buf.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if normals else None, nv, tri.data_ptr(), nt, **params)
        self.synchronize()
        h = out.cpu().numpy()
        mesh = h[0, :nv].copy(), (h[1, :nv].copy() if normals else None), tri.cpu().numpy()[:nt].copy()
        return mesh_compact(*mesh) if compact else mesh

    def tsdf_fuse_mesh(self, frames, poses, intrinsics, volume, normals=True, compact=False, **params):
        """tdv_tsdf_fuse_mesh on host arrays (tsdf_fuse's arguments): (vertices, normals or None, triangles int32[m, 3]).  The first call asks
        for the counts, the second brings the rows."""
        vol = volume if isinstance(volume, TsdfVolumeC) else tsdf_volume_struct(*volume)
        frames = np.ascontiguousarray(frames, np.uint16)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        t, n = _poses16(poses)
        if n != len(frames):
            raise ValueError("tdv_tsdf_fuse_mesh: one pose per frame")
        scale, fx, fy, cx, cy = intrinsics
        p = tsdf_params(**params)

        def call(xyz, nrm, vcap, tri, tcap):
            nv, nt = C.c_int(-1), C.c_int(-1)
            st = lib().tdv_tsdf_fuse_mesh(self._h, C.byref(vol), _ptr(frames), n, frames.shape[2], frames.shape[1], C.c_float(scale), C.c_float(fx),
                                          C.c_float(fy), C.c_float(cx), C.c_float(cy), _ptr(t), C.byref(p), _ptr(xyz), _ptr(nrm), vcap, C.byref(nv),
                                          _ptr(tri), tcap, C.byref(nt))
            if not (st == -2 and (nv.value > vcap or nt.value > tcap)):
                _check(self._h, st, "tdv_tsdf_fuse_mesh")
            return nv.value, nt.value

        nv, nt = call(None, None, 0, None, 0)
        xyz = np.zeros((nv, 3), np.float32)
        nrm = np.zeros((nv, 3), np.float32) if normals else None
        tri = np.zeros((nt, 3), np.int32)
        if nv:
            call(xyz, nrm, nv, tri if nt else None, nt)
        return mesh_compact(xyz, nrm, tri) if compact else (xyz, nrm, tri)

    # ---------------------------------------------------------------- coloured TSDF fusion (include/tdv_hip.h: tdv_tsdf_integrate_color_dev)
    def tsdf_color_volume(self, vol):
        """A fresh colour volume for vol (tsdf_volume()'s struct): a torch float32 tensor [nx*ny*nz, 4] of (r, g, b, wc) quads on the
        device, voxel (i, j, k) at row (k*ny + j)*nx + i, every quad (0, 0, 0, 0).  The caller owns the tensor."""
        import torch
        nbytes = int(lib().tdv_tsdf_color_bytes(C.byref(vol)))
        if nbytes == 0:
            raise ValueError("tsdf_color_volume: sides in [1, TDV_TSDF_MAX_SIDE], at most TDV_TSDF_MAX_VOXELS voxels, voxel_length > 0")
        buf = torch.empty((nbytes // 16, 4), dtype=torch.float32, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(buf.device).synchronize()
        self.tsdf_color_reset_dev(vol, buf.data_ptr())
        self.synchronize()
        return buf

    def tsdf_color_reset_dev(self, vol, d_color):
        """tdv_tsdf_color_reset_dev: every quad of the colour volume becomes (0, 0, 0, 0)."""
        _check(self._h, lib().tdv_tsdf_color_reset_dev(self._h, C.byref(vol), _ptr(d_color)), "tdv_tsdf_color_reset_dev")

    def tsdf_integrate_color_dev(self, vol, d_volume, d_color, d_raw, d_bgr, poses, w, h, scale, fx, fy, cx, cy, want_counts=True, **params):
        """tdv_tsdf_integrate_color_dev: tsdf_integrate_dev with the colour volume d_color and the frames' images d_bgr (uint8[n, h, w, 3],
        B, G, R, on the device).  Returns int64[n], the voxels each frame updated, or None with want_counts=False (no read-back)."""
        t, n = _poses16(poses)
        counts = np.zeros(n, np.int64) if want_counts else None
        _check(self._h, lib().tdv_tsdf_integrate_color_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_color), _ptr(d_raw), _ptr(d_bgr), n, int(w),
                                                           int(h), *self._cam(scale, fx, fy, cx, cy), _ptr(t), C.byref(tsdf_params(**params)),
                                                           _ptr(counts)), "tdv_tsdf_integrate_color_dev")
        return counts

    def tsdf_extract_color_dev(self, vol, d_volume, d_color, d_out_xyz, d_out_normals, d_out_rgb, capacity, **params):
        """tdv_tsdf_extract_color_dev: tsdf_extract_dev with the rows' colours (float32 RGB in [0, 1]) into d_out_rgb; returns (n, fits)."""
        n = C.c_int(-1)
        st = lib().tdv_tsdf_extract_color_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_color), C.byref(tsdf_params(**params)), _ptr(d_out_xyz),
                                              _ptr(d_out_normals), _ptr(d_out_rgb), int(capacity), C.byref(n))
        if st == -2 and n.value > int(capacity) >= 0:
            return n.value, False
        _check(self._h, st, "tdv_tsdf_extract_color_dev")
        return n.value, True

    def tsdf_extract_mesh_color_dev(self, vol, d_volume, d_color, d_out_vertices, d_out_normals, d_out_rgb, vertex_capacity, d_out_triangles,
                                    triangle_capacity, **params):
        """tdv_tsdf_extract_mesh_color_dev: tsdf_extract_mesh_dev with the vertices' colours into d_out_rgb; returns (n_vertices,
        n_triangles, fits)."""
        nv, nt = C.c_int(-1), C.c_int(-1)
        st = lib().tdv_tsdf_extract_mesh_color_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_color), C.byref(tsdf_params(**params)),
                                                   _ptr(d_out_vertices), _ptr(d_out_normals), _ptr(d_out_rgb), int(vertex_capacity), C.byref(nv),
                                                   _ptr(d_out_triangles), int(triangle_capacity), C.byref(nt))
        if st == -2 and ((nv.value > int(vertex_capacity) >= 0) or (nt.value > int(triangle_capacity) >= 0)):
            return nv.value, nt.value, False
        _check(self._h, st, "tdv_tsdf_extract_mesh_color_dev")
        return nv.value, nt.value, True

    def tsdf_integrate_color(self, volume, color, frames, images, poses, intrinsics, **params):
        """tsdf_integrate_color_dev on host frames (uint16[n, h, w]) and images (uint8[n, h, w, 3], B, G, R) into volume = tsdf_volume()'s
        pair and color = tsdf_color_volume()'s tensor; intrinsics = (scale, fx, fy, cx, cy)."""
        import torch
        frames = np.array(frames, np.uint16)                     # (a copy: torch wants a writable array)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        images = np.array(images, np.uint8).reshape(frames.shape + (3,))
        d_raw = torch.from_numpy(frames.view(np.int16) if frames.size else np.zeros((1, 1, 1), np.int16)).to(volume[1].device)
        d_bgr = torch.from_numpy(images if images.size else np.zeros((1, 1, 1, 3), np.uint8)).to(volume[1].device)
        torch.cuda.synchronize()
        return self.tsdf_integrate_color_dev(volume[0], volume[1].data_ptr(), color.data_ptr(), d_raw.data_ptr(), d_bgr.data_ptr(), poses,
                                             frames.shape[2], frames.shape[1], *intrinsics, **params)

    def tsdf_extract_color(self, volume, color, normals=True, **params):
        """The coloured crossings of volume = tsdf_volume()'s pair and color = tsdf_color_volume()'s tensor: (xyz float32[n, 3], normals
        float32[n, 3] or None, rgb float32[n, 3] in [0, 1] - what color_gradients and colored_icp take)."""
        import torch
        n, _ = self.tsdf_extract_color_dev(volume[0], volume[1].data_ptr(), color.data_ptr(), None, None, None, 0, **params)
        out = torch.zeros((3, max(n, 1), 3), dtype=torch.float32, device=volume[1].device)
        torch.cuda.synchronize()
        self.tsdf_extract_color_dev(volume[0], volume[1].data_ptr(), color.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if normals else None,
                                    out[2].data_ptr(), n, **params)
        self.synchronize()
        h = out.cpu().numpy()
        return h[0, :n].copy(), (h[1, :n].copy() if normals else None), h[2, :n].copy()

    def tsdf_extract_mesh_color(self, volume, color, normals=True, compact=False, **params):
        """The coloured mesh of volume and color: (vertices float32[n, 3], normals float32[n, 3] or None, triangles int32[m, 3], rgb
        float32[n, 3]).  compact=True drops the vertices no triangle refers to, and their colours with them."""
        import torch
        vol, buf = volume
        nv, nt, _ = self.tsdf_extract_mesh_color_dev(vol, buf.data_ptr(), color.data_ptr(), None, None, None, 0, None, 0, **params)
        out = torch.zeros((3, max(nv, 1), 3), dtype=torch.float32, device=buf.device)
        tri = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device=buf.device)
        torch.cuda.synchronize()
        self.tsdf_extract_mesh_color_dev(vol, buf.data_ptr(), color.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if normals else None,
                                         out[2].data_ptr(), nv, tri.data_ptr(), nt, **params)
        self.synchronize()
        h = out.cpu().numpy()
        return _colored_mesh(h[0, :nv].copy(), (h[1, :nv].copy() if normals else None), tri.cpu().numpy()[:nt].copy(), h[2, :nv].copy(), compact)

    def tsdf_fuse_color(self, frames, images, poses, intrinsics, volume, normals=True, triangles=False, compact=False, **params):
        """tdv_tsdf_fuse_color on host arrays: frames uint16[n, h, w] and images uint8[n, h, w, 3] (B, G, R) taken at poses [n, 4, 4] with
        intrinsics = (scale, fx, fy, cx, cy), fused in volume = (origin, voxel_length, dims) or a TsdfVolumeC.  Returns (xyz float32[m, 3],
        normals float32[m, 3] or None, rgb float32[m, 3]); with triangles=True (vertices, normals or None, triangles int32[t, 3], rgb), and
        compact=True then drops the vertices no triangle refers to.  The first call asks for the counts, the second brings the rows."""
        vol = volume if isinstance(volume, TsdfVolumeC) else tsdf_volume_struct(*volume)
        frames = np.ascontiguousarray(frames, np.uint16)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        images = np.ascontiguousarray(images, np.uint8).reshape(frames.shape + (3,))
        t, n = _poses16(poses)
        if n != len(frames):
            raise ValueError("tdv_tsdf_fuse_color: one pose per frame")
        scale, fx, fy, cx, cy = intrinsics
        p = tsdf_params(**params)

        def call(xyz, nrm, rgb, vcap, tri, tcap):
            nv, nt = C.c_int(-1), C.c_int(0)
            st = lib().tdv_tsdf_fuse_color(self._h, C.byref(vol), _ptr(frames), _ptr(images), n, frames.shape[2], frames.shape[1],
                                           *self._cam(scale, fx, fy, cx, cy), _ptr(t), C.byref(p), _ptr(xyz), _ptr(nrm), _ptr(rgb), vcap, C.byref(nv),
                                           _ptr(tri), tcap, C.byref(nt) if triangles else None)
            if not (st == -2 and (nv.value > vcap or nt.value > tcap)):
                _check(self._h, st, "tdv_tsdf_fuse_color")
            return nv.value, nt.value

        nv, nt = call(None, None, None, 0, None, 0)
        xyz, rgb = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.float32)
        nrm = np.zeros((nv, 3), np.float32) if normals else None
        tri = np.zeros((nt, 3), np.int32)
        if nv:
            call(xyz, nrm, rgb, nv, tri if nt else None, nt)
        return _colored_mesh(xyz, nrm, tri, rgb, compact) if triangles else (xyz, nrm, rgb)

    # ---------------------------------------------------------------- depth odometry (include/tdv_hip.h: tdv_depth_odometry_dev)
    odometry_params = staticmethod(odometry_params)

    @staticmethod
    def _cam(scale, fx, fy, cx, cy):
        return C.c_float(scale), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy)

    def depth_maps_dev(self, d_raw, w, h, scale, fx, fy, cx, cy, d_vertex_map=None, d_normal_map=None, d_out_xyz=None, d_out_normals=None,
                       capacity=0, want_count=True, **params):
        """tdv_depth_maps_dev: the vertex and normal maps (device, w*h*3 floats each) of the frame d_raw (uint16[h, w] on the device) and the
        rows of the pixels that have a normal into d_out_xyz / d_out_normals (capacity rows); every output optional.  Returns (n, fits): n
        rows were written, or, fits False, n rows are needed and nothing was written; (None, True) with want_count=False (no read-back)."""
        n = C.c_int(-1)
        st = lib().tdv_depth_maps_dev(self._h, _ptr(d_raw), int(w), int(h), *self._cam(scale, fx, fy, cx, cy), C.byref(odometry_params(**params)),
                                      _ptr(d_vertex_map), _ptr(d_normal_map), _ptr(d_out_xyz), _ptr(d_out_normals), int(capacity),
                                      C.byref(n) if want_count else None)
        if want_count and st == -2 and n.value > int(capacity) >= 0:
            return n.value, False
        _check(self._h, st, "tdv_depth_maps_dev")
        return (n.value if want_count else None), True

    def depth_maps(self, frame, intrinsics, **params):
        """tdv_depth_maps on a host frame (uint16[h, w]), intrinsics = (scale, fx, fy, cx, cy): dict(vertex_map float32[h, w, 3], normal_map
        float32[h, w, 3], xyz float32[n, 3], normals float32[n, 3]) - the maps and, in pixel order, the rows of the pixels with a normal.
        The first call asks for the count, the second brings everything."""
        frame = np.ascontiguousarray(frame, np.uint16)
        h, w = frame.shape
        p = odometry_params(**params)

        def call(vm, nm, xyz, nrm, capacity):
            n = C.c_int(-1)
            st = lib().tdv_depth_maps(self._h, _ptr(frame), w, h, *self._cam(*intrinsics), C.byref(p), _ptr(vm), _ptr(nm), _ptr(xyz), _ptr(nrm),
                                      capacity, C.byref(n))
            if not (st == -2 and n.value > capacity):
                _check(self._h, st, "tdv_depth_maps")
            return n.value

        n = call(None, None, None, None, 0)
        out = dict(vertex_map=np.zeros((h, w, 3), np.float32), normal_map=np.zeros((h, w, 3), np.float32), xyz=np.zeros((n, 3), np.float32),
                   normals=np.zeros((n, 3), np.float32))
        call(out["vertex_map"], out["normal_map"], out["xyz"] if n else None, out["normals"] if n else None, n)
        return out

    def depth_odometry_terms_dev(self, d_raw_src, d_raw_tgt, w, h, scale, fx, fy, cx, cy, T, level, **params):
        """tdv_depth_odometry_terms_dev: (float64[29], n_valid_src) - O7's sums for the pose T ([4, 4] row-major) at one level."""
        sums = np.zeros(ODOM_TERMS, np.float64)
        n = C.c_int(-1)
        _check(self._h, lib().tdv_depth_odometry_terms_dev(self._h, _ptr(d_raw_src), _ptr(d_raw_tgt), int(w), int(h), *self._cam(scale, fx, fy, cx, cy),
                                                           _ptr(to_colmajor16(T)), int(level), C.byref(odometry_params(**params)), _ptr(sums),
                                                           C.byref(n)), "tdv_depth_odometry_terms_dev")
        return sums, n.value

    def depth_odometry_dev(self, d_raw_src, d_raw_tgt, w, h, scale, fx, fy, cx, cy, T0=None, **params):
        """tdv_depth_odometry_dev: the motion that takes the source frame's camera coordinates to the target frame's, from T0 ([4, 4]
        row-major, None: the identity), as _odometry_result's dict."""
        r = OdometryResultC()
        _check(self._h, lib().tdv_depth_odometry_dev(self._h, _ptr(d_raw_src), _ptr(d_raw_tgt), int(w), int(h), *self._cam(scale, fx, fy, cx, cy),
                                                     None if T0 is None else _ptr(to_colmajor16(T0)), C.byref(odometry_params(**params)),
                                                     C.byref(r)), "tdv_depth_odometry_dev")
        return _odometry_result(r)

    def depth_odometry(self, src, tgt, intrinsics, T0=None, **params):
        """tdv_depth_odometry on host frames (uint16[h, w] each), intrinsics = (scale, fx, fy, cx, cy)."""
        src, tgt = np.ascontiguousarray(src, np.uint16), np.ascontiguousarray(tgt, np.uint16)
        if src.shape != tgt.shape or src.ndim != 2:
            raise ValueError("tdv_depth_odometry: two frames of one size")
        r = OdometryResultC()
        _check(self._h, lib().tdv_depth_odometry(self._h, _ptr(src), _ptr(tgt), src.shape[1], src.shape[0], *self._cam(*intrinsics),
                                                 None if T0 is None else _ptr(to_colmajor16(T0)), C.byref(odometry_params(**params)), C.byref(r)),
               "tdv_depth_odometry")
        return _odometry_result(r)

    def depth_odometry_sequence_dev(self, d_raw, n_frames, w, h, scale, fx, fy, cx, cy, init=None, **params):
        """tdv_depth_odometry_sequence_dev: frames d_raw (uint16[n, h, w] on the device), init ([n, 4, 4] row-major start poses of the pairs,
        entry 0 unused, or None).  Returns (poses float32[n, 4, 4] row-major - camera k in camera 0's frame, what tsdf_integrate_dev takes
        with pose_direction='source_onto_target' - and the pairs' results, entry 0 zeros)."""
        n = int(n_frames)
        t0 = None
        if init is not None:
            t0, m = _poses16(init)
            if m != n:
                raise ValueError("tdv_depth_odometry_sequence_dev: one start pose per frame")
        poses = np.zeros((max(n, 1), 16), np.float32)
        pairs = (OdometryResultC * max(n, 1))()
        _check(self._h, lib().tdv_depth_odometry_sequence_dev(self._h, _ptr(d_raw), n, int(w), int(h), *self._cam(scale, fx, fy, cx, cy), _ptr(t0),
                                                              C.byref(odometry_params(**params)), _ptr(poses), pairs),
               "tdv_depth_odometry_sequence_dev")
        return poses[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), [_odometry_result(pairs[k]) for k in range(n)]

    def depth_odometry_sequence(self, frames, intrinsics, init=None, **params):
        """depth_odometry_sequence_dev on host frames (uint16[n, h, w])."""
        import torch
        frames = np.array(frames, np.uint16)                     # (a copy: torch wants a writable array)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        d_raw = torch.from_numpy(frames.view(np.int16) if frames.size else np.zeros((1, 1, 1), np.int16)).to(torch.device("cuda", self.device))
        torch.cuda.synchronize()
        return self.depth_odometry_sequence_dev(d_raw.data_ptr(), len(frames), frames.shape[2], frames.shape[1], *intrinsics, init=init, **params)

    def depth_odometry_to_depth_dev(self, d_raw_src, d_depth_tgt, w, h, scale, fx, fy, cx, cy, T0=None, **params):
        """tdv_depth_odometry_to_depth_dev: depth_odometry_dev with the target as an f32 depth image on the device (float32[h, w], metres; rule
        O10) - a ray cast of the volume (tsdf_raycast_dev) or a rendering (render_depth_dev)."""
        r = OdometryResultC()
        _check(self._h, lib().tdv_depth_odometry_to_depth_dev(self._h, _ptr(d_raw_src), _ptr(d_depth_tgt), int(w), int(h),
                                                              *self._cam(scale, fx, fy, cx, cy), None if T0 is None else _ptr(to_colmajor16(T0)),
                                                              C.byref(odometry_params(**params)), C.byref(r)), "tdv_depth_odometry_to_depth_dev")
        return _odometry_result(r)

    def depth_odometry_to_depth(self, src, depth_tgt, intrinsics, T0=None, **params):
        """tdv_depth_odometry_to_depth on host arrays: src uint16[h, w], depth_tgt float32[h, w]; intrinsics = (scale, fx, fy, cx, cy)."""
        src, depth_tgt = np.ascontiguousarray(src, np.uint16), np.ascontiguousarray(depth_tgt, np.float32)
        if src.shape != depth_tgt.shape or src.ndim != 2:
            raise ValueError("tdv_depth_odometry_to_depth: a frame and a depth image of one size")
        r = OdometryResultC()
        _check(self._h, lib().tdv_depth_odometry_to_depth(self._h, _ptr(src), _ptr(depth_tgt), src.shape[1], src.shape[0], *self._cam(*intrinsics),
                                                          None if T0 is None else _ptr(to_colmajor16(T0)), C.byref(odometry_params(**params)),
                                                          C.byref(r)), "tdv_depth_odometry_to_depth")
        return _odometry_result(r)

    # ---------------------------------------------------------------- TSDF ray casting and tracking (include/tdv_hip.h: tdv_tsdf_raycast_dev)
    raycast_params = staticmethod(raycast_params)

    def tsdf_raycast_dev(self, vol, d_volume, pose, w, h, fx, fy, cx, cy, d_depth=None, d_vertex_map=None, d_normal_map=None, want_count=True,
                         **params):
        """tdv_tsdf_raycast_dev: the volume seen from pose ([4, 4] row-major, params' pose_direction) into d_depth (float32[h, w], 0 where a
        ray has no hit), d_vertex_map and d_normal_map (float32[h, w, 3], camera coordinates), every output optional.  params: the fields of
        tsdf_params and of raycast_params.  Returns the number of rays that hit, or None with want_count=False (no read-back)."""
        tp, rp = _split_params(params, "tsdf", "raycast")
        n = C.c_longlong(-1)
        _check(self._h, lib().tdv_tsdf_raycast_dev(self._h, C.byref(vol), _ptr(d_volume), int(w), int(h), C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                                   C.c_float(cy), _ptr(to_colmajor16(pose)), C.byref(tsdf_params(**tp)), C.byref(raycast_params(**rp)),
                                                   _ptr(d_depth), _ptr(d_vertex_map), _ptr(d_normal_map), C.byref(n) if want_count else None),
               "tdv_tsdf_raycast_dev")
        return n.value if want_count else None

    def tsdf_raycast_color_dev(self, vol, d_volume, d_color, pose, w, h, fx, fy, cx, cy, d_depth=None, d_vertex_map=None, d_normal_map=None,
                               d_rgb_map=None, want_count=True, **params):
        """tdv_tsdf_raycast_color_dev: tsdf_raycast_dev with the colour volume d_color and d_rgb_map (float32[h, w, 3], RGB, zeros where a
        ray has no hit or no colour; optional).  Returns the number of rays that hit, or None with want_count=False (no read-back)."""
        tp, rp = _split_params(params, "tsdf", "raycast")
        n = C.c_longlong(-1)
        _check(self._h, lib().tdv_tsdf_raycast_color_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_color), int(w), int(h), C.c_float(fx),
                                                         C.c_float(fy), C.c_float(cx), C.c_float(cy), _ptr(to_colmajor16(pose)),
                                                         C.byref(tsdf_params(**tp)), C.byref(raycast_params(**rp)), _ptr(d_depth),
                                                         _ptr(d_vertex_map), _ptr(d_normal_map), _ptr(d_rgb_map), C.byref(n) if want_count else None),
               "tdv_tsdf_raycast_color_dev")
        return n.value if want_count else None

    def tsdf_raycast_color(self, volume, color, pose, w, h, fx, fy, cx, cy, maps=True, **params):
        """tsdf_raycast_color_dev on volume = tsdf_volume()'s pair and color = tsdf_color_volume()'s tensor, the maps brought to the host:
        dict(depth float32[h, w], rgb_map float32[h, w, 3], vertex_map and normal_map float32[h, w, 3] - with maps - and n_hit)."""
        import torch
        vol, buf = volume
        w, h = int(w), int(h)
        out = torch.zeros((3, max(w * h, 1), 3), dtype=torch.float32, device=buf.device)
        depth = torch.zeros(max(w * h, 1), dtype=torch.float32, device=buf.device)
        torch.cuda.synchronize()
        n = self.tsdf_raycast_color_dev(vol, buf.data_ptr(), color.data_ptr(), pose, w, h, fx, fy, cx, cy, depth.data_ptr(),
                                        out[0].data_ptr() if maps else None, out[1].data_ptr() if maps else None, out[2].data_ptr(), **params)
        self.synchronize()
        m = out.cpu().numpy()[:, :w * h].reshape(3, h, w, 3)
        res = dict(depth=depth.cpu().numpy()[:w * h].reshape(h, w).copy(), rgb_map=m[2].copy(), n_hit=n)
        if maps:
            res.update(vertex_map=m[0].copy(), normal_map=m[1].copy())
        return res

    def tsdf_raycast(self, volume, pose, w, h, fx, fy, cx, cy, maps=True, **params):
        """tdv_tsdf_raycast on a host volume: volume = (vol, buf) with vol = (origin, voxel_length, dims) or a TsdfVolumeC and buf float32
        [nz, ny, nx, 2] (or anything of nx*ny*nz pairs).  Returns dict(depth float32[h, w], vertex_map and normal_map float32[h, w, 3] - with
        maps - and n_hit)."""
        vol, buf = volume
        vol = vol if isinstance(vol, TsdfVolumeC) else tsdf_volume_struct(*vol)
        buf = np.ascontiguousarray(buf, np.float32)
        if buf.size != 2 * vol.nx * vol.ny * vol.nz:
            raise ValueError("tdv_tsdf_raycast: a volume of nx*ny*nz pairs")
        tp, rp = _split_params(params, "tsdf", "raycast")
        w, h = int(w), int(h)
        out = dict(depth=np.zeros((h, w), np.float32))
        if maps:
            out.update(vertex_map=np.zeros((h, w, 3), np.float32), normal_map=np.zeros((h, w, 3), np.float32))
        n = C.c_longlong(-1)
        _check(self._h, lib().tdv_tsdf_raycast(self._h, C.byref(vol), _ptr(buf), w, h, C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                               _ptr(to_colmajor16(pose)), C.byref(tsdf_params(**tp)), C.byref(raycast_params(**rp)),
                                               _ptr(out["depth"]), _ptr(out.get("vertex_map")), _ptr(out.get("normal_map")), C.byref(n)),
               "tdv_tsdf_raycast")
        out["n_hit"] = n.value
        return out

    @staticmethod
    def _track_params(tsdf, ray, odom):
        """The three parameter structs of a tracking call from three dicts (None: the defaults); tracking's poses are the camera's pose in
        the volume's frame, so pose_direction defaults to 'source_onto_target' here."""
        return tsdf_params(**dict(dict(pose_direction="source_onto_target"), **(tsdf or {}))), raycast_params(**(ray or {})), \
            odometry_params(**(odom or {}))

    def tsdf_track_dev(self, vol, d_volume, d_raw, guess, w, h, scale, fx, fy, cx, cy, tsdf=None, ray=None, odom=None):
        """tdv_tsdf_track_dev: the raw frame d_raw (uint16[h, w] on the device) tracked against the volume from guess ([4, 4] row-major, the
        camera's pose in the volume's frame).  tsdf, ray, odom: dicts of tsdf_params', raycast_params' and odometry_params' fields.  Returns
        dict(pose [4, 4] row-major, odom, n_hit)."""
        tp, rp, op = self._track_params(tsdf, ray, odom)
        r = TsdfTrackResultC()
        _check(self._h, lib().tdv_tsdf_track_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_raw), int(w), int(h), *self._cam(scale, fx, fy, cx, cy),
                                                 _ptr(to_colmajor16(guess)), C.byref(tp), C.byref(rp), C.byref(op), C.byref(r)), "tdv_tsdf_track_dev")
        return _track_result(r)

    def tsdf_track(self, volume, frame, guess, intrinsics, tsdf=None, ray=None, odom=None):
        """tsdf_track_dev on a host frame (uint16[h, w]) against volume = tsdf_volume()'s pair; intrinsics = (scale, fx, fy, cx, cy)."""
        import torch
        frame = np.array(frame, np.uint16)                       # (a copy: torch wants a writable array)
        d_raw = torch.from_numpy(frame.view(np.int16) if frame.size else np.zeros((1, 1), np.int16)).to(volume[1].device)
        torch.cuda.synchronize()
        return self.tsdf_track_dev(volume[0], volume[1].data_ptr(), d_raw.data_ptr(), guess, frame.shape[1], frame.shape[0], *intrinsics,
                                   tsdf=tsdf, ray=ray, odom=odom)

    def tsdf_track_sequence_dev(self, vol, d_volume, d_raw, n_frames, w, h, scale, fx, fy, cx, cy, pose0=None, tsdf=None, ray=None, odom=None):
        """tdv_tsdf_track_sequence_dev: frames d_raw (uint16[n, h, w] on the device) tracked against and fused into the volume one after the
        other, frame 0 at pose0 ([4, 4] row-major, None: the identity).  Returns (poses float32[n, 4, 4] row-major, the frames' results as
        tsdf_track_dev's dicts, entry 0 holding pose0 and zeros).  One read-back per frame."""
        n = int(n_frames)
        tp, rp, op = self._track_params(tsdf, ray, odom)
        poses = np.zeros((max(n, 1), 16), np.float32)
        res = (TsdfTrackResultC * max(n, 1))()
        _check(self._h, lib().tdv_tsdf_track_sequence_dev(self._h, C.byref(vol), _ptr(d_volume), _ptr(d_raw), n, int(w), int(h),
                                                          *self._cam(scale, fx, fy, cx, cy), None if pose0 is None else _ptr(to_colmajor16(pose0)),
                                                          C.byref(tp), C.byref(rp), C.byref(op), _ptr(poses), res), "tdv_tsdf_track_sequence_dev")
        return poses[:n].reshape(n, 4, 4).transpose(0, 2, 1).copy(), [_track_result(res[k]) for k in range(n)]

    def tsdf_track_sequence(self, volume, frames, intrinsics, pose0=None, tsdf=None, ray=None, odom=None):
        """tsdf_track_sequence_dev on host frames (uint16[n, h, w]) into volume = tsdf_volume()'s pair."""
        import torch
        frames = np.array(frames, np.uint16)                     # (a copy: torch wants a writable array)
        frames = frames.reshape((-1,) + frames.shape[-2:])
        d_raw = torch.from_numpy(frames.view(np.int16) if frames.size else np.zeros((1, 1, 1), np.int16)).to(volume[1].device)
        torch.cuda.synchronize()
        return self.tsdf_track_sequence_dev(volume[0], volume[1].data_ptr(), d_raw.data_ptr(), len(frames), frames.shape[2], frames.shape[1],
                                            *intrinsics, pose0=pose0, tsdf=tsdf, ray=ray, odom=odom)

    # ---------------------------------------------------------------- PPF matching (include/tdv_hip.h: tdv_ppf_match)
    def ppf_model_bytes(self, nt, **params):
        b = C.c_size_t()
        _check(self._h, lib().tdv_ppf_model_bytes(int(nt), C.byref(ppf_params(**params)), C.byref(b)), "tdv_ppf_model_bytes")
        return b.value

    def ppf_model_dev(self, d_tgt, d_tgt_normals, nt, d_model, model_bytes, **params):
        """tdv_ppf_model_dev: the table of the model into d_model (device, model_bytes); returns the info dict tdv_ppf_match_dev takes."""
        info = PpfModelInfoC()
        _check(self._h, lib().tdv_ppf_model_dev(self._h, _ptr(d_tgt), _ptr(d_tgt_normals), int(nt), C.byref(ppf_params(**params)), _ptr(d_model),
                                                C.c_size_t(model_bytes), C.byref(info)), "tdv_ppf_model_dev")
        return _fields_dict(info)

    def ppf_model(self, tgt, tgt_normals, **params):
        """The model table of host arrays, parsed from the buffer (rule 4's layout): dict(diameter, distance_step, n_pairs, n_keys, nt,
        offsets int32[n_keys + 1], pair uint32[n_pairs] (i * nt + j), alpha_bits uint32[n_pairs], key uint32[n_pairs] - the key of every
        entry, read off the offsets)."""
        import torch
        tgt = np.array(tgt, np.float32).reshape(-1, 3); tn = np.array(tgt_normals, np.float32).reshape(-1, 3)     # (copies: torch wants writable arrays)
        nt = len(tgt)
        nbytes = self.ppf_model_bytes(nt, **params)
        dev = torch.device("cuda", self.device)
        d_t, d_n = _upload_rows(self.device, tgt), _upload_rows(self.device, tn)
        buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        info = self.ppf_model_dev(d_t.data_ptr(), d_n.data_ptr(), nt, buf.data_ptr(), nbytes, **params)
        w = buf.cpu().numpy().view(np.uint32)
        nk, npairs, cap = info["n_keys"], info["n_pairs"], nt * (nt - 1) if nt >= 2 else 0
        base = (nk + 1 + 3) // 4 * 4
        offsets = w[:nk + 1].view(np.int32).copy()
        return dict(info, offsets=offsets, pair=w[base:base + npairs].copy(), alpha_bits=w[base + cap:base + cap + npairs].copy(),
                    key=np.repeat(np.arange(nk, dtype=np.uint32), np.diff(offsets)))

    def ppf_match(self, src, src_normals, tgt, tgt_normals, thr, want_peaks=False, **params):
        """tdv_ppf_match on host arrays: (poses as RegistrationResults ranked by cluster votes, one dict per pose: votes, members, ref,
        model_index, bin); with want_peaks also the peaks (PPF_PEAK_DTYPE, one per reference point)."""
        src = _f32(src).reshape(-1, 3); sn = _f32(src_normals).reshape(-1, 3); tgt = _f32(tgt).reshape(-1, 3); tn = _f32(tgt_normals).reshape(-1, 3)
        p = ppf_params(**params)
        poses = (PpfPoseC * TDV_PPF_POSES_MAX)()
        n, nref = C.c_int(0), C.c_int(0)
        peaks = np.zeros((len(src) + max(p.ref_stride, 1) - 1) // max(p.ref_stride, 1), PPF_PEAK_DTYPE) if want_peaks else None
        _check(self._h, lib().tdv_ppf_match(self._h, _ptr(src), _ptr(sn), len(src), _ptr(tgt), _ptr(tn), len(tgt), C.c_float(thr), C.byref(p), poses,
                                            C.byref(n), _ptr(peaks), C.byref(nref)), "tdv_ppf_match")
        res, more = _ppf_poses(poses, n.value)
        return (res, more, peaks[:nref.value]) if want_peaks else (res, more)

    def ppf_match_dev(self, d_src, d_src_normals, ns, d_tgt, d_tgt_normals, nt, d_model, info, thr, d_peaks=None, **params):
        """tdv_ppf_match_dev on device pointers against a table of ppf_model_dev (info: its dict, or ppf_model's - the fields of
        tdv_ppf_model_info are taken, the rest ignored): (poses, their dicts, n_ref); d_peaks
        (optional, device, 16 bytes per reference point) receives the peaks."""
        ci = PpfModelInfoC(**{k: info[k] for k, _ in PpfModelInfoC._fields_})
        poses = (PpfPoseC * TDV_PPF_POSES_MAX)()
        n, nref = C.c_int(0), C.c_int(0)
        _check(self._h, lib().tdv_ppf_match_dev(self._h, _ptr(d_src), _ptr(d_src_normals), int(ns), _ptr(d_tgt), _ptr(d_tgt_normals), int(nt),
                                                _ptr(d_model), C.byref(ci), C.c_float(thr), C.byref(ppf_params(**params)), poses, C.byref(n),
                                                _ptr(d_peaks), C.byref(nref)), "tdv_ppf_match_dev")
        res, more = _ppf_poses(poses, n.value)
        return res, more, nref.value

    def ppf_match_batch_dev(self, d_src, d_src_normals, offsets, d_tgt, d_tgt_normals, nt, d_model, info, thr, d_peaks=None, **params):
        """tdv_ppf_match_batch_dev on device pointers: cloud b = rows [offsets[b], offsets[b + 1]) of d_src and d_src_normals, all against
        one table of ppf_model_dev.  Returns ([(poses, their dicts) per instance, as ppf_match_dev returns them], peak offsets: int32
        [n_instances + 1]); d_peaks (optional, device, 16 bytes per reference point of every instance) receives instance b's peaks from
        peak offset b on."""
        ci = PpfModelInfoC(**{k: info[k] for k, _ in PpfModelInfoC._fields_})
        p = ppf_params(**params)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        n = 0 if off is None else len(off) - 1
        slots = max(p.max_poses, 1)
        poses = (PpfPoseC * max(n * slots, 1))()
        n_poses = np.zeros(max(n, 1), np.int32)
        peak_off = np.zeros(n + 1, np.int32)
        _check(self._h, lib().tdv_ppf_match_batch_dev(self._h, _ptr(d_src), _ptr(d_src_normals), _ptr(off), n, _ptr(d_tgt), _ptr(d_tgt_normals),
                                                      int(nt), _ptr(d_model), C.byref(ci), C.c_float(thr), C.byref(p), poses, _ptr(n_poses),
                                                      _ptr(d_peaks), _ptr(peak_off)), "tdv_ppf_match_batch_dev")
        return [_ppf_poses(poses[b * slots:(b + 1) * slots], int(n_poses[b])) for b in range(n)], peak_off

    def ppf_match_batch(self, sources, source_normals, tgt, tgt_normals, thr, want_peaks=False, **params):
        """ppf_match_batch_dev on host clouds: lists of (n_b, 3) points and normals against one model, uploaded with torch; the table comes
        from ppf_model_dev.  One (poses, dicts) per instance, with want_peaks (poses, dicts, peaks)."""
        srcs, off = _instance_rows(sources)
        nrms, noff = _instance_rows(source_normals)
        if len(off) != len(noff) or (off != noff).any():
            raise ValueError("ppf_match_batch: every instance needs as many normals as points")
        import torch
        tgt = np.array(tgt, np.float32).reshape(-1, 3); tn = np.array(tgt_normals, np.float32).reshape(-1, 3)     # (copies: torch wants writable arrays)
        if len(tgt) != len(tn):
            raise ValueError("ppf_match_batch: the model needs as many normals as points")
        nt = len(tgt)
        dev = torch.device("cuda", self.device)
        d_src, d_sn, d_tgt, d_tn = (_upload_rows(self.device, a) for a in (srcs, nrms, tgt, tn))
        nbytes = self.ppf_model_bytes(nt, **params)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        stride = max(ppf_params(**params).ref_stride, 1)
        n_ref = [(len(a) + stride - 1) // stride for a in srcs]
        d_pk = torch.zeros(max(sum(n_ref), 1) * PPF_PEAK_DTYPE.itemsize, dtype=torch.uint8, device=dev) if want_peaks else None
        torch.cuda.synchronize()
        info = self.ppf_model_dev(d_tgt.data_ptr(), d_tn.data_ptr(), nt, buf.data_ptr(), nbytes, **params)
        out, peak_off = self.ppf_match_batch_dev(d_src.data_ptr(), d_sn.data_ptr(), off, d_tgt.data_ptr(), d_tn.data_ptr(), nt, buf.data_ptr(), info,
                                                 thr, d_peaks=None if d_pk is None else d_pk.data_ptr(), **params)
        if not want_peaks:
            return out
        self.synchronize()
        pk = d_pk.cpu().numpy().view(PPF_PEAK_DTYPE)
        return [(res, more, pk[peak_off[b]:peak_off[b + 1]].copy()) for b, (res, more) in enumerate(out)]

    def ransac_dev(self, d_src, ns, d_tgt, nt, d_fs, d_ft, d_corr, voxel, max_iterations, confidence=0.999, seed=42, trace=False):
        """trace=True also returns the per-iteration inlier counts (host array) - and thereby makes the call evaluate every
        (hypothesis, point) test: the exact bail-out only runs when no trace is asked for."""
        res = RansacResultC()
        tr = np.full(max_iterations, -2, np.int32) if trace else None
        _check(self._h, lib().tdv_ransac_dev(self._h, _ptr(d_src), ns, _ptr(d_tgt), nt, _ptr(d_fs), _ptr(d_ft), _ptr(d_corr),
                                             C.c_float(voxel), max_iterations, C.c_float(confidence), C.c_uint32(seed),
                                             C.byref(res), _ptr(tr)), "tdv_ransac_dev")
        return RegistrationResult(transformation=from_colmajor16(res.T), fitness=np.float32(res.fitness), rmse=np.float32(res.rmse),
                                  inliers=res.inliers, best_iteration=res.best_iteration, iterations_run=res.iterations_run, trace_inliers=tr)

    def feature_match_dev(self, d_fs, ns, d_ft, nt, d_corr):
        _check(self._h, lib().tdv_feature_match_dev(self._h, _ptr(d_fs), ns, _ptr(d_ft), nt, _ptr(d_corr)), "tdv_feature_match_dev")

    def estimate_normals_dev(self, d_xyz, n, k, d_normals, d_knn=None):
        _check(self._h, lib().tdv_estimate_normals_dev(self._h, _ptr(d_xyz), n, k, _ptr(d_normals), _ptr(d_knn)), "tdv_estimate_normals_dev")

    def compute_fpfh_dev(self, d_xyz, d_normals, n, radius, d_desc, d_nbr=None, d_cnt=None):
        _check(self._h, lib().tdv_compute_fpfh_dev(self._h, _ptr(d_xyz), _ptr(d_normals), n, C.c_float(radius), _ptr(d_desc),
                                                   _ptr(d_nbr), _ptr(d_cnt)), "tdv_compute_fpfh_dev")

    def normals_fpfh_dev(self, d_xyz, n, k, radius, d_normals, d_desc):
        """estimateNormals(k) + computeFPFH(radius) with one neighbour walk (device pointers); same bits as the two calls."""
        _check(self._h, lib().tdv_normals_fpfh_dev(self._h, _ptr(d_xyz), n, k, C.c_float(radius), _ptr(d_normals), _ptr(d_desc)), "tdv_normals_fpfh_dev")

    def radix_sort_pairs_dev(self, d_keys_in, d_keys_out, d_vals_in, d_vals_out, n, end_bit):
        """Stable sort of n (u64 key, u32 value) pairs on the low end_bit bits of the key (device pointers; csrc/sort.hip)."""
        _check(self._h, lib().tdv_radix_sort_pairs_dev(self._h, _ptr(d_keys_in), _ptr(d_keys_out), _ptr(d_vals_in), _ptr(d_vals_out), C.c_size_t(n), end_bit),
               "tdv_radix_sort_pairs_dev")

    # op -> (code, floats in, floats out per problem) of tdv_study_probe (csrc/probe.hip)
    STUDY_PROBE_OPS = {"svd3": (0, 9, 21), "kabsch_rotation": (1, 9, 9), "smallest_eigvec3": (2, 6, 4), "ldlt6_solve": (3, 42, 6),
                       "euler_xyz": (4, 3, 9), "mul44": (5, 32, 16), "sinf": (6, 1, 1), "cosf": (7, 1, 1), "atanf": (8, 1, 1),
                       "atan2f": (9, 2, 1), "ransac_hypothesis": (10, 24, 12)}

    def study_probe(self, op, inputs):
        """One per-lane device function (csrc/device_linalg.hpp, libm_f32.hpp, ransac_hypothesis_lane) on n problems, one per lane:
        `inputs` is float32 [n, floats in] - a numpy array (the result is one too) or a torch tensor on this context's device (the
        result stays there).  The study library only: raises TdvError on the product library, which has no such entry point."""
        import torch
        if not hasattr(lib(), "tdv_study_probe"):
            raise TdvError("study_probe needs the study library (TDV_LIB_VARIANT=study); the product library has no probe")
        code, k_in, k_out = self.STUDY_PROBE_OPS[op]
        host = not isinstance(inputs, torch.Tensor)
        d_in = torch.from_numpy(np.ascontiguousarray(inputs, np.float32)).to(torch.device("cuda", self.device)) if host else inputs.contiguous()
        if d_in.device != torch.device("cuda", self.device):
            raise ValueError("study_probe: the tensor lies on %s, this context runs on cuda:%d" % (d_in.device, self.device))
        if d_in.dtype != torch.float32 or d_in.numel() % k_in:
            raise ValueError("%s takes float32 [n, %d]" % (op, k_in))
        n = d_in.numel() // k_in
        d_out = torch.empty((n, k_out), dtype=torch.float32, device=d_in.device)
        torch.cuda.synchronize(d_in.device)
        _check(self._h, lib().tdv_study_probe(self._h, code, C.c_longlong(n), C.c_void_p(d_in.data_ptr() if n else 0), C.c_void_p(d_out.data_ptr() if n else 0)),
               "tdv_study_probe")
        return d_out.cpu().numpy() if host else d_out

    # op -> code of tdv_study_primitive (csrc/probe.hip: what each op takes in in0..in2 and writes to out0..out3)
    STUDY_PRIMITIVE_OPS = {"exclusive_scan": 0, "sort_records": 1, "segment_sort": 2, "compact": 3, "tree_sum": 4, "tree_count": 5,
                           "tree_block_max": 6}

    def study_primitive(self, op, n, width=1, in0=None, in1=None, in2=None, out0=None, out1=None, out2=None, out3=None):
        """One shared device primitive (csrc/sort.hip, flag_gather.hpp, fixed_tree.hpp) on device pointers (ints), as the table in
        csrc/probe.hip lays them out; returns once the results are there.  The study library only: raises TdvError on the product
        library, which has no such entry point."""
        if not hasattr(lib(), "tdv_study_primitive"):
            raise TdvError("study_primitive needs the study library (TDV_LIB_VARIANT=study); the product library has no probe")
        _check(self._h, lib().tdv_study_primitive(self._h, self.STUDY_PRIMITIVE_OPS[op], C.c_longlong(n), C.c_longlong(width), _ptr(in0), _ptr(in1),
                                                  _ptr(in2), _ptr(out0), _ptr(out1), _ptr(out2), _ptr(out3)), "tdv_study_primitive")

    def depth_to_cloud_dev(self, d_raw, d_mask, d_bgr, w, h, scale, fx, fy, cx, cy, zmax, d_xyz, d_rgb, capacity,
                           mask_mode=TDV_MASK_THRESHOLD10):
        n = C.c_int()
        _check(self._h, lib().tdv_depth_to_cloud_dev(self._h, _ptr(d_raw), _ptr(d_mask), _ptr(d_bgr), w, h, C.c_float(scale), mask_mode,
                                                     C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), C.c_float(zmax),
                                                     _ptr(d_xyz), _ptr(d_rgb), capacity, C.byref(n)), "tdv_depth_to_cloud_dev")
        return n.value

    def voxel_downsample_dev(self, d_xyz, d_rgb, n, voxel, d_out_xyz, d_out_rgb, capacity, order=TDV_VOXEL_ORDER_FIRST):
        m = C.c_int()
        _check(self._h, lib().tdv_voxel_downsample_dev(self._h, _ptr(d_xyz), _ptr(d_rgb), n, C.c_float(voxel), order, _ptr(d_out_xyz),
                                                       _ptr(d_out_rgb), capacity, C.byref(m)), "tdv_voxel_downsample_dev")
        return m.value

    def voxel_downsample_normals_dev(self, d_xyz, d_normals, n, voxel, d_out_xyz, d_out_normals, capacity, d_rgb=None, d_out_rgb=None,
                                     order=TDV_VOXEL_ORDER_FIRST):
        m = C.c_int()
        _check(self._h, lib().tdv_voxel_downsample_normals_dev(self._h, _ptr(d_xyz), _ptr(d_normals), _ptr(d_rgb), n, C.c_float(voxel), order,
                                                               _ptr(d_out_xyz), _ptr(d_out_normals), _ptr(d_out_rgb), capacity, C.byref(m)),
               "tdv_voxel_downsample_normals_dev")
        return m.value


def _voxel_downsample_batch_dev(self, d_xyz, cloud_offsets, voxel, d_out_xyz, pinhole=None):
    """All clouds' voxels (first-occurrence order) in one set of launches; returns the voxel offsets (int32 [n_clouds + 1]).
    pinhole = (fx, fy, cx, cy): the clouds come from depth images with these intrinsics, in row-major pixel order (pixel-window grouping)."""
    off = np.ascontiguousarray(cloud_offsets, np.int32)
    voff = np.zeros(len(off), np.int32)
    if pinhole is None:
        _check(self._h, lib().tdv_voxel_downsample_batch_dev(self._h, _ptr(d_xyz), _ptr(off), len(off) - 1, C.c_float(voxel), _ptr(d_out_xyz), _ptr(voff)),
               "tdv_voxel_downsample_batch_dev")
    else:
        fx, fy, cx, cy = pinhole
        _check(self._h, lib().tdv_voxel_downsample_batch_pinhole_dev(self._h, _ptr(d_xyz), _ptr(off), len(off) - 1, C.c_float(voxel), C.c_float(fx), C.c_float(fy),
                                                                     C.c_float(cx), C.c_float(cy), _ptr(d_out_xyz), _ptr(voff)), "tdv_voxel_downsample_batch_pinhole_dev")
    return voff


def batch_params(width=1280, height=720, scale_to_meters=1000.0, mask_mode=TDV_MASK_THRESHOLD10, fx=900.0, fy=900.0, cx=640.0,
                 cy=360.0, zmax=1.5, voxel_size=0.001, normals_k=30, fpfh_radius_factor=5.0, ransac_max_iterations=100000,
                 ransac_confidence=0.999, icp_distance_factor=0.4, icp_max_iterations=200, point_to_plane=True, seed=42,
                 voxel_order=TDV_VOXEL_ORDER_REFERENCE, n_frames=1, frame_of_instance=None, mask_format=0, mask_width=0, mask_height=0):
    """Defaults = include/pipeline_config.hpp + config/pipeline_config.yaml of the reference; voxel_order defaults to the
    reference's container order (the poses of Pipeline::processInstance).  frame_of_instance: int array or None."""
    p = BatchParamsC(width, height, scale_to_meters, mask_mode, fx, fy, cx, cy, zmax, voxel_size, normals_k, fpfh_radius_factor,
                     ransac_max_iterations, ransac_confidence, icp_distance_factor, icp_max_iterations, int(point_to_plane), seed,
                     voxel_order, n_frames, None, mask_format, mask_width, mask_height)
    if frame_of_instance is not None:
        p._frame_map = np.ascontiguousarray(frame_of_instance, np.int32)   # kept alive by the struct object
        p.frame_of_instance = p._frame_map.ctypes.data
    return p


def _register_batch_dev(self, d_raw, d_bgr, d_masks, n_instances, params, d_model_xyz, d_model_normals, d_model_fpfh, n_model):
    """Batched device-resident Pipeline::processInstance; returns a list of dicts (one per instance)."""
    res = (InstanceResultC * max(n_instances, 1))()
    _check(self._h, lib().tdv_register_batch_dev(self._h, _ptr(d_raw), _ptr(d_bgr), _ptr(d_masks), n_instances, C.byref(params),
                                                 _ptr(d_model_xyz), _ptr(d_model_normals), _ptr(d_model_fpfh), n_model, res),
           "tdv_register_batch_dev")
    return _instance_results(res, n_instances)


def _instance_results(res, n_instances):
    # one structured view over the result array instead of a ctypes attribute walk per instance (1,024 instances: 6 ms -> 0.6 ms)
    dt = np.dtype([("T", np.float32, 16), ("fitness", np.float32), ("rmse", np.float32), ("coarse_fitness", np.float32), ("coarse_inliers", np.int32),
                   ("icp_iterations", np.int32), ("n_points", np.int32), ("n_voxels", np.int32), ("status", np.int32)])
    assert dt.itemsize == C.sizeof(InstanceResultC)
    a = np.frombuffer(res, dtype=dt, count=n_instances).copy() if n_instances else np.zeros(0, dt)
    Ts = a["T"].reshape(-1, 4, 4).transpose(0, 2, 1).copy()          # column-major float[16] -> row-major [4, 4]
    return [dict(T=Ts[i], fitness=a["fitness"][i], rmse=a["rmse"][i], coarse_fitness=a["coarse_fitness"][i], coarse_inliers=int(a["coarse_inliers"][i]),
                 icp_iterations=int(a["icp_iterations"][i]), n_points=int(a["n_points"][i]), n_voxels=int(a["n_voxels"][i]), status=int(a["status"][i]))
            for i in range(n_instances)]


def _refine_batch_dev(self, d_raw, d_bgr, d_masks, n_instances, params, T0s, d_model_xyz, d_model_normals, n_model):
    """tdv_register_batch_dev's clouds and voxels, then ICP from the caller's poses T0s ((B, 4, 4)); the same dicts as register_batch_dev
    (coarse_fitness / coarse_inliers -1: no coarse stage)."""
    T0s = np.asarray(T0s, np.float32).reshape(-1, 4, 4)
    t0 = np.concatenate([to_colmajor16(T) for T in T0s]) if len(T0s) else np.zeros(0, np.float32)
    res = (InstanceResultC * max(n_instances, 1))()
    _check(self._h, lib().tdv_refine_batch_dev(self._h, _ptr(d_raw), _ptr(d_bgr), _ptr(d_masks), n_instances, C.byref(params), _ptr(t0),
                                               _ptr(d_model_xyz), _ptr(d_model_normals), n_model, res), "tdv_refine_batch_dev")
    return _instance_results(res, n_instances)


def _prepare_model_dev(self, d_xyz, n, voxel, k, radius_factor, d_out_xyz, d_out_normals, d_out_fpfh, order=TDV_VOXEL_ORDER_REFERENCE):
    m = C.c_int()
    _check(self._h, lib().tdv_prepare_model_dev(self._h, _ptr(d_xyz), n, C.c_float(voxel), order, k, C.c_float(radius_factor), _ptr(d_out_xyz),
                                                _ptr(d_out_normals), _ptr(d_out_fpfh), C.byref(m)), "tdv_prepare_model_dev")
    return m.value


def _depth_to_cloud_batch_dev(self, d_raw, d_masks, d_bgr, n_instances, w, h, scale, fx, fy, cx, cy, zmax, d_xyz, d_rgb, capacity,
                              mask_format=0, mask_mode=TDV_MASK_THRESHOLD10, n_frames=1, frame_of_instance=None):
    """All instances of a scene -> clouds back to back; returns the offsets array (n_instances + 1)."""
    off = np.zeros(n_instances + 1, np.int32)
    fmap = None if frame_of_instance is None else np.ascontiguousarray(frame_of_instance, np.int32)
    st = lib().tdv_depth_to_cloud_batch_dev(self._h, _ptr(d_raw), _ptr(d_masks), _ptr(d_bgr), n_instances, mask_format, n_frames, _ptr(fmap), w, h,
                                            C.c_float(scale), mask_mode, C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                            C.c_float(zmax), _ptr(d_xyz), _ptr(d_rgb), C.c_longlong(capacity), _ptr(off))
    _check(self._h, st, "tdv_depth_to_cloud_batch_dev")
    return off


def _broadcast_model(self, comm, root, d_xyz, d_normals, d_fpfh, capacity, n_model):
    """tdv_broadcast_model: comm is an ncclComm_t (int / c_void_p); returns the model's point count on every rank."""
    n = C.c_int(int(n_model))
    _check(self._h, lib().tdv_broadcast_model(self._h, C.c_void_p(comm), int(root), _ptr(d_xyz), _ptr(d_normals), _ptr(d_fpfh), int(capacity), C.byref(n)),
           "tdv_broadcast_model")
    return n.value


def _gather_results(self, comm, local, slots_per_rank, world_size):
    """tdv_gather_results: local = list of InstanceResultC; returns world_size * slots_per_rank InstanceResultC (status -1 = unused slot)."""
    loc = (InstanceResultC * max(len(local), 1))(*local)
    out = (InstanceResultC * max(world_size * slots_per_rank, 1))()
    _check(self._h, lib().tdv_gather_results(self._h, C.c_void_p(comm), loc, len(local), int(slots_per_rank), out), "tdv_gather_results")
    return list(out)[:world_size * slots_per_rank]


Context.depth_to_cloud_batch_dev = _depth_to_cloud_batch_dev
Context.broadcast_model = _broadcast_model
Context.gather_results = _gather_results
Context.register_batch_dev = _register_batch_dev
Context.refine_batch_dev = _refine_batch_dev
Context.voxel_downsample_batch_dev = _voxel_downsample_batch_dev
Context.prepare_model_dev = _prepare_model_dev


def sample_triples(n, count, seed=42):
    out = np.empty((count, 3), np.uint64)
    _check(None, lib().tdv_sample_triples(C.c_uint32(seed), C.c_uint64(n), count, _ptr(out)), "tdv_sample_triples")
    return out


def sample_triples_batch(n, count, seed=42):
    """The index stream as RANSAC's batch loop uploads it (tdv_sample_triples_batch): (raw, packed) - raw is uint64[count] when
    packed, int32[count, 4] (i0, i1, i2, valid) otherwise.  unpack_triples turns either into (triples uint64[count, 3], valid bool[count])."""
    buf = np.zeros(2 * count, np.uint64)
    packed = C.c_int(-1)
    _check(None, lib().tdv_sample_triples_batch(C.c_uint32(seed), C.c_uint64(n), count, _ptr(buf), C.byref(packed)), "tdv_sample_triples_batch")
    if packed.value:
        return buf[:count].copy(), True
    return buf.view(np.int32).reshape(count, 4).copy(), False


def unpack_triples(raw, packed):
    if packed:
        m = np.uint64(0x1fffff)
        tri = np.stack([raw & m, (raw >> np.uint64(21)) & m, (raw >> np.uint64(42)) & m], axis=1)
        return tri, (raw >> np.uint64(63)) != 0
    return raw[:, :3].astype(np.uint64), raw[:, 3] != 0


def filter_duplicates(poses, min_distance=0.1):
    """Pipeline::filterDuplicates (src/pipeline.cpp:153-180); poses: [n,4,4]."""
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    cm = np.ascontiguousarray(np.transpose(poses, (0, 2, 1))).reshape(-1, 16)
    out = np.empty_like(cm); m = C.c_int()
    _check(None, lib().tdv_filter_duplicates(_ptr(cm), len(cm), C.c_float(min_distance), _ptr(out), C.byref(m)), "tdv_filter_duplicates")
    return np.transpose(out[:m.value].reshape(-1, 4, 4), (0, 2, 1)).copy()


def load_reference_model(path, capacity=1 << 20):
    """Registration::loadReferenceModel (src/registration.cpp:416-461): returns a PointCloud (empty if the file is missing)."""
    xyz = np.zeros((capacity, 3), np.float32); rgb = np.zeros((capacity, 3), np.float32); n = C.c_int(); hc = C.c_int()
    st = lib().tdv_load_ply_ascii(path.encode(), _ptr(xyz), _ptr(rgb), capacity, C.byref(n), C.byref(hc))
    if st != 0:
        return PointCloud()
    return PointCloud(points=xyz[:n.value].copy(), colors=(rgb[:n.value].copy() if hc.value else None))


def load_mask_png(path):
    """One mask file as Segmentation::loadMasksFromDir reads it (grey PNG, > 10 -> 255): uint8 [h, w], or None if the file
    cannot be decoded here (colour / palette PNG, JPEG, missing)."""
    w = C.c_int(); h = C.c_int()
    if lib().tdv_load_mask_png(path.encode(), None, C.c_longlong(0), C.byref(w), C.byref(h)) != 0:
        return None
    out = np.zeros((h.value, w.value), np.uint8)
    if lib().tdv_load_mask_png(path.encode(), _ptr(out), C.c_longlong(out.size), C.byref(w), C.byref(h)) != 0:
        return None
    return out


def load_masks_from_dir(masks_dir, width, height):
    """Segmentation::loadMasksFromDir (src/segmentation.cpp:12-42): (masks uint8 [n, height, width], n_skipped)."""
    n = C.c_int(); sk = C.c_int()
    _check(None, lib().tdv_load_masks_from_dir(masks_dir.encode(), width, height, None, 0, C.byref(n), C.byref(sk)), "tdv_load_masks_from_dir")
    out = np.zeros((n.value, height, width), np.uint8)
    if n.value:
        _check(None, lib().tdv_load_masks_from_dir(masks_dir.encode(), width, height, _ptr(out), n.value, C.byref(n), C.byref(sk)), "tdv_load_masks_from_dir")
    return out, sk.value


def pose_compose(extrinsics, T):
    e = to_colmajor16(extrinsics); t = to_colmajor16(T); o = np.zeros(16, np.float32)
    _check(None, lib().tdv_pose_compose(_ptr(e), _ptr(t), _ptr(o)), "tdv_pose_compose")
    return from_colmajor16(o)


# --------------------------------------------------------------------------------------------------
# Operator API in the reference's own names.  A thread-local default Context stands in for the
# per-thread state the reference's static methods hide.
_tls = threading.local()


def default_context():
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        ctx = Context(0)
        _tls.ctx = ctx
    return ctx


class GPUDepth:
    """include/gpu_depth.hpp:9-13."""

    @staticmethod
    def isCudaAvailable():
        try:
            return device_count() > 0
        except TdvError:
            return False

    @staticmethod
    def preprocess(raw_depth, mask, scale):
        if not GPUDepth.isCudaAvailable():
            raise RuntimeError("CUDA not available")  # src/gpu_impl.cpp:64
        return default_context().depth_preprocess(raw_depth, mask, scale)


class GPUPointCloud:
    """include/gpu_depth.hpp:15-22.  zmax defaults to the reference dispatch's hard-coded 10.0
    (src/gpu_impl.cpp:97); pass config.depth.clipping_max to follow the CPU branch."""

    @staticmethod
    def generate(depth, rgb, fx, fy, cx, cy, zmax=10.0):
        if not GPUDepth.isCudaAvailable():
            return PointCloud()  # src/gpu_impl.cpp:126
        xyz, col = default_context().deproject(depth, rgb, fx, fy, cx, cy, zmax)
        return PointCloud(points=xyz, colors=col)


class GPURegistration:
    """include/gpu_registration.hpp:8-19."""

    @staticmethod
    def isCudaAvailable():
        return GPUDepth.isCudaAvailable()

    @staticmethod
    def icpRefine(source, target, initial_transform, distance_threshold, max_iterations=200):
        if not GPURegistration.isCudaAvailable():
            raise RuntimeError("CUDA not available")  # src/gpu_impl.cpp:258
        tn = target.normals if target.hasNormals() else None
        return default_context().icp(source.points, target.points, tn, initial_transform, distance_threshold, max_iterations, True)


class Registration:
    """include/registration.hpp:32-60, served by the HIP backend."""

    @staticmethod
    def voxelDownsample(cloud, voxel_size, order=TDV_VOXEL_ORDER_REFERENCE):
        col = cloud.colors if cloud.hasColors() else None
        xyz, c = default_context().voxel_downsample(cloud.points, col, voxel_size, order)
        return PointCloud(points=xyz, colors=c)

    @staticmethod
    def estimateNormals(cloud, k=30):
        cloud.normals = default_context().estimate_normals(cloud.points, k)

    @staticmethod
    def computeFPFH(cloud, radius):
        return default_context().compute_fpfh(cloud.points, cloud.normals, radius)

    @staticmethod
    def ransacRegistration(source, target, source_features, target_features, voxel_size, max_iterations=100000, confidence=0.999):
        return default_context().ransac(source.points, target.points, source_features, target_features, None, voxel_size,
                                        max_iterations, confidence)

    @staticmethod
    def icpRefine(source, target, initial_transform, distance_threshold, max_iterations=200, point_to_plane=True):
        tn = target.normals if target.hasNormals() else None
        return default_context().icp(source.points, target.points, tn, initial_transform, distance_threshold, max_iterations,
                                     point_to_plane)
