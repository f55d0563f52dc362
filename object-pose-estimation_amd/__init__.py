"""object-pose-estimation_amd — MI355X-native registration hot path (ICP + FPFH/SAC-IA).

Thin ctypes binding of the C ABI in include/ope.h (libope_hip.so, hand-written HIP for gfx950).
This package is plumbing for tests, bench.py and the torch.distributed driver; the product is
the shared library and the C++ façade in include/ope/.  There is NO CPU fallback: every entry
point raises if the library or a GPU is missing.

The directory name has a hyphen, so import it with
    importlib.import_module("object-pose-estimation_amd")
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libope_hip.so")

OPE_OK, OPE_EINVAL, OPE_ENODEV, OPE_EHIP, OPE_ENOMEM, OPE_ESTATE, OPE_ECOMM, OPE_EEMPTY, OPE_ERANGE = 0, -1, -2, -3, -4, -5, -6, -7, -8
CONV_NAMES = ["NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES"]
CORR_NEAREST, CORR_NORMAL_SHOOTING = 0, 1
EST_SVD, EST_POINT_TO_PLANE_LLS, EST_POINT_TO_PLANE_LM = 0, 1, 2
COMM_AUTO, COMM_RCCL, COMM_P2P = 0, 1, 2
# ope_coarse_batch_result.status; per-cloud limits of ope_coarse_pose_batch
COARSE_OK, COARSE_EMPTY_TARGET, COARSE_FEW_TARGET_FEATURES = 0, 1, 2
COARSE_MAX_POINTS, COARSE_MAX_KEYS = 65536, 4096
# ope_prerejective_batch_result.status
PREREJ_OK, PREREJ_EMPTY_TARGET, PREREJ_FEW_TARGET_FEATURES, PREREJ_NAN_FEATURES = 0, 1, 2, 3
# ope_corr_sac_batch_result.status
CORRSAC_OK, CORRSAC_EMPTY_TARGET, CORRSAC_FEW_TARGET_FEATURES = 0, 1, 2
# ope_final_batch_result.status
FINAL_OK, FINAL_EMPTY_TARGET, FINAL_FEW_TARGET_FEATURES, FINAL_FEW_FINE_POINTS = 0, 1, 2, 3
# ope_track_gate_result.branch; ope_track_result.coarse_status when the coarse stage was skipped
TRACK_NO_CLUSTERS, TRACK_GATED, TRACK_REALIGN_ALL, TRACK_NOTHING, TRACK_REALIGN_LOOP = 0, 1, 2, 3, 4
TRACK_BRANCH_NAMES = ["NO_CLUSTERS", "GATED", "REALIGN_ALL", "NOTHING", "REALIGN_LOOP"]
TRACK_COARSE_SKIPPED = -1
CERT_AUTO, CERT_OFF, CERT_ALWAYS = 0, 1, 2   # ope_icp_params.skip_certificates
NUM_SUMS, NUM_SUMS_MAX = 17, 44
GREJ_MEDIAN_DISTANCE, GREJ_ONE_TO_ONE, GREJ_VAR_TRIMMED = 0, 1, 2   # ope_global_rejector.kind
GREJ_MAX = 4
COMM_ID_BYTES = 128


class OpeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ope error {code}: {msg}")
        self.code = code


def build_library(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of libope_hip.so (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs += [os.path.join(_HERE, "..", "include", "ope.h"), os.path.join(_HERE, "Makefile")]
    stale = force or not os.path.exists(LIB_PATH)
    if not stale:
        t = os.path.getmtime(LIB_PATH)
        stale = any(os.path.getmtime(s) > t for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", _HERE, "-j8", "libope_hip.so"], stdout=subprocess.DEVNULL)
    return LIB_PATH


class IcpParams(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int),
        ("transformation_epsilon", C.c_double),
        ("euclidean_fitness_epsilon", C.c_double),
        ("max_corr_dist", C.c_double),
        ("min_correspondences", C.c_int),
        ("use_reciprocal", C.c_int),
        ("corr_mode", C.c_int),
        ("k_normal_shooting", C.c_int),
        ("use_surface_normal_rej", C.c_int),
        ("surface_normal_thr", C.c_double),
        ("use_self_occluded_rej", C.c_int),
        ("self_occluded_thr", C.c_double),
        ("mse_threshold_absolute", C.c_double),
        ("failure_after_max_iter", C.c_int),
        ("check_every", C.c_int),
        ("estimator", C.c_int),
        ("deterministic_sums", C.c_int),
        ("tree_walk", C.c_int),
        ("update_launch", C.c_int),
        ("skip_certificates", C.c_int),
    ]


class GlobalRejector(C.Structure):
    _fields_ = [("kind", C.c_int), ("factor", C.c_double), ("min_ratio", C.c_double), ("max_ratio", C.c_double)]


class GlobalRejectorStats(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_out", C.c_int64), ("threshold", C.c_double), ("ratio", C.c_double), ("launches", C.c_int64)]


class IcpResult(C.Structure):
    _fields_ = [
        ("iterations", C.c_int),
        ("converged", C.c_int),
        ("state", C.c_int),
        ("last_mse", C.c_double),
        ("n_corr", C.c_int64),
        ("align_strength", C.c_double),
    ]


class IcpBatchResult(C.Structure):
    _fields_ = [
        ("result", IcpResult),
        ("T", C.c_float * 16),
        ("fitness", C.c_double),
        ("fitness_n", C.c_int64),
    ]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("ms", C.c_double), ("launches", C.c_int), ("algorithmic_bytes", C.c_double)]


class IndexParams(C.Structure):
    _fields_ = [("leaf_size", C.c_int), ("grid", C.c_int), ("grid_fill", C.c_float), ("grid_max_cells", C.c_int)]


class SaciaParams(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int),
        ("nr_samples", C.c_int),
        ("k_correspondences", C.c_int),
        ("max_corr_dist", C.c_double),
        ("min_sample_dist", C.c_float),
        ("seed", C.c_uint64),
    ]


class PrerejectiveParams(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32),
        ("nr_samples", C.c_int32),
        ("k_correspondences", C.c_int32),
        ("similarity_threshold", C.c_float),
        ("max_corr_dist", C.c_double),
        ("inlier_fraction", C.c_float),
        ("seed", C.c_uint64),
    ]


class PrerejectiveResult(C.Structure):
    _fields_ = [
        ("T", C.c_float * 16),
        ("error", C.c_double),
        ("best_iteration", C.c_int32),
        ("inliers", C.c_int32),
        ("converged", C.c_int32),
    ]


class PrerejectiveStats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int64),
        ("survivors", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("nr_samples", C.c_int64),
    ]


class CorrSacParams(C.Structure):
    _fields_ = [
        ("inlier_threshold", C.c_double),
        ("max_iterations", C.c_int32),
        ("probability", C.c_double),
        ("seed", C.c_uint64),
    ]


class CorrSacResult(C.Structure):
    _fields_ = [
        ("T_best", C.c_float * 16),
        ("T_svd", C.c_float * 16),
        ("inliers", C.c_int32),
        ("best", C.c_int32),
        ("iterations", C.c_int32),
        ("found", C.c_int32),
    ]


class CorrSacStats(C.Structure):
    _fields_ = [
        ("hypotheses", C.c_int64),
        ("iterations", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("sample_dist_thresh", C.c_double),
    ]


class CorrSacBatchResult(C.Structure):
    _fields_ = [
        ("T_svd", C.c_float * 16),
        ("T_best", C.c_float * 16),
        ("sample_dist_thresh", C.c_double),
        ("seed", C.c_uint64),
        ("matches", C.c_int32),
        ("inliers", C.c_int32),
        ("best", C.c_int32),
        ("iterations", C.c_int32),
        ("found", C.c_int32),
        ("n_src_keys", C.c_int32),
        ("n_tgt_keys", C.c_int32),
        ("status", C.c_int32),
    ]


class CorrSacBatchStats(C.Structure):
    _fields_ = [
        ("clusters", C.c_int64),
        ("active", C.c_int64),
        ("hypotheses", C.c_int64),
        ("draw_lists", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
    ]


class PrerejectiveBatchResult(C.Structure):
    _fields_ = [
        ("T", C.c_float * 16),
        ("error", C.c_double),
        ("best_iteration", C.c_int32),
        ("inliers", C.c_int32),
        ("converged", C.c_int32),
        ("survivors", C.c_int32),
        ("n_src_keys", C.c_int32),
        ("n_tgt_keys", C.c_int32),
        ("status", C.c_int32),
        ("seed", C.c_uint64),
    ]


class PrerejectiveBatchStats(C.Structure):
    _fields_ = [
        ("clusters", C.c_int64),
        ("active", C.c_int64),
        ("iterations", C.c_int64),
        ("survivors", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("nr_samples", C.c_int64),
    ]


class CoarseParams(C.Structure):
    _fields_ = [
        ("key_leaf", C.c_float),
        ("normals_k", C.c_int),
        ("viewpoint", C.c_float * 3),
        ("fpfh_radius", C.c_float),
        ("sacia", SaciaParams),
    ]


class CoarseBatchResult(C.Structure):
    _fields_ = [
        ("T", C.c_float * 16),
        ("best_error", C.c_double),
        ("best_iteration", C.c_int32),
        ("n_src_keys", C.c_int32),
        ("n_tgt_keys", C.c_int32),
        ("status", C.c_int32),
    ]


class FinalParams(C.Structure):
    _fields_ = [
        ("coarse", CoarseParams),
        ("fine_leaf", C.c_float),
        ("fine_normals_k", C.c_int),
        ("min_fine_points", C.c_int),
        ("icp", IcpParams),
        ("fitness_max_range", C.c_double),
        ("accept_fitness", C.c_double),
        ("accept_strength", C.c_double),
    ]


class FinalBatchResult(C.Structure):
    _fields_ = [
        ("coarse", CoarseBatchResult),
        ("seed", C.c_uint64),
        ("fine", IcpBatchResult),
        ("n_fine_src", C.c_int32),
        ("n_fine_tgt", C.c_int32),
        ("status", C.c_int32),
        ("accepted", C.c_int32),
    ]


class TrackParams(C.Structure):
    _fields_ = [
        ("gate_distance", C.c_double),
        ("coarse_fitness", C.c_double),
        ("final", FinalParams),
    ]


class TrackCentroid(C.Structure):
    _fields_ = [
        ("centroid", C.c_float * 3),
        ("count", C.c_int32),
        ("distance", C.c_float),
    ]


class TrackGateResult(C.Structure):
    _fields_ = [
        ("branch", C.c_int32),
        ("selected", C.c_int32),
        ("source", TrackCentroid),
    ]


class TrackResult(C.Structure):
    _fields_ = [
        ("gate", TrackGateResult),
        ("selected", C.c_int32),
        ("coarse_status", C.c_int32),
        ("seed", C.c_uint64),
        ("coarse", C.c_float * 16),
        ("fine", C.c_float * 16),
        ("rigid", C.c_float * 16),
        ("final_pose", C.c_float * 16),
        ("icp", IcpResult),
        ("fitness", C.c_double),
        ("fitness_n", C.c_int64),
        ("n_fine_src", C.c_int32),
        ("n_fine_tgt", C.c_int32),
        ("status", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ClusterParams(C.Structure):
    _fields_ = [
        ("tolerance", C.c_double),
        ("min_size", C.c_int32),
        ("max_size", C.c_int32),
    ]


class ClusterStats(C.Structure):
    _fields_ = [
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("cells", C.c_int64),
        ("pairs_tested", C.c_int64),
    ]


class RegionParams(C.Structure):
    _fields_ = [
        ("number_of_neighbours", C.c_int32),
        ("normals_k", C.c_int32),
        ("smoothness_threshold", C.c_double),
        ("curvature_threshold", C.c_double),
        ("min_size", C.c_int32),
        ("max_size", C.c_int32),
    ]


class RegionStats(C.Structure):
    _fields_ = [
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("sweeps", C.c_int64),
        ("one_way_edges", C.c_int64),
        ("regions_before_size_filter", C.c_int64),
        ("refused_curvature", C.c_int64),
    ]


class RegionRgbParams(C.Structure):
    _fields_ = [
        ("region_neighbour_number", C.c_int32),
        ("distance_threshold", C.c_double),
        ("point_color_threshold", C.c_double),
        ("region_color_threshold", C.c_double),
        ("min_size", C.c_int32),
        ("max_size", C.c_int32),
    ]


class RegionRgbStats(C.Structure):
    _fields_ = [
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("sweeps", C.c_int64),
        ("one_way_edges", C.c_int64),
        ("segments", C.c_int64),
        ("segment_pairs", C.c_int64),
        ("homogeneous_regions", C.c_int64),
        ("regions_absorbed", C.c_int64),
        ("regions_before_size_filter", C.c_int64),
    ]


class VfhParams(C.Structure):
    _fields_ = [
        ("normals_k", C.c_int32),
        ("viewpoint", C.c_float * 3),
        ("use_given_centroid", C.c_int32),
        ("centroid", C.c_float * 3),
        ("use_given_normal", C.c_int32),
        ("normal", C.c_float * 3),
    ]


class VfhStats(C.Structure):
    _fields_ = [
        ("points", C.c_int64),
        ("rejected_pairs", C.c_int64),
        ("normals_estimated", C.c_int64),
        ("empty_clouds", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
    ]


class PlaneParams(C.Structure):
    _fields_ = [
        ("distance_threshold", C.c_double),
        ("probability", C.c_double),
        ("max_iterations", C.c_int32),
        ("optimize_coefficients", C.c_int32),
        ("seed", C.c_uint64),
    ]


class PlaneStats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int64),
        ("hypotheses", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("best", C.c_int32),
        ("found", C.c_int32),
    ]


class TabletopResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_prism", C.c_int32),
        ("n_plane", C.c_int32),
        ("n_not_plane", C.c_int32),
        ("coeff_first", C.c_float * 4),
        ("coeff_second", C.c_float * 4),
        ("corners", C.c_float * 12),
        ("iterations_first", C.c_int64),
        ("iterations_second", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
    ]


TABLETOP_OK, TABLETOP_NO_PLANE_FIRST, TABLETOP_NO_PLANE_SECOND = 0, 1, 2


class PeelParams(C.Structure):
    _fields_ = [
        ("keep_fraction", C.c_double),
        ("max_planes", C.c_int32),
    ]


class PeelResult(C.Structure):
    _fields_ = [
        ("n_planes", C.c_int32),
        ("n_rest", C.c_int32),
        ("stop", C.c_int32),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
    ]


PEEL_FRACTION, PEEL_NO_INLIERS, PEEL_MAX_PLANES = 0, 1, 2


class DepthParams(C.Structure):
    """ope_depth_params: the reference applies its cx / fx to the ROW and its cy / fy to the COLUMN (datagrabber.cpp:86,170-171)."""
    _fields_ = [
        ("f_row", C.c_float),
        ("c_row", C.c_float),
        ("f_col", C.c_float),
        ("c_col", C.c_float),
        ("scale", C.c_float),
        ("z_max", C.c_double),
    ]


class DepthStats(C.Structure):
    _fields_ = [
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
        ("pixels", C.c_int64),
        ("valid", C.c_int64),
        ("kept", C.c_int64),
    ]


class MlsParams(C.Structure):
    """ope_mls_params: pcl::MovingLeastSquares with upsampling NONE (ProcessingPcd::getSmooth)."""
    _fields_ = [
        ("radius", C.c_double),
        ("polynomial_fit", C.c_int),
        ("order", C.c_int),
        ("sqr_gauss_param", C.c_double),
        ("compute_normals", C.c_int),
    ]


class MlsStats(C.Structure):
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_out", C.c_int64),
        ("n_plane_only", C.c_int64),
        ("n_dropped", C.c_int64),
        ("neighbours_total", C.c_int64),
    ]


class MlsUpsampleParams(C.Structure):
    """ope_mls_upsample_params: pcl::MovingLeastSquares with upsampling VOXEL_GRID_DILATION (RegMeshPcd::generateMesh)."""
    _fields_ = [
        ("radius", C.c_double),
        ("polynomial_fit", C.c_int),
        ("order", C.c_int),
        ("sqr_gauss_param", C.c_double),
        ("compute_normals", C.c_int),
        ("voxel_size", C.c_float),
        ("dilation_iterations", C.c_int),
    ]


class MlsUpsampleStats(C.Structure):
    _fields_ = [
        ("n_in", C.c_int64),
        ("n_valid", C.c_int64),
        ("n_voxels", C.c_int64),
        ("n_invalid_nearest", C.c_int64),
        ("n_polynomial", C.c_int64),
        ("n_rejected_farther", C.c_int64),
        ("n_out", C.c_int64),
        ("data_size", C.c_int64),
        ("launches", C.c_int64),
        ("host_syncs", C.c_int64),
    ]


SENSOR_KINECT, SENSOR_ASTRA, SENSOR_EUCLID = 0, 1, 2
SENSORS = {"kinect": SENSOR_KINECT, "astra": SENSOR_ASTRA, "euclid": SENSOR_EUCLID}

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)
_vp = C.c_void_p

# every symbol include/ope.h declares: (name, restype, argtypes)
ABI = [
    ("ope_abi_version", C.c_int, []),
    ("ope_device_count", C.c_int, []),
    ("ope_ctx_create", C.c_int, [C.POINTER(_vp), C.c_int]),
    ("ope_ctx_destroy", None, [_vp]),
    ("ope_ctx_set_stream", C.c_int, [_vp, _vp]),
    ("ope_ctx_sync", C.c_int, [_vp]),
    ("ope_ctx_set_tracing", C.c_int, [_vp, C.c_int]),
    ("ope_ctx_set_wait_limit", C.c_int, [_vp, C.c_double]),
    ("ope_last_error", C.c_char_p, [_vp]),
    ("ope_profile_kernels", C.c_int, [_vp, C.c_int]),
    ("ope_profile_kernels_read", C.c_int, [_vp, C.POINTER(KernelTime), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_cloud_upload", C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_ssize_t, C.POINTER(_vp)]),
    ("ope_cloud_set_normals", C.c_int, [_vp, _vp, _fp]),
    ("ope_cloud_concat", C.c_int, [_vp, _vp, _fp, _vp, C.POINTER(_vp)]),
    ("ope_cloud_download", C.c_int, [_vp, _vp, _fp]),
    ("ope_cloud_size", C.c_size_t, [_vp]),
    ("ope_cloud_free", None, [_vp]),
    ("ope_index_default_params", None, [C.POINTER(IndexParams)]),
    ("ope_index_build", C.c_int, [_vp, _vp, C.POINTER(IndexParams), C.POINTER(_vp)]),
    ("ope_index_free", None, [_vp]),
    ("ope_nn_search", C.c_int, [_vp, _vp, _vp, _fp, _ip, _fp]),
    ("ope_knn_search", C.c_int, [_vp, _vp, _vp, _fp, C.c_int, _ip, _fp]),
    ("ope_radius_search", C.c_int, [_vp, _vp, _vp, C.c_float, C.c_int, _ip, _ip, _fp]),
    ("ope_icp_default_params", None, [C.POINTER(IcpParams)]),
    ("ope_icp_run", C.c_int, [_vp, _vp, _vp, _fp, C.POINTER(IcpParams), _fp, C.POINTER(IcpResult)]),
    ("ope_icp_run_batch", C.c_int, [_vp, C.c_size_t, C.POINTER(_vp), C.POINTER(_vp), _fp, C.POINTER(IcpParams), C.c_double,
                                     C.POINTER(IcpBatchResult)]),
    ("ope_icp_begin", C.c_int, [_vp, _vp, _vp, _fp, C.POINTER(IcpParams)]),
    ("ope_icp_accumulate", C.c_int, [_vp]),
    ("ope_icp_sums_device", _vp, [_vp]),
    ("ope_icp_update", C.c_int, [_vp]),
    ("ope_icp_set_sums_buffer", C.c_int, [_vp, _vp]),
    ("ope_icp_iterate", C.c_int, [_vp, C.c_int]),
    ("ope_icp_profile", C.c_int, [_vp, C.c_int]),
    ("ope_icp_profile_read", C.c_int, [_vp, _dp, C.POINTER(C.c_int)]),
    ("ope_icp_poll", C.c_int, [_vp, C.POINTER(IcpResult)]),
    ("ope_icp_current_transform", C.c_int, [_vp, _fp]),
    ("ope_icp_end", C.c_int, [_vp, _fp, C.POINTER(IcpResult)]),
    ("ope_icp_set_global_sizes", C.c_int, [_vp, C.c_int64, C.c_int64]),
    ("ope_icp_kernel_launches", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("ope_icp_overlapped_updates", C.c_int64, [_vp]),
    ("ope_icp_certificate_stats", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("ope_icp_set_fixed_correspondences", C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t]),
    ("ope_icp_update_fallbacks", C.c_int, [_vp]),
    ("ope_icp_fixed_correspondences", C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_icp_profile_launches", C.c_int, [_vp, _fp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_cloud_select", C.c_int, [_vp, _vp, _ip, C.c_size_t, C.POINTER(_vp)]),
    ("ope_remove_nan_cloud", C.c_int, [_vp, _vp, C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_pass_through_cloud", C.c_int, [_vp, _vp, _fp, _fp, C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_statistical_outlier_removal_cloud", C.c_int, [_vp, _vp, C.c_int, C.c_double, C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_uniform_sampling_cloud", C.c_int, [_vp, _vp, C.c_float, C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_icp_correspondences", C.c_int, [_vp, _ip, _ip, _fp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_icp_last_incremental", C.c_int, [_vp, _fp]),
    ("ope_reject_pairs", C.c_int, [_vp, C.c_int, _fp, _fp, C.c_size_t, C.c_double, C.POINTER(C.c_ubyte)]),
    ("ope_global_rejector_defaults", None, [C.c_int, C.POINTER(GlobalRejector)]),
    ("ope_icp_set_global_rejectors", C.c_int, [_vp, C.POINTER(GlobalRejector), C.c_size_t]),
    ("ope_icp_global_rejector_stats", C.c_int, [_vp, C.c_size_t, C.POINTER(GlobalRejectorStats)]),
    ("ope_reject_correspondences", C.c_int, [_vp, C.POINTER(GlobalRejector), _ip, _ip, _fp, C.c_size_t, C.POINTER(C.c_ubyte), C.POINTER(GlobalRejectorStats)]),
    ("ope_fitness", C.c_int, [_vp, _vp, _vp, _fp, C.c_double, _dp, _dp, C.POINTER(C.c_int64)]),
    ("ope_rigid_transform_svd", C.c_int, [_vp, _fp, _fp, C.c_size_t, _fp]),
    ("ope_transform_cloud", C.c_int, [_vp, _vp, _fp, _fp]),
    ("ope_comm_get_unique_id", C.c_int, [C.c_char_p]),
    ("ope_comm_init_rank", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    ("ope_comm_destroy", C.c_int, [_vp]),
    ("ope_comm_set_transport", C.c_int, [_vp, C.c_int]),
    ("ope_comm_transport", C.c_int, [_vp]),
    ("ope_comm_p2p_open", C.c_int, [_vp, C.c_char_p]),
    ("ope_comm_p2p_connect", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    ("ope_normals", C.c_int, [_vp, _vp, C.c_int, _fp, _fp, _fp]),
    ("ope_normals_from", C.c_int, [_vp, _vp, _vp, C.c_int, _fp, _fp, _fp]),
    ("ope_fpfh", C.c_int, [_vp, _vp, C.c_float, _fp]),
    ("ope_uniform_sampling", C.c_int, [_vp, _vp, C.c_float, _ip, C.POINTER(C.c_size_t)]),
    ("ope_remove_nan", C.c_int, [_vp, _vp, _ip, C.POINTER(C.c_size_t)]),
    ("ope_pass_through", C.c_int, [_vp, _vp, _fp, _fp, _ip, C.POINTER(C.c_size_t)]),
    ("ope_color_filter", C.c_int, [_vp, _vp, _ip, _ip, _ip, C.POINTER(C.c_size_t)]),
    ("ope_color_filter_cloud", C.c_int, [_vp, _vp, _ip, _ip, C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_voxel_grid", C.c_int, [_vp, _vp, _fp, _fp, C.POINTER(C.c_size_t)]),
    ("ope_voxel_grid_rgb", C.c_int, [_vp, _vp, _fp, _vp, _fp, _vp, C.POINTER(C.c_size_t)]),
    ("ope_statistical_outlier_removal", C.c_int, [_vp, _vp, C.c_int, C.c_double, _ip, C.POINTER(C.c_size_t), _fp]),
    ("ope_sacia_default_params", None, [C.POINTER(SaciaParams)]),
    ("ope_sacia", C.c_int, [_vp, _vp, _fp, _vp, _vp, _fp, C.POINTER(SaciaParams), _ip, _fp, _dp, _ip]),
    ("ope_prerejective_default_params", None, [C.POINTER(PrerejectiveParams)]),
    ("ope_prerejective", C.c_int, [_vp, _vp, _fp, _vp, _vp, _fp, C.POINTER(PrerejectiveParams), _ip, C.POINTER(PrerejectiveResult), _ip]),
    ("ope_prerejective_last_stats", C.c_int, [_vp, C.POINTER(PrerejectiveStats)]),
    ("ope_prerejective_last_hypotheses", C.c_int, [_vp, _ip, _ip, C.POINTER(C.c_uint8), _fp, _ip, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_coarse_default_params", None, [C.POINTER(CoarseParams)]),
    ("ope_coarse_pose_batch", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(CoarseParams), C.POINTER(C.c_uint64),
                                         C.POINTER(CoarseBatchResult)]),
    ("ope_coarse_batch_features", C.c_int, [_vp, C.c_int, _ip, _fp, _fp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_final_default_params", None, [C.POINTER(FinalParams)]),
    ("ope_final_pose_batch", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(FinalParams), C.POINTER(C.c_uint64),
                                        C.POINTER(FinalBatchResult), _ip]),
    ("ope_final_batch_inputs", C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_feature_correspondences", C.c_int, [_vp, _fp, C.c_size_t, _fp, C.c_size_t, _ip, _ip, _fp, C.POINTER(C.c_size_t)]),
    ("ope_corr_sac_default_params", None, [C.POINTER(CorrSacParams)]),
    ("ope_corr_sac", C.c_int, [_vp, _vp, _vp, _ip, _ip, C.c_size_t, C.POINTER(CorrSacParams), _ip, C.c_size_t, C.POINTER(CorrSacResult), _ip]),
    ("ope_corr_sac_last_stats", C.c_int, [_vp, C.POINTER(CorrSacStats)]),
    ("ope_corr_sac_last_hypotheses", C.c_int, [_vp, _ip, _fp, _ip, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_prerejective_pose_batch", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(CoarseParams), C.POINTER(PrerejectiveParams),
                                              C.POINTER(C.c_uint64), C.c_int, C.POINTER(PrerejectiveBatchResult)]),
    ("ope_prerejective_batch_last_stats", C.c_int, [_vp, C.POINTER(PrerejectiveBatchStats)]),
    ("ope_prerejective_batch_hypotheses", C.c_int, [_vp, C.c_int, _ip, _ip, C.POINTER(C.c_uint8), _fp, _ip, _dp, C.c_size_t,
                                                    C.POINTER(C.c_size_t)]),
    ("ope_final_pose_batch_prerejective", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(FinalParams), C.POINTER(PrerejectiveParams),
                                                    C.POINTER(C.c_uint64), C.POINTER(FinalBatchResult), C.POINTER(C.c_int32)]),
    ("ope_corr_sac_pose_batch", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(CoarseParams), C.POINTER(CorrSacParams),
                                          C.POINTER(C.c_uint64), C.c_int, C.POINTER(CorrSacBatchResult)]),
    ("ope_corr_sac_batch_last_stats", C.c_int, [_vp, C.POINTER(CorrSacBatchStats)]),
    ("ope_corr_sac_batch_matches", C.c_int, [_vp, C.c_int, _ip, _ip, _fp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_corr_sac_batch_inliers", C.c_int, [_vp, C.c_int, _ip, _ip, _ip, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_corr_sac_batch_hypotheses", C.c_int, [_vp, C.c_int, _ip, _fp, _ip, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_final_pose_batch_correspondences", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(FinalParams), C.POINTER(CorrSacParams),
                                                       C.POINTER(C.c_uint64), C.POINTER(FinalBatchResult), C.POINTER(C.c_int32)]),
    ("ope_track_default_params", None, [C.POINTER(TrackParams)]),
    ("ope_track_gate", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(TrackParams), C.POINTER(TrackGateResult),
                                  C.POINTER(TrackCentroid)]),
    ("ope_track_pose", C.c_int, [_vp, _vp, _vp, C.c_double, C.c_int64, C.c_size_t, C.POINTER(_vp), C.POINTER(TrackParams),
                                  C.POINTER(TrackResult), C.POINTER(TrackCentroid), C.POINTER(FinalBatchResult), C.POINTER(_vp)]),
    ("ope_cluster_default_params", None, [C.POINTER(ClusterParams)]),
    ("ope_euclidean_clusters", C.c_int, [_vp, _vp, C.POINTER(ClusterParams), C.c_size_t, C.POINTER(C.c_size_t), _ip, _ip, _ip]),
    ("ope_euclidean_clusters_cloud", C.c_int, [_vp, _vp, C.POINTER(ClusterParams), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_vp),
                                                _ip, _ip]),
    ("ope_cluster_last_stats", C.c_int, [_vp, C.POINTER(ClusterStats)]),
    ("ope_region_default_params", None, [C.POINTER(RegionParams)]),
    ("ope_region_grow", C.c_int, [_vp, _vp, C.POINTER(RegionParams), _fp, _fp, C.c_size_t, C.POINTER(C.c_size_t), _ip, _ip, _ip]),
    ("ope_region_grow_cloud", C.c_int, [_vp, _vp, C.POINTER(RegionParams), _fp, _fp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_vp),
                                        _ip, _ip]),
    ("ope_region_last_stats", C.c_int, [_vp, C.POINTER(RegionStats)]),
    ("ope_region_rgb_default_params", None, [C.POINTER(RegionRgbParams)]),
    ("ope_region_grow_rgb", C.c_int, [_vp, _vp, C.POINTER(RegionRgbParams), C.c_size_t, C.POINTER(C.c_size_t), _ip, _ip, _ip]),
    ("ope_region_grow_rgb_cloud", C.c_int, [_vp, _vp, C.POINTER(RegionRgbParams), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_vp), _ip, _ip]),
    ("ope_region_rgb_last_stats", C.c_int, [_vp, C.POINTER(RegionRgbStats)]),
    ("ope_vfh_default_params", None, [C.POINTER(VfhParams)]),
    ("ope_vfh_batch", C.c_int, [_vp, C.c_size_t, C.POINTER(_vp), C.POINTER(VfhParams), _fp, _ip, _vp]),
    ("ope_vfh_last_stats", C.c_int, [_vp, C.POINTER(VfhStats)]),
    ("ope_vfh_db_create", C.c_int, [_vp, _fp, C.c_size_t, C.POINTER(_vp)]),
    ("ope_vfh_db_free", None, [_vp]),
    ("ope_vfh_db_size", C.c_size_t, [_vp]),
    ("ope_vfh_match", C.c_int, [_vp, _vp, _fp, C.c_size_t, C.c_int, _ip, _fp]),
    ("ope_vfh_recognise", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(VfhParams), C.c_int, _fp, _ip, _fp]),
    ("ope_plane_default_params", None, [C.POINTER(PlaneParams)]),
    ("ope_plane_segment", C.c_int, [_vp, _vp, C.POINTER(PlaneParams), _ip, C.c_size_t, _fp, _ip, C.POINTER(C.c_size_t), C.POINTER(_vp),
                                     C.POINTER(_vp)]),
    ("ope_plane_last_stats", C.c_int, [_vp, C.POINTER(PlaneStats)]),
    ("ope_plane_last_hypotheses", C.c_int, [_vp, _ip, _fp, _ip, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_prism_extract", C.c_int, [_vp, _vp, _fp, C.c_size_t, C.c_double, C.c_double, _ip, C.POINTER(C.c_size_t), C.POINTER(_vp), _fp]),
    ("ope_tabletop_segment", C.c_int, [_vp, _vp, C.POINTER(PlaneParams), C.POINTER(TabletopResult), C.POINTER(_vp), C.POINTER(_vp), _ip, _ip,
                                        _ip]),
    ("ope_peel_default_params", None, [C.POINTER(PeelParams)]),
    ("ope_plane_peel", C.c_int, [_vp, _vp, C.POINTER(PlaneParams), C.POINTER(PeelParams), C.c_size_t, _fp, _ip, C.POINTER(C.c_int64), _ip, _ip,
                                 C.POINTER(_vp), C.POINTER(PeelResult)]),
    ("ope_depth_sensor_params", C.c_int, [C.c_int, C.POINTER(DepthParams)]),
    ("ope_depth_to_cloud", C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(DepthParams), _fp, _fp, C.POINTER(_vp), _ip,
                                      C.POINTER(C.c_size_t)]),
    ("ope_depth_last_stats", C.c_int, [_vp, C.POINTER(DepthStats)]),
    ("ope_cloud_set_rgb", C.c_int, [_vp, _vp, _vp]),
    ("ope_cloud_has_rgb", C.c_int, [_vp]),
    ("ope_cloud_download_rgb", C.c_int, [_vp, _vp, _vp]),
    ("ope_depth_to_cloud_rgb", C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.POINTER(DepthParams), _fp, _fp,
                                          C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_cloud_download_normals", C.c_int, [_vp, _vp, _fp, _fp]),
    ("ope_mls_default_params", None, [C.POINTER(MlsParams)]),
    ("ope_mls_smooth", C.c_int, [_vp, _vp, C.POINTER(MlsParams), _fp, _fp, _fp, _ip, C.POINTER(C.c_size_t)]),
    ("ope_mls_smooth_cloud", C.c_int, [_vp, _vp, C.POINTER(MlsParams), C.POINTER(_vp), _ip, C.POINTER(C.c_size_t)]),
    ("ope_mls_last_stats", C.c_int, [_vp, C.POINTER(MlsStats)]),
    ("ope_mls_upsample_default_params", None, [C.POINTER(MlsUpsampleParams)]),
    ("ope_mls_upsample", C.c_int, [_vp, _vp, C.POINTER(MlsUpsampleParams), _fp, _fp, _fp, _ip, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_mls_upsample_cloud", C.c_int, [_vp, _vp, C.POINTER(MlsUpsampleParams), C.POINTER(_vp), _ip, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ope_mls_upsample_last_stats", C.c_int, [_vp, C.POINTER(MlsUpsampleStats)]),
]

# every symbol include/ope_batch_rejectors.h declares (the header ope.h includes for the batched entry points that take a list of
# global rejectors): bound by lib() like ABI
ABI_BATCH_REJECTORS = [
    ("ope_icp_run_batch_rejectors", C.c_int, [_vp, C.c_size_t, C.POINTER(_vp), C.POINTER(_vp), _fp, C.POINTER(IcpParams),
                                               C.POINTER(GlobalRejector), C.c_size_t, C.c_double, C.POINTER(IcpBatchResult),
                                               C.POINTER(GlobalRejectorStats), _ip, _fp]),
    ("ope_final_pose_batch_rejectors", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(FinalParams), C.POINTER(GlobalRejector),
                                                  C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(FinalBatchResult), _ip]),
]

# every symbol include/ope_device_draws.h declares (the draws of the batched prerejective aligner made on the device): bound by
# lib() like ABI.  The header has no struct: its statistics are eight int64.
ABI_DEVICE_DRAWS = [
    ("ope_prerejective_set_draws", C.c_int, [_vp, C.c_int]),
    ("ope_prerejective_get_draws", C.c_int, [_vp, _ip]),
    ("ope_prerejective_set_draws_limits", C.c_int, [_vp, C.c_int, C.c_int64]),
    ("ope_prerejective_draws_device", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_size_t, C.c_int,
                                                 C.c_int64, _ip, _ip, C.POINTER(C.c_int64)]),
    ("ope_prerejective_draws_last_stats", C.c_int, [_vp, C.POINTER(C.c_int64)]),
]
DRAWS_HOST, DRAWS_DEVICE = 0, 1
DRAWS_STATS_FIELDS = ("mode", "device", "overflow", "short", "host_for_size", "positions", "tile", "launches")

_lib = None


def lib() -> C.CDLL:
    """Load libope_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OpeError(OPE_ENODEV, f"{LIB_PATH} is missing: run __graft_entry__.build() / make -C {_HERE}")
        # torch ships its own libamdhip64.so.7 / librccl.so.1; importing it first makes this library
        # bind to the same HIP runtime (same SONAME), so streams and device pointers are shareable.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for pure C-ABI use
            pass
        L = C.CDLL(LIB_PATH)
        for name, res, args in ABI + ABI_BATCH_REJECTORS + ABI_DEVICE_DRAWS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _f32(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if cols is not None and not (a.ndim == 2 and a.shape[1] == cols):
        raise ValueError(f"expected (n,{cols}) float array, got {a.shape}")
    return a


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def colmajor(T) -> np.ndarray:
    """(4,4) math-layout matrix -> column-major float[16] (Eigen::Matrix4f memory order)."""
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16)


def from_colmajor(t16) -> np.ndarray:
    return np.asarray(t16, np.float32).reshape(4, 4).T.copy()


def _T_stack(T16) -> np.ndarray:
    """(h, 16) column-major transforms -> (h, 4, 4) math layout."""
    return T16.reshape(len(T16), 4, 4).transpose(0, 2, 1).copy()


def _set_fields(p, kw):
    """The keyword arguments of a parameter constructor onto its struct: AttributeError for a name that is no field (setattr would
    quietly make a Python attribute of it); an array field takes any sequence of its length."""
    types = dict(p._fields_)
    for k, v in kw.items():
        if k not in types:
            raise AttributeError(k)
        if issubclass(types[k], C.Array):
            getattr(p, k)[:] = list(v)
        else:
            setattr(p, k, v)
    return p


def _params(Struct, entry: str, kw):
    """Struct filled by the library's `entry`(Struct *), then the keyword arguments."""
    p = Struct()
    getattr(lib(), entry)(C.byref(p))
    return _set_fields(p, kw)


def default_depth_params(sensor="kinect", **kw) -> DepthParams:
    """ope_depth_sensor_params: one of the reference's three presets ("kinect", "astra", "euclid" or an OPE_SENSOR_* value)."""
    p = DepthParams()
    code = SENSORS[sensor] if isinstance(sensor, str) else int(sensor)
    if lib().ope_depth_sensor_params(code, C.byref(p)) != OPE_OK:
        raise ValueError(f"unknown sensor {sensor!r}")
    return _set_fields(p, kw)


def default_mls_params(**kw) -> MlsParams:
    return _params(MlsParams, "ope_mls_default_params", kw)


def default_mls_upsample_params(**kw) -> MlsUpsampleParams:
    return _params(MlsUpsampleParams, "ope_mls_upsample_default_params", kw)


def global_rejector(kind: int, **kw) -> GlobalRejector:
    """ope_global_rejector_defaults (factor 1.0, min_ratio 0.05, max_ratio 0.95) with the given fields set."""
    r = GlobalRejector()
    lib().ope_global_rejector_defaults(kind, C.byref(r))
    return _set_fields(r, kw)


def default_icp_params(**kw) -> IcpParams:
    return _params(IcpParams, "ope_icp_default_params", kw)


@dataclass
class IcpOut:
    T: np.ndarray          # (4,4) math layout, float32 — getFinalTransformation()
    iterations: int
    converged: bool
    state: int
    last_mse: float
    n_corr: int
    align_strength: float


@dataclass
class IcpBatchOut(IcpOut):
    fitness: float | None    # getFitnessScore(fitness_max_range) of T (DBL_MAX: no point in range)
    fitness_n: int | None    # points that entered it


@dataclass
class CoarseOut:
    T: np.ndarray          # (4,4) math layout, float32 — the coarse pose (identity unless status == COARSE_OK)
    best_error: float      # computeErrorMetric of the winning hypothesis
    best_iteration: int    # -1 unless COARSE_OK
    n_src_keys: int        # model key points
    n_tgt_keys: int        # this cluster's key points
    status: int            # COARSE_OK, COARSE_EMPTY_TARGET or COARSE_FEW_TARGET_FEATURES


@dataclass
class PrerejectiveOut:
    T: np.ndarray          # (4,4) math layout, float32 — getFinalTransformation(); the identity without a winner
    error: float           # the winner's mean squared inlier distance (FLT_MAX without a winner)
    best_iteration: int    # -1 without a winner
    inliers: int
    converged: bool
    inlier_idx: np.ndarray | None   # getInliers(): ORIGINAL source indices, ascending (with_inliers=True)


@dataclass
class CorrSacOut:
    T_best: np.ndarray     # (4,4) math layout, float32 — getBestTransformation(); the identity without a model
    T_svd: np.ndarray      # TransformationEstimationSVD over the remaining matches (all of them without a model)
    inliers: int           # remaining matches
    best: int              # the winning hypothesis in drawing order, -1 without a model
    iterations: int
    found: bool
    inlier_pos: np.ndarray           # positions of the remaining matches in the given ones, ascending
    matches: tuple | None = None     # (src_idx, tgt_idx, dist) when the call made them (coarse_pose_correspondences)


@dataclass
class PrerejectiveBatchOut:
    T: np.ndarray          # (4,4) math layout, float32; the identity unless converged
    error: float           # FLT_MAX without a winner
    best_iteration: int    # -1 without a winner
    inliers: int
    converged: bool
    survivors: int         # of this cluster's polygon test
    n_src_keys: int        # model key points
    n_tgt_keys: int        # this cluster's key points
    status: int            # PREREJ_OK, PREREJ_EMPTY_TARGET, PREREJ_FEW_TARGET_FEATURES or PREREJ_NAN_FEATURES
    seed: int              # the stream the cluster drew with (0 unless PREREJ_OK)
    raw: bytes             # the bytes of its ope_prerejective_batch_result


@dataclass
class CorrSacBatchOut:
    T_svd: np.ndarray      # (4,4) math layout, float32: the coarse pose; the identity unless CORRSAC_OK and matches > 0
    T_best: np.ndarray     # the winning hypothesis; the identity without a model
    sample_dist_thresh: float
    seed: int              # the stream the cluster drew with (0 unless CORRSAC_OK)
    matches: int           # model rows with a finite match in this cluster
    inliers: int           # remaining matches
    best: int              # the winning hypothesis in drawing order, -1 without a model
    iterations: int
    found: bool
    n_src_keys: int        # model key points
    n_tgt_keys: int        # this cluster's key points
    status: int            # CORRSAC_OK, CORRSAC_EMPTY_TARGET or CORRSAC_FEW_TARGET_FEATURES
    raw: bytes             # the bytes of its ope_corr_sac_batch_result


@dataclass
class FinalOut:
    coarse: CoarseOut      # the coarse stage, as coarse_pose_batch reports it
    seed: int              # the SAC-IA stream the cluster drew with (0: it did not reach SAC-IA)
    fine: IcpBatchOut | None   # the fine ICP from the identity; None unless it ran (FINAL_OK, FINAL_FEW_TARGET_FEATURES)
    n_fine_src: int        # fine key points of the moved model
    n_fine_tgt: int        # ... and of the cluster
    status: int            # FINAL_OK, FINAL_EMPTY_TARGET, FINAL_FEW_TARGET_FEATURES or FINAL_FEW_FINE_POINTS
    accepted: bool         # fitness < accept_fitness or align strength > accept_strength


@dataclass
class GateOut:
    branch: int                # TRACK_NO_CLUSTERS, TRACK_GATED, TRACK_REALIGN_ALL, TRACK_NOTHING (track_pose: TRACK_REALIGN_LOOP)
    selected: int              # the gated cluster, -1 unless TRACK_GATED
    source_centroid: np.ndarray   # (3,) float32, pcl::compute3DCentroid of the source (finite points)
    source_count: int
    centroids: np.ndarray      # (n, 3) float32, each cluster's centroid (all its points)
    counts: np.ndarray         # (n,) int32
    distances: np.ndarray      # (n,) float32, to the source centroid


@dataclass
class TrackOut:
    gate: GateOut
    selected: int              # GATED: the gated cluster; REALIGN_ALL: final_pose_batch's selected; -1 otherwise
    coarse: np.ndarray | None  # GATED: (4,4) float32 coarsePose, finePose, rigidmodelPose, finalPose = rigid * (coarse * fine)
    fine: np.ndarray | None
    rigid: np.ndarray | None
    final: np.ndarray | None
    coarse_status: int         # GATED: COARSE_* or TRACK_COARSE_SKIPPED
    seed: int                  # GATED: the SAC-IA stream (0: SAC-IA did not run)
    icp: IcpBatchOut | None    # GATED: the fine ICP with its fitness; None unless it ran
    n_fine_src: int
    n_fine_tgt: int
    status: int                # GATED: FINAL_*
    realign: list | None       # REALIGN_ALL: [FinalOut per cluster], as final_pose_batch returns them
    aligned: "Cloud | None"    # GATED: the source moved by the coarse, then the fine pose, on the device (the next source)


@dataclass
class PlaneOut:
    found: bool                # a model was found (PCL: ModelCoefficients::values not empty)
    coeff: "np.ndarray | None"  # a b c d, float32
    inliers: np.ndarray        # ORIGINAL indices, ascending
    iterations: int            # iterations RANSAC would have run
    best: int                  # the winning hypothesis
    samples: np.ndarray        # (h, 3) the drawn triples
    hyp_coeffs: np.ndarray     # (h, 4) their planes
    counts: np.ndarray         # (h,) their inlier counts
    plane: "Cloud | None"
    not_plane: "Cloud | None"
    stats: dict


@dataclass
class PeelOut:
    coeffs: np.ndarray         # (k, 4) the peeled planes, in peeling order
    counts: np.ndarray         # (k,) their inliers
    iterations: np.ndarray     # (k,) the iterations RANSAC would have run for each
    rest_idx: np.ndarray       # the remainder, ORIGINAL indices ascending
    rest: "Cloud | None"
    labels: "np.ndarray | None"  # (n,) the round that took each point, -1 for the remainder
    stop: int                  # PEEL_FRACTION / PEEL_NO_INLIERS / PEEL_MAX_PLANES
    stats: dict                # n_planes, n_rest, launches, host_syncs


@dataclass
class TabletopOut:
    status: int                # TABLETOP_OK / NO_PLANE_FIRST / NO_PLANE_SECOND
    coeff_first: np.ndarray
    coeff_second: np.ndarray
    corners: np.ndarray        # (4, 3)
    prism_idx: np.ndarray      # the prism's points, indices into the input
    plane_idx: "np.ndarray | None"
    not_plane_idx: "np.ndarray | None"
    plane: "Cloud | None"
    not_plane: "Cloud | None"
    iterations_first: int
    iterations_second: int
    launches: int
    host_syncs: int


def _gate_out(g: "TrackGateResult", cent, n: int) -> GateOut:
    return GateOut(g.branch, g.selected, np.array(g.source.centroid, np.float32), g.source.count,
                   np.array([list(c.centroid) for c in cent[:n]], np.float32).reshape(n, 3),
                   np.array([c.count for c in cent[:n]], np.int32), np.array([c.distance for c in cent[:n]], np.float32))


def _copy_struct(s):
    """An element of a ctypes array as a structure of its own (the element itself is a view of the array's memory)."""
    return type(s).from_buffer_copy(s)


def _final_out(o) -> FinalOut:
    c = o.coarse
    co = CoarseOut(from_colmajor(np.frombuffer(c.T, np.float32)), c.best_error, c.best_iteration, c.n_src_keys, c.n_tgt_keys, c.status)
    fine = None
    if o.status in (FINAL_OK, FINAL_FEW_TARGET_FEATURES):
        r = o.fine.result
        fine = IcpBatchOut(from_colmajor(np.frombuffer(o.fine.T, np.float32)), r.iterations, bool(r.converged), r.state, r.last_mse,
                           r.n_corr, r.align_strength, o.fine.fitness, o.fine.fitness_n)
    return FinalOut(co, o.seed, fine, o.n_fine_src, o.n_fine_tgt, o.status, bool(o.accepted))


class Context:
    """One ope_ctx (one GPU)."""

    def __init__(self, device: int = 0):
        h = _vp()
        rc = lib().ope_ctx_create(C.byref(h), device)
        if rc != OPE_OK:
            raise OpeError(rc, (lib().ope_last_error(None) or b"").decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib().ope_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != OPE_OK:
            raise OpeError(rc, (lib().ope_last_error(self.h) or b"").decode())

    def _stats(self, entry: str, Struct) -> dict:
        """`entry`(ctx, Struct *) as {field: value}."""
        s = Struct()
        self._chk(getattr(lib(), entry)(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Struct._fields_}

    def _read(self, entry: str, lead, outs) -> list:
        """A "size, then fill" entry point, `entry`(ctx, *lead, one pointer per output array, cap, size_t *n): ask n with no arrays,
        fetch, and return the arrays cut to n.  outs: one (dtype, trailing shape) per array."""
        fn = getattr(lib(), entry)
        n = C.c_size_t(0)
        self._chk(fn(self.h, *lead, *[None] * len(outs), 0, C.byref(n)))
        h = n.value
        arrs = [np.zeros((max(h, 1), *shape), dt) for dt, shape in outs]
        ptrs = [a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype))) for a in arrs]
        self._chk(fn(self.h, *lead, *ptrs, h, C.byref(n)))
        return [a[:h].copy() for a in arrs]

    def _segments(self, idx, off, k: int, cap: int, handles=None):
        """The segment lists idx / off of a call that reported k segments and had room for cap: the index arrays or, with the
        call's cloud handles, (Clouds, index arrays).  last_cluster_count is k, not the number written."""
        self.last_cluster_count = k
        indices = [idx[off[i]:off[i + 1]].copy() for i in range(min(k, cap))]
        if handles is None:
            return indices
        return [Cloud(self, _vp(handles[i]), len(c)) for i, c in enumerate(indices)], indices

    def set_stream(self, stream_ptr: int | None):
        self._chk(lib().ope_ctx_set_stream(self.h, _vp(stream_ptr) if stream_ptr else None))

    def sync(self):
        self._chk(lib().ope_ctx_sync(self.h))

    def profile_kernels(self, on: bool):
        """HIP-event brackets around every coarse-stage / filter kernel launch (ope_profile_kernels)."""
        self._chk(lib().ope_profile_kernels(self.h, int(on)))

    def profile_kernels_read(self) -> dict:
        """{kernel name: {"ms", "launches", "algorithmic_bytes"}} summed since profile_kernels(True)."""
        buf = (KernelTime * 32)()
        n = C.c_size_t(0)
        self._chk(lib().ope_profile_kernels_read(self.h, buf, 32, C.byref(n)))
        return {buf[i].name.decode(): {"ms": buf[i].ms, "launches": buf[i].launches, "algorithmic_bytes": buf[i].algorithmic_bytes}
                for i in range(min(n.value, 32))}

    def set_wait_limit(self, seconds: float):
        """Bound of the device-side waits of the overlapped update launches (ope_ctx_set_wait_limit)."""
        self._chk(lib().ope_ctx_set_wait_limit(self.h, float(seconds)))

    def set_tracing(self, on: bool):
        self._chk(lib().ope_ctx_set_tracing(self.h, int(on)))

    # ---- clouds / index
    def upload(self, xyz, normals=None) -> "Cloud":
        xyz = _f32(xyz, 3)
        h = _vp()
        self._chk(lib().ope_cloud_upload(self.h, xyz.ctypes.data_as(_vp), len(xyz), 12, 0, -1, C.byref(h)))
        c = Cloud(self, h, len(xyz))
        if normals is not None:
            c.set_normals(normals)
        return c

    def upload_struct(self, buf: np.ndarray, stride: int, xyz_off: int, normal_off: int = -1) -> "Cloud":
        """Upload from an array-of-structs byte buffer (e.g. pcl::PointXYZRGBNormal, stride 48)."""
        buf = np.ascontiguousarray(buf)
        n = buf.nbytes // stride
        h = _vp()
        self._chk(lib().ope_cloud_upload(self.h, buf.ctypes.data_as(_vp), n, stride, xyz_off, normal_off, C.byref(h)))
        return Cloud(self, h, n)

    def concat(self, a: "Cloud", T, b: "Cloud") -> "Cloud":
        """[T * a ; b] built on the device (BuildModel's cloudTemp = aligned + target)."""
        t = colmajor(T) if T is not None else None
        h = _vp()
        self._chk(lib().ope_cloud_concat(self.h, a.h, _p(t, _fp), b.h, C.byref(h)))
        return Cloud(self, h, a.n + b.n)

    def select(self, cloud: "Cloud", idx) -> "Cloud":
        """cloud[idx] as a new device-resident cloud (gathered on the device; normals carried)."""
        idx = np.ascontiguousarray(idx, np.int32)
        h = _vp()
        self._chk(lib().ope_cloud_select(self.h, cloud.h, _p(idx, _ip), len(idx), C.byref(h)))
        return Cloud(self, h, len(idx))

    def _filter_cloud(self, fn, cloud, args, want_idx):
        """device-resident form of a filter: (new Cloud, indices or None)"""
        out = np.empty(max(cloud.n, 1), np.int32) if want_idx else None
        n = C.c_size_t(0)
        h = _vp()
        self._chk(fn(self.h, cloud.h, *args, C.byref(h), _p(out, _ip), C.byref(n)))
        return Cloud(self, h, n.value), (out[: n.value].copy() if want_idx else None)

    def remove_nan_cloud(self, cloud: "Cloud", want_idx: bool = False):
        return self._filter_cloud(lib().ope_remove_nan_cloud, cloud, (), want_idx)

    def pass_through_cloud(self, cloud: "Cloud", lo, hi, want_idx: bool = False):
        lo = np.ascontiguousarray(lo, np.float32); hi = np.ascontiguousarray(hi, np.float32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("pass_through: lo and hi are 3-vectors")
        return self._filter_cloud(lib().ope_pass_through_cloud, cloud, (_p(lo, _fp), _p(hi, _fp)), want_idx)

    def statistical_outlier_removal_cloud(self, cloud: "Cloud", mean_k: int = 30, stddev_mul: float = 1.0, want_idx: bool = False):
        return self._filter_cloud(lib().ope_statistical_outlier_removal_cloud, cloud, (mean_k, stddev_mul), want_idx)

    def uniform_sampling_cloud(self, cloud: "Cloud", leaf: float, want_idx: bool = False):
        return self._filter_cloud(lib().ope_uniform_sampling_cloud, cloud, (leaf,), want_idx)

    def download(self, cloud: "Cloud") -> np.ndarray:
        out = np.empty((cloud.n, 3), np.float32)
        self._chk(lib().ope_cloud_download(self.h, cloud.h, _p(out, _fp)))
        return out

    def build_index(self, cloud: "Cloud", leaf_size: int | None = None, grid: bool | None = None, grid_fill: float = 0.0,
                    grid_max_cells: int = 0) -> "Index":
        p = IndexParams()
        lib().ope_index_default_params(C.byref(p))
        if leaf_size:
            p.leaf_size = leaf_size
        if grid is not None:
            p.grid = int(grid)
        p.grid_fill = grid_fill
        p.grid_max_cells = grid_max_cells
        h = _vp()
        self._chk(lib().ope_index_build(self.h, cloud.h, C.byref(p), C.byref(h)))
        return Index(self, h, cloud)

    # ---- searches
    def nn(self, queries: "Cloud", index: "Index", T=None):
        n = queries.n
        idx = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32)
        t = colmajor(T) if T is not None else None
        self._chk(lib().ope_nn_search(self.h, queries.h, index.h, _p(t, _fp), _p(idx, _ip), _p(d2, _fp)))
        return idx, d2

    def knn(self, queries: "Cloud", index: "Index", k: int, T=None):
        n = queries.n
        idx = np.empty((n, k), np.int32)
        d2 = np.empty((n, k), np.float32)
        t = colmajor(T) if T is not None else None
        self._chk(lib().ope_knn_search(self.h, queries.h, index.h, _p(t, _fp), k, _p(idx, _ip), _p(d2, _fp)))
        return idx, d2

    def radius(self, queries: "Cloud", index: "Index", radius: float, max_nn: int = 0):
        n = queries.n
        counts = np.empty(n, np.int32)
        idx = np.empty((n, max_nn), np.int32) if max_nn else None
        d2 = np.empty((n, max_nn), np.float32) if max_nn else None
        self._chk(lib().ope_radius_search(self.h, queries.h, index.h, radius, max_nn, _p(counts, _ip), _p(idx, _ip),
                                          _p(d2, _fp)))
        return counts, idx, d2

    # ---- ICP
    def icp(self, src: "Cloud", tgt: "Index", params: IcpParams | None = None, guess=None) -> IcpOut:
        p = params or default_icp_params()
        g = colmajor(guess) if guess is not None else None
        T = np.empty(16, np.float32)
        r = IcpResult()
        self._chk(lib().ope_icp_run(self.h, src.h, tgt.h if tgt is not None else None, _p(g, _fp), C.byref(p),
                                    _p(T, _fp), C.byref(r)))
        return IcpOut(from_colmajor(T), r.iterations, bool(r.converged), r.state, r.last_mse, r.n_corr, r.align_strength)

    def icp_batch(self, srcs, indexes, params: IcpParams | None = None, guesses=None, fitness_max_range: float | None = None) -> list:
        """ope_icp_run_batch: problem i registers srcs[i] to indexes[i] (guesses[i] a (4,4) or None), all in one launch.
        One IcpBatchOut per problem; fitness / fitness_n are None without fitness_max_range."""
        n, head, rng, out = self._icp_batch_args(srcs, indexes, params, guesses, fitness_max_range)
        self._chk(lib().ope_icp_run_batch(self.h, n, *head, rng, out))
        return self._icp_batch_out(out, n, fitness_max_range)

    def _icp_batch_args(self, srcs, indexes, params, guesses, fitness_max_range):
        """The arguments the batched ICP entries share: n, (sources, targets, guesses, params), the fitness range, the result array."""
        n = len(srcs)
        if len(indexes) != n:
            raise ValueError("one index per source cloud")
        p = params or default_icp_params()
        hs = (_vp * max(n, 1))(*[s.h for s in srcs])
        ht = (_vp * max(n, 1))(*[t.h if t is not None else None for t in indexes])
        g = None
        if guesses is not None:
            if len(guesses) != n:
                raise ValueError("one guess per problem")
            g = np.concatenate([colmajor(np.eye(4) if x is None else x) for x in guesses]) if n else np.zeros(16, np.float32)
        out = (IcpBatchResult * max(n, 1))()
        rng = -1.0 if fitness_max_range is None else float(fitness_max_range)
        return n, (hs, ht, _p(g, _fp), C.byref(p)), rng, out

    @staticmethod
    def _icp_batch_out(out, n, fitness_max_range):
        res = []
        for i in range(n):
            o = out[i]
            r = o.result
            res.append(IcpBatchOut(from_colmajor(np.frombuffer(o.T, np.float32)), r.iterations, bool(r.converged), r.state, r.last_mse,
                                   r.n_corr, r.align_strength, o.fitness if fitness_max_range is not None else None,
                                   o.fitness_n if fitness_max_range is not None else None))
        return res

    def icp_batch_rejectors(self, srcs, indexes, rejectors, params: IcpParams | None = None, guesses=None,
                            fitness_max_range: float | None = None, pairs: bool = False):
        """ope_icp_run_batch_rejectors: icp_batch with the global rejectors `rejectors` (GlobalRejector structures, applied in order)
        inside every problem's workgroup.  Returns (results, stats, pairs): one IcpBatchOut per problem; stats[i][k] = rejector k
        of problem i as the last iteration that searched applied it (launches 0); pairs (None unless asked for) = per problem
        (index_match, distance), addressed by ORIGINAL source index: the surviving pair's original target index and distance
        field, or -1 and 0.  An empty list without pairs is icp_batch; with pairs it runs the staged kernel with an empty list."""
        n, head, rng, out = self._icp_batch_args(srcs, indexes, params, guesses, fitness_max_range)
        rejectors = list(rejectors or [])
        k = len(rejectors)
        arr = (GlobalRejector * max(k, 1))(*rejectors)
        st = (GlobalRejectorStats * max(n * k, 1))()
        sizes = [s.n for s in srcs]
        total = int(sum(sizes))
        im = np.full(max(total, 1), -1, np.int32) if pairs else None
        dist = np.zeros(max(total, 1), np.float32) if pairs else None
        self._chk(lib().ope_icp_run_batch_rejectors(self.h, n, *head, arr, k, rng, out, st, _p(im, _ip), _p(dist, _fp)))
        stats = [[_copy_struct(st[i * k + j]) for j in range(k)] for i in range(n)]
        pr = None
        if pairs:
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            pr = [(im[off[i]:off[i + 1]].copy(), dist[off[i]:off[i + 1]].copy()) for i in range(n)]
        return self._icp_batch_out(out, n, fitness_max_range), stats, pr

    def coarse_pose_batch(self, model: "Cloud", clusters, params: CoarseParams | None = None, seeds=None) -> list:
        """ope_coarse_pose_batch: estimateCoarsePose(model, clusters[i]) for every cluster in one call; one CoarseOut each.
        seeds[i] (or params.sacia.seed + i without seeds) is cluster i's SAC-IA stream."""
        n, hc, sd = self._batch_args(clusters, seeds)
        p = params or default_coarse_params()
        out = (CoarseBatchResult * max(n, 1))()
        self._chk(lib().ope_coarse_pose_batch(self.h, model.h, n, hc, C.byref(p), sd, out))
        return [CoarseOut(from_colmajor(np.frombuffer(o.T, np.float32)), o.best_error, o.best_iteration, o.n_src_keys, o.n_tgt_keys,
                          o.status) for o in out[:n]]

    def coarse_batch_features(self, which: int):
        """What the last coarse_pose_batch computed for `which` (-1 = the model, i = cluster i): (key indices into that
        cloud, normals (m,3), FPFH (m,33)), in key-point order."""
        return tuple(self._read("ope_coarse_batch_features", (which,), [(np.int32, ()), (np.float32, (3,)), (np.float32, (33,))]))

    def _final_pose_batch(self, entry: str, model, clusters, params, extra, seeds, lst=()):
        """One of the ope_final_pose_batch* entries; extra: the coarse stage's own parameter struct, if it has one; lst: (array,
        count) of the fine ICP's global rejectors, for the entry that takes them."""
        n, hc, sd = self._batch_args(clusters, seeds)
        p = params or default_final_params()
        out = (FinalBatchResult * max(n, 1))()
        sel = C.c_int32(-1)
        self._chk(getattr(lib(), entry)(self.h, model.h, n, hc, C.byref(p), *[C.byref(q) for q in extra], *lst, sd, out, C.byref(sel)))
        return [_final_out(o) for o in out[:n]], sel.value

    def final_pose_batch(self, model: "Cloud", clusters, params: FinalParams | None = None, seeds=None):
        """ope_final_pose_batch: estimateFinalPose(model, clusters[i]) of a fresh estimator for every cluster in one call.
        Returns ([FinalOut per cluster], selected): selected = the first accepted cluster, or -1."""
        return self._final_pose_batch("ope_final_pose_batch", model, clusters, params, (), seeds)

    def final_pose_batch_rejectors(self, model: "Cloud", clusters, rejectors, params: FinalParams | None = None, seeds=None):
        """ope_final_pose_batch_rejectors: final_pose_batch whose fine ICP applies the global rejectors `rejectors` (GlobalRejector
        structures, in order) inside every cluster's workgroup; an empty list is final_pose_batch."""
        rejectors = list(rejectors or [])
        arr = (GlobalRejector * max(len(rejectors), 1))(*rejectors)
        return self._final_pose_batch("ope_final_pose_batch_rejectors", model, clusters, params, (), seeds, (arr, len(rejectors)))

    def _batch_args(self, clusters, seeds):
        n = len(clusters)
        hc = (_vp * max(n, 1))(*[c.h for c in clusters])
        sd = None
        if seeds is not None:
            if len(seeds) != n:
                raise ValueError("one seed per cluster")
            sd = (C.c_uint64 * max(n, 1))(*[int(x) for x in seeds])
        return n, hc, sd

    def prerejective_pose_batch(self, model: "Cloud", clusters, front: CoarseParams | None = None, params: PrerejectiveParams | None = None,
                                seeds=None, keep_hypotheses: bool = False) -> list:
        """ope_prerejective_pose_batch: estimateCoarsePose with the prerejective aligner of model against every cluster in one
        call; one PrerejectiveBatchOut each.  front gives key_leaf, normals_k, viewpoint, fpfh_radius; seeds[i] (or params.seed + i
        without seeds) is cluster i's stream."""
        n, hc, sd = self._batch_args(clusters, seeds)
        f = front or default_coarse_params()
        p = params or default_prerejective_params()
        out = (PrerejectiveBatchResult * max(n, 1))()
        self._chk(lib().ope_prerejective_pose_batch(self.h, model.h, n, hc, C.byref(f), C.byref(p), sd, int(bool(keep_hypotheses)), out))
        return [PrerejectiveBatchOut(from_colmajor(np.frombuffer(o.T, np.float32)), o.error, o.best_iteration, o.inliers, bool(o.converged),
                                     o.survivors, o.n_src_keys, o.n_tgt_keys, o.status, o.seed, bytes(o)) for o in out[:n]]

    def prerejective_batch_stats(self) -> dict:
        """ope_prerejective_batch_last_stats: clusters, active, iterations, survivors, launches, host_syncs, nr_samples."""
        return self._stats("ope_prerejective_batch_last_stats", PrerejectiveBatchStats)

    def prerejective_batch_hypotheses(self, which: int) -> dict:
        """ope_prerejective_batch_hypotheses of cluster `which` (after keep_hypotheses=True), in the shape of
        prerejective_hypotheses: samples index the model's key points, targets the cluster's."""
        S = int(self.prerejective_batch_stats()["nr_samples"])
        smp, tg, sv, T, inl, err = self._read("ope_prerejective_batch_hypotheses", (which,), [
            (np.int32, (S,)), (np.int32, (S,)), (np.uint8, ()), (np.float32, (16,)), (np.int32, ()), (np.float64, ())])
        return dict(samples=smp, targets=tg, survived=sv.astype(bool), T=_T_stack(T), inliers=inl, error=err)

    def prerejective_set_draws(self, mode: int):
        """ope_prerejective_set_draws: DRAWS_HOST (the default) or DRAWS_DEVICE for prerejective_pose_batch and
        final_pose_batch_prerejective from now on; the single prerejective ignores it."""
        self._chk(lib().ope_prerejective_set_draws(self.h, int(mode)))

    def prerejective_set_draws_limits(self, window: int = 0, budget: int = 0):
        """ope_prerejective_set_draws_limits: the window and the stream budget of the batched calls' device draws (0 = the
        defaults); smaller values only send more problems back to the host loop."""
        self._chk(lib().ope_prerejective_set_draws_limits(self.h, int(window), int(budget)))

    def prerejective_get_draws(self) -> int:
        mode = C.c_int(0)
        self._chk(lib().ope_prerejective_get_draws(self.h, C.byref(mode)))
        return mode.value

    def prerejective_draws_device(self, ns: int, S: int, K: int, H: int, seeds, window: int = 0, budget: int = 0):
        """ope_prerejective_draws_device: the draws of one problem per seed, made on the device.  Returns (samples, picks), each
        (len(seeds), H, S) int32, and the stats dict of prerejective_draws_stats."""
        sd = np.ascontiguousarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)
        n = len(sd)
        shape = (n, max(int(H), 0), max(int(S), 0))
        samples, picks = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        st = (C.c_int64 * 8)()
        self._chk(lib().ope_prerejective_draws_device(self.h, int(ns), int(S), int(K), int(H), _p(sd, C.POINTER(C.c_uint64)), n, int(window),
                                                      int(budget), _p(samples, _ip), _p(picks, _ip), st))
        return samples, picks, (dict(zip(DRAWS_STATS_FIELDS, (int(v) for v in st))) if n else self.prerejective_draws_stats())

    def prerejective_draws_stats(self) -> dict:
        """ope_prerejective_draws_last_stats: mode, device (problems drawn there), overflow / short (problems that fell back),
        host_for_size, positions (P), tile (T), launches of the draw stage of the last call that had one."""
        st = (C.c_int64 * 8)()
        self._chk(lib().ope_prerejective_draws_last_stats(self.h, st))
        return dict(zip(DRAWS_STATS_FIELDS, (int(v) for v in st)))

    def final_pose_batch_prerejective(self, model: "Cloud", clusters, params: FinalParams | None = None,
                                      prerejective: PrerejectiveParams | None = None, seeds=None):
        """ope_final_pose_batch_prerejective: final_pose_batch with the prerejective aligner as its coarse stage.
        Returns ([FinalOut per cluster], selected)."""
        return self._final_pose_batch("ope_final_pose_batch_prerejective", model, clusters, params,
                                      (prerejective or default_prerejective_params(),), seeds)

    def corr_sac_pose_batch(self, model: "Cloud", clusters, front: CoarseParams | None = None, params: CorrSacParams | None = None,
                            seeds=None, keep_hypotheses: bool = False) -> list:
        """ope_corr_sac_pose_batch: estimateCoarsePose with the correspondence aligner (feature matches, RANSAC rejector, SVD over
        what remains) of model against every cluster in one call; one CorrSacBatchOut each.  front gives key_leaf, normals_k,
        viewpoint, fpfh_radius; seeds[i] (or params.seed for every cluster without seeds) is cluster i's stream."""
        n, hc, sd = self._batch_args(clusters, seeds)
        f = front or default_coarse_params()
        p = params or default_corr_sac_params()
        out = (CorrSacBatchResult * max(n, 1))()
        self._chk(lib().ope_corr_sac_pose_batch(self.h, model.h, n, hc, C.byref(f), C.byref(p), sd, int(bool(keep_hypotheses)), out))
        return [CorrSacBatchOut(from_colmajor(np.array(o.T_svd, np.float32)), from_colmajor(np.array(o.T_best, np.float32)), o.sample_dist_thresh,
                                o.seed, o.matches, o.inliers, o.best, o.iterations, bool(o.found), o.n_src_keys, o.n_tgt_keys, o.status, bytes(o))
                for o in out[:n]]

    def corr_sac_batch_stats(self) -> dict:
        """ope_corr_sac_batch_last_stats: clusters, active, hypotheses, draw_lists, launches, host_syncs."""
        return self._stats("ope_corr_sac_batch_last_stats", CorrSacBatchStats)

    def corr_sac_batch_matches(self, which: int):
        """ope_corr_sac_batch_matches of cluster `which`: (model key, cluster key, squared descriptor distance), in model key order."""
        return tuple(self._read("ope_corr_sac_batch_matches", (which,), [(np.int32, ()), (np.int32, ()), (np.float32, ())]))

    def corr_sac_batch_inliers(self, which: int):
        """ope_corr_sac_batch_inliers of cluster `which`: (positions in its match list, ascending; model key; cluster key) of the
        matches that remain."""
        return tuple(self._read("ope_corr_sac_batch_inliers", (which,), [(np.int32, ()), (np.int32, ()), (np.int32, ())]))

    def corr_sac_batch_hypotheses(self, which: int) -> dict:
        """ope_corr_sac_batch_hypotheses of cluster `which` (after keep_hypotheses=True; empty otherwise), in the shape of
        corr_sac_hypotheses: samples (h, 3) match positions, T (h, 4, 4) math layout, counts (h,)."""
        smp, T, cnt = self._read("ope_corr_sac_batch_hypotheses", (which,), [(np.int32, (3,)), (np.float32, (16,)), (np.int32, ())])
        return dict(samples=smp, T=_T_stack(T), counts=cnt)

    def final_pose_batch_correspondences(self, model: "Cloud", clusters, params: FinalParams | None = None,
                                         corr_sac: CorrSacParams | None = None, seeds=None):
        """ope_final_pose_batch_correspondences: final_pose_batch with the correspondence aligner as its coarse stage.
        Returns ([FinalOut per cluster], selected)."""
        return self._final_pose_batch("ope_final_pose_batch_correspondences", model, clusters, params,
                                      (corr_sac or default_corr_sac_params(),), seeds)

    def _cluster_args(self, cloud, tolerance, min_size, max_size):
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        p = ClusterParams(float(tolerance), int(min_size), int(max_size))
        return cloud, p

    def euclidean_clusters(self, cloud, tolerance: float = 0.05, min_size: int = 300, max_size: int = 100000, want_labels: bool = False,
                           max_clusters: int | None = None):
        """ope_euclidean_clusters: pcl::EuclideanClusterExtraction (objectsegmentationplane.cpp:79-93) of a Cloud (or an (n, 3)
        array, uploaded first).  Returns the clusters as int32 arrays of ORIGINAL indices, ascending, by size descending then
        smallest index; with want_labels, (clusters, labels): labels (n,) the rank of each point's cluster or -1."""
        cloud, p = self._cluster_args(cloud, tolerance, min_size, max_size)
        n = cloud.n
        cap = n if max_clusters is None else int(max_clusters)
        idx = np.empty(max(n, 1), np.int32)
        off = np.zeros(cap + 1, np.int32)
        lab = np.empty(max(n, 1), np.int32) if want_labels else None
        k = C.c_size_t(0)
        self._chk(lib().ope_euclidean_clusters(self.h, cloud.h, C.byref(p), cap, C.byref(k), _p(idx, _ip), _p(off, _ip),
                                               _p(lab, _ip) if lab is not None else None))
        out = self._segments(idx, off, k.value, cap)
        return (out, lab[:n].copy()) if want_labels else out

    def euclidean_clusters_cloud(self, cloud, tolerance: float = 0.05, min_size: int = 300, max_size: int = 100000,
                                 max_clusters: int | None = None):
        """ope_euclidean_clusters_cloud: the clusters as new device clouds (each what select(cloud, indices) builds) and their
        indices.  Returns (clouds, indices)."""
        cloud, p = self._cluster_args(cloud, tolerance, min_size, max_size)
        n = cloud.n
        cap = n if max_clusters is None else int(max_clusters)
        idx = np.empty(max(n, 1), np.int32)
        off = np.zeros(cap + 1, np.int32)
        hs = (_vp * max(cap, 1))()
        k = C.c_size_t(0)
        self._chk(lib().ope_euclidean_clusters_cloud(self.h, cloud.h, C.byref(p), cap, C.byref(k), hs, _p(idx, _ip), _p(off, _ip)))
        return self._segments(idx, off, k.value, cap, hs)

    def cluster_stats(self) -> dict:
        """ope_cluster_last_stats: launches, host synchronisations, occupied cells and compared cell pairs of the last call."""
        return self._stats("ope_cluster_last_stats", ClusterStats)

    def region_grow(self, cloud, params: "RegionParams | None" = None, normals=None, curvature=None, max_clusters: int | None = None,
                    clouds: bool = False):
        """ope_region_grow: pcl::RegionGrowing over normals (segmentationregiongrow.cpp:9-82) of a Cloud (or an (n, 3) array,
        uploaded first).  normals (n, 3) / curvature (n,): both or neither; neither: estimated with params.normals_k and left on
        the cloud.  Returns (clusters, labels, stats): the regions in seed order as int32 arrays of ORIGINAL indices, ascending;
        labels (n,) the rank of each point's written region or -1; stats as region_stats().  With clouds=True the regions also
        come as device clouds: (clouds, clusters, stats)."""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        p = params if params is not None else default_region_params()
        n = cloud.n
        nrm = cur = None
        if normals is not None:
            nrm = _f32(normals, 3)
            if len(nrm) != n:
                raise ValueError("normals length mismatch")
        if curvature is not None:
            cur = np.ascontiguousarray(curvature, np.float32).reshape(-1)
            if len(cur) != n:
                raise ValueError("curvature length mismatch")
        pn = _p(nrm, _fp) if nrm is not None else None
        pc = _p(cur, _fp) if cur is not None else None
        cap = n if max_clusters is None else int(max_clusters)
        idx = np.empty(max(n, 1), np.int32)
        off = np.zeros(cap + 1, np.int32)
        k = C.c_size_t(0)
        if clouds:
            hs = (_vp * max(cap, 1))()
            self._chk(lib().ope_region_grow_cloud(self.h, cloud.h, C.byref(p), pn, pc, cap, C.byref(k), hs, _p(idx, _ip), _p(off, _ip)))
            return (*self._segments(idx, off, k.value, cap, hs), self.region_stats())
        lab = np.empty(max(n, 1), np.int32)
        self._chk(lib().ope_region_grow(self.h, cloud.h, C.byref(p), pn, pc, cap, C.byref(k), _p(idx, _ip), _p(off, _ip), _p(lab, _ip)))
        return self._segments(idx, off, k.value, cap), lab[:n].copy(), self.region_stats()

    def region_stats(self) -> dict:
        """ope_region_last_stats: launches, host synchronisations, sweeps, one-way edges, regions before the size filter and the
        points refused for their curvature, of the last region_grow."""
        return self._stats("ope_region_last_stats", RegionStats)

    def region_grow_rgb(self, cloud: "Cloud", params: "RegionRgbParams | None" = None, max_clusters: int | None = None, clouds: bool = False):
        """ope_region_grow_rgb: pcl::RegionGrowingRGB (segmentationregiongrow.cpp:85-151) of a Cloud with colours (set_rgb).
        Returns (clusters, labels, stats): the regions in PCL's order as int32 arrays of ORIGINAL indices, ascending; labels (n,) the
        index of each point's written region or -1; stats as region_rgb_stats().  With clouds=True the regions also come as device
        clouds (colours and normals carried): (clouds, clusters, stats)."""
        p = params if params is not None else default_region_rgb_params()
        n = cloud.n
        cap = n if max_clusters is None else int(max_clusters)
        idx = np.empty(max(n, 1), np.int32)
        off = np.zeros(cap + 1, np.int32)
        k = C.c_size_t(0)
        if clouds:
            hs = (_vp * max(cap, 1))()
            self._chk(lib().ope_region_grow_rgb_cloud(self.h, cloud.h, C.byref(p), cap, C.byref(k), hs, _p(idx, _ip), _p(off, _ip)))
            return (*self._segments(idx, off, k.value, cap, hs), self.region_rgb_stats())
        lab = np.empty(max(n, 1), np.int32)
        self._chk(lib().ope_region_grow_rgb(self.h, cloud.h, C.byref(p), cap, C.byref(k), _p(idx, _ip), _p(off, _ip), _p(lab, _ip)))
        return self._segments(idx, off, k.value, cap), lab[:n].copy(), self.region_rgb_stats()

    def region_rgb_stats(self) -> dict:
        """ope_region_rgb_last_stats: launches, host synchronisations, sweeps, one-way edges, segments, directed segment pairs,
        homogeneous regions, regions absorbed by the small-region merge and regions before the size filter, of the last
        region_grow_rgb."""
        return self._stats("ope_region_rgb_last_stats", RegionRgbStats)

    # ---- recognition (vfh.hip)
    def _vfh_clusters(self, clusters):
        cl = [c if isinstance(c, Cloud) else self.upload(c) for c in clusters]
        hs = (_vp * max(len(cl), 1))(*[c.h for c in cl])
        return cl, hs

    def vfh(self, clusters, params: "VfhParams | None" = None, want_counts: bool = False, want_bins: bool = False):
        """ope_vfh_batch: one pcl::VFHEstimation signature (308 bins, PCL's defaults) per cluster, every cluster in the same
        launches.  clusters: Clouds (or (n, 3) arrays, uploaded first); a cloud without normals gets the k = params.normals_k
        estimate, left on it.  Returns the (n, 308) float32 signatures; with want_counts / want_bins a tuple (signatures, counts
        (n, 308) int32 or None, bins (total points, 4) uint8 or None): per point the f1, f2, f3 bins (255: rejected pair) and the
        viewpoint bin, clusters packed in call order, each in its original order."""
        cl, hs = self._vfh_clusters(clusters)
        n = len(cl)
        p = params if params is not None else default_vfh_params()
        out = np.zeros((n, 308), np.float32)
        counts = np.zeros((n, 308), np.int32) if want_counts else None
        bins = np.zeros((max(sum(c.n for c in cl), 1), 4), np.uint8) if want_bins else None
        self._chk(lib().ope_vfh_batch(self.h, n, hs, C.byref(p), _p(out, _fp), _p(counts, _ip), _p(bins, _vp)))
        if not (want_counts or want_bins):
            return out
        return out, counts, (bins[:sum(c.n for c in cl)] if bins is not None else None)

    def vfh_db(self, rows) -> "VfhDb":
        """ope_vfh_db_create: a table of trained signatures (m, 308) kept on the device."""
        rows = _f32(rows, 308)
        h = _vp()
        self._chk(lib().ope_vfh_db_create(self.h, _p(rows, _fp), len(rows), C.byref(h)))
        return VfhDb(self, h, len(rows))

    def vfh_match(self, db: "VfhDb | None", queries, k: int = 15):
        """ope_vfh_match: the k nearest rows of every query (q, 308) by chi-square distance, exact; (indices (q, k) int32,
        distances (q, k) float32), -1 / +inf past the table's size."""
        qs = _f32(queries, 308)
        kk = max(int(k), 1)
        idx = np.zeros((len(qs), kk), np.int32)
        dist = np.zeros((len(qs), kk), np.float32)
        self._chk(lib().ope_vfh_match(self.h, db.h if db is not None else None, _p(qs, _fp), len(qs), int(k), _p(idx, _ip), _p(dist, _fp)))
        return idx, dist

    def vfh_recognise(self, db: "VfhDb | None", clusters, k: int = 15, params: "VfhParams | None" = None, want_signatures: bool = False):
        """ope_vfh_recognise: vfh + vfh_match of every cluster with the signatures never leaving the device; (indices, distances)
        or, with want_signatures, (indices, distances, signatures)."""
        cl, hs = self._vfh_clusters(clusters)
        n = len(cl)
        p = params if params is not None else default_vfh_params()
        kk = max(int(k), 1)
        idx = np.zeros((n, kk), np.int32)
        dist = np.zeros((n, kk), np.float32)
        sig = np.zeros((n, 308), np.float32) if want_signatures else None
        self._chk(lib().ope_vfh_recognise(self.h, db.h if db is not None else None, n, hs, C.byref(p), int(k), _p(sig, _fp), _p(idx, _ip),
                                          _p(dist, _fp)))
        return (idx, dist, sig) if want_signatures else (idx, dist)

    def vfh_stats(self) -> dict:
        """ope_vfh_last_stats: points, rejected pairs, clouds whose normals were estimated, empty clouds, launches and host
        synchronisations of the last vfh / vfh_match / vfh_recognise."""
        return self._stats("ope_vfh_last_stats", VfhStats)

    def plane_segment(self, cloud, params: "PlaneParams | None" = None, samples=None, want_clouds: bool = False) -> "PlaneOut":
        """ope_plane_segment: pcl::SACSegmentation (SACMODEL_PLANE, SAC_RANSAC; objectsegmentationplane.cpp:36-55) of a Cloud (or
        an (n, 3) array, uploaded first).  samples: (k, 3) ORIGINAL indices taken instead of the draws."""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        p = params if params is not None else default_plane_params()
        smp = np.ascontiguousarray(samples, np.int32).reshape(-1, 3) if samples is not None else None
        coeff = np.zeros(4, np.float32)
        idx = np.empty(max(cloud.n, 1), np.int32)
        k = C.c_size_t(0)
        hp, hn = _vp(), _vp()
        self._chk(lib().ope_plane_segment(self.h, cloud.h, C.byref(p), _p(smp, _ip) if smp is not None and len(smp) else None,
                                          len(smp) if smp is not None else 0, _p(coeff, _fp), _p(idx, _ip), C.byref(k),
                                          C.byref(hp) if want_clouds else None, C.byref(hn) if want_clouds else None))
        st = self.plane_stats()
        hs, hc, hk = self.plane_hypotheses()
        plane = Cloud(self, hp, k.value) if want_clouds else None
        rest = Cloud(self, hn, cloud.n - k.value) if want_clouds else None
        return PlaneOut(bool(st["found"]), coeff if st["found"] else None, idx[: k.value].copy(), st["iterations"], st["best"], hs, hc, hk,
                        plane, rest, st)

    def plane_stats(self) -> dict:
        """ope_plane_last_stats: iterations, hypotheses scored, launches, host synchronisations, winner, found."""
        return self._stats("ope_plane_last_stats", PlaneStats)

    def plane_hypotheses(self):
        """ope_plane_last_hypotheses: (samples (h, 3) int32, coefficients (h, 4) float32, counts (h,) int32) in drawing order."""
        return tuple(self._read("ope_plane_last_hypotheses", (), [(np.int32, (3,)), (np.float32, (4,)), (np.int32, ())]))

    def prism_extract(self, cloud, hull, height_min: float = 0.0, height_max: float = float(np.finfo(np.float32).max),
                      want_cloud: bool = False):
        """ope_prism_extract: pcl::ExtractPolygonalPrismData (viewpoint 0 0 0).  Returns (indices, hull plane (4,), Cloud or None)."""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        hull = _f32(hull, 3)
        idx = np.empty(max(cloud.n, 1), np.int32)
        k = C.c_size_t(0)
        h = _vp()
        hc = np.zeros(4, np.float32)
        self._chk(lib().ope_prism_extract(self.h, cloud.h, _p(hull, _fp), len(hull), float(height_min), float(height_max), _p(idx, _ip),
                                          C.byref(k), C.byref(h) if want_cloud else None, _p(hc, _fp)))
        return idx[: k.value].copy(), hc, (Cloud(self, h, k.value) if want_cloud else None)

    def tabletop_segment(self, cloud, params: "PlaneParams | None" = None) -> "TabletopOut":
        """ope_tabletop_segment: getSegmentedObjectsOnPlane up to getClusters (objectsegmentationplane.cpp:124-235)."""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        p = params if params is not None else default_plane_params()
        r = TabletopResult()
        hp, hn = _vp(), _vp()
        n1 = max(cloud.n, 1)
        pi, li, ni = np.empty(n1, np.int32), np.empty(n1, np.int32), np.empty(n1, np.int32)
        self._chk(lib().ope_tabletop_segment(self.h, cloud.h, C.byref(p), C.byref(r), C.byref(hp), C.byref(hn), _p(pi, _ip), _p(li, _ip),
                                             _p(ni, _ip)))
        ok = r.status == TABLETOP_OK
        return TabletopOut(r.status, np.array(r.coeff_first, np.float32), np.array(r.coeff_second, np.float32),
                           np.array(r.corners, np.float32).reshape(4, 3), pi[: r.n_prism].copy(),
                           li[: r.n_plane].copy() if ok else None, ni[: r.n_not_plane].copy() if ok else None,
                           Cloud(self, hp, r.n_plane) if ok else None, Cloud(self, hn, r.n_not_plane) if ok else None,
                           r.iterations_first, r.iterations_second, r.launches, r.host_syncs)

    def plane_peel(self, cloud, params: "PlaneParams | None" = None, keep_fraction: float = 0.3, max_planes: int = 0, want_cloud: bool = False,
                   want_labels: bool = False) -> "PeelOut":
        """ope_plane_peel: the loop of getSegmentedObjectsExceptPlane (objectsegmentationplane.cpp:296-319) on a Cloud (or an (n, 3)
        array, uploaded first): fit the dominant plane and remove its inliers until at most keep_fraction of the points are left."""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        p = params if params is not None else default_plane_params()
        q = PeelParams(float(keep_fraction), int(max_planes))
        r = PeelResult()
        n1 = max(cloud.n, 1)
        rest_idx = np.empty(n1, np.int32)
        lab = np.empty(n1, np.int32) if want_labels else None
        h = _vp()
        cap = 32
        while True:   # (a second call only for more planes than the first one had room for)
            coeffs, counts, its = np.zeros((cap, 4), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
            self._chk(lib().ope_plane_peel(self.h, cloud.h, C.byref(p), C.byref(q), cap, _p(coeffs, _fp), _p(counts, _ip),
                                           its.ctypes.data_as(C.POINTER(C.c_int64)), _p(lab, _ip) if lab is not None else None,
                                           _p(rest_idx, _ip), C.byref(h) if want_cloud else None, C.byref(r)))
            if r.n_planes <= cap:
                break
            if want_cloud:
                Cloud(self, h, r.n_rest).free()
                h = _vp()
            cap = r.n_planes
        k = r.n_planes
        stats = dict(n_planes=k, n_rest=r.n_rest, launches=r.launches, host_syncs=r.host_syncs)
        return PeelOut(coeffs[:k].copy(), counts[:k].copy(), its[:k].copy(), rest_idx[: r.n_rest].copy(),
                       Cloud(self, h, r.n_rest) if want_cloud else None, lab[: cloud.n].copy() if lab is not None else None, r.stop, stats)

    def except_plane_segment(self, cloud, params: "PlaneParams | None" = None, keep_fraction: float = 0.3, max_planes: int = 0,
                             tolerance: float = 0.05, min_size: int = 300, max_size: int = 100000, want_clouds: bool = False):
        """getSegmentedObjectsExceptPlane after its crop (objectsegmentationplane.cpp:296-324): plane_peel, then euclidean_clusters
        of the remainder.  Returns (clusters, peel): the clusters as int32 arrays of indices into the INPUT cloud, ascending, in
        euclidean_clusters' order; with want_clouds, (cluster clouds, clusters, peel)."""
        if not isinstance(cloud, Cloud):
            cloud = self.upload(cloud)
        peel = self.plane_peel(cloud, params, keep_fraction, max_planes, want_cloud=True)
        if want_clouds:
            clouds, local = self.euclidean_clusters_cloud(peel.rest, tolerance, min_size, max_size)
            return clouds, [peel.rest_idx[c] for c in local], peel
        local = self.euclidean_clusters(peel.rest, tolerance, min_size, max_size)
        return [peel.rest_idx[c] for c in local], peel

    def depth_to_cloud(self, depth, params: "DepthParams | None" = None, lo=None, hi=None, want_pixels: bool = False, bgr=None):
        """ope_depth_to_cloud: a (rows, cols) uint16 depth image -> the frame's Cloud (rgbd2Pcl, optionally cropped to lo .. hi).
        Rows may be strided (a view with a row pitch); samples within a row must be contiguous.  Returns the Cloud, or
        (Cloud, pixel indices row * cols + col) with want_pixels.
        bgr: a (rows, cols, 3) uint8 image, channels B, G, R (rows may be strided too): ope_depth_to_cloud_rgb, the same cloud
        carrying r << 16 | g << 8 | b of every point's pixel (Cloud.download_rgb)."""
        depth = np.asarray(depth)
        if depth.dtype != np.uint16 or depth.ndim != 2:
            raise ValueError("depth_to_cloud: expected a 2-D uint16 image")
        rows, cols = depth.shape
        if rows * cols and (depth.strides[1] != 2 or (rows > 1 and depth.strides[0] < 2 * cols)):
            depth = np.ascontiguousarray(depth)
        stride = depth.strides[0] if rows > 1 and rows * cols else 2 * cols
        if (lo is None) != (hi is None):
            raise ValueError("depth_to_cloud: give both lo and hi, or neither")
        if lo is not None:
            lo = np.ascontiguousarray(lo, np.float32); hi = np.ascontiguousarray(hi, np.float32)
            if lo.shape != (3,) or hi.shape != (3,):
                raise ValueError("depth_to_cloud: lo and hi are 3-vectors")
        p = params if params is not None else default_depth_params()
        pix = np.empty(max(rows * cols, 1), np.int32) if want_pixels else None
        n = C.c_size_t(0)
        h = _vp()
        if bgr is not None:
            bgr = np.asarray(bgr)
            if bgr.dtype != np.uint8 or bgr.shape != (rows, cols, 3):
                raise ValueError("depth_to_cloud: bgr is a (rows, cols, 3) uint8 image of the depth image's size")
            if rows * cols and (bgr.strides[2] != 1 or bgr.strides[1] != 3 or (rows > 1 and bgr.strides[0] < 3 * cols)):
                bgr = np.ascontiguousarray(bgr)
            bstride = bgr.strides[0] if rows > 1 and rows * cols else 3 * cols
            self._chk(lib().ope_depth_to_cloud_rgb(self.h, _vp(depth.ctypes.data), rows, cols, stride, _vp(bgr.ctypes.data), bstride, C.byref(p),
                                                   _p(lo, _fp), _p(hi, _fp), C.byref(h), _p(pix, _ip), C.byref(n)))
        else:
            self._chk(lib().ope_depth_to_cloud(self.h, _vp(depth.ctypes.data), rows, cols, stride, C.byref(p), _p(lo, _fp), _p(hi, _fp),
                                               C.byref(h), _p(pix, _ip), C.byref(n)))
        c = Cloud(self, h, n.value)
        return (c, pix[: n.value].copy()) if want_pixels else c

    def depth_stats(self) -> dict:
        """ope_depth_last_stats: launches, host synchronisations, pixels, valid pixels, points kept."""
        return self._stats("ope_depth_last_stats", DepthStats)

    def track_gate(self, source: "Cloud", clusters, params: TrackParams | None = None) -> GateOut:
        """ope_track_gate: the centroid gate of the reference's later frames (rosinterface.cpp:264-304)."""
        n = len(clusters)
        hc = (_vp * max(n, 1))(*[c.h for c in clusters])
        out = TrackGateResult()
        cent = (TrackCentroid * max(n, 1))()
        self._chk(lib().ope_track_gate(self.h, source.h, n, hc, C.byref(params) if params else None, C.byref(out), cent))
        return _gate_out(out, cent, n)

    def track_pose(self, model: "Cloud", source: "Cloud", clusters, fitness_fine: float = 10.0, coarse_calls: int = 0,
                   params: TrackParams | None = None) -> TrackOut:
        """ope_track_pose: one later frame of the reference (the gate, then the gated estimateFinalPose or the re-align).
        fitness_fine / coarse_calls: the estimator's state on entry (a fresh one: 10.0 and 0)."""
        n = len(clusters)
        hc = (_vp * max(n, 1))(*[c.h for c in clusters])
        out = TrackResult()
        cent = (TrackCentroid * max(n, 1))()
        re = (FinalBatchResult * max(n, 1))()
        h = _vp()
        self._chk(lib().ope_track_pose(self.h, model.h, source.h, float(fitness_fine), int(coarse_calls), n, hc,
                                       C.byref(params) if params else None, C.byref(out), cent, re, C.byref(h)))
        gate = _gate_out(out.gate, cent, n)
        gated = out.gate.branch == TRACK_GATED
        mat = (lambda t: from_colmajor(np.frombuffer(t, np.float32))) if gated else (lambda t: None)
        icp = None
        if gated and out.status in (FINAL_OK, FINAL_FEW_TARGET_FEATURES):
            r = out.icp
            icp = IcpBatchOut(mat(out.fine), r.iterations, bool(r.converged), r.state, r.last_mse, r.n_corr, r.align_strength,
                              out.fitness, out.fitness_n)
        realign = [_final_out(o) for o in re[:n]] if out.gate.branch == TRACK_REALIGN_ALL else None
        aligned = Cloud(self, h, source.n) if h.value else None
        return TrackOut(gate, out.selected, mat(out.coarse), mat(out.fine), mat(out.rigid), mat(out.final_pose), out.coarse_status,
                        out.seed, icp, out.n_fine_src, out.n_fine_tgt, out.status, realign, aligned)

    def final_batch_inputs(self, which: int, side: int):
        """The fine inputs the last final_pose_batch prepared for cluster `which`: side 0 the moved model, 1 the cluster.
        (xyz (m,3), normals (m,3)) in key-point order, as they would be uploaded."""
        return tuple(self._read("ope_final_batch_inputs", (which, side), [(np.float32, (3,)), (np.float32, (3,))]))

    def icp_begin(self, src: "Cloud", tgt: "Index", params: IcpParams | None = None, guess=None):
        p = params or default_icp_params()
        g = colmajor(guess) if guess is not None else None
        self._chk(lib().ope_icp_begin(self.h, src.h, tgt.h, _p(g, _fp), C.byref(p)))

    def icp_accumulate(self):
        self._chk(lib().ope_icp_accumulate(self.h))

    def icp_sums_ptr(self) -> int:
        return int(lib().ope_icp_sums_device(self.h) or 0)

    def icp_update(self):
        self._chk(lib().ope_icp_update(self.h))

    def icp_set_sums_buffer(self, device_ptr: int | None):
        self._chk(lib().ope_icp_set_sums_buffer(self.h, _vp(device_ptr) if device_ptr else None))

    def icp_iterate(self, n: int = 1):
        self._chk(lib().ope_icp_iterate(self.h, n))

    def icp_profile(self, max_launches: int):
        self._chk(lib().ope_icp_profile(self.h, max_launches))

    def icp_profile_read(self):
        ms = C.c_double(0); n = C.c_int(0)
        self._chk(lib().ope_icp_profile_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def icp_poll(self) -> IcpResult:
        r = IcpResult()
        self._chk(lib().ope_icp_poll(self.h, C.byref(r)))
        return r

    def icp_current_transform(self) -> np.ndarray:
        """(4,4) final transformation after the iterations enqueued so far (synchronises)."""
        T = np.empty(16, np.float32)
        self._chk(lib().ope_icp_current_transform(self.h, _p(T, _fp)))
        return from_colmajor(T)

    def icp_end(self) -> IcpOut:
        T = np.empty(16, np.float32)
        r = IcpResult()
        self._chk(lib().ope_icp_end(self.h, _p(T, _fp), C.byref(r)))
        return IcpOut(from_colmajor(T), r.iterations, bool(r.converged), r.state, r.last_mse, r.n_corr, r.align_strength)

    def icp_profile_launches(self, cap: int = 4096) -> np.ndarray:
        """HIP-event duration (ms) of each accumulate launch timed since icp_profile(n)."""
        ms = np.empty(cap, np.float32)
        n = C.c_size_t(0)
        self._chk(lib().ope_icp_profile_launches(self.h, _p(ms, _fp), cap, C.byref(n)))
        return ms[: n.value].copy()

    def icp_kernel_launches(self) -> dict:
        """Accumulate launches of the current / last run per search kernel: {'grid', 'tree_lane', 'tree_packet', 'knn'}."""
        c = (C.c_int64 * 4)()
        self._chk(lib().ope_icp_kernel_launches(self.h, c))
        return dict(zip(("grid", "tree_lane", "tree_packet", "knn"), (int(v) for v in c)))

    def icp_set_fixed_correspondences(self, src: "Cloud", tgt_cloud: "Cloud", index_query=None, index_match=None):
        """setFixedCorrespondences (icp_mod.h:268): pairs by original indices, for every later run over these clouds; no indices = clear."""
        q = np.ascontiguousarray(index_query if index_query is not None else [], np.int32)
        m = np.ascontiguousarray(index_match if index_match is not None else [], np.int32)
        assert len(q) == len(m)
        self._chk(lib().ope_icp_set_fixed_correspondences(self.h, src.h if src is not None else None, tgt_cloud.h if tgt_cloud is not None else None,
                                                          q.ctypes.data_as(C.POINTER(C.c_int32)), m.ctypes.data_as(C.POINTER(C.c_int32)), len(q)))

    def icp_fixed_correspondences(self):
        """The given pairs as the last iteration saw them: (distance field the reference writes back through the caller's pointer,
        listed in front of the searched pairs, appended behind them) — correspondence_estimation_mod.hpp:150-161, icp_mod.hpp:210-224."""
        n = C.c_size_t(0)
        self._chk(lib().ope_icp_fixed_correspondences(self.h, None, None, None, 0, C.byref(n)))
        d, a, b = np.zeros(n.value, np.float32), np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        if n.value:
            self._chk(lib().ope_icp_fixed_correspondences(self.h, d.ctypes.data_as(C.POINTER(C.c_float)), a.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          b.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)))
        return d, a.astype(bool), b.astype(bool)

    def icp_overlapped_updates(self) -> int:
        """Update steps of the current / last run that were launched overlapped (ope_icp_params.update_launch)."""
        return int(lib().ope_icp_overlapped_updates(self.h))

    def icp_update_fallbacks(self) -> int:
        """Runs of this context that resumed in line after an overlapped update launch gave up its bounded wait (ope.h)."""
        return int(lib().ope_icp_update_fallbacks(self.h))

    def icp_certificate_stats(self) -> dict:
        """Skip certificates of the run in progress (ope_icp_params.skip_certificates): queries answered from their certificate
        (summed over the launches), launches that kept certificates, whether the run keeps them now, the last update's largest
        scene displacement in metres."""
        c = (C.c_int64 * 4)()
        self._chk(lib().ope_icp_certificate_stats(self.h, c))
        return {"certified": int(c[0]), "launches": int(c[1]), "on": bool(c[2]), "last_move": c[3] * 1e-9}

    def icp_set_global_sizes(self, n_src_total: int, n_tgt_total: int):
        self._chk(lib().ope_icp_set_global_sizes(self.h, n_src_total, n_tgt_total))

    def icp_correspondences(self, cap: int):
        q = np.empty(cap, np.int32); m = np.empty(cap, np.int32); d = np.empty(cap, np.float32)
        n = C.c_size_t(0)
        self._chk(lib().ope_icp_correspondences(self.h, _p(q, _ip), _p(m, _ip), _p(d, _fp), cap, C.byref(n)))
        k = min(n.value, cap)
        return q[:k], m[:k], d[:k]

    def icp_last_incremental(self) -> np.ndarray:
        T = np.empty(16, np.float32)
        self._chk(lib().ope_icp_last_incremental(self.h, _p(T, _fp)))
        return from_colmajor(T)

    def reject_pairs(self, kind: int, a, b, threshold: float) -> np.ndarray:
        """CorrespondenceRejector predicates on given pairs (0: surface normal a.b, 1: self-occluded a.(-b/|b|)): bool mask."""
        a, b = _f32(a, 3), _f32(b, 3)
        keep = np.zeros(len(a), np.uint8)
        self._chk(lib().ope_reject_pairs(self.h, kind, _p(a, _fp), _p(b, _fp), len(a), threshold, keep.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return keep.astype(bool)

    def icp_set_global_rejectors(self, rejectors=None):
        """The global correspondence rejectors of every later ope_icp_run / step-wise run of this context, applied in order after
        the search (ope.h): GlobalRejector structures (global_rejector(...)); None or an empty list clears."""
        rejectors = list(rejectors or [])
        arr = (GlobalRejector * max(len(rejectors), 1))(*rejectors)
        self._chk(lib().ope_icp_set_global_rejectors(self.h, arr, len(rejectors)))

    def icp_global_rejector_stats(self, i: int) -> GlobalRejectorStats:
        """Rejector i of the list as the last iteration of the last run applied it."""
        st = GlobalRejectorStats()
        self._chk(lib().ope_icp_global_rejector_stats(self.h, i, C.byref(st)))
        return st

    def reject_correspondences(self, rej: GlobalRejector, index_query, index_match, distance):
        """getRemainingCorrespondences of one global rejector on given pairs: (bool mask in the order given, GlobalRejectorStats)."""
        d = np.ascontiguousarray(distance, np.float32)
        q = np.ascontiguousarray(index_query, np.int32) if index_query is not None else None
        m = np.ascontiguousarray(index_match, np.int32) if index_match is not None else None
        keep = np.zeros(len(d), np.uint8)
        st = GlobalRejectorStats()
        self._chk(lib().ope_reject_correspondences(self.h, C.byref(rej), _p(q, _ip) if q is not None else None, _p(m, _ip) if m is not None else None,
                                                   _p(d, _fp), len(d), keep.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(st)))
        return keep.astype(bool), st

    def fitness(self, src: "Cloud", tgt: "Index", T, max_range: float = float(np.finfo(np.float64).max)):
        t = colmajor(T)
        score = C.c_double(0); s = C.c_double(0); n = C.c_int64(0)
        self._chk(lib().ope_fitness(self.h, src.h, tgt.h, _p(t, _fp), max_range, C.byref(score), C.byref(s), C.byref(n)))
        return score.value, s.value, n.value

    def rigid_transform_svd(self, src_xyz, tgt_xyz) -> np.ndarray:
        a, b = _f32(src_xyz, 3), _f32(tgt_xyz, 3)
        if len(a) != len(b):
            raise ValueError("paired arrays must have equal length")
        T = np.empty(16, np.float32)
        self._chk(lib().ope_rigid_transform_svd(self.h, _p(a, _fp), _p(b, _fp), len(a), _p(T, _fp)))
        return from_colmajor(T)

    def transform_cloud(self, cloud: "Cloud", T) -> np.ndarray:
        out = np.empty((cloud.n, 3), np.float32)
        t = colmajor(T)
        self._chk(lib().ope_transform_cloud(self.h, cloud.h, _p(t, _fp), _p(out, _fp)))
        return out

    # ---- RCCL
    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        self._chk(lib().ope_comm_init_rank(self.h, unique_id, nranks, rank))

    def comm_destroy(self):
        self._chk(lib().ope_comm_destroy(self.h))

    def comm_p2p_open(self) -> bytes:
        """Allocate this rank's slot buffer; returns its 64-byte hipIpc handle (to be passed to every rank)."""
        buf = C.create_string_buffer(64)
        self._chk(lib().ope_comm_p2p_open(self.h, buf))
        return buf.raw

    def comm_p2p_connect(self, handles, rank: int):
        """Collective: map the peers' buffers (handles in rank order) and run the test exchange."""
        blob = b"".join(handles)
        assert len(blob) == 64 * len(handles)
        self._chk(lib().ope_comm_p2p_connect(self.h, blob, len(handles), rank))

    def comm_set_transport(self, transport: int):
        """COMM_AUTO (peer-to-peer slots if every rank set them up, else RCCL), COMM_RCCL, COMM_P2P (or an error)."""
        self._chk(lib().ope_comm_set_transport(self.h, int(transport)))

    def comm_transport(self) -> int:
        """What iterations of a sharded run will use: COMM_RCCL or COMM_P2P (0 without a communicator)."""
        return int(lib().ope_comm_transport(self.h))

    # ---- features
    def normals(self, cloud: "Cloud", k: int = 30, vp=(0.0, 0.0, 0.0), fetch: bool = True):
        """pcl::NormalEstimation (k-NN).  The normals stay attached to `cloud` on the device; fetch=False skips the
        copy back to the host and returns None."""
        v = np.asarray(vp, np.float32)
        if not fetch:
            self._chk(lib().ope_normals(self.h, cloud.h, k, _p(v, _fp), None, None))
            return None
        nrm = np.empty((cloud.n, 3), np.float32)
        curv = np.empty(cloud.n, np.float32)
        self._chk(lib().ope_normals(self.h, cloud.h, k, _p(v, _fp), _p(nrm, _fp), _p(curv, _fp)))
        return nrm, curv

    def normals_from(self, queries: "Cloud", index: "Index", k: int = 30, vp=(0.0, 0.0, 0.0), fetch: bool = True):
        """Normals of `queries` from their k nearest neighbours in `index` (setSearchSurface); attached to `queries`."""
        v = np.asarray(vp, np.float32)
        if not fetch:
            self._chk(lib().ope_normals_from(self.h, queries.h, index.h, k, _p(v, _fp), None, None))
            return None
        nrm = np.empty((queries.n, 3), np.float32)
        curv = np.empty(queries.n, np.float32)
        self._chk(lib().ope_normals_from(self.h, queries.h, index.h, k, _p(v, _fp), _p(nrm, _fp), _p(curv, _fp)))
        return nrm, curv

    def fpfh(self, cloud: "Cloud", radius: float) -> np.ndarray:
        out = np.empty((cloud.n, 33), np.float32)
        self._chk(lib().ope_fpfh(self.h, cloud.h, radius, _p(out, _fp)))
        return out

    def uniform_sampling(self, cloud: "Cloud", leaf: float) -> np.ndarray:
        out = np.empty(cloud.n, np.int32)
        n = C.c_size_t(0)
        self._chk(lib().ope_uniform_sampling(self.h, cloud.h, leaf, _p(out, _ip), C.byref(n)))
        return out[: n.value].copy()

    # ---- filters either side of the path
    def remove_nan(self, cloud: "Cloud") -> np.ndarray:
        """pcl::removeNaNFromPointCloud: original indices of the finite points, ascending."""
        out = np.empty(max(cloud.n, 1), np.int32)
        n = C.c_size_t(0)
        self._chk(lib().ope_remove_nan(self.h, cloud.h, _p(out, _ip), C.byref(n)))
        return out[: n.value].copy()

    def pass_through(self, cloud: "Cloud", lo, hi) -> np.ndarray:
        """pcl::PassThrough on x, y and z (inclusive limits): original indices of the survivors, ascending."""
        lo = np.ascontiguousarray(lo, np.float32); hi = np.ascontiguousarray(hi, np.float32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("pass_through: lo and hi are 3-vectors")
        out = np.empty(max(cloud.n, 1), np.int32)
        n = C.c_size_t(0)
        self._chk(lib().ope_pass_through(self.h, cloud.h, _p(lo, _fp), _p(hi, _fp), _p(out, _ip), C.byref(n)))
        return out[: n.value].copy()

    def color_filter(self, cloud: "Cloud", lo, hi, as_cloud: bool = False):
        """ProcessingPcd::getFilterRgb's condition (pcl::ConditionalRemoval over PackedRGBComparison): original indices, ascending, of
        the points with lo[c] < channel_c < hi[c] for c = r, g, b (strict; the coordinates play no part).  as_cloud=True: (the
        passing points as a new device cloud, colours and normals carried, those indices).  OpeError(OPE_EINVAL) for a cloud
        without colours."""
        lo = np.ascontiguousarray(lo, np.int32); hi = np.ascontiguousarray(hi, np.int32)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("color_filter: lo and hi are 3-vectors (r, g, b)")
        if as_cloud:
            return self._filter_cloud(lib().ope_color_filter_cloud, cloud, (_p(lo, _ip), _p(hi, _ip)), True)
        out = np.empty(max(cloud.n, 1), np.int32)
        n = C.c_size_t(0)
        self._chk(lib().ope_color_filter(self.h, cloud.h, _p(lo, _ip), _p(hi, _ip), _p(out, _ip), C.byref(n)))
        return out[: n.value].copy()

    def voxel_grid(self, cloud: "Cloud", leaf, rgb=None):
        """pcl::VoxelGrid centroids (m,3) in ascending voxel index; OpeError(OPE_ERANGE) where PCL refuses the leaf.
        rgb (optional, n uint32 = the bits of PointXYZRGB::rgb, input order): also the voxels' colours -> (centroids, colours)."""
        lf = np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, np.float32), (3,)))
        out = np.empty((max(cloud.n, 1), 3), np.float32)
        n = C.c_size_t(0)
        if rgb is None:
            self._chk(lib().ope_voxel_grid(self.h, cloud.h, _p(lf, _fp), _p(out, _fp), C.byref(n)))
            return out[: n.value].copy()
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32)
        if rgb.shape != (cloud.n,):
            raise ValueError("rgb: one packed colour per input point")
        oc = np.zeros(max(cloud.n, 1), np.uint32)
        self._chk(lib().ope_voxel_grid_rgb(self.h, cloud.h, _p(lf, _fp), rgb.ctypes.data, _p(out, _fp), oc.ctypes.data, C.byref(n)))
        return out[: n.value].copy(), oc[: n.value].copy()

    def statistical_outlier_removal(self, cloud: "Cloud", mean_k: int = 30, stddev_mul: float = 1.0, return_distances: bool = False):
        """pcl::StatisticalOutlierRemoval (ProcessingPcd::getOutlierRemove): original indices of the inliers, ascending."""
        out = np.empty(max(cloud.n, 1), np.int32)
        dist = np.empty(max(cloud.n, 1), np.float32) if return_distances else None
        n = C.c_size_t(0)
        self._chk(lib().ope_statistical_outlier_removal(self.h, cloud.h, mean_k, stddev_mul, _p(out, _ip), C.byref(n), _p(dist, _fp)))
        return (out[: n.value].copy(), dist[: cloud.n].copy()) if return_distances else out[: n.value].copy()

    def mls_smooth(self, cloud: "Cloud", radius: float, order: int = 2, polynomial_fit: bool = True, compute_normals: bool = False,
                   sqr_gauss_param: float | None = None, as_cloud: bool = False):
        """pcl::MovingLeastSquares, upsampling NONE (ProcessingPcd::getSmooth).  as_cloud=False: (xyz, idx) or, with
        compute_normals, (xyz, idx, normals, curvature), idx the ORIGINAL index of each output point.  as_cloud=True: (Cloud, idx),
        the smoothed points left on the device with the input's colours and, with compute_normals, the normals attached."""
        p = default_mls_params(radius=float(radius), order=int(order), polynomial_fit=int(bool(polynomial_fit)),
                               compute_normals=int(bool(compute_normals)),
                               sqr_gauss_param=0.0 if sqr_gauss_param is None else float(sqr_gauss_param))
        cap = max(cloud.n, 1)
        idx = np.empty(cap, np.int32)
        n = C.c_size_t(0)
        if as_cloud:
            h = _vp()
            self._chk(lib().ope_mls_smooth_cloud(self.h, cloud.h, C.byref(p), C.byref(h), _p(idx, _ip), C.byref(n)))
            return Cloud(self, h, n.value), idx[: n.value].copy()
        xyz = np.empty((cap, 3), np.float32)
        nrm = np.empty((cap, 3), np.float32) if compute_normals else None
        curv = np.empty(cap, np.float32) if compute_normals else None
        self._chk(lib().ope_mls_smooth(self.h, cloud.h, C.byref(p), _p(xyz, _fp), _p(nrm, _fp), _p(curv, _fp), _p(idx, _ip), C.byref(n)))
        m = n.value
        if compute_normals:
            return xyz[:m].copy(), idx[:m].copy(), nrm[:m].copy(), curv[:m].copy()
        return xyz[:m].copy(), idx[:m].copy()

    def mls_upsample(self, cloud: "Cloud", radius: float, order: int = 2, voxel_size: float = 1.0, dilation_iterations: int = 0,
                     compute_normals: bool = False, as_cloud: bool = False, polynomial_fit: bool = True,
                     sqr_gauss_param: float | None = None):
        """pcl::MovingLeastSquares, upsampling VOXEL_GRID_DILATION (RegMeshPcd::generateMesh).  as_cloud=False: (xyz, idx, normals,
        curvature), idx the ORIGINAL index of the input point nearest to each output point, normals the plane's unless
        compute_normals.  as_cloud=True: (Cloud, idx), the new points left on the device with their nearest points' colours and, with
        compute_normals, the normals attached."""
        p = default_mls_upsample_params(radius=float(radius), order=int(order), polynomial_fit=int(bool(polynomial_fit)),
                                        compute_normals=int(bool(compute_normals)), voxel_size=float(voxel_size),
                                        dilation_iterations=int(dilation_iterations),
                                        sqr_gauss_param=0.0 if sqr_gauss_param is None else float(sqr_gauss_param))
        n = C.c_size_t(0)
        cap = max(8 * cloud.n, 1 << 16)   # a guess; the call says what it needs when that is too small
        for _ in range(2):
            idx = np.empty(cap, np.int32)
            if as_cloud:
                h = _vp()
                rc = lib().ope_mls_upsample_cloud(self.h, cloud.h, C.byref(p), C.byref(h), _p(idx, _ip), cap, C.byref(n))
            else:
                xyz = np.empty((cap, 3), np.float32)
                nrm = np.empty((cap, 3), np.float32)
                curv = np.empty(cap, np.float32)
                rc = lib().ope_mls_upsample(self.h, cloud.h, C.byref(p), _p(xyz, _fp), _p(nrm, _fp), _p(curv, _fp), _p(idx, _ip), cap, C.byref(n))
            if rc != OPE_EINVAL or n.value <= cap:
                break
            cap = n.value
        self._chk(rc)
        m = n.value
        if as_cloud:
            return Cloud(self, h, m), idx[:m].copy()
        return xyz[:m].copy(), idx[:m].copy(), nrm[:m].copy(), curv[:m].copy()

    def mls_upsample_stats(self) -> dict:
        """ope_mls_upsample_last_stats: what the last mls_upsample did (include/ope.h)."""
        return self._stats("ope_mls_upsample_last_stats", MlsUpsampleStats)

    def mls_stats(self) -> dict:
        """ope_mls_last_stats: n_in, n_out, n_plane_only, n_dropped, neighbours_total of the last mls_smooth."""
        return self._stats("ope_mls_last_stats", MlsStats)

    def sacia(self, src: "Cloud", src_feat, tgt: "Cloud", tgt_index: "Index", tgt_feat, params: SaciaParams | None = None,
              forced_samples=None):
        p = params or default_sacia_params()
        sf, tf = _f32(src_feat, 33), _f32(tgt_feat, 33)
        fs = np.ascontiguousarray(forced_samples, np.int32) if forced_samples is not None else None
        T = np.empty(16, np.float32)
        err = C.c_double(0); bi = C.c_int32(-1)
        self._chk(lib().ope_sacia(self.h, src.h, _p(sf, _fp), tgt.h, tgt_index.h, _p(tf, _fp), C.byref(p), _p(fs, _ip),
                                  _p(T, _fp), C.byref(err), C.byref(bi)))
        return from_colmajor(T), err.value, bi.value

    def prerejective(self, src: "Cloud", src_feat, tgt: "Cloud", tgt_index: "Index", tgt_feat,
                     params: PrerejectiveParams | None = None, forced_samples=None, with_inliers: bool = False) -> PrerejectiveOut:
        """ope_prerejective: pcl::SampleConsensusPrerejective::align of src onto tgt (include/ope.h).  forced_samples:
        (2, max_iterations, nr_samples) source then target indices, taken instead of the draws (the features may then be None)."""
        p = params or default_prerejective_params()
        sf = _f32(src_feat, 33) if src_feat is not None else None
        tf = _f32(tgt_feat, 33) if tgt_feat is not None else None
        fs = np.ascontiguousarray(forced_samples, np.int32) if forced_samples is not None else None
        if fs is not None and fs.size != 2 * max(p.max_iterations, 0) * max(p.nr_samples, 0):
            raise ValueError("forced_samples holds max_iterations * nr_samples source indices, then as many target indices")
        res = PrerejectiveResult()
        idx = np.empty(max(src.n, 1), np.int32) if with_inliers else None
        self._chk(lib().ope_prerejective(self.h, src.h, _p(sf, _fp), tgt.h, tgt_index.h, _p(tf, _fp), C.byref(p), _p(fs, _ip),
                                         C.byref(res), _p(idx, _ip)))
        return PrerejectiveOut(from_colmajor(np.array(res.T, np.float32)), res.error, res.best_iteration, res.inliers,
                               bool(res.converged), idx[:res.inliers].copy() if with_inliers else None)

    def prerejective_stats(self) -> dict:
        """ope_prerejective_last_stats: iterations, survivors, launches, host synchronisations, nr_samples of the last prerejective call."""
        return self._stats("ope_prerejective_last_stats", PrerejectiveStats)

    def prerejective_hypotheses(self) -> dict:
        """ope_prerejective_last_hypotheses, in drawing order: samples and targets (h, nr_samples) int32, survived (h,) bool,
        T (h, 4, 4) float32 math layout, inliers (h,) int32, error (h,) float64."""
        S = int(self.prerejective_stats()["nr_samples"])   # of the call these arrays belong to
        smp, tg, sv, T, inl, err = self._read("ope_prerejective_last_hypotheses", (), [
            (np.int32, (S,)), (np.int32, (S,)), (np.uint8, ()), (np.float32, (16,)), (np.int32, ()), (np.float64, ())])
        return dict(samples=smp, targets=tg, survived=sv.astype(bool), T=_T_stack(T), inliers=inl, error=err)

    def feature_correspondences(self, src_feat, tgt_feat):
        """ope_feature_correspondences: the 1-NN match of every source FPFH row among the target's rows.  (src_idx, tgt_idx, dist):
        int32, int32 and the float32 squared distance; rows without a finite distance are left out (len(src_feat) - len(src_idx))."""
        sf, tf = _f32(src_feat, 33), _f32(tgt_feat, 33)
        ns = len(sf)
        si, ti, d = np.empty(max(ns, 1), np.int32), np.empty(max(ns, 1), np.int32), np.empty(max(ns, 1), np.float32)
        n = C.c_size_t(0)
        self._chk(lib().ope_feature_correspondences(self.h, _p(sf, _fp), ns, _p(tf, _fp), len(tf), _p(si, _ip), _p(ti, _ip), _p(d, _fp), C.byref(n)))
        return si[:n.value].copy(), ti[:n.value].copy(), d[:n.value].copy()

    def corr_sac(self, src: "Cloud", tgt: "Cloud", src_idx, tgt_idx, params: CorrSacParams | None = None, forced_samples=None) -> CorrSacOut:
        """ope_corr_sac: pcl::registration::CorrespondenceRejectorSampleConsensus over the matches (src_idx[i], tgt_idx[i]) and
        TransformationEstimationSVD over those that remain (include/ope.h).  params None: the library's defaults.  forced_samples:
        (h, 3) match positions taken instead of the draws."""
        si, ti = np.ascontiguousarray(src_idx, np.int32).reshape(-1), np.ascontiguousarray(tgt_idx, np.int32).reshape(-1)
        if len(si) != len(ti):
            raise ValueError("src_idx and tgt_idx pair up")
        fs = np.ascontiguousarray(forced_samples, np.int32).reshape(-1, 3) if forced_samples is not None else None
        res = CorrSacResult()
        pos = np.empty(max(len(si), 1), np.int32)
        self._chk(lib().ope_corr_sac(self.h, src.h, tgt.h, _p(si, _ip), _p(ti, _ip), len(si), C.byref(params) if params is not None else None,
                                     _p(fs, _ip), len(fs) if fs is not None else 0, C.byref(res), _p(pos, _ip)))
        return CorrSacOut(from_colmajor(np.array(res.T_best, np.float32)), from_colmajor(np.array(res.T_svd, np.float32)), res.inliers, res.best,
                          res.iterations, bool(res.found), pos[:res.inliers].copy())

    def corr_sac_stats(self) -> dict:
        """ope_corr_sac_last_stats: hypotheses, iterations, launches, host_syncs, sample_dist_thresh of the last corr_sac call."""
        return self._stats("ope_corr_sac_last_stats", CorrSacStats)

    def corr_sac_hypotheses(self) -> dict:
        """ope_corr_sac_last_hypotheses, in drawing order: samples (h, 3) int32 match positions, T (h, 4, 4) float32 math layout,
        counts (h,) int32."""
        smp, T, cnt = self._read("ope_corr_sac_last_hypotheses", (), [(np.int32, (3,)), (np.float32, (16,)), (np.int32, ())])
        return dict(samples=smp, T=_T_stack(T), counts=cnt)

    def coarse_pose_correspondences(self, src: "Cloud", src_feat, tgt: "Cloud", tgt_feat, params: CorrSacParams | None = None) -> CorrSacOut:
        """The reference's third coarse aligner (BuildModel/src/poseestimator.cpp:43-60, :111-113) over key-point clouds and their
        FPFH rows: feature_correspondences, corr_sac, and the SVD over the remaining matches (out.T_svd is the coarse pose)."""
        si, ti, d = self.feature_correspondences(src_feat, tgt_feat)
        out = self.corr_sac(src, tgt, si, ti, params)
        out.matches = (si, ti, d)
        return out


def default_prerejective_params(**kw) -> PrerejectiveParams:
    """ope_prerejective_default_params (50000 / 3 / 5 / 0.8 / 0.15 / 0.25, seed 1: BuildModel poseestimator.cpp:97-102)."""
    return _params(PrerejectiveParams, "ope_prerejective_default_params", kw)


def default_corr_sac_params(**kw) -> CorrSacParams:
    """ope_corr_sac_default_params (0.05 / 1000 / 0.99, seed 12345: PCL's own defaults; the reference sets 10000 and 0.08)."""
    return _params(CorrSacParams, "ope_corr_sac_default_params", kw)


def default_sacia_params(**kw) -> SaciaParams:
    return _params(SaciaParams, "ope_sacia_default_params", kw)


def default_coarse_params(**kw) -> CoarseParams:
    """ope_coarse_default_params (the reference's values); keyword arguments set fields, `sacia` takes a SaciaParams."""
    return _params(CoarseParams, "ope_coarse_default_params", kw)


def default_cluster_params(**kw) -> ClusterParams:
    """ope_cluster_default_params (tolerance 0.05, min 300, max 100000: objectsegmentationplane.cpp:85-87)."""
    return _params(ClusterParams, "ope_cluster_default_params", kw)


def default_region_params(**kw) -> RegionParams:
    """ope_region_default_params (15 neighbours, normals k 30, smoothness 10 degrees, curvature 1.0, sizes 500 .. 1000000:
    segmentationregiongrow.cpp:25-36)."""
    return _params(RegionParams, "ope_region_default_params", kw)


def default_region_rgb_params(**kw) -> RegionRgbParams:
    """pcl::RegionGrowingRGB as SegmentationRegionGrow::getSegmentRegGrowRgb sets it (segmentationregiongrow.cpp:97-106)"""
    return _params(RegionRgbParams, "ope_region_rgb_default_params", kw)


def default_vfh_params(**kw) -> VfhParams:
    """ope_vfh_default_params (normals_k 30, viewpoint 0 0 0, no given centroid or normal); viewpoint / centroid / normal take
    3-sequences."""
    return _params(VfhParams, "ope_vfh_default_params", kw)


def default_plane_params(**kw) -> PlaneParams:
    """ope_plane_default_params (threshold 0.01, 50 iterations, probability 0.99, optimised coefficients, seed 12345)."""
    return _params(PlaneParams, "ope_plane_default_params", kw)


def default_track_params(**kw) -> TrackParams:
    """ope_track_default_params (gate 0.05, coarse stage above 1e-4, the final stages' defaults); keyword arguments set fields."""
    return _params(TrackParams, "ope_track_default_params", kw)


def default_final_params(**kw) -> FinalParams:
    """ope_final_default_params (the reference's values); keyword arguments set fields (`coarse` a CoarseParams, `icp` an
    IcpParams)."""
    return _params(FinalParams, "ope_final_default_params", kw)


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().ope_comm_get_unique_id(buf)
    if rc != OPE_OK:
        raise OpeError(rc, (lib().ope_last_error(None) or b"").decode())
    return buf.raw


class Cloud:
    def __init__(self, ctx: Context, h, n: int):
        self.ctx, self.h, self.n = ctx, h, n

    def set_normals(self, normals):
        nrm = _f32(normals, 3)
        if len(nrm) != self.n:
            raise ValueError("normals length mismatch")
        self.ctx._chk(lib().ope_cloud_set_normals(self.ctx.h, self.h, _p(nrm, _fp)))

    def download_normals(self):
        """ope_cloud_download_normals: (normals (n, 3), curvature (n,)) in original order (OpeError when the cloud carries none)."""
        nrm = np.empty((self.n, 3), np.float32)
        curv = np.empty(self.n, np.float32)
        self.ctx._chk(lib().ope_cloud_download_normals(self.ctx.h, self.h, _p(nrm, _fp), _p(curv, _fp)))
        return nrm, curv

    def set_rgb(self, rgb):
        """ope_cloud_set_rgb: n uint32 words r << 16 | g << 8 | b in the cloud's original order; None detaches the colours."""
        if rgb is None:
            self.ctx._chk(lib().ope_cloud_set_rgb(self.ctx.h, self.h, None))
            return
        rgb = np.ascontiguousarray(rgb, np.uint32).reshape(-1)
        if len(rgb) != self.n:
            raise ValueError("rgb length mismatch")
        self.ctx._chk(lib().ope_cloud_set_rgb(self.ctx.h, self.h, _vp(rgb.ctypes.data)))

    @property
    def has_rgb(self) -> bool:
        return bool(lib().ope_cloud_has_rgb(self.h))

    def download_rgb(self) -> np.ndarray:
        """ope_cloud_download_rgb: the colour words in original order (OpeError when the cloud has none)."""
        out = np.empty(self.n, np.uint32)
        self.ctx._chk(lib().ope_cloud_download_rgb(self.ctx.h, self.h, _vp(out.ctypes.data)))
        return out

    def free(self):
        if self.h:
            lib().ope_cloud_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


class VfhDb:
    """A device-resident table of VFH signatures (ope_vfh_db)."""

    def __init__(self, ctx: Context, h, m: int):
        self.ctx, self.h, self.m = ctx, h, m

    def free(self):
        if getattr(self, "h", None):
            lib().ope_vfh_db_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Index:
    def __init__(self, ctx: Context, h, cloud: Cloud):
        self.ctx, self.h, self.cloud = ctx, h, cloud

    def free(self):
        if self.h:
            lib().ope_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass
