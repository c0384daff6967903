"""ctypes loader for libsycl_points_amd.so (the C ABI declared in include/sycl_points_amd.h).

The product path has no CPU fallback: if the library is missing this module raises, loudly.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# SP_AMD_LIB: another build of the same library (A/B measurements on one box, scratch/ab.sh); the tests and bench.py never set it
LIB_PATH = os.environ.get("SP_AMD_LIB") or os.path.join(_HERE, "lib", "libsycl_points_amd.so")
CSRC = os.path.join(_HERE, "csrc")

SP_OK, SP_ERR_INVALID_ARGUMENT, SP_ERR_RUNTIME, SP_ERR_HIP = 0, 1, 2, 3
COMM_ID_BYTES = 128  # SP_COMM_ID_BYTES


class SpError(RuntimeError):
    """Mirrors the C++ exceptions of the reference: code 1 -> std::invalid_argument, 2 -> std::runtime_error,
    3 -> device error (sycl::exception from wait_and_throw)."""

    def __init__(self, code, msg):
        super().__init__(f"[sycl_points_amd] error {code}: {msg}")
        self.code = code


class Linearized(C.Structure):  # sp_linearized
    _fields_ = [("H", C.c_float * 36), ("b", C.c_float * 6), ("error", C.c_float), ("inlier", C.c_uint32),
                ("inlier_lo", C.c_float), ("inlier_hi", C.c_float), ("pad", C.c_float * 2)]


class FactorParams(C.Structure):  # sp_factor_params
    _fields_ = [("reg_type", C.c_int), ("robust_type", C.c_int), ("max_correspondence_distance", C.c_float),
                ("robust_scale", C.c_float), ("genz_alpha", C.c_float), ("genz_planarity_threshold", C.c_float),
                ("rotation_constraint_enable", C.c_int), ("rotation_constraint_weight", C.c_float),
                ("rotation_robust_scale", C.c_float)]


class PhotometricParams(C.Structure):  # sp_photometric_params
    _fields_ = [("weight", C.c_float), ("robust_type", C.c_int), ("robust_scale", C.c_float),
                ("max_correspondence_distance", C.c_float)]


class DegenerateRegParams(C.Structure):  # sp_degenerate_reg_params
    _fields_ = [("type", C.c_int), ("rot_eigenvalue_threshold", C.c_float), ("trans_eigenvalue_threshold", C.c_float),
                ("base_factor", C.c_float)]


class MapPriorParams(C.Structure):  # sp_map_prior_params
    _fields_ = [("enabled", C.c_int), ("rot_vel_sigma", C.c_float), ("trans_vel_sigma", C.c_float),
                ("rot_base_sigma", C.c_float), ("trans_base_sigma", C.c_float)]


class MapPriorState(C.Structure):  # sp_map_prior_state
    _fields_ = [("has_prior", C.c_int), ("omega", C.c_float * 36), ("T_pred_inv", C.c_float * 16)]


class GnParams(C.Structure):  # sp_gn_params
    _fields_ = [("lambda_", C.c_float), ("crit_rotation", C.c_float), ("crit_translation", C.c_float)]


class OptParams(C.Structure):  # sp_opt_params
    _fields_ = [("method", C.c_int), ("max_iterations", C.c_int), ("crit_rotation", C.c_float), ("crit_translation", C.c_float),
                ("gn_lambda", C.c_float), ("lm_max_inner_iterations", C.c_int), ("lm_lambda_factor", C.c_float),
                ("lm_init_lambda", C.c_float), ("lm_max_lambda", C.c_float), ("lm_min_lambda", C.c_float),
                ("dl_initial_radius", C.c_float), ("dl_min_radius", C.c_float), ("dl_max_radius", C.c_float),
                ("dl_eta1", C.c_float), ("dl_eta2", C.c_float), ("dl_gamma_decrease", C.c_float),
                ("dl_gamma_increase", C.c_float)]


class OptLogEntry(C.Structure):  # sp_opt_log_entry
    _fields_ = [("level", C.c_uint16), ("iteration", C.c_uint16), ("trials", C.c_uint16), ("accepted", C.c_uint16),
                ("damping", C.c_float), ("error", C.c_float)]


class ScanContextParams(C.Structure):  # sp_scan_context_params
    _fields_ = [("rings", C.c_uint32), ("sectors", C.c_uint32), ("max_range", C.c_float), ("sensor_height", C.c_float)]


OPT_MAX_LEVELS, OPT_LOG_ENTRIES = 8, 64


class AlignResult(C.Structure):  # sp_align_result
    _fields_ = [("T", C.c_float * 16), ("T_lin", C.c_float * 16), ("H", C.c_float * 36), ("b", C.c_float * 6),
                ("error", C.c_float), ("error_raw", C.c_float), ("inlier", C.c_uint32), ("iterations", C.c_uint32),
                ("converged", C.c_uint32), ("status", C.c_uint32), ("linearizations", C.c_uint32), ("trials", C.c_uint32),
                ("searched", C.c_uint32), ("damping", C.c_float), ("log_entries", C.c_uint32), ("pad", C.c_uint32 * 3),
                ("log", OptLogEntry * OPT_LOG_ENTRIES)]


class OptRequest(C.Structure):  # sp_opt_request
    _fields_ = [("want", C.c_int), ("level", C.c_int), ("iteration", C.c_int), ("robust_scale", C.c_float), ("T", C.c_float * 16),
                ("T_lin", C.c_float * 16), ("damping", C.c_float)]


class ImuParams(C.Structure):  # sp_imu_params
    _fields_ = [("gravity", C.c_float * 3), ("accel_scale", C.c_float), ("gyro_noise_density", C.c_float),
                ("accel_noise_density", C.c_float), ("gyro_bias_rw_density", C.c_float), ("accel_bias_rw_density", C.c_float)]


class ImuState(C.Structure):  # sp_imu_state
    _fields_ = [("Delta_R", C.c_float * 9), ("Delta_v", C.c_float * 3), ("Delta_p", C.c_float * 3), ("pad0", C.c_float),
                ("dt_total", C.c_double), ("J_R_bg", C.c_float * 9), ("J_v_bg", C.c_float * 9), ("J_v_ba", C.c_float * 9),
                ("J_p_bg", C.c_float * 9), ("J_p_ba", C.c_float * 9), ("covariance", C.c_float * 225)]


class MotionAxisParams(C.Structure):  # sp_motion_axis_params
    _fields_ = [("factor_min", C.c_float), ("factor_max", C.c_float), ("min_eigenvalue_low", C.c_float),
                ("min_eigenvalue_high", C.c_float)]


class MotionPredictParams(C.Structure):  # sp_motion_predict_params
    _fields_ = [("rotation", MotionAxisParams), ("translation", MotionAxisParams), ("velocity_ema_alpha", C.c_float), ("mode", C.c_int)]


class MotionPredictState(C.Structure):  # sp_motion_predict_state
    _fields_ = [("has_linear", C.c_int), ("has_angular", C.c_int), ("linear", C.c_float * 3), ("angular", C.c_float * 3)]


class InitialAlignmentParams(C.Structure):  # sp_initial_alignment_params
    _fields_ = [("required_duration_sec", C.c_float), ("max_gyro_std", C.c_float), ("max_accel_std", C.c_float),
                ("max_accel_norm_error", C.c_float), ("estimate_gyro_bias", C.c_int)]


class InitialAlignmentResult(C.Structure):  # sp_initial_alignment_result
    _fields_ = [("success", C.c_int), ("window_size", C.c_int), ("R_world_imu", C.c_float * 9), ("gyro_bias", C.c_float * 3),
                ("accel_mean", C.c_float * 3), ("gyro_std", C.c_float * 3), ("accel_std", C.c_float * 3), ("accel_norm", C.c_float),
                ("roll_rad", C.c_float), ("pitch_rad", C.c_float), ("error_message", C.c_char * 96)]


class LioLinearized(C.Structure):  # sp_lio_linearized
    _fields_ = [("H", C.c_float * 225), ("b", C.c_float * 15), ("error_icp", C.c_float), ("error_imu", C.c_float),
                ("inlier", C.c_uint32), ("pad", C.c_uint32)]


class LioDirectionalParams(C.Structure):  # sp_lio_directional_params
    _fields_ = [("enable", C.c_int), ("trans_min_eigenvalue_per_inlier", C.c_float), ("rot_min_eigenvalue_per_inlier", C.c_float),
                ("trans_weak_direction_scale", C.c_float), ("rot_weak_direction_scale", C.c_float)]


class LioParams(C.Structure):  # sp_lio_params
    _fields_ = [("opt", OptParams), ("robust_auto_scale", C.c_int), ("robust_init_scale", C.c_float), ("robust_min_scale", C.c_float),
                ("rotation_robust_init_scale", C.c_float), ("rotation_robust_min_scale", C.c_float),
                ("robust_auto_scaling_iter", C.c_int), ("invalid_regularization_factor", C.c_float),
                ("directional", LioDirectionalParams)]


class LioFactorFacts(C.Structure):  # sp_lio_factor_facts
    _fields_ = [("residual_dim", C.c_int), ("robust_is_none", C.c_int), ("robust_default_scale", C.c_float),
                ("rotation_robust_default_scale", C.c_float)]


class LioRequest(C.Structure):  # sp_lio_request
    _fields_ = [("want", C.c_int), ("level", C.c_int), ("iteration", C.c_int), ("robust_scale", C.c_float),
                ("rotation_robust_scale", C.c_float), ("state", C.c_float * 21), ("T", C.c_float * 16), ("T_lin", C.c_float * 16),
                ("damping", C.c_float), ("icp_weight", C.c_float)]


class LioResult(C.Structure):  # sp_lio_result
    _fields_ = [("state", C.c_float * 21), ("posterior_covariance", C.c_float * 225), ("iterations", C.c_uint32),
                ("inlier", C.c_uint32), ("error", C.c_float), ("converged", C.c_uint32)]


class Pc2Layout(C.Structure):  # sp_pc2_layout
    _fields_ = [("point_step", C.c_uint32), ("x_offset", C.c_int32), ("y_offset", C.c_int32), ("z_offset", C.c_int32),
                ("rgb_offset", C.c_int32), ("intensity_offset", C.c_int32), ("timestamp_offset", C.c_int32), ("xyz_type", C.c_uint8),
                ("rgb_type", C.c_uint8), ("intensity_type", C.c_uint8), ("timestamp_type", C.c_uint8), ("start_time_ms", C.c_double)]


# sensor_msgs/PointField datatypes (SP_PC2_*)
PC2_TYPE = {"INT8": 1, "UINT8": 2, "INT16": 3, "UINT16": 4, "INT32": 5, "UINT32": 6, "FLOAT32": 7, "FLOAT64": 8}
PC2_BLOCK_POINTS, PC2_MAX_POINT_STEP, ER_MAX_RINGS = 256, 240, 256  # SP_PC2_BLOCK_POINTS, SP_PC2_MAX_POINT_STEP, SP_ER_MAX_RINGS
ER_STATE_BYTES = 3 * 4 * ER_MAX_RINGS  # SP_ER_STATE_BYTES
MOTION_MODE = {"LIDAR_CV": 0, "GYRO_LIDAR_CV": 1, "IMU_SE3": 2}  # SP_MOTION_*
# deskew::IMUDeskewStatus (SP_IMU_DESKEW_*)
IMU_DESKEW_STATUS = ("success", "insufficient_imu_coverage", "no_timestamps", "invalid_scan_duration", "empty_cloud")
OPT_WANT_DONE, OPT_WANT_LINEARIZE, OPT_WANT_TRIAL = 0, 1, 2
assert C.sizeof(Linearized) == 192 and C.sizeof(Pc2Layout) == 40
assert C.sizeof(ImuParams) == 32 and C.sizeof(ImuState) == 1152
assert C.sizeof(MotionPredictParams) == 40 and C.sizeof(MotionPredictState) == 32 and C.sizeof(InitialAlignmentResult) == 200
assert C.sizeof(LioLinearized) == 976 and C.sizeof(LioParams) == 68 + 7 * 4 + 20 and C.sizeof(LioRequest) == 4 * 60
assert C.sizeof(LioResult) == 4 * 250 and C.sizeof(LioFactorFacts) == 16
assert C.sizeof(ScanContextParams) == 16 and C.sizeof(PhotometricParams) == 16
assert C.sizeof(OptParams) == 68 and C.sizeof(OptLogEntry) == 16 and C.sizeof(AlignResult) == 4 * (74 + 14) + 16 * 64

_vp, _sz, _f, _i = C.c_void_p, C.c_size_t, C.c_float, C.c_int

# name -> (restype, argtypes); every symbol include/sycl_points_amd.h declares
SIGNATURES = {
    "sp_abi_version": (_i, []),
    "sp_stream_retired": (None, [_vp]),
    "sp_last_error": (C.c_char_p, []),
    "sp_device_count": (_i, []),
    "sp_set_device": (_i, [_i]),
    "sp_knn_bruteforce_workspace_bytes": (_sz, [_sz, _sz, _sz]),
    "sp_knn_bruteforce_set_pass_a": (_i, [_i]),
    "sp_knn_bruteforce": (_i, [_vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp]),
    "sp_kdtree_create": (_i, [_vp, _sz, _sz, _vp, C.POINTER(_vp)]),
    "sp_kdtree_destroy": (None, [_vp]),
    "sp_kdtree_size": (_sz, [_vp]),
    "sp_kdtree_search": (_i, [_vp, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp]),
    "sp_kdtree_radius_search": (_i, [_vp, _vp, _sz, _sz, _f, _vp, _i, _vp, _vp, _vp]),
    "sp_kdtree_remove_by_flags": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "sp_grid_create": (_i, [_vp, _sz, _f, _f, _vp, C.POINTER(_vp)]),
    "sp_grid_create_adaptive": (_i, [_vp, _sz, _f, _vp, C.POINTER(_vp)]),
    "sp_grid_create_bounded": (_i, [_vp, _sz, _vp, _f, _f, _vp, _vp]),
    "sp_grid_destroy": (None, [_vp]),
    "sp_grid_size": (_sz, [_vp]),
    "sp_grid_order": (_i, [_vp, _vp, _vp]),
    "sp_grid_cell_size": (_f, [_vp]),
    "sp_grid_max_cell_points": (C.c_uint32, [_vp]),
    "sp_grid_search": (_i, [_vp, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp]),
    "sp_grid_radius_search": (_i, [_vp, _vp, _sz, _sz, _f, _vp, _i, _vp, _vp, _vp]),
    "sp_grid_remove_by_flags": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "sp_grid_self_workspace_bytes": (_sz, [_vp]),
    "sp_grid_self_knn": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_grid_self_knn_range": (_i, [_vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_grid_gather_rows": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    "sp_grid_scatter_rows": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    "sp_cov_estimate": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "sp_cov_estimate_robust": (_i, [_vp, _sz, _vp, _sz, _i, _f, _f, _sz, _vp, _vp]),
    "sp_cov_normalize": (_i, [_vp, _sz, _vp, _vp]),
    "sp_normals_from_knn": (_i, [_vp, _sz, _vp, _sz, _vp, _vp]),
    "sp_normals_from_cov": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "sp_cov_update_plane": (_i, [_vp, _sz, _vp, _vp]),
    "sp_bvh_create": (_i, [_vp, _sz, _vp, C.POINTER(_vp)]),
    "sp_bvh_destroy": (None, [_vp]),
    "sp_bvh_size": (_sz, [_vp]),
    "sp_bvh_search": (_i, [_vp, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp]),
    "sp_bvh_self_knn": (_i, [_vp, _sz, _vp, _vp, _vp]),
    "sp_bvh_radius_search": (_i, [_vp, _vp, _sz, _sz, _f, _vp, _i, _vp, _vp, _vp]),
    "sp_bvh_remove_by_flags": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "sp_bvh_export_points": (_i, [_vp, _vp, _vp]),
    "sp_octree_create": (_i, [_vp, _sz, _f, _sz, _vp, C.POINTER(_vp)]),
    "sp_octree_destroy": (None, [_vp]),
    "sp_octree_size": (_sz, [_vp]),
    "sp_octree_info": (_i, [_vp, _i, C.POINTER(C.c_uint64)]),
    "sp_octree_search": (_i, [_vp, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp]),
    "sp_octree_remove_by_flags": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "sp_octree_export": (_i, [_vp, _vp, _vp, _vp]),
    "sp_knn_tree_create": (_i, [_vp, _sz, _sz, _vp, C.POINTER(_vp)]),
    "sp_knn_tree_destroy": (None, [_vp]),
    "sp_knn_tree_backend": (_i, [_vp, _sz, _sz, _vp, _i, _i, _vp, C.POINTER(_i)]),
    "sp_knn_tree_search": (_i, [_vp, _vp, _sz, _sz, _vp, _i, _i, _vp, _vp, _vp]),
    "sp_knn_tree_radius_search": (_i, [_vp, _vp, _sz, _sz, _f, _vp, _i, _vp, _vp, _vp]),
    "sp_knn_tree_remove_by_flags": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "sp_knn_tree_set_reference_order": (_i, [_vp, _i]),
    "sp_knn_tree_info": (_i, [_vp, _i, C.POINTER(C.c_uint64)]),
    "sp_voxel_keys": (_i, [_vp, _sz, _f, _vp, _vp]),
    "sp_voxel_downsample_workspace_bytes": (_sz, [_sz]),
    "sp_voxel_downsample": (_i, [_vp, _sz, _f, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_voxel_key_box": (_i, [_vp, _sz, _f, _vp, _vp]),
    "sp_voxel_downsample_boxed": (_i, [_vp, _sz, _f, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_voxel_downsample_report": (_i, [_vp, _sz, _f, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_polar_keys": (_i, [_vp, _sz, _i, _f, _f, _f, _vp, _vp]),
    "sp_polar_keys_host": (_i, [_vp, _sz, _i, _f, _f, _f, _vp]),
    "sp_polar_key_box": (_i, [_vp, _sz, _i, _f, _f, _f, _vp, _vp]),
    "sp_polar_downsample_report": (_i, [_vp, _sz, _i, _f, _f, _f, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _sz, _vp]),
    "sp_transform": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "sp_deskew_constant_velocity": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _f, _vp, _vp, _vp, _vp]),
    "sp_angle_incidence_flags": (_i, [_vp, _vp, _vp, _sz, _f, _f, _vp, _vp]),
    "sp_intensity_correct": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _f, _vp]),
    "sp_intensity_gaussian": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _f, _f, _f, _f, _vp, _vp]),
    "sp_intensity_zscore": (_i, [_vp, _vp, _sz, _sz, _sz, _f, _vp, _vp]),
    "sp_outlier_workspace_bytes": (_sz, [_sz]),
    "sp_outlier_statistical_flags": (_i, [_vp, _sz, _sz, _sz, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_outlier_radius_flags": (_i, [_vp, _sz, _sz, _sz, _f, _vp, _vp]),
    "sp_relative_twist_host": (None, [_vp, _vp, _vp]),
    "sp_imu_preint_create": (_i, [C.POINTER(ImuParams), C.POINTER(_vp)]),
    "sp_imu_preint_destroy": (None, [_vp]),
    "sp_imu_preint_reset": (_i, [_vp, _vp, _vp, _vp]),
    "sp_imu_preint_integrate": (_i, [_vp, C.c_double, _vp, _vp]),
    "sp_imu_preint_num_measurements": (_i, [_vp]),
    "sp_imu_preint_get": (_i, [_vp, _vp, C.POINTER(ImuState)]),
    "sp_imu_preint_predict_relative": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "sp_imu_preint_predict_transform": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "sp_imu_deskew_trajectory_host": (_i, [_vp, _vp, _sz, C.c_double, C.c_double, _vp, _vp, C.POINTER(ImuParams), _vp, _vp, _i, _vp,
                                           _sz, C.POINTER(_sz), C.POINTER(_i)]),
    "sp_imu_deskew_intervals_host": (_i, [_vp, _sz, _vp]),
    "sp_deskew_imu": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "sp_box_filter_flags": (_i, [_vp, _sz, _f, _f, _vp, _vp]),
    "sp_compact_workspace_bytes": (_sz, [_sz]),
    "sp_compact_by_flags": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_compact_by_flags_multi": (_i, [_vp, _vp, _vp, _i, _sz, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gather_rows_multi": (_i, [_vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "sp_fps_workspace_bytes": (_sz, [_sz, _sz]),
    "sp_farthest_point_sampling": (_i, [_vp, _sz, _sz, C.c_uint32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_fps_status": (_i, [_vp, _vp]),
    "sp_weight_check": (_i, [_vp, _sz, _vp, _vp]),
    "sp_weighted_sample_workspace_bytes": (_sz, [_sz]),
    "sp_weighted_sample_flags": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp]),
    "sp_uniform_fill_workspace_bytes": (_sz, [_sz]),
    "sp_uniform_fill_flags": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "sp_box_filter_compact_multi": (_i, [_vp, _sz, _f, _f, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_workspace_bytes": (_sz, [_sz]),
    "sp_gicp_linearize": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FactorParams), _vp, _vp, _sz, _vp]),
    "sp_gicp_error": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FactorParams), _vp, _vp, _sz, _vp]),
    "sp_icp_robust_weights": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FactorParams), _vp, _vp]),
    "sp_genz_counts": (_i, [_vp, _vp, _vp, _sz, _f, _f, _vp, _vp]),
    "sp_gicp_target_create": (_i, [_vp, _vp, _sz, _vp, C.POINTER(_vp)]),
    "sp_gicp_target_create_plain": (_i, [_vp, _vp, _sz, _vp, C.POINTER(_vp)]),
    "sp_gicp_target_certify": (_i, [_vp, _vp, _vp]),
    "sp_gicp_target_has_certificates": (_i, [_vp]),
    "sp_gicp_target_update": (_i, [_vp, _vp, _vp]),
    "sp_gicp_target_prepare": (_i, [_vp, _vp, _i, _vp]),
    "sp_gicp_error_prepared": (_i, [_vp, _vp, _vp, _vp, _i, C.POINTER(FactorParams), _vp, _vp, _sz, _vp]),
    "sp_gicp_target_destroy": (None, [_vp]),
    "sp_gicp_source_create": (_i, [_sz, C.POINTER(_vp)]),
    "sp_gicp_source_prepare": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _i, _i, _vp]),
    "sp_gicp_source_destroy": (None, [_vp]),
    "sp_gicp_iteration_fused": (_i, [_vp, _vp, _vp, _i, C.POINTER(FactorParams), _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_align_optimize": (_i, [_vp, _vp, _vp, C.POINTER(FactorParams), C.POINTER(OptParams), C.POINTER(C.c_float), _i, _vp, _vp,
                                    _sz, _vp]),
    "sp_gicp_source_set_persistent": (_i, [_vp, _i]),
    "sp_gicp_source_set_wave_per_point": (_i, [_vp, _i]),
    "sp_gicp_align_batch_workspace_bytes": (_sz, [_sz, _sz]),
    "sp_gicp_align_batch": (_i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(FactorParams), C.POINTER(OptParams), C.POINTER(C.c_float), _i, _vp,
                                 _vp, _sz, _vp]),
    "sp_align_best_host": (_i, [_vp, _sz, C.POINTER(_sz)]),
    "sp_opt_stepper_create": (_i, [C.POINTER(OptParams), _vp, C.POINTER(C.c_float), _i, C.POINTER(_vp)]),
    "sp_opt_stepper_destroy": (None, [_vp]),
    "sp_opt_stepper_next": (_i, [_vp, C.POINTER(OptRequest)]),
    "sp_opt_stepper_linearized": (_i, [_vp, C.POINTER(Linearized)]),
    "sp_opt_stepper_trial": (_i, [_vp, _f, C.c_uint32, C.POINTER(C.c_float)]),
    "sp_opt_stepper_result": (_i, [_vp, C.POINTER(AlignResult)]),
    "sp_gicp_align_fused": (_i, [_vp, _vp, _vp, C.POINTER(FactorParams), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_align_step": (_i, [_vp, _vp, _vp, C.POINTER(FactorParams), _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_align_linearization_pose": (_i, [_vp, _i, _vp, _vp]),
    "sp_xchg_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "sp_xchg_handle": (_i, [_vp, _vp]),
    "sp_xchg_connect": (_i, [_vp, _vp]),
    "sp_xchg_set_timeout_ms": (_i, [_vp, C.c_uint]),
    "sp_xchg_rank": (_i, [_vp]),
    "sp_xchg_world": (_i, [_vp]),
    "sp_xchg_destroy": (None, [_vp]),
    "sp_gicp_align_direct": (_i, [_vp, _vp, _vp, C.POINTER(FactorParams), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_align_status": (_i, [_vp, _i, _vp]),
    "sp_gicp_align_rows": (_vp, [_vp, _i, _vp]),
    "sp_gicp_align_row": (_vp, [_vp, _i, _vp]),
    "sp_comm_unique_id": (_i, [_vp]),
    "sp_comm_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "sp_comm_destroy": (None, [_vp]),
    "sp_comm_rank": (_i, [_vp]),
    "sp_comm_world": (_i, [_vp]),
    "sp_allreduce_rows": (_i, [_vp, _vp, _i, _vp]),
    "sp_allreduce_f32": (_i, [_vp, _vp, _sz, _vp]),
    "sp_allgather": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_align_sharded": (_i, [_vp, _vp, _vp, C.POINTER(FactorParams), _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gicp_align_finish": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_gn_update": (_i, [_vp, _vp, _f, _f, _f, _vp, _vp]),
    "sp_gn_update_host": (_i, [_vp, _vp, _f, _f, _f, _vp]),
    "sp_se3_exp_host": (None, [_vp, _vp]),
    "sp_rigid_mul_host": (None, [_vp, _vp, _vp]),
    "sp_ldlt6_solve_host": (_i, [_vp, _vp, _vp]),
    "sp_dogleg_step_host": (None, [_vp, _vp, _f, _vp, _vp, _vp]),
    "sp_se3_log_host": (None, [_vp, _vp]),
    "sp_degenerate_regularize_host": (_i, [_vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    "sp_map_prior_update_host": (_i, [_vp, _vp, _f, C.c_uint32, _vp, _vp, _vp]),
    "sp_map_prior_apply_host": (_f, [_vp, _vp, _vp, _vp, _vp]),
    "sp_motion_predict_host": (_i, [C.POINTER(MotionPredictParams), C.POINTER(MotionPredictState), _vp, _vp, _vp, _f, _vp, C.c_uint32, _i,
                                    _vp, _vp, _vp, _vp]),
    "sp_velocity_from_poses_host": (_i, [_vp, _vp, _f, _vp, _vp]),
    "sp_keyframe_decision_host": (_i, [_vp, _vp, C.c_double, C.c_double, _f, _f, _f, C.POINTER(_i), _vp]),
    "sp_initial_alignment_host": (_i, [_vp, _vp, _sz, _vp, C.POINTER(InitialAlignmentParams), _vp, _i, C.POINTER(InitialAlignmentResult)]),
    "sp_yaw_from_rotation_host": (_f, [_vp]),
    "sp_imu_manifold_residual_host": (_i, [_vp, _vp, _vp]),
    "sp_imu_hessian_gradient_host": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "sp_imu_gradient_host": (_i, [_vp, _vp, _vp, _vp]),
    "sp_lio_add_icp_factor_host": (_i, [C.POINTER(LioLinearized), C.POINTER(Linearized), _vp, _f]),
    "sp_lio_directional_weighting_host": (_i, [C.POINTER(LioLinearized), C.POINTER(LioDirectionalParams)]),
    "sp_lio_solve_ldlt_host": (_i, [_vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "sp_lio_retract_host": (_i, [_vp, _vp, _vp]),
    "sp_lio_imu_to_lidar_jacobian_host": (_i, [_vp, _vp, _vp]),
    "sp_lio_transform_covariance_host": (_i, [_vp, _vp, _vp, _i, _vp]),
    "sp_dogleg_step_n_host": (_i, [_i, _vp, _vp, _f, _vp, C.POINTER(_f), C.POINTER(_f)]),
    "sp_lio_stepper_create": (_i, [C.POINTER(LioParams), C.POINTER(LioFactorFacts), _vp, _vp, _vp, _i, C.POINTER(_vp)]),
    "sp_lio_stepper_destroy": (None, [_vp]),
    "sp_lio_stepper_next": (_i, [_vp, C.POINTER(LioRequest)]),
    "sp_lio_stepper_linearized": (_i, [_vp, C.POINTER(Linearized)]),
    "sp_lio_stepper_trial": (_i, [_vp, _f, C.c_uint32]),
    "sp_lio_stepper_result": (_i, [_vp, C.POINTER(LioResult)]),
    "sp_lio_bias_observable_host": (_i, [_vp, _vp, _sz, _i, _f, _f, C.POINTER(_i)]),
    "sp_lio_clamp_bias_host": (_i, [_vp, _f]),
    "sp_lio_predict_state_host": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _vp]),
    "sp_lio_reset_covariance_host": (_i, [_vp, _f, _f, _vp, _vp, _vp, _vp]),
    "sp_vhm_create": (_i, [_f, _vp, C.POINTER(_vp)]),
    "sp_vhm_destroy": (None, [_vp]),
    "sp_vhm_set": (_i, [_vp, _i, _f]),
    "sp_vhm_get": (_f, [_vp, _i]),
    "sp_vhm_info": (_sz, [_vp, _i]),
    "sp_vhm_clear": (_i, [_vp, _vp]),
    "sp_vhm_add_point_cloud": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "sp_vhm_downsampling": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "sp_vhm_overlap_ratio": (_i, [_vp, _vp, _sz, _vp, C.POINTER(_f), _vp]),
    "sp_vhm_remove_old_data": (_i, [_vp, _vp]),
    "sp_vhm_prepare_registration": (_i, [_vp, _i, _vp]),
    "sp_vhm_registration_ready": (_i, [_vp, _i]),
    "sp_vhm_registration_workspace_bytes": (_sz, [_sz]),
    "sp_vhm_prepare_source": (_i, [_vp, _sz, _i, _vp, _sz, _vp]),
    "sp_vhm_neighbor_offsets_host": (_i, [_i, _vp]),
    "sp_vhm_linearize": (_i, [_vp, _vp, _sz, _vp, _i, C.POINTER(FactorParams), _i, _vp, _vp, _vp, _sz, _vp]),
    "sp_vhm_error": (_i, [_vp, _vp, _sz, _vp, _i, C.POINTER(FactorParams), _vp, _vp, _sz, _vp]),
    "sp_vhm_align_batch_workspace_bytes": (_sz, [_sz, _sz]),
    "sp_vhm_align_batch": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, C.POINTER(FactorParams), C.POINTER(OptParams), C.POINTER(C.c_float),
                                _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "sp_ogm_create": (_i, [_f, _vp, C.POINTER(_vp)]),
    "sp_ogm_destroy": (None, [_vp]),
    "sp_ogm_set": (_i, [_vp, _i, _f]),
    "sp_ogm_set_log_odds_limits": (_i, [_vp, _f, _f]),
    "sp_ogm_get": (_f, [_vp, _i]),
    "sp_ogm_info": (_sz, [_vp, _i]),
    "sp_ogm_clear": (_i, [_vp, _vp]),
    "sp_ogm_add_point_cloud": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "sp_ogm_extract_occupied_points": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "sp_ogm_extract_visible_points": (_i, [_vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "sp_ogm_overlap_ratio": (_i, [_vp, _vp, _sz, _vp, C.POINTER(_f), _vp]),
    "sp_ogm_voxel_probability": (_i, [_vp, _vp, C.POINTER(_f), _vp]),
    "sp_ogm_export": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "sp_pc2_resolve_fields_host": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), _sz, C.c_uint32, _i, _i, _i,
                                        C.POINTER(Pc2Layout)]),
    "sp_pc2_unpack_workspace_bytes": (_sz, [_sz]),
    "sp_pc2_unpack": (_i, [_vp, _sz, _sz, C.POINTER(Pc2Layout), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sp_pc2_pack_point_step": (C.c_uint32, [_i, _i, _i]),
    "sp_pc2_pack": (_i, [_vp, _vp, _vp, _vp, _sz, C.c_double, _vp, _vp]),
    "sp_enhanced_reflectivity_workspace_bytes": (_sz, [_sz]),
    "sp_enhanced_reflectivity": (_i, [_vp, _vp, _sz, _vp, C.c_uint32, C.c_int32, _i, C.c_int32, _vp, _f, _f, _vp, _vp]),
    "sp_fpfh_workspace_bytes": (_sz, [_sz]),
    "sp_fpfh_compute": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_feature_match_workspace_bytes": (_sz, [_sz, _sz]),
    "sp_feature_match": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "sp_feature_match_mutual_workspace_bytes": (_sz, [_sz, _sz]),
    "sp_feature_match_mutual": (_i, [_vp, _sz, _vp, _sz, _vp, C.POINTER(C.c_uint32), _vp, _sz, _vp]),
    "sp_correspondence_points": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "sp_ransac_score": (_i, [_vp, _vp, _sz, _sz, C.c_uint64, _f, _f, _f, _vp, _vp]),
    "sp_ransac_triplets_host": (_i, [C.c_uint64, _sz, _sz, _sz, _vp]),
    "sp_ransac_select_host": (_i, [_vp, _sz, _vp, _vp, _sz, C.c_uint64, _sz, _vp, _vp, C.POINTER(_sz)]),
    "sp_scan_context_boundaries_host": (_i, [C.c_uint32, _vp, _vp]),
    "sp_scan_context_compute": (_i, [C.POINTER(ScanContextParams), _vp, _sz, _vp, _vp]),
    "sp_scan_context_compute_host": (_i, [C.POINTER(ScanContextParams), _vp, _sz, _vp]),
    "sp_scan_context_db_create": (_i, [C.POINTER(ScanContextParams), _sz, C.POINTER(_vp)]),
    "sp_scan_context_db_destroy": (None, [_vp]),
    "sp_scan_context_db_size": (_sz, [_vp]),
    "sp_scan_context_db_clear": (_i, [_vp]),
    "sp_scan_context_db_add": (_i, [_vp, _vp, _vp]),
    "sp_scan_context_db_search_workspace_bytes": (_sz, [_vp, _sz]),
    "sp_scan_context_db_search": (_i, [_vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_scan_context_guesses_host": (_i, [C.POINTER(ScanContextParams), C.c_uint32, _sz, _vp]),
    "sp_compat_workspace_bytes": (_sz, [_sz]),
    "sp_compat_seeds": (_i, [_vp, _vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_compat_consensus": (_i, [_sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp]),
    "sp_compat_seeds_host": (_i, [_vp, _vp, _sz, _f, _f, _sz, _vp, _vp, _vp, _vp]),
    "sp_compat_consensus_host": (_i, [_vp, _vp, _sz, _f, _f, _vp, _sz, _sz, _vp, _vp]),
    "sp_compat_poses_host": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz)]),
    "sp_pose_score": (_i, [_vp, _vp, _sz, _vp, _sz, _f, _vp, _vp]),
    "sp_compat_select_host": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, C.POINTER(_sz)]),
    "sp_intensity_gradient": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "sp_intensity_gradient_host": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "sp_photometric_workspace_bytes": (_sz, [_sz]),
    "sp_photometric_linearize": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(PhotometricParams), _vp, _vp, _vp, _sz, _vp]),
    "sp_photometric_error": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(PhotometricParams), _vp, _vp, _sz, _vp]),
    "sp_photometric_linearize_host": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(PhotometricParams), _vp, _vp]),
    "sp_photometric_error_host": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, C.POINTER(PhotometricParams), _vp]),
}
COMPAT_MAX_MATCHES, COMPAT_MAX_SEEDS, COMPAT_MAX_K = 8192, 256, 64  # SP_COMPAT_*
SCAN_CONTEXT_MAX_RINGS, SCAN_CONTEXT_MAX_SECTORS, SCAN_CONTEXT_MAX_K, SCAN_CONTEXT_DB_MAX = 32, 64, 32, 1 << 20  # SP_SCAN_CONTEXT_*
FPFH_BINS, FPFH_STRIDE, FPFH_MAX_K, FEATURE_MATCH_MAX, RANSAC_MAX_HYPOTHESES = 33, 36, 64, 1 << 20, 1 << 20  # SP_FPFH_*, ...


# csrc/sp_internal.h: per-handle measurement / tuning switches, exported for tests/, bench.py and scratch/ — not part of the
# C ABI, so not in the table above (tests/test_cabi.py checks that the public header does not mention them)
INTERNAL_SIGNATURES = {
    "sp_internal_source_option": (_i, [_vp, _i, _i]),
    "sp_internal_grid_option": (_i, [_vp, _i, _i]),
    "sp_internal_bvh_option": (_i, [_vp, _i, _i]),
    "sp_internal_bvh_walk_counts": (_i, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sp_internal_grid_small_build": (_i, [_i]),
    "sp_internal_align_searched_log": (_vp, [_vp, _vp]),
    "sp_internal_source_tile_floats": (_sz, [_vp]),
    "sp_internal_source_tiles_copy": (_i, [_vp, _vp, _sz, _i, _vp]),
    "sp_internal_radix_sort_workspace_bytes": (_sz, [_sz]),
    "sp_internal_radix_sort_u32": (_i, [_vp, _vp, _vp, _vp, _sz, C.c_uint, _vp, _sz, _vp, _vp]),
    "sp_internal_radix_sort_u32_ex": (_i, [_vp, _vp, _vp, _vp, _sz, C.c_uint, C.c_uint, _i, _vp, _sz, _vp, _vp]),
    "sp_internal_radix_first_pass": (None, [_sz, C.c_uint, _vp]),
    "sp_internal_radix_sort_u64": (_i, [_vp, _vp, _vp, _vp, _sz, C.c_uint, _vp, _sz, _vp, _vp]),
    "sp_internal_exclusive_scan_workspace_bytes": (_sz, [_sz]),
    "sp_internal_exclusive_scan_u32": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "sp_internal_atan2f_host": (None, [_vp, _vp, _sz, _vp]),
    "sp_internal_fps": (_i, [_i, _vp, _sz, _sz, C.c_uint32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_internal_eigen3": (_i, [_vp, _sz, _vp, _vp, _vp]),
    "sp_internal_inverse3": (_i, [_vp, _sz, _vp, _vp]),
    "sp_internal_bbox": (_i, [_vp, _sz, C.c_uint, _vp, _vp]),
    "sp_internal_morton_keys": (_i, [_vp, _sz, _vp, _vp, _i, _vp, _vp]),
    "sp_internal_sorted_insert": (_i, [_i, _i, _i, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "sp_internal_block_reduce": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "sp_internal_finish_wave": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sp_internal_scan_context_search_form": (_i, [_i]),
}
VOXEL_BOX_SHARDS, VOXEL_BOX_SHARD_STRIDE = 16, 32  # SP_VOXEL_BOX_SHARDS, SP_VOXEL_BOX_SHARD_STRIDE
COORD = {"LIDAR": 0, "CAMERA": 1}  # SP_COORD_LIDAR, SP_COORD_CAMERA
FPS_FORM = {"auto": 0, "one_workgroup": 1, "per_sample": 2, "persistent": 3}  # sp_internal_fps's form
INTERNAL_OPTION = {"stage_mask": 0, "reuse": 1, "fast_nn": 2, "self_knn_mode": 3, "persistent": 4, "persistent_from": 5,
                   "bvh_self_heap": 6, "bvh_sort_queries": 7, "grid_sort_queries": 8, "opt_wave_query": 9, "opt_fuse_trials": 10,
                   "bvh_walk_counts": 11}


def build(force=False):
    """Compile every HIP source for gfx950 into sycl_points_amd/lib/libsycl_points_amd.so (hipcc cross-compiles
    without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "sycl_points_amd.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-j8", "-s"])
    return LIB_PATH


_lib = None


def lib():
    """The loaded library with typed entry points. torch must be imported first so that its bundled HIP runtime
    (same SONAME, libamdhip64.so.7) is the one both sides share."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the HIP path)")
        import torch  # noqa: F401  (loads libamdhip64 before our library resolves it)

        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(INTERNAL_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.sp_abi_version() != 7:
            raise ImportError("libsycl_points_amd.so ABI version mismatch")
        _lib = L
    return _lib


def check(code):
    if code != SP_OK:
        raise SpError(code, lib().sp_last_error().decode())
