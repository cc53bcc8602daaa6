"""ctypes binding of the product C-ABI (include/dsopp_hip.h -> dsopp_amd/lib/libdsopp_hip.so).

Python is only plumbing here (tests, bench, torch.distributed glue): every compute call goes through the C-ABI into
hand-written HIP kernels.  There is NO fallback: a missing library raises at import of the symbols, and every compute
entry point fails with DSOPP_HIP_ERR_HIP when no GPU is present.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSOPP_HIP_LIB: measurement aid — another build of the same library (an earlier round's, for before / after counters in one run)
LIB_PATH = os.environ.get("DSOPP_HIP_LIB") or os.path.join(_HERE, "lib", "libdsopp_hip.so")

F64, F32 = 0, 1
NUM_KERNEL_CLASSES = 11


class Options(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("initial_trust_region_radius", C.c_double),
                ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("affine_brightness_regularizer", C.c_double * 2), ("fixed_state_regularizer", C.c_double),
                ("sigma_huber_loss", C.c_double), ("estimate_uncertainty", C.c_int32), ("force_accept", C.c_int32),
                ("first_estimate_jacobians", C.c_int32), ("optimize_idepths", C.c_int32), ("dtype", C.c_int32)]


class AlignResult(C.Structure):
    _fields_ = [("rmse", C.c_double), ("energy", C.c_double), ("n_valid", C.c_int32), ("iterations", C.c_int32),
                ("T_world_target", C.c_double * 7), ("affine_brightness", C.c_double * 2), ("covariance", C.c_double * 36),
                ("H", C.c_double * 64)]


class RotationRansacResult(C.Structure):
    _fields_ = [("iterations_run", C.c_int32), ("best_iteration", C.c_int32), ("inlier_count", C.c_int32), ("matches", C.c_int32),
                ("rotation", C.c_double * 9)]


class PnpRansacOptions(C.Structure):
    _fields_ = [("lambda_0", C.c_double), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("decrease_factor", C.c_double), ("increase_factor", C.c_double), ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class PnpRansacResult(C.Structure):
    _fields_ = [("matches", C.c_int32), ("best_iteration", C.c_int32), ("best_solution", C.c_int32), ("ransac_inlier_count", C.c_int32),
                ("refined_inlier_count", C.c_int32), ("refine_iterations", C.c_int32), ("refine_flags", C.c_int32), ("reserved", C.c_int32),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("pose_ransac", C.c_double * 12), ("pose", C.c_double * 12)]


class TwoViewRansacOptions(C.Structure):
    _fields_ = [("a", C.c_double), ("lambda_0", C.c_double), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("decrease_factor", C.c_double), ("increase_factor", C.c_double), ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class TwoViewRansacResult(C.Structure):
    _fields_ = [("matches", C.c_int32), ("best_iteration", C.c_int32), ("best_solution", C.c_int32), ("ransac_inlier_count", C.c_int32),
                ("inlier_count", C.c_int32), ("refine_iterations", C.c_int32 * 2), ("refine_flags", C.c_int32 * 2), ("reserved", C.c_int32),
                ("cost_initial", C.c_double * 2), ("cost_final", C.c_double * 2), ("pose_ransac", C.c_double * 12),
                ("pose_reselect", C.c_double * 12), ("pose", C.c_double * 12)]


MAX_FRAMES = 16  # DSOPP_HIP_MAX_FRAMES
MARGINALIZATION_SPARSE, MARGINALIZATION_MAXIMUM_SIZE = 0, 1


class MarginalizationOptions(C.Structure):
    _fields_ = [("strategy", C.c_int32), ("minimum_size", C.c_int32), ("maximum_size", C.c_int32), ("maximum_share_marginalized", C.c_double)]


class MarginalizationResult(C.Structure):
    _fields_ = [("n_active", C.c_int32), ("active_ids", C.c_int32 * MAX_FRAMES), ("n_selected", C.c_int32), ("selected", C.c_int32 * MAX_FRAMES),
                ("n_marginalized", C.c_int32), ("marginalized_ids", C.c_int32 * MAX_FRAMES), ("scores", C.c_double * MAX_FRAMES),
                ("n_active_landmarks", C.c_int32 * MAX_FRAMES), ("n_marginalized_landmarks", C.c_int32 * MAX_FRAMES),
                ("n_newly_marginalized", C.c_int32), ("n_newly_outlier", C.c_int32)]


class MapOptions(C.Structure):
    _fields_ = [("estimate_uncertainty", C.c_int32), ("channels", C.c_int32), ("min_relative_baseline", C.c_double)]


class MapExportOptions(C.Structure):
    _fields_ = [("classes", C.c_int32), ("apply_filters", C.c_int32), ("max_idepth_variance", C.c_double),
                ("min_relative_baseline_filter", C.c_double), ("frame", C.c_int32), ("colours", C.c_int32)]


class GeometricBAProblem(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("num_frames", C.c_int32), ("num_landmarks", C.c_int32), ("num_observations", C.c_int32), ("reserved", C.c_int32),
                ("poses", C.c_void_p), ("positions", C.c_void_p), ("landmark_offsets", C.c_void_p), ("obs_frame", C.c_void_p),
                ("obs_xy", C.c_void_p)]


class GeometricBAOptions(C.Structure):
    _fields_ = [("a", C.c_double), ("lambda_0", C.c_double), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("decrease_factor", C.c_double), ("increase_factor", C.c_double), ("max_iterations", C.c_int32), ("iteration_group", C.c_int32)]


class GeometricBAResult(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_lambda", C.c_double), ("valid_residuals", C.c_int32),
                ("iterations", C.c_int32), ("accepted_steps", C.c_int32), ("converged", C.c_int32), ("reason", C.c_int32),
                ("reserved", C.c_int32)]


class GeometricBATrace(C.Structure):
    _fields_ = [("cost_before", C.c_double), ("cost_candidate", C.c_double), ("lambda_", C.c_double), ("accepted", C.c_int32),
                ("reserved", C.c_int32)]


GEOMETRIC_BA_DEBUG_FIELDS = ("obs_valid", "obs_residual", "obs_weight", "landmark_H", "landmark_b", "reduced_H", "reduced_b", "pose_step",
                             "system_lambda", "candidate_poses", "candidate_positions", "trace")


class GeometricBADebug(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in GEOMETRIC_BA_DEBUG_FIELDS]


GEOMETRIC_BA_PINHOLE, GEOMETRIC_BA_SIMPLE_RADIAL = 0, 1
GEOMETRIC_BA_FIX_FOCAL, GEOMETRIC_BA_FIX_CENTER, GEOMETRIC_BA_FIX_MODEL_SPECIFIC, GEOMETRIC_BA_FIX_POSES, GEOMETRIC_BA_FIX_LANDMARKS = 1, 2, 4, 8, 16


class GeometricBACamera(C.Structure):
    _fields_ = [("model", C.c_int32), ("fixed", C.c_int32), ("intrinsics", C.c_double * 5), ("max_valid_radius", C.c_double)]


GEOMETRIC_BA_CAMERA_DEBUG_FIELDS = ("obs_camera_jacobian", "candidate_intrinsics", "candidate_max_valid_radius")


class GeometricBACameraDebug(C.Structure):
    _fields_ = [("base", GeometricBADebug)] + [(name, C.c_void_p) for name in GEOMETRIC_BA_CAMERA_DEBUG_FIELDS]


CAMERA_SIMPLE_RADIAL, CAMERA_TUM_FOV, CAMERA_ATAN = 0, 1, 2
CAMERA_MAX_K = 16  # DSOPP_HIP_CAMERA_MAX_K


class CameraModel(C.Structure):
    """dsopp_hip_camera_model; the class methods take the reference constructors' arguments, size = (width, height)"""
    _fields_ = [("type", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("num_k", C.c_int32), ("params", C.c_double * 4),
                ("k", C.c_double * CAMERA_MAX_K)]

    @classmethod
    def make(cls, type_, size, params, k):
        m = cls(type=int(type_), width=int(size[0]), height=int(size[1]), num_k=len(k))
        for i, v in enumerate(params):
            m.params[i] = v
        for i, v in enumerate(list(k)[:CAMERA_MAX_K]):
            m.k[i] = v
        return m

    @classmethod
    def simple_radial(cls, size, f, cx, cy, k1, k2):
        return cls.make(CAMERA_SIMPLE_RADIAL, size, (f, cx, cy), (k1, k2))

    @classmethod
    def tum_fov(cls, size, fx, fy, cx, cy, fov):
        return cls.make(CAMERA_TUM_FOV, size, (fx, fy, cx, cy), (fov,))

    @classmethod
    def atan(cls, size, fx, fy, cx, cy, polynomial=()):
        return cls.make(CAMERA_ATAN, size, (fx, fy, cx, cy), tuple(polynomial))


def camera_model_to_pinhole(model: CameraModel):
    """dsopp_hip_camera_model_to_pinhole, no device needed: (pinhole intrinsics (fx, fy, cx, cy), derived (max_valid_radius,
    line_after_radius 0 and 1; zeros unless simple-radial))"""
    pinhole, derived = np.zeros(4), np.zeros(3)
    _chk(lib().dsopp_hip_camera_model_to_pinhole(C.byref(model), _p(pinhole), _p(derived)))
    return pinhole, derived


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

# every symbol include/dsopp_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "dsopp_hip_pyramid_group_build", "dsopp_hip_pyramid_group_create", "dsopp_hip_pyramid_group_destroy", "dsopp_hip_pyramid_group_get", "dsopp_hip_pyramid_group_set_level", "dsopp_hip_pyramid_group_set_mask", "dsopp_hip_window_group_accept_step", "dsopp_hip_window_group_begin", "dsopp_hip_window_group_calculate_energy", "dsopp_hip_window_group_calculate_step", "dsopp_hip_window_group_create", "dsopp_hip_window_group_create_reference_depth_maps", "dsopp_hip_window_group_destroy", "dsopp_hip_window_group_frame_ids", "dsopp_hip_window_group_get_covariance", "dsopp_hip_window_group_get_frame_state", "dsopp_hip_window_group_get_frame_update", "dsopp_hip_window_group_get_landmarks", "dsopp_hip_window_group_get_marginalized", "dsopp_hip_window_group_get_pose", "dsopp_hip_window_group_get_residuals", "dsopp_hip_window_group_get_system", "dsopp_hip_window_group_last_solve_ms", "dsopp_hip_window_group_linearize", "dsopp_hip_window_group_mark_frame_marginalized", "dsopp_hip_window_group_num_frames", "dsopp_hip_window_group_num_landmarks", "dsopp_hip_window_group_optimize", "dsopp_hip_window_group_optimize_repeated", "dsopp_hip_window_group_push_frame", "dsopp_hip_window_group_refill_reference_depth_maps", "dsopp_hip_window_group_reject_step", "dsopp_hip_window_group_restore", "dsopp_hip_window_group_set_connection", "dsopp_hip_window_group_set_deterministic", "dsopp_hip_window_group_set_landmarks", "dsopp_hip_window_group_set_lm_mode", "dsopp_hip_window_group_set_max_iterations", "dsopp_hip_window_group_shard", "dsopp_hip_window_group_size", "dsopp_hip_window_group_snapshot", "dsopp_hip_window_group_solve", "dsopp_hip_window_group_update_point_statuses",
    "dsopp_hip_window_frame_ids", "dsopp_hip_window_set_deterministic",
    "dsopp_hip_comm_unique_id", "dsopp_hip_comm_create", "dsopp_hip_comm_adopt", "dsopp_hip_comm_destroy", "dsopp_hip_comm_abort", "dsopp_hip_comm_rank",
    "dsopp_hip_comm_allreduce", "dsopp_hip_window_set_comm",
    "dsopp_hip_window_optimize_async", "dsopp_hip_window_optimize_wait",
    "dsopp_hip_immature_sets_estimate",
    "dsopp_hip_undistorter_create", "dsopp_hip_undistorter_destroy", "dsopp_hip_undistorter_sizes", "dsopp_hip_undistorter_undistort",
    "dsopp_hip_undistorter_undistort_device", "dsopp_hip_pyramid_build_undistorted", "dsopp_hip_feature_extractor_extract_from_pyramid",
    "dsopp_hip_feature_extractor_create", "dsopp_hip_feature_extractor_destroy", "dsopp_hip_feature_extractor_set_mask",
    "dsopp_hip_feature_extractor_extract", "dsopp_hip_feature_extractor_get_state", "dsopp_hip_features_shuffle_order",
    "dsopp_hip_feature_extractor_create_eigen", "dsopp_hip_feature_extractor_get_eigen_stats", "dsopp_hip_eigen_random_pattern",
    "dsopp_hip_immature_set_create_from_features", "dsopp_hip_immature_set_download_inputs",
    "dsopp_hip_aligner_set_rotation_prior",
    "dsopp_hip_window_refill_reference_depth_maps",
    "dsopp_hip_initialization_poses",
    "dsopp_hip_depth_maps_mean_square_optical_flow",
    "dsopp_hip_window_activate_landmarks",
    "dsopp_hip_last_error", "dsopp_hip_device_count", "dsopp_hip_version", "dsopp_hip_default_pba_options",
    "dsopp_hip_default_align_options", "dsopp_hip_pyramid_create", "dsopp_hip_pyramid_destroy", "dsopp_hip_pyramid_build",
    "dsopp_hip_pyramid_build_device", "dsopp_hip_pyramid_set_level", "dsopp_hip_pyramid_set_mask", "dsopp_hip_pyramid_get_level",
    "dsopp_hip_pyramid_level_size", "dsopp_hip_window_create", "dsopp_hip_window_destroy", "dsopp_hip_window_push_frame",
    "dsopp_hip_window_set_landmarks", "dsopp_hip_window_set_connection", "dsopp_hip_window_mark_frame_marginalized",
    "dsopp_hip_window_num_frames", "dsopp_hip_window_solve", "dsopp_hip_window_begin", "dsopp_hip_window_calculate_energy",
    "dsopp_hip_window_linearize", "dsopp_hip_window_get_system", "dsopp_hip_window_calculate_step", "dsopp_hip_window_accept_step",
    "dsopp_hip_window_reject_step", "dsopp_hip_window_update_point_statuses", "dsopp_hip_window_get_frame_state",
    "dsopp_hip_window_get_pose", "dsopp_hip_window_num_landmarks", "dsopp_hip_window_get_landmarks", "dsopp_hip_window_get_residuals",
    "dsopp_hip_window_get_marginalized", "dsopp_hip_window_get_covariance", "dsopp_hip_window_set_allreduce",
    "dsopp_hip_window_last_solve_ms", "dsopp_hip_window_optimize", "dsopp_hip_window_optimize_repeated", "dsopp_hip_window_get_frame_update", "dsopp_hip_window_create_reference_depth_maps", "dsopp_hip_depth_maps_destroy", "dsopp_hip_depth_maps_level_size", "dsopp_hip_depth_maps_get_level", "dsopp_hip_aligner_push_reference_depth_maps", "dsopp_hip_aligner_estimate_pose", "dsopp_hip_aligner_set_hypothesis_width", "dsopp_hip_aligner_set_lm_path", "dsopp_hip_estimate_depths", "dsopp_hip_immature_set_create", "dsopp_hip_immature_set_destroy", "dsopp_hip_immature_set_upload_state", "dsopp_hip_immature_set_download_state", "dsopp_hip_immature_set_estimate", "dsopp_hip_window_set_max_iterations", "dsopp_hip_window_set_lm_mode", "dsopp_hip_window_time_kernel", "dsopp_hip_window_snapshot", "dsopp_hip_window_restore",
    "dsopp_hip_window_set_profiling", "dsopp_hip_window_get_profile", "dsopp_hip_kernel_class_name", "dsopp_hip_aligner_create", "dsopp_hip_aligner_destroy", "dsopp_hip_aligner_reset",
    "dsopp_hip_aligner_push_reference_depth_map", "dsopp_hip_aligner_push_reference_points", "dsopp_hip_aligner_push_target",
    "dsopp_hip_aligner_push_known_pose", "dsopp_hip_aligner_solve", "dsopp_hip_aligner_num_points",
    "dsopp_hip_semantics_create", "dsopp_hip_semantics_destroy", "dsopp_hip_pyramid_set_semantics", "dsopp_hip_pyramid_get_semantics",
    "dsopp_hip_pyramid_get_mask", "dsopp_hip_feature_extractor_set_mask_from_pyramid", "dsopp_hip_window_add_semantic_observations",
    "dsopp_hip_window_get_semantic_observations", "dsopp_hip_window_get_semantic_types", "dsopp_hip_pyramid_group_set_semantics",
    "dsopp_hip_window_group_add_semantic_observations", "dsopp_hip_window_group_get_semantic_observations",
    "dsopp_hip_window_group_get_semantic_types",
    "dsopp_hip_transformer_create", "dsopp_hip_transformer_destroy", "dsopp_hip_transformer_sizes", "dsopp_hip_transform_calibration",
    "dsopp_hip_transformer_transform_image", "dsopp_hip_transformer_transform_mask", "dsopp_hip_transformer_transform_device",
    "dsopp_hip_pyramid_build_transformed", "dsopp_hip_semantics_create_transformed",
    "dsopp_hip_undistorter_undistort_bgr_device", "dsopp_hip_transformer_transform_bgr_device", "dsopp_hip_pyramid_build_colour",
    "dsopp_hip_pyramid_get_image",
    "dsopp_hip_camera_model_to_pinhole", "dsopp_hip_undistorter_create_from_model",
    "dsopp_hip_flow_tracker_create", "dsopp_hip_flow_tracker_destroy", "dsopp_hip_flow_tracker_num_levels",
    "dsopp_hip_flow_tracker_set_reference", "dsopp_hip_flow_tracker_set_reference_device", "dsopp_hip_flow_tracker_set_reference_from_pyramid",
    "dsopp_hip_flow_tracker_track", "dsopp_hip_flow_tracker_track_device", "dsopp_hip_flow_tracker_track_from_pyramid",
    "dsopp_hip_flow_tracker_get_level",
    "dsopp_hip_orb_features_per_level", "dsopp_hip_orb_detector_create", "dsopp_hip_orb_detector_destroy", "dsopp_hip_orb_detector_set_mask",
    "dsopp_hip_orb_detector_set_mask_from_pyramid", "dsopp_hip_orb_detector_detect", "dsopp_hip_orb_detector_detect_device",
    "dsopp_hip_orb_detector_detect_from_pyramid", "dsopp_hip_orb_detector_get_level",
    "dsopp_hip_rotation_ransac_create", "dsopp_hip_rotation_ransac_destroy", "dsopp_hip_rotation_ransac_estimate",
    "dsopp_hip_geometric_ba_default_options", "dsopp_hip_geometric_ba_create", "dsopp_hip_geometric_ba_destroy", "dsopp_hip_geometric_ba_evaluate",
    "dsopp_hip_geometric_ba_solve", "dsopp_hip_geometric_ba_triangulate", "dsopp_hip_geometric_ba_flag_outliers",
    "dsopp_hip_geometric_ba_evaluate_camera", "dsopp_hip_geometric_ba_solve_camera",
    "dsopp_hip_pnp_ransac_default_iterations", "dsopp_hip_pnp_ransac_default_options", "dsopp_hip_pnp_ransac_create", "dsopp_hip_pnp_ransac_destroy",
    "dsopp_hip_pnp_ransac_estimate",
    "dsopp_hip_two_view_ransac_default_iterations", "dsopp_hip_two_view_ransac_default_options", "dsopp_hip_two_view_ransac_create",
    "dsopp_hip_two_view_ransac_destroy", "dsopp_hip_two_view_ransac_estimate", "dsopp_hip_two_view_ransac_triangulate",
    "dsopp_hip_window_note_optimization", "dsopp_hip_window_get_optimization_counts", "dsopp_hip_marginalization_default_options",
    "dsopp_hip_window_choose_marginalization",
    "dsopp_hip_debug_views_create", "dsopp_hip_debug_views_destroy", "dsopp_hip_debug_views_frame", "dsopp_hip_debug_views_frame_device",
    "dsopp_hip_debug_views_keyframe", "dsopp_hip_debug_views_keyframe_device", "dsopp_hip_debug_views_keyframe_planes",
    "dsopp_hip_debug_views_get_maximum_idepth", "dsopp_hip_debug_views_set_maximum_idepth",
    "dsopp_hip_map_default_options", "dsopp_hip_map_default_export_options", "dsopp_hip_map_create", "dsopp_hip_map_destroy",
    "dsopp_hip_map_add_keyframe", "dsopp_hip_map_update", "dsopp_hip_map_set_records", "dsopp_hip_map_set_pose", "dsopp_hip_map_num_keyframes",
    "dsopp_hip_map_keyframe_ids", "dsopp_hip_map_num_records", "dsopp_hip_map_get_records", "dsopp_hip_map_export", "dsopp_hip_map_export_device",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                               "dsopp_amd has no CPU fallback")
        # PyTorch ships its own HIP runtime; if it is imported but its CUDA state is not up yet, bring it up BEFORE this library
        # touches the device: initialised second, torch reports "No HIP GPUs are available" (the other order works)
        torch = sys.modules.get("torch")
        if torch is not None:
            try:
                if torch.cuda.is_available() and not torch.cuda.is_initialized():
                    torch.cuda.init()
            except Exception:
                pass
        _lib = C.CDLL(LIB_PATH)
        _lib.dsopp_hip_last_error.restype = C.c_char_p
        _lib.dsopp_hip_version.restype = C.c_char_p
        _lib.dsopp_hip_kernel_class_name.restype = C.c_char_p
    return _lib


class HipError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise HipError(f"dsopp_hip error {rc}: {lib().dsopp_hip_last_error().decode()}")


def _p(a, dtype=np.float64):
    if a is None:
        return None
    assert a.dtype == dtype and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8)


def device_count() -> int:
    n = C.c_int()
    _chk(lib().dsopp_hip_device_count(C.byref(n)))
    return n.value


def default_pba_options(**kw) -> Options:
    o = Options()
    lib().dsopp_hip_default_pba_options(C.byref(o))
    for k, v in kw.items():
        if k == "affine_brightness_regularizer":
            o.affine_brightness_regularizer[0], o.affine_brightness_regularizer[1] = v
        else:
            setattr(o, k, v)
    return o


def default_marginalization_options(**kw) -> MarginalizationOptions:
    o = MarginalizationOptions()
    lib().dsopp_hip_marginalization_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_map_options(**kw) -> MapOptions:
    o = MapOptions()
    lib().dsopp_hip_map_default_options(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def default_align_options(**kw) -> Options:
    o = Options()
    lib().dsopp_hip_default_align_options(C.byref(o))
    for k, v in kw.items():
        if k == "affine_brightness_regularizer":
            o.affine_brightness_regularizer[0], o.affine_brightness_regularizer[1] = v
        else:
            setattr(o, k, v)
    return o


class Undistorter:
    """sensors::calibration::Undistorter on the device (dsopp_hip_undistorter): in_size / out_size = (width, height); map_x / map_y =
    the two float32 remap tables of shape (out_height, out_width), both None = the identity."""

    def __init__(self, in_size, out_size, map_x=None, map_y=None, device=0, stream=None):
        self._h = C.c_void_p()
        self.in_size, self.out_size, self.device = (int(in_size[0]), int(in_size[1])), (int(out_size[0]), int(out_size[1])), device
        mx = None if map_x is None else np.ascontiguousarray(map_x, dtype=np.float32)
        my = None if map_y is None else np.ascontiguousarray(map_y, dtype=np.float32)
        for m in (mx, my):
            assert m is None or m.shape == (self.out_size[1], self.out_size[0]), m.shape
        _chk(lib().dsopp_hip_undistorter_create(int(device), C.c_void_p(stream or 0), self.in_size[0], self.in_size[1], self.out_size[0],
                                                self.out_size[1], _p(mx, np.float32), _p(my, np.float32), C.byref(self._h)))

    @classmethod
    def from_model(cls, model: CameraModel, maps=False, device=0, stream=None):
        """dsopp_hip_undistorter_create_from_model: the undistorter of a distorted camera model, its tables built on the device.  With
        maps the two float32 tables come back as .map_x / .map_y (else None); .pinhole_intrinsics = (fx, fy, cx, cy) of the target"""
        u = cls.__new__(cls)
        u._h = C.c_void_p()
        u.in_size = u.out_size = (int(model.width), int(model.height))
        u.device = device
        u.map_x = np.zeros((model.height, model.width), dtype=np.float32) if maps else None
        u.map_y = np.zeros((model.height, model.width), dtype=np.float32) if maps else None
        u.pinhole_intrinsics = np.zeros(4)
        _chk(lib().dsopp_hip_undistorter_create_from_model(int(device), C.c_void_p(stream or 0), C.byref(model), _p(u.map_x, np.float32),
                                                           _p(u.map_y, np.float32), _p(u.pinhole_intrinsics), C.byref(u._h)))
        return u

    def close(self):
        if self._h:
            lib().dsopp_hip_undistorter_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sizes(self):
        """((in_width, in_height), (out_width, out_height)) as the handle reports them"""
        v = [C.c_int() for _ in range(4)]
        _chk(lib().dsopp_hip_undistorter_sizes(self._h, *[C.byref(x) for x in v]))
        return (v[0].value, v[1].value), (v[2].value, v[3].value)

    def undistort(self, image):
        """Undistorter::undistort(image): (in_height, in_width) uint8 -> (out_height, out_width) uint8, blocking"""
        img = _u8(image)
        assert img.shape == (self.in_size[1], self.in_size[0]), img.shape
        out = np.zeros((self.out_size[1], self.out_size[0]), dtype=np.uint8)
        _chk(lib().dsopp_hip_undistorter_undistort(self._h, _p(img, np.uint8), _p(out, np.uint8)))
        return out

    def undistort_device(self, in_ptr, out_ptr, stream=None):
        """the same between two device buffers (addresses as integers): enqueues on `stream`, None = the undistorter's own"""
        _chk(lib().dsopp_hip_undistorter_undistort_device(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    def undistort_bgr_device(self, bgr_in_ptr, bgr_out_ptr=None, grey_out_ptr=None, stream=None):
        """the remap of an interleaved 8-bit BGR image between device buffers (addresses as integers): the colour result, its grey
        conversion, or both (None = not wanted); enqueues on `stream`, None = the undistorter's own"""
        _chk(lib().dsopp_hip_undistorter_undistort_bgr_device(self._h, C.c_void_p(bgr_in_ptr or 0), C.c_void_p(bgr_out_ptr or 0),
                                                              C.c_void_p(grey_out_ptr or 0), C.c_void_p(stream or 0)))


LINEAR, NEAREST = 0, 1


def transform_calibration(in_size, resize_ratio=1.0, crop_levels=4, intrinsics=None):
    """transformCalibration of a resizer and a cropper on a pinhole calibration, no device needed: in_size = (width, height),
    intrinsics = (fx, fy, cx, cy) or None -> (image_size (2 doubles), intrinsics (4 doubles) or None, (out_width, out_height))"""
    k = None if intrinsics is None else _f64(intrinsics)
    assert k is None or k.shape == (4,), k.shape
    size, k_out, w, h = np.zeros(2), np.zeros(4), C.c_int(), C.c_int()
    _chk(lib().dsopp_hip_transform_calibration(int(in_size[0]), int(in_size[1]), C.c_double(resize_ratio), int(crop_levels), _p(k), _p(size),
                                               _p(k_out), C.byref(w), C.byref(h)))
    return size, (None if k is None else k_out), (w.value, h.value)


class Transformer:
    """The camera's image transformers on the device (dsopp_hip_transformer): CameraResizer at resize_ratio (1.0 = none), then ImageCropper
    down to a multiple of 2^crop_levels (0 = none).  in_size / resized_size / out_size = (width, height)."""

    def __init__(self, in_size, resize_ratio=1.0, crop_levels=4, device=0, stream=None):
        self._h = C.c_void_p()
        self.in_size, self.device = (int(in_size[0]), int(in_size[1])), device
        _chk(lib().dsopp_hip_transformer_create(int(device), C.c_void_p(stream or 0), self.in_size[0], self.in_size[1], C.c_double(resize_ratio),
                                                int(crop_levels), C.byref(self._h)))
        _, self.resized_size, self.out_size = self.sizes()

    def close(self):
        if self._h:
            lib().dsopp_hip_transformer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sizes(self):
        """((in_width, in_height), (resized_width, resized_height), (out_width, out_height)) as the handle reports them"""
        v = [C.c_int() for _ in range(6)]
        _chk(lib().dsopp_hip_transformer_sizes(self._h, *[C.byref(x) for x in v]))
        return (v[0].value, v[1].value), (v[2].value, v[3].value), (v[4].value, v[5].value)

    def _transform(self, entry, image):
        img = _u8(image)
        assert img.shape == (self.in_size[1], self.in_size[0]), img.shape
        out = np.zeros((self.out_size[1], self.out_size[0]), dtype=np.uint8)
        _chk(entry(self._h, _p(img, np.uint8), _p(out, np.uint8)))
        return out

    def transform_image(self, image):
        """runImageTransformers(image): linear resize and crop, (in_height, in_width) uint8 -> (out_height, out_width) uint8, blocking"""
        return self._transform(lib().dsopp_hip_transformer_transform_image, image)

    def transform_mask(self, mask):
        """runMaskTransformers(mask): nearest resize and crop, blocking"""
        return self._transform(lib().dsopp_hip_transformer_transform_mask, mask)

    def transform_device(self, in_ptr, out_ptr, interpolation=LINEAR, stream=None):
        """the same between two device buffers (addresses as integers): enqueues on `stream`, None = the transformer's own"""
        _chk(lib().dsopp_hip_transformer_transform_device(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(interpolation),
                                                          C.c_void_p(stream or 0)))

    def transform_bgr_device(self, bgr_in_ptr, bgr_out_ptr=None, grey_out_ptr=None, stream=None):
        """the linear resize and crop of an interleaved 8-bit BGR image between device buffers (addresses as integers): the colour
        result, its grey conversion, or both (None = not wanted); enqueues on `stream`, None = the transformer's own"""
        _chk(lib().dsopp_hip_transformer_transform_bgr_device(self._h, C.c_void_p(bgr_in_ptr or 0), C.c_void_p(bgr_out_ptr or 0),
                                                              C.c_void_p(grey_out_ptr or 0), C.c_void_p(stream or 0)))


class Semantics:
    """The per-camera constants of semantic segmentation (dsopp_hip_semantics): static_mask (height, width) uint8 or None = all 255,
    is_filtered 256 bytes (non-zero = the class leaves the mask) or None = nothing is filtered, undistorter None = class images
    arrive undistorted.  width and height must be divisible by 2^(levels - 1).  Semantics.transformed() is the form for a camera
    with image transformers."""

    def __init__(self, width, height, levels, static_mask=None, is_filtered=None, undistorter: "Undistorter | None" = None, device=0, stream=None,
                 transformer: "Transformer | None" = None):
        self._h = C.c_void_p()
        self.width, self.height, self.levels, self.device = int(width), int(height), int(levels), device
        self._undistorter, self._transformer = undistorter, transformer  # borrowed by the handle: kept alive here
        m = _u8(static_mask)
        assert m is None or m.shape == (self.height, self.width), m.shape
        f = _u8(is_filtered)
        assert f is None or f.shape == (256,), f.shape
        u = undistorter._h if undistorter is not None else None
        if transformer is not None:
            assert (self.width, self.height) == transformer.out_size, transformer.out_size
            _chk(lib().dsopp_hip_semantics_create_transformed(int(device), C.c_void_p(stream or 0), self.levels, _p(m, np.uint8), _p(f, np.uint8), u,
                                                              transformer._h, C.byref(self._h)))
        else:
            _chk(lib().dsopp_hip_semantics_create(int(device), C.c_void_p(stream or 0), self.width, self.height, self.levels, _p(m, np.uint8),
                                                  _p(f, np.uint8), u, C.byref(self._h)))

    @classmethod
    def transformed(cls, transformer: "Transformer", levels, static_mask=None, is_filtered=None, undistorter: "Undistorter | None" = None, device=0,
                    stream=None):
        """dsopp_hip_semantics_create_transformed: the size is the transformer's output, static_mask = transformer.transform_mask(undistorted
        mask); set_semantics takes the class image as the camera delivers it, remaps it, resizes it (nearest) and crops it"""
        return cls(transformer.out_size[0], transformer.out_size[1], levels, static_mask, is_filtered, undistorter, device, stream, transformer)

    def close(self):
        if self._h:
            lib().dsopp_hip_semantics_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def class_image_shape(self):
        """(rows, cols) of the class image set_semantics takes: the undistorter's input, else the transformer's, else the pyramid's size"""
        u, t = self._undistorter, self._transformer
        if u is not None:
            return (u.in_size[1], u.in_size[0])
        return (t.in_size[1], t.in_size[0]) if t is not None else (self.height, self.width)


class Pyramid:
    """Device-resident image pyramid of one frame (dsopp_hip_pyramid)."""

    def __init__(self, width, height, levels=1, dtype=F64, device=0, stream=None):
        self._h = C.c_void_p()
        self.width, self.height, self.dtype, self.device = int(width), int(height), dtype, device
        _chk(lib().dsopp_hip_pyramid_create(int(device), C.c_void_p(stream or 0), int(width), int(height), int(levels), int(dtype),
                                            C.byref(self._h)))
        self.levels = min(int(levels), 5)

    def close(self):
        if self._h:
            lib().dsopp_hip_pyramid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build(self, image_u8, lut=None, vignetting=None):
        img = _u8(image_u8)
        assert img.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_pyramid_build(self._h, _p(img, np.uint8), _p(None if lut is None else _f64(lut)), _p(_u8(vignetting), np.uint8)))

    def build_undistorted(self, undistorter: "Undistorter", image, lut=None, vignetting=None):
        """build(undistorter.undistort(image)) without the host round trip; vignetting is the already undistorted vignette"""
        img = _u8(image)
        assert img.shape == (undistorter.in_size[1], undistorter.in_size[0]), img.shape
        vig = _u8(vignetting)
        assert vig is None or vig.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_pyramid_build_undistorted(self._h, undistorter._h, _p(img, np.uint8), _p(None if lut is None else _f64(lut)),
                                                       _p(vig, np.uint8)))

    def build_transformed(self, undistorter: "Undistorter | None", transformer: "Transformer", image, lut=None, vignetting=None):
        """build(transformer.transform_image(undistorter.undistort(image))) without the host round trips (undistorter None = the image
        arrives undistorted); vignetting is the vignette already undistorted and transformed"""
        img = _u8(image)
        in_size = undistorter.in_size if undistorter is not None else transformer.in_size
        assert img.shape == (in_size[1], in_size[0]), img.shape
        vig = _u8(vignetting)
        assert vig is None or vig.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_pyramid_build_transformed(self._h, undistorter._h if undistorter is not None else None, transformer._h,
                                                       _p(img, np.uint8), _p(None if lut is None else _f64(lut)), _p(vig, np.uint8)))

    def build_colour(self, undistorter: "Undistorter | None", transformer: "Transformer | None", bgr, lut=None, vignetting=None,
                     keep_colour=False):
        """build(BGR2GRAY(transformer.transform(undistorter.undistort(bgr)))) of an (rows, cols, 3) uint8 BGR frame, all three channels
        through both stages and the grey conversion last; either stage may be None.  vignetting is the single-channel vignette already
        undistorted and transformed.  keep_colour: get_image(3) then returns the transformed colour image."""
        img = _u8(bgr)
        first = undistorter if undistorter is not None else transformer
        in_size = first.in_size if first is not None else (self.width, self.height)
        assert img.shape == (in_size[1], in_size[0], 3), img.shape
        vig = _u8(vignetting)
        assert vig is None or vig.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_pyramid_build_colour(self._h, undistorter._h if undistorter is not None else None,
                                                  transformer._h if transformer is not None else None, _p(img, np.uint8),
                                                  _p(None if lut is None else _f64(lut)), _p(vig, np.uint8), int(bool(keep_colour))))

    def get_image(self, channels=1):
        """the 8-bit image the pyramid keeps, or None: channels = 1 the grey image the levels were built from (height, width), 3 the
        colour image of a build_colour with keep_colour (height, width, 3)"""
        out = np.zeros((self.height, self.width) if channels == 1 else (self.height, self.width, max(int(channels), 1)), dtype=np.uint8)
        present = C.c_int()
        _chk(lib().dsopp_hip_pyramid_get_image(self._h, int(channels), _p(out, np.uint8), C.byref(present)))
        return out if present.value else None

    def build_device(self, image_dev_ptr, lut=None, vignetting_dev_ptr=None, vignetting_max=0.0):
        _chk(lib().dsopp_hip_pyramid_build_device(self._h, C.c_void_p(image_dev_ptr), _p(None if lut is None else _f64(lut)),
                                                  C.c_void_p(vignetting_dev_ptr or 0), C.c_double(vignetting_max)))

    def set_level(self, level, pixelinfo):
        _chk(lib().dsopp_hip_pyramid_set_level(self._h, int(level), _p(_f64(pixelinfo))))

    def set_mask(self, level, mask):
        _chk(lib().dsopp_hip_pyramid_set_mask(self._h, int(level), _p(_u8(mask), np.uint8)))

    def set_semantics(self, semantics: "Semantics", class_image):
        """the frame's class image (None = no semantic data) and the masks of all levels; only enqueues"""
        c = _u8(class_image)
        assert c is None or c.shape == semantics.class_image_shape(), c.shape
        _chk(lib().dsopp_hip_pyramid_set_semantics(self._h, semantics._h, _p(c, np.uint8)))

    def get_semantics(self):
        """the undistorted class image the pyramid keeps, or None"""
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        present = C.c_int()
        _chk(lib().dsopp_hip_pyramid_get_semantics(self._h, _p(out, np.uint8), C.byref(present)))
        return out if present.value else None

    def get_mask(self, level):
        """the mask lane of a level's texels: 1 = valid, 0 = masked"""
        w, h = self.level_size(level)
        out = np.zeros((h, w), dtype=np.uint8)
        _chk(lib().dsopp_hip_pyramid_get_mask(self._h, int(level), _p(out, np.uint8)))
        return out

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _chk(lib().dsopp_hip_pyramid_level_size(self._h, int(level), C.byref(w), C.byref(h)))
        return w.value, h.value

    def get_level(self, level):
        w, h = self.level_size(level)
        out = np.zeros((h, w, 3))
        _chk(lib().dsopp_hip_pyramid_get_level(self._h, int(level), _p(out)))
        return out


class OpticalFlowTracker:
    """features::OpticalFlowMatch's cv::calcOpticalFlowPyrLK on the device (dsopp_hip_flow_tracker): the reference image's levels and
    Scharr planes are kept, every track() builds the new frame's levels and tracks all points in one launch.  Images are (height, width)
    uint8 arrays (any row stride), device addresses as integers, or a Pyramid that keeps its 8-bit grey image."""

    def __init__(self, width, height, window=15, max_level=3, max_iterations=10, epsilon=0.01, min_eig_threshold=1e-4, device=0, stream=None):
        self._h = C.c_void_p()
        self.width, self.height, self.window, self.device = int(width), int(height), int(window), device
        _chk(lib().dsopp_hip_flow_tracker_create(int(width), int(height), int(window), int(max_level), int(max_iterations), C.c_double(epsilon),
                                                 C.c_double(min_eig_threshold), int(device), C.c_void_p(stream or 0), C.byref(self._h)))
        n = C.c_int()
        _chk(lib().dsopp_hip_flow_tracker_num_levels(self._h, C.byref(n)))
        self.num_levels = n.value

    def close(self):
        if self._h:
            lib().dsopp_hip_flow_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _image(self, image):
        """a host image as (pointer, row stride in bytes); rows must be contiguous"""
        img = np.asarray(image)
        assert img.dtype == np.uint8 and img.shape == (self.height, self.width), (img.dtype, img.shape)
        if img.strides[1] != 1 or img.strides[0] < self.width:
            img = np.ascontiguousarray(img)
        return img, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.strides[0])

    def set_reference(self, image):
        """image_from: builds and keeps its levels and derivative planes; only enqueues"""
        if isinstance(image, Pyramid):
            _chk(lib().dsopp_hip_flow_tracker_set_reference_from_pyramid(self._h, image._h))
            return
        img, ptr, stride = self._image(image)
        _chk(lib().dsopp_hip_flow_tracker_set_reference(self._h, ptr, stride))

    def set_reference_device(self, image_ptr, stride=None):
        _chk(lib().dsopp_hip_flow_tracker_set_reference_device(self._h, C.c_void_p(image_ptr), C.c_size_t(self.width if stride is None else stride)))

    def _outputs(self, points_from, with_iterations):
        pts = np.ascontiguousarray(points_from, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        out = (np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32),
               np.zeros((n, self.num_levels), np.int32) if with_iterations else None)
        args = (n, _p(pts, np.float32), _p(out[0], np.float32), _p(out[1], np.uint8), _p(out[2], np.float32), _p(out[3], np.int32))
        return pts, out, args

    def track(self, image, points_from, with_iterations=False):
        """calcOpticalFlowPyrLK(reference, image, points_from): (points_to (n, 2) float32, status (n,) uint8, err (n,) float32), and with
        with_iterations the (n, num_levels) int32 passes per level; blocking"""
        pts, out, args = self._outputs(points_from, with_iterations)
        if isinstance(image, Pyramid):
            _chk(lib().dsopp_hip_flow_tracker_track_from_pyramid(self._h, image._h, *args))
        else:
            img, ptr, stride = self._image(image)
            _chk(lib().dsopp_hip_flow_tracker_track(self._h, ptr, stride, *args))
        return out if with_iterations else out[:3]

    def track_device(self, image_ptr, points_from, stride=None, with_iterations=False):
        pts, out, args = self._outputs(points_from, with_iterations)
        _chk(lib().dsopp_hip_flow_tracker_track_device(self._h, C.c_void_p(image_ptr), C.c_size_t(self.width if stride is None else stride), *args))
        return out if with_iterations else out[:3]

    def level_size(self, level):
        w, h = self.width, self.height
        for _ in range(level):
            w, h = (w + 1) // 2, (h + 1) // 2
        return w, h

    def get_level(self, which, level, with_derivatives=False):
        """level `level` of the reference (which = 0) or of the last tracked frame (1): (h, w) uint8, and of the reference its
        Scharr plane (h, w, 2) int16 (dx, dy)"""
        w, h = self.level_size(level)
        img = np.zeros((h, w), np.uint8)
        der = np.zeros((h, w, 2), np.int16) if with_derivatives else None
        _chk(lib().dsopp_hip_flow_tracker_get_level(self._h, int(which), int(level), _p(img, np.uint8), _p(der, np.int16)))
        return (img, der) if with_derivatives else img


def orb_features_per_level(nfeatures, nlevels):
    """the features cv::ORB grants each of its levels, (nlevels,) int32 (no device needed)"""
    out = np.zeros(max(int(nlevels), 1), np.int32)
    _chk(lib().dsopp_hip_orb_features_per_level(int(nfeatures), int(nlevels), _p(out, np.int32)))
    return out


class OrbDetector:
    """DistinctFeaturesExtractorORB's cv::ORB detection on the device (dsopp_hip_orb_detector): keypoint positions with their level and
    Harris response, in the canonical order (level, y, x).  Images are (height, width) uint8 arrays (any row stride), device addresses
    as integers, or a Pyramid that keeps its 8-bit grey image."""

    def __init__(self, width, height, nfeatures=500, nlevels=5, edge_threshold=31, fast_threshold=20, device=0, stream=None):
        self._h = C.c_void_p()
        self.width, self.height, self.nfeatures, self.num_levels, self.device = int(width), int(height), int(nfeatures), int(nlevels), device
        self._capacity = max(2 * self.nfeatures, 256)
        _chk(lib().dsopp_hip_orb_detector_create(int(width), int(height), int(nfeatures), int(nlevels), int(edge_threshold), int(fast_threshold),
                                                 int(device), C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_orb_detector_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mask(self, mask):
        """the mask bytes of every later detect ((height, width) uint8, 0 = masked), None = no mask; only enqueues"""
        m = _u8(mask)
        assert m is None or m.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_orb_detector_set_mask(self._h, _p(m, np.uint8)))

    def set_mask_from_pyramid(self, pyramid: Pyramid):
        """the level-0 mask `pyramid` kept from its last set_semantics, as validity (255 / 0); only enqueues"""
        _chk(lib().dsopp_hip_orb_detector_set_mask_from_pyramid(self._h, pyramid._h))

    def _image(self, image):
        img = np.asarray(image)
        assert img.dtype == np.uint8 and img.shape == (self.height, self.width), (img.dtype, img.shape)
        if img.strides[1] != 1 or img.strides[0] < self.width:
            img = np.ascontiguousarray(img)
        return img, img.ctypes.data_as(C.c_void_p), C.c_size_t(img.strides[0])

    def detect_raw(self, image, capacity, stride=None, outputs=None):
        """one dsopp_hip_orb_detector_detect* call with room for `capacity`: (return code, n, xy, level, response), the arrays whole
        (`outputs` = the caller's own three).  `image` is a host array, a Pyramid, or a device address with `stride`."""
        cap = int(capacity)
        xy, level, response = outputs or (np.zeros((max(cap, 1), 2), np.float32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32))
        n = C.c_int32(-1)
        args = (cap, _p(xy, np.float32), _p(level, np.int32), _p(response, np.float32), C.byref(n))
        if isinstance(image, Pyramid):
            rc = lib().dsopp_hip_orb_detector_detect_from_pyramid(self._h, image._h, *args)
        elif isinstance(image, int):
            rc = lib().dsopp_hip_orb_detector_detect_device(self._h, C.c_void_p(image), C.c_size_t(self.width if stride is None else stride), *args)
        else:
            img, ptr, row = self._image(image)
            rc = lib().dsopp_hip_orb_detector_detect(self._h, ptr, row, *args)
        return rc, n.value, xy, level, response

    def detect(self, image, stride=None):
        """(xy (n, 2) float32, level (n,) int32, response (n,) float32); blocking"""
        rc, n, xy, level, response = self.detect_raw(image, self._capacity, stride)
        if rc == -5:   # DSOPP_HIP_ERR_CAPACITY: run again with the room reported
            self._capacity = n
            rc, n, xy, level, response = self.detect_raw(image, self._capacity, stride)
        _chk(rc)
        return xy[:n].copy(), level[:n].copy(), response[:n].copy()

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _chk(lib().dsopp_hip_orb_detector_get_level(self._h, int(level), None, None, None, C.byref(w), C.byref(h)))
        return w.value, h.value

    def get_level(self, level):
        """(image, mask, FAST score plane) of level `level` after the last detect, each (h, w) uint8"""
        w, h = self.level_size(level)
        out = [np.zeros((h, w), np.uint8) for _ in range(3)]
        _chk(lib().dsopp_hip_orb_detector_get_level(self._h, int(level), _p(out[0], np.uint8), _p(out[1], np.uint8), _p(out[2], np.uint8), None, None))
        return tuple(out)


class RotationRansac:
    """estimateSO3inlierCount<3> on the device (dsopp_hip_rotation_ransac): the pure-rotation RANSAC of the bootstrap's standstill test,
    every hypothesis scored in one launch.  points_a are the NEW frame's points, points_b the last bootstrap keyframe's; the rotation maps
    bearings of points_a onto bearings of points_b.  The sample triples are the caller's."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self.device = device
        _chk(lib().dsopp_hip_rotation_ransac_create(int(device), C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_rotation_ransac_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, camera, points_a, points_b, samples, threshold=1.5, inliers_tolerance=0.95, with_hypotheses=False):
        """camera = (fx, fy, cx, cy, width, height); points (n, 2) float64; samples (iterations, 3) int32.  Returns a dict: iterations_run,
        best_iteration, inlier_count, matches, rotation (3, 3), inliers (ascending int32), and with with_hypotheses the per-hypothesis
        hyp_counts (iterations,), hyp_rotations (iterations, 3, 3), hyp_valid (iterations,) uint8; blocking"""
        fx, fy, cx, cy, width, height = camera
        a = np.ascontiguousarray(points_a, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(points_b, dtype=np.float64).reshape(-1, 2)
        s = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
        assert a.shape == b.shape, (a.shape, b.shape)
        n, m = len(a), len(s)
        res = RotationRansacResult()
        idx = np.zeros(n, np.int32)
        hyp = (np.zeros(m, np.int32), np.zeros((m, 3, 3)), np.zeros(m, np.uint8)) if with_hypotheses else (None, None, None)
        _chk(lib().dsopp_hip_rotation_ransac_estimate(self._h, C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), int(width), int(height),
                                                      n, _p(a), _p(b), m, _p(s, np.int32), C.c_double(threshold), C.c_double(inliers_tolerance),
                                                      C.byref(res), _p(idx, np.int32), _p(hyp[0], np.int32), _p(hyp[1]), _p(hyp[2], np.uint8)))
        out = {"iterations_run": res.iterations_run, "best_iteration": res.best_iteration, "inlier_count": res.inlier_count,
               "matches": res.matches, "rotation": np.array(res.rotation).reshape(3, 3), "inliers": idx[:res.inlier_count].copy()}
        if with_hypotheses:
            out.update(hyp_counts=hyp[0], hyp_rotations=hyp[1], hyp_valid=hyp[2])
        return out


def default_pnp_ransac_options(**kw) -> PnpRansacOptions:
    o = PnpRansacOptions()
    lib().dsopp_hip_pnp_ransac_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def pnp_ransac_default_iterations() -> int:
    return int(lib().dsopp_hip_pnp_ransac_default_iterations())


class PnpRansac:
    """estimateSE3PnP on the device (dsopp_hip_pnp_ransac): the pose of a bootstrap frame from its landmarks with a position, every
    three-point hypothesis scored in one launch, the winner refined over its inliers and the inliers selected again.  Poses are world to
    camera, 12 doubles: R row-major, then t.  The sample triples are the caller's."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self.device = device
        _chk(lib().dsopp_hip_pnp_ransac_create(int(device), C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_pnp_ransac_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, camera, X, obs, samples, threshold_px=0.5, options=None, with_hypotheses=False):
        """camera = (fx, fy, cx, cy, width, height); X (n, 3) and obs (n, 2) float64; samples (iterations, 3) int32; options: a
        PnpRansacOptions (None = the defaults).  Returns a dict: the result record's fields (pose_ransac and pose as (12,) arrays),
        inliers (ascending int32), and with with_hypotheses the per-hypothesis hyp_num_solutions (iterations,), hyp_poses
        (iterations, 4, 12), hyp_counts (iterations, 4); blocking"""
        fx, fy, cx, cy, width, height = camera
        x = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        o = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 2)
        s = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
        assert len(x) == len(o), (x.shape, o.shape)
        n, m = len(x), len(s)
        res = PnpRansacResult()
        idx = np.zeros(n, np.int32)
        hyp = (np.zeros(m, np.int32), np.zeros((m, 4, 12)), np.zeros((m, 4), np.int32)) if with_hypotheses else (None, None, None)
        _chk(lib().dsopp_hip_pnp_ransac_estimate(self._h, C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), int(width), int(height),
                                                 n, _p(x), _p(o), m, _p(s, np.int32), C.c_double(threshold_px),
                                                 C.byref(options) if options is not None else None, C.byref(res), _p(idx, np.int32),
                                                 _p(hyp[0], np.int32), _p(hyp[1]), _p(hyp[2], np.int32)))
        out = {name: getattr(res, name) for name, _ in PnpRansacResult._fields_ if name not in ("reserved", "pose_ransac", "pose")}
        out.update(pose_ransac=np.array(res.pose_ransac), pose=np.array(res.pose), inliers=idx[:res.refined_inlier_count].copy())
        if with_hypotheses:
            out.update(hyp_num_solutions=hyp[0], hyp_poses=hyp[1], hyp_counts=hyp[2])
        return out


def default_two_view_ransac_options(**kw) -> TwoViewRansacOptions:
    o = TwoViewRansacOptions()
    lib().dsopp_hip_two_view_ransac_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def two_view_ransac_default_iterations() -> int:
    return int(lib().dsopp_hip_two_view_ransac_default_iterations())


class TwoViewRansac:
    """estimateSO3xS2 and the two-view triangulatePoints on the device (dsopp_hip_two_view_ransac): the pose between the first and the
    last bootstrap frame from their matches, every five-point hypothesis scored in one launch, the winner refined over its inliers, the
    inliers selected again and the pose refined over those.  A pose is 12 doubles, R row-major, then t, |t| = 1, and maps the last frame
    (B) into the first (A).  The samples are the caller's."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self.device = device
        _chk(lib().dsopp_hip_two_view_ransac_create(int(device), C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_two_view_ransac_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, camera, A, B, samples, threshold_px=0.5, min_matches=50, options=None, with_hypotheses=False):
        """camera = (fx, fy, cx, cy, width, height); A, B (n, 2) float64: the first and the last frame's observations; samples
        (iterations, 5) int32; options: a TwoViewRansacOptions (None = the defaults).  Returns a dict: the result record's fields (the
        per-stage ones as 2-tuples, the three poses as (12,) arrays), inliers (ascending int32), and with with_hypotheses the
        per-hypothesis hyp_num_solutions (iterations,), hyp_poses (iterations, 10, 12), hyp_counts (iterations, 10); blocking"""
        fx, fy, cx, cy, width, height = camera
        a = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 2)
        s = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 5)
        assert len(a) == len(b), (a.shape, b.shape)
        n, m = len(a), len(s)
        res = TwoViewRansacResult()
        idx = np.zeros(n, np.int32)
        hyp = (np.zeros(m, np.int32), np.zeros((m, 10, 12)), np.zeros((m, 10), np.int32)) if with_hypotheses else (None, None, None)
        _chk(lib().dsopp_hip_two_view_ransac_estimate(self._h, C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), int(width),
                                                      int(height), n, _p(a), _p(b), m, _p(s, np.int32), C.c_double(threshold_px),
                                                      int(min_matches), C.byref(options) if options is not None else None, C.byref(res),
                                                      _p(idx, np.int32), _p(hyp[0], np.int32), _p(hyp[1]), _p(hyp[2], np.int32)))
        out = {name: getattr(res, name) for name in ("matches", "best_iteration", "best_solution", "ransac_inlier_count", "inlier_count")}
        out.update({name: tuple(getattr(res, name)) for name in ("refine_iterations", "refine_flags", "cost_initial", "cost_final")})
        out.update(pose_ransac=np.array(res.pose_ransac), pose_reselect=np.array(res.pose_reselect), pose=np.array(res.pose),
                   inliers=idx[:res.inlier_count].copy())
        if with_hypotheses:
            out.update(hyp_num_solutions=hyp[0], hyp_poses=hyp[1], hyp_counts=hyp[2])
        return out

    def triangulate(self, camera, A, B, pose_a_b, pose_world_a, cos_threshold=0.9999):
        """the two-view triangulation of the pairs under pose_a_b (12,), placed by pose_world_a (12,): (X_world (n, 3), keep (n,) bool)"""
        fx, fy, cx, cy, width, height = camera
        a = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 2)
        assert len(a) == len(b), (a.shape, b.shape)
        pab = np.ascontiguousarray(pose_a_b, dtype=np.float64).reshape(12)
        pwa = np.ascontiguousarray(pose_world_a, dtype=np.float64).reshape(12)
        X, keep = np.zeros((len(a), 3)), np.zeros(len(a), np.uint8)
        _chk(lib().dsopp_hip_two_view_ransac_triangulate(self._h, C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), int(width),
                                                         int(height), len(a), _p(a), _p(b), _p(pab), _p(pwa), C.c_double(cos_threshold), _p(X),
                                                         _p(keep, np.uint8)))
        return X, keep.astype(bool)


def default_geometric_ba_options(**kw) -> GeometricBAOptions:
    o = GeometricBAOptions()
    lib().dsopp_hip_geometric_ba_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class GeometricBA:
    """The bootstrap's geometric bundle adjustment on the device (dsopp_hip_geometric_ba): evaluate, the LM solve, triangulation and pruning
    of one problem: camera = (fx, fy, cx, cy, width, height), poses (F, 12) float64 (R row-major, t of t_agent_world), positions (L, 3),
    landmark_offsets (L + 1,) int32, obs_frame (M,) int32, obs_xy (M, 2): the observations grouped by landmark."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self.device = device
        _chk(lib().dsopp_hip_geometric_ba_create(int(device), C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_geometric_ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def problem(camera, poses, positions, landmark_offsets, obs_frame, obs_xy):
        """(GeometricBAProblem, the arrays it points into: poses and positions are the copies a call updates)"""
        fx, fy, cx, cy, width, height = camera
        arrays = (np.array(poses, dtype=np.float64, order="C").reshape(-1, 12), np.array(positions, dtype=np.float64, order="C").reshape(-1, 3),
                  np.ascontiguousarray(landmark_offsets, dtype=np.int32), np.ascontiguousarray(obs_frame, dtype=np.int32),
                  np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2))
        assert len(arrays[2]) == len(arrays[1]) + 1 and len(arrays[3]) == len(arrays[4]), [a.shape for a in arrays]
        pr = GeometricBAProblem(fx, fy, cx, cy, int(width), int(height), len(arrays[0]), len(arrays[1]), len(arrays[3]), 0,
                                *[a.ctypes.data for a in arrays])
        return pr, arrays

    def evaluate(self, camera, poses, positions, landmark_offsets, obs_frame, obs_xy, a=1.5, with_observations=False):
        """dict: cost, valid_residuals, and with with_observations obs_valid (M,) uint8, obs_residual (M, 2), obs_weight (M,); blocking"""
        pr, keep = self.problem(camera, poses, positions, landmark_offsets, obs_frame, obs_xy)
        m = pr.num_observations
        cost, nvalid = C.c_double(), C.c_int32()
        obs = (np.zeros(m, np.uint8), np.zeros((m, 2)), np.zeros(m)) if with_observations else (None, None, None)
        _chk(lib().dsopp_hip_geometric_ba_evaluate(self._h, C.byref(pr), C.c_double(a), C.byref(cost), C.byref(nvalid), _p(obs[0], np.uint8),
                                                   _p(obs[1]), _p(obs[2])))
        out = {"cost": cost.value, "valid_residuals": nvalid.value}
        if with_observations:
            out.update(obs_valid=obs[0], obs_residual=obs[1], obs_weight=obs[2])
        return out

    def solve(self, camera, poses, positions, landmark_offsets, obs_frame, obs_xy, options=None, debug=False, **option_fields):
        """The LM solve.  Returns a dict: poses (F, 12), positions (L, 3), the result record's fields, and with debug the optional outputs of
        dsopp_hip_geometric_ba_debug (reduced_H (n, n), trace = the records of the iterations run, ...); blocking"""
        pr, keep = self.problem(camera, poses, positions, landmark_offsets, obs_frame, obs_xy)
        opt = options if options is not None else default_geometric_ba_options()
        for k, v in option_fields.items():
            setattr(opt, k, v)
        res = GeometricBAResult()
        f, l, m = pr.num_frames, pr.num_landmarks, pr.num_observations
        n = max(6 * (f - 1) - 1, 0)
        dbg, bufs = None, {}
        if debug:
            bufs = dict(obs_valid=np.zeros(m, np.uint8), obs_residual=np.zeros((m, 2)), obs_weight=np.zeros(m), landmark_H=np.zeros((l, 6)),
                        landmark_b=np.zeros((l, 3)), reduced_H=np.zeros((n, n)), reduced_b=np.zeros(n), pose_step=np.zeros(n),
                        system_lambda=np.zeros(1), candidate_poses=np.zeros((f, 12)), candidate_positions=np.zeros((l, 3)),
                        trace=np.zeros(max(int(opt.max_iterations), 1) * C.sizeof(GeometricBATrace), np.uint8))
            dbg = GeometricBADebug(*[bufs[name].ctypes.data for name in GEOMETRIC_BA_DEBUG_FIELDS])
        _chk(lib().dsopp_hip_geometric_ba_solve(self._h, C.byref(pr), C.byref(opt), C.byref(res), C.byref(dbg) if debug else None))
        out = {"poses": keep[0], "positions": keep[1]}
        out.update({name: getattr(res, name) for name, _ in GeometricBAResult._fields_ if name != "reserved"})
        if debug:
            records = (GeometricBATrace * res.iterations).from_buffer_copy(bufs["trace"][:res.iterations * C.sizeof(GeometricBATrace)].tobytes())
            bufs["trace"] = [(t.cost_before, t.cost_candidate, t.accepted, t.lambda_) for t in records]
            bufs["system_lambda"] = float(bufs["system_lambda"][0])
            out.update(bufs)
        return out

    @staticmethod
    def camera_record(model, intrinsics, fixed):
        values = [float(v) for v in intrinsics]
        assert len(values) in (4, 5), values
        return GeometricBACamera(int(model), int(fixed), (C.c_double * 5)(*(values + [0.0] * (5 - len(values)))), 0.0)

    @staticmethod
    def unknowns(model, fixed, num_frames):
        """(pose unknowns, free intrinsics' indices) of solve_camera's reduced system"""
        groups = ((GEOMETRIC_BA_FIX_FOCAL, GEOMETRIC_BA_FIX_FOCAL, GEOMETRIC_BA_FIX_CENTER, GEOMETRIC_BA_FIX_CENTER)
                  if model == GEOMETRIC_BA_PINHOLE else
                  (GEOMETRIC_BA_FIX_FOCAL, GEOMETRIC_BA_FIX_CENTER, GEOMETRIC_BA_FIX_CENTER, GEOMETRIC_BA_FIX_MODEL_SPECIFIC,
                   GEOMETRIC_BA_FIX_MODEL_SPECIFIC))
        return (0 if fixed & GEOMETRIC_BA_FIX_POSES else max(6 * (num_frames - 1) - 1, 0)), [k for k, g in enumerate(groups) if not fixed & g]

    def evaluate_camera(self, size, model, intrinsics, poses, positions, landmark_offsets, obs_frame, obs_xy, fixed=0, a=1.5,
                        with_observations=False):
        """evaluate with the camera (model, intrinsics: pinhole fx fy cx cy | simple radial f cx cy k1 k2) on a size = (width, height)
        image; the dict of evaluate and max_valid_radius; blocking"""
        pr, keep = self.problem((0.0, 0.0, 0.0, 0.0, size[0], size[1]), poses, positions, landmark_offsets, obs_frame, obs_xy)
        cam = self.camera_record(model, intrinsics, fixed)
        m = pr.num_observations
        cost, nvalid = C.c_double(), C.c_int32()
        obs = (np.zeros(m, np.uint8), np.zeros((m, 2)), np.zeros(m)) if with_observations else (None, None, None)
        _chk(lib().dsopp_hip_geometric_ba_evaluate_camera(self._h, C.byref(pr), C.byref(cam), C.c_double(a), C.byref(cost), C.byref(nvalid),
                                                          _p(obs[0], np.uint8), _p(obs[1]), _p(obs[2])))
        out = {"cost": cost.value, "valid_residuals": nvalid.value, "max_valid_radius": cam.max_valid_radius}
        if with_observations:
            out.update(obs_valid=obs[0], obs_residual=obs[1], obs_weight=obs[2])
        return out

    def solve_camera(self, size, model, intrinsics, poses, positions, landmark_offsets, obs_frame, obs_xy, fixed=0, options=None, debug=False,
                     **option_fields):
        """The LM solve with the camera as a parameter block: `fixed` holds the GEOMETRIC_BA_FIX_* bits.  Returns the dict of solve and
        intrinsics (4 or 5), max_valid_radius; with debug also the outputs of dsopp_hip_geometric_ba_camera_debug (reduced_H (n, n) with the
        free intrinsics' rows last, obs_camera_jacobian (M, 2, 5), candidate_intrinsics (5,), candidate_max_valid_radius); blocking"""
        pr, keep = self.problem((0.0, 0.0, 0.0, 0.0, size[0], size[1]), poses, positions, landmark_offsets, obs_frame, obs_xy)
        cam = self.camera_record(model, intrinsics, fixed)
        opt = options if options is not None else default_geometric_ba_options()
        for k, v in option_fields.items():
            setattr(opt, k, v)
        res = GeometricBAResult()
        f, l, m = pr.num_frames, pr.num_landmarks, pr.num_observations
        npose, free = self.unknowns(int(model), int(fixed), f)
        n = npose + len(free)
        dbg, bufs = None, {}
        if debug:
            bufs = dict(obs_valid=np.zeros(m, np.uint8), obs_residual=np.zeros((m, 2)), obs_weight=np.zeros(m), landmark_H=np.zeros((l, 6)),
                        landmark_b=np.zeros((l, 3)), reduced_H=np.zeros((n, n)), reduced_b=np.zeros(n), pose_step=np.zeros(n),
                        system_lambda=np.zeros(1), candidate_poses=np.zeros((f, 12)), candidate_positions=np.zeros((l, 3)),
                        trace=np.zeros(max(int(opt.max_iterations), 1) * C.sizeof(GeometricBATrace), np.uint8),
                        obs_camera_jacobian=np.zeros((m, 2, 5)), candidate_intrinsics=np.zeros(5), candidate_max_valid_radius=np.zeros(1))
            dbg = GeometricBACameraDebug(GeometricBADebug(*[bufs[name].ctypes.data for name in GEOMETRIC_BA_DEBUG_FIELDS]),
                                         *[bufs[name].ctypes.data for name in GEOMETRIC_BA_CAMERA_DEBUG_FIELDS])
        _chk(lib().dsopp_hip_geometric_ba_solve_camera(self._h, C.byref(pr), C.byref(cam), C.byref(opt), C.byref(res),
                                                       C.byref(dbg) if debug else None))
        out = {"poses": keep[0], "positions": keep[1], "intrinsics": np.array(cam.intrinsics[:len(intrinsics)]),
               "max_valid_radius": cam.max_valid_radius}
        out.update({name: getattr(res, name) for name, _ in GeometricBAResult._fields_ if name != "reserved"})
        if debug:
            records = (GeometricBATrace * res.iterations).from_buffer_copy(bufs["trace"][:res.iterations * C.sizeof(GeometricBATrace)].tobytes())
            bufs["trace"] = [(t.cost_before, t.cost_candidate, t.accepted, t.lambda_) for t in records]
            bufs["system_lambda"] = float(bufs["system_lambda"][0])
            bufs["candidate_max_valid_radius"] = float(bufs["candidate_max_valid_radius"][0])
            out.update(bufs)
        return out

    def triangulate(self, camera, poses, positions, landmark_offsets, obs_frame, obs_xy, has_position, min_number_of_projections=4,
                    retriangulation=False):
        """(triangulated (L,) uint8, positions (L, 3): the rows of the triangulated landmarks rewritten, the others as given); blocking"""
        pr, keep = self.problem(camera, poses, positions, landmark_offsets, obs_frame, obs_xy)
        has = np.ascontiguousarray(has_position, dtype=np.uint8)
        assert len(has) == pr.num_landmarks, (len(has), pr.num_landmarks)
        done = np.zeros(pr.num_landmarks, np.uint8)
        _chk(lib().dsopp_hip_geometric_ba_triangulate(self._h, C.byref(pr), _p(has, np.uint8), int(min_number_of_projections),
                                                      int(bool(retriangulation)), _p(done, np.uint8)))
        return done, keep[1]

    def flag_outliers(self, camera, poses, positions, landmark_offsets, obs_frame, obs_xy, outlier_threshold=0.5):
        """flags (M,) uint8: 1 = removeOutliers would drop the projection; blocking"""
        pr, keep = self.problem(camera, poses, positions, landmark_offsets, obs_frame, obs_xy)
        flags, count = np.zeros(pr.num_observations, np.uint8), C.c_int32()
        _chk(lib().dsopp_hip_geometric_ba_flag_outliers(self._h, C.byref(pr), C.c_double(outlier_threshold), _p(flags, np.uint8), C.byref(count)))
        assert count.value == int(flags.sum())
        return flags


class DepthMaps:
    """Device-resident reference depth maps of the newest keyframe (dsopp_hip_depth_maps)."""

    def __init__(self, handle, levels):
        self._h, self.levels = handle, int(levels)

    def close(self):
        if self._h:
            lib().dsopp_hip_depth_maps_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_depth_maps_level_size(self._h, int(level), C.byref(w), C.byref(h)))
        return w.value, h.value

    def mean_square_optical_flow(self, level, intrinsics, transforms):
        """calculateMeanSquareOpticalFlow for a list of T_target_reference (7-vectors, at most 4); returns an array"""
        T = _f64(np.concatenate([_f64(t) for t in transforms]))
        out = np.zeros(len(transforms))
        _chk(lib().dsopp_hip_depth_maps_mean_square_optical_flow(self._h, int(level), _p(_f64(intrinsics)), len(transforms), _p(T), _p(out)))
        return out

    def get_level(self, level):
        """(idepth_sum, weight), each H x W"""
        w, h = self.level_size(level)
        ids, wgt = np.zeros((h, w)), np.zeros((h, w))
        _chk(lib().dsopp_hip_depth_maps_get_level(self._h, int(level), _p(ids), _p(wgt)))
        return ids, wgt


class DebugViews:
    """The tracker's two debug views on the device (dsopp_hip_debug_views): debugCurrentFrame and debugCurrentKeyframe as (height, width, 3)
    uint8 BGR images.  colormap = 256 x {B, G, R} (None = the library's jet), stencil = 7 x 7 bytes, a circle's footprint (None = radius 3)."""

    def __init__(self, width, height, colormap=None, stencil=None, device=0, stream=None):
        self._h = C.c_void_p()
        self.width, self.height, self.device = int(width), int(height), device
        cm, st = _u8(colormap), _u8(stencil)
        assert cm is None or cm.size == 768, cm.shape
        assert st is None or st.size == 49, st.shape
        _chk(lib().dsopp_hip_debug_views_create(int(device), C.c_void_p(stream or 0), self.width, self.height, _p(cm, np.uint8), _p(st, np.uint8),
                                                C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_debug_views_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _grey(self, grey):
        g = _u8(grey)
        assert g is None or g.shape == (self.height, self.width), g.shape
        return g

    def _out(self):
        return np.zeros((self.height, self.width, 3), dtype=np.uint8)

    def frame(self, pyramid: "Pyramid", grey=None):
        """debugCurrentFrame: the pyramid's kept grey image (or `grey`) and its level-0 mask -> BGR; blocking"""
        out = self._out()
        _chk(lib().dsopp_hip_debug_views_frame(self._h, pyramid._h if pyramid is not None else None, _p(self._grey(grey), np.uint8), _p(out, np.uint8)))
        return out

    def frame_device(self, grey_ptr, mask_ptr, bgr_out_ptr, stream=None):
        """the same between device buffers (addresses as integers; mask_ptr None = all valid); only enqueues"""
        _chk(lib().dsopp_hip_debug_views_frame_device(self._h, C.c_void_p(grey_ptr or 0), C.c_void_p(mask_ptr or 0), C.c_void_p(bgr_out_ptr or 0),
                                                      C.c_void_p(stream or 0)))

    def keyframe(self, pyramid: "Pyramid", maps: "DepthMaps", grey=None):
        """debugCurrentKeyframe over level 0 of device-resident maps -> (BGR, the new maximum idepth, qualifying cells); blocking"""
        out, M, cells = self._out(), C.c_double(), C.c_int64()
        _chk(lib().dsopp_hip_debug_views_keyframe(self._h, pyramid._h if pyramid is not None else None, _p(self._grey(grey), np.uint8),
                                                  maps._h if maps is not None else None, _p(out, np.uint8), C.byref(M), C.byref(cells)))
        return out, M.value, cells.value

    def keyframe_device(self, grey_ptr, maps: "DepthMaps", bgr_out_ptr, stream=None):
        """the same from a device grey image into a device BGR image; only enqueues; maximum_idepth waits for it"""
        _chk(lib().dsopp_hip_debug_views_keyframe_device(self._h, C.c_void_p(grey_ptr or 0), maps._h if maps is not None else None,
                                                         C.c_void_p(bgr_out_ptr or 0), C.c_void_p(stream or 0)))

    def keyframe_planes(self, grey, idepth_sum, weight):
        """the same from two host planes in DepthMaps.get_level's layout; blocking"""
        ids, wgt = _f64(idepth_sum), _f64(weight)
        assert ids.shape == wgt.shape == (self.height, self.width), (ids.shape, wgt.shape)
        out, M, cells = self._out(), C.c_double(), C.c_int64()
        _chk(lib().dsopp_hip_debug_views_keyframe_planes(self._h, _p(self._grey(grey), np.uint8), _p(ids), _p(wgt), _p(out, np.uint8), C.byref(M),
                                                         C.byref(cells)))
        return out, M.value, cells.value

    @property
    def maximum_idepth(self):
        M = C.c_double()
        _chk(lib().dsopp_hip_debug_views_get_maximum_idepth(self._h, C.byref(M)))
        return M.value

    @maximum_idepth.setter
    def maximum_idepth(self, value):
        _chk(lib().dsopp_hip_debug_views_set_maximum_idepth(self._h, C.c_double(value)))


class Map:
    """The map on the device (dsopp_hip_map): keyframe landmark records that outlive the window, exported as a filtered, coloured point
    cloud.  include/dsopp_hip.h states the rules; tests/point_cloud_model.py is their NumPy statement."""
    FLAG_MARGINALIZED, FLAG_OUTLIER = 1, 2
    CLASS_ACTIVE, CLASS_MARGINALIZED, CLASS_OUTLIER = 1, 2, 4
    FRAME_KEYFRAME, FRAME_WORLD = 0, 1
    COLOURS_LANDMARK_TYPE, COLOURS_CONSTANT, COLOURS_SEMANTIC, COLOURS_IMAGE = 0, 1, 2, 3
    OUTPUTS = (("xyz", np.float64, 3), ("rgb", np.uint8, 3), ("type", np.uint8, 1), ("relative_baseline", np.float64, 1),
               ("idepth_variance", np.float64, 1), ("keyframe_index", np.int32, 1), ("record_index", np.int32, 1))

    def __init__(self, options: "MapOptions | None" = None, device=0, stream=None, **option_fields):
        self._h = C.c_void_p()
        self.options = options or default_map_options(**option_fields)
        self.device = device
        _chk(lib().dsopp_hip_map_create(int(device), C.c_void_p(stream or 0), C.byref(self.options), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _window(window):
        if not isinstance(window, HipWindow):  # (a HipWindowGroup has no single window behind it: the group form is not built)
            raise HipError(f"dsopp_hip error -1: a map takes a HipWindow, not a {type(window).__name__}")
        return window._h

    def add_keyframe(self, window: "HipWindow", frame_id, pyramid: "Pyramid | None" = None):
        """after window.push_frame(frame_id, ...): a live keyframe; the pyramid's kept 8-bit image (colour before grey) is copied"""
        _chk(lib().dsopp_hip_map_add_keyframe(self._h, self._window(window), int(frame_id), pyramid._h if pyramid is not None else None))

    def update(self, window: "HipWindow", weights=None):
        """one launch over the landmarks of all window frames the map knows; keyframes the window dropped are finalised; only enqueues"""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
        assert w is None or w.size == 256, w.shape
        _chk(lib().dsopp_hip_map_update(self._h, self._window(window), _p(w, np.uint64)))

    def set_records(self, frame_id, intrinsics, T_world_agent, uv, idepth, variance, relative_baseline, flags, type=None, rgb=None):
        """loads or replaces a finalised keyframe from host arrays"""
        n = len(idepth)
        uv, idepth, variance, rb = _f64(uv), _f64(idepth), _f64(variance), _f64(relative_baseline)
        flags, type, rgb = _u8(flags), _u8(type), _u8(rgb)
        assert uv.size == 2 * n and variance.size == n and rb.size == n and flags.size == n, (uv.shape, n)
        assert (type is None or type.size == n) and (rgb is None or rgb.size == 3 * n)
        _chk(lib().dsopp_hip_map_set_records(self._h, int(frame_id), _p(_f64(intrinsics)), _p(_f64(T_world_agent)), n, _p(uv), _p(idepth), _p(variance),
                                             _p(rb), _p(flags, np.uint8), _p(type, np.uint8), _p(rgb, np.uint8)))

    def set_pose(self, frame_id, T_world_agent):
        _chk(lib().dsopp_hip_map_set_pose(self._h, int(frame_id), _p(_f64(T_world_agent))))

    @property
    def num_keyframes(self) -> int:
        n = C.c_int32()
        _chk(lib().dsopp_hip_map_num_keyframes(self._h, C.byref(n)))
        return n.value

    def keyframe_ids(self):
        cap = max(1, self.num_keyframes)
        ids, n = np.zeros(cap, dtype=np.int32), C.c_int32()
        _chk(lib().dsopp_hip_map_keyframe_ids(self._h, cap, _p(ids, np.int32), C.byref(n)))
        return [int(x) for x in ids[:min(n.value, cap)]]

    def num_records(self, frame_id) -> int:
        n = C.c_int32()
        _chk(lib().dsopp_hip_map_num_records(self._h, int(frame_id), C.byref(n)))
        return n.value

    def records(self, frame_id):
        """one keyframe's raw records: dict(uv, idepth, variance, relative_baseline, flags, type, rgb, intrinsics, pose, has_image,
        finalised); blocking"""
        n = self.num_records(frame_id)
        out = dict(uv=np.zeros((n, 2)), idepth=np.zeros(n), variance=np.zeros(n), relative_baseline=np.zeros(n), flags=np.zeros(n, dtype=np.uint8),
                   type=np.zeros(n, dtype=np.uint8), rgb=np.zeros((n, 3), dtype=np.uint8), intrinsics=np.zeros(4), pose=np.zeros(7))
        state = np.zeros(2, dtype=np.int32)
        _chk(lib().dsopp_hip_map_get_records(self._h, int(frame_id), _p(out["uv"]), _p(out["idepth"]), _p(out["variance"]), _p(out["relative_baseline"]),
                                             _p(out["flags"], np.uint8), _p(out["type"], np.uint8), _p(out["rgb"], np.uint8), _p(out["intrinsics"]),
                                             _p(out["pose"]), _p(state, np.int32)))
        out["has_image"], out["finalised"] = bool(state[0]), bool(state[1])
        return out

    @staticmethod
    def export_options(**fields) -> "MapExportOptions":
        o = MapExportOptions()
        lib().dsopp_hip_map_default_export_options(C.byref(o))
        for k, v in fields.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        return o

    def export_raw(self, options, frame_ids, capacity, outputs, count=True, per_keyframe_counts=None, device=False):
        """dsopp_hip_map_export / _export_device as they are: `outputs` maps the names of OUTPUTS to arrays (device=True: to addresses);
        returns (return code, count or None)"""
        ids = None if frame_ids is None else np.ascontiguousarray(frame_ids, dtype=np.int32)
        n = C.c_int64(-1)
        args = [outputs.get(name) for name, _, _ in self.OUTPUTS]
        args = [C.c_void_p(a or 0) for a in args] if device else [None if a is None else a.ctypes.data_as(C.c_void_p) for a in args]
        fn = lib().dsopp_hip_map_export_device if device else lib().dsopp_hip_map_export
        rc = fn(self._h, C.byref(options) if options is not None else None, 0 if ids is None else len(ids), _p(ids, np.int32), C.c_int64(int(capacity)),
                *args, C.byref(n) if count else None, _p(per_keyframe_counts, np.int32))
        return rc, (n.value if count else None)

    def export(self, frame_ids=None, outputs=None, options: "MapExportOptions | None" = None, **option_fields):
        """the records that pass, packed, in the canonical order: dict of NumPy arrays (the names of OUTPUTS, all of them unless
        `outputs` lists some), count and per_keyframe_counts; blocking"""
        o = options or self.export_options(**option_fields)
        ids = self.keyframe_ids() if frame_ids is None else [int(i) for i in frame_ids]
        capacity = sum(self.num_records(i) for i in ids)
        wanted = [name for name, _, _ in self.OUTPUTS] if outputs is None else list(outputs)
        arrays = {name: np.zeros((capacity, k) if k > 1 else capacity, dtype=dt) for name, dt, k in self.OUTPUTS if name in wanted}
        per_kf = np.zeros(max(1, len(ids)), dtype=np.int32)
        rc, n = self.export_raw(o, None if frame_ids is None else ids, capacity, arrays, per_keyframe_counts=per_kf)
        _chk(rc)
        out = {name: a[:n] for name, a in arrays.items()}
        out["count"], out["per_keyframe_counts"] = n, per_kf[:len(ids)]
        return out


class Comm:
    """One rank of the native RCCL communicator (dsopp_hip_comm): one process per GPU.  `exchange(id_bytes_or_None) -> bytes`
    moves the 128-byte id from rank 0 to every rank (e.g. torch.distributed.broadcast_object_list, MPI, a file)."""

    ID_BYTES = 128

    def __init__(self, rank: int, world_size: int, device: int, exchange):
        self._h = C.c_void_p()
        buf = (C.c_uint8 * self.ID_BYTES)()
        if rank == 0:
            _chk(lib().dsopp_hip_comm_unique_id(buf))
        raw = exchange(bytes(buf) if rank == 0 else None)
        buf = (C.c_uint8 * self.ID_BYTES).from_buffer_copy(raw)
        _chk(lib().dsopp_hip_comm_create(buf, int(rank), int(world_size), int(device), C.byref(self._h)))
        self.rank, self.world_size = int(rank), int(world_size)

    def size(self) -> int:
        """ranks of the communicator as RCCL itself reports them (ncclCommCount, read when the communicator was created)"""
        r, n = C.c_int(), C.c_int()
        _chk(lib().dsopp_hip_comm_rank(self._h, C.byref(r), C.byref(n)))
        return n.value

    def allreduce(self, device_ptr: int, count: int, stream: int = 0):
        _chk(lib().dsopp_hip_comm_allreduce(self._h, C.c_void_p(device_ptr), C.c_size_t(count), C.c_void_p(stream or 0)))

    def close(self):
        if self._h:
            lib().dsopp_hip_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipWindow:
    """Sliding-window photometric BA on the GPU; same Python interface as oracle.pyoracle.OracleWindow."""

    def __init__(self, options: Options | None = None, device=0, stream=None):
        self.options = options or default_pba_options()
        self.device = device
        self._stream = stream
        self._h = C.c_void_p()
        _chk(lib().dsopp_hip_window_create(C.byref(self.options), int(device), C.c_void_p(stream or 0), C.byref(self._h)))
        self._pyramids = {}
        self._cb = None

    def close(self):
        if self._h:
            lib().dsopp_hip_window_destroy(self._h)
            self._h = C.c_void_p()
        for p, owned in self._pyramids.values():
            if owned:
                p.close()
        self._pyramids = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_frames(self) -> int:
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_num_frames(self._h, C.byref(n)))
        return n.value

    @property
    def K(self) -> int:
        return 8 * self.num_frames

    def push_frame(self, frame_id, timestamp, pixelinfo, mask, intrinsics, T_w_agent, exposure, affine, fixed, is_marginalized,
                   pyramid: Pyramid | None = None, level=0):
        """pixelinfo: H x W x 3 host array (uploaded into a 1-level pyramid owned by this wrapper) unless `pyramid` given."""
        owned = pyramid is None
        if pyramid is None:
            pix = _f64(pixelinfo)
            H, W = pix.shape[:2]
            pyramid = Pyramid(W, H, 1, self.options.dtype, self.device, self._stream)
            pyramid.set_level(0, pix)
            if mask is not None:
                pyramid.set_mask(0, mask)
            level = 0
        self._pyramids[int(frame_id)] = (pyramid, owned)
        _chk(lib().dsopp_hip_window_push_frame(self._h, int(frame_id), C.c_int64(int(timestamp)), pyramid._h, int(level),
                                               _p(_f64(intrinsics)), _p(_f64(T_w_agent)), C.c_double(exposure), _p(_f64(affine)),
                                               int(bool(fixed)), int(bool(is_marginalized))))
        # pushFrame folds the frames flagged for marginalisation into the prior and erases them: their pyramids are no longer
        # borrowed.  Wrapper-owned ones are freed here (a long sliding-window run would otherwise keep one per keyframe, ~10 MB each)
        alive = set(self.frame_ids())
        for fid in [k for k in self._pyramids if k not in alive]:
            p, was_owned = self._pyramids.pop(fid)
            if was_owned:
                p.close()

    def frame_ids(self):
        # sized from the window's own frame count (not from a constant mirrored here): a short buffer would make push_frame's
        # garbage collection close pyramids the window still borrows
        cap = max(1, self.num_frames)
        ids = np.zeros(cap, dtype=np.int32)
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_frame_ids(self._h, cap, ids.ctypes.data_as(C.c_void_p), C.byref(n)))
        return [int(x) for x in ids[:min(n.value, cap)]]

    def set_landmarks(self, frame_id, uv, idepth, patch, flags):
        n = len(idepth)
        _chk(lib().dsopp_hip_window_set_landmarks(self._h, int(frame_id), n, _p(_f64(uv)), _p(_f64(idepth)), _p(_f64(patch)),
                                                  _p(_u8(flags), np.uint8)))

    def set_connection(self, ref_id, tgt_id, statuses):
        st = _u8(statuses)
        _chk(lib().dsopp_hip_window_set_connection(self._h, int(ref_id), int(tgt_id), len(st), _p(st, np.uint8)))

    def mark_frame_marginalized(self, frame_id):
        _chk(lib().dsopp_hip_window_mark_frame_marginalized(self._h, int(frame_id)))

    def set_allreduce(self, fn, rank=0, world_size=1):
        """fn(device_ptr:int, count:int, stream:int) -> int.  Keeps the ctypes callback alive."""
        if fn is None:
            self._cb = None
            _chk(lib().dsopp_hip_window_set_allreduce(self._h, None, None, 0, 1))
            return
        self._cb = ALLREDUCE_FN(lambda user, ptr, count, stream: int(fn(ptr, count, stream) or 0))
        _chk(lib().dsopp_hip_window_set_allreduce(self._h, self._cb, None, int(rank), int(world_size)))

    def set_comm(self, comm: "Comm | None"):
        """native multi-GPU exchange: the library enqueues ncclAllReduce itself (no Python in the solve loop)"""
        self._comm = comm
        self._cb = None
        _chk(lib().dsopp_hip_window_set_comm(self._h, comm._h if comm is not None else None))

    def optimize(self):
        """LM loop only (no relinearisation / covariance / point statuses)."""
        e, it, nv = C.c_double(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_optimize(self._h, C.byref(e), C.byref(it), C.byref(nv)))
        return e.value, it.value, nv.value

    def get_frame_update(self, frame_id, target_ids):
        """everything updateFrame reads back for one keyframe in one transfer: dict(idepth, inv_hdd, relative_baseline,
        n_inliers, flags, status={target_id: array})"""
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_num_landmarks(self._h, int(frame_id), C.byref(n)))
        n = n.value
        tids = np.ascontiguousarray(target_ids, dtype=np.int32)
        out = dict(idepth=np.zeros(n), inv_hdd=np.zeros(n), relative_baseline=np.zeros(n), n_inliers=np.zeros(n, dtype=np.int32),
                   flags=np.zeros(n, dtype=np.uint8))
        st = np.zeros((len(tids), n), dtype=np.uint8)
        _chk(lib().dsopp_hip_window_get_frame_update(self._h, int(frame_id), _p(out["idepth"]), _p(out["inv_hdd"]), _p(out["relative_baseline"]),
                                                     out["n_inliers"].ctypes.data_as(C.c_void_p), _p(out["flags"], np.uint8), len(tids),
                                                     tids.ctypes.data_as(C.c_void_p), _p(st, np.uint8)))
        out["status"] = {int(t): st[k] for k, t in enumerate(tids)}
        return out

    def create_reference_depth_maps(self, levels: int) -> DepthMaps:
        """createReferenceDepthMaps of the window's newest keyframe, on the device"""
        h = C.c_void_p()
        _chk(lib().dsopp_hip_window_create_reference_depth_maps(self._h, int(levels), C.byref(h)))
        return DepthMaps(h, levels)

    def activate_landmarks(self, frame_ids, immature_sets, newest_pyramid: "Pyramid", T_world_newest, exposure_newest=1.0,
                           affine_newest=(0, 0), number_of_desired_points=2000, min_distance_to_neighbor=0.0, refine=True,
                           sigma_huber_loss=20.0):
        """LandmarksActivator::activate for the listed window keyframes (oldest first) and their device-resident immature
        sets against a new keyframe.  Returns (statuses per keyframe, idepths per keyframe, result dict)."""
        n = len(frame_ids)
        ids = np.ascontiguousarray(frame_ids, dtype=np.int32)
        sets = (C.c_void_p * n)(*[s._h if s is not None else None for s in immature_sets])
        st = [np.zeros(s.n if s is not None else 0, dtype=np.uint8) for s in immature_sets]
        idp = [np.zeros(s.n if s is not None else 0) for s in immature_sets]
        st_p = (C.c_void_p * n)(*[a.ctypes.data_as(C.c_void_p) for a in st])
        id_p = (C.c_void_p * n)(*[a.ctypes.data_as(C.c_void_p) for a in idp])
        dist = C.c_double(min_distance_to_neighbor)
        res = ActivationResult()
        _chk(lib().dsopp_hip_window_activate_landmarks(self._h, n, _p(ids, np.int32), sets, newest_pyramid._h, _p(_f64(T_world_newest)),
                                                       C.c_double(exposure_newest), _p(_f64(affine_newest)), int(number_of_desired_points),
                                                       C.byref(dist), int(bool(refine)), C.c_double(sigma_huber_loss), st_p, id_p, C.byref(res)))
        return st, idp, {k: getattr(res, k) for k, _ in ActivationResult._fields_}

    def refill_reference_depth_maps(self, maps: DepthMaps):
        """createReferenceDepthMaps into an existing DepthMaps object (no allocation)"""
        _chk(lib().dsopp_hip_window_refill_reference_depth_maps(self._h, maps._h))

    def optimize_async(self):
        """enqueue the LM loop on the window's stream (no host synchronisation)"""
        _chk(lib().dsopp_hip_window_optimize_async(self._h))

    def optimize_wait(self):
        e, it, nv = C.c_double(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_optimize_wait(self._h, C.byref(e), C.byref(it), C.byref(nv)))
        return e.value, it.value, nv.value

    def optimize_repeated(self, iterations_target: int):
        """{restore(); optimize()} from the snapshot until exactly `iterations_target` GN iterations ran; returns
        (iterations_done, last_energy).  Same work as the Python loop, without its per-call overhead between solves."""
        done, e = C.c_int32(), C.c_double()
        _chk(lib().dsopp_hip_window_optimize_repeated(self._h, int(iterations_target), C.byref(done), C.byref(e)))
        return done.value, e.value

    def set_max_iterations(self, n: int):
        _chk(lib().dsopp_hip_window_set_max_iterations(self._h, int(n)))
        self.options.max_iterations = int(n)

    KERNEL_CLASSES = {"pair_setup": 0, "fej": 1, "sweep_linearize": 2, "sweep_energy": 3, "schur": 4, "assemble": 5, "assemble_solve": 6,
                      "backsub": 7, "energy_reduce": 8, "accept_decide": 9,
                      "sweep_linearize_loop": 10}

    def time_kernel(self, name: str, repeats: int = 50) -> float:
        """average microseconds of `repeats` back-to-back launches of one kernel class (one HIP event pair)"""
        us = C.c_double()
        _chk(lib().dsopp_hip_window_time_kernel(self._h, self.KERNEL_CLASSES[name], int(repeats), C.byref(us)))
        return us.value

    def set_deterministic(self, enable: bool):
        """two-stage (atomic-free, bit-reproducible) build of the reduced normal equations at every window size"""
        _chk(lib().dsopp_hip_window_set_deterministic(self._h, int(bool(enable))))

    def set_lm_mode(self, mode: int):
        """0 fused device loop (default), 1 host-driven stages"""
        _chk(lib().dsopp_hip_window_set_lm_mode(self._h, int(mode)))

    def snapshot(self):
        _chk(lib().dsopp_hip_window_snapshot(self._h))

    def restore(self):
        _chk(lib().dsopp_hip_window_restore(self._h))

    def set_profiling(self, enable: bool):
        _chk(lib().dsopp_hip_window_set_profiling(self._h, int(bool(enable))))

    def get_profile(self):
        """{kernel class name: (total device ms, launches)} since profiling was enabled."""
        out = {}
        for k in range(NUM_KERNEL_CLASSES):
            ms, n = C.c_double(), C.c_int64()
            _chk(lib().dsopp_hip_window_get_profile(self._h, k, C.byref(ms), C.byref(n)))
            out[lib().dsopp_hip_kernel_class_name(k).decode()] = (ms.value, n.value)
        return out

    # stage level
    def begin(self):
        _chk(lib().dsopp_hip_window_begin(self._h))

    def calculate_energy(self):
        e, n = C.c_double(), C.c_int32()
        _chk(lib().dsopp_hip_window_calculate_energy(self._h, C.byref(e), C.byref(n)))
        return e.value, n.value

    def linearize(self):
        _chk(lib().dsopp_hip_window_linearize(self._h))

    def get_system(self):
        K = self.K
        Hpp, bpp, Hsc, bsc = np.zeros((K, K)), np.zeros(K), np.zeros((K, K)), np.zeros(K)
        _chk(lib().dsopp_hip_window_get_system(self._h, _p(Hpp), _p(bpp), _p(Hsc), _p(bsc)))
        return Hpp, bpp, Hsc, bsc

    def calculate_step(self, lam):
        step = np.zeros(self.K)
        _chk(lib().dsopp_hip_window_calculate_step(self._h, C.c_double(lam), _p(step)))
        return step

    def accept_step(self):
        a, b = C.c_double(), C.c_double()
        _chk(lib().dsopp_hip_window_accept_step(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reject_step(self):
        _chk(lib().dsopp_hip_window_reject_step(self._h))

    def update_point_statuses(self):
        _chk(lib().dsopp_hip_window_update_point_statuses(self._h))

    def solve(self):
        e, it, nv = C.c_double(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_solve(self._h, C.byref(e), C.byref(it), C.byref(nv)))
        return e.value, it.value, nv.value

    def last_solve_ms(self) -> float:
        ms = C.c_float()
        _chk(lib().dsopp_hip_window_last_solve_ms(self._h, C.byref(ms)))
        return ms.value

    # getters
    def get_frame_state(self, frame_id):
        T0, ab0, eps, step = np.zeros(7), np.zeros(2), np.zeros(8), np.zeros(8)
        _chk(lib().dsopp_hip_window_get_frame_state(self._h, int(frame_id), _p(T0), _p(ab0), _p(eps), _p(step)))
        return T0, ab0, eps, step

    def get_pose(self, frame_id):
        T, ab = np.zeros(7), np.zeros(2)
        _chk(lib().dsopp_hip_window_get_pose(self._h, int(frame_id), _p(T), _p(ab)))
        return T, ab

    def num_landmarks(self, frame_id):
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_num_landmarks(self._h, int(frame_id), C.byref(n)))
        return n.value

    def get_landmarks(self, frame_id, with_hpib=True):
        n = self.num_landmarks(frame_id)
        K = self.K
        out = dict(idepth=np.zeros(n), idepth_step=np.zeros(n), inv_hdd=np.zeros(n), b_d=np.zeros(n), relative_baseline=np.zeros(n),
                   n_inliers=np.zeros(n, dtype=np.int32), flags=np.zeros(n, dtype=np.uint8))
        hp = np.zeros((n, K)) if with_hpib else None
        _chk(lib().dsopp_hip_window_get_landmarks(self._h, int(frame_id), _p(out["idepth"]), _p(out["idepth_step"]), _p(out["inv_hdd"]),
                                                  _p(out["b_d"]), _p(out["relative_baseline"]), _p(out["n_inliers"], np.int32),
                                                  _p(out["flags"], np.uint8), _p(hp)))
        if with_hpib:
            out["hpib"] = hp
        return out

    def get_residuals(self, ref_id, tgt_id, full=False):
        n = self.num_landmarks(ref_id)
        out = dict(status=np.zeros(n, dtype=np.uint8), candidate=np.zeros(n, dtype=np.uint8), energy=np.zeros(n))
        _chk(lib().dsopp_hip_window_get_residuals(self._h, int(ref_id), int(tgt_id), n, _p(out["status"], np.uint8),
                                                  _p(out["candidate"], np.uint8), _p(out["energy"])))
        return out

    def get_marginalized(self):
        K = self.K
        H, b, e, sz = np.zeros((K, K)), np.zeros(K), C.c_double(), C.c_int32()
        _chk(lib().dsopp_hip_window_get_marginalized(self._h, _p(H), _p(b), C.byref(e), C.byref(sz)))
        return H, b, e.value

    def note_optimization(self):
        """the counting half of updateFrame: numberOfSuccessfulOptimizations += n_inliers > 3 for every landmark not flagged marginalised"""
        _chk(lib().dsopp_hip_window_note_optimization(self._h))

    def get_optimization_counts(self, frame_id):
        counts = np.zeros(self.num_landmarks(frame_id), dtype=np.int32)
        _chk(lib().dsopp_hip_window_get_optimization_counts(self._h, int(frame_id), _p(counts, np.int32)))
        return counts

    def choose_marginalization(self, options: "MarginalizationOptions | None" = None, camera_frame_ids=None, immature_sets=None, apply=False):
        """FrameMarginalizationStrategy::marginalize on the window's state.  camera_frame_ids / immature_sets: one entry per window frame
        (None: the window's ids / no immature landmarks).  Returns dict(active_ids, selected, marginalized_ids, scores, n_active_landmarks,
        n_marginalized_landmarks, n_newly_marginalized, n_newly_outlier, flags={frame id: bytes, bit0 marginalised, bit1 outlier})."""
        options = options or default_marginalization_options()
        ids = self.frame_ids() if self.num_frames else []
        cam = None if camera_frame_ids is None else np.ascontiguousarray(camera_frame_ids, dtype=np.int32)
        assert cam is None or len(cam) == len(ids)
        sets = None
        if immature_sets is not None:
            assert len(immature_sets) == len(ids)
            sets = (C.c_void_p * max(1, len(ids)))(*[s._h if s is not None else None for s in immature_sets])
        counts = [self.num_landmarks(i) for i in ids]
        flags = np.zeros(max(1, sum(counts)), dtype=np.uint8)
        res = MarginalizationResult()
        _chk(lib().dsopp_hip_window_choose_marginalization(self._h, C.byref(options), _p(cam, np.int32), sets, int(bool(apply)), C.byref(res),
                                                           _p(flags, np.uint8)))
        A = res.n_active
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        return dict(active_ids=list(res.active_ids[:A]), selected=list(res.selected[:res.n_selected]),
                    marginalized_ids=list(res.marginalized_ids[:res.n_marginalized]), scores=np.array(res.scores[:A]),
                    n_active_landmarks=list(res.n_active_landmarks[:A]), n_marginalized_landmarks=list(res.n_marginalized_landmarks[:A]),
                    n_newly_marginalized=res.n_newly_marginalized, n_newly_outlier=res.n_newly_outlier,
                    flags={fid: flags[offsets[k]:offsets[k + 1]].copy() for k, fid in enumerate(ids)})

    def get_covariance(self, ref_id, tgt_id):
        cov = np.zeros((6, 6))
        _chk(lib().dsopp_hip_window_get_covariance(self._h, int(ref_id), int(tgt_id), _p(cov)))
        return cov

    def add_semantic_observations(self, marginalized_frame_ids):
        """addSemanticObservations for the listed frames against every frame that is neither listed nor flagged marginalised"""
        ids = np.ascontiguousarray(marginalized_frame_ids, dtype=np.int32)
        _chk(lib().dsopp_hip_window_add_semantic_observations(self._h, len(ids), ids.ctypes.data_as(C.c_void_p)))

    def get_semantic_observations(self, frame_id):
        """(n_landmarks, 256) uint8: semantic_type_observations_ of every landmark of the frame"""
        hist = np.zeros((self.num_landmarks(frame_id), 256), dtype=np.uint8)
        _chk(lib().dsopp_hip_window_get_semantic_observations(self._h, int(frame_id), _p(hist, np.uint8)))
        return hist

    def get_semantic_types(self, frame_id, weights=None):
        """semanticTypeId of every landmark; weights = SemanticLegend::weights_ (256 integers) or None = no legend"""
        t = np.zeros(self.num_landmarks(frame_id), dtype=np.uint8)
        wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
        assert wt is None or wt.shape == (256,), wt.shape
        _chk(lib().dsopp_hip_window_get_semantic_types(self._h, int(frame_id), _p(wt, np.uint64), _p(t, np.uint8)))
        return t



TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_LOCAL, TRANSPORT_P2P = 0, 1, 2, 3


class PyramidGroup:
    """One keyframe's image pyramid on every distinct device of a window group (dsopp_hip_pyramid_group)."""

    def __init__(self, group: "HipWindowGroup", width, height, levels=1):
        self._h = C.c_void_p()
        self.width, self.height, self.levels = int(width), int(height), min(int(levels), 5)
        _chk(lib().dsopp_hip_pyramid_group_create(group._h, int(width), int(height), int(levels), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_pyramid_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build(self, image_u8, lut=None, vignetting=None):
        img = _u8(image_u8)
        assert img.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_pyramid_group_build(self._h, _p(img, np.uint8), _p(None if lut is None else _f64(lut)), _p(_u8(vignetting), np.uint8)))

    def set_level(self, level, pixelinfo):
        _chk(lib().dsopp_hip_pyramid_group_set_level(self._h, int(level), _p(_f64(pixelinfo))))

    def set_mask(self, level, mask):
        _chk(lib().dsopp_hip_pyramid_group_set_mask(self._h, int(level), _p(_u8(mask), np.uint8)))

    def set_semantics(self, semantics: "Semantics", class_image):
        """Pyramid.set_semantics on every pyramid of the group (all on the semantics object's device)"""
        c = _u8(class_image)
        assert c is None or c.shape == semantics.class_image_shape(), c.shape
        _chk(lib().dsopp_hip_pyramid_group_set_semantics(self._h, semantics._h, _p(c, np.uint8)))


class HipWindowGroup:
    """n landmark shards of ONE sliding window on n devices behind one object (dsopp_hip_window_group): the single-process
    multi-GPU form of the drop-in.  Same Python interface as HipWindow / oracle.pyoracle.OracleWindow; landmark arrays are the
    whole keyframe's, the group deals them over the shards and interleaves the read-backs."""

    def __init__(self, options: Options | None = None, devices=(0,), transport=TRANSPORT_AUTO):
        self.options = options or default_pba_options()
        self.devices = [int(d) for d in devices]
        self._h = C.c_void_p()
        ids = np.ascontiguousarray(self.devices, dtype=np.int32)
        _chk(lib().dsopp_hip_window_group_create(C.byref(self.options), ids.ctypes.data_as(C.c_void_p), len(ids), int(transport), C.byref(self._h)))
        self._pyramids = {}

    def close(self):
        if self._h:
            lib().dsopp_hip_window_group_destroy(self._h)
            self._h = C.c_void_p()
        for p, owned in self._pyramids.values():
            if owned:
                p.close()
        self._pyramids = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        n, t = C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_size(self._h, C.byref(n), C.byref(t)))
        return n.value

    @property
    def transport(self):
        n, t = C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_size(self._h, C.byref(n), C.byref(t)))
        return t.value

    @property
    def num_frames(self) -> int:
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_group_num_frames(self._h, C.byref(n)))
        return n.value

    @property
    def K(self) -> int:
        return 8 * self.num_frames

    def frame_ids(self):
        cap = max(1, self.num_frames)
        ids = np.zeros(cap, dtype=np.int32)
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_group_frame_ids(self._h, cap, ids.ctypes.data_as(C.c_void_p), C.byref(n)))
        return [int(x) for x in ids[:min(n.value, cap)]]

    def shard_num_landmarks(self, shard, frame_id):
        """landmarks of `frame_id` held by one shard (introspection through the shard's own window)"""
        w, dev, n = C.c_void_p(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_shard(self._h, int(shard), C.byref(w), C.byref(dev)))
        _chk(lib().dsopp_hip_window_num_landmarks(w, int(frame_id), C.byref(n)))
        return n.value

    def push_frame(self, frame_id, timestamp, pixelinfo, mask, intrinsics, T_w_agent, exposure, affine, fixed, is_marginalized,
                   pyramid: PyramidGroup | None = None, level=0):
        owned = pyramid is None
        if pyramid is None:
            pix = _f64(pixelinfo)
            H, W = pix.shape[:2]
            pyramid = PyramidGroup(self, W, H, 1)
            pyramid.set_level(0, pix)
            if mask is not None:
                pyramid.set_mask(0, mask)
            level = 0
        self._pyramids[int(frame_id)] = (pyramid, owned)
        _chk(lib().dsopp_hip_window_group_push_frame(self._h, int(frame_id), C.c_int64(int(timestamp)), pyramid._h, int(level),
                                                     _p(_f64(intrinsics)), _p(_f64(T_w_agent)), C.c_double(exposure), _p(_f64(affine)),
                                                     int(bool(fixed)), int(bool(is_marginalized))))
        alive = set(self.frame_ids())
        for fid in [k for k in self._pyramids if k not in alive]:
            p, was_owned = self._pyramids.pop(fid)
            if was_owned:
                p.close()

    def set_landmarks(self, frame_id, uv, idepth, patch, flags):
        n = len(idepth)
        _chk(lib().dsopp_hip_window_group_set_landmarks(self._h, int(frame_id), n, _p(_f64(uv)), _p(_f64(idepth)), _p(_f64(patch)),
                                                        _p(_u8(flags), np.uint8)))

    def set_connection(self, ref_id, tgt_id, statuses):
        st = _u8(statuses)
        _chk(lib().dsopp_hip_window_group_set_connection(self._h, int(ref_id), int(tgt_id), len(st), _p(st, np.uint8)))

    def mark_frame_marginalized(self, frame_id):
        _chk(lib().dsopp_hip_window_group_mark_frame_marginalized(self._h, int(frame_id)))

    def solve(self):
        e, it, nv = C.c_double(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_solve(self._h, C.byref(e), C.byref(it), C.byref(nv)))
        return e.value, it.value, nv.value

    def optimize(self):
        e, it, nv = C.c_double(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_optimize(self._h, C.byref(e), C.byref(it), C.byref(nv)))
        return e.value, it.value, nv.value

    def optimize_repeated(self, iterations_target: int):
        done, e = C.c_int32(), C.c_double()
        _chk(lib().dsopp_hip_window_group_optimize_repeated(self._h, int(iterations_target), C.byref(done), C.byref(e)))
        return done.value, e.value

    def last_solve_ms(self) -> float:
        ms = C.c_float()
        _chk(lib().dsopp_hip_window_group_last_solve_ms(self._h, C.byref(ms)))
        return ms.value

    def set_max_iterations(self, n: int):
        _chk(lib().dsopp_hip_window_group_set_max_iterations(self._h, int(n)))
        self.options.max_iterations = int(n)

    def set_deterministic(self, enable: bool):
        _chk(lib().dsopp_hip_window_group_set_deterministic(self._h, int(bool(enable))))

    def set_lm_mode(self, mode: int):
        _chk(lib().dsopp_hip_window_group_set_lm_mode(self._h, int(mode)))

    def snapshot(self):
        _chk(lib().dsopp_hip_window_group_snapshot(self._h))

    def restore(self):
        _chk(lib().dsopp_hip_window_group_restore(self._h))

    # stage level
    def begin(self):
        _chk(lib().dsopp_hip_window_group_begin(self._h))

    def calculate_energy(self):
        e, n = C.c_double(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_calculate_energy(self._h, C.byref(e), C.byref(n)))
        return e.value, n.value

    def linearize(self):
        _chk(lib().dsopp_hip_window_group_linearize(self._h))

    def get_system(self):
        K = self.K
        Hpp, bpp, Hsc, bsc = np.zeros((K, K)), np.zeros(K), np.zeros((K, K)), np.zeros(K)
        _chk(lib().dsopp_hip_window_group_get_system(self._h, _p(Hpp), _p(bpp), _p(Hsc), _p(bsc)))
        return Hpp, bpp, Hsc, bsc

    def calculate_step(self, lam):
        step = np.zeros(self.K)
        _chk(lib().dsopp_hip_window_group_calculate_step(self._h, C.c_double(lam), _p(step)))
        return step

    def accept_step(self):
        a, b = C.c_double(), C.c_double()
        _chk(lib().dsopp_hip_window_group_accept_step(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reject_step(self):
        _chk(lib().dsopp_hip_window_group_reject_step(self._h))

    def update_point_statuses(self):
        _chk(lib().dsopp_hip_window_group_update_point_statuses(self._h))

    # getters
    def get_frame_state(self, frame_id):
        T0, ab0, eps, step = np.zeros(7), np.zeros(2), np.zeros(8), np.zeros(8)
        _chk(lib().dsopp_hip_window_group_get_frame_state(self._h, int(frame_id), _p(T0), _p(ab0), _p(eps), _p(step)))
        return T0, ab0, eps, step

    def get_pose(self, frame_id):
        T, ab = np.zeros(7), np.zeros(2)
        _chk(lib().dsopp_hip_window_group_get_pose(self._h, int(frame_id), _p(T), _p(ab)))
        return T, ab

    def num_landmarks(self, frame_id):
        n = C.c_int32()
        _chk(lib().dsopp_hip_window_group_num_landmarks(self._h, int(frame_id), C.byref(n)))
        return n.value

    def get_landmarks(self, frame_id, with_hpib=True):
        n = self.num_landmarks(frame_id)
        K = self.K
        out = dict(idepth=np.zeros(n), idepth_step=np.zeros(n), inv_hdd=np.zeros(n), b_d=np.zeros(n), relative_baseline=np.zeros(n),
                   n_inliers=np.zeros(n, dtype=np.int32), flags=np.zeros(n, dtype=np.uint8))
        hp = np.zeros((n, K)) if with_hpib else None
        _chk(lib().dsopp_hip_window_group_get_landmarks(self._h, int(frame_id), _p(out["idepth"]), _p(out["idepth_step"]), _p(out["inv_hdd"]),
                                                        _p(out["b_d"]), _p(out["relative_baseline"]), _p(out["n_inliers"], np.int32),
                                                        _p(out["flags"], np.uint8), _p(hp)))
        if with_hpib:
            out["hpib"] = hp
        return out

    def get_frame_update(self, frame_id, target_ids):
        n = self.num_landmarks(frame_id)
        tids = np.ascontiguousarray(target_ids, dtype=np.int32)
        out = dict(idepth=np.zeros(n), inv_hdd=np.zeros(n), relative_baseline=np.zeros(n), n_inliers=np.zeros(n, dtype=np.int32),
                   flags=np.zeros(n, dtype=np.uint8))
        st = np.zeros((len(tids), n), dtype=np.uint8)
        _chk(lib().dsopp_hip_window_group_get_frame_update(self._h, int(frame_id), _p(out["idepth"]), _p(out["inv_hdd"]), _p(out["relative_baseline"]),
                                                           out["n_inliers"].ctypes.data_as(C.c_void_p), _p(out["flags"], np.uint8), len(tids),
                                                           tids.ctypes.data_as(C.c_void_p), _p(st, np.uint8)))
        out["status"] = {int(t): st[k] for k, t in enumerate(tids)}
        return out

    def get_residuals(self, ref_id, tgt_id, full=False):
        n = self.num_landmarks(ref_id)
        out = dict(status=np.zeros(n, dtype=np.uint8), candidate=np.zeros(n, dtype=np.uint8), energy=np.zeros(n))
        _chk(lib().dsopp_hip_window_group_get_residuals(self._h, int(ref_id), int(tgt_id), n, _p(out["status"], np.uint8),
                                                        _p(out["candidate"], np.uint8), _p(out["energy"])))
        return out

    def get_marginalized(self):
        K = self.K
        H, b, e, sz = np.zeros((K, K)), np.zeros(K), C.c_double(), C.c_int32()
        _chk(lib().dsopp_hip_window_group_get_marginalized(self._h, _p(H), _p(b), C.byref(e), C.byref(sz)))
        return H, b, e.value

    def get_covariance(self, ref_id, tgt_id):
        cov = np.zeros((6, 6))
        _chk(lib().dsopp_hip_window_group_get_covariance(self._h, int(ref_id), int(tgt_id), _p(cov)))
        return cov

    def add_semantic_observations(self, marginalized_frame_ids):
        """addSemanticObservations for the listed frames against every frame that is neither listed nor flagged marginalised"""
        ids = np.ascontiguousarray(marginalized_frame_ids, dtype=np.int32)
        _chk(lib().dsopp_hip_window_group_add_semantic_observations(self._h, len(ids), ids.ctypes.data_as(C.c_void_p)))

    def get_semantic_observations(self, frame_id):
        """(n_landmarks, 256) uint8: semantic_type_observations_ of every landmark of the frame"""
        hist = np.zeros((self.num_landmarks(frame_id), 256), dtype=np.uint8)
        _chk(lib().dsopp_hip_window_group_get_semantic_observations(self._h, int(frame_id), _p(hist, np.uint8)))
        return hist

    def get_semantic_types(self, frame_id, weights=None):
        """semanticTypeId of every landmark; weights = SemanticLegend::weights_ (256 integers) or None = no legend"""
        t = np.zeros(self.num_landmarks(frame_id), dtype=np.uint8)
        wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
        assert wt is None or wt.shape == (256,), wt.shape
        _chk(lib().dsopp_hip_window_group_get_semantic_types(self._h, int(frame_id), _p(wt, np.uint64), _p(t, np.uint8)))
        return t

    def create_reference_depth_maps(self, levels: int) -> DepthMaps:
        h = C.c_void_p()
        _chk(lib().dsopp_hip_window_group_create_reference_depth_maps(self._h, int(levels), C.byref(h)))
        return DepthMaps(h, levels)

    def refill_reference_depth_maps(self, maps: DepthMaps):
        _chk(lib().dsopp_hip_window_group_refill_reference_depth_maps(self._h, maps._h))


def estimate_depths(lms, target_pyramid: Pyramid, level, intrinsics, T_target_reference, reference_exposure=1.0, reference_affine=(0, 0),
                    target_exposure=1.0, target_affine=(0, 0), sigma_huber_loss=20.0):
    """DepthEstimation::estimate on the device; `lms` is the dict of arrays of oracle.pyoracle.new_immature_landmarks, updated in place"""
    n = len(lms["status"])
    for k in ("idepth_min", "idepth_max", "uniqueness", "search_pixel_interval"):
        lms[k] = _f64(lms[k])
    for k in ("status", "traced"):
        lms[k] = _u8(lms[k])
    _chk(lib().dsopp_hip_estimate_depths(target_pyramid._h, int(level), _p(_f64(intrinsics)), _p(_f64(T_target_reference)), C.c_double(reference_exposure),
                                         _p(_f64(reference_affine)), C.c_double(target_exposure), _p(_f64(target_affine)), C.c_double(sigma_huber_loss), n,
                                         _p(_f64(lms["projection"])), _p(_f64(lms["direction"])), _p(_f64(lms["patch"])), _p(_f64(lms["gradient"])),
                                         _p(lms["idepth_min"]), _p(lms["idepth_max"]), _p(lms["uniqueness"]), _p(lms["search_pixel_interval"]),
                                         _p(lms["status"], np.uint8), _p(lms["traced"], np.uint8)))
    return lms


def initialization_poses(T_world_previous, T_world_last, T_world_keyframe):
    """initializationPoses of the tracker (monocular_tracker.cpp:136-176); T_world_previous None = fewer than two frames"""
    out, n = np.zeros((128, 7)), C.c_int32()
    if T_world_previous is None:
        _chk(lib().dsopp_hip_initialization_poses(None, None, None, 128, _p(out), C.byref(n)))
    else:
        _chk(lib().dsopp_hip_initialization_poses(_p(_f64(T_world_previous)), _p(_f64(T_world_last)), _p(_f64(T_world_keyframe)), 128, _p(out), C.byref(n)))
    return out[:n.value].copy()


def estimate_depths_batched(sets, target_pyramid, level, intrinsics, T_target_reference, reference_exposure, reference_affine,
                            target_exposure=1.0, target_affine=(0, 0), sigma_huber_loss=20.0):
    """DepthEstimation::estimate for several keyframes' device-resident sets against one new frame in one launch"""
    n = len(sets)
    arr = (C.c_void_p * n)(*[s._h for s in sets])
    _chk(lib().dsopp_hip_immature_sets_estimate(n, arr, target_pyramid._h, int(level), _p(_f64(intrinsics)), _p(_f64(np.asarray(T_target_reference).reshape(-1))),
                                                _p(_f64(reference_exposure)), _p(_f64(np.asarray(reference_affine).reshape(-1))), C.c_double(target_exposure),
                                                _p(_f64(target_affine)), C.c_double(sigma_huber_loss)))


class ActivationResult(C.Structure):
    _fields_ = [("number_of_active_points", C.c_int32), ("n_activated", C.c_int32), ("n_skipped", C.c_int32), ("n_deleted", C.c_int32),
                ("selection_rounds", C.c_int32), ("min_distance_to_neighbor", C.c_double)]


class ImmatureSet:
    """Device-resident immature landmarks of one keyframe (dsopp_hip_immature_set)."""

    def __init__(self, lms, device=0, stream=None):
        self._h = C.c_void_p()
        self.n = len(lms["status"])
        _chk(lib().dsopp_hip_immature_set_create(int(device), C.c_void_p(stream or 0), self.n, _p(_f64(lms["projection"])), _p(_f64(lms["direction"])),
                                                 _p(_f64(lms["patch"])), _p(_f64(lms["gradient"])), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_immature_set_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, target_pyramid: Pyramid, level, intrinsics, T_target_reference, reference_exposure=1.0, reference_affine=(0, 0),
                 target_exposure=1.0, target_affine=(0, 0), sigma_huber_loss=20.0):
        _chk(lib().dsopp_hip_immature_set_estimate(self._h, target_pyramid._h, int(level), _p(_f64(intrinsics)), _p(_f64(T_target_reference)),
                                                   C.c_double(reference_exposure), _p(_f64(reference_affine)), C.c_double(target_exposure),
                                                   _p(_f64(target_affine)), C.c_double(sigma_huber_loss)))

    def sync(self):
        """wait for the set's stream (dsopp_hip_immature_set_download_state with no outputs)"""
        _chk(lib().dsopp_hip_immature_set_download_state(self._h, None, None, None, None, None, None))

    def upload(self, lms):
        """replace the estimator state (idepth interval, uniqueness, search interval, status, traced)"""
        _chk(lib().dsopp_hip_immature_set_upload_state(self._h, _p(_f64(lms["idepth_min"])), _p(_f64(lms["idepth_max"])), _p(_f64(lms["uniqueness"])),
                                                       _p(_f64(lms["search_pixel_interval"])), _p(np.ascontiguousarray(lms["status"], dtype=np.uint8), np.uint8),
                                                       _p(np.ascontiguousarray(lms["traced"], dtype=np.uint8), np.uint8)))

    def download(self):
        n = self.n
        out = dict(idepth_min=np.zeros(n), idepth_max=np.zeros(n), uniqueness=np.zeros(n), search_pixel_interval=np.zeros(n),
                   status=np.zeros(n, dtype=np.uint8), traced=np.zeros(n, dtype=np.uint8))
        _chk(lib().dsopp_hip_immature_set_download_state(self._h, _p(out["idepth_min"]), _p(out["idepth_max"]), _p(out["uniqueness"]),
                                                         _p(out["search_pixel_interval"]), _p(out["status"], np.uint8), _p(out["traced"], np.uint8)))
        return out

    @classmethod
    def from_features(cls, extractor: "FeatureExtractor", pyramid: Pyramid, intrinsics, device=0, stream=None) -> "ImmatureSet":
        """buildFeatures + pushImmatureLandmarks on the device: the landmarks of the extractor's last list inside the camera ROI, with
        patch and gradient read from level 0 of `pyramid` (dsopp_hip_immature_set_create_from_features)"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        n = C.c_int32()
        _chk(lib().dsopp_hip_immature_set_create_from_features(int(device), C.c_void_p(stream or 0), extractor._h, pyramid._h, _p(_f64(intrinsics)),
                                                               C.byref(self._h), C.byref(n)))
        self.n = n.value
        return self

    def inputs(self):
        """the input planes: projection (n, 2), direction (n, 3), patch (n, 8), gradient (n, 2)"""
        n = self.n
        out = dict(projection=np.zeros((n, 2)), direction=np.zeros((n, 3)), patch=np.zeros((n, 8)), gradient=np.zeros((n, 2)))
        _chk(lib().dsopp_hip_immature_set_download_inputs(self._h, _p(out["projection"]), _p(out["direction"]), _p(out["patch"]), _p(out["gradient"])))
        return out


def features_shuffle_order(n):
    """the permutation std::shuffle with a fresh std::default_random_engine applies to n elements (no device needed)"""
    perm = np.zeros(int(n), dtype=np.int32)
    _chk(lib().dsopp_hip_features_shuffle_order(int(n), _p(perm, np.int32)))
    return perm


class FeatureExtractor:
    """features::SobelTrackingFeaturesExtractor on the device (dsopp_hip_feature_extractor): stateful across extract() calls."""

    def __init__(self, width, height, point_density_for_detector=1500.0, quantile_level=0.6, device=0, stream=None):
        self._h = C.c_void_p()
        self.width, self.height, self.device = int(width), int(height), device
        self._mask = None
        self._capacity = 4096
        _chk(lib().dsopp_hip_feature_extractor_create(int(device), C.c_void_p(stream or 0), self.width, self.height,
                                                      C.c_double(point_density_for_detector), C.c_double(quantile_level), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_feature_extractor_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mask(self, mask):
        m = _u8(mask)
        assert m is None or m.shape == (self.height, self.width)
        _chk(lib().dsopp_hip_feature_extractor_set_mask(self._h, _p(m, np.uint8)))
        self._mask = None if m is None else m.copy()

    def set_mask_from_pyramid(self, pyramid: Pyramid):
        """the level-0 mask `pyramid` kept from its last set_semantics, eroded on the device; only enqueues.  The extract() wrappers
        compare their `mask` argument with the last set_mask: pass keep_mask=True to them after this call."""
        _chk(lib().dsopp_hip_feature_extractor_set_mask_from_pyramid(self._h, pyramid._h))
        self._mask = None

    def extract_raw(self, image, capacity):
        """one dsopp_hip_feature_extractor_extract call: (return code, xy (n, 2) or None, n)"""
        img = _u8(image)
        assert img.shape == (self.height, self.width)
        xy = np.zeros((max(int(capacity), 1), 2))
        n = C.c_int32()
        rc = lib().dsopp_hip_feature_extractor_extract(self._h, _p(img, np.uint8), int(capacity), _p(xy), C.byref(n))
        return rc, (xy[:n.value].copy() if rc == 0 else None), n.value

    def extract(self, image, mask=None, keep_mask=False):
        """TrackingFeaturesExtractor::extract(image, mask) -> (n, 2) float64 (x, y); mask None = all pixels valid; keep_mask = the
        extractor's mask stays what the last set_mask / set_mask_from_pyramid made it"""
        if not keep_mask and ((mask is None) != (self._mask is None) or (mask is not None and not np.array_equal(_u8(mask), self._mask))):
            self.set_mask(mask)
        rc, xy, n = self.extract_raw(image, self._capacity)
        if rc == -5:   # DSOPP_HIP_ERR_CAPACITY: the state is unchanged, run again with the room reported
            self._capacity = n
            rc, xy, n = self.extract_raw(image, self._capacity)
        _chk(rc)
        return xy

    def extract_from_pyramid_raw(self, pyramid: Pyramid, capacity):
        """one dsopp_hip_feature_extractor_extract_from_pyramid call: (return code, xy (n, 2) or None, n)"""
        xy = np.zeros((max(int(capacity), 1), 2))
        n = C.c_int32()
        rc = lib().dsopp_hip_feature_extractor_extract_from_pyramid(self._h, pyramid._h, int(capacity), _p(xy), C.byref(n))
        return rc, (xy[:n.value].copy() if rc == 0 else None), n.value

    def extract_from_pyramid(self, pyramid: Pyramid, mask=None, keep_mask=False):
        """extract(image, mask) of the 8-bit image `pyramid` kept from its last build_undistorted or build_transformed"""
        if not keep_mask and ((mask is None) != (self._mask is None) or (mask is not None and not np.array_equal(_u8(mask), self._mask))):
            self.set_mask(mask)
        rc, xy, n = self.extract_from_pyramid_raw(pyramid, self._capacity)
        if rc == -5:   # DSOPP_HIP_ERR_CAPACITY: the state is unchanged, run again with the room reported
            self._capacity = n
            rc, xy, n = self.extract_from_pyramid_raw(pyramid, self._capacity)
        _chk(rc)
        return xy

    def state(self):
        init, thr, ws, found = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        dens = C.c_double()
        _chk(lib().dsopp_hip_feature_extractor_get_state(self._h, C.byref(init), C.byref(thr), C.byref(ws), C.byref(dens), C.byref(found)))
        return dict(initialized=bool(init.value), grad_norm_threshold=thr.value, window_size=ws.value, point_density=dens.value,
                    found_last=found.value)


def eigen_random_pattern(width, height):
    """the eigen extractor's random pattern, (height, width) uint8: srand(3141592), then (uint8_t)rand() per pixel (no device needed)"""
    out = np.zeros((int(height), int(width)), dtype=np.uint8)
    _chk(lib().dsopp_hip_eigen_random_pattern(int(width), int(height), _p(out, np.uint8)))
    return out


class EigenFeatureExtractor(FeatureExtractor):
    """features::EigenTrackingFeaturesExtractor (DSO's pixel selector) on the device: the same handle type and methods as
    FeatureExtractor (dsopp_hip_feature_extractor_create_eigen); the window size (current_potential_) persists across extract() calls."""

    def __init__(self, width, height, point_density_for_detector=1500.0, device=0, stream=None):
        self._h = C.c_void_p()
        self.width, self.height, self.device = int(width), int(height), device
        self._mask = None
        self._capacity = 4096
        _chk(lib().dsopp_hip_feature_extractor_create_eigen(int(device), C.c_void_p(stream or 0), self.width, self.height,
                                                            C.c_double(point_density_for_detector), C.byref(self._h)))

    def stats(self):
        """the last extract's passes, window size and emissions per pass, and the top windows walked in order"""
        passes, chained = C.c_int32(), C.c_int32()
        potentials, found = (C.c_int32 * 2)(), (C.c_int32 * 2)()
        _chk(lib().dsopp_hip_feature_extractor_get_eigen_stats(self._h, C.byref(passes), potentials, found, C.byref(chained)))
        return dict(passes=passes.value, potentials=list(potentials), found=list(found), chained_windows=chained.value)


class HipAligner:
    """Two-frame direct image alignment of one pyramid level (dsopp_hip_aligner)."""

    def __init__(self, options: Options | None = None, device=0, stream=None):
        self.options = options or default_align_options()
        self._h = C.c_void_p()
        _chk(lib().dsopp_hip_aligner_create(C.byref(self.options), int(device), C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().dsopp_hip_aligner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _chk(lib().dsopp_hip_aligner_reset(self._h))

    def push_reference_depth_map(self, timestamp, T_w_agent, pyramid: Pyramid, level, intrinsics, idepth_sum, weight, exposure, affine):
        _chk(lib().dsopp_hip_aligner_push_reference_depth_map(self._h, C.c_int64(int(timestamp)), _p(_f64(T_w_agent)), pyramid._h, int(level),
                                                              _p(_f64(intrinsics)), _p(_f64(idepth_sum)), _p(_f64(weight)), C.c_double(exposure),
                                                              _p(_f64(affine))))

    def push_reference_depth_maps(self, timestamp, T_w_agent, pyramid: Pyramid, level, intrinsics, maps: DepthMaps, exposure, affine):
        _chk(lib().dsopp_hip_aligner_push_reference_depth_maps(self._h, C.c_int64(int(timestamp)), _p(_f64(T_w_agent)), pyramid._h, int(level),
                                                               _p(_f64(intrinsics)), maps._h, C.c_double(exposure), _p(_f64(affine))))

    def estimate_pose(self, ref_time, T_w_ref, ref_pyramid: Pyramid, ref_maps: DepthMaps, ref_exposure, ref_affine, tgt_time,
                      tgt_pyramid: Pyramid, tgt_exposure, intrinsics, T_w_inits, affine_init, rmse_last):
        """estimatePose of the tracker (monocular_tracker.cpp:179-245): coarse-to-fine over all levels, one C call per frame.
        T_w_inits: (n, 7) initialisations; rmse_last: per-level array, updated in place."""
        inits = _f64(np.atleast_2d(T_w_inits))
        rl = _f64(rmse_last)
        T, ab = np.zeros(7), np.zeros(2)
        ok, tries, its = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(lib().dsopp_hip_aligner_estimate_pose(self._h, C.c_int64(int(ref_time)), _p(_f64(T_w_ref)), ref_pyramid._h, ref_maps._h,
                                                   C.c_double(ref_exposure), _p(_f64(ref_affine)), C.c_int64(int(tgt_time)), tgt_pyramid._h,
                                                   C.c_double(tgt_exposure), _p(_f64(intrinsics)), len(inits), _p(inits), _p(_f64(affine_init)),
                                                   _p(rl), _p(T), _p(ab), C.byref(ok), C.byref(tries), C.byref(its)))
        rmse_last[:] = rl
        return dict(T_w_target=T, affine_brightness=ab, success=bool(ok.value), tries=tries.value, lm_iterations=its.value)

    def push_reference_points(self, timestamp, T_w_agent, pyramid: Pyramid, level, intrinsics, u, v, idepth, exposure, affine):
        _chk(lib().dsopp_hip_aligner_push_reference_points(self._h, C.c_int64(int(timestamp)), _p(_f64(T_w_agent)), pyramid._h, int(level),
                                                           _p(_f64(intrinsics)), len(u), _p(_f64(u)), _p(_f64(v)), _p(_f64(idepth)),
                                                           C.c_double(exposure), _p(_f64(affine))))

    def push_target(self, timestamp, T_w_agent_init, pyramid: Pyramid, level, intrinsics, exposure, affine):
        _chk(lib().dsopp_hip_aligner_push_target(self._h, C.c_int64(int(timestamp)), _p(_f64(T_w_agent_init)), pyramid._h, int(level),
                                                 _p(_f64(intrinsics)), C.c_double(exposure), _p(_f64(affine))))

    def set_rotation_prior(self, R_target_reference):
        """setRotationPrior (3x3, None clears); reset() clears it too"""
        R = None if R_target_reference is None else _f64(np.asarray(R_target_reference).reshape(9))
        _chk(lib().dsopp_hip_aligner_set_rotation_prior(self._h, _p(R)))

    def set_lm_path(self, path: int):
        _chk(lib().dsopp_hip_aligner_set_lm_path(self._h, int(path)))

    def set_hypothesis_width(self, width: int):
        """initialisations estimate_pose evaluates per launch: 0 automatic, 1 sequential, 2 .. 8 concurrent (one XCD each)"""
        _chk(lib().dsopp_hip_aligner_set_hypothesis_width(self._h, int(width)))

    def push_known_pose(self, timestamp, T_w_agent):
        _chk(lib().dsopp_hip_aligner_push_known_pose(self._h, C.c_int64(int(timestamp)), _p(_f64(T_w_agent))))

    def num_points(self) -> int:
        n = C.c_int32()
        _chk(lib().dsopp_hip_aligner_num_points(self._h, C.byref(n)))
        return n.value

    def solve(self):
        out = AlignResult()
        _chk(lib().dsopp_hip_aligner_solve(self._h, C.byref(out)))
        return dict(rmse=out.rmse, energy=out.energy, n_valid=out.n_valid, iterations=out.iterations,
                    T_w_target=np.array(out.T_world_target), affine_brightness=np.array(out.affine_brightness),
                    covariance=np.array(out.covariance).reshape(6, 6), H=np.array(out.H).reshape(8, 8))
