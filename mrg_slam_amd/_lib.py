"""ctypes loader of libmrgfe.so (the C ABI of include/mrgfe.h).

There is NO CPU fallback: if the HIP library is missing it is built with hipcc (cross-compiles without a GPU), and if it
cannot be loaded, or no GPU is present when a context is created, an exception is raised.  Nothing under ``oracle/`` is
ever imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
LIB_PATH = os.environ.get("MRGFE_LIB") or os.path.join(_PKG, "libmrgfe.so")  # MRGFE_LIB: kernel-variant experiments only

MRGFE_OK, ERR_INVALID, ERR_HIP, ERR_OVERFLOW, ERR_EMPTY, ERR_STATE = 0, -1, -2, -3, -4, -5
NDT_HIP, GICP_HIP, SMALL_GICP_HIP, VGICP_HIP, ICP_HIP, PCL_GICP_HIP, PCL_GICP_OMP_HIP, PCL_NDT_HIP = 0, 1, 2, 3, 4, 5, 6, 7
FIT_EXACT, FIT_PRUNED, FIT_ABOVE_CAP, FIT_SKIPPED = 0, 1, 2, 3  # enum mrgfe_fit_state (mrgfe_batch_align_best)
SEARCH = {"KDTREE": 0, "DIRECT26": 1, "DIRECT7": 2, "DIRECT1": 3}
# bits of the device-driven prefilter chain's anomaly word (mrgfe_ctx_prefilter_stats out[1])
PF_ANOMALY_EMPTY, PF_ANOMALY_OVERFLOW, PF_ANOMALY_NO_VOXEL, PF_ANOMALY_CERTIFICATE, PF_ANOMALY_RECHECK, PF_ANOMALY_CELLS = 1, 2, 4, 8, 16, 256
PF_ANOMALY_NON_FINITE = 32  # a non-finite point reached the outlier filter


def layout(stride: int, xyz_offset: int = 0, intensity_offset: int = 12) -> int:
    """MRGFE_LAYOUT(stride, xyz_offset, intensity_offset) of include/mrgfe.h: the point-layout descriptor passed as ``stride_bytes``."""
    return int(stride) | ((int(intensity_offset) + 1) << 16) | (int(xyz_offset) << 24)


LAYOUT_PACKED = 16
LAYOUT_PCL_XYZI = layout(32, 0, 16)  # in-memory pcl::PointXYZI


class MrgfeError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libmrgfe error {status}: {message}")
        self.status = status


class PrefilterParams(C.Structure):
    """struct mrgfe_prefilter_params (the prefiltering_component ROS parameters, config/mrg_slam.yaml:41-64)."""

    _fields_ = [("enable_distance_filter", C.c_int), ("distance_near_thresh", C.c_double), ("distance_far_thresh", C.c_double), ("downsample_method", C.c_int),
                ("downsample_resolution", C.c_double), ("downsample_min_points_per_voxel", C.c_int), ("outlier_removal_method", C.c_int), ("radius_radius", C.c_double),
                ("radius_min_neighbors", C.c_int), ("statistical_mean_k", C.c_int), ("statistical_stddev", C.c_double)]


class ScanParams(C.Structure):
    """struct mrgfe_scan_params: the layout of a sensor_msgs/PointCloud2 payload, what ``cloud_callback`` does to the scan before its filters
    (deskewing, the transform into base_link_frame) and the prefilter parameters."""

    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("off_z", C.c_uint32), ("off_intensity", C.c_int32), ("deskew", C.c_int), ("ang_v", C.c_float * 3), ("scan_period", C.c_double), ("transform", C.c_int),
                ("T", C.c_float * 16), ("filters", PrefilterParams)]


class ScanOutputs(C.Structure):
    """struct mrgfe_scan_outputs: where ``mrgfe_scan_callback_outputs`` leaves the filtered scan's records, the coloured cloud's records and the device cloud."""

    _fields_ = [("point_step", C.c_int), ("records", C.c_void_p), ("capacity_bytes", C.c_size_t), ("colored_records", C.c_void_p), ("colored_capacity_bytes", C.c_size_t),
                ("d_out_xyzi", C.c_void_p)]


class KeyframeParams(C.Structure):
    """struct mrgfe_keyframe_params: the layout of the sensor_msgs/PointCloud2 payload ``mrgfe_keyframe_callback`` reads."""

    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("off_z", C.c_uint32), ("off_intensity", C.c_int32)]


class PointField(C.Structure):
    """struct mrgfe_pointcloud2_field: one sensor_msgs/PointField of a message, as ``mrgfe_pointcloud2_layout`` reads it."""

    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint32), ("datatype", C.c_uint8), ("count", C.c_uint32)]


class KeyframeMsg(C.Structure):
    """struct mrgfe_keyframe_msg: one message of ``mrgfe_map_store_add_keyframes`` (key, layout, payload)."""

    _fields_ = [("key", C.c_uint64), ("layout", KeyframeParams), ("data", C.c_void_p), ("data_bytes", C.c_size_t)]


class GraphEdge(C.Structure):
    """struct mrgfe_graph_edge: one edge of ``mrgfe_map_store_edges`` (relpose column-major, Isometry3d::matrix())."""

    _fields_ = [("key1", C.c_uint64), ("key2", C.c_uint64), ("relpose", C.c_double * 16)]


class MapPublishParams(C.Structure):
    """struct mrgfe_map_publish_params: the generator's parameters (config/mrg_slam.yaml:235-237), the record layout and the save offsets."""

    _fields_ = [("resolution", C.c_float), ("min_points_per_voxel", C.c_int32), ("distance_far_thresh", C.c_float), ("skip_first_cloud", C.c_int32),
                ("point_step", C.c_int32), ("n_offsets", C.c_int32), ("offsets", C.c_float * 6)]


class MapPublishResult(C.Structure):
    """struct mrgfe_map_publish_result: the counts and the record layout of one ``mrgfe_map_store_publish``."""

    _fields_ = [("n_points", C.c_uint64), ("n_unfiltered", C.c_uint64), ("data_bytes", C.c_uint64), ("point_step", C.c_int32), ("off_intensity", C.c_int32)]


class GroundFillParams(C.Structure):
    """struct mrgfe_ground_fill_params: fill_first_cloud_radius, map_cloud_resolution, fill_first_cloud_simple (apps/mrg_slam_component.cpp:245,271-272)."""

    _fields_ = [("radius", C.c_double), ("map_resolution", C.c_double), ("simple", C.c_int32), ("pad", C.c_int32)]


class GroundFillResult(C.Structure):
    """struct mrgfe_ground_fill_result: the plane the disc was laid on and the counts of the fill."""

    _fields_ = [("has_model", C.c_int32), ("ransac_iterations", C.c_int32), ("coeffs", C.c_float * 4), ("n_before", C.c_uint32), ("n_rings", C.c_uint32),
                ("n_angles", C.c_uint32), ("n_added", C.c_uint32)]


class FloorParams(C.Structure):
    """struct mrgfe_floor_params (the floor_detection_component ROS parameters, apps/floor_detection_component.cpp:55-62, config/mrg_slam.yaml:113-122)."""

    _fields_ = [("tilt_deg", C.c_double), ("sensor_height", C.c_double), ("height_clip_range", C.c_double), ("floor_pts_thresh", C.c_int),
                ("floor_normal_thresh_deg", C.c_double), ("use_normal_filtering", C.c_int), ("normal_filter_thresh_deg", C.c_double)]


class FloorResult(C.Structure):
    """struct mrgfe_floor_result: what detect() returned and why, with the point counts of its stages."""

    _fields_ = [("found", C.c_int32), ("reason", C.c_int32), ("coeffs", C.c_float * 4), ("n_clipped", C.c_uint32), ("n_filtered", C.c_uint32),
                ("n_inliers", C.c_uint32), ("iterations", C.c_int32), ("skipped", C.c_int32), ("reserved", C.c_int32)]


class MatchingStatus(C.Structure):
    """struct mrgfe_matching_status: the fields of mrg_slam_msgs/ScanMatchingStatus that ``publish_scan_matching_status`` fills
    (apps/scan_matching_odometry_component.cpp:391-431); poses are position x y z, orientation x y z w."""

    _fields_ = [("has_converged", C.c_int32), ("n_points", C.c_uint32), ("num_inliers", C.c_uint32), ("inlier_fraction", C.c_float), ("matching_error", C.c_double),
                ("relative_pose", C.c_double * 7), ("prediction_error", C.c_double * 7), ("has_prediction", C.c_int32), ("reserved", C.c_int32)]


class OdomParams(C.Structure):
    """struct mrgfe_odom_params (the scan_matching_odometry_component ROS parameters, config/mrg_slam.yaml:77-95)."""

    _fields_ = [("downsample_method", C.c_int32), ("downsample_resolution", C.c_float), ("downsample_min_points_per_voxel", C.c_int32), ("reserved0", C.c_int32),
                ("keyframe_delta_translation", C.c_double), ("keyframe_delta_angle", C.c_double), ("keyframe_delta_time", C.c_double),
                ("enable_transform_thresholding", C.c_int32), ("max_consecutive_rejections", C.c_int32), ("max_acceptable_translation", C.c_double),
                ("max_acceptable_angle", C.c_double), ("status_max_correspondence_dist", C.c_double)]


class OdomResult(C.Structure):
    """struct mrgfe_odom_result: what one ``mrgfe_odom_frame`` decided and returns (matrices column-major)."""

    _fields_ = [("outcome", C.c_int32), ("new_keyframe", C.c_int32), ("consecutive_rejections", C.c_int32), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("n_source", C.c_uint32), ("odom", C.c_float * 16), ("keyframe_pose", C.c_float * 16), ("trans", C.c_float * 16), ("has_status", C.c_int32),
                ("reserved", C.c_int32), ("status", MatchingStatus)]


class OdomState(C.Structure):
    """struct mrgfe_dbg_odom_state (include/mrgfe_debug.h): everything ``matching()`` keeps between frames."""

    _fields_ = [("has_keyframe", C.c_int32), ("consecutive_rejections", C.c_int32), ("has_prev_time", C.c_int32), ("reserved", C.c_int32), ("keyframe_stamp", C.c_double),
                ("prev_time", C.c_double), ("keyframe_pose", C.c_float * 16), ("prev_trans", C.c_float * 16)]


class LoopParams(C.Structure):
    """struct mrgfe_loop_params (the loop detector's ROS parameters, config/mrg_slam.yaml:169-179)."""

    _fields_ = [("candidate_max_xy_distance", C.c_double), ("accum_distance_thresh_same_robot", C.c_double), ("accum_distance_thresh_other_robot", C.c_double),
                ("fitness_score_max_range", C.c_double), ("fitness_score_thresh", C.c_double), ("loop_closure_consistency_max_delta_trans", C.c_double),
                ("loop_closure_consistency_max_delta_angle", C.c_double), ("fitness_selection", C.c_int32), ("use_planar_registration_guess", C.c_int32),
                ("enable_loop_closure_consistency_check", C.c_int32), ("reserved", C.c_int32)]


class LoopKeyframe(C.Structure):
    """struct mrgfe_loop_keyframe: the slice of KeyFrame ``mrgfe_loop_detect`` reads (matrices column-major)."""

    _fields_ = [("key", C.c_uint64), ("slam_id", C.c_uint64), ("estimate", C.c_double * 16), ("accum_distance", C.c_double), ("first_keyframe", C.c_int32),
                ("static_keyframe", C.c_int32), ("prev_key", C.c_uint64), ("next_key", C.c_uint64), ("prev_relpose", C.c_double * 16), ("next_relpose", C.c_double * 16)]


class LoopResult(C.Structure):
    """struct mrgfe_loop_result: one Loop of ``mrgfe_loop_detect`` (relative_pose column-major)."""

    _fields_ = [("key1", C.c_uint64), ("key2", C.c_uint64), ("relative_pose", C.c_float * 16), ("score", C.c_double)]


ODOM_FIRST_FRAME, ODOM_ACCEPTED, ODOM_NOT_CONVERGED, ODOM_REJECTED, ODOM_REJECTED_RESET = 0, 1, 2, 3, 4  # enum mrgfe_odom_outcome
ODOM_OUTCOMES = ("first_frame", "accepted", "not_converged", "rejected", "rejected_reset")
FLOOR_REASONS = ("found", "empty_input", "none_after_clip", "too_few_filtered", "no_model", "too_few_inliers", "not_vertical")


class InfParams(C.Structure):
    """struct mrgfe_inf_params (InformationMatrixCalculator's ROS parameters, config/mrg_slam.yaml:216-223,173)."""

    _fields_ = [("use_const_inf_matrix", C.c_int), ("const_stddev_x", C.c_double), ("const_stddev_q", C.c_double), ("var_gain_a", C.c_double), ("min_stddev_x", C.c_double),
                ("max_stddev_x", C.c_double), ("min_stddev_q", C.c_double), ("max_stddev_q", C.c_double), ("fitness_score_thresh", C.c_double)]


class RegParams(C.Structure):
    """struct mrgfe_reg_params (mirrors the reg_* ROS parameters of registrations.cpp:34-43)."""

    _fields_ = [
        ("method", C.c_int),
        ("num_threads", C.c_int),
        ("transformation_epsilon", C.c_double),
        ("maximum_iterations", C.c_int),
        ("max_correspondence_distance", C.c_double),
        ("max_optimizer_iterations", C.c_int),
        ("use_reciprocal_correspondences", C.c_int),
        ("correspondence_randomness", C.c_int),
        ("resolution", C.c_double),
        ("nn_search_method", C.c_int),
        ("step_size", C.c_double),
        ("outlier_ratio", C.c_double),
        ("rotation_epsilon", C.c_double),
    ]


class PairResult(C.Structure):
    """struct mrgfe_pair_result: the 384-byte record gathered across ranks."""

    _fields_ = [
        ("T", C.c_float * 16),
        ("H", C.c_double * 36),
        ("fitness", C.c_double),
        ("trans_probability", C.c_double),
        ("converged", C.c_int32),
        ("iterations", C.c_int32),
        ("evaluations", C.c_int32),
        ("pair_id", C.c_int32),
    ]


assert C.sizeof(PairResult) == 384

# every symbol include/mrgfe.h declares: name -> (restype, argtypes)
_vp, _fp, _dp, _ip, _u32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
_szp = C.POINTER(C.c_size_t)
SIGNATURES = {
    "mrgfe_last_error": (C.c_char_p, []),
    "mrgfe_version": (C.c_char_p, []),
    "mrgfe_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mrgfe_ctx_create_priority": (C.c_int, [C.c_int, C.c_int, C.POINTER(_vp)]),
    "mrgfe_ctx_create_reserving": (C.c_int, [C.c_int, C.c_int, C.POINTER(_vp)]),
    "mrgfe_ctx_destroy": (None, [_vp]),
    "mrgfe_ctx_synchronize": (C.c_int, [_vp]),
    "mrgfe_pin_host_buffer": (C.c_int, [_vp, _vp, C.c_size_t]),
    "mrgfe_unpin_host_buffer": (C.c_int, [_vp, _vp]),
    "mrgfe_ctx_set_zero_copy_uploads": (C.c_int, [_vp, C.c_int]),
    "mrgfe_ctx_set_byte_layouts": (C.c_int, [_vp, C.c_int]),
    "mrgfe_ctx_set_bfgs_batches": (C.c_int, [_vp, C.c_int]),
    "mrgfe_ctx_set_ndt_reference_order": (C.c_int, [_vp, C.c_int]),
    "mrgfe_ctx_set_statistical_chains": (C.c_int, [_vp, C.c_int]),
    "mrgfe_ctx_set_wide_statistical_chains": (C.c_int, [_vp, C.c_int]),
    "mrgfe_ctx_sor_grid_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_ctx_stream": (_vp, [_vp]),
    "mrgfe_ctx_fitness_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_ctx_knn_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_ctx_prefilter_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_ingest_pointcloud2": (C.c_int, [_vp, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, _fp, _vp]),
    "mrgfe_reg_default_params": (None, [C.c_int, C.POINTER(RegParams)]),
    "mrgfe_reg_create": (C.c_int, [_vp, C.POINTER(RegParams), C.POINTER(_vp)]),
    "mrgfe_reg_destroy": (None, [_vp]),
    "mrgfe_reg_set_target": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t]),
    "mrgfe_reg_set_source": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t]),
    "mrgfe_reg_set_target_device": (C.c_int, [_vp, _vp, C.c_size_t]),
    "mrgfe_reg_set_source_device": (C.c_int, [_vp, _vp, C.c_size_t]),
    "mrgfe_reg_source_becomes_target": (C.c_int, [_vp]),
    "mrgfe_reg_set_source_from_prefilter": (C.c_int, [_vp, _vp, C.c_size_t]),
    "mrgfe_reg_align": (C.c_int, [_vp, _fp, _fp]),
    "mrgfe_reg_has_converged": (C.c_int, [_vp]),
    "mrgfe_reg_final_transformation": (C.c_int, [_vp, _fp]),
    "mrgfe_reg_fitness": (C.c_int, [_vp, C.c_double, _dp]),
    "mrgfe_reg_nn1_target": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, _ip, _fp]),
    "mrgfe_matching_status_size": (C.c_size_t, []),
    "mrgfe_reg_matching_status": (C.c_int, [_vp, C.c_double, _fp, C.POINTER(MatchingStatus)]),
    "mrgfe_status_poses": (C.c_int, [_fp, _fp, _dp, _dp]),
    "mrgfe_reg_iterations": (C.c_int, [_vp]),
    "mrgfe_reg_evaluations": (C.c_int, [_vp]),
    "mrgfe_reg_trans_probability": (C.c_double, [_vp]),
    "mrgfe_reg_hessian": (C.c_int, [_vp, _dp]),
    "mrgfe_ndt_evaluate": (C.c_int, [_vp, _fp, _dp, C.c_int, _dp, _dp, _dp]),
    "mrgfe_map_store_create": (C.c_int, [_vp, C.POINTER(C.c_void_p)]),
    "mrgfe_map_store_destroy": (None, [_vp]),
    "mrgfe_map_store_add": (C.c_int, [_vp, C.c_uint64, _fp, C.c_size_t, C.c_size_t]),
    "mrgfe_map_store_has": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_size_t)]),
    "mrgfe_map_store_bytes": (C.c_size_t, [_vp]),
    "mrgfe_map_store_generate": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), _dp, C.POINTER(C.c_uint8), C.c_float, C.c_int, C.c_float, C.c_int, _fp, C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "mrgfe_map_publish_default_params": (None, [C.POINTER(MapPublishParams)]),
    "mrgfe_map_publish_params_size": (C.c_size_t, []),
    "mrgfe_map_publish_result_size": (C.c_size_t, []),
    "mrgfe_map_store_publish": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), _dp, C.POINTER(C.c_uint8), C.POINTER(MapPublishParams), _vp, C.c_size_t, C.POINTER(MapPublishResult)]),
    "mrgfe_map_store_publish_device": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), _dp, C.POINTER(C.c_uint8), C.POINTER(MapPublishParams), C.POINTER(_vp),
                                                 C.POINTER(MapPublishResult)]),
    "mrgfe_map_store_read": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), C.c_int, _vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    "mrgfe_map_store_egress_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "mrgfe_keyframe_default_params": (None, [C.POINTER(KeyframeParams)]),
    "mrgfe_keyframe_params_size": (C.c_size_t, []),
    "mrgfe_pointcloud2_field_size": (C.c_size_t, []),
    "mrgfe_pointcloud2_layout": (C.c_int, [C.POINTER(PointField), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(KeyframeParams), C.POINTER(C.c_int)]),
    "mrgfe_keyframe_callback": (C.c_int, [_vp, C.c_uint64, C.POINTER(KeyframeParams), _vp, C.c_size_t, _fp, C.c_int, C.c_float, _fp, _szp, _fp, _szp]),
    "mrgfe_keyframe_callback_device": (C.c_int, [_vp, C.c_uint64, _vp, C.c_size_t, _fp, C.c_int, C.c_float, _fp, _szp, _fp, _szp]),
    "mrgfe_keyframe_callback_records": (C.c_int, [_vp, C.c_uint64, C.POINTER(KeyframeParams), _vp, C.c_size_t, _fp, C.c_int, C.c_float, C.c_int, _vp, C.c_size_t, _szp, _vp,
                                                  C.c_size_t, _szp]),
    "mrgfe_keyframe_callback_records_device": (C.c_int, [_vp, C.c_uint64, _vp, C.c_size_t, _fp, C.c_int, C.c_float, C.c_int, _vp, C.c_size_t, _szp, _vp, C.c_size_t, _szp]),
    "mrgfe_keyframe_msg_size": (C.c_size_t, []),
    "mrgfe_map_store_add_keyframes": (C.c_int, [_vp, C.c_int, C.POINTER(KeyframeMsg), C.POINTER(C.c_uint8)]),
    "mrgfe_graph_edge_size": (C.c_size_t, []),
    "mrgfe_map_store_edges": (C.c_int, [_vp, C.POINTER(InfParams), C.c_int, C.POINTER(GraphEdge), _dp, _dp]),
    "mrgfe_ground_fill_default_params": (None, [C.POINTER(GroundFillParams)]),
    "mrgfe_ground_fill_params_size": (C.c_size_t, []),
    "mrgfe_ground_fill_result_size": (C.c_size_t, []),
    "mrgfe_ground_fill_counts": (C.c_int, [C.POINTER(GroundFillParams), _u32p, _u32p]),
    "mrgfe_fill_ground_plane": (C.c_int, [_vp, C.POINTER(GroundFillParams), _dp, _fp, C.c_size_t, C.c_size_t, _fp, C.c_size_t, C.POINTER(GroundFillResult)]),
    "mrgfe_map_store_fill_ground": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(GroundFillParams), _dp, _fp, C.c_size_t, C.POINTER(GroundFillResult)]),
    "mrgfe_prefilter_default_params": (None, [C.POINTER(PrefilterParams)]),
    "mrgfe_prefilter": (C.c_int, [_vp, C.POINTER(PrefilterParams), _fp, C.c_size_t, C.c_size_t, _fp, C.POINTER(C.c_size_t)]),
    "mrgfe_prefilter_device": (C.c_int, [_vp, C.POINTER(PrefilterParams), _fp, C.c_size_t, C.c_size_t, _vp, C.POINTER(C.c_size_t)]),
    "mrgfe_scan_default_params": (None, [C.POINTER(ScanParams)]),
    "mrgfe_scan_params_size": (C.c_size_t, []),
    "mrgfe_scan_callback": (C.c_int, [_vp, C.POINTER(ScanParams), C.POINTER(C.c_uint8), _fp, C.POINTER(C.c_size_t)]),
    "mrgfe_scan_callback_device": (C.c_int, [_vp, C.POINTER(ScanParams), C.POINTER(C.c_uint8), _vp, C.POINTER(C.c_size_t)]),
    "mrgfe_scan_callback_records": (C.c_int, [_vp, C.POINTER(ScanParams), C.POINTER(C.c_uint8), C.c_int, _vp, C.c_size_t, _vp, C.POINTER(C.c_size_t)]),
    "mrgfe_scan_outputs_size": (C.c_size_t, []),
    "mrgfe_scan_callback_outputs": (C.c_int, [_vp, C.POINTER(ScanParams), C.POINTER(C.c_uint8), C.POINTER(ScanOutputs), _szp, _szp]),
    "mrgfe_prefilter_records": (C.c_int, [_vp, C.POINTER(PrefilterParams), _fp, C.c_size_t, C.c_size_t, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(C.c_size_t)]),
    "mrgfe_cloud_records_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t]),
    "mrgfe_ctx_egress_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "mrgfe_ctx_second_egress_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "mrgfe_floor_default_params": (None, [C.POINTER(FloorParams)]),
    "mrgfe_floor_detect": (C.c_int, [_vp, C.POINTER(FloorParams), _fp, C.c_size_t, C.c_size_t, C.POINTER(FloorResult), _fp, _fp]),
    "mrgfe_floor_detect_device": (C.c_int, [_vp, C.POINTER(FloorParams), _vp, C.c_size_t, C.POINTER(FloorResult), _fp, _fp]),
    "mrgfe_floor_callback": (C.c_int, [_vp, C.POINTER(FloorParams), C.POINTER(KeyframeParams), _vp, C.c_size_t, C.POINTER(FloorResult), _fp, _fp]),
    "mrgfe_knn": (C.c_int, [_vp, _fp, C.c_size_t, _fp, C.c_size_t, C.c_size_t, C.c_int, _ip, _fp]),
    "mrgfe_pclgicp_evaluate": (C.c_int, [_vp, _fp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    "mrgfe_gicp_linearize": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _ip]),
    "mrgfe_gicp_error": (C.c_int, [_vp, _dp, _dp, _ip]),
    "mrgfe_gicp_covariances": (C.c_int, [_vp, C.c_int, _dp]),
    "mrgfe_ndt_num_leaves": (C.c_int, [_vp]),
    "mrgfe_ndt_grid": (C.c_int, [_vp, _ip, _ip, _ip]),
    "mrgfe_ndt_leaves": (C.c_int, [_vp, _ip, _ip, _dp, _dp]),
    "mrgfe_ndt_mean_neighbours": (C.c_double, [_vp]),
    "mrgfe_distance_filter": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_double, C.c_double, _fp, _szp]),
    "mrgfe_voxelgrid": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_float, C.c_int, _fp, _szp, C.POINTER(C.c_int)]),
    "mrgfe_approx_voxelgrid": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_float, _fp, _szp]),
    "mrgfe_radius_outlier": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_double, C.c_int, _fp, _szp]),
    "mrgfe_statistical_outlier": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_int, C.c_double, _fp, _szp]),
    "mrgfe_calc_fitness_score": (C.c_int, [_vp, _fp, C.c_size_t, _fp, C.c_size_t, C.c_size_t, _dp, C.c_double, _dp]),
    "mrgfe_inf_default_params": (None, [C.POINTER(InfParams)]),
    "mrgfe_inf_weight": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "mrgfe_inf_matrix_from_fitness": (C.c_int, [C.POINTER(InfParams), C.c_double, _dp]),
    "mrgfe_calc_information_matrix": (C.c_int, [_vp, C.POINTER(InfParams), _fp, C.c_size_t, _fp, C.c_size_t, C.c_size_t, _dp, _dp, _dp]),
    "mrgfe_map_store_fitness": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _dp, C.c_double, _dp]),
    "mrgfe_map_store_information_matrix": (C.c_int, [_vp, C.POINTER(InfParams), C.c_uint64, C.c_uint64, _dp, _dp, _dp]),
    "mrgfe_map_cloud_generate": (C.c_int, [_vp, C.c_int, C.POINTER(_fp), _szp, C.c_size_t, _dp, C.POINTER(C.c_uint8), C.c_float, C.c_int, C.c_float, C.c_int, _fp,
                                           C.c_size_t, _szp]),
    "mrgfe_remove_points_near": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, _fp, C.c_int, C.c_float, _fp, _szp, _fp, _szp]),
    "mrgfe_deskew": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, _fp, C.c_double, _fp]),
    "mrgfe_transform_cloud": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, _fp, _fp]),
    "mrgfe_odom_default_params": (None, [C.POINTER(OdomParams)]),
    "mrgfe_odom_params_size": (C.c_size_t, []),
    "mrgfe_odom_result_size": (C.c_size_t, []),
    "mrgfe_odom_create": (C.c_int, [_vp, C.POINTER(OdomParams), C.POINTER(_vp)]),
    "mrgfe_odom_destroy": (None, [_vp]),
    "mrgfe_odom_reset": (C.c_int, [_vp]),
    "mrgfe_odom_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "mrgfe_odom_frame": (C.c_int, [_vp, C.POINTER(KeyframeParams), _vp, C.c_size_t, C.c_double, _fp, C.c_int, _fp, C.POINTER(OdomResult)]),
    "mrgfe_odom_frame_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_double, _fp, C.c_int, _fp, C.POINTER(OdomResult)]),
    "mrgfe_odom_frame_records": (C.c_int, [_vp, C.POINTER(KeyframeParams), _vp, C.c_size_t, C.c_double, _fp, C.c_int, C.c_int, _vp, C.c_size_t, _szp, C.POINTER(OdomResult)]),
    "mrgfe_odom_frame_records_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_double, _fp, C.c_int, C.c_int, _vp, C.c_size_t, _szp, C.POINTER(OdomResult)]),
    "mrgfe_batch_create": (C.c_int, [_vp, C.POINTER(RegParams), C.POINTER(_vp)]),
    "mrgfe_batch_destroy": (None, [_vp]),
    "mrgfe_batch_clear": (C.c_int, [_vp]),
    "mrgfe_batch_clear_pairs": (C.c_int, [_vp]),
    "mrgfe_batch_add_target": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t]),
    "mrgfe_batch_add_target_device": (C.c_int, [_vp, _vp, C.c_size_t]),
    "mrgfe_batch_add_pair": (C.c_int, [_vp, C.c_int, _fp, C.c_size_t, C.c_size_t, _fp]),
    "mrgfe_batch_add_pair_device": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _fp]),
    "mrgfe_batch_add_device": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_void_p), _szp, C.c_int, _ip, C.POINTER(C.c_void_p), _szp, _fp]),
    "mrgfe_batch_add_pair_keyed": (C.c_int, [_vp, C.c_int, C.c_uint64, _fp, C.c_size_t, C.c_size_t, _fp]),
    "mrgfe_batch_has_cloud": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_size_t)]),
    "mrgfe_batch_store_bytes": (C.c_size_t, [_vp]),
    "mrgfe_batch_forget": (C.c_int, [_vp, C.c_uint64]),
    "mrgfe_batch_add_target_from_store": (C.c_int, [_vp, _vp, C.c_uint64]),
    "mrgfe_batch_add_pair_from_store": (C.c_int, [_vp, C.c_int, _vp, C.c_uint64, _fp]),
    "mrgfe_batch_set_guess": (C.c_int, [_vp, C.c_int, _fp]),
    "mrgfe_batch_build_targets": (C.c_int, [_vp]),
    "mrgfe_batch_align": (C.c_int, [_vp, C.c_double, C.POINTER(PairResult)]),
    "mrgfe_batch_align_async": (C.c_int, [_vp, C.c_double, C.POINTER(PairResult)]),
    "mrgfe_batch_wait": (C.c_int, [_vp]),
    "mrgfe_batch_num_pairs": (C.c_int, [_vp]),
    "mrgfe_batch_fitness_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_batch_align_best": (C.c_int, [_vp, C.c_double, C.c_double, _ip, C.c_int, C.POINTER(PairResult), _ip, _ip, _dp]),
    "mrgfe_batch_select_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_batch_align_best_async": (C.c_int, [_vp, C.c_double, C.c_double, _ip, C.c_int, C.POINTER(PairResult), _ip, _ip, _dp]),
    "mrgfe_batch_kernel_stats": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_int64), _dp]),
    "mrgfe_reg_kernel_stats": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_int64), _dp]),
    "mrgfe_batch_pair_counts": (C.c_int, [_vp, C.c_int, _dp, _dp]),
    "mrgfe_batch_largest_launch": (C.c_int, [_vp, _dp]),
    "mrgfe_node_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(RegParams), C.POINTER(_vp)]),
    "mrgfe_node_destroy": (None, [_vp]),
    "mrgfe_node_num_members": (C.c_int, [_vp]),
    "mrgfe_node_clear": (C.c_int, [_vp]),
    "mrgfe_node_add_target": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t]),
    "mrgfe_node_add_target_keyed": (C.c_int, [_vp, C.c_uint64, _fp, C.c_size_t, C.c_size_t]),
    "mrgfe_node_add_pair": (C.c_int, [_vp, C.c_int, _fp, C.c_size_t, C.c_size_t, _fp]),
    "mrgfe_node_add_pair_keyed": (C.c_int, [_vp, C.c_int, C.c_uint64, _fp, C.c_size_t, C.c_size_t, _fp]),
    "mrgfe_node_num_pairs": (C.c_int, [_vp]),
    "mrgfe_node_add_target_from_store": (C.c_int, [_vp, _vp, C.c_uint64]),
    "mrgfe_node_add_pair_from_store": (C.c_int, [_vp, C.c_int, _vp, C.c_uint64, _fp]),
    "mrgfe_node_clear_pairs": (C.c_int, [_vp]),
    "mrgfe_node_store_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "mrgfe_node_align": (C.c_int, [_vp, C.c_double, C.POINTER(PairResult)]),
    "mrgfe_node_align_best": (C.c_int, [_vp, C.c_double, C.c_double, _ip, C.c_int, C.POINTER(PairResult), _ip, _ip, _dp]),
    "mrgfe_node_select_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_node_shard": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mrgfe_node_last_gather": (C.c_int, [_vp]),
    "mrgfe_node_forget": (C.c_int, [_vp, C.c_uint64]),
    "mrgfe_node_store_bytes": (C.c_size_t, [_vp]),
    "mrgfe_node_select_best": (C.c_int, [C.POINTER(PairResult), C.c_int, _ip, _ip, _dp]),
    "mrgfe_batch_rounds": (C.c_int, [_vp]),
    "mrgfe_batch_timing": (C.c_int, [_vp, _dp]),
    "mrgfe_batch_timing_reset": (C.c_int, [_vp]),
    "mrgfe_loop_default_params": (None, [C.POINTER(LoopParams)]),
    "mrgfe_loop_params_size": (C.c_size_t, []),
    "mrgfe_loop_keyframe_size": (C.c_size_t, []),
    "mrgfe_loop_result_size": (C.c_size_t, []),
    "mrgfe_loop_create": (C.c_int, [_vp, _vp, C.POINTER(LoopParams), C.POINTER(_vp)]),
    "mrgfe_loop_create_node": (C.c_int, [_vp, _vp, C.POINTER(LoopParams), C.POINTER(_vp)]),
    "mrgfe_loop_destroy": (None, [_vp]),
    "mrgfe_loop_reset": (C.c_int, [_vp]),
    "mrgfe_loop_detect": (C.c_int, [_vp, C.c_int, C.POINTER(LoopKeyframe), C.c_int, C.POINTER(LoopKeyframe), C.c_int, C.POINTER(C.c_uint64), C.POINTER(LoopResult), C.c_int,
                                    C.POINTER(C.c_int)]),
    "mrgfe_loop_stats": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "mrgfe_loop_timing": (C.c_int, [_vp, C.c_int, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "mrgfe_loop_normalize_estimate": (C.c_int, [_dp, _dp]),
    "mrgfe_loop_guess": (C.c_int, [_dp, _dp, C.c_int, _fp]),
}
# mrgfe_dbg_loop_aligner (include/mrgfe_debug.h): the callback that stands in for both stages' GPU batches
LOOP_ALIGNER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, _ip, C.POINTER(C.c_uint64), _fp, C.c_int, C.POINTER(PairResult))

# include/mrgfe_debug.h: diagnostic entry points (exported by the shipped library) ...
DEBUG_SIGNATURES = {
    "mrgfe_dbg_set_gicp_corr_passes": (C.c_int, [C.c_int]),
    "mrgfe_dbg_grid_set_query": (C.c_int, [_vp, C.POINTER(_fp), C.POINTER(C.c_size_t), C.c_int, _fp, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int32), _fp]),
    "mrgfe_dbg_sort_pairs": (C.c_int, [_vp, _u32p, _u32p, C.c_size_t, C.c_int, _u32p, _u32p]),
    "mrgfe_dbg_wave_sums": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp]),
    "mrgfe_dbg_exclusive_scan": (C.c_int, [_vp, _u32p, C.c_size_t, _u32p, _u32p]),
    "mrgfe_dbg_minmax": (C.c_int, [_vp, _fp, C.c_size_t, _fp, _fp, _u32p]),
    "mrgfe_dbg_set_host_control": (C.c_int, [C.c_int]),
    "mrgfe_dbg_set_fused_launch": (C.c_int, [C.c_int]),
    "mrgfe_dbg_set_ndt_reference_order": (C.c_int, [C.c_int]),
    "mrgfe_dbg_ndt_evaluate_ppt": (C.c_int, [_vp, _fp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "mrgfe_dbg_ndt_eval_neighbours": (C.c_int, [_vp, _dp]),
    "mrgfe_dbg_set_ndt_round_shape": (C.c_int, [C.c_int, C.c_int]),
    "mrgfe_dbg_reg_ndt_rounds": (C.c_int, [_vp, C.c_int, _u32p, _u32p]),
    "mrgfe_dbg_batch_ndt_rounds": (C.c_int, [_vp, C.c_int, _u32p, _u32p]),
    "mrgfe_dbg_node_ndt_rounds": (C.c_int, [_vp, C.c_int, C.c_int, _u32p, _u32p]),
    "mrgfe_dbg_set_fit_sweep": (C.c_int, [C.c_int]),
    "mrgfe_dbg_set_prefilter_device_driven": (C.c_int, [C.c_int]),
    "mrgfe_dbg_set_sor_grid_rule": (C.c_int, [C.c_float, C.c_double, C.c_int]),
    "mrgfe_dbg_prefilter_output": (C.c_int, [_vp, _ip, _szp, _fp]),
    "mrgfe_dbg_ctx_create_detached": (C.c_int, [C.POINTER(_vp)]),
    "mrgfe_dbg_wide_statistical_chains": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mrgfe_dbg_sor_threshold": (C.c_int, [_vp, _fp, _u32p, C.c_size_t, C.c_double, C.c_int, _dp]),
    "mrgfe_dbg_floor_ransac": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(C.c_int), _fp, _ip, _szp, _ip, _ip]),
    "mrgfe_dbg_floor_normals": (C.c_int, [_vp, _fp, C.c_size_t, C.c_size_t, C.c_double, _fp, C.POINTER(C.c_uint8)]),
    "mrgfe_dbg_floor_stats": (C.c_int, [_vp, _dp]),
    "mrgfe_dbg_set_pclgicp_reference_order": (C.c_int, [C.c_int]),
    "mrgfe_dbg_set_fit_stats": (C.c_int, [C.c_int]),
    "mrgfe_dbg_sincosf": (None, [_fp, C.c_size_t, _fp, _fp]),
    "mrgfe_dbg_exp": (C.c_int, [_vp, _dp, C.c_size_t, C.c_int, _dp]),
    "mrgfe_dbg_exp_float_args": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), _u32p, C.POINTER(C.c_uint64)]),
    "mrgfe_dbg_ctl_math": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _fp, _dp, _dp]),
    "mrgfe_dbg_ctl_create": (C.c_int, [C.POINTER(RegParams), _fp, C.c_uint32, C.POINTER(_vp)]),
    "mrgfe_dbg_ctl_destroy": (None, [_vp]),
    "mrgfe_dbg_ctl_request": (C.c_int, [_vp, C.POINTER(C.c_int), _fp, _dp]),
    "mrgfe_dbg_ctl_result": (C.c_int, [_vp, C.c_double, _dp, _dp, C.c_double]),
    "mrgfe_dbg_ctl_final": (C.c_int, [_vp, _fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mrgfe_dbg_ctl_record": (C.c_int, [_vp, _dp, _dp]),
    "mrgfe_dbg_icp_ctl_create": (C.c_int, [C.POINTER(RegParams), _fp, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "mrgfe_dbg_icp_ctl_destroy": (None, [_vp]),
    "mrgfe_dbg_icp_ctl_result": (C.c_int, [_vp, _dp, C.POINTER(C.c_int), _fp]),
    "mrgfe_dbg_icp_ctl_final": (C.c_int, [_vp, _fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mrgfe_dbg_batch_fit_bounds": (C.c_int, [_vp, _dp, _dp]),
    "mrgfe_dbg_node_fit_bounds": (C.c_int, [_vp, _dp, _dp]),
    "mrgfe_dbg_select_prune": (C.c_int, [C.c_int, _dp, _dp, _ip, _ip, C.c_int, C.c_double, _ip]),
    "mrgfe_dbg_odom_ctl_create": (C.c_int, [C.POINTER(OdomParams), C.POINTER(_vp)]),
    "mrgfe_dbg_odom_ctl_destroy": (None, [_vp]),
    "mrgfe_dbg_odom_ctl_begin": (C.c_int, [_vp, C.c_double, _fp, C.POINTER(C.c_int), _fp]),
    "mrgfe_dbg_odom_ctl_end": (C.c_int, [_vp, C.c_int, _fp, C.POINTER(OdomResult)]),
    "mrgfe_dbg_odom_ctl_state": (C.c_int, [_vp, C.POINTER(OdomState)]),
    "mrgfe_dbg_odom_state_of": (C.c_int, [_vp, C.POINTER(OdomState)]),
    "mrgfe_dbg_odom_source": (C.c_int, [_vp, _fp, _szp, _fp, _u32p]),
    "mrgfe_dbg_loop_set_aligner": (C.c_int, [_vp, _vp, _vp]),  # (the callback goes in as ctypes.cast(LOOP_ALIGNER(fn), c_void_p); NULL: the GPU batches again)
    "mrgfe_dbg_loop_set_stage_reuse": (C.c_int, [_vp, C.c_int]),
    "mrgfe_dbg_node_set_store_copy": (C.c_int, [_vp, C.c_int]),
    "mrgfe_dbg_loop_manager": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
}
# ... and its fault injectors and their allocation count, which exist only in the -DMRGFE_TESTING build (libmrgfe_testing.so: tests/faultinject/ runs under MRGFE_LIB=that file)
TESTING_SIGNATURES = {
    "mrgfe_dbg_node_fail_member": (C.c_int, [_vp, C.c_int]),
    "mrgfe_dbg_fail_alloc_after": (C.c_long, [C.c_long]),
    "mrgfe_dbg_live_allocations": (C.c_long, []),
}
TESTING_LIB_PATH = os.path.join(_PKG, "libmrgfe_testing.so")


def build(force: bool = False) -> str:
    """Compile libmrgfe.so for gfx950 with hipcc (csrc/Makefile). No-op when it is newer than its sources."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".cpp", ".h")) or f == "Makefile"]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "mrgfe.h"))
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "mrgfe_debug.h"))
    default_lib = os.path.join(_PKG, "libmrgfe.so")
    outs = [default_lib, TESTING_LIB_PATH]  # (make builds both: the shipped library and the -DMRGFE_TESTING variant)
    stale = force or any(not os.path.exists(o) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs) for o in outs)
    if stale:
        subprocess.run(["make", "-C", _CSRC, "-j8", "-s"] + (["-B"] if force else []), check=True)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            try:
                build()
            except Exception as e:  # noqa: BLE001
                raise RuntimeError(f"libmrgfe.so is missing and could not be built with hipcc ({e}); there is no CPU fallback") from e
        # A process that uses both this library and PyTorch must bind them to ONE HIP runtime, and that only works out
        # when torch's bundled runtime (same soname) is loaded first: loaded after libmrgfe, torch reports "No HIP GPUs are
        # available".  So import torch here if it is installed (MRGFE_NO_TORCH=1 skips this for torch-free programs).
        if "torch" not in sys.modules and os.environ.get("MRGFE_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401
            except Exception:  # noqa: BLE001
                pass
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if "torch" in sys.modules else C.DEFAULT_MODE)
        for name, (res, args) in {**SIGNATURES, **DEBUG_SIGNATURES}.items():
            if os.environ.get("MRGFE_LIB") and os.environ.get("MRGFE_LIB_ALLOW_MISSING") and not hasattr(L, name):
                continue  # an OLDER library file in an A/B measurement (MRGFE_LIB): symbols added since are simply not there
            f = getattr(L, name)  # AttributeError here == the library does not export a declared symbol
            f.restype, f.argtypes = res, args
        for name, (res, args) in TESTING_SIGNATURES.items():  # only the testing variant has them
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = res, args
        if hasattr(L, "mrgfe_matching_status_size") and L.mrgfe_matching_status_size() != C.sizeof(MatchingStatus):
            raise RuntimeError(f"libmrgfe.so was built with a mrgfe_matching_status of {L.mrgfe_matching_status_size()} bytes, the binding mirrors {C.sizeof(MatchingStatus)}")
        if hasattr(L, "mrgfe_keyframe_params_size") and L.mrgfe_keyframe_params_size() != C.sizeof(KeyframeParams):
            raise RuntimeError(f"libmrgfe.so was built with a mrgfe_keyframe_params of {L.mrgfe_keyframe_params_size()} bytes, the binding mirrors {C.sizeof(KeyframeParams)}")
        for fn, mirror in (("mrgfe_pointcloud2_field_size", PointField), ("mrgfe_keyframe_msg_size", KeyframeMsg), ("mrgfe_graph_edge_size", GraphEdge), ("mrgfe_odom_params_size", OdomParams),
                           ("mrgfe_odom_result_size", OdomResult), ("mrgfe_loop_params_size", LoopParams), ("mrgfe_loop_keyframe_size", LoopKeyframe),
                           ("mrgfe_loop_result_size", LoopResult), ("mrgfe_ground_fill_params_size", GroundFillParams), ("mrgfe_ground_fill_result_size", GroundFillResult),
                           ("mrgfe_map_publish_params_size", MapPublishParams), ("mrgfe_map_publish_result_size", MapPublishResult),
                           ("mrgfe_scan_outputs_size", ScanOutputs)):
            if hasattr(L, fn) and getattr(L, fn)() != C.sizeof(mirror):
                raise RuntimeError(f"libmrgfe.so was built with a {fn[:-5]} of {getattr(L, fn)()} bytes, the binding mirrors {C.sizeof(mirror)}")
        _lib = L
    return _lib


def last_error() -> str:
    return lib().mrgfe_last_error().decode("utf-8", "replace")


def check(status: int) -> int:
    if status < 0:
        raise MrgfeError(status, last_error())
    return status


class Context:
    """mrgfe_ctx: one per (process, GPU)."""

    def __init__(self, device: int = 0, high_priority: bool = False, reserve_cus: int = 0):
        """``high_priority``: the context's stream gets the device's highest stream priority (odometry next to loop-closure batches).
        ``reserve_cus`` > 0: the kernels of this context never occupy that many of the device's compute units (``mrgfe_ctx_create_reserving``:
        the loop-closure batches' context, so that the odometry contexts' small launches always find free compute units)."""
        self._h = _vp()
        if reserve_cus:
            check(lib().mrgfe_ctx_create_reserving(device, int(reserve_cus), C.byref(self._h)))
        else:
            check(lib().mrgfe_ctx_create_priority(device, int(bool(high_priority)), C.byref(self._h)))
        self.device = device

    def synchronize(self):
        check(lib().mrgfe_ctx_synchronize(self._h))

    def set_zero_copy_uploads(self, on: bool = True):
        """``mrgfe_ctx_set_zero_copy_uploads``: clouds in page-locked host memory go up by DMA from the caller's buffer — which must then stay
        unchanged until the consuming call (align / wait / synchronize) has returned."""
        check(lib().mrgfe_ctx_set_zero_copy_uploads(self._h, int(bool(on))))

    def set_byte_layouts(self, on: bool = True):
        """``mrgfe_ctx_set_byte_layouts``: the calls that read PointCloud2 bytes on this context (and on the stores and registrations made on it) take
        layouts whose field offsets or steps are not multiples of 4 — Velodyne's 22-byte records — as ``pcl::fromROSMsg`` does."""
        check(lib().mrgfe_ctx_set_byte_layouts(self._h, int(bool(on))))

    def set_bfgs_batches(self, on: bool = True):
        """``mrgfe_ctx_set_bfgs_batches``: ``BatchMatcher`` on this context takes PCL_GICP_HIP and PCL_GICP_OMP_HIP (the candidates' BFGS loops in lock
        step, records bit-identical to :class:`PclGicpHip`).  Off, the default, such a batch is refused as it always was."""
        check(lib().mrgfe_ctx_set_bfgs_batches(self._h, int(bool(on))))

    def set_ndt_reference_order(self, on: bool = True):
        """``mrgfe_ctx_set_ndt_reference_order``: :class:`NdtHip` and :class:`PclNdtHip` registrations, ``evaluate`` calls and batches on this context add
        their sums in the reference's own order (host-stepped record + chain kernels; a full-size alignment takes 75 ms for NDT_HIP and about a second for
        PCL_NDT_HIP instead of a millisecond or two: a verification mode): bit-identical to the reference-order oracles.
        Read when an alignment or evaluation starts.  Off, the default, nothing changes."""
        check(lib().mrgfe_ctx_set_ndt_reference_order(self._h, int(bool(on))))

    def set_statistical_chains(self, on: bool = True):
        """``mrgfe_ctx_set_statistical_chains``: the prefilter chains NONE -> STATISTICAL and APPROX_VOXELGRID -> STATISTICAL on this context wait for the
        device once (route 1), the k-NN grid's cell edge chosen on the device; off, the default, they run the host-driven passes.  Same output."""
        check(lib().mrgfe_ctx_set_statistical_chains(self._h, int(bool(on))))

    def set_wide_statistical_chains(self, on: bool = True):
        """``mrgfe_ctx_set_wide_statistical_chains``: STATISTICAL chains with ``statistical_mean_k`` 64..255 on this context are served where 1..63 is
        (behind VOXELGRID; behind NONE / APPROX_VOXELGRID with :meth:`set_statistical_chains` too): one device wait (route 1) and no neighbour rows;
        off, the default, they run the host-driven passes.  Same output."""
        check(lib().mrgfe_ctx_set_wide_statistical_chains(self._h, int(bool(on))))

    def sor_grid_stats(self) -> dict:
        """The statistical filter's k-NN grid of the last prefilter chain call on this context (``mrgfe_ctx_sor_grid_stats``): ``sized`` the device chose
        its edge, ``start_edge``, ``edge`` = start_edge * 2^-halvings, ``halvings``, ``crowding`` last measured, ``cells`` of the built grid."""
        v = (C.c_double * 6)()
        check(lib().mrgfe_ctx_sor_grid_stats(self._h, v))
        return {"sized": bool(v[0]), "start_edge": float(v[1]), "edge": float(v[2]), "halvings": int(v[3]), "crowding": float(v[4]), "cells": int(v[5])}

    def fitness_stats(self) -> dict:
        """What the last getFitnessScore pass on this context did (``mrgfe_ctx_fitness_stats``)."""
        v = (C.c_double * 11)()
        check(lib().mrgfe_ctx_fitness_stats(self._h, v))
        keys = ("ms_block", "ms_sweep", "ms_far", "queries", "queued", "queued_far", "words", "boxes_tested", "cells", "points", "calls")
        return dict(zip(keys, [float(x) for x in v]))

    def knn_stats(self) -> dict:
        """The last exact k-NN launch on this context (``mrgfe_ctx_knn_stats``)."""
        v = (C.c_double * 5)()
        check(lib().mrgfe_ctx_knn_stats(self._h, v))
        return dict(zip(("ms", "queries", "k", "candidates", "launches"), [float(x) for x in v]))

    def prefilter_stats(self) -> dict:
        """Which route served the last prefilter chain call on this context (``mrgfe_ctx_prefilter_stats``): ``route`` 0 host-driven, 1 device-driven,
        2 device-driven attempted and handed back; ``anomaly`` the device-driven chain's word (``PF_ANOMALY_*``); ``counts`` its five stage counts."""
        v = (C.c_double * 10)()
        check(lib().mrgfe_ctx_prefilter_stats(self._h, v))
        return {"route": int(v[0]), "anomaly": int(v[1]), "counts": [int(x) for x in v[2:7]], "points_out": int(v[7]), "calls": int(v[8]), "served": int(v[9])}

    def egress_stats(self) -> dict:
        """The record stage of the last ``scan_callback_records`` / ``prefilter_records`` / ``cloud_records_from_device`` on this context
        (``mrgfe_ctx_egress_stats``): ``direct`` the kernel wrote the caller's page-locked buffer, ``launches`` of the record stage, ``waits`` beyond the
        chain's own (0 on the one-wait route), ``bytes`` of records that reached the host, ``copied`` of them by the host, ``calls`` so far."""
        v = (C.c_int64 * 6)()
        check(lib().mrgfe_ctx_egress_stats(self._h, v))
        return {"direct": bool(v[0]), "launches": int(v[1]), "waits": int(v[2]), "bytes": int(v[3]), "copied": int(v[4]), "calls": int(v[5])}

    def second_egress_stats(self) -> dict:
        """The same for the SECOND record sink of the last call on this context that had one (``mrgfe_ctx_second_egress_stats``): the coloured cloud of
        ``scan_callback_outputs``, the removed cloud of the keyframe callback's record form."""
        v = (C.c_int64 * 6)()
        check(lib().mrgfe_ctx_second_egress_stats(self._h, v))
        return {"direct": bool(v[0]), "launches": int(v[1]), "waits": int(v[2]), "bytes": int(v[3]), "copied": int(v[4]), "calls": int(v[5])}

    def close(self):
        if getattr(self, "_h", None):
            lib().mrgfe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_default_ctx: dict[int, Context] = {}


def default_context(device: int | None = None) -> Context:
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("MRGFE_DEVICE") is None else int(os.environ["MRGFE_DEVICE"])
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
