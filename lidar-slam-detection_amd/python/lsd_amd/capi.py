"""ctypes binding of liblio_hip.so (include/lio_hip.h) -- the MI355X-native LIO scan-matching core.

There is no CPU fallback: importing this module without the built library raises, and every handle
constructor raises when no HIP device is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# the application's job (the library does not touch the environment): HIP's hardware-queue count, read by the runtime at its first call.  With the
# default of 4 the rounds in flight of lio_batch share queues and mostly serialise; lio_batch_create notes a lower value in lio_last_warning
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
LIB_PATH = os.environ.get("LIO_HIP_LIB") or os.path.join(_HERE, "liblio_hip.so")  # LIO_HIP_LIB: a variant build (tools/experiments)

LIO_OK, LIO_E_INVALID, LIO_E_CAPACITY, LIO_E_DEVICE, LIO_E_STATE = 0, -1, -2, -3, -4
MAIN_FIRST_SCAN, MAIN_SEEDED, MAIN_SKIPPED, MAIN_UPDATED, MAIN_IMU_INIT, MAIN_IDLE = 0, 1, 2, 3, 4, 5  # lio_fastlio_main

# every symbol include/lio_hip.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "lio_last_warning",
    "lio_last_error", "lio_device_count", "lio_map_bytes",
    "lio_map_create", "lio_map_destroy", "lio_map_set_lru", "lio_map_lru_stats", "lio_map_lru_exact_stats", "lio_map_set_tie_mode", "lio_map_tie_stats", "lio_map_clear", "lio_map_pool_stats", "lio_map_set_stencil", "lio_map_insert", "lio_map_insert_device", "lio_map_stats",
    "lio_abi_version", "lio_pinned_alloc", "lio_pinned_free",
    "lio_map_dump", "lio_map_knn", "lio_map_knn_candidates", "lio_map_knn_touched", "lio_map_knn_unique",
    "lio_scan_create", "lio_scan_destroy", "lio_scan_reset", "lio_scan_upload", "lio_scan_set_device", "lio_scan_undistort_delta", "lio_scan_undistort_poses", "lio_scan_undistort_imu", "lio_scan_download_raw", "lio_scan_voxel_downsample", "lio_scan_voxel_downsample_batch", "lio_scan_set_ds",
    "lio_scan_num_ds", "lio_scan_download_ds", "lio_scan_download_world", "lio_scan_download_match",
    "lio_p2plane_linearize", "lio_scan_set_degeneracy_mode", "lio_p2plane_degeneracy", "lio_engine_set_reduce_hook", "lio_p2plane_rows", "lio_map_incremental", "lio_map_seed",
    "lio_engine_create", "lio_engine_create_shared", "lio_engine_destroy", "lio_engine_map", "lio_engine_scan", "lio_engine_set_state", "lio_engine_get_state",
    "lio_engine_set_cov", "lio_engine_get_cov", "lio_engine_set_flags", "lio_engine_travel", "lio_engine_is_degenerate",
    "lio_engine_update", "lio_engine_pass_log", "lio_engine_process_scan", "lio_engine_process_scan_device", "lio_engine_timings", "lio_engine_flush",
    "lio_engine_enable_timing", "lio_comm_unique_id", "lio_comm_init", "lio_comm_destroy", "lio_comm_rank", "lio_comm_world", "lio_allgather_normal_eq", "lio_comm_stats", "lio_engine_set_joint", "lio_engine_joint_register", "lio_engine_joint_register_device", "lio_allgather_records", "lio_engines_process_batch", "lio_batch_create", "lio_batch_create_joint", "lio_batch_create_sequences", "lio_batch_sequences_step", "lio_batch_fastlio_main", "lio_batch_set_gather_hook", "lio_batch_exchange_stats", "lio_batch_destroy", "lio_batch_process", "lio_batch_engine", "lio_batch_enable_kernel_timing", "lio_batch_kernel_times", "lio_engine_set_static_map", "lio_scan_enable_kernel_timing", "lio_scan_kernel_times",
    "lio_state_boxplus", "lio_state_boxminus",
    "lio_localmap_create", "lio_localmap_destroy", "lio_localmap_add_keyframe", "lio_localmap_num_keyframes", "lio_localmap_update",
    "lio_localmap_download",
    "lio_localmap_nearest", "lio_localmap_gather", "lio_localmap_z_mean", "lio_localmap_download_gather", "lio_localmap_gather_device", "lio_localmap_store_frame",
    "lio_localmap_frame", "lio_estimate_matcher_params", "lio_localmap_estimate_pose", "lio_scan_ds_device", "lio_gicp_set_target_device", "lio_gicp_set_source_device",
    "lio_cloud_create", "lio_cloud_destroy", "lio_cloud_clear", "lio_cloud_size", "lio_cloud_append_scan", "lio_cloud_append_host",
    "lio_cloud_voxel_downsample", "lio_cloud_download", "lio_cloud_scratch_bytes", "lio_cloud_last_times",
    "lio_knn_index_create", "lio_knn_index_destroy", "lio_knn_index_build", "lio_knn_index_query", "lio_knn_index_colour", "lio_knn_index_last_times",
    "lio_ground_default_params", "lio_ground_draw", "lio_ground_create", "lio_ground_destroy", "lio_ground_detect_scan", "lio_ground_detect_host",
    "lio_ground_download_indices", "lio_ground_download_normals", "lio_ground_download_inliers", "lio_ground_download_draws", "lio_ground_last_run",
    "lio_ground_last_times",
    "lio_bev_create", "lio_bev_destroy", "lio_bev_preprocess_host", "lio_bev_preprocess_cloud", "lio_bev_upload_pixels", "lio_bev_convert", "lio_bev_get_info",
    "lio_bev_download_pixel_coords", "lio_bev_download_kept", "lio_bev_download_pixels", "lio_bev_download_nodes", "lio_bev_download_equalised",
    "lio_bev_download_image", "lio_bev_grey_table", "lio_bev_last_times",
    "lio_keyframe_decide", "lio_keyframer_default_params", "lio_keyframer_create", "lio_keyframer_destroy", "lio_keyframer_reset", "lio_keyframer_push_host",
    "lio_keyframer_pending", "lio_keyframer_pop", "lio_radius_outlier_host", "lio_keyframe_filter_host", "lio_keyframer_fitness_host",
    "lio_keyframer_append_local_map_host", "lio_keyframer_download_local_map", "lio_keyframer_last_times",
    "lio_pose_estimator_create", "lio_pose_estimator_destroy", "lio_pose_estimator_predict", "lio_pose_estimator_match", "lio_pose_estimator_match_gps", "lio_pose_estimator_guess", "lio_pose_estimator_observe",
    "lio_pose_estimator_match_gps_only", "lio_pose_estimator_get_timed_pose", "lio_pose_estimator_predict_nostate",
    "lio_pose_estimator_correct", "lio_pose_estimator_get_dt", "lio_pose_estimator_get", "lio_pose_estimator_set", "lio_pose_estimator_matrix",
    "lio_fastlio_init", "lio_fastlio_is_init", "lio_fastlio_imu_enqueue", "lio_engine_set_device_loop", "lio_fastlio_ins_enqueue", "lio_fastlio_set_wheelspeed", "lio_fastlio_pcl_enqueue", "lio_fastlio_pcl_enqueue_device", "lio_fastlio_pcl_stage", "lio_fastlio_pcl_commit",
    "lio_fastlio_main", "lio_fastlio_odometry", "lio_fastlio_state", "lio_fastlio_start_state", "lio_fastlio_download_undistorted",
    "lio_state_predict", "lio_eskf_update_cb", "lio_eskf_update_ws_cb", "lio_eskf_update_sums_cb",
    "lio_ndt_create", "lio_ndt_destroy", "lio_ndt_set_target", "lio_ndt_set_target_device", "lio_ndt_num_voxels", "lio_ndt_fitness_score", "lio_ndt_overlap_score", "lio_ndt_voxel_at",
    "lio_ndt_linearize", "lio_ndt_default_params", "lio_ndt_align", "lio_ndt_align_batch", "lio_ndt_enable_kernel_timing", "lio_ndt_kernel_times",
    "lio_gicp_create", "lio_gicp_destroy", "lio_gicp_set_target", "lio_gicp_set_source", "lio_gicp_set_voxel_mode", "lio_gicp_voxel_at", "lio_gicp_download", "lio_gicp_correspondences", "lio_gicp_neighbours", "lio_gicp_mahalanobis", "lio_gicp_linearize", "lio_gicp_align", "lio_gicp_fitness_score",
    "lio_loop_default_params", "lio_loop_find_candidates", "lio_loop_information_matrix", "lio_loop_create", "lio_loop_destroy", "lio_loop_reset",
    "lio_loop_add_keyframe_host", "lio_loop_set_pose", "lio_loop_num_keyframes", "lio_loop_download_keyframe", "lio_loop_detect", "lio_loop_edges",
    "lio_loop_last_report", "lio_loop_last_times", "lio_loop_align_candidates", "lio_loop_align_fine", "lio_loop_pair_information",
    "lio_overlap_default_params", "lio_overlap_connection_count", "lio_overlap_find_candidates", "lio_overlap_create", "lio_overlap_destroy",
    "lio_overlap_gate_batch", "lio_overlap_align_pairs", "lio_overlap_accumulate", "lio_overlap_download_accum", "lio_overlap_detect",
    "lio_overlap_last_report", "lio_overlap_last_times",
    "lio_sc_create", "lio_sc_destroy", "lio_sc_reset", "lio_sc_num_frames", "lio_sc_add_frames_host", "lio_sc_download_frame", "lio_sc_describe_host", "lio_sc_set_active",
    "lio_sc_distance", "lio_sc_search", "lio_sc_global_search_host", "lio_sc_shift_to_yaw", "lio_sc_last_dropped", "lio_sc_last_times",
    "lio_sc_set_positions", "lio_sc_local_search", "lio_sc_last_local", "lio_update_origin",
    "lio_graph_default_params", "lio_graph_create", "lio_graph_destroy", "lio_graph_reset", "lio_graph_add_node", "lio_graph_set_fixed", "lio_graph_set_estimate",
    "lio_graph_num_nodes", "lio_graph_get_fixed", "lio_graph_add_edge", "lio_graph_remove_edge", "lio_graph_optimize", "lio_graph_estimates", "lio_graph_edges",
    "lio_graph_chi2", "lio_graph_linearize", "lio_graph_last_times", "lio_se3_from_mqt", "lio_se3_to_mqt", "lio_graph_edge_error",
    "lio_graph_add_prior", "lio_graph_set_kernel", "lio_graph_priors", "lio_graph_prior_error", "lio_graph_remove_gnss_outliers",
    "lio_graph_remove_node", "lio_graph_node_live", "lio_graph_edge_records", "lio_loop_retire",
    "lio_graph_estimate_gnss_moment", "lio_graph_moment_begin", "lio_graph_moment_end", "lio_graph_moment_get", "lio_graph_moment_linearize",
    "lio_render_create", "lio_render_destroy", "lio_render_clear", "lio_render_set_cameras", "lio_render_set_active", "lio_render_frame", "lio_render_size",
    "lio_render_download", "lio_render_download_voxels", "lio_render_download_points", "lio_render_download_last_image", "lio_render_last_times",
    "lio_utm_create", "lio_utm_destroy", "lio_utm_zone", "lio_utm_forward", "lio_utm_inverse", "lio_utm_longitude0", "lio_grid_convergence",
    "lio_transform_from_rpyt", "lio_quat_of_transform", "lio_interpolate_transform", "lio_rtk_transform_utm", "lio_rtk_transform_origin",
    "lio_rtk_track_create", "lio_rtk_track_destroy", "lio_rtk_track_set_origin", "lio_rtk_track_origin", "lio_rtk_track_feed", "lio_rtk_track_size",
    "lio_rtk_track_interpolate",
    "lio_gnss_queue_create", "lio_gnss_queue_destroy", "lio_gnss_queue_set_origin", "lio_gnss_queue_push", "lio_gnss_queue_size", "lio_gnss_queue_stamps",
    "lio_gnss_queue_flush",
    "lio_scan_merge_create", "lio_scan_merge_destroy", "lio_scan_merge_set_transform", "lio_scan_merge_run_host", "lio_scan_merge_download",
    "lio_scan_merge_device", "lio_scan_merge_last_times",
    "lio_calib_subsample", "lio_se3f_exp", "lio_se3f_log", "lio_se3f_mul", "lio_se3f_inverse", "lio_se3f_matrix", "lio_se3f_from_matrix",
    "lio_calib_interpolate", "lio_dfo_default_params", "lio_dfo_direct_l", "lio_dfo_nelder_mead", "lio_calib_default_params",
    "lio_calib_ins_create", "lio_calib_ins_destroy", "lio_calib_ins_reset", "lio_calib_ins_add_scan", "lio_calib_ins_add_odom", "lio_calib_ins_counts",
    "lio_calib_ins_set_transform", "lio_calib_ins_scan_matrices", "lio_calib_ins_combined", "lio_calib_ins_error", "lio_calib_ins_error_terms",
    "lio_calib_ins_calibrate", "lio_calib_ins_progress", "lio_calib_ins_result", "lio_calib_ins_last_times",
    "lio_calib_ground_default_params", "lio_calib_ground_create", "lio_calib_ground_destroy", "lio_calib_ground_crop_host",
    "lio_calib_ground_set_points_host", "lio_calib_ground_fit", "lio_calib_ground_download_indices", "lio_calib_ground_download_points",
    "lio_calib_ground_download_draws", "lio_calib_ground_last_run", "lio_calib_ground_last_times",
    "lio_calib_imu_integrate", "lio_calib_imu_interpolate", "lio_calib_imu_time_align", "lio_calib_imu_solve", "lio_calib_imu_create",
    "lio_calib_imu_destroy", "lio_calib_imu_reset", "lio_calib_imu_add_imu", "lio_calib_imu_add_frame", "lio_calib_imu_lidar_pose",
    "lio_calib_imu_calibrate", "lio_calib_imu_lidar_poses", "lio_calib_imu_imu_poses", "lio_calib_imu_map_download",
    "lio_calib_imu_target_download", "lio_calib_imu_counts", "lio_calib_imu_last_times", "lio_calib_imu_set_max_iterations",
    "lio_boxes_create", "lio_boxes_destroy", "lio_boxes_pairwise", "lio_boxes_nms", "lio_boxes_set_gate", "lio_boxes_postprocess",
    "lio_boxes_postprocess_device", "lio_boxes_last_indices", "lio_boxes_last_times",
    "lio_voxelize_grid_size", "lio_voxelizer_create", "lio_voxelizer_destroy", "lio_voxelizer_reset", "lio_voxelizer_forward",
    "lio_voxelizer_forward_device", "lio_voxelizer_output", "lio_voxelizer_output_device", "lio_voxelizer_window",
    "lio_voxelizer_window_counts", "lio_voxelizer_window_device", "lio_voxelizer_last_counts", "lio_voxelizer_last_times",
]
ABI_VERSION = 22  # kept at 22 for callers that compare against it; the revision the binding needs is ABI_REQUIRED
ABI_REQUIRED = 23  # the oldest library revision that has every symbol above; lib() refuses an older one
RTK_INTERPOLATED, RTK_EXACT, RTK_NO_ORIGIN, RTK_TOO_FEW, RTK_EARLY, RTK_LATE = 0, 1, 2, 3, 4, 5  # lio_rtk_track_interpolate


class NormalEq(C.Structure):
    _fields_ = [("JtJ", C.c_double * 36), ("Jtr", C.c_double * 6), ("nnT", C.c_double * 9), ("eigvec", C.c_double * 9),
                ("eigval", C.c_double * 3), ("contri", C.c_double * 3), ("strong", C.c_double * 3), ("sum_abs_res", C.c_double),
                ("n_eff", C.c_uint32), ("n_ds", C.c_uint32), ("n_knn_candidates_lo", C.c_uint32), ("n_knn_candidates_hi", C.c_uint32),
                ("n_tie", C.c_uint32), ("seq", C.c_uint32)]


class BatchTimes(C.Structure):
    _fields_ = [("downsample_us", C.c_double), ("knn_us", C.c_double), ("linearize_us", C.c_double), ("step_us", C.c_double),
                ("downsample_launches", C.c_uint32), ("knn_launches", C.c_uint32), ("linearize_launches", C.c_uint32), ("step_launches", C.c_uint32),
                ("insert_us", C.c_double), ("insert_launches", C.c_uint32), ("pad", C.c_uint32)]


class PassLog(C.Structure):
    _fields_ = [("knn", C.c_int32), ("n_eff", C.c_int32), ("valid", C.c_int32), ("degenerate", C.c_int32), ("sum_abs_res", C.c_double),
                ("JtJ", C.c_double * 36), ("Jtr", C.c_double * 6), ("dx", C.c_double * 23)]


SUMS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double))
DEG_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))
MEAS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int)


class Timings(C.Structure):
    _fields_ = [("downsample_us", C.c_float), ("knn_us", C.c_float), ("linearize_us", C.c_float), ("insert_us", C.c_float),
                ("total_device_us", C.c_float), ("host_solve_us", C.c_float), ("total_wall_us", C.c_float), ("n_knn_pass", C.c_int32),
                ("n_pass", C.c_int32), ("n_ds", C.c_int32), ("n_eff_last", C.c_int32), ("n_added", C.c_int32),
                ("knn_candidates", C.c_uint64), ("undistort_us", C.c_float), ("imu_host_us", C.c_float)]


class ScanJob(C.Structure):
    _fields_ = [("d_raw", C.c_void_p), ("n_raw", C.c_uint32), ("flags", C.c_uint32), ("lidar_beg_time", C.c_double),
                ("state_in", C.POINTER(C.c_double)), ("cov_in", C.POINTER(C.c_double)), ("state_out", C.POINTER(C.c_double)),
                ("rc", C.c_int32), ("n_ds", C.c_int32), ("n_pass", C.c_int32), ("n_knn_pass", C.c_int32)]


class GpsObservation(C.Structure):  # lio_gps_observation
    _fields_ = [("T", C.c_double * 16), ("precision", C.c_double), ("dimension", C.c_int32)]


class NdtParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("lm_max_iterations", C.c_int32), ("rotation_epsilon_deg", C.c_double),
                ("transformation_epsilon", C.c_double), ("lm_init_lambda_factor", C.c_double), ("max_process_time_ms", C.c_double)]


class GroundParams(C.Structure):  # lio_ground_params
    _fields_ = [("sensor_height", C.c_double), ("clip_low", C.c_double), ("clip_high", C.c_double), ("use_normal_filter", C.c_int32),
                ("normal_thresh_deg", C.c_double), ("k", C.c_int32), ("distance_threshold", C.c_double), ("min_points", C.c_int32),
                ("floor_normal_thresh_deg", C.c_double), ("max_iterations", C.c_int32), ("probability", C.c_double), ("seed", C.c_uint32)]


class RenderImage(C.Structure):  # lio_render_image
    _fields_ = [("camera", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32), ("bgr", C.c_void_p), ("pose", C.c_double * 16)]


RENDER_SKIPPED, RENDER_NO_FLOOR, RENDER_DONE = 0, 1, 2  # lio_render_frame


class KeyframerParams(C.Structure):  # lio_keyframer_params
    _fields_ = [("key_frame_distance", C.c_double), ("key_frame_degree", C.c_double), ("resolution", C.c_double), ("key_frame_range", C.c_double),
                ("scan_period", C.c_double), ("radius", C.c_double), ("min_neighbours", C.c_int32), ("local_map_cap", C.c_uint32),
                ("local_map_distance", C.c_double), ("fitness_range", C.c_double)]


class KeyframeReport(C.Structure):  # lio_keyframe_report
    _fields_ = [("first", C.c_int32), ("need", C.c_int32), ("must", C.c_int32), ("elected", C.c_int32), ("emitted", C.c_int32), ("nr", C.c_uint32),
                ("n_downsampled", C.c_uint32), ("local_map_size", C.c_uint32), ("dx", C.c_double), ("da", C.c_double), ("score", C.c_double),
                ("accum_distance", C.c_double), ("average_score", C.c_double)]


class LoopParams(C.Structure):  # lio_loop_params
    _fields_ = [("distance_thresh", C.c_double), ("accum_distance_thresh", C.c_double), ("distance_from_last_edge_thresh", C.c_double),
                ("distance_new_keyframe_thresh", C.c_double), ("distance_keyframe_thresh", C.c_double), ("fitness_score_max_range", C.c_double),
                ("fitness_score_thresh", C.c_double), ("fine_max_corr_dist", C.c_double), ("voxel_resolution", C.c_double),
                ("coarse_translation_epsilon", C.c_double), ("coarse_rotation_epsilon_deg", C.c_double), ("fine_translation_epsilon", C.c_double),
                ("fine_rotation_epsilon_deg", C.c_double), ("max_iterations", C.c_int32), ("k_correspondences", C.c_int32), ("grid_resolution", C.c_float),
                ("max_points", C.c_uint32), ("max_candidates", C.c_uint32), ("pad", C.c_uint32)]


class LoopEdge(C.Structure):  # lio_loop_edge
    _fields_ = [("key1", C.c_int32), ("key2", C.c_int32), ("relative_pose", C.c_float * 16), ("score", C.c_double), ("information", C.c_double * 36)]


class LoopReport(C.Structure):  # lio_loop_report
    _fields_ = [("new_id", C.c_int32), ("n_candidates", C.c_int32), ("best", C.c_int32), ("fine_converged", C.c_int32), ("fine_iterations", C.c_int32),
                ("reason", C.c_int32), ("coarse_rounds", C.c_int32), ("pad", C.c_int32), ("best_score", C.c_double), ("fine_score", C.c_double)]


class OverlapParams(C.Structure):  # lio_overlap_params
    _fields_ = [("distance_thresh", C.c_double), ("candidate_link_dist", C.c_int32), ("max_candidate_num", C.c_int32), ("knn", C.c_int32), ("min_z", C.c_float),
                ("fitness_score_max_range", C.c_double), ("fitness_score_thresh", C.c_double), ("fitness_inlier_thresh", C.c_double), ("gate_max_range", C.c_double),
                ("xy_range", C.c_double), ("fine_max_corr_dist", C.c_double), ("fine_translation_epsilon", C.c_double), ("max_accum_points", C.c_uint32),
                ("pad", C.c_uint32)]


class OverlapEdge(C.Structure):  # lio_overlap_edge
    _fields_ = [("key1", C.c_int32), ("key2", C.c_int32), ("relative_pose", C.c_float * 16), ("score", C.c_double), ("information", C.c_double * 36)]


class OverlapReport(C.Structure):  # lio_overlap_report
    _fields_ = [("new_id", C.c_int32), ("n_candidates", C.c_int32), ("best", C.c_int32), ("fine_converged", C.c_int32), ("fine_iterations", C.c_int32),
                ("reason", C.c_int32), ("n_accum", C.c_uint32), ("n_neighbours_skipped", C.c_int32), ("best_score", C.c_double), ("fine_score", C.c_double),
                ("n_neighbours_dropped", C.c_int32), ("pad", C.c_int32)]


class OverlapTimes(C.Structure):  # lio_overlap_times
    _fields_ = [("candidates_us", C.c_double), ("gate_us", C.c_double), ("targets_us", C.c_double), ("coarse_us", C.c_double), ("fitness_us", C.c_double),
                ("accumulate_us", C.c_double), ("fine_us", C.c_double), ("coarse_rounds", C.c_int32), ("n_pairs", C.c_int32), ("n_targets", C.c_int32),
                ("pad", C.c_int32)]


OVERLAP_ACCUM = -1  # LIO_OVERLAP_ACCUM


class GraphParams(C.Structure):  # lio_graph_params
    _fields_ = [("cg_epsilon", C.c_double), ("chi2_rel_stop", C.c_double), ("min_edges", C.c_int32), ("cg_max_iterations", C.c_int32)]


class GraphReport(C.Structure):  # lio_graph_report
    _fields_ = [("iterations", C.c_int32), ("stop_reason", C.c_int32), ("trials", C.c_int32), ("accepted", C.c_int32), ("n_active", C.c_int32),
                ("n_live_edges", C.c_int32), ("cg_iterations", C.c_int32), ("cg_iterations_total", C.c_int32), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double), ("lambda_", C.c_double), ("cg_residual", C.c_double)]


GRAPH_KERNEL_NONE, GRAPH_KERNEL_HUBER = 0, 1
GRAPH_KERNEL_DCS2 = 2
GRAPH_PRIOR_XYZ, GRAPH_PRIOR_QUAT, GRAPH_PRIOR_PLANE = 0, 1, 2


class BevInfo(C.Structure):  # lio_bev_info
    _fields_ = [("n_in", C.c_uint32), ("n_dropped", C.c_uint32), ("n_kept", C.c_uint32), ("rank_lo", C.c_uint32), ("rank_hi", C.c_uint32),
                ("n_pixels", C.c_uint32), ("image_w", C.c_uint32), ("image_h", C.c_uint32), ("padded_w", C.c_uint32), ("padded_h", C.c_uint32),
                ("patch", C.c_int32), ("half_patch", C.c_int32), ("quarter_patch", C.c_int32), ("nodes_x", C.c_uint32), ("nodes_y", C.c_uint32),
                ("reserved", C.c_uint32), ("pixel_per_meter", C.c_double), ("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double),
                ("y_max", C.c_double)]


class AlignJob(C.Structure):  # lio_align_job
    _fields_ = [("target", C.c_void_p), ("source", C.c_void_p), ("guess", C.POINTER(C.c_double)), ("out", C.c_double * 16), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("evaluations", C.c_int32), ("rc", C.c_int32)]


ESTIMATE_K = 5  # LIO_ESTIMATE_K


class EstimateReport(C.Structure):  # lio_estimate_report
    _fields_ = [("n_ids", C.c_int32), ("ids", C.c_int32 * ESTIMATE_K), ("n_target", C.c_uint32), ("n_source", C.c_uint32), ("converged", C.c_int32),
                ("iterations", C.c_int32), ("result", C.c_int32), ("pose_replaced", C.c_int32), ("z_mean_target", C.c_double), ("z_mean_source", C.c_double),
                ("guess", C.c_double * 16), ("score", C.c_double), ("nearest_us", C.c_double), ("gather_us", C.c_double), ("set_target_us", C.c_double),
                ("set_source_us", C.c_double), ("z_source_us", C.c_double), ("align_us", C.c_double), ("fitness_us", C.c_double)]


class NdtTimes(C.Structure):  # lio_ndt_times
    _fields_ = [("cost_us", C.c_double), ("launches", C.c_uint64), ("update_launches", C.c_uint64), ("pairs", C.c_uint64), ("source_points", C.c_uint64)]


class RtkFix(C.Structure):  # lio_rtk_fix
    _fields_ = [("stamp_us", C.c_uint64), ("latitude", C.c_double), ("longitude", C.c_double), ("altitude", C.c_double), ("heading", C.c_double),
                ("pitch", C.c_double), ("roll", C.c_double), ("precision", C.c_double), ("dimension", C.c_int32), ("reserved", C.c_int32)]


class GnssMatch(C.Structure):  # lio_gnss_match
    _fields_ = [("keyframe", C.c_int32), ("dimension", C.c_int32), ("first_stamp_us", C.c_uint64), ("second_stamp_us", C.c_uint64),
                ("xyz", C.c_double * 3), ("quat", C.c_double * 4), ("precision", C.c_double)]


class KernelTimes(C.Structure):
    _fields_ = [("knn_us", C.c_double), ("linearize_us", C.c_double), ("finalize_us", C.c_double), ("knn_launches", C.c_uint32),
                ("linearize_launches", C.c_uint32), ("finalize_launches", C.c_uint32), ("pad", C.c_uint32)]


DFO_MAX_DIM = 8  # LIO_DFO_MAX_DIM
DFO_STOP_EVALS, DFO_STOP_XTOL, DFO_STOP_HOOK = 0, 1, 2
CALIB_MAX_SCANS, CALIB_GLOBAL, CALIB_LOCAL, CALIB_UNCAPPED = 64, 0, 1, 2


class DfoParams(C.Structure):  # lio_dfo_params
    _fields_ = [("max_evals", C.c_int32), ("reserved", C.c_int32), ("xtol_abs", C.c_double), ("epsilon", C.c_double), ("step", C.c_double * DFO_MAX_DIM)]


class DfoReport(C.Structure):  # lio_dfo_report
    _fields_ = [("evals", C.c_int32), ("stop", C.c_int32), ("f_best", C.c_double)]


class CalibParams(C.Structure):  # lio_calib_params
    _fields_ = [("local_only", C.c_int32), ("time_cal", C.c_int32), ("max_time_offset", C.c_double), ("max_evals", C.c_int32),
                ("knn_batch_size", C.c_int32), ("xtol", C.c_double), ("local_knn_k", C.c_int32), ("global_knn_k", C.c_int32),
                ("local_knn_max_dist", C.c_float), ("global_knn_max_dist", C.c_float), ("direct_epsilon", C.c_double), ("nm_step", C.c_double * 7)]


class CalibGroundParams(C.Structure):  # lio_calib_ground_params
    _fields_ = [("sigma", C.c_double), ("num_iteration", C.c_int32), ("thresh", C.c_double), ("seed", C.c_uint32)]


class VoxelizerParams(C.Structure):  # lio_voxelizer_params
    _fields_ = [("min_range", C.c_float * 3), ("max_range", C.c_float * 3), ("voxel_size", C.c_float * 3), ("max_voxels", C.c_uint32),
                ("max_points_per_voxel", C.c_uint32), ("max_points", C.c_uint32), ("max_frame_num", C.c_uint32), ("order", C.c_int32)]


CALIB_GROUND_MAX_VERTICES = 256  # LIO_CALIB_GROUND_MAX_VERTICES
BOXES_NMS_ROTATED, BOXES_NMS_AABB_GATE = 0, 1  # LIO_BOXES_NMS_*
BOXES_MAX = 16384  # the most boxes a lio_boxes handle takes
VOXEL_ORDER_XYZ, VOXEL_ORDER_ZYX = 1, 2  # LIO_VOXEL_ORDER_*

DFO_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int, C.c_void_p)  # lio_dfo_fn
DFO_HOOK = C.CFUNCTYPE(C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_void_p)  # lio_dfo_hook
REDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.c_int)
GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p)  # lio_gather_fn: (ctx, d_local, d_gathered, n_records, stream)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback for the LIO hot path.")
    L = C.CDLL(LIB_PATH)
    vp, f32p, f64p, i32p, u8p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    u32, u64, dbl, flt, cint = C.c_uint32, C.c_uint64, C.c_double, C.c_float, C.c_int

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("lio_last_error", C.c_char_p)
    sig("lio_last_warning", C.c_char_p)
    sig("lio_device_count", cint)
    sig("lio_abi_version", cint)
    if L.lio_abi_version() < ABI_REQUIRED:
        raise RuntimeError(f"{LIB_PATH} is at ABI revision {L.lio_abi_version()}, this binding needs {ABI_REQUIRED}: build it again")
    sig("lio_pinned_alloc", vp, u64)
    sig("lio_pinned_free", None, vp)
    sig("lio_map_bytes", u64, vp)
    sig("lio_map_create", vp, cint, flt, u64, u64, cint)
    sig("lio_map_destroy", None, vp)
    sig("lio_map_set_stencil", cint, vp, cint)
    sig("lio_map_insert", cint, vp, f32p, u64, dbl)
    sig("lio_map_insert_device", cint, vp, vp, u64, dbl)
    sig("lio_map_stats", cint, vp, C.POINTER(u64), C.POINTER(u64))
    sig("lio_map_dump", C.c_int64, vp, f32p, u64)
    sig("lio_map_set_lru", cint, vp, u64, dbl)
    sig("lio_map_lru_stats", cint, vp, C.POINTER(u64), C.POINTER(u64))
    sig("lio_map_lru_exact_stats", cint, vp, C.POINTER(u64), C.POINTER(u64))
    sig("lio_map_clear", cint, vp)
    sig("lio_map_set_tie_mode", cint, vp, cint)
    sig("lio_map_tie_stats", cint, vp, C.POINTER(u64), C.POINTER(u64))
    sig("lio_map_pool_stats", cint, vp, C.POINTER(u64), C.POINTER(u64))
    sig("lio_map_knn_candidates", u64, vp)
    sig("lio_map_knn_touched", u64, vp)
    sig("lio_map_knn_unique", u64, vp)
    sig("lio_map_knn", cint, vp, f32p, u32, f32p, i32p)
    sig("lio_scan_create", vp, cint, u32, u32)
    sig("lio_scan_destroy", None, vp)
    sig("lio_scan_reset", cint, vp)
    sig("lio_scan_upload", cint, vp, f32p, u32)
    sig("lio_scan_set_device", cint, vp, vp, u32)
    sig("lio_scan_undistort_delta", cint, vp, vp, cint, f32p, C.c_double)
    sig("lio_scan_undistort_poses", cint, vp, vp, cint, u64, C.POINTER(u64), f64p, u32)
    sig("lio_scan_undistort_imu", cint, vp, vp, cint, f64p, u32, f64p, f64p, f64p, f64p, dbl, cint, cint)
    sig("lio_scan_download_raw", cint, vp, f32p, u32)
    sig("lio_scan_voxel_downsample", cint, vp, flt, cint, C.POINTER(u32))
    sig("lio_scan_voxel_downsample_batch", cint, C.POINTER(vp), cint, flt, C.POINTER(u32))
    sig("lio_scan_set_ds", cint, vp, f32p, u32)
    sig("lio_scan_num_ds", cint, vp)
    sig("lio_scan_download_ds", cint, vp, f32p, u32)
    sig("lio_scan_download_world", cint, vp, f32p, u32)
    sig("lio_scan_download_match", cint, vp, u8p, f32p, i32p, f32p)
    sig("lio_p2plane_linearize", cint, vp, vp, f64p, f64p, cint, C.POINTER(NormalEq))
    sig("lio_scan_set_degeneracy_mode", cint, vp, cint)
    sig("lio_p2plane_degeneracy", cint, vp, f64p, f64p, f64p)
    sig("lio_engine_set_reduce_hook", cint, vp, REDUCE_FN, vp)
    sig("lio_p2plane_rows", cint, vp, f64p, f64p, f64p, f64p, u32)
    sig("lio_map_incremental", cint, vp, vp, f64p, f64p, flt, cint, dbl)
    sig("lio_map_seed", cint, vp, vp, f64p, f64p, dbl)
    sig("lio_engine_create", vp, cint, flt, cint, u64, u64, u32, u32)
    sig("lio_engine_create_shared", vp, vp, u32, u32)
    sig("lio_engine_destroy", None, vp)
    sig("lio_engine_map", vp, vp)
    sig("lio_engine_scan", vp, vp)
    sig("lio_engine_set_state", cint, vp, f64p)
    sig("lio_engine_get_state", cint, vp, f64p)
    sig("lio_engine_set_cov", cint, vp, f64p)
    sig("lio_engine_get_cov", cint, vp, f64p)
    sig("lio_engine_set_flags", cint, vp, cint, cint, dbl, dbl)
    sig("lio_engine_travel", dbl, vp)
    sig("lio_engine_is_degenerate", cint, vp)
    sig("lio_engine_update", cint, vp)
    sig("lio_engine_pass_log", cint, vp, cint, C.POINTER(PassLog))
    sig("lio_engine_process_scan", cint, vp, f32p, u32, dbl)
    sig("lio_engine_process_scan_device", cint, vp, vp, u32, dbl)
    sig("lio_engine_timings", cint, vp, C.POINTER(Timings))
    sig("lio_engine_flush", cint, vp)
    sig("lio_engine_enable_timing", cint, vp, cint)
    sig("lio_engines_process_batch", cint, C.POINTER(vp), cint, C.POINTER(ScanJob), cint)
    sig("lio_comm_unique_id", cint, C.POINTER(C.c_uint8))
    sig("lio_comm_init", vp, cint, cint, cint, C.POINTER(C.c_uint8))
    sig("lio_comm_destroy", None, vp)
    sig("lio_comm_rank", cint, vp)
    sig("lio_comm_world", cint, vp)
    sig("lio_allgather_normal_eq", cint, vp, vp, vp, vp, vp)
    sig("lio_comm_stats", cint, vp, C.POINTER(u64), f64p)
    sig("lio_engine_set_joint", cint, vp, C.POINTER(vp), cint, vp)
    sig("lio_engine_joint_register", cint, vp, f32p, u32, dbl, f64p, f64p)
    sig("lio_engine_joint_register_device", cint, vp, vp, u32, dbl, f64p, f64p)
    sig("lio_allgather_records", cint, vp, vp, vp, u32, vp)
    sig("lio_batch_create_joint", vp, C.POINTER(vp), cint, vp, cint, cint, u32, u32)
    sig("lio_batch_set_gather_hook", cint, vp, GATHER_FN, vp, cint, cint)
    sig("lio_batch_exchange_stats", cint, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
    sig("lio_batch_create", vp, vp, cint, cint, u32, u32)
    sig("lio_batch_create_sequences", vp, cint, C.c_float, cint, u64, u64, cint, cint, u32, u32)
    sig("lio_batch_sequences_step", cint, vp, C.POINTER(ScanJob), cint, C.POINTER(C.c_double))
    sig("lio_batch_fastlio_main", cint, vp, C.POINTER(cint))
    sig("lio_batch_destroy", None, vp)
    sig("lio_batch_process", cint, vp, C.POINTER(ScanJob), cint)
    sig("lio_batch_engine", vp, vp, cint, cint)
    sig("lio_batch_enable_kernel_timing", cint, vp, cint)
    sig("lio_batch_kernel_times", cint, vp, C.POINTER(BatchTimes), cint)
    sig("lio_engine_set_static_map", cint, vp, cint)
    sig("lio_localmap_create", vp, cint, u64, u32, u32)
    sig("lio_localmap_destroy", None, vp)
    sig("lio_localmap_add_keyframe", cint, vp, f32p, u32, f32p)
    sig("lio_localmap_num_keyframes", cint, vp)
    sig("lio_localmap_update", cint, vp, vp, f64p, dbl, dbl, dbl, flt, C.POINTER(cint), C.POINTER(u32))
    sig("lio_localmap_download", cint, vp, f32p, u32)
    sig("lio_localmap_nearest", cint, vp, f64p, u32, i32p, f32p)
    sig("lio_localmap_gather", cint, vp, i32p, u32, C.POINTER(u32), f64p)
    sig("lio_localmap_z_mean", cint, vp, vp, u32, f64p)
    sig("lio_localmap_download_gather", cint, vp, f32p, u32)
    sig("lio_localmap_gather_device", vp, vp, C.POINTER(u32))
    sig("lio_localmap_store_frame", cint, vp, cint, vp, u32)
    sig("lio_localmap_frame", vp, vp, cint, C.POINTER(u32))
    sig("lio_estimate_matcher_params", None, C.POINTER(NdtParams))
    sig("lio_localmap_estimate_pose", cint, vp, vp, vp, u32, f64p, C.POINTER(EstimateReport), f64p)
    sig("lio_scan_ds_device", vp, vp, C.POINTER(u32))
    sig("lio_cloud_create", vp, cint, u64)
    sig("lio_cloud_destroy", None, vp)
    sig("lio_cloud_clear", cint, vp)
    sig("lio_cloud_size", cint, vp, C.POINTER(u64))
    sig("lio_cloud_append_scan", cint, vp, vp, f64p, flt, cint, dbl, dbl)
    sig("lio_cloud_append_host", cint, vp, f32p, u64, f64p, flt, cint, dbl, dbl)
    sig("lio_cloud_voxel_downsample", cint, vp, flt, C.POINTER(u64))
    sig("lio_cloud_download", C.c_int64, vp, f32p, u64)
    sig("lio_cloud_scratch_bytes", cint, vp, C.POINTER(u64))
    sig("lio_cloud_last_times", cint, vp, f64p, f64p)
    sig("lio_knn_index_create", vp, cint)
    sig("lio_knn_index_destroy", None, vp)
    sig("lio_knn_index_build", cint, vp, f32p, C.POINTER(C.c_uint32), u64, C.POINTER(u64))
    sig("lio_knn_index_query", cint, vp, f32p, u64, cint, i32p, f32p)
    sig("lio_knn_index_colour", cint, vp, f32p, u64, cint, u8p)
    sig("lio_knn_index_last_times", cint, vp, f64p, f64p)
    gp, u32p = C.POINTER(GroundParams), C.POINTER(u32)
    sig("lio_ground_default_params", None, gp, cint)
    sig("lio_ground_draw", None, u32, u32, u32, u32p)
    sig("lio_ground_create", vp, cint)
    sig("lio_ground_destroy", None, vp)
    sig("lio_ground_detect_scan", cint, vp, vp, gp, cint, C.POINTER(cint), f32p, u32p, u32p, u32p)
    sig("lio_ground_detect_host", cint, vp, f32p, u64, gp, C.POINTER(cint), f32p, u32p, u32p, u32p)
    sig("lio_ground_download_indices", C.c_int64, vp, cint, u32p, u64)
    sig("lio_ground_download_normals", C.c_int64, vp, f32p, u64)
    sig("lio_ground_download_inliers", C.c_int64, vp, f32p, u64)
    sig("lio_ground_download_draws", C.c_int64, vp, u32p, u32p, f32p, u64)
    sig("lio_ground_last_run", cint, vp, C.POINTER(cint), C.POINTER(cint), C.POINTER(cint), C.POINTER(cint))
    sig("lio_ground_last_times", cint, vp, f64p, f64p)
    kp, kr, u64p = C.POINTER(KeyframerParams), C.POINTER(KeyframeReport), C.POINTER(u64)
    sig("lio_keyframe_decide", cint, f64p, f64p, dbl, dbl, C.POINTER(cint), C.POINTER(cint), f64p, f64p)
    sig("lio_keyframer_default_params", None, kp)
    sig("lio_keyframer_create", vp, cint, kp)
    sig("lio_keyframer_destroy", None, vp)
    sig("lio_keyframer_reset", cint, vp)
    sig("lio_keyframer_push_host", cint, vp, f32p, u32p, u32, u64, f64p, f64p, u64p, f64p, u32, kr)
    sig("lio_keyframer_pending", cint, vp)
    sig("lio_keyframer_pop", C.c_int64, vp, f32p, u64, f64p, u64p, f64p, u32p, u32p)
    sig("lio_radius_outlier_host", C.c_int64, vp, f32p, u64, dbl, cint, u32p, u64, u32p)
    sig("lio_keyframe_filter_host", C.c_int64, vp, f32p, u64, dbl, cint, dbl, u32p, u64, u32p, u32p)
    sig("lio_keyframer_fitness_host", cint, vp, f32p, u32, f64p, f64p, u32p)
    sig("lio_keyframer_append_local_map_host", cint, vp, f32p, u32, f64p)
    sig("lio_keyframer_download_local_map", C.c_int64, vp, f32p, u64)
    sig("lio_keyframer_last_times", cint, vp, f64p, f64p, f64p, f64p)
    u16p = C.POINTER(C.c_uint16)
    sig("lio_bev_create", vp, cint)
    sig("lio_bev_destroy", None, vp)
    sig("lio_bev_preprocess_host", cint, vp, f32p, u64, dbl)
    sig("lio_bev_preprocess_cloud", cint, vp, vp, dbl)
    sig("lio_bev_upload_pixels", cint, vp, u32p, f32p, f32p, u64, u32, u32)
    sig("lio_bev_convert", cint, vp, dbl, dbl)
    sig("lio_bev_get_info", cint, vp, C.POINTER(BevInfo))
    sig("lio_bev_download_pixel_coords", C.c_int64, vp, i32p, u64)
    sig("lio_bev_download_kept", C.c_int64, vp, u32p, u64)
    sig("lio_bev_download_pixels", C.c_int64, vp, u32p, f32p, f32p, u64)
    sig("lio_bev_download_nodes", C.c_int64, vp, u32p, i32p, f64p, u64)
    sig("lio_bev_download_equalised", C.c_int64, vp, f32p, u64)
    sig("lio_bev_download_image", C.c_int64, vp, u16p, u64)
    sig("lio_bev_grey_table", None, u16p)
    sig("lio_bev_last_times", cint, vp, f64p, f64p)
    sig("lio_pose_estimator_create", vp, f32p, u64, f32p, f32p, dbl)
    sig("lio_pose_estimator_destroy", None, vp)
    sig("lio_pose_estimator_predict", cint, vp, u64, f32p, f32p)
    sig("lio_pose_estimator_match", cint, vp, vp, vp, C.POINTER(NdtParams), f32p, C.POINTER(cint))
    sig("lio_pose_estimator_match_gps", cint, vp, vp, vp, C.POINTER(NdtParams), C.POINTER(GpsObservation), f32p, f32p, C.POINTER(cint))
    sig("lio_pose_estimator_guess", cint, vp, C.POINTER(GpsObservation), f32p)
    sig("lio_pose_estimator_observe", cint, vp, f32p, f32p, cint, C.POINTER(GpsObservation), f32p, f32p)
    sig("lio_pose_estimator_match_gps_only", cint, vp, C.POINTER(GpsObservation), f32p, f32p)
    sig("lio_pose_estimator_get_timed_pose", cint, vp, u64, f64p, f64p, f64p)
    sig("lio_pose_estimator_predict_nostate", cint, vp, u64, f64p)
    sig("lio_pose_estimator_correct", cint, vp, u64, f32p)
    sig("lio_pose_estimator_get_dt", u64, vp)
    sig("lio_pose_estimator_get", cint, vp, f32p, f32p)
    sig("lio_pose_estimator_set", cint, vp, f32p, f32p)
    sig("lio_pose_estimator_matrix", cint, vp, f32p)
    sig("lio_fastlio_init", cint, vp, f64p, f64p, cint, cint, dbl, cint)
    sig("lio_fastlio_is_init", cint, vp)
    sig("lio_fastlio_imu_enqueue", cint, vp, dbl, f64p, f64p)
    sig("lio_engine_set_device_loop", cint, vp, cint)
    sig("lio_fastlio_set_wheelspeed", cint, vp, cint)
    sig("lio_fastlio_ins_enqueue", cint, vp, dbl, f64p)
    sig("lio_fastlio_pcl_enqueue", cint, vp, f32p, C.POINTER(u32), u32, dbl)
    sig("lio_fastlio_pcl_enqueue_device", cint, vp, vp, vp, u32, dbl)
    sig("lio_fastlio_main", cint, vp)
    sig("lio_fastlio_odometry", cint, vp, f64p, f64p)
    sig("lio_fastlio_state", cint, vp, f64p)
    sig("lio_fastlio_start_state", cint, vp, f64p)
    sig("lio_fastlio_download_undistorted", cint, vp, f32p, u32, C.POINTER(u32))
    sig("lio_eskf_update_cb", cint, f64p, f64p, dbl, cint, MEAS_FN, vp, cint, f64p, f64p)
    sig("lio_eskf_update_ws_cb", cint, f64p, f64p, dbl, cint, MEAS_FN, vp, cint, f64p, cint, f64p, f64p)
    sig("lio_state_predict", cint, f64p, f64p, dbl, f64p, f64p, f64p, f64p, f64p)
    sig("lio_eskf_update_sums_cb", cint, f64p, f64p, dbl, cint, cint, SUMS_FN, DEG_FN, vp, f64p, f64p, C.POINTER(PassLog), cint, C.POINTER(cint))
    sig("lio_eskf_update_cb", cint, f64p, f64p, dbl, cint, MEAS_FN, vp, cint, f64p, f64p)
    sig("lio_scan_enable_kernel_timing", cint, vp, cint)
    sig("lio_scan_kernel_times", cint, vp, C.POINTER(KernelTimes), cint)
    sig("lio_ndt_create", vp, cint, flt, cint, u64, u64, u32)
    sig("lio_ndt_destroy", None, vp)
    sig("lio_ndt_set_target", cint, vp, f32p, u64)
    sig("lio_ndt_set_target_device", cint, vp, vp, u64)
    sig("lio_ndt_fitness_score", cint, vp, vp, f64p, dbl, f64p, C.POINTER(u32))
    sig("lio_ndt_overlap_score", cint, vp, vp, f64p, dbl, dbl, dbl, f64p, f64p)
    sig("lio_ndt_num_voxels", cint, vp)
    sig("lio_ndt_voxel_at", cint, vp, f32p, f32p, f32p)
    sig("lio_ndt_linearize", cint, vp, vp, f64p, cint, cint, f64p, f64p, f64p, C.POINTER(u32))
    sig("lio_ndt_default_params", None, C.POINTER(NdtParams))
    sig("lio_ndt_align", cint, vp, vp, f64p, C.POINTER(NdtParams), f64p, C.POINTER(cint), C.POINTER(cint))
    sig("lio_ndt_align_batch", cint, vp, C.POINTER(AlignJob), cint, C.POINTER(NdtParams))
    sig("lio_ndt_enable_kernel_timing", cint, vp, cint)
    sig("lio_ndt_kernel_times", cint, vp, C.POINTER(NdtTimes), cint)
    sig("lio_gicp_create", vp, cint, flt, u32, cint)
    sig("lio_gicp_destroy", None, vp)
    sig("lio_gicp_set_target", cint, vp, f32p, u32)
    sig("lio_gicp_set_source", cint, vp, f32p, u32)
    sig("lio_gicp_set_target_device", cint, vp, vp, u32)
    sig("lio_gicp_set_source_device", cint, vp, vp, u32)
    sig("lio_gicp_set_voxel_mode", cint, vp, C.c_double, cint)
    sig("lio_gicp_voxel_at", cint, vp, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double))
    sig("lio_gicp_download", cint, vp, cint, f32p, f64p, u32)
    sig("lio_gicp_correspondences", cint, vp, i32p, u32)
    sig("lio_gicp_neighbours", cint, vp, cint, i32p, u32)
    sig("lio_gicp_mahalanobis", cint, vp, f64p, u32)
    sig("lio_gicp_linearize", cint, vp, f64p, dbl, cint, cint, f64p, f64p, f64p, C.POINTER(u32))
    sig("lio_gicp_align", cint, vp, f64p, C.POINTER(NdtParams), dbl, f64p, C.POINTER(cint), C.POINTER(cint))
    sig("lio_gicp_fitness_score", cint, vp, f64p, dbl, f64p, C.POINTER(u32))
    lp, le, lr = C.POINTER(LoopParams), C.POINTER(LoopEdge), C.POINTER(LoopReport)
    sig("lio_loop_default_params", None, lp)
    sig("lio_loop_find_candidates", cint, f64p, f64p, u32, dbl, f64p, dbl, lp, i32p, u32)
    sig("lio_loop_information_matrix", cint, dbl, f64p)
    sig("lio_loop_create", vp, cint, lp)
    sig("lio_loop_destroy", None, vp)
    sig("lio_loop_reset", cint, vp)
    sig("lio_loop_add_keyframe_host", cint, vp, f32p, u32, f64p, dbl)
    sig("lio_loop_set_pose", cint, vp, cint, f64p)
    sig("lio_loop_num_keyframes", cint, vp, C.POINTER(cint))
    sig("lio_loop_download_keyframe", cint, vp, cint, f32p, f64p, u32)
    sig("lio_loop_detect", cint, vp, le, u32)
    sig("lio_loop_edges", cint, vp, le, u32)
    sig("lio_loop_last_report", cint, vp, lr, i32p, i32p, i32p, f64p, u32)
    sig("lio_loop_last_times", cint, vp, f64p, f64p, f64p, f64p, f64p)
    sig("lio_loop_align_candidates", cint, vp, cint, i32p, u32, f64p, f64p, i32p, i32p, f64p, C.POINTER(u32))
    sig("lio_loop_align_fine", cint, vp, cint, cint, f64p, f64p, i32p, i32p, f64p, C.POINTER(u32))
    sig("lio_loop_pair_information", cint, vp, cint, cint, f64p, f64p, C.POINTER(u32), f64p)
    op, oe = C.POINTER(OverlapParams), C.POINTER(OverlapEdge)
    sig("lio_overlap_default_params", None, vp, op)
    sig("lio_overlap_connection_count", cint, i32p, i32p, u32, C.c_int32, C.c_int32, C.c_int32)
    sig("lio_overlap_find_candidates", cint, f64p, i32p, u32, i32p, i32p, u32, C.c_int32, f64p, op, i32p, u32)
    sig("lio_overlap_create", vp, vp, op)
    sig("lio_overlap_destroy", None, vp)
    sig("lio_overlap_gate_batch", cint, vp, cint, i32p, u32, f64p, dbl, f64p, C.POINTER(u32), C.POINTER(u32))
    sig("lio_overlap_align_pairs", cint, vp, i32p, i32p, u32, f64p, f64p, i32p, i32p)
    sig("lio_overlap_accumulate", cint, vp, cint, i32p, u32)
    sig("lio_overlap_download_accum", cint, vp, f32p, f64p, u32)
    sig("lio_overlap_detect", cint, vp, i32p, i32p, u32, i32p, i32p, u32, i32p, i32p, u32, oe, u32)
    sig("lio_overlap_last_report", cint, vp, u32, C.POINTER(OverlapReport), i32p, f64p, i32p, i32p, f64p, u32)
    sig("lio_overlap_last_times", cint, vp, C.POINTER(OverlapTimes))
    sig("lio_sc_create", vp, cint, u32, u32)
    sig("lio_sc_destroy", None, vp)
    sig("lio_sc_reset", cint, vp)
    sig("lio_sc_num_frames", cint, vp)
    sig("lio_sc_add_frames_host", cint, vp, f32p, C.POINTER(u64), u32)
    sig("lio_sc_download_frame", cint, vp, cint, f64p, f32p, f64p)
    sig("lio_sc_describe_host", cint, vp, f32p, u32, f64p, u32, f64p, f32p, f64p)
    sig("lio_sc_set_active", cint, vp, i32p, C.c_int32)
    sig("lio_sc_distance", cint, vp, f64p, f64p, u32, f64p, i32p)
    sig("lio_sc_search", cint, vp, f64p, f32p, u32, i32p, f64p, i32p, i32p)
    sig("lio_sc_global_search_host", cint, vp, f32p, u32, dbl, i32p, f32p, f64p, i32p)
    sig("lio_sc_shift_to_yaw", flt, C.c_int32)
    sig("lio_sc_last_dropped", cint, vp, C.POINTER(u64))
    sig("lio_sc_last_times", cint, vp, f64p, f64p, f64p)
    gp, gr = C.POINTER(GraphParams), C.POINTER(GraphReport)
    sig("lio_graph_default_params", None, gp)
    sig("lio_graph_create", vp, cint, gp)
    sig("lio_graph_destroy", None, vp)
    sig("lio_graph_reset", cint, vp)
    sig("lio_graph_add_node", cint, vp, f64p)
    sig("lio_graph_set_fixed", cint, vp, cint, cint)
    sig("lio_graph_set_estimate", cint, vp, cint, f64p)
    sig("lio_graph_num_nodes", cint, vp)
    sig("lio_graph_get_fixed", cint, vp, u8p, u32)
    sig("lio_graph_add_edge", cint, vp, cint, cint, f64p, f64p, cint, dbl)
    sig("lio_graph_remove_edge", cint, vp, cint)
    sig("lio_graph_optimize", cint, vp, cint, gr)
    sig("lio_graph_estimates", cint, vp, f64p, u32)
    sig("lio_graph_edges", cint, vp, i32p, i32p, i32p, u32)
    sig("lio_graph_chi2", cint, vp, f64p)
    sig("lio_graph_linearize", cint, vp, f64p, f64p, f64p, u32, f64p, f64p, u32)
    sig("lio_graph_last_times", cint, vp, f64p, f64p, f64p, f64p)
    sig("lio_se3_from_mqt", None, f64p, f64p)
    sig("lio_se3_to_mqt", None, f64p, f64p)
    sig("lio_graph_edge_error", cint, f64p, f64p, f64p, f64p)
    sig("lio_graph_add_prior", cint, vp, cint, cint, f64p, f64p, f64p, cint, dbl)
    sig("lio_graph_set_kernel", cint, vp, cint, cint, dbl)
    sig("lio_graph_priors", cint, vp, i32p, i32p, i32p, f64p, f64p, f64p, i32p, f64p, u32)
    sig("lio_graph_prior_error", cint, f64p, cint, f64p, f64p, f64p)
    sig("lio_graph_remove_gnss_outliers", cint, vp, dbl, cint, i32p, u32, gr)
    sig("lio_graph_remove_node", cint, vp, cint)
    sig("lio_graph_node_live", cint, vp, u8p, u32)
    sig("lio_graph_edge_records", cint, vp, i32p, i32p, i32p, f64p, f64p, i32p, f64p, u32)
    sig("lio_graph_estimate_gnss_moment", cint, vp, dbl, cint, f64p, f64p, gr)
    sig("lio_graph_moment_begin", cint, vp, f64p, f64p)
    sig("lio_graph_moment_end", cint, vp, cint)
    sig("lio_graph_moment_get", cint, vp, f64p)
    sig("lio_graph_moment_linearize", cint, vp, f64p, f64p, f64p, u32)
    sig("lio_loop_retire", cint, vp, cint)
    sig("lio_render_create", vp, cint, u64, u64)
    sig("lio_render_destroy", None, vp)
    sig("lio_render_clear", cint, vp)
    sig("lio_render_set_cameras", cint, vp, cint, C.POINTER(C.c_char_p), f64p, f64p, f64p)
    sig("lio_render_set_active", cint, vp, cint)
    sig("lio_render_frame", cint, vp, f32p, u64, f64p, cint, u32, C.POINTER(RenderImage), cint)
    sig("lio_render_size", cint, vp, C.POINTER(u64), C.POINTER(u64))
    sig("lio_render_download", C.c_int64, vp, f32p, u64)
    sig("lio_render_download_voxels", C.c_int64, vp, i32p, u32p, u32p, u64)
    sig("lio_render_download_points", C.c_int64, vp, f32p, u32p, f32p, f32p, f32p, u64)
    sig("lio_render_download_last_image", C.c_int64, vp, f32p, i32p, u8p, u64, C.POINTER(cint), C.POINTER(cint))
    sig("lio_render_last_times", cint, vp, f64p, f64p, f64p)
    fixp, u64p = C.POINTER(RtkFix), C.POINTER(u64)
    sig("lio_utm_create", vp, cint)
    sig("lio_utm_destroy", None, vp)
    sig("lio_utm_zone", cint, vp)
    sig("lio_utm_forward", cint, vp, dbl, dbl, f64p, f64p)
    sig("lio_utm_inverse", cint, vp, dbl, dbl, f64p, f64p)
    sig("lio_utm_longitude0", dbl, vp)
    sig("lio_grid_convergence", dbl, dbl, dbl, dbl)
    sig("lio_transform_from_rpyt", None, dbl, dbl, dbl, dbl, dbl, dbl, f64p)
    sig("lio_quat_of_transform", None, f64p, f64p)
    sig("lio_interpolate_transform", None, f64p, f64p, dbl, f64p)
    sig("lio_rtk_transform_utm", cint, vp, fixp, f64p, f64p)
    sig("lio_rtk_transform_origin", cint, vp, fixp, fixp, f64p)
    sig("lio_rtk_track_create", vp)
    sig("lio_rtk_track_destroy", None, vp)
    sig("lio_rtk_track_set_origin", cint, vp, fixp, f64p)
    sig("lio_rtk_track_origin", cint, vp, fixp)
    sig("lio_rtk_track_feed", cint, vp, cint, fixp)
    sig("lio_rtk_track_size", cint, vp)
    sig("lio_rtk_track_interpolate", cint, vp, u64, f64p)
    sig("lio_gnss_queue_create", vp)
    sig("lio_gnss_queue_destroy", None, vp)
    sig("lio_gnss_queue_set_origin", cint, vp, fixp, cint, dbl, f64p)
    sig("lio_gnss_queue_push", cint, vp, fixp)
    sig("lio_gnss_queue_size", cint, vp)
    sig("lio_gnss_queue_stamps", cint, vp, u64p, u32)
    sig("lio_gnss_queue_flush", cint, vp, u64p, u8p, u32, f64p, C.POINTER(GnssMatch), u32)
    sig("lio_update_origin", cint, fixp, fixp, f64p, u32, f64p, u32)
    sig("lio_sc_set_positions", cint, vp, f32p, u32)
    sig("lio_sc_local_search", cint, vp, f32p, u32, f64p, dbl, i32p, f32p, f64p, i32p)
    sig("lio_sc_last_local", cint, vp, i32p, f32p, f64p, i32p, i32p)
    sig("lio_scan_merge_create", vp, cint, u32, u64)
    sig("lio_scan_merge_destroy", None, vp)
    sig("lio_scan_merge_set_transform", cint, vp, f64p)
    sig("lio_scan_merge_run_host", cint, vp, u32, C.POINTER(f32p), C.POINTER(C.POINTER(u32)), C.POINTER(u32), u64p, u64, C.POINTER(u32), C.POINTER(u32),
        C.POINTER(u32), u64p)
    sig("lio_scan_merge_download", C.c_int64, vp, f32p, C.POINTER(u32), u64)
    sig("lio_scan_merge_device", vp, vp, C.POINTER(C.POINTER(u32)), u64p)
    sig("lio_scan_merge_last_times", cint, vp, f64p, f64p)
    sig("lio_state_boxplus", None, f64p, f64p, f64p)
    sig("lio_state_boxminus", None, f64p, f64p, f64p)
    i64, i64p = C.c_int64, C.POINTER(C.c_int64)
    dpp, drp, cpp = C.POINTER(DfoParams), C.POINTER(DfoReport), C.POINTER(CalibParams)
    sig("lio_calib_subsample", cint, u64, i64, u8p)
    sig("lio_se3f_exp", None, f32p, f32p)
    sig("lio_se3f_log", None, f32p, f32p)
    sig("lio_se3f_mul", None, f32p, f32p, f32p)
    sig("lio_se3f_inverse", None, f32p, f32p)
    sig("lio_se3f_matrix", None, f32p, f32p)
    sig("lio_se3f_from_matrix", None, f32p, f32p)
    sig("lio_calib_interpolate", cint, i64p, f32p, u32, i64, u32, f32p, u32p)
    sig("lio_dfo_default_params", None, dpp)
    sig("lio_dfo_direct_l", cint, DFO_FN, vp, cint, f64p, f64p, dpp, DFO_HOOK, vp, f64p, drp)
    sig("lio_dfo_nelder_mead", cint, DFO_FN, vp, cint, f64p, f64p, f64p, dpp, DFO_HOOK, vp, f64p, drp)
    sig("lio_calib_default_params", None, cpp)
    sig("lio_calib_ins_create", vp, cint)
    sig("lio_calib_ins_destroy", None, vp)
    sig("lio_calib_ins_reset", cint, vp, f32p)
    sig("lio_calib_ins_add_scan", cint, vp, f32p, u64, u32, i64)
    sig("lio_calib_ins_add_odom", cint, vp, f32p, i64)
    sig("lio_calib_ins_counts", cint, vp, u32p, u32p, u64p)
    sig("lio_calib_ins_set_transform", cint, vp, f64p)
    sig("lio_calib_ins_scan_matrices", cint, vp, dbl, f32p)
    sig("lio_calib_ins_combined", i64, vp, f64p, cint, f32p, u64)
    sig("lio_calib_ins_error", cint, vp, f64p, cint, cint, f64p)
    sig("lio_calib_ins_error_terms", i64, vp, f64p, cint, cint, f32p, u64)
    sig("lio_calib_ins_calibrate", cint, vp, cpp)
    sig("lio_calib_ins_progress", cint, vp, i32p, f64p, i32p)
    sig("lio_calib_ins_result", cint, vp, f32p)
    sig("lio_calib_ins_last_times", cint, vp, f64p, f64p, f64p)
    cgp, cip = C.POINTER(CalibGroundParams), C.POINTER(cint)
    sig("lio_calib_ground_default_params", None, cgp)
    sig("lio_calib_ground_create", vp, cint)
    sig("lio_calib_ground_destroy", None, vp)
    sig("lio_calib_ground_crop_host", cint, vp, f32p, u64, u32, f64p, cint, u32p)
    sig("lio_calib_ground_set_points_host", cint, vp, f32p, u64, u32)
    sig("lio_calib_ground_fit", cint, vp, cgp, u32p, u64, cip, f32p)
    sig("lio_calib_ground_download_indices", i64, vp, u32p, u64)
    sig("lio_calib_ground_download_points", i64, vp, f32p, u64)
    sig("lio_calib_ground_download_draws", i64, vp, u32p, u32p, u32p, f32p, u64)
    sig("lio_calib_ground_last_run", cint, vp, cip, cip, cip, cip, cip)
    sig("lio_calib_ground_last_times", cint, vp, f64p, f64p, f64p, f64p)
    if L.lio_abi_version() >= 27:  # (ABI_REQUIRED stays where callers pin it: an older library simply lacks the lidar-IMU calibration)
        sig("lio_calib_imu_integrate", cint, f64p, f64p, u32, f64p)
        sig("lio_calib_imu_interpolate", cint, f64p, f64p, dbl, f64p)
        sig("lio_calib_imu_time_align", cint, f64p, f64p, u32, f64p, u32, u32p, u32p, f64p)
        sig("lio_calib_imu_solve", cint, f64p, u32, f64p)
        sig("lio_calib_imu_create", vp, cint, u32, u32)
        sig("lio_calib_imu_destroy", None, vp)
        sig("lio_calib_imu_reset", cint, vp)
        sig("lio_calib_imu_add_imu", cint, vp, f64p, u32)
        sig("lio_calib_imu_add_frame", cint, vp, u64, f32p, u32, u32, f64p, f64p)
        sig("lio_calib_imu_lidar_pose", cint, vp, f32p, u32, u32, f64p)
        sig("lio_calib_imu_calibrate", cint, vp, f64p)
        sig("lio_calib_imu_lidar_poses", i64, vp, f64p, u64)
        sig("lio_calib_imu_imu_poses", i64, vp, f64p, u64)
        sig("lio_calib_imu_map_download", i64, vp, f32p, u64)
        sig("lio_calib_imu_target_download", i64, vp, f32p, u64)
        sig("lio_calib_imu_counts", cint, vp, u32p, u32p, u32p, u32p, u32p, cip)
        sig("lio_calib_imu_last_times", cint, vp, f64p, f64p, f64p, f64p)
        sig("lio_calib_imu_set_max_iterations", cint, vp, cint)
    if L.lio_abi_version() >= 28:  # the detection boxes
        sig("lio_boxes_create", vp, cint, u32)
        sig("lio_boxes_destroy", None, vp)
        sig("lio_boxes_pairwise", cint, vp, f32p, u32, f32p, u32, f32p, f32p, f32p, f32p)
        sig("lio_boxes_nms", i64, vp, f32p, f32p, u32, flt, cint, u32, i64p)
        sig("lio_boxes_set_gate", cint, vp, cint)
        sig("lio_boxes_postprocess", i64, vp, f32p, f32p, i32p, u32, f32p, cint, flt, u32, f32p, f32p, i32p)
        sig("lio_boxes_postprocess_device", i64, vp, vp, vp, vp, u32, f32p, cint, flt, u32, f32p, f32p, i32p)
        sig("lio_boxes_last_indices", i64, vp, u32p, u64)
        sig("lio_boxes_last_times", cint, vp, f64p, f64p, f64p, f64p)
    if L.lio_abi_version() >= 29:  # the detection front end
        u16p, u64p = C.POINTER(C.c_uint16), C.POINTER(u64)
        sig("lio_voxelize_grid_size", cint, f32p, f32p, f32p, i32p)
        sig("lio_voxelizer_create", vp, cint, C.POINTER(VoxelizerParams))
        sig("lio_voxelizer_destroy", None, vp)
        sig("lio_voxelizer_reset", cint, vp)
        sig("lio_voxelizer_forward", i64, vp, f32p, u32, f32p, cint)
        sig("lio_voxelizer_forward_device", i64, vp, vp, u32, f32p, cint)
        sig("lio_voxelizer_output", i64, vp, u16p, i32p, u32p, u64)
        sig("lio_voxelizer_output_device", i64, vp, C.POINTER(vp), C.POINTER(vp))
        sig("lio_voxelizer_window", i64, vp, f32p, u64)
        sig("lio_voxelizer_window_counts", i64, vp, i32p, u32)
        sig("lio_voxelizer_window_device", i64, vp, C.POINTER(vp))
        sig("lio_voxelizer_last_counts", cint, vp, u64p, u64p, u64p)
        sig("lio_voxelizer_last_times", cint, vp, f64p, f64p, f64p, f64p, f64p, f64p)
    _lib = L
    return L


class LioError(RuntimeError):
    pass


def check(rc, what=""):
    if rc < 0:
        msg = lib().lio_last_error()
        raise LioError(f"{what}: error {rc}: {msg.decode() if msg else ''}")
    return rc


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))
