"""ctypes binding of libpwclo_hip.so (the C ABI declared in include/pwclo_ops.h).

There is deliberately no CPU or pure-PyTorch fallback: if the library is missing or a launch
fails, the call raises.  ``load()`` never builds anything; run
``python -m pwclonet_pylidarslam_amd.build`` (or ``__graft_entry__.build()``) first.
"""
import contextlib
import ctypes
import gc
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PWCLO_TRACE_LIB=1 (tools/wgtrace.py sets it) loads the developer variant built with the workgroup-trace hooks
LIB_PATH = os.path.join(_HERE, "lib", "libpwclo_hip_trace.so" if os.environ.get("PWCLO_TRACE_LIB", "0") != "0"
                        else "libpwclo_hip.so")

_F = ctypes.c_void_p  # device pointers travel as integers
_i = ctypes.c_int

# name -> argtypes, exactly the prototypes of include/pwclo_ops.h
SIGNATURES = {
    "pwclo_abi_version": ([], _i),
    "pwclo_set_stream": ([ctypes.c_void_p], None),
    "pwclo_get_stream": ([], ctypes.c_void_p),
    "pwclo_last_error": ([], _i),
    "pwclo_last_error_message": ([], ctypes.c_char_p),
    "pwclo_clear_error": ([], None),
    "pwclo_take_launch": ([ctypes.c_char_p, _i, ctypes.POINTER(ctypes.c_int)], _i),
    "pwclo_set_dry_run": ([_i], None),
    "pwclo_fps_large_cloud_launch": ([_i], None),
    "pwclo_fps_large_cloud_exchange": ([_i], None),
    "pwclo_trace_enable": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint], None),
    "pwclo_stream_set_create": ([_i, ctypes.POINTER(ctypes.c_longlong)], _i),
    "pwclo_stream_set_create_ex": ([_i, _i, ctypes.POINTER(ctypes.c_longlong)], _i),
    "pwclo_stream_set_concurrency": ([ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)], _i),
    "pwclo_stream_set_probe": ([ctypes.c_longlong, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint),
                                ctypes.POINTER(ctypes.c_longlong)], _i),
    "pwclo_stream_set_size": ([ctypes.c_longlong], _i),
    "pwclo_stream_set_stream": ([ctypes.c_longlong, _i, ctypes.POINTER(ctypes.c_void_p)], _i),
    "pwclo_stream_set_wait_stream": ([ctypes.c_longlong, _i, ctypes.c_void_p], _i),
    "pwclo_stream_set_record": ([ctypes.c_longlong, _i, _i], _i),
    "pwclo_stream_set_query": ([ctypes.c_longlong, _i], _i),
    "pwclo_stream_set_wait_slot": ([ctypes.c_longlong, _i, ctypes.c_void_p], _i),
    "pwclo_stream_set_synchronize_slot": ([ctypes.c_longlong, _i], _i),
    "pwclo_stream_set_synchronize": ([ctypes.c_longlong], _i),
    "pwclo_stream_set_destroy": ([ctypes.c_longlong], _i),
    "gather_points_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F], None),
    "gather_points_grad_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F], None),
    "furthest_point_sampling_kernel_wrapper": ([_i, _i, _i, _F, _F, _F], None),
    "group_points_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, _F, _F], None),
    "group_points_grad_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, _F, _F], None),
    "query_ball_point_kernel_wrapper": ([_i, _i, _i, ctypes.c_float, _i, _F, _F, _F], None),
    "three_nn_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F], None),
    "three_interpolate_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F], None),
    "three_interpolate_grad_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F], None),
    "knn_point_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F], None),
    "knn_point_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "knn_point_workspace_sections": ([_i, _i, ctypes.POINTER(ctypes.c_longlong)], _i),
    "knn_point_ws_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F, _F], None),
    "knn_point_build_bytes": ([_i, _i], ctypes.c_longlong),
    "knn_point_slabs": ([_i], _i),
    "knn_build_kernel_wrapper": ([_i, _i, _F, _F, _F], None),
    "knn_point_prebuilt_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F], None),
    "knn_point_prebuilt_slice_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F, _i, _i], None),
    "furthest_point_sampling_sorted_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F, _F, _F], None),
    "furthest_point_sampling_slab_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F, _i, _F, _F, _F], None),
    "quat_warp_kernel_wrapper": ([_i, _i, _F, _F, _F, _F], None),
    "sa_fused_kernel_wrapper": ([_i] * 8 + [_F] * 6, None),
    "furthest_point_sampling_xyz_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F], None),
    "furthest_point_sampling_chain_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F, _F, _i, _F], None),
    "hamilton_product_kernel_wrapper": ([_i] * 6 + [_F] * 3, None),
    "quat_warp_pm_kernel_wrapper": ([_i, _i, _F, _F, _F, _F], None),
    "ingest_pairs_kernel_wrapper": ([_i, _i, _F, _F, _F], None),
    "ingest_frames_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F], None),
    "ingest_sequence_kernel_wrapper": ([_i, _i, _i, _i, _F, _F], None),
    "kitti_transform_filter_kernel_wrapper": ([_i, _F, _F, _F, _F], None),
    "kitti360_filter_kernel_wrapper": ([_i, ctypes.c_float, ctypes.c_float, _F, _F, _F], None),
    "fps_spatial_order_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "fps_spatial_order_kernel_wrapper": ([_i, _i, _F, _F, _F, _F], None),
    "softmax_wsum_supported_k": ([_i], _i),
    "softmax_wsum_forward_kernel_wrapper": ([ctypes.c_longlong, _i, _F, _F, _F], None),
    "softmax_wsum_backward_kernel_wrapper": ([ctypes.c_longlong, _i, _F, _F, _F, _F, _F], None),
    "pose_head_train_begin_kernel_wrapper": ([_F], None),
    "pose_head_train_forward_kernel_wrapper": ([_i, _i] + [_F] * 9 + [_i, _i] + [_F] * 9, None),
    "pose_head_train_backward_kernel_wrapper": ([_i, _i] + [_F] * 24, None),
    "compact_frames_scan_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F], None),
    "sweep_filter_compact_kernel_wrapper": ([_i, _i, _i, _F, _F, _i, _F, ctypes.c_float, ctypes.c_float, _F, _F], None),
    "grid_sample_workspace_bytes": ([_i, _i], ctypes.c_longlong),
    "grid_sample_keep_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, ctypes.c_double, _F, _F, _F], None),
    "sweep_filter_grid_compact_kernel_wrapper": ([_i, _i, _i, _F, _F, _i, _F, ctypes.c_float, ctypes.c_float, ctypes.c_double,
                                                 _F, _F, _F, _F], None),
    "deskew_rows_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F, _F, _F], None),
    "sweep_filter_deskew_compact_kernel_wrapper": ([_i, _i, _i, _F, _F, _i, _F, ctypes.c_float, ctypes.c_float, _F, _F, _F,
                                                   _F, _F, _F], None),
    "sweep_filter_deskew_grid_compact_kernel_wrapper": ([_i, _i, _i, _F, _F, _i, _F, ctypes.c_float, ctypes.c_float, _F, _F,
                                                        _F, _F, ctypes.c_double, _F, _F, _F, _F], None),
    "stream_motion_handover_kernel_wrapper": ([_i, _F, _F, _i, _F], None),
    "train_batch_pose_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F, _F, _F], None),
    "train_batch_sample_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, ctypes.c_float, ctypes.c_float, _F, _F, _i, _F, _F, _F,
                                           _F], None),
    "flat_step_entries_per_launch": ([], _i),
    "flat_pack_kernel_wrapper": ([_i, ctypes.POINTER(ctypes.c_void_p)] + [ctypes.POINTER(ctypes.c_longlong)] * 2
                                 + [ctypes.c_float, _F, ctypes.c_longlong], None),
    "flat_adam_kernel_wrapper": ([_i, ctypes.POINTER(ctypes.c_void_p)] + [ctypes.POINTER(ctypes.c_longlong)] * 2
                                 + [_F, _F, _F, ctypes.c_longlong, _F, _F, _F] + [ctypes.c_double] * 4 + [_i], None),
    "flat_adam_skipped_kernel_wrapper": ([_i, ctypes.POINTER(ctypes.c_void_p)] + [ctypes.POINTER(ctypes.c_longlong)] * 2
                                         + [_F, _F, _F, ctypes.c_longlong, _F, _F, _F] + [ctypes.c_double] * 4 + [_i, _F], None),
    "batchnorm_train_workspace_bytes": ([_i], ctypes.c_longlong),
    "batchnorm_train_forward_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, ctypes.c_float, ctypes.c_float, _F, _F, _F, _F,
                                                _F, _F, _i], None),
    "batchnorm_train_forward_devmom_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, ctypes.c_float, _F, _F, _F, _F, _F, _F, _F,
                                                       _i], None),
    "batchnorm_train_backward_kernel_wrapper": ([_i, _i, _i] + [_F] * 10 + [_i], None),
    "batchnorm_train_relu_maxk_forward_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, ctypes.c_float, ctypes.c_float]
                                                         + [_F] * 8, None),
    "batchnorm_train_relu_maxk_forward_devmom_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, ctypes.c_float, _F] + [_F] * 8,
                                                                None),
    "batchnorm_train_relu_maxk_backward_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 12, None),
    "conv1x1_forward_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _i, _F], None),
    "conv1x1_affine_forward_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F, _i, _F], None),
    "conv1x1_affine_maxk_forward_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, _F, _F, _F, _i, _F], None),
    "conv1x1_bnrelu_forward_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 7, None),
    "conv1x1_bnrelu_wgrad_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 8, None),
    "conv1x1_wgrad_workspace_bytes": ([_i, _i, _i, _i], ctypes.c_longlong),
    "conv1x1_stats_workspace_bytes": ([_i, _i, _i, _i], ctypes.c_longlong),
    "conv1x1_dgrad_bnstats_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 11, None),
    "batchnorm_train_backward_apply_kernel_wrapper": ([_i, _i, _i] + [_F] * 9 + [_i], None),
    "conv1x1_forward_bnstats_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 7 + [ctypes.c_float, ctypes.c_float] + [_F] * 5, None),
    "conv1x1_forward_bnstats_devmom_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 7 + [ctypes.c_float, _F] + [_F] * 5, None),
    "batchnorm_train_apply_kernel_wrapper": ([_i, _i, _i] + [_F] * 6 + [_i], None),
    "batchnorm_train_relu_maxk_apply_kernel_wrapper": ([_i, _i, _i, _i] + [_F] * 8, None),
    "conv1x1_wgrad_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F], None),
    "conv1x1_plan_query": ([_i] * 6 + [ctypes.POINTER(ctypes.c_int)], _i),
    "group_points_grad_plan_query": ([_i] * 6 + [ctypes.POINTER(ctypes.c_int)], _i),
    "three_interpolate_grad_plan_query": ([_i] * 5 + [ctypes.POINTER(ctypes.c_int)], _i),
    "group_points_plan_query": ([_i] * 9 + [ctypes.POINTER(ctypes.c_int)], _i),
    "pwclo_group_points_tuning": ([_i] * 4, None),
    "knn_point_plan_query": ([_i] * 6 + [ctypes.POINTER(ctypes.c_int)], _i),
    "furthest_point_sampling_plan_query": ([_i] * 14 + [ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, _i], _i),
    "batchnorm_train_plan_query": ([_i, ctypes.c_longlong, _i, ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int)], _i),
    "group_points_grad_sorted_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, _F, _F, _F], None),
    "xyz_diff_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F, ctypes.c_longlong], None),
    "geometry_encode_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F, ctypes.c_longlong], None),
    "geometry_encode_grad_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, _F, _F, ctypes.c_longlong, _F, _F, _F], None),
    "broadcast_centre_kernel_wrapper": ([_i, _i, _i, _i, _F, _F, ctypes.c_longlong], None),
    "broadcast_centre_grad_kernel_wrapper": ([_i, _i, _i, _i, _F, ctypes.c_longlong, _F], None),
    "group_points_strided_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, _F, _F, ctypes.c_longlong], None),
    "group_points_grad_strided_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, ctypes.c_longlong, _F, _F], None),
    "group_points_grad_sorted_strided_kernel_wrapper": ([_i, _i, _i, _i, _i, _F, ctypes.c_longlong, _F, _F, _F], None),
    "upconv_fused_kernel_wrapper": ([_i] * 4 + [_F] * 6, None),
    "pointwise_fused_kernel_wrapper": ([_i] * 7 + [_F] * 5, None),
    "pointwise_tail_fused_kernel_wrapper": ([_i] * 8 + [_F] * 7 + [_i], None),
    "cv_fused_a1_kernel_wrapper": ([_i] * 5 + [_F] * 7 + [_i], None),
    "cv_fused_a2_kernel_wrapper": ([_i] * 4 + [_F] * 6 + [_i] * 3, None),
    "cv_fused_b_kernel_wrapper": ([_i] * 4 + [_F] * 6, None),
    "masked_pool_kernel_wrapper": ([_i, _i, _F, _F, _F], None),
    "pose_head_fused_kernel_wrapper": ([_i, _i] + [_F] * 13 + [_i], None),
    "pose_head_warp_fused_kernel_wrapper": ([_i, _i] + [_F] * 13 + [_i, _i, _F, _F], None),
    "linear_jobs_kernel_wrapper": ([_i] + [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.POINTER(ctypes.c_void_p)] * 3
                                   + [ctypes.POINTER(ctypes.c_int)], None),
    "sa_fused_h_kernel_wrapper": ([_i] * 7 + [_F] * 6 + [_i] * 3, None),
    "upconv_fused_h_kernel_wrapper": ([_i] * 4 + [_F] * 6 + [_i] * 2, None),
    "upconv_post_fused_h_kernel_wrapper": ([_i] * 6 + [_F] * 4 + [ctypes.POINTER(ctypes.c_void_p)] * 4 + [_i] * 2, None),
    "cv_fused_a1_h_kernel_wrapper": ([_i] * 4 + [_F] * 7 + [_i] * 3, None),
    "cv_fused_a_lane6_kernel_wrapper": ([_i] * 3 + [_F] * 10 + [_i] * 3, None),
    "cv_fused_b_h_kernel_wrapper": ([_i] * 3 + [_F] * 7 + [_i] * 2, None),
    "pwclo_pack_layers_kernel_wrapper": ([_F, _i, _i], None),
    "odom_rows_to_transforms_kernel_wrapper": ([_i, _i, _F, _F, _i], None),
    "odom_accumulate_kernel_wrapper": ([_i, _F, _F, _F], None),
    "odom_cumulative_distance_kernel_wrapper": ([_i, _F, _F, _F], None),
    "stream_append_masked_kernel_wrapper": ([_i, _i] + [_F] * 9, None),
    "stream_handover_max_segments": ([], _i),
    "stream_handover_masked_kernel_wrapper": ([_i] + [ctypes.POINTER(ctypes.c_void_p)] * 2
                                              + [ctypes.POINTER(ctypes.c_longlong)] * 3 + [_i, _F], None),
    "odom_sequence_errors_kernel_wrapper": ([_i, _i] + [_F] * 5 + [_i, _i] + [_F] * 3, None),
    "icp_normals_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F], None),
    "icp_queries_kernel_wrapper": ([_i, _i, _i, _F, _F, _F, _F], None),
    "icp_accumulate_groups": ([_i], _i),
    "icp_accumulate_kernel_wrapper": ([_i, _i, _i] + [_F] * 9 + [ctypes.c_double, ctypes.c_float, _F], None),
    "icp_solve_kernel_wrapper": ([_i, _i, _i, _F, ctypes.c_double, ctypes.c_double, _i] + [_F] * 7, None),
    "icp_map_push_kernel_wrapper": ([_i, _i, _i] + [_F] * 11, None),
    "icp_begin_kernel_wrapper": ([_i, _i] + [_F] * 7, None),
    "icp_queries_masked_kernel_wrapper": ([_i, _i, _i] + [_F] * 5, None),
    "icp_accumulate_masked_kernel_wrapper": ([_i, _i, _i] + [_F] * 9 + [ctypes.c_double, ctypes.c_float, _F, _F], None),
    "icp_solve_masked_kernel_wrapper": ([_i, _i, _i, _F, ctypes.c_double, ctypes.c_double, _i] + [_F] * 8, None),
    "icp_map_push_masked_kernel_wrapper": ([_i, _i, _i] + [_F] * 12, None),
    "stream_record_refined_kernel_wrapper": ([_i, _i] + [_F] * 6, None),
    "proj_vertex_map_workspace_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "proj_vertex_map_kernel_wrapper": ([_i] * 5 + [ctypes.c_double] * 2 + [_F] * 6, None),
    "proj_normal_map_kernel_wrapper": ([_i, _i, _i, _i, _F, _F], None),
    "proj_model_build_workspace_bytes": ([_i, _i, _i, _i], ctypes.c_longlong),
    "proj_model_build_kernel_wrapper": ([_i] * 4 + [ctypes.c_double] * 2 + [_F] * 8, None),
    "proj_accumulate_kernel_wrapper": ([_i] * 4 + [ctypes.c_double] * 2 + [_F] * 4 + [ctypes.c_double, ctypes.c_float]
                                       + [_F] * 3, None),
    "proj_map_push_kernel_wrapper": ([_i] * 4 + [_F] * 8, None),
    "keyframe_gate_kernel_wrapper": ([_i, _i, _F, _F, _F, ctypes.c_double, ctypes.c_double, _F, _F, _F], None),
    "keyframe_icp_push_kernel_wrapper": ([_i, _i, _i] + [_F] * 13, None),
    "stream_motion_from_refined_kernel_wrapper": ([_i, _F, _F, _F, _F], None),
    "voxel_map_bytes": ([_i, _i, _i, _i], ctypes.c_longlong),
    "voxel_begin_kernel_wrapper": ([_i] * 4 + [_F] * 7, None),
    "voxel_insert_kernel_wrapper": ([_i] * 5 + [ctypes.c_double] + [_F] * 10, None),
    "voxel_pose_kernel_wrapper": ([_i] + [_F] * 7, None),
    "voxel_accumulate_kernel_wrapper": ([_i] * 5 + [ctypes.c_double] + [_F] * 4 + [ctypes.c_double, ctypes.c_float] + [_F] * 5,
                                        None),
    "pose_graph_begin_kernel_wrapper": ([_i] * 3 + [_F] * 9, None),
    "pose_graph_append_kernel_wrapper": ([_i, _i] + [_F] * 12, None),
    "pose_graph_linearise_kernel_wrapper": ([_i] * 4 + [_F] * 15, None),
    "pose_graph_linearise_robust_kernel_wrapper": ([_i] * 6 + [ctypes.c_double] + [_F] * 15, None),
    "pose_graph_edge_weights_kernel_wrapper": ([_i] * 6 + [ctypes.c_double] + [_F] * 10, None),
    "pose_graph_solve_kernel_wrapper": ([_i] * 7 + [ctypes.c_double] + [_F] * 19 + [_i], None),
    "pose_graph_retract_kernel_wrapper": ([_i] * 3 + [_F] * 6, None),
    "pose_graph_judge_kernel_wrapper": ([_i] * 6 + [_F] * 18 + [_i], None),
    "scan_context_build_kernel_wrapper": ([_i] * 5 + [ctypes.c_float] + [_F] * 12, None),
    "loop_score_kernel_wrapper": ([_i] * 4 + [_F] * 8 + [_i, _F, _i, ctypes.c_double, _F, _F], None),
    "loop_select_kernel_wrapper": ([_i] * 4 + [ctypes.c_float] + [_F] * 13, None),
    "loop_fetch_kernel_wrapper": ([_i] * 3 + [_F] * 4, None),
    "loop_accept_kernel_wrapper": ([_i] * 3 + [_F] * 8 + [ctypes.c_double] * 2 + [_F] * 6, None),
    "loop_insert_kernel_wrapper": ([_i] * 5 + [_F] * 10, None),
    "elevation_image_kernel_wrapper": ([_i] * 6 + [ctypes.c_float] * 3 + [_F] * 9, None),
    "elevation_score_kernel_wrapper": ([_i] * 5 + [_F] * 5, None),
    "elevation_choose_kernel_wrapper": ([_i] * 6 + [ctypes.c_float] * 2 + [_F] * 8, None),
    "global_map_bytes": ([_i] * 4, ctypes.c_longlong),
    "global_map_begin_kernel_wrapper": ([_i] * 6 + [_F] * 8, None),
    "global_map_push_kernel_wrapper": ([_i] * 3 + [_F] * 3, None),
    "global_map_clear_kernel_wrapper": ([_i] * 3 + [_F] * 3, None),
    "global_map_insert_kernel_wrapper": ([_i] * 4 + [ctypes.c_double, _F, _i] + [_F] * 7, None),
    "global_map_count_kernel_wrapper": ([_i] * 4 + [_F] * 6, None),
    "global_map_scan_kernel_wrapper": ([_i] * 3 + [_F] * 2, None),
    "global_map_write_kernel_wrapper": ([_i] * 5 + [_F, _i] + [_F] * 10, None),
    "global_map_end_kernel_wrapper": ([_i, _F], None),
    "map_localize_index_bytes": ([_i, ctypes.c_longlong], ctypes.c_longlong),
    "map_index_kernel_wrapper": ([_i, ctypes.c_longlong, _i, ctypes.c_double] + [_F] * 4 + [_i, _i, _F, _F, _F], None),
    "map_localize_begin_kernel_wrapper": ([_i, _F, _F, _F], None),
    "map_localize_accumulate_kernel_wrapper": ([_i, _i, ctypes.c_longlong, _i, ctypes.c_double, _i] + [_F] * 4 + [_i]
                                               + [_F] * 4 + [ctypes.c_double, ctypes.c_float, _i] + [_F] * 6, None),
}

_lib = None


def load():
    """Load the shared library and declare every prototype.  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libpwclo_hip.so is not built (%s missing). Build it with "
                "`python -m pwclonet_pylidarslam_amd.build`; there is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = header and library out of sync
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def check(what):
    """Raise if the previous launch recorded an error (the reference would exit(-1))."""
    lib = _lib
    code = lib.pwclo_last_error()
    if code != 0:
        msg = lib.pwclo_last_error_message().decode("utf-8", "replace")
        lib.pwclo_clear_error()
        raise RuntimeError("%s failed (error %d): %s" % (what, code, msg))


def capture(graph, **kw):
    """``torch.cuda.graph(graph, **kw)`` after a full garbage collection.  torch (2.9 on) no longer collects before a
    capture, so a dead Python cycle that holds captured graphs or device memory -- the traceback of a failed call keeps
    its frame's locals in one -- would be freed by the automatic collector whenever it next runs, possibly in the middle
    of this capture, where destroying another graph aborts the process.  Collected here, it is freed outside every
    capture, like any object that goes out of scope."""
    gc.collect()
    return torch.cuda.graph(graph, **kw)


def synchronize(device=None):
    """Wait for the device and raise if a kernel that has run reported a device-side failure (e.g. the
    cooperative large-cloud sampler timing out: PWCLO_ECOOP_TIMEOUT).  Launches are asynchronous, so such a
    failure surfaces at the next library call made after the kernel ran, or here."""
    load()
    torch.cuda.synchronize(device)
    check("device-side check after synchronize")


# Optional launch profiler (bench.py / tools): an object with .add(name, meta, start_evt, end_evt).
# Wrappers describe the next launch's algorithmic work with annotate(); both are no-ops otherwise.  When the wrapper
# launched through the library's launch layer, the profiler's meta also carries kernel=<the instantiation launched>.
profiler = None
_meta = None


def annotate(**meta):
    """Algorithmic work of the NEXT launch (flops / bytes / units), consumed by the profiler."""
    global _meta
    _meta = meta


_fn_cache = {}

# Inside ``launches()``: the list its caller reads, and whether the library is in dry-run mode.
_recording = None
_dry = False


@contextlib.contextmanager
def launches(dry=False):
    """Yields a list to which every ``call()`` inside appends ``(wrapper name, kernel name, waves, (grid x, grid y), lds
    bytes)`` when the wrapper launched through the library's launch layer (include/pwclo_ops.h: pwclo_take_launch) --
    what the library DID launch, named as rocprofv3 names it.  ``dry=True`` sets the library's dry-run flag and skips
    the stream lookups: the wrappers' whole dispatch runs, nothing is launched, and the tensors may live on the CPU
    (outputs stay uninitialised).  Only for calls of the recorded kernels: other entry points ignore the flag."""
    global _recording, _dry
    lib = load()
    saved = _recording, _dry
    _recording, _dry = [], bool(dry)
    lib.pwclo_set_dry_run(int(_dry))
    try:
        yield _recording
    finally:
        _recording, _dry = saved
        lib.pwclo_set_dry_run(int(_dry))


def _observed(name, device, launch, set_stream, args):
    """``call()`` under a profiler or inside ``launches()``: the launch between two takes of the launch record."""
    take = _lib.pwclo_take_launch
    take(None, 0, None)                                  # whatever an earlier call left behind
    timed = profiler is not None and not _dry
    if _dry:
        launch(*args)
    else:
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            set_stream(stream.cuda_stream)
            if timed:   # HIP events on the very stream the kernel is launched on
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(stream)
            launch(*args)
            if timed:
                e.record(stream)
    buf, geo = ctypes.create_string_buffer(256), (ctypes.c_int * 4)()
    took = take(buf, len(buf), geo)
    kernel = buf.value.decode() if took else None
    if timed:
        profiler.add(name, dict(_meta or {}, kernel=kernel) if took else _meta, s, e)
    if took and _recording is not None:
        _recording.append((name, kernel, geo[0], (geo[1], geo[2]), geo[3]))


def call(name, device, *args):
    """Launch `name` on torch's current stream of `device` and check the sticky error.
    (The host cost of this function is the floor of every eager launch: function pointers are looked up once, the device
    guard is skipped when `device` already is the current one, and the launch record is taken only under a profiler or
    inside ``launches()``.)"""
    global _meta
    fn = _fn_cache.get(name)
    if fn is None:
        lib = load()
        fn = _fn_cache[name] = (getattr(lib, name), lib.pwclo_set_stream, lib.pwclo_last_error)
    launch, set_stream, last_error = fn
    if profiler is not None or _recording is not None:
        _observed(name, device, launch, set_stream, args)
    else:
        idx = device.index if isinstance(device, torch.device) and device.index is not None else None
        if idx is None or idx == torch.cuda.current_device():
            set_stream(torch.cuda.current_stream().cuda_stream)
            launch(*args)
        else:
            with torch.cuda.device(device):
                set_stream(torch.cuda.current_stream(device).cuda_stream)
                launch(*args)
    _meta = None
    if last_error() != 0:
        check(name)
