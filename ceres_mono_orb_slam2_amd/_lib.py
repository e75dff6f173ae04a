"""ctypes loader for the in-tree HIP C-ABI library (include/orbslam_hip.h).

There is no CPU fallback: if the library is missing or a call fails the product raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBHIP_LIB") or os.path.join(_HERE, "lib", "liborbslam_hip.so")   # (ORBHIP_LIB: a profiling / experiment build)

# every symbol include/orbslam_hip.h declares (tests check that the library exports them all)
SYMBOLS = [
    "orbhip_last_error", "orbhip_device_count", "orbhip_version", "orbhip_set_default_device", "orbhip_get_default_device", "orbhip_set_thread_priority", "orbhip_copy_pinned_async", "orbl_create_new_map_points", "orbl_fuse_batch", "orbl_update_map_points", "orbl_update_map_points_device", "orbl_update_map_points_workspace", "orbl_keyframe_culling", "orbl_keyframe_culling_device", "orbl_keyframe_culling_workspace",
    "orbl_update_connections", "orbl_update_connections_device", "orbl_update_connections_workspace",
    "orbl_set_bad_keyframes", "orbl_set_bad_keyframes_device", "orbl_set_bad_keyframes_workspace",
    "orbl_apply_map_edits", "orbl_apply_map_edits_device", "orbl_apply_map_edits_workspace",
    "orbl_fuse_targets", "orbl_fuse_targets_device", "orbl_fuse_targets_workspace", "orbl_fuse_rows", "orbl_fuse_rows_device", "orbl_fuse_rows_workspace",
    "orbl_fuse_candidates", "orbl_fuse_candidates_device", "orbl_fuse_candidates_workspace",
    "orbl_update_map_points_on_tables", "orbl_update_map_points_on_tables_device", "orbl_update_map_points_on_tables_workspace",
    "orbl_correct_loop", "orbl_correct_loop_device", "orbl_correct_loop_workspace",
    "orbl_propagate_global_ba", "orbl_propagate_global_ba_device", "orbl_propagate_global_ba_workspace",
    "orbl_local_ba_assemble", "orbl_local_ba_assemble_device", "orbl_local_ba_assemble_workspace",
    "orbl_local_ba_apply", "orbl_local_ba_apply_device", "orbl_local_ba_apply_workspace",
    "orbl_essential_graph_assemble", "orbl_essential_graph_assemble_device", "orbl_essential_graph_assemble_workspace",
    "orbl_essential_graph_apply", "orbl_essential_graph_apply_device", "orbl_essential_graph_apply_workspace",
    "orbl_global_ba_assemble", "orbl_global_ba_assemble_device", "orbl_global_ba_assemble_workspace",
    "orbl_global_ba_apply", "orbl_global_ba_apply_device", "orbl_global_ba_apply_workspace",
    "orbt_relocalization_search_by_bow", "orbt_relocalization_refine",
    "orbt_initialize", "orbt_initialize_batch_device", "orbt_initialize_workspace",
    "orbt_pnp_ransac_params", "orbt_pnp_iterate", "orbt_pnp_iterate_batch_device", "orbt_pnp_iterate_workspace",
    "orbt_sim3_ransac_params", "orbt_sim3_iterate", "orbt_sim3_iterate_batch_device", "orbt_sim3_iterate_workspace",
    "orbx_create", "orbx_destroy", "orbx_get_levels", "orbx_set_opencv_variant", "orbx_get_tables", "orbx_max_keypoints", "orbx_extract",
    "orbx_extract_batch_device", "orbx_set_profiling", "orbx_get_stage_ms", "orbx_get_level_image", "orbx_get_level_candidates", "orbx_get_level_selected",
    "orbm_descriptor_distance", "orbm_hamming_best2_device", "orbm_hamming_best2", "orbm_match_frames_batch_device",
    "orbm_search_for_initialization", "orbm_search_by_projection", "orbm_search_by_sim3", "orbm_search_by_bow", "orbm_search_for_triangulation",
    "orbv_create", "orbv_destroy", "orbv_load_text", "orbv_parse_text", "orbv_free_parsed", "orbv_transform", "orbv_descend_device", "orbv_score_l1",
    "orbv_db_create", "orbv_db_destroy", "orbv_db_clear", "orbv_db_add", "orbv_db_erase", "orbv_db_size", "orbv_db_set_best_covisibles", "orbv_db_get_state",
    "orbv_db_min_score", "orbv_db_detect_loop_candidates", "orbv_db_detect_relocalization_candidates", "orbv_db_detect_loop_candidates_begin",
    "orbv_db_detect_relocalization_candidates_begin", "orbv_db_detect_candidates_finish", "orbv_db_pending_fields", "orbv_db_detect_loop_candidates_batch_device",
    "orbv_db_detect_relocalization_candidates_batch_device", "orbv_db_detect_workspace",
    "orbm_undistort_keypoints", "orbm_assign_features_to_grid", "orbm_features_in_area", "orbm_is_in_frustum", "orbm_is_in_frustum_gates",
    "orbm_triangulate_matches", "orbt_track_with_motion_model", "orbt_track_local_map", "orbt_track_reference_keyframe", "orbt_last_call_ms",
    "orbt_track_local_map_device", "orbt_update_local_keyframes", "orbt_update_local_points", "orbt_update_local_map_device", "orbt_update_local_map_workspace",
    "orbt_image_bounds", "orbt_set_distortion", "orbt_last_undistorted_keypoints",
    "ba_pose_optimization", "ba_pose_optimization_batch_device", "ba_solve", "ba_check_outlier",
    "ba_local_bundle_adjustment", "ba_optimize_sim3", "ba_optimize_sim3_batch_device", "ba_sim3_exp", "ba_sim3_log", "ba_sim3_mul", "ba_sim3_inverse",
    "ba_solve_batch", "ba_local_bundle_adjustment_batch", "ba_optimize_essential_graph", "ba_essential_graph_correct",
    "ba_matrix4d_to_pose7", "ba_pose7_to_matrix4d", "ba_set_profiling", "ba_get_profile", "ba_get_last_plan", "ba_set_wait_limit_ms",
    "orbl_fuse_batch_sim3", "orbhip_comm_get_unique_id", "orbhip_comm_create", "orbhip_comm_adopt", "orbhip_comm_info", "orbhip_comm_destroy", "orbhip_allgather_landmarks",
]


class BaProblem(C.Structure):                 # ba_problem
    _fields_ = [("K4", C.c_void_p), ("poses7", C.c_void_p), ("cam_fixed", C.c_void_p), ("ncam", C.c_int32),
                ("pts3", C.c_void_p), ("npts", C.c_int32), ("obs_cam", C.c_void_p), ("obs_pt", C.c_void_p),
                ("obs_uv", C.c_void_p), ("obs_weight", C.c_void_p), ("obs_robust", C.c_void_p), ("nobs", C.c_int32)]


class BaLocalProblem(C.Structure):            # ba_local_problem
    _fields_ = [("K4", C.c_void_p), ("poses7", C.c_void_p), ("cam_fixed", C.c_void_p), ("cam_local", C.c_void_p),
                ("ncam", C.c_int32), ("pts3", C.c_void_p), ("npts", C.c_int32), ("obs_cam", C.c_void_p),
                ("obs_pt", C.c_void_p), ("obs_uv", C.c_void_p), ("obs_inv_sigma2", C.c_void_p), ("nobs", C.c_int32),
                ("obs_erase", C.c_void_p)]


class OrbHipError(RuntimeError):
    pass


class InitReport(C.Structure):                # orbt_init_report
    _fields_ = [("model", C.c_int32), ("reason", C.c_int32), ("score_h", C.c_float), ("score_f", C.c_float), ("rh", C.c_float),
                ("best_h", C.c_int32), ("best_f", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("motion", C.c_int32),
                ("n_good", C.c_int32 * 8), ("parallax", C.c_float * 8)]


class InitTrace(C.Structure):                 # orbt_init_trace
    _fields_ = [("H21", C.c_void_p), ("H12", C.c_void_p), ("F21", C.c_void_p), ("score_h", C.c_void_p), ("score_f", C.c_void_p),
                ("motion_R", C.c_void_p), ("motion_t", C.c_void_p), ("inliers_h", C.c_void_p), ("inliers_f", C.c_void_p)]


class PnpParams(C.Structure):                 # orbt_pnp_params
    _fields_ = [("n", C.c_int32), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("epsilon", C.c_float)]


class PnpResult(C.Structure):                 # orbt_pnp_result
    _fields_ = [("status", C.c_int32), ("consumed", C.c_int32), ("n_inliers", C.c_int32), ("n_refits", C.c_int32), ("Tcw", C.c_double * 16)]


class PnpTrace(C.Structure):                  # orbt_pnp_trace
    _fields_ = [("R", C.c_void_p), ("t", C.c_void_p), ("approx", C.c_void_p), ("rep_error", C.c_void_p), ("count", C.c_void_p),
                ("refit_iteration", C.c_void_p), ("refit_R", C.c_void_p), ("refit_t", C.c_void_p), ("refit_count", C.c_void_p)]


class Sim3Params(C.Structure):                # orbt_sim3_params
    _fields_ = [("n", C.c_int32), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("reserved", C.c_int32)]


class Sim3Result(C.Structure):                # orbt_sim3_result
    _fields_ = [("status", C.c_int32), ("consumed", C.c_int32), ("n_inliers", C.c_int32), ("scale", C.c_float), ("T12", C.c_double * 16),
                ("R", C.c_double * 9), ("t", C.c_double * 3)]


class Sim3Trace(C.Structure):                 # orbt_sim3_trace
    _fields_ = [("R", C.c_void_p), ("t", C.c_void_p), ("scale", C.c_void_p), ("count", C.c_void_p), ("relgap", C.c_void_p)]


class DbQueryInfo(C.Structure):              # orbv_db_query_info
    _fields_ = [("max_common", C.c_int32), ("n_sharing", C.c_int32), ("n_scored", C.c_int32), ("n_kept", C.c_int32), ("n_cand", C.c_int32),
                ("status", C.c_int32), ("best_acc", C.c_float), ("min_common", C.c_int32)]


class DbTrace(C.Structure):                  # orbv_db_trace
    _fields_ = [("info", C.POINTER(DbQueryInfo)), ("kept_slot", C.c_void_p), ("kept_score", C.c_void_p), ("kept_acc", C.c_void_p),
                ("kept_best", C.c_void_p), ("kept_cap", C.c_int32), ("reserved", C.c_int32)]


class BaOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("huber_delta", C.c_double), ("fix_points", C.c_int32),
                ("stop_flag", C.c_void_p)]


class BaSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int32),
                ("successful_steps", C.c_int32), ("termination", C.c_int32), ("final_radius", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def load():
    """Load liborbslam_hip.so (built by __graft_entry__.build()); raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrbHipError("HIP library %s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    # PyTorch (device memory / streams / torch.distributed plumbing) bundles its own libamdhip64.so.7;
    # load it FIRST so this library binds to the same HIP runtime instead of a second copy from
    # /opt/rocm (two runtimes in one process cannot both own the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, f64, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
    L.orbhip_last_error.restype = C.c_char_p
    L.orbhip_version.restype = C.c_char_p
    L.orbx_create.argtypes = [i32, f32, i32, i32, i32, i32, C.POINTER(vp)]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_tables.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbx_max_keypoints.argtypes = [vp]
    L.orbx_extract.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, C.POINTER(i32)]
    L.orbx_extract_batch_device.argtypes = [vp, vp, i32, i32, i32, sz, i32, vp, vp, i32, vp, vp]
    L.orbx_set_profiling.argtypes = [vp, i32]
    L.orbx_get_stage_ms.argtypes = [vp, vp, C.POINTER(i32)]
    L.orbx_get_level_image.argtypes = [vp, i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.orbx_get_level_candidates.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.orbx_get_level_selected.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.orbm_descriptor_distance.argtypes = [vp, vp]
    L.orbm_hamming_best2_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.orbm_hamming_best2.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.orbm_match_frames_batch_device.argtypes = [vp, vp, vp, i32, vp, vp, i32, f32, i32, i32, vp, vp, vp]
    L.orbm_search_for_initialization.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, i32, f32, i32, vp, C.POINTER(i32)]
    L.orbm_search_by_projection.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, i32, f32, i32, i32,
                                            vp, vp, C.POINTER(i32)]
    L.orbm_search_by_sim3.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
    L.orbm_search_by_bow.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, i32, i32, i32, vp,
                                     C.POINTER(i32)]
    L.orbm_search_for_triangulation.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, f32, f32, vp, vp,
                                                i32, vp, C.POINTER(i32)]
    L.orbv_create.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(vp)]
    L.orbv_destroy.argtypes = [vp]
    L.orbv_load_text.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.orbv_parse_text.argtypes = [C.c_char_p] + [C.POINTER(i32)] * 6 + [C.POINTER(vp)] * 5
    L.orbv_free_parsed.argtypes = [vp]
    L.orbv_free_parsed.restype = None
    L.orbv_transform.argtypes = [vp, vp, i32, i32, vp, vp, C.POINTER(i32), vp, vp, vp, C.POINTER(i32)]
    L.orbv_descend_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    L.orbv_score_l1.argtypes = [vp, vp, i32, vp, vp, i32]
    L.orbv_score_l1.restype = f64
    L.orbm_undistort_keypoints.argtypes = [vp, i32, vp, vp, vp]
    L.orbm_assign_features_to_grid.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.orbm_features_in_area.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, i32, C.POINTER(i32)]
    L.orbm_triangulate_matches.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, f32, vp, vp]
    L.orbm_is_in_frustum.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, i32, vp, vp, vp, vp]
    L.orbt_last_call_ms.argtypes = []; L.orbt_last_call_ms.restype = C.c_double
    L.orbt_track_with_motion_model.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.orbt_image_bounds.argtypes = [i32, i32, vp, vp, vp]
    L.orbt_set_distortion.argtypes = [vp, vp]
    L.orbt_last_undistorted_keypoints.argtypes = [vp, vp, i32, C.POINTER(i32)]
    L.orbx_set_opencv_variant.argtypes = [vp, i32]
    L.orbt_track_reference_keyframe.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, i32, vp, vp, i32, vp, vp, C.POINTER(i32), vp, vp, vp,
                                                C.POINTER(i32), vp, vp, vp, vp]
    L.orbt_track_local_map.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp]
    L.orbt_track_local_map_device.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp]
    L.orbt_relocalization_refine.argtypes = [vp, vp, vp, f32, vp, i32, i32, i32, i32, vp, vp, vp, C.POINTER(i32)]
    L.orbt_update_local_keyframes.argtypes = [i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), vp]
    L.orbt_update_local_points.argtypes = [i32, vp, vp, i32] + [vp] * 7 + [i32, vp, i32, vp, i32, vp, C.POINTER(i32)] + [vp] * 8
    L.orbt_update_local_map_device.argtypes = [i32, vp, i32, vp, i32, vp, i32, vp, vp, i32] + [vp] * 7 + [i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp,
                                               i32, i32, i32] + [vp] * 16
    L.orbt_update_local_map_workspace.argtypes = [i32, i32, i32, C.POINTER(sz)]
    L.orbm_is_in_frustum_gates.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp]
    L.ba_pose_optimization.argtypes = [vp, vp, vp, vp, vp, i32, vp, C.POINTER(i32), C.POINTER(BaSummary)]
    L.ba_pose_optimization_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.ba_solve.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(BaOptions),
                           C.POINTER(BaSummary)]
    L.ba_check_outlier.argtypes = [vp, vp, vp, vp, f64, f64, vp]
    L.ba_local_bundle_adjustment.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, i32, vp,
                                             C.POINTER(i32), C.POINTER(BaSummary), C.POINTER(BaSummary)]
    L.ba_optimize_sim3.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f64, i32, vp, C.POINTER(i32), C.POINTER(BaSummary)]
    L.ba_optimize_sim3_batch_device.argtypes = [vp] * 11 + [i32, vp, vp, vp, vp]
    L.ba_sim3_exp.argtypes = [vp, vp]
    L.ba_sim3_log.argtypes = [vp, vp]
    L.ba_sim3_mul.argtypes = [vp, vp, vp]; L.ba_sim3_inverse.argtypes = [vp, vp]
    L.ba_optimize_essential_graph.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, vp, C.POINTER(BaSummary)]
    L.ba_essential_graph_correct.argtypes = [vp, vp, i32, vp, vp, vp, i32]
    L.ba_matrix4d_to_pose7.argtypes = [vp, vp]
    L.ba_pose7_to_matrix4d.argtypes = [vp, vp]
    L.ba_set_profiling.argtypes = [i32]
    L.ba_get_profile.argtypes = [C.POINTER(f64), C.POINTER(i32), C.POINTER(i32)]
    L.ba_get_last_plan.argtypes = [C.POINTER(i32)]
    L.orbhip_comm_get_unique_id.argtypes = [vp]
    L.orbhip_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.orbhip_comm_adopt.argtypes = [vp, i32, C.POINTER(vp)]
    L.orbhip_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.orbhip_comm_destroy.argtypes = [vp]
    L.orbhip_allgather_landmarks.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, vp, C.POINTER(i32), vp]
    L.ba_set_wait_limit_ms.argtypes = [C.c_double]
    L.orbhip_copy_pinned_async.argtypes = [vp, vp, C.c_size_t, vp]
    L.orbl_update_map_points_workspace.argtypes = [i32, vp]
    L.orbl_keyframe_culling.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, f64, vp, vp, vp, vp, vp, vp]
    L.orbl_keyframe_culling_device.argtypes = [i32, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbl_keyframe_culling_workspace.argtypes = [i32, i32, i32, i32, C.POINTER(sz)]
    L.orbl_update_connections.argtypes = [i32, vp, vp, vp, vp, i32, i32] + [vp] * 9 + [i32] * 5 + [vp] * 12
    L.orbl_update_connections_device.argtypes = [i32, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp] + [i32] * 5 + [vp] * 15
    L.orbl_update_connections_workspace.argtypes = [i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.orbl_set_bad_keyframes.argtypes = [i32, vp, vp, vp, i32] + [vp] * 12 + [i32] + [vp] * 9 + [i32, i32] + [vp] * 11
    L.orbl_set_bad_keyframes_device.argtypes = ([i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32] + [vp] * 5 + [i32] +
                                                [vp] * 4 + [i32, i32] + [vp] * 14)
    L.orbl_set_bad_keyframes_workspace.argtypes = [i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.orbl_apply_map_edits.argtypes = [i32] + [vp] * 5 + [i32] + [vp] * 5 + [i32] + [vp] * 9 + [i32] + [vp] * 10
    L.orbl_apply_map_edits_device.argtypes = [i32] + [vp] * 5 + [i32, vp, vp, i32, vp, vp, vp, i32] + [vp] * 5 + [i32] + [vp] * 4 + [i32] + [vp] * 13
    L.orbl_apply_map_edits_workspace.argtypes = [i32, i32, i32, i32, i32, C.POINTER(sz)]
    L.orbl_fuse_targets.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.orbl_fuse_targets_device.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, i32, i32, i32] + [vp] * 5
    L.orbl_fuse_targets_workspace.argtypes = [i32, C.POINTER(sz)]
    L.orbl_fuse_rows.argtypes = [i32, i32, vp, i32] + [vp] * 8 + [i32] + [vp] * 7 + [f32, i32, f32] + [vp] * 9
    L.orbl_fuse_rows_device.argtypes = [vp, i32, vp, i32] + [vp] * 5 + [i32, vp, vp, vp, i32] + [vp] * 7 + [f32, i32, f32] + [vp] * 12
    L.orbl_fuse_rows_workspace.argtypes = [i32, C.POINTER(sz)]
    L.orbl_fuse_candidates.argtypes = [i32, vp, i32, vp, vp, i32, vp, vp, i32, i32, vp, vp]
    L.orbl_fuse_candidates_device.argtypes = [i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32] + [vp] * 5
    L.orbl_fuse_candidates_workspace.argtypes = [i32, i32, C.POINTER(sz)]
    L.orbl_update_map_points_on_tables.argtypes = [i32, vp, i32, i32] + [vp] * 6 + [i32] + [vp] * 7 + [i32] + [vp] * 6
    L.orbl_update_map_points_on_tables_device.argtypes = [i32, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32] + [vp] * 9
    L.orbl_update_map_points_on_tables_workspace.argtypes = [i32, i32, C.POINTER(sz)]
    L.orbl_correct_loop.argtypes = [i32, vp, vp, i32, vp, vp, vp, vp, vp, i32] + [vp] * 8 + [i32] + [vp] * 7
    L.orbl_correct_loop_device.argtypes = [i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32] + [vp] * 5 + [i32] + [vp] * 10
    L.orbl_correct_loop_workspace.argtypes = [i32, i32, i32, C.POINTER(sz)]
    L.orbl_propagate_global_ba.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, i32] + [vp] * 9
    L.orbl_propagate_global_ba_device.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, i32] + [vp] * 12
    L.orbl_propagate_global_ba_workspace.argtypes = [i32, i32, C.POINTER(sz)]
    L.orbl_local_ba_assemble.argtypes = [i32, i32, vp, i32] + [vp] * 7 + [i32] + [vp] * 8 + [i32] * 4 + [vp] * 15
    L.orbl_local_ba_assemble_device.argtypes = [i32, i32, vp, i32] + [vp] * 5 + [i32, vp, vp, i32, vp, vp, vp, i32] + [vp] * 5 + [i32] * 4 + [vp] * 18
    L.orbl_local_ba_assemble_workspace.argtypes = [i32, i32, C.POINTER(sz)]
    L.orbl_local_ba_apply.argtypes = [i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32] + [vp] * 10 + [i32] + [vp] * 5
    L.orbl_local_ba_apply_device.argtypes = [i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32] + [vp] * 6 + [i32] + [vp] * 8
    L.orbl_local_ba_apply_workspace.argtypes = [i32, C.POINTER(sz)]
    L.orbl_essential_graph_assemble.argtypes = [i32] + [vp] * 15 + [i32, vp, vp, vp, i32, vp, vp, vp] + [i32] * 5 + [vp] * 9
    L.orbl_essential_graph_assemble_device.argtypes = [i32] + [vp] * 5 + [i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32, vp, vp] + \
        [i32] * 5 + [vp] * 12
    L.orbl_essential_graph_assemble_workspace.argtypes = [i32, C.POINTER(sz)]
    L.orbl_essential_graph_apply.argtypes = [i32, vp, vp, vp, i32, vp, vp, i32] + [vp] * 9 + [i32] + [vp] * 5
    L.orbl_essential_graph_apply_device.argtypes = [i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32] + [vp] * 8
    L.orbl_essential_graph_apply_workspace.argtypes = [i32, i32, C.POINTER(sz)]
    L.orbl_global_ba_assemble.argtypes = [i32, vp, i32, vp, i32] + [vp] * 4 + [i32] + [vp] * 7 + [i32] * 5 + [vp] * 15
    L.orbl_global_ba_assemble_device.argtypes = [i32, vp, i32, vp, i32] + [vp] * 4 + [i32, vp, vp, i32] + [vp] * 5 + [i32] * 5 + [vp] * 18
    L.orbl_global_ba_assemble_workspace.argtypes = [i32, i32, i32, i32, C.POINTER(sz)]
    L.orbl_global_ba_apply.argtypes = [i32, vp, vp, i32, vp, vp, i32, i32] + [vp] * 3 + [i32] + [vp] * 11 + [i32] + [vp] * 4
    L.orbl_global_ba_apply_device.argtypes = [i32, vp, vp, i32, vp, vp, i32, i32] + [vp] * 3 + [i32] + [vp] * 7 + [i32] + [vp] * 4 + [i32] + [vp] * 7
    L.orbl_global_ba_apply_workspace.argtypes = [i32, i32, C.POINTER(sz)]
    L.orbt_initialize.argtypes = [vp, i32, vp, i32, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, C.POINTER(InitReport), C.POINTER(InitTrace)]
    L.orbt_initialize_batch_device.argtypes = [i32, vp, vp, i32, vp, vp, i32, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbt_initialize_workspace.argtypes = [i32, i32, i32, i32, C.POINTER(C.c_size_t)]
    L.orbt_pnp_ransac_params.argtypes = [i32, f64, i32, i32, i32, f32, C.POINTER(PnpParams)]
    L.orbt_pnp_iterate.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, C.POINTER(i32), vp, vp, C.POINTER(PnpResult), vp, C.POINTER(PnpTrace)]
    L.orbt_pnp_iterate_batch_device.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbt_pnp_iterate_workspace.argtypes = [i32, i32, i32, C.POINTER(C.c_size_t)]
    L.orbt_sim3_ransac_params.argtypes = [i32, f64, i32, i32, C.POINTER(Sim3Params)]
    L.orbt_sim3_iterate.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, i32, vp, i32, C.POINTER(i32), vp, vp, vp, C.POINTER(C.c_float),
                                    C.POINTER(Sim3Result), vp, C.POINTER(Sim3Trace)]
    L.orbt_sim3_iterate_batch_device.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbt_sim3_iterate_workspace.argtypes = [i32, i32, i32, C.POINTER(C.c_size_t)]
    L.ba_solve_batch.argtypes = [vp, i32, C.POINTER(BaOptions), vp]
    L.ba_local_bundle_adjustment_batch.argtypes = [vp, i32, vp, i32, C.POINTER(i32), vp, vp]
    i64 = C.c_int64
    L.orbv_db_create.argtypes = [i32, i32, C.POINTER(vp)]
    L.orbv_db_destroy.argtypes = [vp]
    L.orbv_db_clear.argtypes = [vp]
    L.orbv_db_add.argtypes = [vp, i32, vp, vp, i32]
    L.orbv_db_erase.argtypes = [vp, i32]
    L.orbv_db_size.argtypes = [vp]
    L.orbv_db_set_best_covisibles.argtypes = [vp, i32, vp, i32]
    L.orbv_db_get_state.argtypes = [vp, vp, i32, vp, vp]
    L.orbv_db_min_score.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(f32)]
    L.orbv_db_detect_loop_candidates.argtypes = [vp, vp, vp, i32, vp, i32, f32, i64, vp, i32, C.POINTER(i32), C.POINTER(DbTrace)]
    L.orbv_db_detect_relocalization_candidates.argtypes = [vp, vp, vp, i32, i64, vp, i32, C.POINTER(i32), C.POINTER(DbTrace)]
    L.orbv_db_detect_loop_candidates_begin.argtypes = [vp, vp, vp, i32, vp, i32, f32, i64, vp, i32, C.POINTER(i32)]
    L.orbv_db_detect_relocalization_candidates_begin.argtypes = [vp, vp, vp, i32, i64, vp, i32, C.POINTER(i32)]
    L.orbv_db_detect_candidates_finish.argtypes = [vp, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(DbTrace)]
    L.orbv_db_detect_loop_candidates_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, sz, vp]
    L.orbv_db_detect_relocalization_candidates_batch_device.argtypes = [vp, i32, vp, vp, vp, i64, vp, vp, i32, vp, sz, vp]
    L.orbv_db_pending_fields.argtypes = [vp, C.POINTER(DbQueryInfo), vp, vp, i32]
    L.orbv_db_detect_workspace.argtypes = [vp, i32, C.POINTER(sz)]
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = load().orbhip_last_error().decode("utf-8", "replace")
        raise OrbHipError("%s failed (code %d): %s" % (what or "HIP call", rc, msg))


def ptr(a):
    """host numpy array or torch tensor -> void*"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)
