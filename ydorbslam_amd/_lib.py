"""Loader for libydorb.so (the C-ABI product library).  Fails loudly; never substitutes a CPU path."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class YdorbError(RuntimeError):
    pass


def library_path():
    # YDORB_LIB: an alternative build of the same library (kernel experiments); the default is the in-tree product build
    return os.environ.get("YDORB_LIB") or os.path.join(_HERE, "libydorb.so")


def build_library(jobs=4):
    """Compile every HIP source for gfx950 into ydorbslam_amd/libydorb.so (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", os.path.join(_HERE, "csrc")])
    return library_path()


class YdKeyPoint(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("class_id", C.c_int32)]


class YdExtractorConfig(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_fast_thr", C.c_int32), ("min_fast_thr", C.c_int32), ("device", C.c_int32),
                ("max_batch", C.c_int32), ("flags", C.c_int32)]


# every symbol include/ydorb/c_api.h declares: (restype, argtypes)
_VP, _I, _Z = C.c_void_p, C.c_int32, C.c_size_t
SYMBOLS = {
    "ydorb_last_error": (C.c_char_p, []),
    "ydorb_device_count": (C.c_int, []),
    "ydorb_version": (C.c_char_p, []),
    "ydorb_extractor_create": (C.c_int, [C.POINTER(YdExtractorConfig), C.POINTER(_VP)]),
    "ydorb_extractor_destroy": (None, [_VP]),
    "ydorb_extractor_tables": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_extractor_max_keypoints": (C.c_int, [_VP]),
    "ydorb_extract": (C.c_int, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, C.POINTER(_I)]),
    "ydorb_extract_batch": (C.c_int, [_VP, _VP, _I, _I, _I, _Z, _I, _VP, _VP, _I, _VP]),
    "ydorb_extract_batch_device": (C.c_int, [_VP, _VP, _I, _I, _I, _Z, _I, _VP, _VP, _I, _VP, _VP]),
    "ydorb_extractor_synchronize": (C.c_int, [_VP]),
    "ydorb_extractor_pyramid": (C.c_int, [_VP, _I, _I, C.POINTER(_VP), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "ydorb_extractor_read_level": (C.c_int, [_VP, _I, _I, _VP, _Z]),
    "ydorb_extractor_read_pyramid": (C.c_int, [_VP, _I, _VP, _VP, _I]),
    "ydorb_extractor_debug_read": (C.c_int, [_VP, _I, _I, _I, _VP, _Z, C.POINTER(_Z)]),
    "ydorb_extractor_set_profiling": (C.c_int, [_VP, _I]),
    "ydorb_extractor_stage_times": (C.c_int, [_VP, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(_I)]),
    "ydorb_matcher_create": (C.c_int, [_I, C.POINTER(_VP)]),
    "ydorb_matcher_destroy": (None, [_VP]),
    "ydorb_descriptor_distance": (C.c_int, [_VP, _VP]),
    "ydorb_descriptor_distance_rows": (C.c_int, [_VP, _VP, _VP, _I, _VP]),
    "ydorb_frame_keypoints_in_area": (C.c_int, [_VP, _VP, C.c_float, C.c_float, C.c_float, _I, _I, _VP, _I, C.POINTER(_I)]),
    "ydorb_search_by_projection": (C.c_int, [_VP, _I, _VP, _VP, _VP, _I, C.c_float, _I, _I, _VP, _VP, C.POINTER(_I)]),
    "ydorb_search_by_bow": (C.c_int, [_VP, _I, _VP, _VP, C.c_float, _I, _VP, C.POINTER(_I)]),
    "ydorb_fuse_search": (C.c_int, [_VP, _VP, _VP, _VP, _I, _VP, _I, _VP, C.POINTER(_I)]),
    "ydorb_window_search": (C.c_int, [_VP, _VP, _VP, _VP, _I, _VP, _I, _I, _VP, C.POINTER(_I)]),
    "ydorb_search_for_triangulation": (C.c_int, [_VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _I, _I, _I, _VP, C.POINTER(_I)]),
    "ydorb_distinctive_descriptors": (C.c_int, [_VP, _VP, _VP, _I, _VP]),
    "ydorb_vocabulary_create": (C.c_int, [_VP, _I, C.POINTER(_VP)]),
    "ydorb_vocabulary_destroy": (None, [_VP]),
    "ydorb_vocabulary_transform": (C.c_int, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_stereo_matches": (C.c_int, [_VP, _VP, _VP, _I, C.c_float, C.c_float, _I, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_match_consecutive_device": (C.c_int, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "ydorb_match_pairs_device": (C.c_int, [_VP, _VP, _VP, _VP, _I, _I, _I, C.c_float, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "ydorb_hamming_topk": (C.c_int, [_VP, _VP, _I, _VP, _I, _VP, _VP, _VP]),
    "ydorb_hamming_topk_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "ydorb_matcher_synchronize": (C.c_int, [_VP]),
    "ydorb_matcher_set_profiling": (C.c_int, [_VP, _I]),
    "ydorb_matcher_stage_times": (C.c_int, [_VP, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(_I)]),
    "ydorb_ba_default_options": (None, [_VP]),
    "ydorb_ba_release": (C.c_int, [_I]),
    "ydorb_ba_solve": (C.c_int, [_VP, _VP, _VP]),
    "ydorb_ba_solve_batch": (C.c_int, [_VP, _I, _VP, _VP, _I, _VP]),
    "ydorb_ba_dense_solve": (C.c_int, [_I, _VP, _I, _VP, _VP, C.POINTER(_I)]),
    "ydorb_ba_plan": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_ba_solve_with": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "ydorb_ba_reduced_system_with": (C.c_int, [_VP, _VP, _VP, C.c_double, _VP, _VP, _VP, C.POINTER(_I)]),
    "ydorb_ba_skyline_solve": (C.c_int, [_I, _VP, _I, _VP, _I, _VP, C.POINTER(_I)]),
    "ydorb_pose_optimize": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "ydorb_sim3_ransac": (C.c_int, [_VP, _I, _I, _I]),
    "ydorb_sim3_optimize": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "ydorb_sim3_release": (C.c_int, [_I]),
    "ydorb_pnp_ransac": (C.c_int, [_VP, _I, _I, _I]),
    "ydorb_pnp_release": (C.c_int, [_I]),
    "ydorb_kfdb_create": (C.c_int, [_I, _I, _I, C.c_int64, C.POINTER(_VP)]),
    "ydorb_kfdb_destroy": (None, [_VP]),
    "ydorb_kfdb_add": (C.c_int, [_VP, _VP, _VP, _VP, _I, _VP]),
    "ydorb_kfdb_erase": (C.c_int, [_VP, _VP, _I]),
    "ydorb_kfdb_clear": (C.c_int, [_VP]),
    "ydorb_kfdb_size": (C.c_int, [_VP, C.POINTER(_I), C.POINTER(_I)]),
    "ydorb_kfdb_set_covisibility": (C.c_int, [_VP, _VP, _VP, _I]),
    "ydorb_kfdb_score": (C.c_int, [_VP, _VP, _VP, _I, _VP, _I, _VP]),
    "ydorb_kfdb_detect_reloc": (C.c_int, [_VP, _VP, _VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "ydorb_kfdb_detect_loop": (C.c_int, [_VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "ydorb_triangulate_matches": (C.c_int, [_VP, _VP, _VP, _VP]),
    "ydorb_triangulate_release": (C.c_int, [_I]),
    "ydorb_frustum_cull": (C.c_int, [_VP, _VP, _VP, _VP]),
    "ydorb_frustum_release": (C.c_int, [_I]),
    "ydorb_search_local_points": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP, _VP, C.POINTER(_I), C.POINTER(_I)]),
    "ydorb_undistort_points": (C.c_int, [_VP, _VP, _I, _VP, _I]),
    "ydorb_image_bounds": (C.c_int, [_VP, _I, _I, _VP, _I]),
    "ydorb_frame_tail": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_extract_rgbd": (C.c_int, [_VP, _VP, _I, _I, _I, _VP, _I, _I, C.c_float, _VP, C.c_float, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I,
                                     C.POINTER(_I), C.POINTER(_I)]),
    "ydorb_frame_release": (C.c_int, [_I]),
    "ydorb_essential_graph_optimize": (C.c_int, [_VP, _VP, _VP]),
    "ydorb_essential_graph_linearize": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "ydorb_essential_graph_trial_step": (C.c_int, [_VP, C.c_double, _VP, C.POINTER(_I)]),
    "ydorb_essential_graph_set_profiling": (C.c_int, [_I, _I]),
    "ydorb_essential_graph_release": (C.c_int, [_I]),
    "ydorb_essential_graph_plan": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "ydorb_essential_graph_optimize_with": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "ydorb_essential_graph_trial_step_with": (C.c_int, [_VP, _VP, C.c_double, _VP, C.POINTER(_I), _VP, _VP]),
    "ydorb_map_update_normal_depth": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP]),
    "ydorb_map_covisibility": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "ydorb_map_keyframe_redundancy": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "ydorb_map_release": (C.c_int, [_I]),
    "ydorb_mapdb_create": (C.c_int, [_I, _I, _I, C.c_int64, C.POINTER(_VP)]),
    "ydorb_mapdb_destroy": (None, [_VP]),
    "ydorb_mapdb_clear": (C.c_int, [_VP]),
    "ydorb_mapdb_set_centres": (C.c_int, [_VP, _VP, _I, _VP]),
    "ydorb_mapdb_set_points": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_set_positions": (C.c_int, [_VP, _VP, _I, _VP]),
    "ydorb_mapdb_update_normal_depth": (C.c_int, [_VP, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_covisibility": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_keyframe_redundancy": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP]),
    "ydorb_mapdb_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_export": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_correct": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_set_keyframe_rows": (C.c_int, [_VP, _VP, _I, _VP, _VP]),
    "ydorb_mapdb_set_row_entries": (C.c_int, [_VP, _VP, _VP, _VP, _I]),
    "ydorb_mapdb_export_rows": (C.c_int, [_VP, _VP, _VP]),
    "ydorb_mapdb_row_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_points_of_keyframes": (C.c_int, [_VP, _VP, _I, _VP, _I, _I, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_observer_counter": (C.c_int, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_local_ba_graph": (C.c_int, [_VP, _VP, _I, _VP, _VP]),
    "ydorb_mapdb_lba_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_lba_set_profiling": (C.c_int, [_VP, _I]),
    "ydorb_mapdb_reserve_descriptors": (C.c_int, [_VP, C.c_int64, C.c_int64]),
    "ydorb_mapdb_set_keyframe_descriptors": (C.c_int, [_VP, _VP, _I, _VP, _VP]),
    "ydorb_mapdb_set_point_views": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP]),
    "ydorb_mapdb_distinctive_descriptors": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_export_views": (C.c_int, [_VP, _VP, _VP, _VP]),
    "ydorb_mapdb_export_descriptors": (C.c_int, [_VP, _VP, _VP]),
    "ydorb_mapdb_desc_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_enable_attributes": (C.c_int, [_VP]),
    "ydorb_mapdb_set_point_attributes": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_export_attributes": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_attr_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_frustum_cull": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_search_local_points": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I, _VP, C.c_float, C.c_float, _VP, _VP, _VP, _VP, C.POINTER(_I),
                                                  C.POINTER(_I)]),
    "ydorb_mapdb_enable_features": (C.c_int, [_VP]),
    "ydorb_mapdb_set_keyframe_features": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP]),
    "ydorb_mapdb_export_features": (C.c_int, [_VP, _VP, _VP, _VP]),
    "ydorb_mapdb_feat_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_fuse_search": (C.c_int, [_VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_enable_bow": (C.c_int, [_VP]),
    "ydorb_mapdb_set_keyframe_bow": (C.c_int, [_VP, _VP, _I, _VP, _VP, _VP]),
    "ydorb_mapdb_export_bow": (C.c_int, [_VP, _VP, _VP, _VP]),
    "ydorb_mapdb_bow_stats": (C.c_int, [_VP, _VP]),
    "ydorb_mapdb_create_new_points": (C.c_int, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ydorb_matcher_create_points_times": (C.c_int, [_VP, _VP, C.POINTER(_I)]),
    "ydorb_mapdb_search_by_bow_keyframes": (C.c_int, [_VP, _VP, _I, _VP, _I, C.c_float, _I, _I, _VP, _VP, _VP, _VP]),
    "ydorb_mapdb_search_by_bow_frame": (C.c_int, [_VP, _VP, _VP, _I, _VP, C.c_float, _I, _VP, _VP, _VP, _VP]),
    "ydorb_matcher_bow_search_stats": (C.c_int, [_VP, _VP]),
}

BA_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)


class YdBaProblem(C.Structure):
    _fields_ = [("n_poses", _I), ("n_points", _I), ("n_edges", _I), ("poses", _VP), ("pose_fixed", _VP), ("points", _VP),
                ("edge_pose", _VP), ("edge_point", _VP), ("edge_meas", _VP), ("edge_inv_sigma2", _VP),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double), ("stop", _VP)]


class YdPoseBatch(C.Structure):
    _fields_ = [("n_frames", _I), ("device", _I), ("edge_start", _VP), ("poses", _VP), ("points", _VP), ("meas", _VP),
                ("inv_sigma2", _VP), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double)]


class YdSim3Problem(C.Structure):
    _fields_ = [("n", _I), ("fix_scale", _I), ("min_inliers", _I), ("max_its", _I), ("X1", _VP), ("X2", _VP), ("P1", _VP), ("P2", _VP),
                ("max_err1", _VP), ("max_err2", _VP), ("K1", C.c_float * 4), ("K2", C.c_float * 4), ("n_hyp", _I), ("triples", _VP),
                ("next_hyp", _I), ("best_inliers", _I), ("best_T12", C.c_float * 13), ("ret_hyp", _I), ("no_more", _I), ("n_calls", _I),
                ("reserved", _I), ("inliers", _VP), ("hyp_inliers", _VP)]


class YdPnpProblem(C.Structure):
    _fields_ = [("n", _I), ("min_inliers", _I), ("max_its", _I), ("loop_or", _I), ("Xw", _VP), ("P2D", _VP), ("max_err", _VP),
                ("K", C.c_float * 4), ("n_hyp", _I), ("quads", _VP), ("next_hyp", _I), ("best_inliers", _I), ("best_mask", _VP),
                ("best_Tcw", C.c_float * 12), ("ret_hyp", _I), ("ret_how", _I), ("no_more", _I), ("n_calls", _I), ("Tcw", C.c_float * 12),
                ("n_inliers", _I), ("reserved", _I), ("inliers", _VP), ("hyp_inliers", _VP)]


class YdSim3Batch(C.Structure):
    _fields_ = [("n_problems", _I), ("device", _I), ("corr_start", _VP), ("S12", _VP), ("K1", _VP), ("K2", _VP), ("fix_scale", _VP),
                ("X1c", _VP), ("X2c", _VP), ("obs1", _VP), ("obs2", _VP), ("inv_sigma2_1", _VP), ("inv_sigma2_2", _VP), ("th2", C.c_double)]


class YdEssentialGraph(C.Structure):
    _fields_ = [("device", _I), ("n_vertices", _I), ("n_edges", _I), ("n_points", _I), ("sim3", _VP), ("fixed", _VP), ("edge_v0", _VP),
                ("edge_v1", _VP), ("edge_meas", _VP), ("points", _VP), ("point_ref", _VP), ("fix_scale", _I), ("iterations", _I),
                ("max_trials", _I), ("lambda_init", C.c_double)]


ESS_SOLVER_AUTO, ESS_SOLVER_DENSE, ESS_SOLVER_SKYLINE = 0, 1, 2
ESS_ORDER_SMALLER, ESS_ORDER_NATURAL, ESS_ORDER_RCM = 0, 1, 2


class YdEssentialSolverOptions(C.Structure):
    _fields_ = [("solver", _I), ("ordering", _I), ("max_factor_bytes", C.c_int64)]


class YdEssentialSolverInfo(C.Structure):
    _fields_ = [("solver_used", _I), ("ordering_used", _I), ("n_free", _I), ("max_row_blocks", _I), ("envelope_blocks", C.c_int64),
                ("envelope_blocks_natural", C.c_int64), ("envelope_blocks_rcm", C.c_int64), ("factor_bytes", C.c_int64)]


class YdTriView(C.Structure):
    _fields_ = [("kps", _VP), ("right_x", _VP), ("depth", _VP), ("n", _I), ("Tcw", C.c_float * 12), ("Rwc", C.c_float * 9),
                ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float),
                ("invfy", C.c_float), ("b", C.c_float), ("bf", C.c_float), ("level_sigma2", _VP), ("scale_factors", _VP), ("n_levels", _I)]


class YdTriBatch(C.Structure):
    _fields_ = [("device", _I), ("n_views", _I), ("n_problems", _I), ("views", _VP), ("first_view", _VP), ("second_view", _VP),
                ("match_start", _VP), ("idx1", _VP), ("idx2", _VP), ("ratio_factor", _VP)]


class YdFrustumView(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("viewing_cos_limit", C.c_float), ("n_levels", _I), ("level_ratio", C.c_float * 7), ("scale_factors", C.c_float * 8)]


class YdMapPointTable(C.Structure):
    _fields_ = [("pos_min", _VP), ("normal_max", _VP), ("max_distance", _VP), ("desc", _VP), ("n", _I)]


class YdFrustumBatch(C.Structure):
    _fields_ = [("device", _I), ("n_views", _I), ("views", _VP), ("table", YdMapPointTable), ("list_start", _VP), ("point_idx", _VP),
                ("skip", _VP)]


class YdObservationTable(C.Structure):
    _fields_ = [("n_points", _I), ("n_keyframes", _I), ("obs_start", _VP), ("obs_kf", _VP), ("obs_level", _VP), ("bad", _VP)]


class YdMapDbStats(C.Structure):
    _fields_ = [("n_points", _I), ("n_keyframes", _I), ("n_observations", C.c_int64), ("pool_used", C.c_int64), ("pool_capacity", C.c_int64),
                ("repacks_kept", _I), ("repacks_grown", _I), ("point_table_growths", _I), ("keyframe_table_growths", _I),
                ("point_capacity", _I), ("keyframe_capacity", _I), ("last_sync_bytes", C.c_int64), ("last_sync_records", C.c_int64)]


class YdMapDbRowStats(C.Structure):
    _fields_ = [("n_entries", C.c_int64), ("pool_used", C.c_int64), ("pool_capacity", C.c_int64), ("repacks_kept", _I), ("repacks_grown", _I),
                ("header_growths", _I), ("header_capacity", _I), ("last_row_sync_bytes", C.c_int64), ("last_row_sync_records", C.c_int64)]


class YdMapDbDescStats(C.Structure):
    _fields_ = [("n_views", C.c_int64), ("n_descriptors", C.c_int64), ("view_pool_used", C.c_int64), ("view_pool_capacity", C.c_int64),
                ("desc_pool_used", C.c_int64), ("desc_pool_capacity", C.c_int64), ("view_repacks_kept", _I), ("view_repacks_grown", _I),
                ("desc_repacks_kept", _I), ("desc_repacks_grown", _I), ("last_desc_sync_bytes", C.c_int64), ("last_desc_sync_records", C.c_int64)]


class YdMapDbAttrStats(C.Structure):
    _fields_ = [("enabled", _I), ("growths", _I), ("capacity", C.c_int64), ("last_attr_sync_bytes", C.c_int64),
                ("last_attr_sync_records", C.c_int64), ("last_write_through_records", C.c_int64)]


class YdMapDbFeatStats(C.Structure):
    _fields_ = [("enabled", _I), ("repacks_kept", _I), ("repacks_grown", _I), ("n_features", C.c_int64), ("pool_used", C.c_int64),
                ("pool_capacity", C.c_int64), ("last_feat_sync_bytes", C.c_int64), ("last_feat_sync_records", C.c_int64)]


class YdMapDbBowStats(C.Structure):
    _fields_ = [("enabled", _I), ("repacks_kept", _I), ("repacks_grown", _I), ("n_entries", C.c_int64), ("pool_used", C.c_int64),
                ("pool_capacity", C.c_int64), ("last_bow_sync_bytes", C.c_int64), ("last_bow_sync_records", C.c_int64)]


class YdMapDbLbaStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_calls", "last_launches", "last_syncs", "last_upload_bytes", "last_download_bytes", "last_n_local",
                                         "last_n_fixed", "last_n_points", "last_n_edges")] + \
               [(n, C.c_double) for n in ("last_ms_points", "last_ms_walk", "last_ms_emit", "last_ms_copy")]


class YdLocalBaGraph(C.Structure):
    _fields_ = [("problem", YdBaProblem), ("n_local", _I), ("n_fixed", _I), ("pose_kf", _VP), ("point_slot", _VP), ("edge_kf", _VP),
                ("edge_idx", _VP), ("point_status", _VP)]


class YdBowSearchStats(C.Structure):
    _fields_ = [("calls", C.c_int64), ("attempts", C.c_int64), ("launches", C.c_int64), ("synchronisations", C.c_int64), ("bytes_up", C.c_int64),
                ("bytes_down", C.c_int64), ("pool_per_pair", C.c_int64), ("profiled_calls", _I), ("ms", C.c_float * 3)]


class YdCreateView(C.Structure):
    _fields_ = [("kf_slot", _I), ("n", _I), ("depth", _VP), ("Tcw", C.c_float * 12), ("Rwc", C.c_float * 9), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float),
                ("b", C.c_float), ("bf", C.c_float), ("level_sigma2", C.c_float * 8), ("scale_factors", C.c_float * 8), ("n_levels", _I)]


class YdCreateNeighbour(C.Structure):
    _fields_ = [("view", YdCreateView), ("F", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float), ("ratio_factor", C.c_float)]


class YdFuseTarget(C.Structure):
    _fields_ = [("kf_slot", _I), ("view", YdFrustumView), ("inv_sigma2", C.c_float * 8), ("th", C.c_float), ("max_dist", _I), ("flags", _I)]


class YdMapCorrection(C.Structure):
    _fields_ = [("n_kf", _I), ("arithmetic", _I), ("kf_slots", _VP), ("before", _VP), ("after", _VP), ("centre_after", _VP), ("centres", _I),
                ("n", _I), ("slots", _VP), ("corrector", _VP), ("scale_factors", _VP), ("n_levels", _I), ("reserved", _I), ("normal", _VP),
                ("min_distance", _VP), ("max_distance", _VP), ("pos_out", _VP), ("status", _VP)]


class YdCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("dist", C.c_float * 5), ("n_iter", _I)]


class YdFrameTail(C.Structure):
    _fields_ = [("kps", _VP), ("n", _VP), ("n_frames", _I), ("cap", _I), ("depth", _VP), ("depth_type", _I), ("depth_w", _I), ("depth_h", _I),
                ("depth_row_stride", C.c_int64), ("depth_frame_stride", C.c_int64), ("depth_factor", C.c_float), ("bf", C.c_float),
                ("cam", YdCamera), ("bounds", C.c_float * 4), ("flags", _I), ("device", _I)]


class YdBaOptions(C.Structure):
    _fields_ = [("iters1", _I), ("iters2", _I), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double),
                ("delta_mono", C.c_double), ("delta_stereo", C.c_double), ("max_trials", _I), ("device", _I),
                ("allreduce", BA_ALLREDUCE_FN), ("allreduce_user", _VP), ("d_comm_buf", _VP), ("comm_doubles", C.c_int64),
                ("rank", _I), ("world", _I), ("flags", _I), ("reserved", _I)]


BA_SINGLE_STAGE, BA_NO_ROBUST, BA_PHASE_TIMES = 1, 2, 4
BA_TEST_LATE_UPLOADS = 8   # test only: see c_api.h


BA_SOLVER_AUTO, BA_SOLVER_DENSE, BA_SOLVER_SKYLINE = 0, 1, 2   # orderings: ESS_ORDER_*


class YdBaSolverOptions(C.Structure):
    _fields_ = [("solver", _I), ("ordering", _I), ("max_factor_bytes", C.c_int64)]


class YdBaSolverInfo(C.Structure):
    _fields_ = [("solver_used", _I), ("ordering_used", _I), ("n_free", _I), ("max_row_blocks", _I), ("dense_max_rows", _I), ("reserved", _I),
                ("covisible_pairs", C.c_int64), ("envelope_blocks", C.c_int64), ("envelope_blocks_natural", C.c_int64),
                ("envelope_blocks_rcm", C.c_int64), ("pair_updates", C.c_int64), ("factor_bytes", C.c_int64)]


class YdBaResult(C.Structure):
    _fields_ = [("n_trials", _I), ("n_iterations", _I), ("n_log", _I), ("stopped", _I), ("log_chi2", C.c_double * 32),
                ("log_lambda", C.c_double * 32), ("log_trials", _I * 32), ("log_stage", _I * 32), ("edge_outlier", _VP),
                ("ms_total", C.c_float), ("ms_errors", C.c_float), ("ms_build", C.c_float), ("ms_schur", C.c_float),
                ("ms_solve", C.c_float), ("ms_update", C.c_float)]


class YdFrameSetDev(C.Structure):
    _fields_ = [("d_kps", _VP), ("d_desc", _VP), ("d_n", _VP), ("n_frames", _I), ("cap", _I)]


class YdFrameView(C.Structure):
    _fields_ = [("kps", _VP), ("desc", _VP), ("right_x", _VP), ("n", _I), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float)]


class YdFeatureVector(C.Structure):
    _fields_ = [("node_ids", _VP), ("node_start", _VP), ("feat", _VP), ("n_nodes", _I)]


class YdBowSide(C.Structure):
    _fields_ = [("kps", _VP), ("desc", _VP), ("valid", _VP), ("n", _I), ("fv", YdFeatureVector)]


class YdTriSide(C.Structure):
    _fields_ = [("kps", _VP), ("desc", _VP), ("right_x", _VP), ("has_map_point", _VP), ("n", _I), ("fv", YdFeatureVector)]


class YdVocabularyTree(C.Structure):
    _fields_ = [("n_nodes", _I), ("levels", _I), ("child_begin", _VP), ("child_ids", _VP), ("node_desc", _VP), ("node_weight", _VP),
                ("node_word", _VP), ("weighting", _I), ("norm", _I)]


class YdStereoSide(C.Structure):
    _fields_ = [("extractor", _VP), ("first_frame", _I), ("frame_step", _I), ("kps", _VP), ("desc", _VP), ("n", _VP), ("cap", _I),
                ("reserved", _I)]


STEREO_INDEX_BY_KEYPOINT = 1
STEREO_DEVICE_POINTERS = 2


def lib():
    """The loaded C-ABI library.  Raises YdorbError when it has not been built — there is no fallback."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise YdorbError("%s is missing: build it with ydorbslam_amd.build_library(); the hot path has no CPU fallback" % path)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; loading it
        # first lets libydorb.so bind to that same copy (same SONAME) instead of bringing /opt/rocm's beside it,
        # which leaves torch with "No HIP GPUs are available".  Plumbing only: nothing here computes with torch.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            L = C.CDLL(path)
        except OSError as e:
            raise YdorbError("cannot load %s: %s" % (path, e))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        raise YdorbError("ydorb error %d: %s" % (rc, lib().ydorb_last_error().decode()))
