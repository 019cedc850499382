"""amos-slam_amd: MI355X-native front-end hot path of Amos-SLAM (ORB extract + Hamming match +
mask gate), as a thin Python mirror of the C ABI in include/amos_frontend.h.

The compute is in csrc/libamos_frontend.so (hand-written HIP for gfx950).  There is no CPU
fallback: importing the binding without the built library raises, and every call goes to the GPU.
The directory name has a hyphen (it is the project's name); load it with `load_package()` from
__graft_entry__.py or tests/conftest.py, which registers it as module `amos_slam_amd`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMOS_FRONTEND_LIB", os.path.join(_HERE, "csrc", "libamos_frontend.so"))  # override: kernel experiments

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
BEST2_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i4"), ("second_idx", "<i4"),
                        ("second_dist", "<i4")])

TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # ORBmatcher.cc:49-51

# The C ABI, declared once: every function include/amos_frontend.h exports -> (restype, argtypes).  Handles, device pointers, host
# buffers, out-parameters and structs passed by pointer are all void pointers (an address, None, a numpy buffer through _p() or
# C.byref(x)); lib() applies the table, so a wrapper passes plain Python values.
_v, _i, _z, _f, _d, _q, _u = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_double, C.c_longlong, C.c_uint32
PROTOTYPES = {
    "amos_last_error": (C.c_char_p, ()),
    "amos_device_count": (_i, ()),
    "amos_current_device": (_i, ()),
    "amos_build_variant": (C.c_char_p, ()),
    "amos_orb_create": (_i, (_v, _i, _i, _i, _i, _v, _v)),
    "amos_orb_destroy": (None, (_v,)),
    "amos_orb_geometry_probe": (_i, (_v, _i, _i, _i, _i, _v, _v)),
    "amos_orb_tables": (_i, (_v, _v, _v, _v, _v, _v, _v)),
    "amos_orb_tables_host": (_i, (_v, _v, _v, _v, _v, _v, _v)),
    "amos_orb_level_sizes": (_i, (_v, _i, _i, _v, _v)),
    "amos_orb_detect": (_i, (_v, _v, _z, _i, _i)),
    "amos_orb_level_count": (_i, (_v, _i, _i)),
    "amos_orb_level_keypoints": (_i, (_v, _i, _i, _v, _i)),
    "amos_orb_set_level_keypoints": (_i, (_v, _i, _i, _v, _i)),
    "amos_orb_level_layout": (_i, (_v, _v, _v, _v)),
    "amos_orb_fetch_levels": (_i, (_v, _i, _v, _v, _i)),
    "amos_orb_store_levels": (_i, (_v, _i, _v, _v, _i)),
    "amos_orb_gate": (_i, (_v, _v, _z, _v, _z, _v, _i, _v, _i, _v, _i, _v)),
    "amos_orb_closed_mask": (_i, (_v, _v, _z)),
    "amos_orb_describe": (_i, (_v, _v, _v, _i, _v)),
    "amos_orb_extract": (_i, (_v, _v, _z, _i, _i, _v, _v, _i, _v)),
    "amos_orb_level_image": (_i, (_v, _i, _i, _v, _z, _i)),
    "amos_orb_pyramid_images": (_i, (_v, _i, _v, _v, _i)),
    "amos_orb_blurred_image": (_i, (_v, _i, _i, _v, _z)),
    "amos_orb_level_candidates": (_i, (_v, _i, _i, _v, _i)),
    "amos_orb_extract_batch_device": (_i, (_v, _v, _z, _z, _i, _i, _i)),
    "amos_orb_detect_batch_device": (_i, (_v, _v, _z, _z, _i, _i, _i)),
    "amos_orb_gate_batch_device": (_i, (_v, _v, _z, _z)),
    "amos_orb_gate_labels_batch_device": (_i, (_v, _v, _z, _z, _v, _z, _z, _v, _z, _i, _v, _z, _i, _v)),
    "amos_orb_gate_mode": (_i, (_i,)),
    "amos_orb_batch_removed": (_i, (_v, _i, _v, _i, _v)),
    "amos_orb_describe_batch_device": (_i, (_v,)),
    "amos_orb_extract_batch_device_color": (_i, (_v, _v, _z, _z, _i, _i, _i, _i, _i)),
    "amos_frame_rgbd_glue_batch_device": (_i, (_v, _v, _i, _f, _z, _z, _f, _f, _f, _f, _f, _v, _v, _v, _v)),
    "amos_frame_stereo_match": (_i, (_v, _v, _f, _f, _v, _v, _i)),
    "amos_frame_stereo_match_batch_device": (_i, (_v, _v, _i, _f, _f, _v, _v, _v, _v)),
    "amos_frame_stereo_match_arrays_device": (_i, (_v, _v, _i, _v, _v, _v, _i, _v, _v, _v, _i, _f, _f, _v, _v, _v, _v)),
    "amos_frame_undistort_batch_device": (_i, (_v, _f, _f, _f, _f, _v, _i, _v)),
    "amos_frame_image_bounds": (_i, (_i, _i, _f, _f, _f, _f, _v, _i, _v)),
    "amos_orb_batch_results_device": (_i, (_v, _v, _v, _v, _v)),
    "amos_orb_batch_fetch": (_i, (_v, _i, _v, _v, _i, _v)),
    "amos_orb_sync": (_i, (_v,)),
    "amos_orb_timing_enable": (_i, (_v, _i)),
    "amos_orb_timing_collect": (_i, (_v, _v, _v)),
    "amos_orb_stream": (_v, (_v,)),
    "amos_match_create": (_i, (_i, _v, _v)),
    "amos_match_destroy": (None, (_v,)),
    "amos_match_sync": (_i, (_v,)),
    "amos_match_stream": (_v, (_v,)),
    "amos_match_distances": (_i, (_v, _v, _i, _v, _i, _v)),
    "amos_match_list_distances": (_i, (_v, _v, _i, _v, _i, _v, _v, _v)),
    "amos_match_list_best2": (_i, (_v, _v, _i, _v, _i, _v, _v, _i, _v)),
    "amos_match_bruteforce_best2": (_i, (_v, _v, _i, _v, _i, _i, _v)),
    "amos_match_set_bruteforce_kernel": (_i, (_v, _i)),
    "amos_match_bruteforce_best2_batch_device": (_i, (_v, _v, _z, _v, _v, _v, _i, _i, _i, _v)),
    "amos_frame_grid_build_batch_device": (_i, (_v, _v, _v, _i, _i, _v, _v)),
    "amos_match_window_best2_batch_device": (_i, (_v, _v, _v)),
    "amos_match_local_points_batch_device": (_i, (_v, _v)),
    "amos_match_local_points": (_i, (_v, _v, _v, _v, _i, _v, _i, _v, _v, _v, _i, _f, _f, _f, _f, _v, _v, _v, _v)),
    "amos_match_motion_model_batch_device": (_i, (_v, _v)),
    "amos_match_motion_model": (_i, (_v, _v, _v, _v, _i, _v, _i, _v, _v, _i, _f, _f, _f, _f, _v, _v, _v, _v)),
    "amos_match_reloc_batch_device": (_i, (_v, _v)),
    "amos_match_reloc": (_i, (_v, _v, _v, _i, _v, _i, _v, _v, _v, _i, _f, _f, _f, _f, _v, _v, _v, _v)),
    "amos_reloc_pnp_state_bytes": (_z, (_i,)),
    "amos_match_reloc_pnp_batch_device": (_i, (_v, _v)),
    "amos_match_reloc_pnp": (_i, (_v, _v, _i, _v, _v, _i, _v, _i, _v, _v, _v, _v, _v, _v)),
    "amos_match_pose_optimization_batch_device": (_i, (_v, _v)),
    "amos_match_pose_optimization": (_i, (_v, _v, _v, _i, _v, _v, _v, _i, _v, _v, _i, _i, _v, _v)),
    "amos_bow_create": (_i, (_i, _v, _i, _i, _i, _i, _i, _v, _v, _v, _v, _v)),
    "amos_bow_destroy": (None, (_v,)),
    "amos_bow_sync": (_i, (_v,)),
    "amos_bow_stream": (_v, (_v,)),
    "amos_bow_check": (_i, (_i, _i, _i, _i, _i, _v, _v, _v)),
    "amos_bow_transform_batch_device": (_i, (_v, _v, _v, _i, _i, _i, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v)),
    "amos_bow_transform": (_i, (_v, _v, _i, _i, _v, _v, _v, _v, _v, _v, _v, _v)),
    "amos_match_bow_batch_device": (_i, (_v, _v)),
    "amos_match_bow": (_i, (_v, _v, _v, _f, _i, _v, _v)),
    "amos_match_bow_kf_batch_device": (_i, (_v, _v, _f, _i)),
    "amos_match_triangulation_batch_device": (_i, (_v, _v, _v, _v, _v, _i, _i, _i)),
    "amos_match_bow_kf": (_i, (_v, _v, _v, _f, _i, _v, _v)),
    "amos_match_triangulation": (_i, (_v, _v, _v, _i, _v, _v, _v, _i, _i, _i, _v, _v)),
    "amos_match_new_points_batch_device": (_i, (_v, _v)),
    "amos_kf_geometry_from_poses": (_i, (_v, _v, _v)),
    "amos_match_new_points": (_i, (_v, _v, _v, _i, _v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _v, _v)),
    "amos_sim3_state_bytes": (_z, (_i,)),
    "amos_match_sim3_batch_device": (_i, (_v, _v)),
    "amos_match_sim3": (_i, (_v, _v, _v, _i, _v, _v, _i, _v, _v, _v, _i, _v, _v, _v, _v, _v)),
    "amos_match_sim3_search_batch_device": (_i, (_v, _v)),
    "amos_match_sim3_search": (_i, (_v, _v, _v, _v, _v, _v, _v, _v, _i, _v, _v, _v, _v, _v)),
    "amos_match_sim3_optimize_batch_device": (_i, (_v, _v)),
    "amos_match_sim3_optimize": (_i, (_v, _v, _v, _i, _v, _v, _i, _v, _v, _v, _i, _v, _v, _v)),
    "amos_match_loop_points_batch_device": (_i, (_v, _v)),
    "amos_match_loop_points": (_i, (_v, _v, _v, _i, _v, _v, _v, _v, _i, _v, _i, _v, _v)),
    "amos_match_fuse_batch_device": (_i, (_v, _v)),
    "amos_match_fuse": (_i, (_v, _v, _i, _v, _i, _i, _v, _v, _v, _v, _v, _v, _i, _v, _v, _i, _i, _i, _v, _v, _v, _v, _v)),
    "amos_mask_pre_create": (_i, (_i, _v, _i, _i, _i, _v)),
    "amos_mask_pre_destroy": (None, (_v,)),
    "amos_mask_pre_stream": (_v, (_v,)),
    "amos_mask_preprocess_batch_device": (_i, (_v, _v, _i, _v)),
    "amos_mask_pre_mode": (_i, (_i,)),
    "amos_mask_pre_one_pass": (_i, (_v, _v)),
    "amos_orb_detect_color_with_mask_pre_batch_device": (_i, (_v, _v, _v, _z, _z, _i, _i, _i, _i, _i, _v)),
    "amos_mask_bias_act_device": (_i, (_v, _v, _v, _v, _z, _i, _i)),
    "amos_mask_bias_relu_maxpool_device": (_i, (_v, _v, _v, _v, _i, _i, _i, _i)),
    "amos_mask_stem_weight_floats": (_i, ()),
    "amos_mask_stem_weights_device": (_i, (_v, _v, _q, _q, _q, _q, _v)),
    "amos_mask_stem_device": (_i, (_v, _v, _q, _q, _q, _q, _v, _v, _v, _i, _i, _i)),
    "amos_mask_conv_supported": (_i, (_i, _i, _i, _i, _i, _i)),
    "amos_mask_conv_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_conv_workspace_bytes": (_z, (_i, _i, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_conv_ws_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z)),
    "amos_mask_conv_tile_mode": (_i, (_i,)),
    "amos_mask_conv_kernel_name": (_i, (_i, _i, _i, _i, _i, _i, _i, _i, _i, _v, _i)),
    "amos_mask_conv_chain_supported": (_i, (_i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_conv_chain_device": (_i, (_v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_conv1x1_supported": (_i, (_i, _i, _i)),
    "amos_mask_conv_upsampled_residual_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _f, _f, _i)),
    "amos_mask_fpn_fold_mode": (_i, (_i,)),
    "amos_mask_winograd_supported": (_i, (_i, _i)),
    "amos_mask_winograd_weight_floats": (_z, (_i, _i)),
    "amos_mask_winograd_weights_device": (_i, (_v, _v, _v, _i, _i)),
    "amos_mask_winograd_conv_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i)),
    "amos_mask_winograd24_weight_floats": (_z, (_i, _i)),
    "amos_mask_winograd24_weights_device": (_i, (_v, _v, _v, _i, _i)),
    "amos_mask_winograd24_conv_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i)),
    "amos_mask_winograd24_conv_layout_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_winograd24_persistent_mode": (_i, (_i,)),
    "amos_mask_winograd24_narrow_mode": (_i, (_i,)),
    "amos_mask_conv1x1_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_bilinear_nhwc_device": (_i, (_v, _v, _v, _i, _i, _i, _i, _i, _i, _f, _f)),
    "amos_mask_bilinear_nhwc_act_device": (_i, (_v, _v, _v, _i, _i, _i, _i, _i, _i, _f, _f, _i)),
    "amos_mask_bilinear_x2_mode": (_i, (_i,)),
    "amos_mask_nms_column_max_device": (_i, (_v, _v, _v, _i, _i)),
    "amos_mask_class_scores_device": (_i, (_v, _v, _v, _i, _i, _i, _f)),
    "amos_mask_person_mask_device": (_i, (_v, _v, _v, _v, _i, _i, _i, _i, _i, _i)),
    "amos_mask_person_mask_rects_device": (_i, (_v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i)),
    "amos_mask_person_window_mode": (_i, (_i,)),
    "amos_mask_head_outputs_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_head_outputs_scores_device": (_i, (_v, _v, _v, _v, _v, _v, _v, _f, _i, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_topk_rows_device": (_i, (_v, _v, _v, _v, _i, _i, _i)),
    "amos_mask_topk_rows_sparse_device": (_i, (_v, _v, _v, _v, _i, _i, _i, _f)),
    "amos_mask_post_workspace_bytes": (_z, (_i, _i, _i, _i, _i, _i)),
    "amos_mask_person_masks_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z, _v, _v)),
    "amos_mask_person_masks_scores_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z, _v, _v)),
    "amos_mask_coef_at_priors_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _v, _v, _v, _i, _i, _i, _i, _v)),
    "amos_mask_person_masks_at_priors_device": (_i, (_v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z, _v, _v)),
    "amos_mask_person_masks_scores_at_priors_device": (_i, (_v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z, _v, _v)),
    "amos_mask_candidates_bytes": (_z, (_i, _i, _i)),
    "amos_mask_candidates_reset_device": (_i, (_v, _v, _i, _i)),
    "amos_mask_head_candidates_device": (_i, (_v, _v, _v, _v, _v, _v, _f, _i, _i, _i, _i, _i, _i, _i, _i)),
    "amos_mask_head_form_mode": (_i, (_i,)),
    "amos_mask_topk_lists_device": (_i, (_v, _v, _v, _i, _v, _v, _i, _i)),
    "amos_mask_person_masks_candidates_device": (_i, (_v, _v, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z, _v, _v)),
    "amos_mask_person_masks_candidates_at_priors_device": (_i, (_v, _v, _v, _v, _v, _v, _v, _v, _i, _i, _i, _v, _v, _v, _v, _i, _i, _i, _i, _i, _i, _i, _i, _v, _z, _v, _v)),
    "amos_slic_center_count": (_i, (_i, _i, _i, _v, _v)),
    "amos_slic_create": (_i, (_i, _v, _i, _i, _i, _v)),
    "amos_slic_destroy": (None, (_v,)),
    "amos_slic_stream": (_v, (_v,)),
    "amos_slic_run": (_i, (_v, _v, _v, _i, _i, _i, _i, _i, _v, _v, _v)),
    "amos_slic_batch_device": (_i, (_v, _v, _v, _i, _i, _i, _i, _i, _i, _v, _v)),
    "amos_cluster_bgr2lab_batch_device": (_i, (_v, _v, _z, _i, _v)),
    "amos_cluster_kmeans_batch_device": (_i, (_v, _v, _i, _i, _i, _u, _i, _v)),
    "amos_cluster_kmeans": (_i, (_v, _v, _i, _i, _u, _i, _v)),
    "amos_flow_check_device": (_i, (_v, _v, _z, _v, _z, _i, _i, _v, _v, _v, _i, _v)),
    "amos_flow_epipolar_device": (_i, (_v, _v, _v, _v, _v, _i, _v)),
    "amos_flow_scene_flow_device": (_i, (_v, _v, _z, _v, _z, _v, _v, _i, _v, _v)),
    "amos_flow_fundamental_score_device": (_i, (_v, _v, _i, _v, _v, _i, _d, _v, _v, _v)),
    "amos_flow_pnp_score_device": (_i, (_v, _v, _i, _v, _v, _i, _d, _d, _d, _d, _d, _v, _v, _v)),
    "amos_lk_create": (_i, (_i, _v, _i, _i, _i, _i, _v)),
    "amos_lk_destroy": (None, (_v,)),
    "amos_lk_stream": (_v, (_v,)),
    "amos_lk_levels": (_i, (_v,)),
    "amos_lk_track_device": (_i, (_v, _v, _z, _v, _z, _v, _i, _i, _d, _f, _v, _v, _v)),
    "amos_corners_create": (_i, (_i, _v, _i, _i, _v)),
    "amos_corners_destroy": (None, (_v,)),
    "amos_corners_stream": (_v, (_v,)),
    "amos_corners_good_features_device": (_i, (_v, _v, _z, _i, _i, _i, _d, _d, _d, _v, _i, _v, _v)),
    "amos_corners_candidate_count": (_i, (_v, _v)),
    "amos_corners_subpix_device": (_i, (_v, _v, _z, _i, _i, _v, _v, _i, _i, _i, _d)),
    "amos_fmat_create": (_i, (_i, _v, _i, _i, _v)),
    "amos_fmat_destroy": (None, (_v,)),
    "amos_fmat_stream": (_v, (_v,)),
    "amos_fmat_ransac_device": (_i, (_v, _i, _v, _v, _v, _v, _v, _d, _d, _i, _v, _v, _v)),
    "amos_fmat_scene_flow_pair_device": (_i, (_v, _v, _v, _v, _v, _v, _v, _v, _v)),
    "amos_fmat_ransac": (_i, (_v, _i, _v, _v, _d, _d, _i, _v, _v, _v)),
    "amos_pnp_create": (_i, (_i, _v, _i, _i, _v)),
    "amos_pnp_destroy": (None, (_v,)),
    "amos_pnp_stream": (_v, (_v,)),
    "amos_pnp_ransac_device": (_i, (_v, _i, _v, _v, _v, _v, _v, _d, _d, _d, _d, _d, _d, _i, _v, _v, _v)),
    "amos_pnp_scene_flow_device": (_i, (_v, _v, _v, _v, _v, _v, _z, _v, _z, _i, _i, _v, _d, _d, _v, _v, _v)),
    "amos_pnp_ransac": (_i, (_v, _i, _v, _v, _d, _d, _d, _d, _d, _d, _i, _v, _v, _v)),
    "amos_dyna_create": (_i, (_i, _v, _i, _i, _v)),
    "amos_dyna_destroy": (None, (_v,)),
    "amos_dyna_stream": (_v, (_v,)),
    "amos_dyna_results_device": (_i, (_v, _v)),
    "amos_dyna_copy_to_host": (_i, (_v, _v, _v, _z)),
    "amos_dyna_tail_device": (_i, (_v, _i, _v, _v, _v, _v, _v, _v, _v, _v, _v, _z, _v, _z, _i, _i, _v, _d, _d, _v)),
    "amos_dyna_reset_frame_device": (_i, (_v, _i)),
    "amos_dyna_decide_batch_device": (_i, (_v, _i, _v, _z, _z, _i, _i, _v, _z, _i, _i, _v, _z)),
    "amos_dyna_scene_flow_obj_device": (_i, (_v, _i, _v, _v, _v, _v, _v, _z, _v, _z, _i, _i, _v, _z, _v, _z, _v, _d, _d, _v)),
}
EXPORTS = list(PROTOTYPES)


class AmosError(RuntimeError):
    pass


class OrbParams(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


_lib = None


def lib():
    """The C-ABI library.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AmosError(f"{LIB_PATH} is missing: build it with `make -C amos-slam_amd/csrc` "
                            "(or __graft_entry__.build()); there is no CPU fallback")
        try:
            # torch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1 under the same sonames as
            # /opt/rocm.  One process must hold ONE HIP runtime: when torch is used beside this library
            # (device memory, streams, torch.distributed), load torch's copy first so both share it.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)

        def declare(name):
            f = getattr(L, name)
            f.restype, f.argtypes = PROTOTYPES[name]

        declare("amos_build_variant")
        variant = L.amos_build_variant().decode()
        if variant != "default" and os.environ.get("AMOS_ALLOW_EXPERIMENT_BUILD") != "1":
            # timing-experiment builds (tools/*_variants.sh) compute WRONG results by design: never load one by accident (a stale
            # AMOS_FRONTEND_LIB export); the experiment scripts set AMOS_ALLOW_EXPERIMENT_BUILD=1 themselves
            raise AmosError(f"{LIB_PATH} is an experiment build ({variant}): its results are wrong; unset AMOS_FRONTEND_LIB "
                            "or set AMOS_ALLOW_EXPERIMENT_BUILD=1 for a timing run")
        for name in PROTOTYPES:
            declare(name)
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise AmosError(f"{what} failed (rc={rc}): {lib().amos_last_error().decode()}")
    return rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def geometry_probe(max_width, max_height, width, height, n_features=1000, scale_factor=1.2, n_levels=8, ini_th=20, min_th=7):
    """Host-only: (rc, need[6], cap[6]) of amos_orb_geometry_probe -- no device is touched."""
    params = OrbParams(n_features, scale_factor, n_levels, ini_th, min_th)
    need, cap = np.zeros(6, np.int32), np.zeros(6, np.int32)
    rc = lib().amos_orb_geometry_probe(C.byref(params), max_width, max_height, width, height, _p(need), _p(cap))
    return rc, need, cap


def device_count():
    return _check(lib().amos_device_count(), "amos_device_count")


class _Handle:
    """A stream-owning library handle amos_<kind>_*, the base of every class below that wraps one: .h the handle, .L the library,
    .stream its HIP stream (hipStream_t as an integer); close() destroys it."""
    _kind = None

    def _open(self, *args):
        """amos_<kind>_create(*args, &handle): device, stream, sizes for every kind but the extractor (params, sizes, device, stream)"""
        self.L = lib()
        h = C.c_void_p()
        _check(getattr(self.L, f"amos_{self._kind}_create")(*args, C.byref(h)), f"amos_{self._kind}_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, f"amos_{self._kind}_destroy")(self.h)
            self.h = None

    __del__ = close

    @property
    def stream(self):
        return getattr(self.L, f"amos_{self._kind}_stream")(self.h)


class OrbExtractor(_Handle):
    """Mirror of ORB_SLAM2::ORBextractor (include/ORBextractor.h:93-168) over the C ABI.

    detect()            = 3-arg operator()      (ORBextractor.cc:1672)
    gate()              = MovingKeyPoints       (ORBextractor.cc:1688)
    describe()          = ProcessDesp           (ORBextractor.cc:1747)
    extract()           = 4-arg operator()      (ORBextractor.cc:1544)
    """

    _kind = "orb"

    def __init__(self, n_features=1000, scale_factor=1.2, n_levels=8, ini_th=20, min_th=7,
                 max_width=640, max_height=480, max_batch=1, device=0, stream=None):
        self.params = OrbParams(n_features, scale_factor, n_levels, ini_th, min_th)
        self.n_levels, self.n_features = n_levels, n_features
        self.max_batch = max_batch
        self._open(C.byref(self.params), max_width, max_height, max_batch, device, stream)
        self.shape = None
        cap = C.c_int(0)
        self.L.amos_orb_batch_results_device(self.h, None, None, None, C.byref(cap))
        self.capacity = cap.value

    # -- a1
    def tables(self):
        n = self.n_levels
        sc, isc, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        fpl, umax = np.zeros(n, np.int32), np.zeros(16, np.int32)
        _check(self.L.amos_orb_tables(self.h, _p(sc), _p(isc), _p(s2), _p(is2), _p(fpl), _p(umax)), "amos_orb_tables")
        return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, features_per_level=fpl, umax=umax)

    def level_sizes(self, width, height):
        lw, lh = np.zeros(self.n_levels, np.int32), np.zeros(self.n_levels, np.int32)
        _check(self.L.amos_orb_level_sizes(self.h, width, height, _p(lw), _p(lh)), "amos_orb_level_sizes")
        return lw, lh

    # -- a7
    def detect(self, gray):
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape
        self.shape = (h, w)
        _check(self.L.amos_orb_detect(self.h, _p(gray), gray.strides[0], w, h), "amos_orb_detect")

    def level_keypoints(self, level, frame=0):
        n = _check(self.L.amos_orb_level_count(self.h, frame, level), "amos_orb_level_count")
        out = np.zeros(max(n, 1), KP_DTYPE)
        _check(self.L.amos_orb_level_keypoints(self.h, frame, level, _p(out), len(out)), "amos_orb_level_keypoints")
        return out[:n]

    def set_level_keypoints(self, level, kps, frame=0):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        _check(self.L.amos_orb_set_level_keypoints(self.h, frame, level, _p(kps), len(kps)), "amos_orb_set_level_keypoints")

    def level_candidates(self, level, frame=0, cap=1 << 20):
        out = np.zeros(cap, KP_DTYPE)
        n = _check(self.L.amos_orb_level_candidates(self.h, frame, level, _p(out), cap), "amos_orb_level_candidates")
        return out[:n].copy()

    def level_image(self, level, padded=False, frame=0):
        lw, lh = self.level_sizes(self.shape[1], self.shape[0])
        w, h = int(lw[level]), int(lh[level])
        if padded:
            w, h = w + 38, h + 38
        out = np.zeros((h, w), np.uint8)
        _check(self.L.amos_orb_level_image(self.h, frame, level, _p(out), w, int(padded)), "amos_orb_level_image")
        return out

    def blurred_image(self, level, frame=0):
        lw, lh = self.level_sizes(self.shape[1], self.shape[0])
        out = np.zeros((int(lh[level]), int(lw[level])), np.uint8)
        _check(self.L.amos_orb_blurred_image(self.h, frame, level, _p(out), out.shape[1]), "amos_orb_blurred_image")
        return out

    # -- a8
    def gate(self, mask, labels=None, center_ids=None, rm_vector=None):
        mask = np.ascontiguousarray(mask, np.uint8)
        removed = np.zeros(self.capacity + 1, KP_DTYPE)
        nrem = C.c_int(0)
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.float64)
            center_ids = np.ascontiguousarray(center_ids, np.int32)
            rm_vector = np.ascontiguousarray(rm_vector, np.int32)
            rc = self.L.amos_orb_gate(self.h, _p(mask), mask.strides[0], _p(labels), labels.shape[1], _p(center_ids), len(center_ids), _p(rm_vector), len(rm_vector),
                                      _p(removed), len(removed), C.byref(nrem))
        else:
            rc = self.L.amos_orb_gate(self.h, _p(mask), mask.strides[0], None, 0, None, 0, None, 0, _p(removed), len(removed), C.byref(nrem))
        _check(rc, "amos_orb_gate")
        return removed[:nrem.value].copy()

    def closed_mask(self):
        out = np.zeros(self.shape, np.uint8)
        _check(self.L.amos_orb_closed_mask(self.h, _p(out), out.shape[1]), "amos_orb_closed_mask")
        return out

    # -- a9 / a11
    def describe(self):
        kps = np.zeros(self.capacity + 1, KP_DTYPE)
        desc = np.zeros((self.capacity + 1, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.amos_orb_describe(self.h, _p(kps), _p(desc), len(kps), C.byref(n)), "amos_orb_describe")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract(self, gray):
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape
        self.shape = (h, w)
        kps = np.zeros(self.capacity + 1, KP_DTYPE)
        desc = np.zeros((self.capacity + 1, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.amos_orb_extract(self.h, _p(gray), gray.strides[0], w, h, _p(kps), _p(desc), len(kps), C.byref(n)), "amos_orb_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    # -- batched, device resident
    def extract_batch_device(self, d_ptr, frame_stride, row_stride, width, height, n_frames):
        """d_ptr: integer device address of n_frames gray frames.  Asynchronous on the handle's stream."""
        self.shape = (height, width)
        _check(self.L.amos_orb_extract_batch_device(self.h, d_ptr, frame_stride, row_stride, width, height, n_frames), "amos_orb_extract_batch_device")

    def detect_batch_device(self, d_ptr, frame_stride, row_stride, width, height, n_frames):
        self.shape = (height, width)
        _check(self.L.amos_orb_detect_batch_device(self.h, d_ptr, frame_stride, row_stride, width, height, n_frames), "amos_orb_detect_batch_device")

    def gate_batch_device(self, d_masks, mask_frame_stride, mask_row_stride):
        _check(self.L.amos_orb_gate_batch_device(self.h, d_masks, mask_frame_stride, mask_row_stride), "amos_orb_gate_batch_device")

    def gate_labels_batch_device(self, d_masks, mask_frame_stride, mask_row_stride, d_labels, label_frame_stride, label_row_stride, d_centers,
                                 centers_frame_stride, n_centers, d_rm, rm_frame_stride, n_rm, d_status):
        """MovingKeyPoints with CalDyna's label gate per frame (Frame.cc:633): labels float64 [frames][h][w], centres amos_slic_center
        records (.id read), rm int32 [frames][n_rm]; strides in elements (records for the centres).  d_status int32 [n_frames]."""
        _check(self.L.amos_orb_gate_labels_batch_device(self.h, d_masks, mask_frame_stride, mask_row_stride, d_labels, label_frame_stride, label_row_stride,
                                                        d_centers, centers_frame_stride, n_centers, d_rm, rm_frame_stride, n_rm, d_status),
               "amos_orb_gate_labels_batch_device")

    def batch_removed(self, frame):
        """The keypoints the last (batch) gate removed from `frame`, in the reference's order."""
        total, n = C.c_int32(0), C.c_int(0)
        _check(self.L.amos_orb_level_layout(self.h, None, None, C.byref(total)), "amos_orb_level_layout")
        removed = np.zeros(total.value + 1, KP_DTYPE)
        _check(self.L.amos_orb_batch_removed(self.h, frame, _p(removed), len(removed), C.byref(n)), "amos_orb_batch_removed")
        return removed[:n.value].copy()

    def describe_batch_device(self):
        _check(self.L.amos_orb_describe_batch_device(self.h), "amos_orb_describe_batch_device")

    def extract_batch_device_color(self, d_ptr, frame_stride, row_stride, width, height, n_frames, channels=3, rgb_order=False):
        """cvtColor(BGR/RGB[A] -> gray) fused into the level-0 import (Tracking.cc:308-321)."""
        self.shape = (height, width)
        _check(self.L.amos_orb_extract_batch_device_color(self.h, d_ptr, frame_stride, row_stride, width, height, n_frames, channels, int(rgb_order)),
               "amos_orb_extract_batch_device_color")

    def detect_color_with_mask_pre_batch_device(self, pre, d_ptr, frame_stride, row_stride, width, height, n_frames, d_net_input, channels=3,
                                                rgb_order=False):
        """8f-4: one read of the colour frames -> padded gray level 0 (+ the rest of detect) and the mask network's input tensor."""
        self.shape = (height, width)
        _check(self.L.amos_orb_detect_color_with_mask_pre_batch_device(self.h, pre.h, d_ptr, frame_stride, row_stride, width, height, n_frames, channels,
                                                                       int(rgb_order), d_net_input), "amos_orb_detect_color_with_mask_pre_batch_device")

    def rgbd_glue_batch_device(self, d_depth, depth_is_u16, depth_map_factor, depth_frame_stride, depth_row_stride, mbf, bounds,
                               d_u_right, d_depth_out, d_grid_cell, d_kps_un=None):
        """ComputeStereoFromRGBD + grid cell of every keypoint of the last batch (Frame.cc:1576-1615, 1007-1030)."""
        _check(self.L.amos_frame_rgbd_glue_batch_device(self.h, d_depth, int(depth_is_u16), depth_map_factor, depth_frame_stride, depth_row_stride, mbf, bounds[0],
                                                        bounds[1], bounds[2], bounds[3], d_kps_un, d_u_right, d_depth_out, d_grid_cell),
               "amos_frame_rgbd_glue_batch_device")

    def stereo_match_batch_device(self, right, n_pairs, mbf, min_z, d_u_right, d_depth, d_sad=None, d_status=None):
        """Frame::ComputeStereoMatches (Frame.cc:1179-1573) on the last batch results: pair p is frame p of self (left) and of `right`, or
        -- right None / self -- frames 2p and 2p + 1 of this handle's batch.  float32 d_u_right / d_depth [n_pairs][capacity], -1 = no match;
        int32 d_sad [n_pairs][capacity] and d_status [n_pairs] optional.  min_z is the reference's mb = mbf / fx.  Asynchronous on self's stream."""
        r = self if right is None else right
        _check(self.L.amos_frame_stereo_match_batch_device(self.h, r.h, n_pairs, mbf, min_z, d_u_right, d_depth, d_sad, d_status),
               "amos_frame_stereo_match_batch_device")

    def stereo_match(self, right, mbf, min_z, n):
        """The synchronous host form: (u_right, depth) of the first n left keypoints of pair 0, one device-to-host transfer."""
        r = self if right is None else right
        ur, dep = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        _check(self.L.amos_frame_stereo_match(self.h, r.h, mbf, min_z, _p(ur), _p(dep), n), "amos_frame_stereo_match")
        return ur[:n], dep[:n]

    def stereo_match_arrays_device(self, right, n_pairs, d_kps_l, d_desc_l, d_counts_l, capacity_l, d_kps_r, d_desc_r, d_counts_r, capacity_r, mbf, min_z,
                                   d_u_right, d_depth, d_sad=None, d_status=None):
        """The same with explicit [frames][capacity] keypoint / descriptor / count arrays; the handles give the pyramid planes and tables."""
        r = self if right is None else right
        _check(self.L.amos_frame_stereo_match_arrays_device(self.h, r.h, n_pairs, d_kps_l, d_desc_l, d_counts_l, capacity_l, d_kps_r, d_desc_r, d_counts_r,
                                                            capacity_r, mbf, min_z, d_u_right, d_depth, d_sad, d_status),
               "amos_frame_stereo_match_arrays_device")

    def undistort_batch_device(self, fx, fy, cx, cy, dist_coef, d_kps_un):
        """Frame::UndistortKeyPoints for every keypoint of the last batch (Frame.cc:1052-1118)."""
        dc = np.ascontiguousarray(dist_coef, np.float32)
        _check(self.L.amos_frame_undistort_batch_device(self.h, fx, fy, cx, cy, _p(dc), len(dc), d_kps_un), "amos_frame_undistort_batch_device")

    def batch_results_device(self):
        kps, desc, cnt, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        _check(self.L.amos_orb_batch_results_device(self.h, C.byref(kps), C.byref(desc), C.byref(cnt), C.byref(cap)), "amos_orb_batch_results_device")
        return kps.value, desc.value, cnt.value, cap.value

    def batch_fetch(self, frame):
        kps = np.zeros(self.capacity + 1, KP_DTYPE)
        desc = np.zeros((self.capacity + 1, 32), np.uint8)
        n = C.c_int(0)
        _check(self.L.amos_orb_batch_fetch(self.h, frame, _p(kps), _p(desc), len(kps), C.byref(n)), "amos_orb_batch_fetch")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def sync(self):
        _check(self.L.amos_orb_sync(self.h), "amos_orb_sync")

    def pyramid_launches(self):
        """launches of the resize kernel(s) per pass (the "pyramid" stage of timing_collect)"""
        return self.n_levels - 1

    STAGES = ("import", "pyramid", "fast", "octree", "orient", "blur", "describe")

    def timing_enable(self, max_records):
        _check(self.L.amos_orb_timing_enable(self.h, max_records), "amos_orb_timing_enable")

    def timing_collect(self):
        """Average milliseconds per stage over the passes recorded since the last collect."""
        ms = np.zeros(len(self.STAGES), np.float32)
        n = C.c_int(0)
        _check(self.L.amos_orb_timing_collect(self.h, _p(ms), C.byref(n)), "amos_orb_timing_collect")
        return dict(zip(self.STAGES, ms.tolist())), n.value


SLIC_CENTER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("L", "<i4"), ("A", "<i4"), ("B", "<i4"), ("D", "<i4"), ("label", "<i4"), ("id", "<i4")])


class Slic(_Handle):
    """cluster::SLIC of the reference from the Lab image on (src/cluster.cc:300-343): superpixel label map + centres."""

    _kind = "slic"

    def __init__(self, max_width=640, max_height=480, max_batch=1, device=0, stream=None):
        self._open(device, stream, max_width, max_height, max_batch)

    @staticmethod
    def center_count(width, height, length=5):
        nx, ny = C.c_int(0), C.c_int(0)
        n = lib().amos_slic_center_count(width, height, length, C.byref(nx), C.byref(ny))
        return n, nx.value, ny.value

    def run(self, lab, depth, length=5, m=10, iterations=5):
        lab = np.ascontiguousarray(lab, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        assert lab.shape == (h, w, 3)
        n = self.center_count(w, h, length)[0]
        labels = np.zeros((h, w), np.float64)
        centers = np.zeros(max(n, 1), SLIC_CENTER_DTYPE)
        nc = C.c_int(0)
        _check(self.L.amos_slic_run(self.h, _p(lab), _p(depth), w, h, length, m, iterations, _p(labels), _p(centers), C.byref(nc)), "amos_slic_run")
        return labels, centers[:nc.value]

    def run_batch_device(self, d_lab, d_depth, width, height, n_frames, d_labels, d_centers, length=5, m=10, iterations=5):
        _check(self.L.amos_slic_batch_device(self.h, d_lab, d_depth, width, height, n_frames, length, m, iterations, d_labels, d_centers), "amos_slic_batch_device")

    def bgr2lab_batch_device(self, d_bgr, n_pixels, d_lab, rgb_order=False):
        """cv::cvtColor(COLOR_BGR2Lab), 8-bit (cluster.cc:310)."""
        _check(self.L.amos_cluster_bgr2lab_batch_device(self.h, d_bgr, n_pixels, int(rgb_order), d_lab), "amos_cluster_bgr2lab_batch_device")

    def kmeans(self, centers, k=15, seed=1, max_iter=1000):
        """cluster::randCent + kmeans on the SLIC centres (cluster.cc:353-460, seeded): returns (centres with .id set, passes)."""
        c = np.ascontiguousarray(centers, SLIC_CENTER_DTYPE).copy()
        passes = C.c_int(0)
        _check(self.L.amos_cluster_kmeans(self.h, _p(c), len(c), k, seed, max_iter, C.byref(passes)), "amos_cluster_kmeans")
        return c, passes.value

    def kmeans_batch_device(self, d_centers, n_centers, n_frames, k=15, seed=1, max_iter=1000, d_passes=None):
        _check(self.L.amos_cluster_kmeans_batch_device(self.h, d_centers, n_centers, n_frames, k, seed, max_iter, d_passes), "amos_cluster_kmeans_batch_device")

    def sync(self):
        import torch  # noqa: F401  (the HIP runtime is torch's)
        torch.cuda.ExternalStream(self.stream).synchronize()


class MaskPreprocessor(_Handle):
    """amos_mask_pre_*: BGR frames -> the mask network's [n, 3, 550, 550] input tensor in one HIP kernel (mask_pre_mode 0: three)
    (yolact.cc:220, 385-451; yolact_interface.py:862-866; utils/augmentations.py:616-657)."""

    _kind = "mask_pre"

    def __init__(self, width=640, height=480, max_batch=16, device=0, stream=None):
        self._open(device, stream, width, height, max_batch)
        self.max_batch, self.shape = max_batch, (height, width)

    def run(self, d_bgr, n_frames, d_out):
        _check(self.L.amos_mask_preprocess_batch_device(self.h, d_bgr, n_frames, d_out), "amos_mask_preprocess_batch_device")

    def one_pass(self):
        """(calls on this handle take the one-pass kernel under the current amos_mask_pre_mode, bytes of its source window the frame size needs)"""
        need = C.c_int(0)
        return bool(_check(self.L.amos_mask_pre_one_pass(self.h, C.byref(need)), "amos_mask_pre_one_pass")), need.value


def mask_pre_mode(mode=-1):
    """amos_mask_pre_mode: 1 = the pre-processing chain runs as one kernel where the frame size allows it (default), 0 = three kernels; returns the
    previous mode."""
    return int(lib().amos_mask_pre_mode(mode))


def mask_bias_act(stream_ptr, y_ptr, bias_ptr, residual_ptr, n, channels, relu):
    """amos_mask_bias_act_device: y = act((y + bias[c]) + residual) in place on an NHWC float32 tensor (device pointers)."""
    _check(lib().amos_mask_bias_act_device(stream_ptr, y_ptr, bias_ptr, residual_ptr, n, channels, int(relu)), "amos_mask_bias_act_device")


class SceneFlowCamera(C.Structure):
    """amos_scene_flow_camera (include/amos_frontend.h)."""
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("Tlw", C.c_float * 12), ("Rwc", C.c_float * 9),
                ("Ow", C.c_float * 3)]


def flow_check(stream, d_last, last_stride, d_cur, cur_stride, cols, rows, d_pre, d_next, d_state_in, n, d_state_out):
    _check(lib().amos_flow_check_device(stream, d_last, last_stride, d_cur, cur_stride, cols, rows, d_pre, d_next, d_state_in, n, d_state_out),
           "amos_flow_check_device")


def flow_epipolar(stream, d_F, d_pre, d_next, d_state, n, d_dd):
    _check(lib().amos_flow_epipolar_device(stream, d_F, d_pre, d_next, d_state, n, d_dd), "amos_flow_epipolar_device")


def flow_scene_flow(stream, d_depth_last, last_stride, d_depth_cur, cur_stride, d_match_pre, d_match_cur, n, cam, d_out):
    _check(lib().amos_flow_scene_flow_device(stream, d_depth_last, last_stride, d_depth_cur, cur_stride, d_match_pre, d_match_cur, n, C.byref(cam), d_out),
           "amos_flow_scene_flow_device")


def flow_fundamental_score(stream, d_F, n_hyp, d_p1, d_p2, n, threshold, d_err, d_inliers, d_mask):
    """amos_flow_fundamental_score_device: error / inlier test / inlier count of n correspondences under n_hyp fundamental matrices (device pointers)."""
    _check(lib().amos_flow_fundamental_score_device(stream, d_F, n_hyp, d_p1, d_p2, n, threshold, d_err, d_inliers, d_mask), "amos_flow_fundamental_score_device")


def flow_pnp_score(stream, d_Rt, n_hyp, d_obj, d_img, n, fx, fy, cx, cy, reprojection_error, d_err, d_inliers, d_mask):
    """amos_flow_pnp_score_device: reprojection error / inlier test / inlier count of n 3-D -> 2-D correspondences under n_hyp poses (device pointers)."""
    _check(lib().amos_flow_pnp_score_device(stream, d_Rt, n_hyp, d_obj, d_img, n, fx, fy, cx, cy, reprojection_error, d_err, d_inliers, d_mask),
           "amos_flow_pnp_score_device")


def mask_bias_relu_maxpool(stream_ptr, x_ptr, bias_ptr, y_ptr, n, in_h, in_w, channels):
    """amos_mask_bias_relu_maxpool_device: max_pool2d(relu(x + bias), 3, 2, 1) of an NHWC float32 tensor in one pass (device pointers)."""
    _check(lib().amos_mask_bias_relu_maxpool_device(stream_ptr, x_ptr, bias_ptr, y_ptr, n, in_h, in_w, channels), "amos_mask_bias_relu_maxpool_device")


def mask_stem_weight_floats():
    return int(lib().amos_mask_stem_weight_floats())


def mask_stem_weights(stream_ptr, w_ptr, w_strides, packed_ptr):
    """amos_mask_stem_weights_device: the [64][3][7][7] stem weight (element strides: out channel, in channel, row, column) -> the kernel's layout."""
    sn, sc, sy, sx = (int(v) for v in w_strides)
    _check(lib().amos_mask_stem_weights_device(stream_ptr, w_ptr, sn, sc, sy, sx, packed_ptr), "amos_mask_stem_weights_device")


def mask_stem(stream_ptr, x_ptr, x_strides, packed_ptr, bias_ptr, y_ptr, batch, height, width):
    """amos_mask_stem_device: conv 7 x 7 / 2 (3 -> 64) + bias + ReLU + max-pool 3 x 3 / 2 in one kernel; x float32 [batch][3][height][width]
    through its element strides, y channels-last [batch][ph][pw][64] (device pointers)."""
    sb, sc, sy, sx = (int(v) for v in x_strides)
    _check(lib().amos_mask_stem_device(stream_ptr, x_ptr, sb, sc, sy, sx, packed_ptr, bias_ptr, y_ptr, batch, height, width), "amos_mask_stem_device")


def orb_gate_mode(mode=-1):
    """amos_orb_gate_mode: 1 = the batch gates close the masks on bit planes (default), 0 = on grey planes; returns the previous mode."""
    return int(lib().amos_orb_gate_mode(mode))


def mask_bilinear_x2_mode(mode=-1):
    """amos_mask_bilinear_x2_mode: 1 = exact x 2 enlargements take the 2 x 2-outputs-per-thread kernel (default), 0 = never; returns the previous mode."""
    return int(lib().amos_mask_bilinear_x2_mode(mode))


def mask_conv1x1_supported(cin, cout, stride):
    return lib().amos_mask_conv1x1_supported(cin, cout, stride) == 0


def mask_conv1x1(stream_ptr, x_ptr, w_ptr, bias_ptr, residual_ptr, y_ptr, batch, in_h, in_w, cin, cout, stride, relu):
    """amos_mask_conv1x1_device: a 1 x 1 convolution + bias (+ residual) (+ ReLU) on NHWC float32 tensors (device pointers)."""
    _check(lib().amos_mask_conv1x1_device(stream_ptr, x_ptr, w_ptr, bias_ptr, residual_ptr, y_ptr, batch, in_h, in_w, cin, cout, stride, int(relu)),
           "amos_mask_conv1x1_device")


def mask_conv_supported(cin, cout, kh, kw, stride, pad):
    return lib().amos_mask_conv_supported(cin, cout, kh, kw, stride, pad) == 0


def mask_winograd_supported(cin, cout):
    return lib().amos_mask_winograd_supported(cin, cout) == 0


def mask_winograd_weights(stream_ptr, w_ptr, u_ptr, cin, cout):
    """amos_mask_winograd_weights_device: weight [cout][3][3][cin] -> transformed weight (16 * cin * cout floats at u_ptr)."""
    _check(lib().amos_mask_winograd_weights_device(stream_ptr, w_ptr, u_ptr, cin, cout), "amos_mask_winograd_weights_device")


def mask_winograd_conv(stream_ptr, x_ptr, u_ptr, bias_ptr, residual_ptr, y_ptr, batch, h, w, cin, cout, relu):
    """amos_mask_winograd_conv_device: 3 x 3 / stride 1 / pad 1 convolution + bias (+ residual) (+ ReLU) on NHWC float32 tensors."""
    _check(lib().amos_mask_winograd_conv_device(stream_ptr, x_ptr, u_ptr, bias_ptr, residual_ptr, y_ptr, batch, h, w, cin, cout, int(relu)),
           "amos_mask_winograd_conv_device")


def mask_winograd24_weights(stream_ptr, w_ptr, u_ptr, cin, cout):
    """amos_mask_winograd24_weights_device: weight [cout][3][3][cin] -> G2 g G4^T (24 * cin * cout floats at u_ptr), F(2 x 4, 3 x 3)."""
    _check(lib().amos_mask_winograd24_weights_device(stream_ptr, w_ptr, u_ptr, cin, cout), "amos_mask_winograd24_weights_device")


def mask_winograd24_conv(stream_ptr, x_ptr, u_ptr, bias_ptr, residual_ptr, y_ptr, batch, h, w, cin, cout, relu):
    """amos_mask_winograd24_conv_device: the same convolution as mask_winograd_conv as Winograd F(2 x 4, 3 x 3) (its own weight layout)."""
    _check(lib().amos_mask_winograd24_conv_device(stream_ptr, x_ptr, u_ptr, bias_ptr, residual_ptr, y_ptr, batch, h, w, cin, cout, int(relu)),
           "amos_mask_winograd24_conv_device")


def mask_winograd24_conv_layout(stream_ptr, x_ptr, u_ptr, bias_ptr, residual_ptr, y_ptr, batch, h, w, cin, cout, relu, in_blocked, out_blocked):
    """amos_mask_winograd24_conv_layout_device: mask_winograd24_conv with the channel-blocked layout [batch][c / 8][h][w][8] on the input
    (in_blocked) and / or on the output and residual (out_blocked); False = channels-last."""
    _check(lib().amos_mask_winograd24_conv_layout_device(stream_ptr, x_ptr, u_ptr, bias_ptr, residual_ptr, y_ptr, batch, h, w, cin, cout, int(relu), int(in_blocked),
                                                         int(out_blocked)), "amos_mask_winograd24_conv_layout_device")


def mask_winograd24_persistent_mode(mode=-2):
    """amos_mask_winograd24_persistent_mode: -1 by launch size, 0 one work-group per id, 1 persistent; returns the previous mode (-2: query only)."""
    return int(lib().amos_mask_winograd24_persistent_mode(mode))


def mask_winograd24_narrow_mode(mode=-2):
    """amos_mask_winograd24_narrow_mode: -1 by launch size, 0 64 output channels per work-group, 1 32; returns the previous mode (-2: query only)."""
    return int(lib().amos_mask_winograd24_narrow_mode(mode))


def mask_conv_tile_mode(mode=-2):
    """amos_mask_conv_tile_mode: -1 automatic, 0 wide (128 x 128), 1 narrow (128 x 64); returns the previous mode (-2: query only)."""
    return int(lib().amos_mask_conv_tile_mode(mode))


def mask_conv_kernel_name(batch, in_h, in_w, cin, cout, kh, kw, stride, pad):
    buf = C.create_string_buffer(96)
    _check(lib().amos_mask_conv_kernel_name(batch, in_h, in_w, cin, cout, kh, kw, stride, pad, buf, 96), "amos_mask_conv_kernel_name")
    return buf.value.decode()


def mask_conv(stream_ptr, x_ptr, w_ptr, bias_ptr, residual_ptr, y_ptr, batch, in_h, in_w, cin, cout, kh, kw, stride, pad, relu):
    """amos_mask_conv_device: convolution + bias (+ residual) (+ ReLU) on NHWC float32 tensors, weight [cout][kh][kw][cin] (device pointers)."""
    _check(lib().amos_mask_conv_device(stream_ptr, x_ptr, w_ptr, bias_ptr, residual_ptr, y_ptr, batch, in_h, in_w, cin, cout, kh, kw, stride, pad, int(relu)),
           "amos_mask_conv_device")


def mask_conv_chain_supported(batch, in_h, in_w, cin, planes, cout, stride):
    """amos_mask_conv_chain_supported: may a stage's first block run its projection shortcut and its expanding 1 x 1 convolution as one launch?"""
    return lib().amos_mask_conv_chain_supported(batch, in_h, in_w, cin, planes, cout, stride) == 0


def mask_conv_chain(stream_ptr, x_ptr, wd_ptr, bd_ptr, yc_ptr, w3_ptr, b3_ptr, y_ptr, batch, in_h, in_w, cin, planes, cout, stride):
    """amos_mask_conv_chain_device: y = relu((conv1x1(yc, w3) + b3) + ((conv1x1(x, wd, stride) + bd) + 0)) on NHWC float32 tensors in one
    launch, bit for bit the two mask_conv calls it replaces."""
    _check(lib().amos_mask_conv_chain_device(stream_ptr, x_ptr, wd_ptr, bd_ptr, yc_ptr, w3_ptr, b3_ptr, y_ptr, batch, in_h, in_w, cin, planes, cout, stride),
           "amos_mask_conv_chain_device")


def mask_conv_upsampled_residual(stream_ptr, x_ptr, w_ptr, bias_ptr, up_ptr, y_ptr, batch, in_h, in_w, cin, cout, up_h, up_w, scale_h, scale_w, relu):
    """amos_mask_conv_upsampled_residual_device: y = act((conv1x1(x, w) + bias) + bilinear(up -> in_h x in_w)) on NHWC float32 tensors in one
    launch, bit for bit mask_bilinear_nhwc followed by mask_conv with its output as the residual."""
    _check(lib().amos_mask_conv_upsampled_residual_device(stream_ptr, x_ptr, w_ptr, bias_ptr, up_ptr, y_ptr, batch, in_h, in_w, cin, cout, up_h, up_w,
                                                          scale_h, scale_w, int(relu)), "amos_mask_conv_upsampled_residual_device")


def mask_fpn_fold_mode(mode=-1):
    """amos_mask_fpn_fold_mode: 1 = the pyramid's top-down resize runs inside the lateral GEMM's epilogue (default), 0 = as a launch of its own;
    returns the previous mode."""
    return int(lib().amos_mask_fpn_fold_mode(mode))


def mask_conv_workspace_bytes(batch, in_h, in_w, cin, cout, kh, kw, stride, pad):
    """amos_mask_conv_workspace_bytes: scratch mask_conv_ws wants for its split-K plan of this shape; 0 = the plan is an ordinary launch."""
    return int(lib().amos_mask_conv_workspace_bytes(batch, in_h, in_w, cin, cout, kh, kw, stride, pad))


def mask_conv_ws(stream_ptr, x_ptr, w_ptr, bias_ptr, residual_ptr, y_ptr, batch, in_h, in_w, cin, cout, kh, kw, stride, pad, relu, workspace_ptr, workspace_bytes):
    """amos_mask_conv_ws_device: mask_conv with split-K for small launches (workspace: mask_conv_workspace_bytes; its first 16 KB zero before the
    first use and left zero; launches sharing a workspace ordered on one stream)."""
    _check(lib().amos_mask_conv_ws_device(stream_ptr, x_ptr, w_ptr, bias_ptr, residual_ptr, y_ptr, batch, in_h, in_w, cin, cout, kh, kw, stride, pad, int(relu),
                                          workspace_ptr, workspace_bytes), "amos_mask_conv_ws_device")


def mask_bilinear_nhwc(stream_ptr, x_ptr, y_ptr, n, in_h, in_w, out_h, out_w, channels, scale_h, scale_w, relu=False):
    _check(lib().amos_mask_bilinear_nhwc_act_device(stream_ptr, x_ptr, y_ptr, n, in_h, in_w, out_h, out_w, channels, scale_h, scale_w, int(relu)),
           "amos_mask_bilinear_nhwc_act_device")


def mask_class_scores(stream_ptr, conf_ptr, scores_ptr, batch, n_priors, n_classes_with_background, threshold):
    _check(lib().amos_mask_class_scores_device(stream_ptr, conf_ptr, scores_ptr, batch, n_priors, n_classes_with_background, threshold),
           "amos_mask_class_scores_device")


def mask_person_mask(stream_ptr, masks_ptr, flags_ptr, out_ptr, batch, n_det, mask_h, mask_w, out_h, out_w):
    _check(lib().amos_mask_person_mask_device(stream_ptr, masks_ptr, flags_ptr, out_ptr, batch, n_det, mask_h, mask_w, out_h, out_w), "amos_mask_person_mask_device")


def mask_person_mask_rects(stream_ptr, masks_ptr, flags_ptr, rects_ptr, out_ptr, batch, n_det, mask_h, mask_w, out_h, out_w):
    """amos_mask_person_mask_rects_device: mask_person_mask with the masks' crop rectangles [batch][n_det][4] = (x0, x1, y0, y1); every mask
    is zero outside its rectangle."""
    _check(lib().amos_mask_person_mask_rects_device(stream_ptr, masks_ptr, flags_ptr, rects_ptr, out_ptr, batch, n_det, mask_h, mask_w, out_h, out_w),
           "amos_mask_person_mask_rects_device")


def mask_person_window_mode(mode=-1):
    """amos_mask_person_window_mode: 1 = k_person_mask derives its staging rows and uses the crop rectangles (default), 0 = the earlier form;
    returns the previous mode."""
    return int(lib().amos_mask_person_window_mode(mode))


def mask_head_outputs(stream_ptr, raw_ptr, bias_ptr, loc_ptr, conf_ptr, coef_ptr, batch, cells, channels_padded, anchors, n_classes_with_background, mask_dim,
                      n_priors_total, prior_offset):
    _check(lib().amos_mask_head_outputs_device(stream_ptr, raw_ptr, bias_ptr, loc_ptr, conf_ptr, coef_ptr, batch, cells, channels_padded, anchors,
                                               n_classes_with_background, mask_dim, n_priors_total, prior_offset), "amos_mask_head_outputs_device")


def mask_head_outputs_scores(stream_ptr, raw_ptr, bias_ptr, loc_ptr, conf_ptr, coef_ptr, scores_ptr, threshold, batch, cells, channels_padded, anchors,
                             n_classes_with_background, mask_dim, n_priors_total, prior_offset):
    """amos_mask_head_outputs_scores_device: mask_head_outputs + Detect's class scores [batch][classes][n_priors_total] from the same kernel; conf_ptr may be
    None (the softmax tensor is then not written)."""
    _check(lib().amos_mask_head_outputs_scores_device(stream_ptr, raw_ptr, bias_ptr, loc_ptr, conf_ptr, coef_ptr, scores_ptr, threshold, batch, cells,
                                                      channels_padded, anchors, n_classes_with_background, mask_dim, n_priors_total, prior_offset),
           "amos_mask_head_outputs_scores_device")


def mask_person_masks_scores(stream_ptr, loc_ptr, scores_ptr, coef_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background, mask_dim, proto_h, proto_w,
                             out_h, out_w, workspace_ptr, workspace_bytes, masks_ptr, found_ptr):
    """amos_mask_person_masks_scores_device: mask_person_masks from the class scores mask_head_outputs_scores wrote instead of the softmax tensor."""
    _check(lib().amos_mask_person_masks_scores_device(stream_ptr, loc_ptr, scores_ptr, coef_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background,
                                                      mask_dim, proto_h, proto_w, out_h, out_w, workspace_ptr, workspace_bytes, masks_ptr, found_ptr),
           "amos_mask_person_masks_scores_device")


def mask_topk_rows(stream_ptr, x_ptr, values_ptr, indices_ptr, rows, n, k):
    _check(lib().amos_mask_topk_rows_device(stream_ptr, x_ptr, values_ptr, indices_ptr, rows, n, k), "amos_mask_topk_rows_device")


def mask_topk_rows_sparse(stream_ptr, x_ptr, values_ptr, indices_ptr, rows, n, k, fill):
    """amos_mask_topk_rows_sparse_device: mask_topk_rows for rows that are mostly `fill` (one scan instead of five; the same result)."""
    _check(lib().amos_mask_topk_rows_sparse_device(stream_ptr, x_ptr, values_ptr, indices_ptr, rows, n, k, fill), "amos_mask_topk_rows_sparse_device")


def mask_post_workspace_bytes(batch, n_priors, n_classes_with_background, mask_dim, proto_h, proto_w):
    """amos_mask_post_workspace_bytes: device scratch mask_person_masks needs for these sizes."""
    return int(lib().amos_mask_post_workspace_bytes(batch, n_priors, n_classes_with_background, mask_dim, proto_h, proto_w))


def mask_person_masks(stream_ptr, loc_ptr, conf_ptr, coef_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background, mask_dim, proto_h, proto_w,
                      out_h, out_w, workspace_ptr, workspace_bytes, masks_ptr, found_ptr):
    """amos_mask_person_masks_device: Detect + postprocess + prep_display of the static-shape batch path in seven launches (device pointers)."""
    _check(lib().amos_mask_person_masks_device(stream_ptr, loc_ptr, conf_ptr, coef_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background, mask_dim,
                                               proto_h, proto_w, out_h, out_w, workspace_ptr, workspace_bytes, masks_ptr, found_ptr),
           "amos_mask_person_masks_device")


def _coef_levels(level_ptrs, level_hw, level_blocked, anchors):
    """The host arrays amos_mask_coef_at_priors_device reads: (pointers, heights, widths, blocked flags, prior offsets, count)"""
    n = len(level_ptrs)
    offs, off = [], 0
    for h, w in level_hw:
        offs.append(off)
        off += h * w * anchors
    ints = C.c_int * n
    return ((C.c_void_p * n)(*level_ptrs), ints(*[h for h, _ in level_hw]), ints(*[w for _, w in level_hw]), ints(*[int(bool(f)) for f in level_blocked]),
            ints(*offs), n)


def mask_coef_at_priors(stream_ptr, level_ptrs, level_hw, level_blocked, cin, weight_ptr, bias_ptr, prior_idx_ptr, batch, n_slots, anchors, mask_dim, out_ptr):
    """amos_mask_coef_at_priors_device: the head's mask layer (weight channels-last [anchors x mask_dim][3][3][cin]) at the int32 priors
    [batch][n_slots] of the `upfeature` levels (device pointers, (h, w) pairs, channel-blocked flags) -> out [batch][n_slots][mask_dim]."""
    _check(lib().amos_mask_coef_at_priors_device(stream_ptr, *_coef_levels(level_ptrs, level_hw, level_blocked, anchors), cin, weight_ptr, bias_ptr, prior_idx_ptr,
                                                 batch, n_slots, anchors, mask_dim, out_ptr), "amos_mask_coef_at_priors_device")


def mask_candidates_bytes(batch, n_priors, n_classes_with_background):
    """amos_mask_candidates_bytes: the size of the candidate lists' buffer (counters + batch x classes lists of n_priors entries)."""
    return int(lib().amos_mask_candidates_bytes(batch, n_priors, n_classes_with_background))


def mask_candidates_reset(stream_ptr, candidates_ptr, batch, n_classes_with_background):
    """amos_mask_candidates_reset_device: the lists' counters to zero (one memset on the stream), before the first level's mask_head_candidates."""
    _check(lib().amos_mask_candidates_reset_device(stream_ptr, candidates_ptr, batch, n_classes_with_background), "amos_mask_candidates_reset_device")


def mask_head_candidates(stream_ptr, raw_ptr, bias_ptr, loc_ptr, coef_ptr, candidates_ptr, threshold, batch, cells, channels_padded, anchors,
                         n_classes_with_background, mask_dim, n_priors_total, prior_offset):
    """amos_mask_head_candidates_device: mask_head_outputs with, instead of a softmax tensor, every class score above `threshold` appended to the
    list of its (frame, class)."""
    _check(lib().amos_mask_head_candidates_device(stream_ptr, raw_ptr, bias_ptr, loc_ptr, coef_ptr, candidates_ptr, threshold, batch, cells, channels_padded,
                                                  anchors, n_classes_with_background, mask_dim, n_priors_total, prior_offset), "amos_mask_head_candidates_device")


def mask_head_form_mode(mode=-1):
    """amos_mask_head_form_mode: 1 = mask_head_candidates' kernel gives a thread one (anchor, class) column (default), 0 = its element loops;
    returns the previous mode."""
    return int(lib().amos_mask_head_form_mode(mode))


def mask_topk_lists(stream_ptr, counts_ptr, entries_ptr, capacity, values_ptr, indices_ptr, rows, k):
    """amos_mask_topk_lists_device: top-k (score descending, lowest index first) of lists of (score key << 32 | ~index) entries."""
    _check(lib().amos_mask_topk_lists_device(stream_ptr, counts_ptr, entries_ptr, capacity, values_ptr, indices_ptr, rows, k), "amos_mask_topk_lists_device")


def mask_person_masks_candidates(stream_ptr, loc_ptr, candidates_ptr, coef_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background, mask_dim,
                                 proto_h, proto_w, out_h, out_w, workspace_ptr, workspace_bytes, masks_ptr, found_ptr):
    """amos_mask_person_masks_candidates_device: mask_person_masks from the candidate lists mask_head_candidates wrote."""
    _check(lib().amos_mask_person_masks_candidates_device(stream_ptr, loc_ptr, candidates_ptr, coef_ptr, priors_ptr, proto_ptr, batch, n_priors,
                                                          n_classes_with_background, mask_dim, proto_h, proto_w, out_h, out_w, workspace_ptr, workspace_bytes,
                                                          masks_ptr, found_ptr), "amos_mask_person_masks_candidates_device")


def mask_person_masks_at_priors(stream_ptr, loc_ptr, scores_ptr, scores_are_class_scores, level_ptrs, level_hw, level_blocked, cin, anchors, mask_weight_ptr,
                                mask_bias_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background, mask_dim, proto_h, proto_w, out_h, out_w,
                                workspace_ptr, workspace_bytes, masks_ptr, found_ptr):
    """amos_mask_person_masks_at_priors_device (scores_ptr: the softmax tensor), amos_mask_person_masks_scores_at_priors_device (True: Detect's class
    scores) or amos_mask_person_masks_candidates_at_priors_device ("candidates": the lists of mask_head_candidates): mask_person_masks with the
    displayed detections' coefficients evaluated from the `upfeature` levels instead of read from a tensor."""
    name = ("amos_mask_person_masks_candidates_at_priors_device" if scores_are_class_scores == "candidates" else
            "amos_mask_person_masks_scores_at_priors_device" if scores_are_class_scores else "amos_mask_person_masks_at_priors_device")
    _check(getattr(lib(), name)(stream_ptr, loc_ptr, scores_ptr, *_coef_levels(level_ptrs, level_hw, level_blocked, anchors), cin, anchors, mask_weight_ptr,
                                mask_bias_ptr, priors_ptr, proto_ptr, batch, n_priors, n_classes_with_background, mask_dim, proto_h, proto_w, out_h, out_w,
                                workspace_ptr, workspace_bytes, masks_ptr, found_ptr), name)


def mask_nms_column_max(stream_ptr, boxes_ptr, out_ptr, n_lists, k):
    """amos_mask_nms_column_max_device: out[list][j] = max_{i < j} IoU(box i, box j) for score-sorted box lists (device pointers)."""
    _check(lib().amos_mask_nms_column_max_device(stream_ptr, boxes_ptr, out_ptr, n_lists, k), "amos_mask_nms_column_max_device")


class LkTracker(_Handle):
    """cv::calcOpticalFlowPyrLK on given points (Tracking.cc:896: 22 x 22 window, 5 levels, 20 iterations / 0.01), device resident."""

    _kind = "lk"

    def __init__(self, width=640, height=480, win_size=22, max_level=5, device=0, stream=None):
        self._open(device, stream, width, height, win_size, max_level)
        self.levels = self.L.amos_lk_levels(self.h)

    def track_device(self, d_prev, prev_stride, d_next, next_stride, d_prev_xy, n, d_next_xy, d_status, d_err=None, max_count=20, epsilon=0.01,
                     min_eig=1e-4):
        _check(self.L.amos_lk_track_device(self.h, d_prev, prev_stride, d_next, next_stride, d_prev_xy, n, max_count, epsilon, min_eig, d_next_xy, d_status,
                                           d_err), "amos_lk_track_device")


def image_bounds(width, height, fx, fy, cx, cy, dist_coef):
    """Frame::ComputeImageBounds (Frame.cc:1121-1170): (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    dc = np.ascontiguousarray(dist_coef, np.float32)
    out = np.zeros(4, np.float32)
    _check(lib().amos_frame_image_bounds(width, height, fx, fy, cx, cy, _p(dc), len(dc), _p(out)), "amos_frame_image_bounds")
    return tuple(float(v) for v in out)


class WindowSearch(C.Structure):
    """amos_window_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p),
                ("d_items", C.c_void_p), ("d_query_uv", C.c_void_p), ("d_query_invz", C.c_void_p), ("d_u_right", C.c_void_p),
                ("d_pairs_q", C.c_void_p), ("d_pairs_t", C.c_void_p), ("scale_factors", C.c_void_p), ("n_pairs", C.c_int32),
                ("capacity", C.c_int32), ("n_levels", C.c_int32), ("mode", C.c_int32), ("init_dist", C.c_int32), ("th", C.c_float),
                ("mbf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class MapPoint(C.Structure):
    """amos_map_point (include/amos_frontend.h): 80 bytes; MAP_POINT_DTYPE is the same record for numpy."""
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3), ("min_distance", C.c_float), ("max_distance", C.c_float),
                ("flags", C.c_int32), ("desc", C.c_uint8 * 32), ("pad", C.c_uint8 * 12)]


class LocalCamera(C.Structure):
    """amos_local_camera: 92 bytes; LOCAL_CAMERA_DTYPE is the same record for numpy."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("view_cos_limit", C.c_float), ("th", C.c_float),
                ("nn_ratio", C.c_float)]


class LocalStats(C.Structure):
    """amos_local_stats; LOCAL_STATS_DTYPE is the same record for numpy."""
    _fields_ = [("n_in_view", C.c_int32), ("n_matches", C.c_int32), ("n_researched", C.c_int32), ("status", C.c_int32)]


MAP_POINT_SKIP, MAP_POINT_HAS_OBS = 1, 2
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                            ("flags", "<i4"), ("desc", "u1", (32,)), ("pad", "u1", (12,))])
LOCAL_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                               ("cy", "<f4"), ("mbf", "<f4"), ("view_cos_limit", "<f4"), ("th", "<f4"), ("nn_ratio", "<f4")])
LOCAL_STATS_DTYPE = np.dtype([("n_in_view", "<i4"), ("n_matches", "<i4"), ("n_researched", "<i4"), ("status", "<i4")])
# amos_map_query (include/amos_host_types.h)
MAP_QUERY_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                            ("has_obs", "<i4"), ("desc", "u1", (32,))])
assert (C.sizeof(MapPoint), C.sizeof(LocalCamera), C.sizeof(LocalStats)) == (MAP_POINT_DTYPE.itemsize, LOCAL_CAMERA_DTYPE.itemsize,
                                                                            LOCAL_STATS_DTYPE.itemsize) == (80, 92, 16)


class LocalSearch(C.Structure):
    """amos_local_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p), ("d_items", C.c_void_p),
                ("d_u_right", C.c_void_p), ("d_points", C.c_void_p), ("point_off", C.c_void_p), ("cameras", C.c_void_p),
                ("d_occupied", C.c_void_p), ("scale_factors", C.c_void_p), ("d_query", C.c_void_p), ("d_in_view", C.c_void_p),
                ("d_match", C.c_void_p), ("d_stats", C.c_void_p), ("n_frames", C.c_int32), ("capacity", C.c_int32), ("n_levels", C.c_int32),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class LastPoint(C.Structure):
    """amos_last_point (include/amos_frontend.h): 64 bytes; LAST_POINT_DTYPE is the same record for numpy."""
    _fields_ = [("pos", C.c_float * 3), ("angle", C.c_float), ("octave", C.c_int32), ("flags", C.c_int32), ("desc", C.c_uint8 * 32),
                ("pad", C.c_uint8 * 8)]


class MotionCamera(C.Structure):
    """amos_motion_camera: 140 bytes; MOTION_CAMERA_DTYPE is the same record for numpy."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Rlw", C.c_float * 9), ("tlw", C.c_float * 3), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("mb", C.c_float), ("th", C.c_float),
                ("th_retry", C.c_float), ("retry_below", C.c_int32), ("mono", C.c_int32), ("check_orientation", C.c_int32)]


class MotionStats(C.Structure):
    """amos_motion_stats: 32 bytes; MOTION_STATS_DTYPE is the same record for numpy."""
    _fields_ = [("n_projected", C.c_int32), ("n_matches", C.c_int32), ("n_first", C.c_int32), ("pass_", C.c_int32),
                ("n_researched", C.c_int32), ("flags", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32)]


LAST_POINT_SKIP, LAST_POINT_HAS_OBS = 1, 2
MOTION_FORWARD, MOTION_BACKWARD = 1, 2  # amos_motion_stats.flags
LAST_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("octave", "<i4"), ("flags", "<i4"), ("desc", "u1", (32,)),
                             ("pad", "u1", (8,))])
MOTION_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Rlw", "<f4", (9,)), ("tlw", "<f4", (3,)), ("fx", "<f4"),
                                ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("mb", "<f4"), ("th", "<f4"),
                                ("th_retry", "<f4"), ("retry_below", "<i4"), ("mono", "<i4"), ("check_orientation", "<i4")])
MOTION_STATS_DTYPE = np.dtype([("n_projected", "<i4"), ("n_matches", "<i4"), ("n_first", "<i4"), ("pass", "<i4"), ("n_researched", "<i4"),
                               ("flags", "<i4"), ("status", "<i4"), ("pad", "<i4")])
# amos_proj_query (include/amos_host_types.h)
PROJ_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("invz", "<f4"), ("octave", "<i4"), ("angle", "<f4"), ("has_obs", "<i4"),
                             ("desc", "u1", (32,))])
assert (C.sizeof(LastPoint), C.sizeof(MotionCamera), C.sizeof(MotionStats)) == (LAST_POINT_DTYPE.itemsize, MOTION_CAMERA_DTYPE.itemsize,
                                                                                MOTION_STATS_DTYPE.itemsize) == (64, 140, 32)


class MotionSearch(C.Structure):
    """amos_motion_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p), ("d_items", C.c_void_p),
                ("d_u_right", C.c_void_p), ("d_points", C.c_void_p), ("point_off", C.c_void_p), ("cameras", C.c_void_p),
                ("scale_factors", C.c_void_p), ("d_query", C.c_void_p), ("d_projected", C.c_void_p), ("d_match", C.c_void_p),
                ("d_stats", C.c_void_p), ("n_frames", C.c_int32), ("capacity", C.c_int32), ("n_levels", C.c_int32), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class RelocPoint(C.Structure):
    """amos_reloc_point (include/amos_frontend.h): 64 bytes; RELOC_POINT_DTYPE is the same record for numpy."""
    _fields_ = [("pos", C.c_float * 3), ("angle", C.c_float), ("min_distance", C.c_float), ("max_distance", C.c_float), ("flags", C.c_int32),
                ("desc", C.c_uint8 * 32), ("pad", C.c_uint8 * 4)]


class RelocCamera(C.Structure):
    """amos_reloc_camera: 84 bytes; RELOC_CAMERA_DTYPE is the same record for numpy."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("th", C.c_float), ("orb_dist", C.c_int32), ("check_orientation", C.c_int32), ("found_from_match", C.c_int32),
                ("enabled", C.c_int32)]


class RelocStats(C.Structure):
    """amos_reloc_stats: 32 bytes; RELOC_STATS_DTYPE is the same record for numpy."""
    _fields_ = [("n_candidates", C.c_int32), ("n_projected", C.c_int32), ("n_matches", C.c_int32), ("n_researched", C.c_int32),
                ("n_found", C.c_int32), ("n_occupied", C.c_int32), ("status", C.c_int32), ("skipped", C.c_int32)]


RELOC_POINT_SKIP, RELOC_POINT_HAS_OBS = 1, 2
RELOC_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("min_distance", "<f4"), ("max_distance", "<f4"), ("flags", "<i4"),
                              ("desc", "u1", (32,)), ("pad", "u1", (4,))])
RELOC_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                               ("th", "<f4"), ("orb_dist", "<i4"), ("check_orientation", "<i4"), ("found_from_match", "<i4"),
                               ("enabled", "<i4")])
RELOC_STATS_DTYPE = np.dtype([("n_candidates", "<i4"), ("n_projected", "<i4"), ("n_matches", "<i4"), ("n_researched", "<i4"),
                              ("n_found", "<i4"), ("n_occupied", "<i4"), ("status", "<i4"), ("skipped", "<i4")])
# amos_kf_query (include/amos_host_types.h)
KF_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("level", "<i4"), ("angle", "<f4"), ("desc", "u1", (32,))])
assert (C.sizeof(RelocPoint), C.sizeof(RelocCamera), C.sizeof(RelocStats)) == (RELOC_POINT_DTYPE.itemsize, RELOC_CAMERA_DTYPE.itemsize,
                                                                              RELOC_STATS_DTYPE.itemsize) == (64, 84, 32)


class RelocSearch(C.Structure):
    """amos_reloc_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p), ("d_items", C.c_void_p),
                ("d_points", C.c_void_p), ("frame_of_pair", C.c_void_p), ("point_off", C.c_void_p), ("cameras", C.c_void_p),
                ("d_found", C.c_void_p), ("d_pose", C.c_void_p), ("scale_factors", C.c_void_p), ("d_query", C.c_void_p),
                ("d_projected", C.c_void_p), ("d_match", C.c_void_p), ("d_stats", C.c_void_p), ("n_frames", C.c_int32), ("n_pairs", C.c_int32),
                ("capacity", C.c_int32), ("n_levels", C.c_int32), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float)]


class RelocPnpParams(C.Structure):
    """amos_reloc_pnp_params: 64 bytes; RELOC_PNP_PARAMS_DTYPE is the same record for numpy."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("probability", C.c_double),
                ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("epsilon", C.c_float), ("th2", C.c_float),
                ("n_iterations", C.c_int32), ("reset", C.c_int32), ("seed", C.c_uint64), ("enabled", C.c_int32), ("pad", C.c_int32)]


class RelocPnpResult(C.Structure):
    """amos_reloc_pnp_result: 104 bytes; RELOC_PNP_RESULT_DTYPE is the same record for numpy."""
    _fields_ = [("Tcw", C.c_float * 12), ("code", C.c_int32), ("has_pose", C.c_int32), ("no_more", C.c_int32), ("refined", C.c_int32),
                ("n_inliers", C.c_int32), ("n_correspondences", C.c_int32), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
                ("iterations", C.c_int32), ("iterations_call", C.c_int32), ("best_inliers", C.c_int32), ("status", C.c_int32),
                ("skipped", C.c_int32), ("pad", C.c_int32)]


RELOC_PNP_PARAMS_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("probability", "<f8"), ("min_inliers", "<i4"),
                                   ("max_iterations", "<i4"), ("epsilon", "<f4"), ("th2", "<f4"), ("n_iterations", "<i4"), ("reset", "<i4"),
                                   ("seed", "<u8"), ("enabled", "<i4"), ("pad", "<i4")])
RELOC_PNP_RESULT_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("code", "<i4"), ("has_pose", "<i4"), ("no_more", "<i4"), ("refined", "<i4"),
                                   ("n_inliers", "<i4"), ("n_correspondences", "<i4"), ("min_inliers", "<i4"), ("max_iterations", "<i4"),
                                   ("iterations", "<i4"), ("iterations_call", "<i4"), ("best_inliers", "<i4"), ("status", "<i4"),
                                   ("skipped", "<i4"), ("pad", "<i4")])
assert (C.sizeof(RelocPnpParams), C.sizeof(RelocPnpResult)) == (RELOC_PNP_PARAMS_DTYPE.itemsize, RELOC_PNP_RESULT_DTYPE.itemsize) == (64, 104)


def reloc_pnp_params(K, seed, reset=1, n_iterations=5, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991, enabled=1):
    """One RELOC_PNP_PARAMS_DTYPE record with the parameters of Tracking.cc:2665 (SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), iterate(5))."""
    p = np.zeros(1, RELOC_PNP_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = K
    p["probability"], p["min_inliers"], p["max_iterations"], p["epsilon"], p["th2"] = probability, min_inliers, max_iterations, epsilon, th2
    p["n_iterations"], p["reset"], p["seed"], p["enabled"] = n_iterations, reset, seed, enabled
    return p[0]


class RelocPnp(C.Structure):
    """amos_reloc_pnp (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_counts", C.c_void_p), ("frame_of_pair", C.c_void_p), ("point_off", C.c_void_p), ("d_points", C.c_void_p),
                ("d_bow_match", C.c_void_p), ("level_sigma2", C.c_void_p), ("params", C.c_void_p), ("d_state", C.c_void_p),
                ("d_result", C.c_void_p), ("d_inlier", C.c_void_p), ("d_match", C.c_void_p), ("d_found", C.c_void_p), ("n_frames", C.c_int32),
                ("n_pairs", C.c_int32), ("capacity", C.c_int32), ("n_levels", C.c_int32)]


def reloc_pnp_state_bytes(capacity):
    """Bytes of one pair's carried PnPsolver state (amos_reloc_pnp_state_bytes)."""
    return int(lib().amos_reloc_pnp_state_bytes(int(capacity)))


class PoseCamera(C.Structure):
    """amos_pose_camera: 68 bytes; POSE_CAMERA_DTYPE is the same record for numpy."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mbf", C.c_float)]


class PoseResult(C.Structure):
    """amos_pose_result: 272 bytes; POSE_RESULT_DTYPE is the same record for numpy."""
    _fields_ = [("Rt", C.c_double * 12), ("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("n_edges", C.c_int32), ("n_inliers", C.c_int32),
                ("n_inliers_with_obs", C.c_int32), ("rounds", C.c_int32), ("status", C.c_int32), ("iterations", C.c_int32 * 4),
                ("trials", C.c_int32 * 4), ("lambda_", C.c_double * 4), ("chi2", C.c_double * 4)]


POSE_STATUS_OCTAVE, POSE_STATUS_MATCH_INDEX = 1, 2  # amos_pose_result.status
POSE_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                              ("mbf", "<f4")])
POSE_RESULT_DTYPE = np.dtype([("Rt", "<f8", (12,)), ("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("n_edges", "<i4"), ("n_inliers", "<i4"),
                              ("n_inliers_with_obs", "<i4"), ("rounds", "<i4"), ("status", "<i4"), ("iterations", "<i4", (4,)),
                              ("trials", "<i4", (4,)), ("lambda", "<f8", (4,)), ("chi2", "<f8", (4,))])
assert (C.sizeof(PoseCamera), C.sizeof(PoseResult)) == (POSE_CAMERA_DTYPE.itemsize, POSE_RESULT_DTYPE.itemsize) == (68, 272)


class PoseOptimization(C.Structure):
    """amos_pose_optimization (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_u_right", C.c_void_p), ("d_counts", C.c_void_p), ("d_match", C.c_void_p), ("d_points", C.c_void_p),
                ("point_stride", C.c_int32), ("flags_offset", C.c_int32), ("has_obs_bit", C.c_int32), ("point_off", C.c_void_p),
                ("cameras", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("d_outlier", C.c_void_p), ("d_result", C.c_void_p),
                ("n_frames", C.c_int32), ("capacity", C.c_int32), ("n_levels", C.c_int32), ("clear_outliers", C.c_int32)]


BOW_L1_NORM, BOW_TF_IDF = 0, 0  # DBoW2::ScoringType, DBoW2::WeightingType: what a vocabulary handle is built for
BOW_MAX_CHILDREN, BOW_MAX_CAPACITY, BOW_NO_WORD, BOW_STATUS_EARLY_LEAF = 32, 16384, 0xFFFFFFFF, 1
BOW_STATS_DTYPE = np.dtype([("n_words", "<i4"), ("n_nodes", "<i4"), ("n_stopped", "<i4"), ("status", "<i4")])
BOW_SEARCH_STATS_DTYPE = np.dtype([("n_queries", "<i4"), ("n_matches", "<i4"), ("n_researched", "<i4"), ("status", "<i4")])
assert BOW_STATS_DTYPE.itemsize == BOW_SEARCH_STATS_DTYPE.itemsize == 16


class BowSearch(C.Structure):
    """amos_bow_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_n_nodes", C.c_void_p), ("d_node_ids", C.c_void_p),
                ("d_node_off", C.c_void_p), ("d_node_idx", C.c_void_p), ("d_has_point", C.c_void_p), ("d_pairs_kf", C.c_void_p),
                ("d_pairs_f", C.c_void_p), ("d_match", C.c_void_p), ("d_stats", C.c_void_p), ("n_pairs", C.c_int32), ("capacity", C.c_int32),
                ("nn_ratio", C.c_float), ("check_orientation", C.c_int32)]


class KfPairSearch(C.Structure):
    """amos_kf_pair_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_n_nodes", C.c_void_p), ("d_node_ids", C.c_void_p),
                ("d_node_off", C.c_void_p), ("d_node_idx", C.c_void_p), ("d_has_point", C.c_void_p), ("d_u_right", C.c_void_p),
                ("d_pairs_1", C.c_void_p), ("d_pairs_2", C.c_void_p), ("d_match12", C.c_void_p), ("d_stats", C.c_void_p), ("n_pairs", C.c_int32),
                ("capacity", C.c_int32)]


KF_GEOMETRY_DTYPE = np.dtype([("f12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4")])  # amos_kf_geometry
assert KF_GEOMETRY_DTYPE.itemsize == 44
KF_STATUS_BAD_INDEX, KF_STATUS_BAD_OCTAVE = 1, 2  # amos_bow_search_stats.status of the keyframe pair searches


class NewPoints(C.Structure):
    """amos_new_points (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_kps_raw", C.c_void_p), ("d_counts", C.c_void_p), ("d_u_right", C.c_void_p), ("d_depth", C.c_void_p),
                ("d_pairs_1", C.c_void_p), ("d_pairs_2", C.c_void_p), ("d_match12", C.c_void_p), ("d_scale_factors", C.c_void_p),
                ("d_level_sigma2", C.c_void_p), ("cameras", C.c_void_p), ("pairs_1", C.c_void_p), ("pairs_2", C.c_void_p), ("enabled", C.c_void_p),
                ("d_new", C.c_void_p), ("d_verdict", C.c_void_p), ("d_stats", C.c_void_p), ("n_frames", C.c_int32), ("n_pairs", C.c_int32),
                ("capacity", C.c_int32), ("n_levels", C.c_int32)]


# AMOS_NEW_POINT_*: the verdict of a match
(NEW_POINT_TRIANGULATED, NEW_POINT_UNPROJECTED_1, NEW_POINT_UNPROJECTED_2, NEW_POINT_LOW_PARALLAX, NEW_POINT_W_ZERO, NEW_POINT_BEHIND_1,
 NEW_POINT_BEHIND_2, NEW_POINT_REPROJECTION_1, NEW_POINT_REPROJECTION_2, NEW_POINT_DISTANCE_ZERO, NEW_POINT_SCALE, NEW_POINT_CLAIMED,
 NEW_POINT_OCTAVE) = range(13)
NEW_POINT_VERDICTS = 13
NEW_POINTS_BAD_MATCH, NEW_POINTS_BAD_OCTAVE, NEW_POINTS_BAD_SLOT = 1, 2, 4  # amos_new_points_stats.status
KF_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                            ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mb", "<f4"), ("mbf", "<f4"), ("scale_factor", "<f4")])  # amos_kf_camera
NEW_POINT_DTYPE = np.dtype([("idx1", "<i4"), ("idx2", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("verdict", "<i4")])  # amos_new_point
NEW_POINTS_STATS_DTYPE = np.dtype([("n_matches", "<i4"), ("n_new", "<i4"), ("n_verdict", "<i4", (NEW_POINT_VERDICTS,)), ("status", "<i4")])
assert (KF_CAMERA_DTYPE.itemsize, NEW_POINT_DTYPE.itemsize, NEW_POINTS_STATS_DTYPE.itemsize) == (96, 24, 64)


def kf_geometry_from_poses(cam1, cam2):
    """LocalMapping::ComputeF12, the epipole and the stereo / RGB-D baseline gate from two KF_CAMERA_DTYPE records
    (amos_kf_geometry_from_poses) -> (KF_GEOMETRY_DTYPE record, False when the neighbour is skipped).  Host only."""
    c1, c2 = np.ascontiguousarray(cam1, KF_CAMERA_DTYPE).reshape(1), np.ascontiguousarray(cam2, KF_CAMERA_DTYPE).reshape(1)
    g = np.zeros(1, KF_GEOMETRY_DTYPE)
    rc = _check(lib().amos_kf_geometry_from_poses(_p(c1), _p(c2), _p(g)), "amos_kf_geometry_from_poses")
    return g[0], rc == 1


class Sim3(C.Structure):
    """amos_sim3 (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_counts", C.c_void_p), ("d_points", C.c_void_p), ("cameras", C.c_void_p), ("d_pairs_1", C.c_void_p),
                ("d_pairs_2", C.c_void_p), ("d_match12", C.c_void_p), ("level_sigma2", C.c_void_p), ("params", C.c_void_p),
                ("d_state", C.c_void_p), ("d_result", C.c_void_p), ("d_inlier", C.c_void_p), ("d_match_out", C.c_void_p),
                ("n_frames", C.c_int32), ("n_pairs", C.c_int32), ("capacity", C.c_int32), ("n_levels", C.c_int32)]


SIM3_POINT_SKIP = 1  # amos_sim3_point.flags
SIM3_STATUS_OCTAVE, SIM3_STATUS_MATCH_INDEX, SIM3_STATUS_RESTARTED = 1, 2, 4  # amos_sim3_result.status
SIM3_MAX_CORRESPONDENCES = 2048
SIM3_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("flags", "<i4")])  # amos_sim3_point
SIM3_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
SIM3_PARAMS_DTYPE = np.dtype([("probability", "<f8"), ("min_inliers", "<i4"), ("max_iterations", "<i4"), ("n_iterations", "<i4"),
                              ("fix_scale", "<i4"), ("reset", "<i4"), ("enabled", "<i4"), ("seed", "<u8")])
SIM3_RESULT_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("T12", "<f4", (16,)), ("code", "<i4"),
                              ("has_sim3", "<i4"), ("no_more", "<i4"), ("n_inliers", "<i4"), ("n_correspondences", "<i4"),
                              ("max_iterations", "<i4"), ("iterations", "<i4"), ("iterations_call", "<i4"), ("best_inliers", "<i4"),
                              ("status", "<i4"), ("skipped", "<i4")])
assert (SIM3_POINT_DTYPE.itemsize, SIM3_CAMERA_DTYPE.itemsize, SIM3_PARAMS_DTYPE.itemsize, SIM3_RESULT_DTYPE.itemsize) == (16, 64, 40, 160)


def sim3_params(seed, reset=1, n_iterations=5, probability=0.99, min_inliers=20, max_iterations=300, fix_scale=0, enabled=1):
    """One SIM3_PARAMS_DTYPE record with the parameters of LoopClosing.cc:390, 424 (SetRansacParameters(0.99, 20, 300), iterate(5))."""
    p = np.zeros(1, SIM3_PARAMS_DTYPE)
    p["probability"], p["min_inliers"], p["max_iterations"], p["n_iterations"] = probability, min_inliers, max_iterations, n_iterations
    p["fix_scale"], p["reset"], p["enabled"], p["seed"] = fix_scale, reset, enabled, seed
    return p[0]


def sim3_state_bytes(capacity):
    """Bytes of one pair's carried Sim3Solver state (amos_sim3_state_bytes)."""
    return int(lib().amos_sim3_state_bytes(int(capacity)))


class Sim3Search(C.Structure):
    """amos_sim3_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p), ("d_items", C.c_void_p),
                ("d_points", C.c_void_p), ("cameras", C.c_void_p), ("scale_factors", C.c_void_p), ("d_pairs_1", C.c_void_p),
                ("d_pairs_2", C.c_void_p), ("pairs", C.c_void_p), ("d_sim3", C.c_void_p), ("d_match12", C.c_void_p), ("d_match_out", C.c_void_p),
                ("d_match1", C.c_void_p), ("d_match2", C.c_void_p), ("d_stats", C.c_void_p), ("n_frames", C.c_int32), ("n_pairs", C.c_int32),
                ("capacity", C.c_int32), ("n_levels", C.c_int32), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float)]


SIM3_SEARCH_MATCHED_ELSEWHERE = -2  # AMOS_SIM3_SEARCH_MATCHED_ELSEWHERE
SIM3_SEARCH_PAIR_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("th", "<f4"), ("enabled", "<i4")])  # amos_sim3_search_pair
SIM3_SEARCH_STATS_DTYPE = np.dtype([("n_found", "<i4"), ("n_in_view_12", "<i4"), ("n_in_view_21", "<i4"), ("n_single_12", "<i4"),
                                    ("n_single_21", "<i4"), ("skipped", "<i4"), ("code", "<i4"), ("pad", "<i4")])  # amos_sim3_search_stats
assert (SIM3_SEARCH_PAIR_DTYPE.itemsize, SIM3_SEARCH_STATS_DTYPE.itemsize) == (60, 32)


def sim3_search_pair(R12, t12, s12, th=7.5, enabled=1):
    """One SIM3_SEARCH_PAIR_DTYPE record (th: 7.5 in LoopClosing.cc:454)."""
    p = np.zeros(1, SIM3_SEARCH_PAIR_DTYPE)
    p["R12"], p["t12"], p["s12"], p["th"], p["enabled"] = np.asarray(R12, np.float32).reshape(9), t12, s12, th, enabled
    return p[0]


class Sim3Optimize(C.Structure):
    """amos_sim3_optimize (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_counts", C.c_void_p), ("d_points", C.c_void_p), ("cameras", C.c_void_p), ("d_pairs_1", C.c_void_p),
                ("d_pairs_2", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("pairs", C.c_void_p), ("d_sim3", C.c_void_p),
                ("d_match12", C.c_void_p), ("d_match_out", C.c_void_p), ("d_result", C.c_void_p), ("n_frames", C.c_int32), ("n_pairs", C.c_int32),
                ("capacity", C.c_int32), ("n_levels", C.c_int32)]


SIM3_OPT_STATUS_OCTAVE = 1  # amos_sim3_opt_result.status
SIM3_OPT_PAIR_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("th2", "<f4"), ("fix_scale", "<i4"),
                                ("enabled", "<i4")])  # amos_sim3_opt_pair
SIM3_OPT_RESULT_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("lambda", "<f8", (2,)), ("chi2", "<f8", (2,)),
                                  ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("Scw", "<f4", (16,)), ("n_correspondences", "<i4"),
                                  ("n_bad_first", "<i4"), ("n_inliers", "<i4"), ("rounds", "<i4"), ("iterations", "<i4", (2,)),
                                  ("trials", "<i4", (2,)), ("status", "<i4"), ("skipped", "<i4"), ("code", "<i4")])  # amos_sim3_opt_result
assert (SIM3_OPT_PAIR_DTYPE.itemsize, SIM3_OPT_RESULT_DTYPE.itemsize) == (64, 256)


def sim3_opt_pair(R12, t12, s12, th2=10.0, fix_scale=0, enabled=1):
    """One SIM3_OPT_PAIR_DTYPE record (th2: 10 in LoopClosing.cc:461)."""
    p = np.zeros(1, SIM3_OPT_PAIR_DTYPE)
    p["R12"], p["t12"], p["s12"], p["th2"] = np.asarray(R12, np.float32).reshape(9), t12, s12, th2
    p["fix_scale"], p["enabled"] = fix_scale, enabled
    return p[0]


class LoopPointsSearch(C.Structure):
    """amos_loop_points_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p), ("d_items", C.c_void_p),
                ("scale_factors", C.c_void_p), ("d_points", C.c_void_p), ("point_first", C.c_void_p), ("point_count", C.c_void_p),
                ("queries", C.c_void_p), ("d_opt", C.c_void_p), ("d_matched", C.c_void_p), ("d_found", C.c_void_p),
                ("d_point_of_feature2", C.c_void_p), ("d_loop_match", C.c_void_p), ("d_stats", C.c_void_p), ("n_frames", C.c_int32),
                ("n_queries", C.c_int32), ("n_points", C.c_int32), ("capacity", C.c_int32), ("n_levels", C.c_int32), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


LOOP_POINTS_QUERY_DTYPE = np.dtype([("Scw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("th", "<f4"), ("frame", "<i4"),
                                    ("max_dist", "<i4"), ("min_inliers", "<i4"), ("min_total", "<i4"), ("enabled", "<i4"),
                                    ("found_from_match", "<i4")])  # amos_loop_points_query
LOOP_POINTS_STATS_DTYPE = np.dtype([("n_candidates", "<i4"), ("n_in_view", "<i4"), ("n_matches", "<i4"), ("n_researched", "<i4"),
                                    ("n_total", "<i4"), ("accepted", "<i4"), ("status", "<i4"), ("skipped", "<i4")])  # amos_loop_points_stats
assert (LOOP_POINTS_QUERY_DTYPE.itemsize, LOOP_POINTS_STATS_DTYPE.itemsize) == (108, 32)


def loop_points_query(frame, Scw, fx, fy, cx, cy, th=10.0, max_dist=50, min_inliers=20, min_total=40, enabled=1, found_from_match=0):
    """One LOOP_POINTS_QUERY_DTYPE record with the parameters of LoopClosing.cc:464, :534 and :546."""
    q = np.zeros(1, LOOP_POINTS_QUERY_DTYPE)
    q["Scw"] = np.asarray(Scw, np.float32).reshape(16)
    q["fx"], q["fy"], q["cx"], q["cy"], q["th"], q["frame"] = fx, fy, cx, cy, th, frame
    q["max_dist"], q["min_inliers"], q["min_total"], q["enabled"], q["found_from_match"] = max_dist, min_inliers, min_total, enabled, found_from_match
    return q[0]


FUSE_LOCAL, FUSE_SIM3 = 0, 1
FUSE_CAMERA_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                              ("cy", "<f4"), ("mbf", "<f4"), ("th", "<f4")])  # amos_fuse_camera
FUSE_STATS_DTYPE = np.dtype([("n_in_view", "<i4"), ("n_accepted", "<i4")])  # amos_fuse_stats
# amos_window_query (include/amos_host_types.h)
WINDOW_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("level", "<i4"), ("src", "<i4"), ("desc", "u1", (32,))])


class FuseCamera(C.Structure):
    """amos_fuse_camera (include/amos_frontend.h): 84 bytes; FUSE_CAMERA_DTYPE is the same record for numpy."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("mbf", C.c_float), ("th", C.c_float)]


FUSE_CAMERA_BYTES = 84  # the header's static_assert (amos_fuse.hip)
assert (C.sizeof(FuseCamera), FUSE_CAMERA_DTYPE.itemsize, FUSE_STATS_DTYPE.itemsize, WINDOW_QUERY_DTYPE.itemsize) == (FUSE_CAMERA_BYTES, 84, 8, 52)


class FuseSearch(C.Structure):
    """amos_fuse_search (include/amos_frontend.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_cell_start", C.c_void_p), ("d_items", C.c_void_p),
                ("d_u_right", C.c_void_p), ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("d_points", C.c_void_p),
                ("pair_frame", C.c_void_p), ("point_first", C.c_void_p), ("point_count", C.c_void_p), ("out_off", C.c_void_p),
                ("cameras", C.c_void_p), ("d_skip", C.c_void_p), ("d_query", C.c_void_p), ("d_in_view", C.c_void_p), ("d_best_idx", C.c_void_p),
                ("d_best_dist", C.c_void_p), ("d_stats", C.c_void_p), ("n_frames", C.c_int32), ("n_pairs", C.c_int32), ("n_points", C.c_int32),
                ("capacity", C.c_int32), ("n_levels", C.c_int32), ("mode", C.c_int32), ("max_dist", C.c_int32), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class FrameView(C.Structure):
    """amos_frame_view (include/amos_host_types.h)."""
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("descriptors", C.c_void_p), ("u_right", C.c_void_p), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class BowView(C.Structure):
    """amos_bow_view (include/amos_host_types.h)."""
    _fields_ = [("n", C.c_int32), ("keys", C.c_void_p), ("descriptors", C.c_void_p), ("has_point", C.c_void_p), ("u_right", C.c_void_p),
                ("n_nodes", C.c_int32), ("node_ids", C.c_void_p), ("node_off", C.c_void_p), ("node_idx", C.c_void_p)]


def bow_vocabulary_arrays(parent, is_leaf, desc, weight):
    """The four node arrays of amos_bow_create / amos_bow_check as contiguous arrays of one entry per node (entry 0, the root's, is not read)."""
    parent = np.ascontiguousarray(parent, np.int32)
    is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    weight = np.ascontiguousarray(weight, np.float64)
    if not (len(parent) == len(is_leaf) == len(desc) == len(weight)):
        raise ValueError("parent, is_leaf, desc and weight hold one entry per node")
    return parent, is_leaf, desc, weight


def bow_check(k, L, scoring, weighting, parent, is_leaf):
    """amos_bow_check: (rc, n_words) of the vocabulary checks alone; no device is touched."""
    parent, is_leaf = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(is_leaf, np.uint8)
    n_words = C.c_int32(0)
    rc = lib().amos_bow_check(k, L, scoring, weighting, len(parent), _p(parent), _p(is_leaf), C.byref(n_words))
    return rc, n_words.value


class BowVocabulary(_Handle):
    """A DBoW2 vocabulary tree on the device and Frame::ComputeBoW over it: TemplatedVocabulary::transform(features, BowVector&,
    FeatureVector&, levelsup) (TemplatedVocabulary.h:1127-1259).  Built from the arrays loadFromTextFile reads (:1338-1424): for node i >= 1
    its parent, leaf flag, descriptor and weight; node 0 is the root."""

    _kind = "bow"

    def __init__(self, k, L, parent, is_leaf, desc, weight, scoring=BOW_L1_NORM, weighting=BOW_TF_IDF, device=0, stream=None):
        parent, is_leaf, desc, weight = bow_vocabulary_arrays(parent, is_leaf, desc, weight)
        self.branching, self.levels, self.n_nodes = k, L, len(parent)
        self._open(device, stream, k, L, scoring, weighting, len(parent), _p(parent), _p(is_leaf), _p(desc), _p(weight))

    def transform_batch_device(self, d_desc, d_counts, n_frames, capacity, levelsup, d_feat_word, d_feat_node, d_n_nodes, d_node_ids, d_node_off,
                               d_node_idx, d_n_words, d_words, d_word_weights, d_stats):
        """The transform of resident frames (amos_bow_transform_batch_device); asynchronous on the handle's stream."""
        _check(self.L.amos_bow_transform_batch_device(self.h, d_desc, d_counts, n_frames, capacity, levelsup, d_feat_word, d_feat_node, d_n_nodes,
                                                       d_node_ids, d_node_off, d_node_idx, d_n_words, d_words, d_word_weights, d_stats),
               "amos_bow_transform_batch_device")

    def transform(self, desc, levelsup=4):
        """ONE frame from a host array (amos_bow_transform).  Returns a dict: feat_word, feat_node [n]; node_ids [n_nodes], node_off
        [n_nodes + 1], node_idx (the FeatureVector as CSR); words, word_weights [n_words] (the BowVector); stats."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        fw, fn, ids, idx, words = (np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32),
                                   np.zeros(n, np.uint32))
        off, wts, stats = np.zeros(n + 1, np.int32), np.zeros(n, np.float64), np.zeros(1, BOW_STATS_DTYPE)
        _check(self.L.amos_bow_transform(self.h, _p(desc), n, levelsup, _p(fw), _p(fn), _p(ids), _p(off), _p(idx), _p(words), _p(wts), _p(stats)),
               "amos_bow_transform")
        s = stats[0]
        nn, nw = int(s["n_nodes"]), int(s["n_words"])
        return {"feat_word": fw, "feat_node": fn, "node_ids": ids[:nn], "node_off": off[:nn + 1], "node_idx": idx[:n - int(s["n_stopped"])],
                "words": words[:nw], "word_weights": wts[:nw], "stats": s}

    def sync(self):
        _check(self.L.amos_bow_sync(self.h), "amos_bow_sync")


class OrbMatcher(_Handle):
    """The distance / best-two primitives every ORBmatcher::Search* inner loop reduces to
    (ORBmatcher.cc:1913-1933 and the candidate loops at :127-148, :278-304, :560-580, :1644-1690)."""

    _kind = "match"

    def __init__(self, device=0, stream=None):
        self._open(device, stream)

    @staticmethod
    def _sets(q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        return q, t

    def distances(self, q, t):
        q, t = self._sets(q, t)
        out = np.zeros((len(q), len(t)), np.uint16)
        _check(self.L.amos_match_distances(self.h, _p(q), len(q), _p(t), len(t), _p(out)), "amos_match_distances")
        return out

    def list_distances(self, q, t, cand_off, cand_idx):
        q, t = self._sets(q, t)
        cand_off, cand_idx = np.ascontiguousarray(cand_off, np.int32), np.ascontiguousarray(cand_idx, np.int32)
        out = np.zeros(len(cand_idx), np.uint16)
        _check(self.L.amos_match_list_distances(self.h, _p(q), len(q), _p(t), len(t), _p(cand_off), _p(cand_idx), _p(out)), "amos_match_list_distances")
        return out

    def list_best2(self, q, t, cand_off, cand_idx, init_dist=256):
        q, t = self._sets(q, t)
        cand_off, cand_idx = np.ascontiguousarray(cand_off, np.int32), np.ascontiguousarray(cand_idx, np.int32)
        out = np.zeros(len(q), BEST2_DTYPE)
        _check(self.L.amos_match_list_best2(self.h, _p(q), len(q), _p(t), len(t), _p(cand_off), _p(cand_idx), init_dist, _p(out)), "amos_match_list_best2")
        return out

    def bruteforce_best2(self, q, t, init_dist=256):
        q, t = self._sets(q, t)
        out = np.zeros(len(q), BEST2_DTYPE)
        _check(self.L.amos_match_bruteforce_best2(self.h, _p(q), len(q), _p(t), len(t), init_dist, _p(out)), "amos_match_bruteforce_best2")
        return out

    def set_bruteforce_kernel(self, mode):
        """0 = by size, 1 = xor + popcount kernel, 2 = i8 MFMA kernel (identical results)."""
        _check(self.L.amos_match_set_bruteforce_kernel(self.h, {"auto": 0, "popcount": 1, "mfma": 2}.get(mode, mode)), "amos_match_set_bruteforce_kernel")

    def bruteforce_best2_batch_device(self, d_desc, frame_stride_bytes, d_counts, d_pairs_q, d_pairs_t, n_pairs,
                                      capacity, init_dist, d_out):
        _check(self.L.amos_match_bruteforce_best2_batch_device(self.h, d_desc, frame_stride_bytes, d_counts, d_pairs_q, d_pairs_t, n_pairs, capacity, init_dist,
                                                               d_out), "amos_match_bruteforce_best2_batch_device")

    def grid_build_batch_device(self, d_grid_cell, d_counts, n_frames, capacity, d_cell_start, d_items):
        """Frame::AssignFeaturesToGrid for a resident batch (Frame.cc:431-461)."""
        _check(self.L.amos_frame_grid_build_batch_device(self.h, d_grid_cell, d_counts, n_frames, capacity, d_cell_start, d_items),
               "amos_frame_grid_build_batch_device")

    def window_best2_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, d_pairs_q, d_pairs_t, n_pairs, capacity,
                                  scale_factors, th, d_out, mode=0, init_dist=256, bounds=(0.0, 640.0, 0.0, 480.0), d_query_uv=None,
                                  d_query_invz=None, d_u_right=None, mbf=0.0):
        """GetFeaturesInArea + best/second loop of SearchByProjection(F, LastF) (Frame.cc:894-1003, ORBmatcher.cc:1629-1690)."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        w = WindowSearch(d_kps, d_desc, d_counts, d_cell_start, d_items, d_query_uv, d_query_invz, d_u_right, d_pairs_q, d_pairs_t,
                         sf.ctypes.data, n_pairs, capacity, len(sf), mode, init_dist, th, mbf, *bounds)
        _check(self.L.amos_match_window_best2_batch_device(self.h, C.byref(w), d_out), "amos_match_window_best2_batch_device")

    def local_points_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, d_points, point_off, cameras, d_occupied, capacity,
                                  scale_factors, d_query, d_in_view, d_match, d_stats, bounds=(0.0, 640.0, 0.0, 480.0), d_u_right=None):
        """Step 2 of Tracking::SearchLocalPoints for resident frames: isInFrustum + PredictScale on every point, then
        SearchByProjection(F, vpMapPoints, th) (Frame.cc:761-891, ORBmatcher.cc:70-175).  point_off: n_frames + 1 host ints; cameras: host
        LOCAL_CAMERA_DTYPE records, one per frame.  Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        off = np.ascontiguousarray(point_off, np.int32)
        cams = np.ascontiguousarray(cameras, LOCAL_CAMERA_DTYPE).reshape(-1)
        if len(off) != len(cams) + 1:
            raise ValueError("point_off holds one entry more than cameras")
        s = LocalSearch(d_kps, d_desc, d_counts, d_cell_start, d_items, d_u_right, d_points, off.ctypes.data, cams.ctypes.data, d_occupied,
                        sf.ctypes.data, d_query, d_in_view, d_match, d_stats, len(cams), capacity, len(sf), *bounds)
        _check(self.L.amos_match_local_points_batch_device(self.h, C.byref(s)), "amos_match_local_points_batch_device")

    def local_points(self, kps_un, desc, points, camera, occupied, scale_factors, bounds=(0.0, 640.0, 0.0, 480.0), u_right=None):
        """The same for ONE frame from host arrays (amos_match_local_points): returns (query, in_view, match, stats)."""
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        points = np.ascontiguousarray(points, MAP_POINT_DTYPE)
        cam = np.ascontiguousarray(camera, LOCAL_CAMERA_DTYPE).reshape(1)
        occupied = np.ascontiguousarray(occupied, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        n, m = len(kps_un), len(points)
        if len(desc) != n or len(occupied) != n or (ur is not None and len(ur) != n):
            raise ValueError("desc, occupied and u_right hold one entry per keypoint")
        query, in_view = np.zeros(m, MAP_QUERY_DTYPE), np.zeros(m, np.uint8)
        match, stats = np.full(n, -1, np.int32), np.zeros(1, LOCAL_STATS_DTYPE)
        _check(self.L.amos_match_local_points(self.h, _p(kps_un), _p(desc), _p(ur), n, _p(points), m, _p(cam), _p(occupied), _p(sf), len(sf),
                                              *bounds, _p(query), _p(in_view), _p(match), _p(stats)), "amos_match_local_points")
        return query, in_view, match, stats[0]

    def motion_model_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, d_points, point_off, cameras, capacity, scale_factors,
                                  d_query, d_projected, d_match, d_stats, bounds=(0.0, 640.0, 0.0, 480.0), d_u_right=None):
        """Tracking::TrackWithMotionModel's search for resident frames: the projection of the last frame's points, SearchByProjection(
        CurrentFrame, LastFrame, th, bMono) with its rotation histogram, and the second search with th_retry (Tracking.cc:1925-1945,
        ORBmatcher.cc:1569-1728).  point_off: n_frames + 1 host ints; cameras: host MOTION_CAMERA_DTYPE records, one per frame.
        Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        off = np.ascontiguousarray(point_off, np.int32)
        cams = np.ascontiguousarray(cameras, MOTION_CAMERA_DTYPE).reshape(-1)
        if len(off) != len(cams) + 1:
            raise ValueError("point_off holds one entry more than cameras")
        s = MotionSearch(d_kps, d_desc, d_counts, d_cell_start, d_items, d_u_right, d_points, off.ctypes.data, cams.ctypes.data,
                         sf.ctypes.data, d_query, d_projected, d_match, d_stats, len(cams), capacity, len(sf), *bounds)
        _check(self.L.amos_match_motion_model_batch_device(self.h, C.byref(s)), "amos_match_motion_model_batch_device")

    def motion_model(self, kps_un, desc, points, camera, scale_factors, bounds=(0.0, 640.0, 0.0, 480.0), u_right=None):
        """The same for ONE frame from host arrays (amos_match_motion_model): returns (query, projected, match, stats)."""
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        points = np.ascontiguousarray(points, LAST_POINT_DTYPE)
        cam = np.ascontiguousarray(camera, MOTION_CAMERA_DTYPE).reshape(1)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        n, m = len(kps_un), len(points)
        if len(desc) != n or (ur is not None and len(ur) != n):
            raise ValueError("desc and u_right hold one entry per keypoint")
        query, projected = np.zeros(m, PROJ_QUERY_DTYPE), np.zeros(m, np.uint8)
        match, stats = np.full(n, -1, np.int32), np.zeros(1, MOTION_STATS_DTYPE)
        _check(self.L.amos_match_motion_model(self.h, _p(kps_un), _p(desc), _p(ur), n, _p(points), m, _p(cam), _p(sf), len(sf), *bounds,
                                              _p(query), _p(projected), _p(match), _p(stats)), "amos_match_motion_model")
        return query, projected, match, stats[0]

    def reloc_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, n_frames, d_points, frame_of_pair, point_off, cameras, capacity,
                           scale_factors, d_query, d_projected, d_match, d_stats, bounds=(0.0, 640.0, 0.0, 480.0), d_found=None, d_pose=None):
        """Relocalization's SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1731-1863) for pairs (frame,
        candidate keyframe) on resident frames.  frame_of_pair: n_pairs host ints; point_off: n_pairs + 1 host ints; cameras: host
        RELOC_CAMERA_DTYPE records, one per pair; d_match [pairs][capacity] is read and written; d_pose: POSE_RESULT_DTYPE records on the
        device, one per pair, or None (the cameras' poses).  Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        off = np.ascontiguousarray(point_off, np.int32)
        fop = np.ascontiguousarray(frame_of_pair, np.int32)
        cams = np.ascontiguousarray(cameras, RELOC_CAMERA_DTYPE).reshape(-1)
        if len(off) != len(cams) + 1 or len(fop) != len(cams):
            raise ValueError("point_off holds one entry more than cameras, frame_of_pair as many")
        s = RelocSearch(d_kps, d_desc, d_counts, d_cell_start, d_items, d_points, fop.ctypes.data, off.ctypes.data, cams.ctypes.data, d_found,
                        d_pose, sf.ctypes.data, d_query, d_projected, d_match, d_stats, n_frames, len(cams), capacity, len(sf), *bounds)
        _check(self.L.amos_match_reloc_batch_device(self.h, C.byref(s)), "amos_match_reloc_batch_device")

    def reloc(self, kps_un, desc, points, camera, scale_factors, match, found=None, bounds=(0.0, 640.0, 0.0, 480.0)):
        """The same for ONE pair from host arrays (amos_match_reloc): match [n] is the frame's matches on entry (not modified); returns
        (query, projected, match, stats)."""
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        points = np.ascontiguousarray(points, RELOC_POINT_DTYPE)
        cam = np.ascontiguousarray(camera, RELOC_CAMERA_DTYPE).reshape(1)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        match = np.ascontiguousarray(match, np.int32).copy()
        fd = None if found is None else np.ascontiguousarray(found, np.uint8)
        n, m = len(kps_un), len(points)
        if len(desc) != n or len(match) != n or (fd is not None and len(fd) != m):
            raise ValueError("desc and match hold one entry per keypoint, found one per point")
        query, projected = np.zeros(m, KF_QUERY_DTYPE), np.zeros(m, np.uint8)
        stats = np.zeros(1, RELOC_STATS_DTYPE)
        _check(self.L.amos_match_reloc(self.h, _p(kps_un), _p(desc), n, _p(points), m, _p(fd), _p(cam), _p(sf), len(sf), *bounds, _p(query),
                                       _p(projected), _p(match), _p(stats)), "amos_match_reloc")
        return query, projected, match, stats[0]

    def reloc_pnp_batch_device(self, d_kps, d_counts, n_frames, d_points, frame_of_pair, point_off, d_bow_match, level_sigma2, params, capacity,
                               d_state, d_result, d_inlier, d_match, d_found=None):
        """Relocalization's PnPsolver (PnPsolver.cc:120-458), one iterate() call per pair (frame, candidate keyframe) on resident frames.
        frame_of_pair: n_pairs host ints; point_off: n_pairs + 1 host ints; params: host RELOC_PNP_PARAMS_DTYPE records, one per pair;
        d_state: n_pairs blocks of reloc_pnp_state_bytes(capacity) bytes; d_result: RELOC_PNP_RESULT_DTYPE records.  Asynchronous on the
        matcher's stream."""
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        off = np.ascontiguousarray(point_off, np.int32)
        fop = np.ascontiguousarray(frame_of_pair, np.int32)
        par = np.ascontiguousarray(params, RELOC_PNP_PARAMS_DTYPE).reshape(-1)
        if len(off) != len(par) + 1 or len(fop) != len(par):
            raise ValueError("point_off holds one entry more than params, frame_of_pair as many")
        s = RelocPnp(d_kps, d_counts, fop.ctypes.data, off.ctypes.data, d_points, d_bow_match, sig.ctypes.data, par.ctypes.data, d_state, d_result,
                     d_inlier, d_match, d_found, n_frames, len(par), capacity, len(sig))
        _check(self.L.amos_match_reloc_pnp_batch_device(self.h, C.byref(s)), "amos_match_reloc_pnp_batch_device")

    def reloc_pnp(self, kps_un, bow_match, points, level_sigma2, params, state=None):
        """The same for ONE pair from host arrays (amos_match_reloc_pnp): returns (result, inlier, match, found, state).  state: the blob an
        earlier call returned (params['reset'] = 0 goes on from it), or None for a fresh one.  match and found are None without a pose."""
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        bow_match = np.ascontiguousarray(bow_match, np.int32)
        points = np.ascontiguousarray(points, RELOC_POINT_DTYPE)
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        par = np.ascontiguousarray(params, RELOC_PNP_PARAMS_DTYPE).reshape(1)
        n, m = len(kps_un), len(points)
        if len(bow_match) != n:
            raise ValueError("bow_match holds one entry per keypoint")
        nbytes = reloc_pnp_state_bytes(max(n, 1))
        state = np.zeros(nbytes, np.uint8) if state is None else np.ascontiguousarray(state, np.uint8).copy()
        if len(state) != nbytes:
            raise ValueError("state is not a blob of reloc_pnp_state_bytes(n) bytes")
        result = np.zeros(1, RELOC_PNP_RESULT_DTYPE)
        inlier, match, found = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.zeros(m, np.uint8)
        _check(self.L.amos_match_reloc_pnp(self.h, _p(kps_un), n, _p(bow_match), _p(points), m, _p(sig), len(sig), _p(par), _p(state), _p(result),
                                           _p(inlier), _p(match), _p(found)), "amos_match_reloc_pnp")
        pose = bool(result[0]["has_pose"])
        return result[0], inlier, (match if pose else None), (found if pose else None), state

    def sim3_batch_device(self, d_kps, d_counts, d_points, cameras, d_pairs_1, d_pairs_2, n_pairs, d_match12, level_sigma2, params, capacity,
                          d_state, d_result, d_inlier, d_match_out):
        """LoopClosing::ComputeSim3's Sim3Solver (Sim3Solver.cc:48-523), one iterate() call per pair (keyframe-1 slot, keyframe-2 slot) on
        resident keyframes.  cameras: host SIM3_CAMERA_DTYPE records, one per frame slot; d_pairs_1 / d_pairs_2: device int32 [n_pairs];
        params: host SIM3_PARAMS_DTYPE records, one per pair; d_state: n_pairs blocks of sim3_state_bytes(capacity) bytes; d_result:
        SIM3_RESULT_DTYPE records.  Asynchronous on the matcher's stream."""
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        cams = np.ascontiguousarray(cameras, SIM3_CAMERA_DTYPE).reshape(-1)
        par = np.ascontiguousarray(params, SIM3_PARAMS_DTYPE).reshape(-1)
        if len(par) != n_pairs:
            raise ValueError("params holds one record per pair")
        s = Sim3(d_kps, d_counts, d_points, cams.ctypes.data, d_pairs_1, d_pairs_2, d_match12, sig.ctypes.data, par.ctypes.data, d_state, d_result,
                 d_inlier, d_match_out, len(cams), n_pairs, capacity, len(sig))
        _check(self.L.amos_match_sim3_batch_device(self.h, C.byref(s)), "amos_match_sim3_batch_device")

    def sim3(self, kps1, points1, kps2, points2, cameras, match12, level_sigma2, params, state=None):
        """The same for ONE pair from host arrays (amos_match_sim3): returns (result, inlier, match_out, state).  state: the blob an earlier
        call returned (params['reset'] = 0 goes on from it), or None for a fresh one.  match_out is None without a Sim3."""
        kps1, kps2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
        points1, points2 = np.ascontiguousarray(points1, SIM3_POINT_DTYPE), np.ascontiguousarray(points2, SIM3_POINT_DTYPE)
        cams = np.ascontiguousarray(cameras, SIM3_CAMERA_DTYPE).reshape(-1)
        match12 = np.ascontiguousarray(match12, np.int32)
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        par = np.ascontiguousarray(params, SIM3_PARAMS_DTYPE).reshape(1)
        n1, n2 = len(kps1), len(kps2)
        if len(points1) != n1 or len(points2) != n2 or len(match12) != n1 or len(cams) != 2:
            raise ValueError("points and match12 hold one entry per keypoint, cameras two records")
        nbytes = sim3_state_bytes(max(n1, 1))
        state = np.zeros(nbytes, np.uint8) if state is None else np.ascontiguousarray(state, np.uint8).copy()
        if len(state) != nbytes:
            raise ValueError("state is not a blob of sim3_state_bytes(n1) bytes")
        result = np.zeros(1, SIM3_RESULT_DTYPE)
        inlier, match_out = np.zeros(n1, np.uint8), np.full(n1, -1, np.int32)
        _check(self.L.amos_match_sim3(self.h, _p(kps1), _p(points1), n1, _p(kps2), _p(points2), n2, _p(cams), _p(match12), _p(sig), len(sig), _p(par),
                                      _p(state), _p(result), _p(inlier), _p(match_out)), "amos_match_sim3")
        return result[0], inlier, (match_out if result[0]["has_sim3"] else None), state

    def pose_optimization_batch_device(self, d_kps, d_counts, d_match, d_points, point_off, cameras, capacity, inv_level_sigma2, d_outlier,
                                       d_result, point_stride=12, flags_offset=-1, has_obs_bit=0, clear_outliers=False, d_u_right=None):
        """Optimizer::PoseOptimization for resident frames (Optimizer.cc:363-605), one launch: d_match / d_points are a search's output and
        input (point_stride / flags_offset / has_obs_bit say which record: amos_map_point 80 / 32 / 2, amos_last_point 64 / 20 / 2, bare
        float[3] 12 / -1).  point_off: n_frames + 1 host ints; cameras: host POSE_CAMERA_DTYPE records.  Writes d_outlier and POSE_RESULT_DTYPE
        records into d_result.  Asynchronous on the matcher's stream."""
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        off = np.ascontiguousarray(point_off, np.int32)
        cams = np.ascontiguousarray(cameras, POSE_CAMERA_DTYPE).reshape(-1)
        if len(off) != len(cams) + 1:
            raise ValueError("point_off holds one entry more than cameras")
        s = PoseOptimization(d_kps, d_u_right, d_counts, d_match, d_points, point_stride, flags_offset, has_obs_bit, off.ctypes.data,
                             cams.ctypes.data, sig.ctypes.data, d_outlier, d_result, len(cams), capacity, len(sig), int(bool(clear_outliers)))
        _check(self.L.amos_match_pose_optimization_batch_device(self.h, C.byref(s)), "amos_match_pose_optimization_batch_device")

    def pose_optimization(self, kps_un, match, points_xyz, camera, inv_level_sigma2, outlier=None, has_obs=None, clear_outliers=False,
                          u_right=None):
        """The same for ONE frame from host arrays (amos_match_pose_optimization): returns (result, outlier, match); the arguments are
        not modified.  outlier: what mvbOutlier holds on entry (zeros by default)."""
        kps_un = np.ascontiguousarray(kps_un, KP_DTYPE)
        n = len(kps_un)
        match = np.array(match, np.int32).reshape(-1)
        pts = np.ascontiguousarray(points_xyz, np.float32).reshape(-1, 3)
        cam = np.ascontiguousarray(camera, POSE_CAMERA_DTYPE).reshape(1)
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        ho = None if has_obs is None else np.ascontiguousarray(has_obs, np.uint8)
        outlier = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8).reshape(-1)
        if len(match) != n or len(outlier) != n or (ur is not None and len(ur) != n) or (ho is not None and len(ho) != len(pts)):
            raise ValueError("match, outlier and u_right hold one entry per keypoint, has_obs one per point")
        result = np.zeros(1, POSE_RESULT_DTYPE)
        _check(self.L.amos_match_pose_optimization(self.h, _p(kps_un), _p(ur), n, _p(match), _p(pts), _p(ho), len(pts), _p(cam), _p(sig), len(sig),
                                                   int(bool(clear_outliers)), _p(outlier), _p(result)), "amos_match_pose_optimization")
        return result[0], outlier, match

    def bow_batch_device(self, d_kps, d_desc, d_counts, d_n_nodes, d_node_ids, d_node_off, d_node_idx, d_pairs_kf, d_pairs_f, n_pairs, capacity,
                         d_match, d_stats, nn_ratio=0.7, check_orientation=True, d_has_point=None):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:230-382) for (keyframe slot, frame slot) pairs of resident frames
        whose FeatureVectors are BowVocabulary.transform_batch_device's CSR.  Asynchronous on the matcher's stream."""
        s = BowSearch(d_kps, d_desc, d_counts, d_n_nodes, d_node_ids, d_node_off, d_node_idx, d_has_point, d_pairs_kf, d_pairs_f, d_match, d_stats,
                      n_pairs, capacity, nn_ratio, int(bool(check_orientation)))
        _check(self.L.amos_match_bow_batch_device(self.h, C.byref(s)), "amos_match_bow_batch_device")

    @staticmethod
    def _bow_view(keys, desc, node_ids, node_off, node_idx, has_point=None, u_right=None):
        """-> (BowView, the arrays it points into)"""
        keys = np.ascontiguousarray(keys, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        ids, off, idx = np.ascontiguousarray(node_ids, np.uint32), np.ascontiguousarray(node_off, np.int32), np.ascontiguousarray(node_idx, np.int32)
        hp = None if has_point is None else np.ascontiguousarray(has_point, np.uint8)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        if len(desc) != len(keys) or (hp is not None and len(hp) != len(keys)) or (ur is not None and len(ur) != len(keys)) or \
                (len(ids) and len(off) != len(ids) + 1):
            raise ValueError("desc, has_point and u_right hold one entry per keypoint, node_off one more than node_ids")
        keep = (keys, desc, ids, off, idx, hp, ur)
        return BowView(len(keys), keys.ctypes.data, desc.ctypes.data, None if hp is None else hp.ctypes.data, None if ur is None else ur.ctypes.data,
                       len(ids), ids.ctypes.data, off.ctypes.data, idx.ctypes.data), keep

    def bow(self, kf, f, nn_ratio=0.7, check_orientation=True):
        """The same for ONE keyframe and ONE frame from host arrays (amos_match_bow).  kf and f are dicts with keys, desc, node_ids, node_off,
        node_idx and, for kf, optionally has_point.  Returns (matches_f, stats)."""
        vk, keep_k = self._bow_view(kf["keys"], kf["desc"], kf["node_ids"], kf["node_off"], kf["node_idx"], kf.get("has_point"))
        vf, keep_f = self._bow_view(f["keys"], f["desc"], f["node_ids"], f["node_off"], f["node_idx"])
        matches, stats = np.full(vf.n, -1, np.int32), np.zeros(1, BOW_SEARCH_STATS_DTYPE)
        _check(self.L.amos_match_bow(self.h, C.byref(vk), C.byref(vf), nn_ratio, int(bool(check_orientation)), _p(matches), _p(stats)),
               "amos_match_bow")
        return matches, stats[0]

    def bow_kf_batch_device(self, d_kps, d_desc, d_counts, d_n_nodes, d_node_ids, d_node_off, d_node_idx, d_pairs_1, d_pairs_2, n_pairs, capacity,
                            d_match12, d_stats, nn_ratio=0.75, check_orientation=True, d_has_point=None):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:656-799) for (keyframe-1 slot, keyframe-2 slot) pairs of resident
        frames (LoopClosing::ComputeSim3's call, once per loop candidate).  Asynchronous on the matcher's stream."""
        s = KfPairSearch(d_kps, d_desc, d_counts, d_n_nodes, d_node_ids, d_node_off, d_node_idx, d_has_point, None, d_pairs_1, d_pairs_2, d_match12,
                         d_stats, n_pairs, capacity)
        _check(self.L.amos_match_bow_kf_batch_device(self.h, C.byref(s), nn_ratio, int(bool(check_orientation))), "amos_match_bow_kf_batch_device")

    def bow_kf(self, k1, k2, nn_ratio=0.75, check_orientation=True):
        """The same for two keyframes from host arrays (amos_match_bow_kf).  k1 and k2 are dicts with keys, desc, node_ids, node_off, node_idx
        and optionally has_point.  Returns (match12, stats)."""
        v1, keep1 = self._bow_view(k1["keys"], k1["desc"], k1["node_ids"], k1["node_off"], k1["node_idx"], k1.get("has_point"))
        v2, keep2 = self._bow_view(k2["keys"], k2["desc"], k2["node_ids"], k2["node_off"], k2["node_idx"], k2.get("has_point"))
        match12, stats = np.full(v1.n, -1, np.int32), np.zeros(1, BOW_SEARCH_STATS_DTYPE)
        _check(self.L.amos_match_bow_kf(self.h, C.byref(v1), C.byref(v2), nn_ratio, int(bool(check_orientation)), _p(match12), _p(stats)),
               "amos_match_bow_kf")
        return match12, stats[0]

    def triangulation_batch_device(self, d_kps, d_desc, d_counts, d_n_nodes, d_node_ids, d_node_off, d_node_idx, d_pairs_1, d_pairs_2, n_pairs,
                                   capacity, d_geometry, d_scale_factors, d_level_sigma2, n_levels, d_match12, d_stats, only_stereo=False,
                                   check_orientation=True, d_has_point=None, d_u_right=None):
        """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:810-1009) for (keyframe-1 slot, keyframe-2 slot) pairs of resident frames
        (LocalMapping::CreateNewMapPoints' call, once per neighbour).  d_geometry: KF_GEOMETRY_DTYPE records, one per pair.  Asynchronous on
        the matcher's stream."""
        s = KfPairSearch(d_kps, d_desc, d_counts, d_n_nodes, d_node_ids, d_node_off, d_node_idx, d_has_point, d_u_right, d_pairs_1, d_pairs_2,
                         d_match12, d_stats, n_pairs, capacity)
        _check(self.L.amos_match_triangulation_batch_device(self.h, C.byref(s), d_geometry, d_scale_factors, d_level_sigma2, n_levels,
                                                            int(bool(only_stereo)), int(bool(check_orientation))),
               "amos_match_triangulation_batch_device")

    def triangulation(self, k1, k2s, geometry, scale_factors, level_sigma2, only_stereo=False, check_orientation=True):
        """The same for ONE keyframe 1 against the keyframes k2s from host arrays (amos_match_triangulation): dicts as for bow_kf, has_point
        meaning "has a map point" and u_right optional.  geometry: KF_GEOMETRY_DTYPE records, one per keyframe 2.  Returns (match12
        [len(k2s)][n1], stats [len(k2s)])."""
        def view(k):
            return self._bow_view(k["keys"], k["desc"], k["node_ids"], k["node_off"], k["node_idx"], k.get("has_point"), k.get("u_right"))
        v1, keep1 = view(k1)
        views = [view(k) for k in k2s]
        geo = np.ascontiguousarray(geometry, KF_GEOMETRY_DTYPE).reshape(-1)
        sf, sg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
        if len(geo) != len(views) or len(sf) != len(sg):
            raise ValueError("geometry holds one record per keyframe 2, scale_factors and level_sigma2 one entry per level")
        ptrs = (C.c_void_p * max(len(views), 1))(*[C.addressof(v) for v, _ in views])
        match12, stats = np.full((len(views), v1.n), -1, np.int32), np.zeros(len(views), BOW_SEARCH_STATS_DTYPE)
        _check(self.L.amos_match_triangulation(self.h, C.byref(v1), ptrs, len(views), _p(geo), _p(sf), _p(sg), len(sf), int(bool(only_stereo)),
                                               int(bool(check_orientation)), _p(match12), _p(stats)), "amos_match_triangulation")
        return match12, stats

    def new_points_batch_device(self, d_kps, d_counts, d_pairs_1, d_pairs_2, pairs, capacity, d_match12, d_scale_factors, d_level_sigma2, n_levels,
                                cameras, d_new, d_stats, d_verdict=None, d_u_right=None, d_depth=None, d_kps_raw=None, enabled=None):
        """LocalMapping::CreateNewMapPoints between its search and its `new MapPoint` (LocalMapping.cc:424-597) for the pairs of one
        triangulation_batch_device call, reading d_match12 in place (amos_match_new_points_batch_device).  pairs: the host (slot 1, slot 2)
        pairs that d_pairs_1 / d_pairs_2 hold; cameras: host KF_CAMERA_DTYPE records, one per frame slot; enabled: host flags, one per pair
        (a neighbour that failed the baseline gate: 0), or None.  Asynchronous on the matcher's stream."""
        cams = np.ascontiguousarray(cameras, KF_CAMERA_DTYPE).reshape(-1)
        prs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        p1, p2 = np.ascontiguousarray(prs[:, 0]), np.ascontiguousarray(prs[:, 1])
        en = None if enabled is None else np.ascontiguousarray(enabled, np.uint8)
        if en is not None and len(en) != len(prs):
            raise ValueError("enabled holds one flag per pair")
        s = NewPoints(d_kps, d_kps_raw, d_counts, d_u_right, d_depth, d_pairs_1, d_pairs_2, d_match12, d_scale_factors, d_level_sigma2,
                      cams.ctypes.data, p1.ctypes.data, p2.ctypes.data, None if en is None else en.ctypes.data, d_new, d_verdict, d_stats, len(cams),
                      len(prs), capacity, n_levels)
        _check(self.L.amos_match_new_points_batch_device(self.h, C.byref(s)), "amos_match_new_points_batch_device")

    def new_points(self, k1, k2s, cam1, cams2, scale_factors, level_sigma2, only_stereo=False, check_orientation=False):
        """The whole of CreateNewMapPoints up to `new MapPoint` for ONE keyframe 1 against the keyframes k2s from host arrays
        (amos_match_new_points): dicts as for triangulation plus depth (float32 per feature; needed with u_right) and optionally keys_raw
        (mvKeys; default: keys).  cam1 / cams2: KF_CAMERA_DTYPE records.  Returns (one NEW_POINT_DTYPE array per keyframe 2 in creation order,
        stats [len(k2s)]); a neighbour that fails the baseline gate has zero stats."""
        def view(k):
            return self._bow_view(k["keys"], k["desc"], k["node_ids"], k["node_off"], k["node_idx"], k.get("has_point"), k.get("u_right"))

        def extra(k, n):
            raw = None if k.get("keys_raw") is None else np.ascontiguousarray(k["keys_raw"], KP_DTYPE)
            depth = None if k.get("depth") is None else np.ascontiguousarray(k["depth"], np.float32)
            if (raw is not None and len(raw) != n) or (depth is not None and len(depth) != n):
                raise ValueError("keys_raw and depth hold one entry per keypoint")
            return raw, depth
        v1, keep1 = view(k1)
        views = [view(k) for k in k2s]
        raw1, depth1 = extra(k1, v1.n)
        extras = [extra(k, v.n) for k, (v, _) in zip(k2s, views)]
        c1 = np.ascontiguousarray(cam1, KF_CAMERA_DTYPE).reshape(1)
        c2 = np.ascontiguousarray(cams2, KF_CAMERA_DTYPE).reshape(-1)
        sf, sg = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
        if len(c2) != len(views) or len(sf) != len(sg):
            raise ValueError("cams2 holds one record per keyframe 2, scale_factors and level_sigma2 one entry per level")
        n2 = len(views)
        ptrs = (C.c_void_p * max(n2, 1))(*[C.addressof(v) for v, _ in views])
        raws = (C.c_void_p * max(n2, 1))(*[None if r is None else r.ctypes.data for r, _ in extras])
        depths = (C.c_void_p * max(n2, 1))(*[None if d is None else d.ctypes.data for _, d in extras])
        rows, stats = np.zeros((n2, max(v1.n, 1)), NEW_POINT_DTYPE), np.zeros(n2, NEW_POINTS_STATS_DTYPE)
        _check(self.L.amos_match_new_points(self.h, C.byref(v1), ptrs, n2, _p(c1), _p(c2), _p(raw1), raws, _p(depth1), depths, _p(sf), _p(sg), len(sf),
                                            int(bool(only_stereo)), int(bool(check_orientation)), _p(rows), _p(stats)), "amos_match_new_points")
        if v1.n == 0:
            return [np.zeros(0, NEW_POINT_DTYPE) for _ in range(n2)], stats
        return [rows[k, :stats["n_new"][k]].copy() for k in range(n2)], stats

    def fuse_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, d_points, n_points, n_frames, pair_frame, point_first, point_count,
                          out_off, cameras, capacity, scale_factors, inv_level_sigma2, d_query, d_in_view, d_best_idx, d_best_dist, d_stats,
                          mode=FUSE_LOCAL, max_dist=50, bounds=(0.0, 640.0, 0.0, 480.0), d_u_right=None, d_skip=None):
        """ORBmatcher::Fuse (ORBmatcher.cc:1020-1177; FUSE_SIM3: :1179-1312) without its write-back for (keyframe slot, point range, camera)
        pairs of resident keyframes: the pre-filter and the search of every point in one launch.  pair_frame, point_first, point_count, out_off:
        host ints, one per pair; cameras: host FUSE_CAMERA_DTYPE records.  Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        pf, p0, pc, oo = (np.ascontiguousarray(a, np.int32) for a in (pair_frame, point_first, point_count, out_off))
        cams = np.ascontiguousarray(cameras, FUSE_CAMERA_DTYPE).reshape(-1)
        if not (len(pf) == len(p0) == len(pc) == len(oo) == len(cams)) or (s2 is not None and len(s2) != len(sf)):
            raise ValueError("one entry per pair in pair_frame, point_first, point_count, out_off and cameras; one per level in the tables")
        s = FuseSearch(d_kps, d_desc, d_counts, d_cell_start, d_items, d_u_right, sf.ctypes.data, _p(s2), d_points, _p(pf), _p(p0), _p(pc), _p(oo),
                       _p(cams), d_skip, d_query, d_in_view, d_best_idx, d_best_dist, d_stats, n_frames, len(cams), n_points, capacity, len(sf), mode,
                       max_dist, *bounds)
        _check(self.L.amos_match_fuse_batch_device(self.h, C.byref(s)), "amos_match_fuse_batch_device")

    def fuse(self, kfs, points, pair_frame, point_first, point_count, out_off, cameras, scale_factors, inv_level_sigma2, n_out, skip=None,
             mode=FUSE_LOCAL, max_dist=50, bounds=(0.0, 640.0, 0.0, 480.0)):
        """The same from host arrays (amos_match_fuse): kfs is a list of dicts with keys_un, desc and optionally u_right.  Returns (query,
        in_view, best_idx, best_dist, stats); entries no pair owns keep query 0, in_view 0, best_idx -1, best_dist 256."""
        keep, views = [], (FrameView * max(len(kfs), 1))()
        for v, k in zip(views, kfs):
            kp, d = np.ascontiguousarray(k["keys_un"], KP_DTYPE), np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
            ur = None if k.get("u_right") is None else np.ascontiguousarray(k["u_right"], np.float32)
            keep.append((kp, d, ur))
            v.n, v.keys_un, v.descriptors, v.u_right = len(kp), kp.ctypes.data, d.ctypes.data, None if ur is None else ur.ctypes.data
            v.min_x, v.max_x, v.min_y, v.max_y = bounds
        points = np.ascontiguousarray(points, MAP_POINT_DTYPE)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        pf, p0, pc, oo = (np.ascontiguousarray(a, np.int32) for a in (pair_frame, point_first, point_count, out_off))
        cams = np.ascontiguousarray(cameras, FUSE_CAMERA_DTYPE).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        query, in_view = np.zeros(n_out, WINDOW_QUERY_DTYPE), np.zeros(n_out, np.uint8)
        best_idx, best_dist, stats = np.full(n_out, -1, np.int32), np.full(n_out, 256, np.int32), np.zeros(len(cams), FUSE_STATS_DTYPE)
        _check(self.L.amos_match_fuse(self.h, views, len(kfs), _p(points), len(points), len(cams), _p(pf), _p(p0), _p(pc), _p(oo), _p(cams), _p(sk),
                                      n_out, _p(sf), _p(s2), len(sf), mode, max_dist, _p(query), _p(in_view), _p(best_idx), _p(best_dist),
                                      _p(stats)), "amos_match_fuse")
        return query, in_view, best_idx, best_dist, stats

    def sim3_search_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, d_points, cameras, d_pairs_1, d_pairs_2, pairs, d_match12,
                                 d_match_out, d_match1, d_match2, d_stats, capacity, scale_factors, bounds=(0.0, 640.0, 0.0, 480.0), d_sim3=None):
        """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1314-1555) for pairs (keyframe-1 slot, keyframe-2 slot) of resident keyframes: both
        directions and the agreement pass in two launches.  cameras: host SIM3_CAMERA_DTYPE records, one per frame slot; pairs: host
        SIM3_SEARCH_PAIR_DTYPE records, one per pair; d_sim3: the solver's d_result (its Sim3 replaces the records'), or None; d_match_out
        may be d_match12.  Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        cams = np.ascontiguousarray(cameras, SIM3_CAMERA_DTYPE).reshape(-1)
        prs = np.ascontiguousarray(pairs, SIM3_SEARCH_PAIR_DTYPE).reshape(-1)
        s = Sim3Search(d_kps, d_desc, d_counts, d_cell_start, d_items, d_points, cams.ctypes.data, sf.ctypes.data, d_pairs_1, d_pairs_2,
                       prs.ctypes.data, d_sim3, d_match12, d_match_out, d_match1, d_match2, d_stats, len(cams), len(prs), capacity, len(sf), *bounds)
        _check(self.L.amos_match_sim3_search_batch_device(self.h, C.byref(s)), "amos_match_sim3_search_batch_device")

    def sim3_search(self, kf1, points1, kf2, points2, cameras, pair, scale_factors, match12, bounds=(0.0, 640.0, 0.0, 480.0)):
        """The same for ONE pair from host arrays (amos_match_sim3_search): kf1 / kf2 are dicts with keys_un and desc, cameras two
        SIM3_CAMERA_DTYPE records (KF1's, KF2's).  Returns (match_out, match1, match2, stats); a skipped pair returns match12 and -1 rows."""
        keep, views = [], (FrameView * 2)()
        for v, k in zip(views, (kf1, kf2)):
            kp, d = np.ascontiguousarray(k["keys_un"], KP_DTYPE), np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
            keep.append((kp, d))
            v.n, v.keys_un, v.descriptors, v.u_right = len(kp), kp.ctypes.data, d.ctypes.data, None
            v.min_x, v.max_x, v.min_y, v.max_y = bounds
        points1, points2 = np.ascontiguousarray(points1, MAP_POINT_DTYPE), np.ascontiguousarray(points2, MAP_POINT_DTYPE)
        n1, n2 = views[0].n, views[1].n
        if len(points1) != n1 or len(points2) != n2 or len(match12) != n1:
            raise ValueError("one point record per feature of each keyframe and one row entry per feature of keyframe 1")
        cams = np.ascontiguousarray(cameras, SIM3_CAMERA_DTYPE).reshape(2)
        pr = np.ascontiguousarray(pair, SIM3_SEARCH_PAIR_DTYPE).reshape(1)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        match12 = np.ascontiguousarray(match12, np.int32)
        match_out, match1, match2 = match12.copy(), np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
        stats = np.zeros(1, SIM3_SEARCH_STATS_DTYPE)
        _check(self.L.amos_match_sim3_search(self.h, C.addressof(views[0]), _p(points1), C.addressof(views[1]), _p(points2), _p(cams), _p(pr), _p(sf),
                                             len(sf), _p(match12), _p(match_out), _p(match1), _p(match2), _p(stats)), "amos_match_sim3_search")
        return match_out, match1, match2, stats[0]

    def sim3_optimize_batch_device(self, d_kps, d_counts, d_points, cameras, d_pairs_1, d_pairs_2, pairs, d_match12, d_match_out, d_result,
                                   capacity, inv_level_sigma2, d_sim3=None):
        """Optimizer::OptimizeSim3 (Optimizer.cc:1364-1590) for pairs (keyframe-1 slot, keyframe-2 slot) of resident keyframes, one launch.
        cameras: host SIM3_CAMERA_DTYPE records, one per frame slot; pairs: host SIM3_OPT_PAIR_DTYPE records, one per pair; d_sim3: the
        solver's d_result (its Sim3 replaces the records'), or None; d_match_out may be d_match12; d_result: SIM3_OPT_RESULT_DTYPE records.
        Asynchronous on the matcher's stream."""
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        cams = np.ascontiguousarray(cameras, SIM3_CAMERA_DTYPE).reshape(-1)
        prs = np.ascontiguousarray(pairs, SIM3_OPT_PAIR_DTYPE).reshape(-1)
        s = Sim3Optimize(d_kps, d_counts, d_points, cams.ctypes.data, d_pairs_1, d_pairs_2, sig.ctypes.data, prs.ctypes.data, d_sim3, d_match12,
                         d_match_out, d_result, len(cams), len(prs), capacity, len(sig))
        _check(self.L.amos_match_sim3_optimize_batch_device(self.h, C.byref(s)), "amos_match_sim3_optimize_batch_device")

    def sim3_optimize(self, kps1, points1, kps2, points2, cameras, match12, inv_level_sigma2, pair):
        """The same for ONE pair from host arrays (amos_match_sim3_optimize): returns (result, match_out); a skipped pair returns match12."""
        kps1, kps2 = np.ascontiguousarray(kps1, KP_DTYPE), np.ascontiguousarray(kps2, KP_DTYPE)
        points1, points2 = np.ascontiguousarray(points1, SIM3_POINT_DTYPE), np.ascontiguousarray(points2, SIM3_POINT_DTYPE)
        cams = np.ascontiguousarray(cameras, SIM3_CAMERA_DTYPE).reshape(-1)
        match12 = np.ascontiguousarray(match12, np.int32)
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        pr = np.ascontiguousarray(pair, SIM3_OPT_PAIR_DTYPE).reshape(1)
        n1, n2 = len(kps1), len(kps2)
        if len(points1) != n1 or len(points2) != n2 or len(match12) != n1 or len(cams) != 2:
            raise ValueError("points and match12 hold one entry per keypoint, cameras two records")
        result, match_out = np.zeros(1, SIM3_OPT_RESULT_DTYPE), match12.copy()
        _check(self.L.amos_match_sim3_optimize(self.h, _p(kps1), _p(points1), n1, _p(kps2), _p(points2), n2, _p(cams), _p(match12), _p(sig), len(sig),
                                               _p(pr), _p(match_out), _p(result)), "amos_match_sim3_optimize")
        return result[0], match_out

    def loop_points_batch_device(self, d_kps, d_desc, d_counts, d_cell_start, d_items, n_frames, d_points, n_points, point_first, point_count, queries,
                                 d_matched, d_loop_match, d_stats, capacity, scale_factors, bounds=(0.0, 640.0, 0.0, 480.0), d_opt=None, d_found=None,
                                 d_point_of_feature2=None):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:388-512) and nTotalMatches >= min_total
        (LoopClosing.cc:538-546) for queries (keyframe slot, point range, Scw, row) on resident keyframes.  point_first, point_count: host ints,
        one per query; queries: host LOOP_POINTS_QUERY_DTYPE records; d_opt: amos_match_sim3_optimize_batch_device's d_result (its Scw replaces
        the records', and its rows decide which queries run), or None.  Asynchronous on the matcher's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        p0, pc = (np.ascontiguousarray(a, np.int32) for a in (point_first, point_count))
        qs = np.ascontiguousarray(queries, LOOP_POINTS_QUERY_DTYPE).reshape(-1)
        if not (len(p0) == len(pc) == len(qs)):
            raise ValueError("one entry per query in point_first, point_count and queries")
        s = LoopPointsSearch(d_kps, d_desc, d_counts, d_cell_start, d_items, sf.ctypes.data, d_points, _p(p0), _p(pc), qs.ctypes.data, d_opt, d_matched,
                             d_found, d_point_of_feature2, d_loop_match, d_stats, n_frames, len(qs), n_points, capacity, len(sf), *bounds)
        _check(self.L.amos_match_loop_points_batch_device(self.h, C.byref(s)), "amos_match_loop_points_batch_device")

    def loop_points(self, kf, points, query, scale_factors, matched=None, found=None, point_of_feature2=None, bounds=(0.0, 640.0, 0.0, 480.0)):
        """The same for ONE query from host arrays (amos_match_loop_points): kf is a dict with keys_un and desc.  Returns (loop_match, stats);
        a skipped query returns a row of -1."""
        kp, d = np.ascontiguousarray(kf["keys_un"], KP_DTYPE), np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32)
        view = FrameView()
        view.n, view.keys_un, view.descriptors, view.u_right = len(kp), kp.ctypes.data, d.ctypes.data, None
        view.min_x, view.max_x, view.min_y, view.max_y = bounds
        points = np.ascontiguousarray(points, MAP_POINT_DTYPE)
        q = np.ascontiguousarray(query, LOOP_POINTS_QUERY_DTYPE).reshape(1)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        row = None if matched is None else np.ascontiguousarray(matched, np.int32)
        fd = None if found is None else np.ascontiguousarray(found, np.uint8)
        pf2 = None if point_of_feature2 is None else np.ascontiguousarray(point_of_feature2, np.int32)
        if (row is not None and len(row) != len(kp)) or (fd is not None and len(fd) != len(points)):
            raise ValueError("one row entry per feature and one found byte per point")
        loop_match, stats = np.full(len(kp), -1, np.int32), np.zeros(1, LOOP_POINTS_STATS_DTYPE)
        _check(self.L.amos_match_loop_points(self.h, C.addressof(view), _p(points), len(points), _p(q), _p(row), _p(fd), _p(pf2),
                                             0 if pf2 is None else len(pf2), _p(sf), len(sf), _p(loop_match), _p(stats)), "amos_match_loop_points")
        return loop_match, stats[0]

    def sync(self):
        _check(self.L.amos_match_sync(self.h), "amos_match_sync")


class CornerDetector(_Handle):
    """amos_corners_*: cv::goodFeaturesToTrack (Harris) + cv::cornerSubPix of Tracking::GetSceneFlowObj (Tracking.cc:894-895) on
    device-resident gray frames; the corners stay on the device (feed LkTracker.track_device)."""

    _kind = "corners"

    def __init__(self, max_width=640, max_height=480, device=0, stream=None):
        self._open(device, stream, max_width, max_height)

    def good_features_device(self, gray_ptr, stride, width, height, xy_ptr, xy_capacity, count_ptr, max_corners=1000, quality=0.01, min_distance=8.0,
                             harris_k=0.04, response_ptr=None):
        _check(self.L.amos_corners_good_features_device(self.h, gray_ptr, stride, width, height, max_corners, quality, min_distance, harris_k, xy_ptr, xy_capacity,
                                                        count_ptr, response_ptr), "amos_corners_good_features_device")

    def candidate_count(self):
        n = C.c_int(0)
        _check(self.L.amos_corners_candidate_count(self.h, C.byref(n)), "amos_corners_candidate_count")
        return n.value

    def subpix_device(self, gray_ptr, stride, width, height, xy_ptr, count_ptr=None, n=0, win=10, max_count=20, epsilon=0.03):
        _check(self.L.amos_corners_subpix_device(self.h, gray_ptr, stride, width, height, xy_ptr, count_ptr, n, win, max_count, epsilon),
               "amos_corners_subpix_device")


class FundamentalRansac(_Handle):
    """amos_fmat_*: cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence) of Tracking::GetSceneFlowObj (Tracking.cc:927, 945) on the
    device (restated, parity with OpenCV unpinned).  status = (result, inliers, iterations, points): result 1 model, 0 none, -1 for
    7 <= points < 15 (OpenCV's LMeDS branch, not built), -2 sampler cap, -3 count out of range."""

    _kind = "fmat"

    def __init__(self, max_points=4096, max_problems=64, device=0, stream=None):
        self._open(device, stream, max_points, max_problems)
        self.max_points = max_points

    def ransac(self, p1, p2, threshold=0.1, confidence=0.99, max_iters=1000):
        """One problem from host arrays [n][2]: returns (F [3][3] float64, mask [n] uint8, status [4] int32)."""
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
        assert len(p1) == len(p2)
        F, mask, status = np.zeros(9), np.zeros(len(p1), np.uint8), np.zeros(4, np.int32)
        _check(self.L.amos_fmat_ransac(self.h, len(p1), _p(p1), _p(p2), threshold, confidence, max_iters, _p(F), _p(mask), _p(status)), "amos_fmat_ransac")
        return F.reshape(3, 3), mask, status

    def ransac_device(self, n_problems, d_p1, d_p2, d_offsets, d_counts, d_select, d_F, d_status, d_mask=None, threshold=0.1, confidence=0.99, max_iters=1000):
        _check(self.L.amos_fmat_ransac_device(self.h, n_problems, d_p1, d_p2, d_offsets, d_counts, d_select, threshold, confidence, max_iters, d_F, d_status,
                                              d_mask), "amos_fmat_ransac_device")

    def scene_flow_pair_device(self, d_pre, d_next, d_state, d_n, d_F1, d_F2, d_keep, d_status):
        """Tracking.cc:927-945: F1 on state != 0, keep = dd <= 0.5 under F1, F2 on keep; d_status [2][4]."""
        _check(self.L.amos_fmat_scene_flow_pair_device(self.h, d_pre, d_next, d_state, d_n, d_F1, d_F2, d_keep, d_status), "amos_fmat_scene_flow_pair_device")


class PnpRansac(_Handle):
    """amos_pnp_*: cv::solvePnPRansac(obj, img, K, 0, ..., SOLVEPNP_P3P) of Tracking::GetSceneFlowObj (Tracking.cc:1006) on the device: the
    RANSAC over P3P samples, then the EPnP refit on its inliers (restated, parity with OpenCV unpinned).  status = (result, inliers,
    iterations, points, refit): result 1 model, 0 none, -1 fewer than 4 points, -2 sampler cap, -3 count out of range; refit 1 EPnP
    refit returned, -1 refit not finite (the RANSAC model returned), 0 none.  Poses are R | t: R row-major, then t."""

    _kind = "pnp"

    def __init__(self, max_points=4096, max_problems=64, device=0, stream=None):
        self._open(device, stream, max_points, max_problems)
        self.max_points = max_points

    def ransac(self, obj, img, fx, fy, cx, cy, reprojection_error=0.4, confidence=0.98, max_iters=500):
        """One problem from host arrays obj [n][3], img [n][2]: returns (Rt [12] float64, mask [n] uint8, status [5] int32)."""
        obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        assert len(obj) == len(img)
        Rt, mask, status = np.zeros(12), np.zeros(len(obj), np.uint8), np.zeros(5, np.int32)
        _check(self.L.amos_pnp_ransac(self.h, len(obj), _p(obj), _p(img), fx, fy, cx, cy, reprojection_error, confidence, max_iters, _p(Rt), _p(mask), _p(status)),
               "amos_pnp_ransac")
        return Rt, mask, status

    def ransac_device(self, n_problems, d_obj, d_img, d_offsets, d_counts, d_select, fx, fy, cx, cy, d_Rt, d_status, d_mask=None,
                      reprojection_error=0.4, confidence=0.98, max_iters=500):
        _check(self.L.amos_pnp_ransac_device(self.h, n_problems, d_obj, d_img, d_offsets, d_counts, d_select, fx, fy, cx, cy, reprojection_error, confidence,
                                             max_iters, d_Rt, d_status, d_mask), "amos_pnp_ransac_device")

    def scene_flow_device(self, d_pre, d_next, d_state, d_n, d_depth_last, last_stride, d_depth_cur, cur_stride, width, height, cam, fx, fy,
                          d_Rt, d_status, d_mask=None):
        """Tracking.cc:955-1007: the point lists (pre_3d -> next where both depths > 0, (0,0,0) -> (0,0) elsewhere) over state != 0, then
        solvePnPRansac(500, 0.4, 0.98); strides in floats; cam a SceneFlowCamera; d_Rt [12], d_status [5]."""
        _check(self.L.amos_pnp_scene_flow_device(self.h, d_pre, d_next, d_state, d_n, d_depth_last, last_stride, d_depth_cur, cur_stride, width, height,
                                                 C.byref(cam), fx, fy, d_Rt, d_status, d_mask), "amos_pnp_scene_flow_device")


DYNA_MAX_K, DYNA_COUNTS = 64, 6
DYNA_NO_PNP, DYNA_NO_F2, DYNA_BAD_N, DYNA_RESET = 1, 2, 4, 8
DYNA_BAD_MATCH_LABEL, DYNA_BAD_TM_LABEL, DYNA_BAD_ID = 1, 2, 4


class DynaPoses(C.Structure):
    """amos_dyna_poses: MotionModel and computeMtcwUseLK's mTcw as rows of [R | t] (3 x 4 floats)."""
    _fields_ = [("motion", C.c_float * 12), ("lk", C.c_float * 12), ("has_lk", C.c_int32)]

    @classmethod
    def of(cls, motion, lk=None):
        p = cls()
        for i, v in enumerate(np.asarray(motion, np.float32).reshape(-1)[:12]):
            p.motion[i] = float(v)
        if lk is not None:
            for i, v in enumerate(np.asarray(lk, np.float32).reshape(-1)[:12]):
                p.lk[i] = float(v)
            p.has_lk = 1
        return p


class DynaResults(C.Structure):
    """amos_dyna_results: device addresses of the per-slot arrays (see include/amos_frontend.h)."""
    _fields_ = [("max_points", C.c_int32), ("max_frames", C.c_int32)] + [(k, C.c_void_p) for k in (
        "pose", "rwc", "ow", "choice", "counts", "match_xy", "rpe", "epipolar", "tm_xy", "flow", "status", "ave_rpe", "ep_num", "decide_status",
        "pre_xy", "next_xy", "state", "n", "F1", "F2", "fmat_status", "Rt", "pnp_status")]


class SceneFlowDyna(_Handle):
    """amos_dyna_*: the tail of Tracking::GetSceneFlowObj (Tracking.cc:1012-1184: both poses' reprojection errors, the choice, SetPose,
    mvepipolar / T_M under F2, vFlow_3d) and CalDyna's moving-cluster decision (Frame.cc:552-628) on the device, per result slot."""

    _kind = "dyna"

    def __init__(self, max_points=4096, max_frames=64, device=0, stream=None):
        self._open(device, stream, max_points, max_frames)
        self.max_points, self.max_frames = max_points, max_frames
        self.results = DynaResults()
        _check(self.L.amos_dyna_results_device(self.h, C.byref(self.results)), "amos_dyna_results_device")

    def tail_device(self, frame, d_pre, d_next, d_state, d_n, d_F2, d_fmat_status, d_Rt, d_pnp_status, d_depth_last, last_stride, d_depth_cur,
                    cur_stride, width, height, cam, fx, fy, poses):
        """Tracking.cc:1012-1184 into slot `frame`; strides in floats; cam a SceneFlowCamera, poses a DynaPoses."""
        _check(self.L.amos_dyna_tail_device(self.h, frame, d_pre, d_next, d_state, d_n, d_F2, d_fmat_status, d_Rt, d_pnp_status, d_depth_last, last_stride,
                                            d_depth_cur, cur_stride, width, height, C.byref(cam), fx, fy, C.byref(poses)), "amos_dyna_tail_device")

    def reset_frame_device(self, frame):
        _check(self.L.amos_dyna_reset_frame_device(self.h, frame), "amos_dyna_reset_frame_device")

    def decide_batch_device(self, n_frames, d_labels, label_frame_stride, label_row_stride, width, height, d_centers, centers_frame_stride, n_centers,
                            k, d_rm, rm_frame_stride):
        """Frame.cc:552-628 for slots 0 .. n_frames - 1: rm int32 [n_frames][rm_frame_stride] (k entries); strides in elements."""
        _check(self.L.amos_dyna_decide_batch_device(self.h, n_frames, d_labels, label_frame_stride, label_row_stride, width, height, d_centers, centers_frame_stride,
                                                    n_centers, k, d_rm, rm_frame_stride), "amos_dyna_decide_batch_device")

    def scene_flow_obj_device(self, frame, corners, lk, fmat, pnp, d_imlast, last_gray_stride, d_gray, gray_stride, width, height, d_depth_last,
                              last_stride, d_depth_cur, cur_stride, cam, fx, fy, poses):
        """The whole of GetSceneFlowObj (Tracking.cc:894-1184) as one call on the four handles (same stream as this one)."""
        _check(self.L.amos_dyna_scene_flow_obj_device(self.h, frame, corners.h, lk.h, fmat.h, pnp.h, d_imlast, last_gray_stride, d_gray, gray_stride, width, height,
                                                      d_depth_last, last_stride, d_depth_cur, cur_stride, C.byref(cam), fx, fy, C.byref(poses)),
               "amos_dyna_scene_flow_obj_device")

    def _get(self, addr, dtype, count, offset=0):
        out = np.zeros(count, dtype)
        if count:
            _check(self.L.amos_dyna_copy_to_host(self.h, out.ctypes.data, addr + offset * np.dtype(dtype).itemsize, out.nbytes), "amos_dyna_copy_to_host")
        return out

    def fetch(self, frame, n_tracked=0, k=0):
        """Slot `frame` copied to the host (synchronous): a dict of numpy arrays, lists cut to their counts; mvepipolar has n_tracked
        entries, AveClusterRpe / epNum k (from the last decide)."""
        r, P = self.results, self.max_points
        counts = self._get(r.counts, np.int32, DYNA_COUNTS, DYNA_COUNTS * frame)
        N, V, _, _, T, F = (int(c) for c in counts)
        return dict(
            counts=counts, pose=self._get(r.pose, np.float32, 12, 12 * frame), rwc=self._get(r.rwc, np.float32, 9, 9 * frame),
            ow=self._get(r.ow, np.float32, 3, 3 * frame), choice=int(self._get(r.choice, np.int32, 1, frame)[0]),
            status=int(self._get(r.status, np.int32, 1, frame)[0]),
            match=self._get(r.match_xy, np.float32, 2 * V, 2 * P * frame).reshape(-1, 2), rpe=self._get(r.rpe, np.float32, V, P * frame),
            epipolar=self._get(r.epipolar, np.float64, n_tracked, P * frame), tm=self._get(r.tm_xy, np.float32, 2 * T, 2 * P * frame).reshape(-1, 2),
            flow=self._get(r.flow, np.float32, 3 * F, 3 * P * frame).reshape(-1, 3),
            ave_rpe=self._get(r.ave_rpe, np.float32, k, DYNA_MAX_K * frame), ep_num=self._get(r.ep_num, np.int32, k, DYNA_MAX_K * frame),
            decide_status=int(self._get(r.decide_status, np.int32, 1, frame)[0]))
