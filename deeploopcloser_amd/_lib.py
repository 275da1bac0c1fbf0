"""ctypes binding of the C ABI in include/dlc.h (libdlc_hip.so, built in-tree).

There is NO CPU fallback: if the shared library is missing or no MI355X is
visible the product path raises.  The CPU oracle under ``oracle/`` is test
infrastructure and is never imported from here.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdlc_hip.so")

DLC_OK = 0
DLC_ERR_BAD_ARG, DLC_ERR_BAD_SHAPE, DLC_ERR_UNSUPPORTED, DLC_ERR_HIP, DLC_ERR_WORKSPACE = -1, -2, -3, -4, -5
DLC_BF16, DLC_F16, DLC_F32, DLC_F64, DLC_I8, DLC_U8, DLC_I64 = 0, 1, 2, 3, 4, 5, 6
DLC_ACT_NONE, DLC_ACT_SIGMOID, DLC_ACT_RELU = 0, 1, 2
DLC_B_KN, DLC_B_NK = 0, 1
DLC_MAX_K = 128
DLC_MAX_STEP = 8             # the largest step of the elastic sequence search (d_max)
DLC_MAX_SHIFT = 8            # the largest lateral shift of dlc_sad_u8_shift_rows (thumbnail columns)
DLC_ABI_VERSION = 20        # include/dlc.h; load() refuses a library built from another header
DLC_SELECT_COOP, DLC_SELECT_NO_HINTS, DLC_SELECT_SERIAL = 1, 2, 4
DLC_PRUNE_ON, DLC_PRUNE_OFF, DLC_PRUNE_KEEP = 0, 1, 2     # dlc_set_prune_mode
DLC_SIM_FORCE_F64, DLC_SIM_NO_HOST_SYNC = 1, 2
DLC_MAX_FUSE = 8             # the most score sources dlc_fuse_rows takes
DLC_FUSE_NONE, DLC_FUSE_ZSCORE, DLC_FUSE_MINMAX = 0, 1, 2
DLC_FUSE_PLAN_AUTO, DLC_FUSE_PLAN_ROW, DLC_FUSE_PLAN_SLAB = 0, 1, 2
DLC_TRACK_AUTO, DLC_TRACK_RESIDENT, DLC_TRACK_ROWS = 0, 1, 2
DLC_TRACK_RESIDENT_MAX = 8192   # the most columns the RESIDENT plan of dlc_track_rows keeps in LDS
DLC_TRACK_JUMP, DLC_TRACK_FROM_NULL, DLC_TRACK_ORIGIN, DLC_TRACK_ABSENT = -1, -2, -3, -128     # back-pointer codes
DLC_TRACK_END_FILTERED, DLC_TRACK_NO_PATH = -2, -2
DLC_VLAD_MAX_WORDS, DLC_VLAD_MAX_PATCHES = 256, 1024   # the most words of a codebook and patches of a frame (dlc_vlad_encode)
DLC_KMEANS_BLOCK = 1024      # rows of a block of dlc_kmeans_step's member sums (the leaves of its TREE)
DLC_VLAD_NORM_NONE, DLC_VLAD_NORM_INTRA = 0, 1
DLC_PCA_CHUNK = 1024         # columns of x of one serial chain of dlc_pca_project; the chunks' sums are added in order
DLC_PCA_MAX_COMPONENTS, DLC_PCA_SPLIT_MAX_ROWS = 8192, 64
DLC_PCA_PLAN_AUTO, DLC_PCA_PLAN_ONE_PASS, DLC_PCA_PLAN_SPLIT = 0, 1, 2
DLC_LSH_MAX_BITS, DLC_LSH_MAX_D = 8192, 131071   # dlc_lsh_hash_i8: 128 * 128 * D < 2^31, the int32 sum cannot overflow
DLC_LSH_CHUNK, DLC_LSH_SPLIT_MAX_ROWS = 8192, 64  # bytes of D per split piece; the most rows the SPLIT plan takes
DLC_LSH_PLAN_AUTO, DLC_LSH_PLAN_ONE_PASS, DLC_LSH_PLAN_SPLIT = 0, 1, 2
DLC_VERIFY_MAX_PATCHES = 64 # the most patches of a frame dlc_verify_pairs matches (one bit of its inlier mask each)
DLC_VERIFY_SIMILARITY, DLC_VERIFY_TRANSLATION = 0, 1

_vp, _i64, _int, _sz, _dbl, _flt = C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_double, C.c_float

# name -> (restype, argtypes): every function include/dlc.h declares.
SIGNATURES = {
    "dlc_abi_version": (_int, []),
    "dlc_create": (_int, [_int, C.POINTER(_vp)]),
    "dlc_destroy": (_int, [_vp]),
    "dlc_last_error": (C.c_char_p, [_vp]),
    "dlc_status_string": (C.c_char_p, [_int]),
    "dlc_gemm_bias_act": (_int, [_vp, _int, _int, _int, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "dlc_bias_act": (_int, [_vp, _int, _int, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "dlc_sdav_encode_workspace_bytes": (_sz, [_i64, C.POINTER(_i64), _int, _int]),
    "dlc_sdav_encode": (_int, [_vp, _int, _i64, _int, C.POINTER(_i64), _vp, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp,
                               _sz, _vp]),
    "dlc_sdav_split_panels_bytes": (_sz, [_int, C.POINTER(_i64)]),
    "dlc_sdav_split_prepare": (_int, [_vp, _int, C.POINTER(_i64), C.POINTER(_vp), _vp, _sz, _vp]),
    "dlc_sdav_encode_split_workspace_bytes": (_sz, [_i64, C.POINTER(_i64), _int]),
    "dlc_cnnvtl_split_panels_bytes": (_sz, [_int, C.POINTER(C.c_int32)]),
    "dlc_cnnvtl_split_prepare": (_int, [_vp, _int, C.POINTER(C.c_int32), C.POINTER(_vp), _vp, _sz, _vp]),
    "dlc_cnnvtl_encode_split_workspace_bytes": (_sz, [_i64, _int, _int, _int, _int, C.POINTER(C.c_int32)]),
    "dlc_cnnvtl_encode_split": (_int, [_vp, _int, _vp, _i64, _int, _int, _int, _int, _int, C.POINTER(C.c_int32), _vp, C.POINTER(_vp),
                                       _vp, _i64, _vp, C.POINTER(_vp), _vp, _vp, _sz, _vp]),
    "dlc_cnnvtl_layers_split": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, C.POINTER(C.c_int32), _int, _int, _vp, C.POINTER(_vp),
                                       C.POINTER(_vp), _vp, _vp, _sz, _vp]),
    "dlc_sdav_encode_split": (_int, [_vp, _i64, _int, C.POINTER(_i64), _vp, _vp, C.POINTER(_vp), _vp, _vp, _sz, _vp]),
    "dlc_sdav_train_workspace_bytes": (_sz, [_i64, _i64, C.POINTER(_i64), _int, _int]),
    "dlc_sdav_train_step": (_int, [_vp, _int, _i64, _i64, _int, C.POINTER(_i64), _vp, C.POINTER(_vp), C.POINTER(_vp),
                                  C.POINTER(_vp), _vp, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _sz, _vp]),
    "dlc_random_mask_f64": (_int, [_vp, _vp, _i64, _i64, C.c_uint64, C.c_uint64, _vp]),
    "dlc_salt_pepper_mask_f64": (_int, [_vp, _vp, _vp, _i64, _i64, C.c_uint64, C.c_uint64, _vp]),
    "dlc_da_corrupt_f64": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp]),
    "dlc_da_train_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "dlc_da_train_step": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _sz,
                                _vp]),
    "dlc_rgb_to_gray_u8": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "dlc_harris_keypoints_workspace_bytes": (_sz, [_i64, _int, _int]),
    "dlc_harris_keypoints_u8": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dlc_extract_patches": (_int, [_vp, _vp, _i64, _int, _int, _vp, _int, _int, _int, _vp, _vp]),
    "dlc_im2col_nhwc_f64": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _int, _int, _int, _int, _vp, _vp]),
    "dlc_conv2d_nhwc_f64": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp, _int, _int, _int, _int, _int, _int, _int,
                                  _int, _int, _vp, _vp]),
    "dlc_space_to_depth_nhwc_f64": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    "dlc_maxpool3x3s2_nhwc_f64": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "dlc_minmax_quant_gather_i8": (_int, [_vp, C.POINTER(_vp), C.POINTER(_i64), _int, _i64, _vp, _i64, _vp, _vp, _vp]),
    "dlc_cnnvtl_frame_minmax_init": (_int, [_vp, _vp, _i64, _vp]),
    "dlc_conv2d_nhwc_f64_stats": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp, _int, _int, _int, _int, _int, _int, _int,
                                         _int, _int, _vp, _vp, _vp]),
    "dlc_quant_gather_i8": (_int, [_vp, C.POINTER(_vp), C.POINTER(_i64), _int, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "dlc_sdav_range_words": (_sz, [_i64]),
    "dlc_sdav_distinctive_score": (_int, [_vp, _vp, _i64, _i64, _dbl, _dbl, _vp, _vp, _vp]),
    "dlc_sdav_similarity_workspace_bytes": (_sz, [_i64, _i64, _i64, _int, _i64]),
    "dlc_sdav_similarity_matrix": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _dbl, _dbl, _vp, _vp, _int, _i64, _vp, _vp, _vp,
                                         _vp, _sz, _vp]),
    "dlc_topk_rows_f64": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "dlc_sdav_stream_state_bytes": (_sz, [_i64, _i64, _i64]),
    "dlc_sdav_stream_init": (_int, [_vp, _vp, _sz, _i64, _i64, _i64, _dbl, _dbl, _vp, _vp]),
    "dlc_sdav_stream_append": (_int, [_vp, _vp, _sz, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    "dlc_sdav_stream_query": (_int, [_vp, _vp, _sz, _i64, _i64, _i64, _vp, _i64, _vp, _dbl, _dbl, _vp, _vp, _vp]),
    "dlc_sdav_stream_query_batch_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dlc_sdav_stream_query_batch": (_int, [_vp, _vp, _sz, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _dbl, _dbl, _vp, _i64, _vp,
                                           _vp, _sz, _vp]),
    "dlc_sdav_stream_query_batch_staged": (_int, [_vp, _vp, _sz, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _dbl, _dbl, _vp, _i64,
                                                  _vp, _vp, _sz, _int, _vp]),
    "dlc_cnnvtl_distance_matrix": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "dlc_cnnvtl_distance_topk_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "dlc_cnnvtl_distance_topk": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _sz,
                                        _vp]),
    "dlc_cnnvtl_distance_rows": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _vp]),
    "dlc_sad_u8_rows": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _vp]),
    "dlc_sad_u8_shift_rows": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _int, _int, _int, _i64, _i64, _vp, _i64, _vp, _i64,
                                     _vp]),
    "dlc_seqslam_describe_u8": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _vp, _i64, _vp]),
    "dlc_ldb_row_bytes": (_i64, [C.POINTER(_int), _int]),
    "dlc_ldb_describe_u8": (_int, [_vp, _vp, _i64, _int, _int, _int, _int, C.POINTER(_int), _int, _vp, _i64, _vp]),
    "dlc_lsh_quantize_i8": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    "dlc_lsh_row_bytes": (_i64, [_int]),
    "dlc_lsh_hash_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "dlc_lsh_hash_i8": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _int, _i64, _vp, _i64, _int, _vp, _sz, _vp]),
    "dlc_hamming_rows": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _vp]),
    "dlc_sequence_topk_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int]),
    "dlc_sequence_topk": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, C.POINTER(C.c_int32), _int, _int,
                                 _vp, _vp, _vp, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dlc_sequence_elastic_topk_workspace_bytes": (_sz, [_i64, _i64, _int, _int, _int, _int]),
    "dlc_sequence_elastic_topk": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int,
                                         _vp, _vp, _vp, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dlc_sequence_elastic_chains": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int,
                                           _vp, _vp, _vp, _vp, _vp]),
    "dlc_sequence_chains": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, C.POINTER(C.c_int32), _int, _int,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlc_contrast_rows": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _i64, _vp]),
    "dlc_fuse_rows_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "dlc_fuse_rows": (_int, [_vp, _int, C.POINTER(_int), C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_dbl), C.POINTER(_int),
                             _i64, _i64, _i64, _i64, _int, _int, _vp, _i64, _vp, _sz, _vp]),
    "dlc_peak_topk_rows_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "dlc_peak_topk_rows": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _i64, _int, _i64, _int, _vp, _vp, _vp,
                                  _vp, _sz, _vp]),
    "dlc_track_rows_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "dlc_track_rows": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _dbl, _dbl, _dbl, _int, _vp, _vp,
                              _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _sz, _vp]),
    "dlc_track_backtrace": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
    "dlc_vlad_assign": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _int, _i64, _vp, _vp, _vp]),
    "dlc_vlad_encode_workspace_bytes": (_sz, [_i64, _int, _i64, _int]),
    "dlc_vlad_encode": (_int, [_vp, _vp, _i64, _int, _i64, _i64, _vp, _int, _i64, _int, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dlc_kmeans_step_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "dlc_kmeans_step": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _int, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dlc_pca_project_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "dlc_pca_project": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _int, _vp, _int, _i64, _vp, _vp, _i64, _int, _vp, _sz, _vp]),
    "dlc_verify_pairs_workspace_bytes": (_sz, [_i64, _int, _int]),
    "dlc_verify_pairs": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _vp, _i64, _int, _int, _int, _int, _int,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dlc_pr_cell_counts_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "dlc_pr_cell_counts": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _int, _i64, _vp, _i64, _vp, _int, _vp, _vp,
                                  _vp, _sz, _vp]),
    "dlc_positive_rank_rows_workspace_bytes": (_sz, [_i64, _i64]),
    "dlc_positive_rank_rows": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _int, _i64, _vp, _i64, _vp, _vp, _vp,
                                      _vp, _sz, _vp]),
    "dlc_l2_normalize_rows": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _int, _int, _vp, _i64, _vp]),
    "dlc_cosine_topk_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "dlc_cosine_topk": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                              _vp]),
    "dlc_max_row_norm": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _vp]),
    "dlc_cosine_tau_scale": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "dlc_cosine_topk_older": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _sz, _vp]),
    "dlc_cosine_score_error_bound": (_dbl, [_i64, _i64, _i64, _int]),
    "dlc_cosine_score_error_bound_any_plan": (_dbl, [_i64]),
    "dlc_cosine_score_groups": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp, _sz, _vp]),
    "dlc_cosine_select_topk": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _sz, _int, _vp]),
    "dlc_cosine_groups_per_query": (_int, [_int]),
    "dlc_cosine_select_groups": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp, _sz, _vp, _vp, _int,
                                       _vp]),
    "dlc_cosine_rescore_topk": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _i64, _vp, _vp, _vp, _int,
                                      _vp, _vp, _vp, _vp, _int, _vp]),
    "dlc_cosine_exhaustive_topk": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _i64, _vp, _i64, _dbl,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dlc_topk_merge_strided": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _i64, _int, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlc_topk_merge": (_int, [_vp, _vp, _vp, _int, _i64, _int, _vp, _vp, _vp, _vp]),
    "dlc_topk_keep_older": (_int, [_vp, _vp, _vp, _i64, _int, _i64, _int, _vp, _vp, _vp]),
    "dlc_cosine_scores_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dlc_cosine_scores": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _sz, _vp]),
    "dlc_cosine_score_rows": (_int, [_vp, _int, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    "dlc_host_to_device": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "dlc_device_to_host": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "dlc_set_host_threads": (_int, [_vp, _int]),
    "dlc_set_scratch": (_int, [_vp, _vp, _sz]),
    "dlc_set_profiling": (_int, [_vp, _int]),
    "dlc_set_prune_mode": (_int, [_vp, _int]),
    "dlc_cosine_topk_prune_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "dlc_profile_gemm_ms": (_int, [_vp, C.POINTER(_flt), _int]),
}

_lib = None


class DlcError(RuntimeError):
    """A HIP-side failure (DLC_ERR_HIP / DLC_ERR_WORKSPACE) reported by the C ABI."""


def load():
    """dlopen libdlc_hip.so and declare every prototype.  Raises ImportError
    (loudly) when the extension has not been built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "deeploopcloser_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C deeploopcloser_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.dlc_abi_version() != DLC_ABI_VERSION:
        raise ImportError("deeploopcloser_amd: %s has ABI %d, these bindings are for ABI %d -- rebuild it"
                          % (LIB_PATH, lib.dlc_abi_version(), DLC_ABI_VERSION))
    _lib = lib
    return lib


def raise_for_status(lib, ctx, rc):
    if rc == DLC_OK:
        return
    msg = lib.dlc_last_error(ctx).decode() if ctx else ""
    text = "%s: %s" % (lib.dlc_status_string(rc).decode(), msg)
    if rc in (DLC_ERR_BAD_ARG, DLC_ERR_BAD_SHAPE, DLC_ERR_UNSUPPORTED):
        raise ValueError(text)
    raise DlcError(text)
