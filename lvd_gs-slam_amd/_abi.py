"""The C ABI of ``include/lvdgs.h`` as data: every struct, every named constant and every prototype, written by hand and
compared with the header, whole, by ``tests/test_abi.py``.

Nothing here loads the library or imports torch (``_lib`` does both and re-exports these names).  The header's ``LVDGS_X`` is
``X`` here; a struct's ``_c_name_`` is its typedef in the header; ``PROTOTYPES`` holds the functions in the header's order.
"""
import ctypes as C

import numpy as np

OK, E_INVALID, E_HIP, E_RANGE, E_CAPACITY = 0, 1, 2, 3, 4
FLAG_LIST_ALL_TILES = 1
FLAG_ACCUMULATE_PARAM_GRADS = 2   # lvdgs_args.flags
FLAG_POSE_ONLY = 4
FLAG_NO_BLEND = 8   # the call leaves its blend pass to lvdgs_blend_*_batch
FLAG_SUPER_TILES = 16   # hint: group and depth-sort the pairs per 64 x 64-pixel super-tile (same outputs; rasterizer.super_tiles_flag)
F32, F16, BF16 = 0, 1, 2     # lvdgs_rope2d_strided's dtype

_fp = C.c_void_p


class Args(C.Structure):
    _c_name_ = "lvdgs_args"     # field order must match the header
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("sh_degree", C.c_int32), ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("bg", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("projmatrix_raw", _fp), ("campos", _fp),
        ("num_gaussians", C.c_int32), ("sh_coeffs", C.c_int32),
        ("means3D", _fp), ("opacities", _fp), ("scales", _fp), ("rotations", _fp), ("cov3D_precomp", _fp),
        ("shs", _fp), ("colors_precomp", _fp),
        ("geom_state", _fp), ("geom_bytes", C.c_size_t),
        ("binning_state", _fp), ("binning_bytes", C.c_size_t),
        ("image_state", _fp), ("image_bytes", C.c_size_t),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("num_rendered", C.c_int64),
        ("radii", _fp), ("out_color", _fp), ("out_depth", _fp), ("out_opacity", _fp), ("n_touched", _fp),
        ("dL_dout_color", _fp), ("dL_dout_depth", _fp), ("dL_dout_opacity", _fp),
        ("dL_dmeans3D", _fp), ("dL_dmeans2D", _fp), ("dL_dopacities", _fp), ("dL_dscales", _fp),
        ("dL_drotations", _fp), ("dL_dcov3D", _fp), ("dL_dshs", _fp), ("dL_dcolors", _fp), ("dL_dtau", _fp),
        ("pair_capacity", C.c_int64), ("activations", C.c_int32),
        ("flags", C.c_int32), ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32),
    ]


class LossArgs(C.Structure):
    _c_name_ = "lvdgs_loss_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("image", _fp), ("depth", _fp), ("opacity", _fp), ("gt_image", _fp), ("gt_depth", _fp), ("grad_mask", _fp),
        ("exposure_a", _fp), ("exposure_b", _fp),
        ("rgb_boundary_threshold", C.c_float), ("weight_rgb", C.c_float), ("weight_depth", C.c_float),
        ("weight_by_opacity", C.c_int32), ("depth_needs_opaque", C.c_int32),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("loss", _fp), ("grad_loss", _fp), ("d_image", _fp), ("d_depth", _fp), ("d_opacity", _fp),
        ("d_exposure_a", _fp), ("d_exposure_b", _fp),
    ]


class MaskedDepthArgs(C.Structure):
    _c_name_ = "lvdgs_masked_depth_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("depth", _fp), ("gt_depth", _fp), ("static_mask", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("out", _fp), ("grad_loss", _fp), ("d_depth", _fp),
    ]


class PoseStepArgs(C.Structure):
    _c_name_ = "lvdgs_pose_step_args"
    _fields_ = [
        ("R", _fp), ("T", _fp), ("cam_rot_delta", _fp), ("cam_trans_delta", _fp), ("exposure_a", _fp), ("exposure_b", _fp),
        ("grad_tau", _fp), ("grad_exposure_a", _fp), ("grad_exposure_b", _fp), ("state", _fp),
        ("lr_rot", C.c_double), ("lr_trans", C.c_double), ("lr_exposure", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_double), ("converged_threshold", C.c_float),
        ("projmatrix_raw", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("campos", _fp),
        ("grad_rot", _fp), ("grad_trans", _fp), ("host_flags", _fp),
    ]


class ViewStatsArgs(C.Structure):
    _c_name_ = "lvdgs_view_stats_args"
    _fields_ = [("radii_max", _fp), ("norm_sum", _fp), ("vis_count", _fp), ("touched_row", _fp), ("split_xy", _fp)]


ADAM_MAX_TENSORS = 8


class AdamTensor(C.Structure):
    _c_name_ = "lvdgs_adam_tensor"
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("numel", C.c_int64), ("step", C.c_int64),
                ("lr", C.c_double)]


class SsimArgs(C.Structure):
    _c_name_ = "lvdgs_ssim_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("planes", C.c_int32), ("channels", C.c_int32),
        ("img1", _fp), ("img2", _fp), ("keep_mask", _fp), ("bg", _fp),
        ("weight_l1", C.c_float), ("weight_ssim", C.c_float),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("out", _fp), ("d_img1", _fp),
    ]


class MaskedLossArgs(C.Structure):
    _c_name_ = "lvdgs_masked_loss_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("image", _fp), ("gt_image", _fp), ("static_mask", _fp), ("bg", _fp), ("depth", _fp), ("gt_depth", _fp),
        ("lambda_dssim", C.c_float), ("depth_lambda", C.c_float),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("d_image", _fp), ("out", _fp),
    ]


class DepthAlignArgs(C.Structure):
    _c_name_ = "lvdgs_depth_align_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("patch_size", C.c_int32), ("max_iter", C.c_int32),
        ("mean_threshold", C.c_double), ("std_threshold", C.c_double), ("error_threshold", C.c_double),
        ("final_error_threshold", C.c_double), ("epsilon", C.c_double), ("min_accurate_pixels_ratio", C.c_double),
        ("render_depth", _fp), ("mono_depth", _fp), ("final_depth", _fp), ("error_mask", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


DEPTH_ALIGN_MAX_PATCH, DEPTH_ALIGN_STATE_WORDS = 64, 8
DEPTH_ALIGN_RUNNING, DEPTH_ALIGN_CONVERGED, DEPTH_ALIGN_EXHAUSTED, DEPTH_ALIGN_REMEDY = 0, 1, 2, 3


class PnpArgs(C.Structure):
    _c_name_ = "lvdgs_pnp_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("num_matches", C.c_int32), ("hypotheses", C.c_int32), ("min_inliers", C.c_int32),
        ("seed", C.c_uint32),
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 5),
        ("reproj_error", C.c_double),
        ("depth", _fp), ("matches_im1", _fp), ("matches_im2", _fp), ("inlier_mask", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


PNP_MAX_HYPOTHESES, PNP_STATE_WORDS, PNP_HOST_BYTES = 4096, 8, 128
PNP_OK, PNP_FAILED = 1, 2
PNP_FAIL_NONE, PNP_FAIL_FEW_VALID, PNP_FAIL_ALL_VOID, PNP_FAIL_FEW_INLIERS, PNP_FAIL_SINGULAR = 0, 1, 2, 3, 4


class RecipNnArgs(C.Structure):
    _c_name_ = "lvdgs_recip_nn_args"
    _fields_ = [
        ("width1", C.c_int32), ("height1", C.c_int32), ("width2", C.c_int32), ("height2", C.c_int32),
        ("dim", C.c_int32), ("subsample", C.c_int32), ("max_iter", C.c_int32), ("capacity", C.c_int32),
        ("desc1", _fp), ("desc2", _fp), ("matches_im1", _fp), ("matches_im2", _fp), ("seed_state", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


RNN_MAX_DIM, RNN_MAX_SEEDS, RNN_STATE_WORDS = 64, 8192, 8
RNN_OK = 1


class FormatPlan(C.Structure):
    _c_name_ = "lvdgs_format_plan"
    _fields_ = [(n, C.c_int32) for n in ("resized_width", "resized_height", "filter", "crop_x", "crop_y", "out_width", "out_height",
                                         "taps_x", "taps_y", "row_first", "row_count")]


class FormatImageArgs(C.Structure):
    _c_name_ = "lvdgs_format_image_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("size", C.c_int32),
        ("image", _fp), ("table_x", _fp), ("table_y", _fp), ("out", _fp), ("quantised", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


FORMAT_MAX_EDGE, FORMAT_MAX_SIZE = 16384, 4096
FORMAT_BICUBIC, FORMAT_LANCZOS = 0, 1


class MatchScaleArgs(C.Structure):
    _c_name_ = "lvdgs_match_scale_args"
    _fields_ = [
        ("num_matches", C.c_int32), ("raster_width", C.c_int32), ("raster_height", C.c_int32),
        ("width1", C.c_int32), ("height1", C.c_int32), ("width2", C.c_int32), ("height2", C.c_int32),
        ("matches_im1", _fp), ("matches_im2", _fp), ("depth1", _fp), ("depth2", _fp), ("host_state", _fp),
    ]


MATCH_SCALE_STATE_WORDS, MATCH_SCALE_HOST_BYTES = 8, 64
MATCH_SCALE_OK, MATCH_SCALE_NO_VALID = 1, 2


class EdgeMaskArgs(C.Structure):
    _c_name_ = "lvdgs_edge_mask_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("mode", C.c_int32), ("edge_threshold", C.c_double),
        ("image", _fp), ("mask", _fp), ("loss_mask", _fp), ("magnitude", _fp), ("stats", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


EDGE_MASK_MEDIAN, EDGE_MASK_BLOCKS = 0, 1
FRAME_SUMMARY_MAX_ROWS, FRAME_SUMMARY_HOST_BYTES = 16, 256
FRAME_SUMMARY_SEQ, FRAME_SUMMARY_MEDIAN, FRAME_SUMMARY_SELECTED, FRAME_SUMMARY_VISIBLE, FRAME_SUMMARY_MASK_COUNT, FRAME_SUMMARY_ROWS = 0, 1, 2, 3, 4, 8


class FrameSummaryArgs(C.Structure):
    _c_name_ = "lvdgs_frame_summary_args"
    _fields_ = [
        ("num_pixels", C.c_int32), ("num_gaussians", C.c_int32), ("num_rows", C.c_int32), ("seq", C.c_uint32), ("opacity_bar", C.c_float),
        ("depth", _fp), ("opacity", _fp), ("mask", _fp), ("n_touched", _fp), ("rows", _fp * FRAME_SUMMARY_MAX_ROWS), ("count_mask", _fp),
        ("host_state", _fp), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class DynamicMaskArgs(C.Structure):
    _c_name_ = "lvdgs_dynamic_mask_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("first_frame", C.c_int32), ("box_format", C.c_int32), ("num_boxes", C.c_int32),
        ("boxes", _fp), ("vehicle", _fp), ("num_sam_masks", C.c_int32), ("sam_masks", _fp), ("history_length", C.c_int32),
        ("vehicle_kernel_first", C.c_int32), ("vehicle_kernel", C.c_int32), ("expand_kernel", C.c_int32),
        ("image", _fp), ("rgb_boundary_threshold", C.c_double), ("depth_in", _fp), ("depth_out", _fp),
        ("static_mask", _fp), ("dynamic_mask", _fp), ("expanded_dynamic", _fp), ("expanded_static", _fp), ("valid_rgb", _fp),
        ("info", _fp), ("state", _fp), ("state_bytes", C.c_size_t), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


DYNAMIC_MASK_BOXES_XYXY, DYNAMIC_MASK_BOXES_CXCYWH = 0, 1
DYNAMIC_MASK_INFO_WORDS = 16
(DYNAMIC_MASK_INFO_BOXES, DYNAMIC_MASK_INFO_VEHICLE, DYNAMIC_MASK_INFO_USE_SAM, DYNAMIC_MASK_INFO_FILTERED, DYNAMIC_MASK_INFO_HISTORY,
 DYNAMIC_MASK_INFO_BOX_PIXELS, DYNAMIC_MASK_INFO_SAM_PIXELS, DYNAMIC_MASK_INFO_DYNAMIC_PIXELS, DYNAMIC_MASK_INFO_STATIC_PIXELS,
 DYNAMIC_MASK_INFO_EXPANDED_PIXELS, DYNAMIC_MASK_INFO_VALID_PIXELS, DYNAMIC_MASK_INFO_DEPTH_PIXELS) = range(12)
DYNAMIC_MASK_INFO = ("boxes", "vehicle_detected", "use_sam_result", "filtered", "history", "box_pixels", "sam_pixels", "dynamic_pixels",
                     "static_pixels", "expanded_pixels", "valid_pixels", "depth_pixels")   # the words' names, in LVDGS_DYNAMIC_MASK_INFO_* order


class FarnebackParams(C.Structure):
    _c_name_ = "lvdgs_farneback_params"
    _fields_ = [("pyr_scale", C.c_double), ("levels", C.c_int32), ("winsize", C.c_int32), ("iterations", C.c_int32), ("poly_n", C.c_int32),
                ("poly_sigma", C.c_double)]


class FarnebackArgs(C.Structure):
    _c_name_ = "lvdgs_farneback_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("params", FarnebackParams),
        ("prev", _fp), ("next", _fp), ("flow", _fp), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class MotionMaskArgs(C.Structure):
    _c_name_ = "lvdgs_motion_mask_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("mode", C.c_int32), ("dilate_kernel", C.c_int32), ("params", FarnebackParams),
        ("motion_threshold", C.c_double), ("image", _fp), ("mask", _fp), ("flow", _fp), ("info", _fp),
        ("state", _fp), ("state_bytes", C.c_size_t), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


FARNEBACK_MAX_BLUR_TAPS = 127
MOTION_OBSERVE, MOTION_MASK, MOTION_ADVANCE = 1, 2, 4
MOTION_INFO_WORDS = 8
MOTION_INFO_HAS_PREV, MOTION_INFO_LEVELS, MOTION_INFO_MOVING_PIXELS, MOTION_INFO_MASK_PIXELS = range(4)
MOTION_INFO = ("has_prev", "levels", "moving_pixels", "mask_pixels")   # the words' names, in LVDGS_MOTION_INFO_* order


class SeedArgs(C.Structure):
    _c_name_ = "lvdgs_seed_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("depth_trunc", C.c_float),
        ("want_median", C.c_int32), ("inv_downsample", C.c_double), ("seed", C.c_uint64), ("seq", C.c_uint32), ("capacity", C.c_int32),
        ("image", _fp), ("gain", _fp), ("offset", _fp), ("depth", _fp), ("R", _fp), ("T", _fp),
        ("xyz", _fp), ("rgb", _fp), ("f_dc", _fp), ("pixel", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


SEED_HOST_BYTES = 64
SEED_SEQ, SEED_N_VALID, SEED_N_KEEP, SEED_MEDIAN, SEED_THRESHOLD = 0, 1, 2, 3, 4


EDIT_MAX_COLUMNS, EDIT_MAX_VIS_ROWS = 48, 16
EDIT_PRUNE, EDIT_DENSIFY = 0, 1
EDIT_KEEP, EDIT_CLONE, EDIT_SPLIT0, EDIT_SPLIT1 = 0, 1, 2, 3
EDIT_COPY, EDIT_ZERO, EDIT_XYZ, EDIT_SCALE = 0, 1, 2, 3
EDIT_SEQ, EDIT_N_OUT, EDIT_N_KEEP, EDIT_N_CLONE, EDIT_N_SPLIT_SEL, EDIT_N_PRUNED_FINAL, EDIT_HOST_SRC = 0, 1, 2, 3, 4, 5, 16


class MapEditPlanArgs(C.Structure):
    _c_name_ = "lvdgs_map_edit_plan_args"
    _fields_ = [
        ("mode", C.c_int32), ("num_gaussians", C.c_int32), ("seq", C.c_uint32), ("scale_dims", C.c_int32),
        ("remove", _fp), ("num_vis_rows", C.c_int32), ("prune_num", C.c_int32), ("min_kf_id", C.c_int32), ("capacity", C.c_int32),
        ("vis_rows", _fp * EDIT_MAX_VIS_ROWS), ("kf_id", _fp), ("n_obs", _fp),
        ("grad_accum", _fp), ("denom", _fp), ("scaling", _fp), ("opacity", _fp), ("max_radii2D", _fp),
        ("grad_threshold", C.c_float), ("dense_extent", C.c_float), ("min_opacity", C.c_float), ("max_screen_size", C.c_float),
        ("world_extent", C.c_float), ("vis_stride", C.c_int32),
        ("src", _fp), ("kind", _fp), ("noise_row", _fp), ("host_state", _fp), ("host_bytes", C.c_size_t),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class MapEditColumn(C.Structure):
    _c_name_ = "lvdgs_map_edit_column"
    _c_field_names_ = {"in_": "in"}     # Python field -> C field, where a keyword forbids the C name
    _fields_ = [("in_", _fp), ("out", _fp), ("row_bytes", C.c_int32), ("new_rows", C.c_int32)]


class MapEditApplyArgs(C.Structure):
    _c_name_ = "lvdgs_map_edit_apply_args"
    _fields_ = [
        ("num_gaussians", C.c_int32), ("n_out", C.c_int32), ("n_split_sel", C.c_int32), ("scale_dims", C.c_int32),
        ("num_columns", C.c_int32), ("reserved", C.c_int32),
        ("src", _fp), ("kind", _fp), ("noise_row", _fp), ("noise", _fp), ("scaling", _fp), ("rotation", _fp),
        ("columns", MapEditColumn * EDIT_MAX_COLUMNS),
    ]


class IngestArgs(C.Structure):
    _c_name_ = "lvdgs_ingest_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("src", _fp), ("src_row_bytes", C.c_int64),
        ("map_sx", _fp), ("map_sy", _fp), ("image", _fp), ("image_u8", _fp),
    ]


class IngestDepthArgs(C.Structure):
    _c_name_ = "lvdgs_ingest_depth_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("src", _fp), ("sample_type", C.c_int32), ("pixel_stride", C.c_int32),
        ("src_row_bytes", C.c_int64), ("divisor", C.c_double), ("out", _fp),
    ]


class FrameEvalArgs(C.Structure):
    _c_name_ = "lvdgs_frame_eval_args"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("render", _fp), ("gt_image", _fp), ("static_mask", _fp), ("bg", _fp), ("depth", _fp), ("out_row", _fp),
        ("pred8", _fp), ("gt8", _fp), ("residual8", _fp), ("depth8", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class FrameEvalRow(C.Structure):
    _c_name_ = "lvdgs_frame_eval_row"     # what one call leaves at ``out_row``
    _fields_ = [
        ("sum_sq_full", C.c_double), ("sum_sq_static", C.c_double), ("n_basic", C.c_uint64), ("n_keep", C.c_uint64),
        ("ssim_full", C.c_double), ("ssim_static", C.c_double), ("depth_min", C.c_float), ("depth_max", C.c_float),
        ("flags", C.c_uint32), ("reserved", C.c_uint32),
    ]


FRAME_EVAL_ROW_BYTES = 64
FRAME_EVAL_HAS_MASK, FRAME_EVAL_HAS_DEPTH, FRAME_EVAL_DEPTH_CONSTANT = 1, 2, 4
# the row as a NumPy record (same offsets as FrameEvalRow)
FRAME_EVAL_ROW_DTYPE = np.dtype([("sum_sq_full", "<f8"), ("sum_sq_static", "<f8"), ("n_basic", "<u8"), ("n_keep", "<u8"),
                                 ("ssim_full", "<f8"), ("ssim_static", "<f8"), ("depth_min", "<f4"), ("depth_max", "<f4"),
                                 ("flags", "<u4"), ("reserved", "<u4")])


class TsdfVolumeArgs(C.Structure):
    _c_name_ = "lvdgs_tsdf_volume"
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3),
        ("voxel_size", C.c_float), ("trunc", C.c_float), ("max_weight", C.c_float),
        ("tsdf", _fp), ("weight", _fp), ("r", _fp), ("g", _fp), ("b", _fp),
    ]


class TsdfViewArgs(C.Structure):
    _c_name_ = "lvdgs_tsdf_view"
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("depth_min", C.c_float), ("depth_trunc", C.c_float),
        ("R", _fp), ("T", _fp), ("depth", _fp), ("image", _fp), ("mask", _fp),
    ]


class TsdfMeshArgs(C.Structure):
    _c_name_ = "lvdgs_tsdf_mesh_args"
    _fields_ = [
        ("vol", TsdfVolumeArgs), ("seq", C.c_uint32), ("vertex_capacity", C.c_int32), ("face_capacity", C.c_int32),
        ("vertices", _fp), ("colors", _fp), ("faces", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


TSDF_MAX_VIEWS, TSDF_HOST_BYTES = 16, 64
TSDF_SEQ, TSDF_N_VERTICES, TSDF_N_FACES, TSDF_OVERFLOW = 0, 1, 2, 3
TSDF_OVERFLOW_VERTICES, TSDF_OVERFLOW_FACES, TSDF_OVERFLOW_INT32 = 1, 2, 4     # bits of the [TSDF_OVERFLOW] word


class TsdfBlocksArgs(C.Structure):
    _c_name_ = "lvdgs_tsdf_blocks"
    _fields_ = [
        ("pool_blocks", C.c_int32), ("table_slots", C.c_int32), ("origin", C.c_float * 3),
        ("voxel_size", C.c_float), ("trunc", C.c_float), ("max_weight", C.c_float),
        ("tsdf", _fp), ("weight", _fp), ("r", _fp), ("g", _fp), ("b", _fp),
        ("block_key", _fp), ("table_keys", _fp), ("table_values", _fp), ("header", _fp),
    ]


class TsdfBlocksMeshArgs(C.Structure):
    _c_name_ = "lvdgs_tsdf_blocks_mesh_args"
    _fields_ = [
        ("vol", TsdfBlocksArgs), ("seq", C.c_uint32), ("vertex_capacity", C.c_int32), ("face_capacity", C.c_int32),
        ("cell_lo", C.c_int32 * 3), ("cell_hi", C.c_int32 * 3), ("order", _fp), ("vertices", _fp), ("colors", _fp), ("faces", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


TSDF_BLOCKS_HEADER_WORDS, TSDF_BLOCKS_HOST_BYTES, TSDF_BLOCKS_MAX_POOL, TSDF_BLOCKS_MAX_STEPS = 8, 64, 4194304, 1025
TSDF_BLOCKS_HEADER_USED, TSDF_BLOCKS_HEADER_DROPPED, TSDF_BLOCKS_HEADER_OUT_OF_RANGE, TSDF_BLOCKS_HEADER_FLAGS = 0, 1, 2, 3
TSDF_BLOCKS_TABLE_FULL = 1
(TSDF_BLOCKS_SEQ, TSDF_BLOCKS_N_VERTICES, TSDF_BLOCKS_N_FACES, TSDF_BLOCKS_OVERFLOW, TSDF_BLOCKS_USED, TSDF_BLOCKS_DROPPED,
 TSDF_BLOCKS_OUT_OF_RANGE, TSDF_BLOCKS_FLAGS) = range(8)


class MeshSampleInfo(C.Structure):
    _c_name_ = "lvdgs_mesh_sample_info"     # what one lvdgs_mesh_sample leaves at ``info``
    _fields_ = [("flags", C.c_uint32), ("n_weighted", C.c_uint32), ("total", C.c_uint64)]


class MeshSampleArgs(C.Structure):
    _c_name_ = "lvdgs_mesh_sample_args"
    _fields_ = [
        ("num_vertices", C.c_int64), ("num_faces", C.c_int64), ("num_samples", C.c_int64), ("seed", C.c_uint64),
        ("vertices", _fp), ("faces", _fp), ("vertex_colors", _fp), ("points", _fp), ("face_index", _fp), ("colors", _fp), ("info", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


MESH_SAMPLE_INFO_BYTES, MESH_SAMPLE_NO_AREA = 16, 1
CLOUD_DISTANCE_ROW_BYTES, CLOUD_DISTANCE_MAX_THRESHOLDS, CLOUD_DISTANCE_POINTS_PER_CELL, CLOUD_DISTANCE_MAX_DIM = 64, 4, 8, 1024
CLOUD_DISTANCE_NO_REFERENCE = 1
MESH_SAMPLE_INFO_DTYPE = np.dtype([("flags", "<u4"), ("n_weighted", "<u4"), ("total", "<u8")])


class CloudDistanceRow(C.Structure):
    _c_name_ = "lvdgs_cloud_distance_row"     # what one lvdgs_cloud_distance leaves at ``out_row``
    _fields_ = [
        ("sum_distance", C.c_double), ("sum_squared", C.c_double), ("n_counted", C.c_uint32), ("n_skipped", C.c_uint32),
        ("n_below", C.c_uint32 * CLOUD_DISTANCE_MAX_THRESHOLDS), ("max_distance", C.c_float), ("flags", C.c_uint32),
        ("n_reference", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


# the row as a NumPy record (same offsets as CloudDistanceRow)
CLOUD_DISTANCE_ROW_DTYPE = np.dtype([("sum_distance", "<f8"), ("sum_squared", "<f8"), ("n_counted", "<u4"), ("n_skipped", "<u4"),
                                     ("n_below", "<u4", (CLOUD_DISTANCE_MAX_THRESHOLDS,)), ("max_distance", "<f4"), ("flags", "<u4"),
                                     ("n_reference", "<u4"), ("reserved", "<u4", (3,))])


class CloudDistanceArgs(C.Structure):
    _c_name_ = "lvdgs_cloud_distance_args"
    _fields_ = [
        ("num_queries", C.c_int64), ("num_reference", C.c_int64), ("queries", _fp), ("reference", _fp),
        ("num_thresholds", C.c_int32), ("points_per_cell", C.c_int32), ("thresholds", C.c_float * CLOUD_DISTANCE_MAX_THRESHOLDS),
        ("d2", _fp), ("idx", _fp), ("out_row", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class MeshVisibilityArgs(C.Structure):
    _c_name_ = "lvdgs_mesh_visibility_args"
    _fields_ = [
        ("num_vertices", C.c_int64), ("vertices", _fp), ("views", _fp), ("count", C.c_int32), ("occlusion_eps", C.c_float), ("seen", _fp),
    ]


class MeshCullArgs(C.Structure):
    _c_name_ = "lvdgs_mesh_cull_args"
    _fields_ = [
        ("num_vertices", C.c_int64), ("num_faces", C.c_int64), ("vertices", _fp), ("vertex_colors", _fp), ("faces", _fp), ("seen", _fp),
        ("face_rule", C.c_int32), ("seq", C.c_uint32),
        ("out_vertices", _fp), ("out_colors", _fp), ("out_faces", _fp), ("vertex_origin", _fp), ("face_origin", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


MESH_CULL_HOST_BYTES = 64
MESH_CULL_SEQ, MESH_CULL_N_VERTICES, MESH_CULL_N_FACES = 0, 1, 2
MESH_CULL_ALL, MESH_CULL_ANY = 0, 1     # lvdgs_mesh_cull_args.face_rule


class MeshDepthArgs(C.Structure):
    _c_name_ = "lvdgs_mesh_depth_args"
    _fields_ = [
        ("num_vertices", C.c_int64), ("num_faces", C.c_int64), ("vertices", _fp), ("faces", _fp), ("views", _fp), ("count", C.c_int32),
        ("depth", _fp), ("face_index", _fp), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


DEPTH_SAMPLE_BYTE, DEPTH_SAMPLE_WORD = 1, 2     # lvdgs_ingest_depth_args.sample_type
MAP_OUTSIDE = -2 ** 31     # INT32_MIN in an undistortion map: the destination pixel's source lies outside


class StateLayout(C.Structure):
    _c_name_ = "lvdgs_state_layout"
    _fields_ = [(n, C.c_size_t) for n in (
        "geom_rec", "geom_tiles_touched", "geom_slot_base", "bin_point_list", "bin_tile_keys",
        "img_ranges", "img_final_T", "img_n_contrib", "geom_rec_floats")]


class KernelTime(C.Structure):
    _c_name_ = "lvdgs_kernel_time"
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


_i32, _i64, _f, _d, _size, _status, _stream = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_int, C.c_void_p
_P = C.POINTER

# every function include/lvdgs.h declares, in its order: name -> (restype, [argtypes]); None: void
PROTOTYPES = {
    "lvdgs_geom_bytes": (_size, [_i32]),
    "lvdgs_prepare_scratch_bytes": (_size, [_i32]),
    "lvdgs_binning_bytes": (_size, [_i64]),
    "lvdgs_image_bytes": (_size, [_i32, _i32]),
    "lvdgs_render_scratch_bytes": (_size, [_i32, _i64, _i32, _i32]),
    "lvdgs_backward_scratch_bytes": (_size, [_i32, _i64]),
    "lvdgs_forward_prepare": (_status, [_P(Args), _P(_i64), _stream]),
    "lvdgs_forward_render": (_status, [_P(Args), _stream]),
    "lvdgs_forward": (_status, [_P(Args), _P(_i64), _stream]),
    "lvdgs_backward": (_status, [_P(Args), _stream]),
    "lvdgs_mark_visible": (_status, [_i32, _fp, _fp, _fp, _fp, _stream]),
    "lvdgs_state_layout_query": (_status, [_i32, _i64, _i32, _i32, _P(StateLayout)]),
    "lvdgs_knn_scratch_bytes": (_size, [_i32]),
    "lvdgs_dist2_knn3": (_status, [_i32, _fp, _fp, _fp, _size, _stream]),
    "lvdgs_rope2d": (_status, [_fp, _fp, _i32, _i32, _i32, _i32, _f, _f, _stream]),
    "lvdgs_rope2d_strided": (_status, [_fp, _i32, _fp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _f, _f, _stream]),
    "lvdgs_ms_deform_attn_forward": (_status, [_fp] * 5 + [_i32] * 7 + [_fp, _stream]),
    "lvdgs_ms_deform_attn_backward": (_status, [_fp] * 5 + [_i32] * 7 + [_fp] * 4 + [_stream]),
    "lvdgs_loss_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_photometric_loss_forward": (_status, [_P(LossArgs), _stream]),
    "lvdgs_photometric_loss_backward": (_status, [_P(LossArgs), _stream]),
    "lvdgs_photometric_loss_value_and_grad": (_status, [_P(LossArgs), _stream]),
    "lvdgs_photometric_loss_partials": (_status, [_P(LossArgs), _stream]),
    "lvdgs_pose_step": (_status, [_P(PoseStepArgs), _stream]),
    "lvdgs_host_device_pointer": (_status, [_fp, _P(_fp)]),
    "lvdgs_pose_step_batch": (_status, [_P(PoseStepArgs), _i32, _stream]),
    "lvdgs_backward_fused_loss": (_status, [_P(Args), _P(LossArgs), _i32, _stream]),
    "lvdgs_forward_backward_fused_loss": (_status, [_P(Args), _P(LossArgs), _i32, _P(_i64), _stream]),
    "lvdgs_blend_forward_batch": (_status, [_P(_P(Args)), _i32, _stream]),
    "lvdgs_forward_batch": (_status, [_P(_P(Args)), _i32, _P(_i64), _stream]),
    "lvdgs_blend_backward_fused_loss_batch": (_status, [_P(_P(Args)), _P(_P(LossArgs)), _i32, _i32, _stream]),
    "lvdgs_tracking_tail": (_status, [_P(LossArgs), _P(Args), _P(PoseStepArgs), _fp, _i32, _stream]),
    "lvdgs_map_view_tail": (_status, [_P(LossArgs), _P(Args), _fp, _P(ViewStatsArgs), _stream]),
    "lvdgs_map_view_tail_batch": (_status, [_P(_P(LossArgs)), _P(_P(Args)), _P(_fp), _P(_P(ViewStatsArgs)), _i32, _stream]),
    "lvdgs_adam_step": (_status, [_P(AdamTensor), _i32, _d, _d, _d, _stream]),
    "lvdgs_isotropic_scratch_bytes": (_size, [_i32]),
    "lvdgs_isotropic_reg": (_status, [_i32, _fp, _fp, _f, _fp, _size, _fp, _stream]),
    "lvdgs_view_stats": (_status, [_i32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _stream]),
    "lvdgs_map_stats_apply": (_status, [_i32, _fp, _fp, _fp, _fp, _i32, _fp, _fp, _fp, _stream]),
    "lvdgs_masked_depth_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_masked_depth_l1_forward": (_status, [_P(MaskedDepthArgs), _stream]),
    "lvdgs_masked_depth_l1_backward": (_status, [_P(MaskedDepthArgs), _stream]),
    "lvdgs_ssim_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "lvdgs_ssim_l1": (_status, [_P(SsimArgs), _stream]),
    "lvdgs_masked_loss_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_masked_loss_batch": (_status, [_P(_P(MaskedLossArgs)), _i32, _stream]),
    "lvdgs_backward_masked_loss": (_status, [_P(Args), _P(MaskedLossArgs), _stream]),
    "lvdgs_blend_backward_window_batch": (_status, [_P(_P(Args)), _P(_P(LossArgs)), _P(_P(MaskedLossArgs)), _i32, _i32, _stream]),
    "lvdgs_gaussian_backward_batch": (_status, [_P(_P(Args)), _i32, _stream]),
    "lvdgs_depth_align_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "lvdgs_depth_align": (_status, [_P(DepthAlignArgs), _stream]),
    "lvdgs_depth_align_resume": (_status, [_P(DepthAlignArgs), _f, _stream]),
    "lvdgs_pnp_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_pnp_ransac": (_status, [_P(PnpArgs), _stream]),
    "lvdgs_recip_nn_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "lvdgs_reciprocal_nn": (_status, [_P(RecipNnArgs), _stream]),
    "lvdgs_format_plan_query": (_status, [_i32, _i32, _i32, _P(FormatPlan)]),
    "lvdgs_format_table": (_status, [_i32, _i32, _i32, _i32, _i32, _fp]),
    "lvdgs_format_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "lvdgs_format_image": (_status, [_P(FormatImageArgs), _stream]),
    "lvdgs_match_depth_scale": (_status, [_P(MatchScaleArgs), _stream]),
    "lvdgs_edge_mask_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_edge_mask": (_status, [_P(EdgeMaskArgs), _stream]),
    "lvdgs_frame_summary_scratch_bytes": (_size, []),
    "lvdgs_frame_summary": (_status, [_P(FrameSummaryArgs), _stream]),
    "lvdgs_dynamic_mask_state_bytes": (_size, [_i32, _i32, _i32]),
    "lvdgs_dynamic_mask_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_dynamic_mask": (_status, [_P(DynamicMaskArgs), _stream]),
    "lvdgs_farneback_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_farneback_flow": (_status, [_P(FarnebackArgs), _stream]),
    "lvdgs_motion_mask_state_bytes": (_size, [_i32, _i32]),
    "lvdgs_motion_mask_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_motion_mask": (_status, [_P(MotionMaskArgs), _stream]),
    "lvdgs_seed_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_seed_points": (_status, [_P(SeedArgs), _stream]),
    "lvdgs_map_edit_scratch_bytes": (_size, [_i32]),
    "lvdgs_map_edit_plan": (_status, [_P(MapEditPlanArgs), _stream]),
    "lvdgs_map_edit_apply": (_status, [_P(MapEditApplyArgs), _stream]),
    "lvdgs_undistort_map": (_status, [_i32, _i32, _d, _d, _d, _d, _P(_d), _fp, _fp, _stream]),
    "lvdgs_ingest_frame": (_status, [_P(IngestArgs), _stream]),
    "lvdgs_ingest_depth": (_status, [_P(IngestDepthArgs), _stream]),
    "lvdgs_frame_eval_scratch_bytes": (_size, [_i32, _i32]),
    "lvdgs_frame_eval": (_status, [_P(FrameEvalArgs), _stream]),
    "lvdgs_tsdf_integrate": (_status, [_P(TsdfVolumeArgs), _P(_P(TsdfViewArgs)), _i32, _stream]),
    "lvdgs_tsdf_mesh_scratch_bytes": (_size, [_i32, _i32, _i32]),
    "lvdgs_tsdf_mesh": (_status, [_P(TsdfMeshArgs), _stream]),
    "lvdgs_tsdf_blocks_integrate": (_status, [_P(TsdfBlocksArgs), _P(_P(TsdfViewArgs)), _i32, _stream]),
    "lvdgs_tsdf_blocks_mesh_scratch_bytes": (_size, [_i32]),
    "lvdgs_tsdf_blocks_mesh": (_status, [_P(TsdfBlocksMeshArgs), _stream]),
    "lvdgs_tsdf_blocks_rehash": (_status, [_P(TsdfBlocksArgs), _stream]),
    "lvdgs_mesh_sample_scratch_bytes": (_size, [_i64]),
    "lvdgs_mesh_sample": (_status, [_P(MeshSampleArgs), _stream]),
    "lvdgs_cloud_distance_scratch_bytes": (_size, [_i64, _i64]),
    "lvdgs_cloud_distance": (_status, [_P(CloudDistanceArgs), _stream]),
    "lvdgs_mesh_visibility": (_status, [_P(MeshVisibilityArgs), _stream]),
    "lvdgs_mesh_cull_scratch_bytes": (_size, [_i64, _i64]),
    "lvdgs_mesh_cull": (_status, [_P(MeshCullArgs), _stream]),
    "lvdgs_mesh_depth_scratch_bytes": (_size, [_i64]),
    "lvdgs_mesh_depth": (_status, [_P(MeshDepthArgs), _stream]),
    "lvdgs_last_error": (C.c_char_p, []),
    "lvdgs_version": (C.c_char_p, []),
    "lvdgs_profile_enable": (None, [C.c_int]),
    "lvdgs_profile_reset": (None, []),
    "lvdgs_profile_read": (_status, [_P(KernelTime), C.c_int]),
}
