"""ctypes binding of ``lib/liblvdgs.so`` (C ABI: ``include/lvdgs.h``).

The library is the only compute path: if it is missing or fails to load, importing a symbol
from here raises -- there is no CPU or PyTorch fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LVDGS_LIB: another build of the library (same-box A/B of compile-time variants: `make OUT=../lib_b EXTRA=-D...`)
LIB_PATH = os.environ.get("LVDGS_LIB") or os.path.join(_HERE, "lib", "liblvdgs.so")

OK, E_INVALID, E_HIP, E_RANGE, E_CAPACITY = 0, 1, 2, 3, 4
FLAG_LIST_ALL_TILES = 1
FLAG_ACCUMULATE_PARAM_GRADS = 2   # lvdgs_args.flags
FLAG_POSE_ONLY = 4
FLAG_NO_BLEND = 8   # the call leaves its blend pass to lvdgs_blend_*_batch
FLAG_SUPER_TILES = 16   # hint: group and depth-sort the pairs per 64 x 64-pixel super-tile (same outputs; rasterizer.super_tiles_flag)

_fp = C.c_void_p


class Args(C.Structure):
    """struct lvdgs_args (include/lvdgs.h) -- field order must match the header."""
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
    """struct lvdgs_loss_args (include/lvdgs.h)."""
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
    """struct lvdgs_masked_depth_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("depth", _fp), ("gt_depth", _fp), ("static_mask", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("out", _fp), ("grad_loss", _fp), ("d_depth", _fp),
    ]


class PoseStepArgs(C.Structure):
    """struct lvdgs_pose_step_args (include/lvdgs.h)."""
    _fields_ = [
        ("R", _fp), ("T", _fp), ("cam_rot_delta", _fp), ("cam_trans_delta", _fp), ("exposure_a", _fp), ("exposure_b", _fp),
        ("grad_tau", _fp), ("grad_exposure_a", _fp), ("grad_exposure_b", _fp), ("state", _fp),
        ("lr_rot", C.c_double), ("lr_trans", C.c_double), ("lr_exposure", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_double), ("converged_threshold", C.c_float),
        ("projmatrix_raw", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("campos", _fp),
        ("grad_rot", _fp), ("grad_trans", _fp), ("host_flags", _fp),
    ]


class ViewStatsArgs(C.Structure):
    """struct lvdgs_view_stats_args (include/lvdgs.h)."""
    _fields_ = [("radii_max", _fp), ("norm_sum", _fp), ("vis_count", _fp), ("touched_row", _fp), ("split_xy", _fp)]


class AdamTensor(C.Structure):
    """struct lvdgs_adam_tensor (include/lvdgs.h)."""
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("numel", C.c_int64), ("step", C.c_int64),
                ("lr", C.c_double)]


class SsimArgs(C.Structure):
    """struct lvdgs_ssim_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("planes", C.c_int32), ("channels", C.c_int32),
        ("img1", _fp), ("img2", _fp), ("keep_mask", _fp), ("bg", _fp),
        ("weight_l1", C.c_float), ("weight_ssim", C.c_float),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("out", _fp), ("d_img1", _fp),
    ]


class MaskedLossArgs(C.Structure):
    """struct lvdgs_masked_loss_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("image", _fp), ("gt_image", _fp), ("static_mask", _fp), ("bg", _fp), ("depth", _fp), ("gt_depth", _fp),
        ("lambda_dssim", C.c_float), ("depth_lambda", C.c_float),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
        ("d_image", _fp), ("out", _fp),
    ]


class DepthAlignArgs(C.Structure):
    """struct lvdgs_depth_align_args (include/lvdgs.h)."""
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
    """struct lvdgs_pnp_args (include/lvdgs.h)."""
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
    """struct lvdgs_recip_nn_args (include/lvdgs.h)."""
    _fields_ = [
        ("width1", C.c_int32), ("height1", C.c_int32), ("width2", C.c_int32), ("height2", C.c_int32),
        ("dim", C.c_int32), ("subsample", C.c_int32), ("max_iter", C.c_int32), ("capacity", C.c_int32),
        ("desc1", _fp), ("desc2", _fp), ("matches_im1", _fp), ("matches_im2", _fp), ("seed_state", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


RNN_MAX_DIM, RNN_MAX_SEEDS, RNN_STATE_WORDS = 64, 8192, 8
RNN_OK = 1


class FormatPlan(C.Structure):
    """struct lvdgs_format_plan (include/lvdgs.h)."""
    _fields_ = [(n, C.c_int32) for n in ("resized_width", "resized_height", "filter", "crop_x", "crop_y", "out_width", "out_height",
                                         "taps_x", "taps_y", "row_first", "row_count")]


class FormatImageArgs(C.Structure):
    """struct lvdgs_format_image_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("size", C.c_int32),
        ("image", _fp), ("table_x", _fp), ("table_y", _fp), ("out", _fp), ("quantised", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


FORMAT_MAX_EDGE, FORMAT_MAX_SIZE = 16384, 4096
FORMAT_BICUBIC, FORMAT_LANCZOS = 0, 1


class MatchScaleArgs(C.Structure):
    """struct lvdgs_match_scale_args (include/lvdgs.h)."""
    _fields_ = [
        ("num_matches", C.c_int32), ("raster_width", C.c_int32), ("raster_height", C.c_int32),
        ("width1", C.c_int32), ("height1", C.c_int32), ("width2", C.c_int32), ("height2", C.c_int32),
        ("matches_im1", _fp), ("matches_im2", _fp), ("depth1", _fp), ("depth2", _fp), ("host_state", _fp),
    ]


MATCH_SCALE_STATE_WORDS, MATCH_SCALE_HOST_BYTES = 8, 64
MATCH_SCALE_OK, MATCH_SCALE_NO_VALID = 1, 2


class EdgeMaskArgs(C.Structure):
    """struct lvdgs_edge_mask_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("mode", C.c_int32), ("edge_threshold", C.c_double),
        ("image", _fp), ("mask", _fp), ("loss_mask", _fp), ("magnitude", _fp), ("stats", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


EDGE_MASK_MEDIAN, EDGE_MASK_BLOCKS = 0, 1
FRAME_SUMMARY_MAX_ROWS, FRAME_SUMMARY_HOST_BYTES = 16, 256
FRAME_SUMMARY_SEQ, FRAME_SUMMARY_MEDIAN, FRAME_SUMMARY_SELECTED, FRAME_SUMMARY_VISIBLE, FRAME_SUMMARY_MASK_COUNT, FRAME_SUMMARY_ROWS = 0, 1, 2, 3, 4, 8


class FrameSummaryArgs(C.Structure):
    """struct lvdgs_frame_summary_args (include/lvdgs.h)."""
    _fields_ = [
        ("num_pixels", C.c_int32), ("num_gaussians", C.c_int32), ("num_rows", C.c_int32), ("seq", C.c_uint32), ("opacity_bar", C.c_float),
        ("depth", _fp), ("opacity", _fp), ("mask", _fp), ("n_touched", _fp), ("rows", _fp * FRAME_SUMMARY_MAX_ROWS), ("count_mask", _fp),
        ("host_state", _fp), ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class DynamicMaskArgs(C.Structure):
    """struct lvdgs_dynamic_mask_args (include/lvdgs.h)."""
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
DYNAMIC_MASK_INFO = ("boxes", "vehicle_detected", "use_sam_result", "filtered", "history", "box_pixels", "sam_pixels", "dynamic_pixels",
                     "static_pixels", "expanded_pixels", "valid_pixels", "depth_pixels")   # the words' names, in LVDGS_DYNAMIC_MASK_INFO_* order


class SeedArgs(C.Structure):
    """struct lvdgs_seed_args (include/lvdgs.h)."""
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
    """struct lvdgs_map_edit_plan_args (include/lvdgs.h)."""
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
    """struct lvdgs_map_edit_column (include/lvdgs.h)."""
    _fields_ = [("in_", _fp), ("out", _fp), ("row_bytes", C.c_int32), ("new_rows", C.c_int32)]


class MapEditApplyArgs(C.Structure):
    """struct lvdgs_map_edit_apply_args (include/lvdgs.h)."""
    _fields_ = [
        ("num_gaussians", C.c_int32), ("n_out", C.c_int32), ("n_split_sel", C.c_int32), ("scale_dims", C.c_int32),
        ("num_columns", C.c_int32), ("reserved", C.c_int32),
        ("src", _fp), ("kind", _fp), ("noise_row", _fp), ("noise", _fp), ("scaling", _fp), ("rotation", _fp),
        ("columns", MapEditColumn * EDIT_MAX_COLUMNS),
    ]


class IngestArgs(C.Structure):
    """struct lvdgs_ingest_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("src", _fp), ("src_row_bytes", C.c_int64),
        ("map_sx", _fp), ("map_sy", _fp), ("image", _fp), ("image_u8", _fp),
    ]


class IngestDepthArgs(C.Structure):
    """struct lvdgs_ingest_depth_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("src", _fp), ("sample_type", C.c_int32), ("pixel_stride", C.c_int32),
        ("src_row_bytes", C.c_int64), ("divisor", C.c_double), ("out", _fp),
    ]


class FrameEvalArgs(C.Structure):
    """struct lvdgs_frame_eval_args (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("render", _fp), ("gt_image", _fp), ("static_mask", _fp), ("bg", _fp), ("depth", _fp), ("out_row", _fp),
        ("pred8", _fp), ("gt8", _fp), ("residual8", _fp), ("depth8", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


class FrameEvalRow(C.Structure):
    """struct lvdgs_frame_eval_row (include/lvdgs.h): what one call leaves at ``out_row``."""
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
    """struct lvdgs_tsdf_volume (include/lvdgs.h)."""
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3),
        ("voxel_size", C.c_float), ("trunc", C.c_float), ("max_weight", C.c_float),
        ("tsdf", _fp), ("weight", _fp), ("r", _fp), ("g", _fp), ("b", _fp),
    ]


class TsdfViewArgs(C.Structure):
    """struct lvdgs_tsdf_view (include/lvdgs.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("depth_min", C.c_float), ("depth_trunc", C.c_float),
        ("R", _fp), ("T", _fp), ("depth", _fp), ("image", _fp), ("mask", _fp),
    ]


class TsdfMeshArgs(C.Structure):
    """struct lvdgs_tsdf_mesh_args (include/lvdgs.h)."""
    _fields_ = [
        ("vol", TsdfVolumeArgs), ("seq", C.c_uint32), ("vertex_capacity", C.c_int32), ("face_capacity", C.c_int32),
        ("vertices", _fp), ("colors", _fp), ("faces", _fp), ("host_state", _fp),
        ("scratch", _fp), ("scratch_bytes", C.c_size_t),
    ]


TSDF_MAX_VIEWS, TSDF_HOST_BYTES = 16, 64
TSDF_SEQ, TSDF_N_VERTICES, TSDF_N_FACES, TSDF_OVERFLOW = 0, 1, 2, 3
TSDF_OVERFLOW_VERTICES, TSDF_OVERFLOW_FACES, TSDF_OVERFLOW_INT32 = 1, 2, 4     # bits of the [TSDF_OVERFLOW] word


DEPTH_SAMPLE_BYTE, DEPTH_SAMPLE_WORD = 1, 2     # lvdgs_ingest_depth_args.sample_type
MAP_OUTSIDE = -2 ** 31     # INT32_MIN in an undistortion map: the destination pixel's source lies outside


class StateLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "geom_rec", "geom_tiles_touched", "geom_slot_base", "bin_point_list", "bin_tile_keys",
        "img_ranges", "img_final_T", "img_n_contrib", "geom_rec_floats")]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


# every symbol include/lvdgs.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "lvdgs_geom_bytes", "lvdgs_prepare_scratch_bytes", "lvdgs_binning_bytes", "lvdgs_image_bytes",
    "lvdgs_render_scratch_bytes", "lvdgs_backward_scratch_bytes", "lvdgs_forward_prepare", "lvdgs_forward_render",
    "lvdgs_forward",
    "lvdgs_backward", "lvdgs_mark_visible", "lvdgs_state_layout_query", "lvdgs_knn_scratch_bytes",
    "lvdgs_dist2_knn3", "lvdgs_rope2d", "lvdgs_rope2d_strided", "lvdgs_loss_scratch_bytes", "lvdgs_photometric_loss_forward",
    "lvdgs_photometric_loss_backward", "lvdgs_photometric_loss_value_and_grad", "lvdgs_photometric_loss_partials", "lvdgs_tracking_tail", "lvdgs_backward_fused_loss", "lvdgs_blend_forward_batch", "lvdgs_blend_backward_fused_loss_batch", "lvdgs_masked_depth_scratch_bytes", "lvdgs_masked_depth_l1_forward",
    "lvdgs_masked_depth_l1_backward", "lvdgs_pose_step", "lvdgs_host_device_pointer", "lvdgs_pose_step_batch", "lvdgs_adam_step", "lvdgs_isotropic_scratch_bytes", "lvdgs_isotropic_reg", "lvdgs_view_stats", "lvdgs_map_stats_apply", "lvdgs_map_view_tail", "lvdgs_ssim_scratch_bytes", "lvdgs_ssim_l1",
    "lvdgs_masked_loss_scratch_bytes", "lvdgs_masked_loss_batch", "lvdgs_backward_masked_loss", "lvdgs_blend_backward_window_batch", "lvdgs_forward_batch", "lvdgs_forward_backward_fused_loss", "lvdgs_map_view_tail_batch", "lvdgs_gaussian_backward_batch",
    "lvdgs_depth_align_scratch_bytes", "lvdgs_depth_align", "lvdgs_depth_align_resume", "lvdgs_pnp_scratch_bytes", "lvdgs_pnp_ransac", "lvdgs_recip_nn_scratch_bytes", "lvdgs_reciprocal_nn",
    "lvdgs_format_plan_query", "lvdgs_format_table", "lvdgs_format_scratch_bytes", "lvdgs_format_image", "lvdgs_match_depth_scale",
    "lvdgs_edge_mask_scratch_bytes", "lvdgs_edge_mask", "lvdgs_frame_summary_scratch_bytes", "lvdgs_frame_summary",
    "lvdgs_ms_deform_attn_forward", "lvdgs_ms_deform_attn_backward",
    "lvdgs_dynamic_mask_state_bytes", "lvdgs_dynamic_mask_scratch_bytes", "lvdgs_dynamic_mask",
    "lvdgs_seed_scratch_bytes", "lvdgs_seed_points",
    "lvdgs_map_edit_scratch_bytes", "lvdgs_map_edit_plan", "lvdgs_map_edit_apply",
    "lvdgs_undistort_map", "lvdgs_ingest_frame", "lvdgs_ingest_depth",
    "lvdgs_frame_eval_scratch_bytes", "lvdgs_frame_eval",
    "lvdgs_tsdf_integrate", "lvdgs_tsdf_mesh_scratch_bytes", "lvdgs_tsdf_mesh",
    "lvdgs_last_error", "lvdgs_version", "lvdgs_profile_enable",
    "lvdgs_profile_reset", "lvdgs_profile_read",
)

_lib = None


class LvdgsError(RuntimeError):
    pass


def lib():
    """The loaded library (loads on first use; raises if the HIP build is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LvdgsError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C lvd_gs-slam_amd/csrc`). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.lvdgs_last_error.restype = C.c_char_p
        L.lvdgs_version.restype = C.c_char_p
        for name in ("lvdgs_geom_bytes", "lvdgs_prepare_scratch_bytes"):
            getattr(L, name).restype = C.c_size_t
            getattr(L, name).argtypes = [C.c_int32]
        L.lvdgs_binning_bytes.restype = C.c_size_t
        L.lvdgs_binning_bytes.argtypes = [C.c_int64]
        L.lvdgs_image_bytes.restype = C.c_size_t
        L.lvdgs_image_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_render_scratch_bytes.restype = C.c_size_t
        L.lvdgs_render_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32]
        L.lvdgs_backward_scratch_bytes.restype = C.c_size_t
        L.lvdgs_backward_scratch_bytes.argtypes = [C.c_int32, C.c_int64]
        L.lvdgs_forward_prepare.argtypes = [C.POINTER(Args), C.POINTER(C.c_int64), C.c_void_p]
        L.lvdgs_forward_render.argtypes = [C.POINTER(Args), C.c_void_p]
        L.lvdgs_forward.argtypes = [C.POINTER(Args), C.POINTER(C.c_int64), C.c_void_p]
        L.lvdgs_backward.argtypes = [C.POINTER(Args), C.c_void_p]
        L.lvdgs_blend_forward_batch.argtypes = [C.POINTER(C.POINTER(Args)), C.c_int32, C.c_void_p]
        L.lvdgs_blend_backward_fused_loss_batch.argtypes = [C.POINTER(C.POINTER(Args)), C.POINTER(C.POINTER(LossArgs)), C.c_int32, C.c_int32, C.c_void_p]
        L.lvdgs_mark_visible.argtypes = [C.c_int32, _fp, _fp, _fp, _fp, C.c_void_p]
        L.lvdgs_host_device_pointer.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.lvdgs_state_layout_query.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(StateLayout)]
        L.lvdgs_knn_scratch_bytes.restype = C.c_size_t
        L.lvdgs_knn_scratch_bytes.argtypes = [C.c_int32]
        L.lvdgs_dist2_knn3.argtypes = [C.c_int32, _fp, _fp, _fp, C.c_size_t, C.c_void_p]
        L.lvdgs_rope2d.argtypes = [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p]
        L.lvdgs_rope2d_strided.argtypes = [_fp, C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                           C.c_int64, C.c_float, C.c_float, C.c_void_p]
        L.lvdgs_loss_scratch_bytes.restype = C.c_size_t
        L.lvdgs_loss_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_photometric_loss_forward.argtypes = [C.POINTER(LossArgs), C.c_void_p]
        L.lvdgs_photometric_loss_backward.argtypes = [C.POINTER(LossArgs), C.c_void_p]
        L.lvdgs_photometric_loss_value_and_grad.argtypes = [C.POINTER(LossArgs), C.c_void_p]
        L.lvdgs_masked_depth_scratch_bytes.restype = C.c_size_t
        L.lvdgs_masked_depth_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_masked_depth_l1_forward.argtypes = [C.POINTER(MaskedDepthArgs), C.c_void_p]
        L.lvdgs_masked_depth_l1_backward.argtypes = [C.POINTER(MaskedDepthArgs), C.c_void_p]
        L.lvdgs_pose_step.argtypes = [C.POINTER(PoseStepArgs), C.c_void_p]
        L.lvdgs_pose_step_batch.argtypes = [C.POINTER(PoseStepArgs), C.c_int32, C.c_void_p]
        L.lvdgs_photometric_loss_partials.argtypes = [C.POINTER(LossArgs), C.c_void_p]
        L.lvdgs_tracking_tail.argtypes = [C.POINTER(LossArgs), C.POINTER(Args), C.POINTER(PoseStepArgs), C.c_void_p, C.c_int32, C.c_void_p]
        L.lvdgs_backward_fused_loss.argtypes = [C.POINTER(Args), C.POINTER(LossArgs), C.c_int32, C.c_void_p]
        L.lvdgs_adam_step.argtypes = [C.POINTER(AdamTensor), C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.lvdgs_isotropic_scratch_bytes.restype = C.c_size_t
        L.lvdgs_isotropic_scratch_bytes.argtypes = [C.c_int32]
        L.lvdgs_isotropic_reg.argtypes = [C.c_int32, _fp, _fp, C.c_float, _fp, C.c_size_t, _fp, C.c_void_p]
        L.lvdgs_view_stats.argtypes = [C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
        L.lvdgs_map_view_tail.argtypes = [C.POINTER(LossArgs), C.POINTER(Args), _fp, C.POINTER(ViewStatsArgs), C.c_void_p]
        L.lvdgs_map_view_tail_batch.argtypes = [C.POINTER(C.POINTER(LossArgs)), C.POINTER(C.POINTER(Args)), C.POINTER(C.c_void_p),
                                                C.POINTER(C.POINTER(ViewStatsArgs)), C.c_int32, C.c_void_p]
        L.lvdgs_map_stats_apply.argtypes = [C.c_int32, _fp, _fp, _fp, _fp, C.c_int32, _fp, _fp, _fp, C.c_void_p]
        L.lvdgs_ssim_scratch_bytes.restype = C.c_size_t
        L.lvdgs_ssim_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lvdgs_ssim_l1.argtypes = [C.POINTER(SsimArgs), C.c_void_p]
        L.lvdgs_forward_backward_fused_loss.argtypes = [C.POINTER(Args), C.POINTER(LossArgs), C.c_int32, C.POINTER(C.c_int64), C.c_void_p]
        L.lvdgs_forward_batch.argtypes = [C.POINTER(C.POINTER(Args)), C.c_int32, C.POINTER(C.c_int64), C.c_void_p]
        L.lvdgs_masked_loss_scratch_bytes.restype = C.c_size_t
        L.lvdgs_masked_loss_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_masked_loss_batch.argtypes = [C.POINTER(C.POINTER(MaskedLossArgs)), C.c_int32, C.c_void_p]
        L.lvdgs_backward_masked_loss.argtypes = [C.POINTER(Args), C.POINTER(MaskedLossArgs), C.c_void_p]
        L.lvdgs_gaussian_backward_batch.argtypes = [C.POINTER(C.POINTER(Args)), C.c_int32, C.c_void_p]
        L.lvdgs_blend_backward_window_batch.argtypes = [C.POINTER(C.POINTER(Args)), C.POINTER(C.POINTER(LossArgs)), C.POINTER(C.POINTER(MaskedLossArgs)),
                                                        C.c_int32, C.c_int32, C.c_void_p]
        L.lvdgs_depth_align_scratch_bytes.restype = C.c_size_t
        L.lvdgs_depth_align_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lvdgs_depth_align.argtypes = [C.POINTER(DepthAlignArgs), C.c_void_p]
        L.lvdgs_depth_align_resume.argtypes = [C.POINTER(DepthAlignArgs), C.c_float, C.c_void_p]
        L.lvdgs_pnp_scratch_bytes.restype = C.c_size_t
        L.lvdgs_pnp_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_pnp_ransac.argtypes = [C.POINTER(PnpArgs), C.c_void_p]
        L.lvdgs_recip_nn_scratch_bytes.restype = C.c_size_t
        L.lvdgs_recip_nn_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lvdgs_reciprocal_nn.argtypes = [C.POINTER(RecipNnArgs), C.c_void_p]
        L.lvdgs_format_plan_query.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(FormatPlan)]
        L.lvdgs_format_table.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.lvdgs_format_scratch_bytes.restype = C.c_size_t
        L.lvdgs_format_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lvdgs_format_image.argtypes = [C.POINTER(FormatImageArgs), C.c_void_p]
        L.lvdgs_match_depth_scale.argtypes = [C.POINTER(MatchScaleArgs), C.c_void_p]
        L.lvdgs_edge_mask_scratch_bytes.restype = C.c_size_t
        L.lvdgs_edge_mask_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_edge_mask.argtypes = [C.POINTER(EdgeMaskArgs), C.c_void_p]
        L.lvdgs_frame_summary_scratch_bytes.restype = C.c_size_t
        L.lvdgs_frame_summary_scratch_bytes.argtypes = []
        L.lvdgs_frame_summary.argtypes = [C.POINTER(FrameSummaryArgs), C.c_void_p]
        L.lvdgs_ms_deform_attn_forward.argtypes = [_fp] * 5 + [C.c_int32] * 7 + [_fp, C.c_void_p]
        L.lvdgs_ms_deform_attn_backward.argtypes = [_fp] * 5 + [C.c_int32] * 7 + [_fp] * 4 + [C.c_void_p]
        L.lvdgs_dynamic_mask_state_bytes.restype = C.c_size_t
        L.lvdgs_dynamic_mask_state_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lvdgs_dynamic_mask_scratch_bytes.restype = C.c_size_t
        L.lvdgs_dynamic_mask_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_dynamic_mask.argtypes = [C.POINTER(DynamicMaskArgs), C.c_void_p]
        L.lvdgs_seed_scratch_bytes.restype = C.c_size_t
        L.lvdgs_seed_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_seed_points.argtypes = [C.POINTER(SeedArgs), C.c_void_p]
        L.lvdgs_map_edit_scratch_bytes.restype = C.c_size_t
        L.lvdgs_map_edit_scratch_bytes.argtypes = [C.c_int32]
        L.lvdgs_map_edit_plan.argtypes = [C.POINTER(MapEditPlanArgs), C.c_void_p]
        L.lvdgs_map_edit_apply.argtypes = [C.POINTER(MapEditApplyArgs), C.c_void_p]
        L.lvdgs_undistort_map.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                                          _fp, _fp, C.c_void_p]
        L.lvdgs_ingest_frame.argtypes = [C.POINTER(IngestArgs), C.c_void_p]
        L.lvdgs_ingest_depth.argtypes = [C.POINTER(IngestDepthArgs), C.c_void_p]
        L.lvdgs_frame_eval_scratch_bytes.restype = C.c_size_t
        L.lvdgs_frame_eval_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.lvdgs_frame_eval.argtypes = [C.POINTER(FrameEvalArgs), C.c_void_p]
        L.lvdgs_tsdf_integrate.argtypes = [C.POINTER(TsdfVolumeArgs), C.POINTER(C.POINTER(TsdfViewArgs)), C.c_int32, C.c_void_p]
        L.lvdgs_tsdf_mesh_scratch_bytes.restype = C.c_size_t
        L.lvdgs_tsdf_mesh_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lvdgs_tsdf_mesh.argtypes = [C.POINTER(TsdfMeshArgs), C.c_void_p]
        L.lvdgs_profile_enable.argtypes = [C.c_int]
        L.lvdgs_profile_read.argtypes = [C.POINTER(KernelTime), C.c_int]
        _lib = L
    return _lib


def ptr(t):
    """A tensor's data as a pointer field of an argument block (None: NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def is_f32(t, device=None):
    """Is ``t`` a contiguous float32 tensor on ``device`` (None: on any GPU)?"""
    return (torch.is_tensor(t) and (t.is_cuda if device is None else t.device == device) and t.dtype is torch.float32
            and t.is_contiguous())


def f32(t, device):
    """``t`` detached, as a contiguous float32 tensor on ``device`` (itself when it is one: no conversion kernel, no dispatcher
    round trip through ``.to()``)."""
    t = t.detach()
    return t if is_f32(t, device) else t.to(device=device, dtype=torch.float32).contiguous()


def device_bytes(n, device):
    """A byte buffer of at least ``n`` bytes (and at least 256) on ``device``."""
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=device)


def raw_stream(device):
    """hipStream_t of PyTorch's current stream ON `device` (the tensor's device, which need not be the current one),
    as a c_void_p.  A direct C call: torch.cuda.current_stream() costs tens of microseconds of Python per call."""
    idx = device.index if (device is not None and device.index is not None) else torch.cuda.current_device()
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


class on_device:
    """Make `device` the current HIP device for the duration of a library call when it is not already (kernels are
    launched on the current device; a stream of another device would be rejected)."""
    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index

    def __enter__(self):
        self.prev = None
        if self.idx is not None:
            cur = torch.cuda.current_device()
            if cur != self.idx:
                self.prev = cur
                torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


class DeviceScratch:
    """A library call's scratch, one buffer per device: kept while large enough, replaced by a larger one on demand
    (``device_bytes``).  ``zeroed``: a new buffer is zero-filled once; ``headroom``: a new buffer gets half as much again."""

    def __init__(self, *, zeroed=False, headroom=False):
        self.zeroed, self.headroom, self.buffers = zeroed, headroom, {}

    def get(self, device, nbytes):
        nbytes = int(nbytes)
        buf = self.buffers.get(device.index)
        if buf is None or buf.numel() < nbytes:
            buf = self.buffers[device.index] = device_bytes(nbytes + (nbytes // 2 if self.headroom else 0), device)
            if self.zeroed:
                buf.zero_()
        return buf


def next_seq(seq):
    """The sequence number that follows ``seq``: 1 .. 0x7FFFFFFF round and round, never 0 -- what a cleared tag word holds."""
    return (int(seq) % 0x7FFFFFFF) + 1


def host_block_verdict(words, name, tag, seq=None, statuses=()):
    """The tag word of a host block after the call's one wait: returned when it is the call's sequence number or one of the statuses
    the call can end in; anything else -- the cleared word above all -- means the call wrote no state."""
    found = int(words[tag])
    if (seq is not None and found == seq) or found in statuses:
        return found
    expected = f"sequence number {seq}" if seq is not None else "status " + " or ".join(str(s) for s in statuses)
    raise LvdgsError(f"{name} left no state (word [{tag}] of its host block holds {found}, expected {expected})")


class HostCall:
    """One entry point of the library that reports through a block of pinned host memory (include/lvdgs.h, "Host blocks"): its
    per-device block, scratch and sequence counter, and the call with its one wait.

    ``name``: the library function.  ``statuses``: what its tag word -- ``[tag]`` of the block -- may hold after the call; None: the
    call is tagged with the ``seq`` of its argument block, which ``run`` fills in.  ``tag=None``: no tag (``lvdgs_depth_align``,
    whose block is a state that its resume call reads: ``run`` neither clears nor judges it)."""

    def __init__(self, name, *, statuses=None, tag=0, zeroed=False, headroom=False):
        self.name, self.statuses, self.tag, self.headroom = name, statuses, tag, headroom
        self.scratch = DeviceScratch(zeroed=zeroed, headroom=headroom)
        self.blocks, self.words, self.seq = {}, {}, {}      # device index -> pinned block; -> its int32 words; -> last sequence number
        self.fn = None

    def resources(self, device, block_bytes, scratch_bytes=None):
        """(the device's pinned block of at least ``block_bytes`` bytes -- the one of the call before while large enough --, its scratch
        of at least ``scratch_bytes``; None: the call takes no scratch)."""
        block_bytes = int(block_bytes)
        block = self.blocks.get(device.index)
        if block is None or block.numel() < block_bytes:
            block = self.blocks[device.index] = torch.zeros(block_bytes + (block_bytes // 2 if self.headroom else 0), dtype=torch.uint8).pin_memory()
            self.words[device.index] = block.numpy().view(np.int32)
        return block, None if scratch_bytes is None else self.scratch.get(device, scratch_bytes)

    def wait(self, device):
        """The one wait of the call: until everything enqueued on the device's current stream has run."""
        torch.cuda.current_stream(device).synchronize()

    def run(self, device, args, fn=None):
        """``fn(byref(args), stream)`` (default: the library function) on ``device``, whose block ``args.host_state`` is, and the
        wait -> the block as int32 words (a view: copy what is to outlive the next call)."""
        words = self.words[device.index]
        if fn is None:
            fn = self.fn = self.fn or getattr(lib(), self.name)
        seq = None
        if self.tag is not None:
            words[self.tag] = 0      # whatever the call before left: only this call's own tag counts
            if self.statuses is None:
                seq = args.seq = self.seq[device.index] = next_seq(self.seq.get(device.index, 0))
        with on_device(device):
            check(fn(C.byref(args), raw_stream(device)), self.name)
            self.wait(device)
        if self.tag is not None:
            host_block_verdict(words, self.name, self.tag, seq, self.statuses or ())
        return words


_gc_policy = None      # "scoped" | "process" | "off"; None: not decided yet (LVDGS_GC_FREEZE / set_gc_policy / first loop entry)
_gc_depth = 0


def set_gc_policy(policy):
    """How the product's loops keep CPython's full-heap garbage collections out of their iterations.

    The loops run at 0.2-2 ms per iteration and allocate a few hundred small Python objects in each, which makes CPython start a
    FULL collection every few dozen to few hundred iterations; with the whole heap of an application that has PyTorch imported
    (about a million objects) in the oldest generation that is one stall of 40-110 ms (measured: ``tools/side_stall_diag.py``) --
    20-60 iterations' worth of time.

    * ``"scoped"`` (the default): ``gc.freeze()`` when the outermost product loop is entered (``track_frame``, ``map_window``,
      ``initialize_map``, ``color_refinement``, ``slam_sequence``) -- everything alive moves to the permanent generation, two list
      splices, no collection -- and ``gc.unfreeze()`` when it returns: inside the loop the collector walks only what the loop itself
      allocated, and afterwards the host application's collector sees its heap exactly as before (``gc.get_freeze_count() == 0``).
      An application that calls ``gc.freeze()`` ITSELF should pick one of the other two: the scoped exit would thaw its objects too
      (a freeze found in place at the first loop entry of the process switches the policy to "off" by itself).
    * ``"process"`` (``LVDGS_GC_FREEZE=1``, what every round up to 5 did unasked): one ``gc.collect(); gc.freeze()`` at the first loop
      entry, for the life of the process.  Cyclic garbage among the objects alive at that moment is never reclaimed.
    * ``"off"`` (``LVDGS_GC_FREEZE=0``): the collector is left alone.
    """
    global _gc_policy
    if policy not in ("scoped", "process", "off"):
        raise ValueError("gc policy: 'scoped', 'process' or 'off'")
    if policy == "process" and _gc_policy != "process":
        import gc
        gc.collect()
        gc.freeze()
    _gc_policy = policy


class quiet_gc:
    """Context manager around a product loop: see ``set_gc_policy``.  Re-entrant (only the outermost scope acts)."""
    __slots__ = ("acted",)

    def __enter__(self):
        global _gc_policy, _gc_depth
        import gc
        self.acted = False
        if _gc_policy is None:
            env = os.environ.get("LVDGS_GC_FREEZE", "scoped")
            _gc_policy = {"0": "off", "1": "process"}.get(env, "scoped")
            if _gc_policy == "scoped" and gc.get_freeze_count() > 0:   # (walks the permanent generation: asked once per process)
                _gc_policy = "off"   # the host application manages a freeze of its own: hands off
            if _gc_policy == "process":
                gc.collect()
                gc.freeze()
        _gc_depth += 1
        if _gc_policy == "scoped" and _gc_depth == 1:
            gc.freeze()
            self.acted = True
        return self

    def __exit__(self, *exc):
        global _gc_depth
        _gc_depth -= 1
        if self.acted:
            import gc
            gc.unfreeze()
        return False


def check(status, what):
    if status != OK:
        raise LvdgsError(f"{what} failed ({status}): {lib().lvdgs_last_error().decode()}")


def profile_enable(on=True):
    lib().lvdgs_profile_enable(1 if on else 0)


def profile_reset():
    lib().lvdgs_profile_reset()


def profile_read():
    """{kernel name: (launches, total_ms)} measured with HIP events on the launch stream."""
    buf = (KernelTime * 64)()
    n = lib().lvdgs_profile_read(buf, 64)
    return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(n)}
