/*
 * lvdgs.h -- C ABI of the MI355X (gfx950) differentiable 3D-Gaussian tile rasterizer.
 *
 * This is the drop-in boundary for the path LVD-GS reaches through
 *     gaussian_splatting.gaussian_renderer.render(viewpoint, gaussians, pipe, bg)
 * (call sites: reference utils/slam_frontend.py:1493, utils/slam_backend.py:98,184,277,407,
 *  utils/eval_utils_0806.py:215, utils/init_pose.py:145).  Upstream that facade calls the
 * `diff_gaussian_rasterization` extension (reference README.md:43; sources absent from the
 * reference checkout), whose Python-visible entry points are
 *     _C.rasterize_gaussians(...)            -> lvdgs_forward_prepare + lvdgs_forward_render
 *     _C.rasterize_gaussians_backward(...)   -> lvdgs_backward
 *     _C.mark_visible(...)                   -> lvdgs_mark_visible
 * Other absent native dependencies the north star names:
 *     simple_knn._C.distCUDA2  (README.md:42) -> lvdgs_dist2_knn3
 *     curope rope_2d           (README.md:49) -> lvdgs_rope2d
 *
 * Conventions
 *  - plain C: raw device pointers, sizes, a hipStream_t passed as void*; no C++ exceptions
 *    cross the boundary; every entry point returns an lvdgs_status (0 = ok) and
 *    lvdgs_last_error() returns a thread-local message for the last failure;
 *  - all work is enqueued on the given stream and is ordered with it; the host waits for the
 *    device in two places only, both for the number of (Gaussian, tile) pairs the caller sizes
 *    the binning buffer with (the device->host read upstream performs): lvdgs_forward_prepare
 *    synchronises the stream, lvdgs_forward waits -- with everything else of the frame already
 *    enqueued -- until the tile-scan kernel has stored the count into pinned host memory;
 *  - the library owns no device memory: the caller allocates the three state buffers
 *    (geometry, binning, image -- upstream's geomBuffer / binningBuffer / imgBuffer) and the
 *    scratch buffers, with the sizes the lvdgs_*_bytes functions report, and keeps the state
 *    buffers alive until backward (PyTorch: ctx.save_for_backward);
 *  - no global mutable state that results depend on: besides the optional profiling counters, lvdgs_forward keeps a
 *    per-thread, per-device block of pinned, device-visible words (the tile-scan kernel writes the pair count lvdgs_forward
 *    returns there, and the frame's longest tile segment, which only selects WHICH kernels the next frame launches for its long tile
 *    lists -- the sort kernels, and the deep-lists build of the forward blend kernel: a hint, never a result); the environment is looked at once per
 *    process for the test hook LVDGS_FORCE_RADIX_GROUPING;
 *  - all float tensors are float32, contiguous, row-major; matrices are 4x4 in the
 *    row-vector layout the reference's Camera produces (world_view_transform =
 *    getWorld2View2(R,T).transpose(0,1), utils/camera_utils.py:106-116).
 *
 * Host blocks
 *  Nine calls enqueue their launches, do not wait, and report through a block of host memory, `host_state`: lvdgs_depth_align,
 *  lvdgs_pnp_ransac, lvdgs_reciprocal_nn, lvdgs_match_depth_scale, lvdgs_frame_summary, lvdgs_seed_points, lvdgs_map_edit_plan,
 *  lvdgs_tsdf_mesh, lvdgs_mesh_cull.
 *  - the block is the caller's: page-locked, mapped host memory (hipHostMalloc, a pinned PyTorch tensor) of the size its section
 *    states, which the caller passes by its HOST address; memory that is not so is refused with LVDGS_E_HIP, "<call>: host_state is
 *    not mapped pinned memory", before any launch;
 *  - the call's last launch writes the block as int32 words, and its TAG word LAST.  The calls tagged with `seq` store it behind a
 *    system-scope fence: a host that finds the tag finds every other word of the block.  The calls tagged with a status store it
 *    last with no fence in front (the fence measurably slows them): their block is complete behind the caller's wait for the
 *    stream, not before;
 *  - the caller clears the tag word, makes the call, synchronises the stream ONCE and looks at the tag: a word that is not this
 *    call's tag means that the call left no state (nothing else in the block is then to be believed);
 *  - the tag is the `seq` of the argument block -- any value the caller's previous call did not use, 0 excepted -- for
 *    lvdgs_frame_summary, lvdgs_seed_points, lvdgs_map_edit_plan, lvdgs_tsdf_mesh and lvdgs_mesh_cull, and the status word [0], never 0, for lvdgs_pnp_ransac,
 *    lvdgs_reciprocal_nn and lvdgs_match_depth_scale;
 *  - lvdgs_depth_align is the exception: its block has no tag, it is a state that every launch which changes it mirrors, that is
 *    complete behind the caller's wait for the stream, and that lvdgs_depth_align_resume reads ON THE HOST -- the caller leaves it
 *    alone between the two.
 *  The sections below give each block's size and word layout only.
 */
#ifndef LVDGS_H
#define LVDGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LVDGS_OK = 0,
    LVDGS_E_INVALID = 1, /* bad argument (null pointer, size mismatch, buffer too small) */
    LVDGS_E_HIP = 2,     /* a HIP runtime call or kernel launch failed                   */
    LVDGS_E_RANGE = 3,   /* problem exceeds a built-in limit (e.g. > 2^31 pairs)         */
    LVDGS_E_CAPACITY = 4 /* lvdgs_forward: pair_capacity was too small; see lvdgs_forward */
} lvdgs_status;

/* One argument block serves the three rasterizer calls; each call reads the fields it needs
 * (marked P = prepare, R = render, B = backward).  Zero-initialise, then fill. */
typedef struct lvdgs_args {
    /* ---- GaussianRasterizationSettings (P R B) ---- */
    int32_t image_height, image_width;
    float tanfovx, tanfovy;
    float scale_modifier;
    int32_t sh_degree;   /* 0..3 */
    int32_t prefiltered; /* accepted for signature parity; unused */
    int32_t debug;       /* 1: synchronise and check after every launch */
    const float *bg;             /* device, 3  */
    const float *viewmatrix;     /* device, 16 */
    const float *projmatrix;     /* device, 16: viewmatrix * projmatrix_raw */
    const float *projmatrix_raw; /* device, 16 (B: pose gradient) */
    const float *campos;         /* device, 3  */

    /* ---- Gaussians (P B) ---- */
    int32_t num_gaussians; /* N */
    int32_t sh_coeffs;     /* M: coefficients per Gaussian in `shs` (>= (sh_degree+1)^2) */
    const float *means3D;        /* N*3 */
    const float *opacities;      /* N   (activated, in [0,1]) */
    const float *scales;         /* N*3 (activated) or NULL with cov3D_precomp */
    const float *rotations;      /* N*4 (r,x,y,z; used as given) or NULL */
    const float *cov3D_precomp;  /* N*6 (xx,xy,xz,yy,yz,zz) or NULL */
    const float *shs;            /* N*M*3 or NULL with colors_precomp */
    const float *colors_precomp; /* N*3 or NULL */

    /* ---- state + scratch buffers (caller-allocated, 256-byte aligned) ---- */
    void *geom_state;     size_t geom_bytes;    /* P w, R rw, B r : lvdgs_geom_bytes(N)           */
    void *binning_state;  size_t binning_bytes; /*      R w,  B r : lvdgs_binning_bytes(D)        */
    void *image_state;    size_t image_bytes;   /*      R w,  B r : lvdgs_image_bytes(W,H)        */
    void *scratch;        size_t scratch_bytes; /* P: lvdgs_prepare_scratch_bytes(N)
                                                   R: lvdgs_render_scratch_bytes(N,D,W,H)
                                                   B: lvdgs_backward_scratch_bytes(N,D)           */
    int64_t num_rendered; /* D, as returned by prepare (R B) */

    /* ---- forward outputs ---- */
    int32_t *radii;     /* N       (P w, B r) */
    float *out_color;   /* 3*H*W   (R w, B r) */
    float *out_depth;   /* H*W     (R w)      */
    float *out_opacity; /* H*W     (R w)      */
    int32_t *n_touched; /* N       (R w)      */

    /* ---- backward inputs ---- */
    const float *dL_dout_color;   /* 3*H*W         */
    const float *dL_dout_depth;   /* H*W or NULL   */
    const float *dL_dout_opacity; /* H*W or NULL   */

    /* ---- backward outputs (every element is written) ---- */
    float *dL_dmeans3D;   /* N*3 */
    float *dL_dmeans2D;   /* N*3: d/d NDC x,y of the projected mean (viewspace_points.grad), z = 0 */
    float *dL_dopacities; /* N   */
    float *dL_dscales;    /* N*3 or NULL with cov3D_precomp */
    float *dL_drotations; /* N*4 or NULL with cov3D_precomp */
    float *dL_dcov3D;     /* N*6 or NULL (only written when cov3D_precomp != NULL) */
    float *dL_dshs;       /* N*M*3 or NULL with colors_precomp */
    float *dL_dcolors;    /* N*3 or NULL with shs */
    float *dL_dtau;       /* 6: [d/d rho (3), d/d theta (3)] of T_w2c <- Exp(tau) T_w2c
                             (reference utils/pose_utils.py:70-87).  NULL: the per-workgroup partial sums stay in
                             `scratch` and lvdgs_tracking_tail reduces them (one launch less) */

    /* ---- single-call forward only ---- */
    int64_t pair_capacity; /* pairs binning_state / scratch were sized for (lvdgs_forward) */

    /* ---- optional: activations fused into the projection kernel (P B) ----
     * bit 0: `scales` holds log-scales (exp applied), bit 1: `rotations` is un-normalised (divided by its
     * norm), bit 2: `opacities` holds logits (sigmoid applied).  The matching gradient outputs are then
     * w.r.t. the raw values.  0 = inputs are already activated, as upstream's render() passes them. */
    int32_t activations;

    /* ---- optional switches (P R B; the same value in all calls of one frame) ---- */
    int32_t flags;          /* LVDGS_FLAG_* below; 0 = default behaviour */
    /* ---- optional: render a horizontal band of the image only (P R B) ----
     * Tile rows [tile_row_begin, tile_row_end) of the 16-pixel tile grid; both 0 = the whole image.  Pixels outside the
     * band are not written (out_color / out_depth / out_opacity / image_state keep what they held), only the band's
     * (Gaussian, tile) pairs are listed, n_touched counts the band's pixels, and the backward returns the band's share
     * of every gradient: bands that partition the image add up to the whole frame's gradients (the loss's partial sums
     * of lvdgs_backward_fused_loss are left for the band's tiles, zeros elsewhere).  This is what lets one view of the
     * mapping window (reference utils/slam_backend.py:180-306: losses summed over views before one backward) be split
     * between GPUs. */
    int32_t tile_row_begin, tile_row_end;
} lvdgs_args;

/* lvdgs_args.flags */
enum {
    LVDGS_FLAG_LIST_ALL_TILES = 1, /* list every tile of a Gaussian's 3-sigma rectangle -- the reference's pair list, bit
                                      for bit (num_rendered, point_list, ranges, n_contrib) -- instead of only the tiles
                                      on which it can reach alpha >= 1/255 (outputs are the same either way) */
    LVDGS_FLAG_NO_BLEND = 8,       /* R, B: the call leaves its blend pass out -- lvdgs_forward / lvdgs_forward_render stop behind the
                                      per-tile depth sort (out_color / out_depth / out_opacity / n_touched and the image
                                      state's final_T / n_contrib are not written), lvdgs_backward_fused_loss starts behind the
                                      backward blend pass -- because the caller runs that pass for several views of one size in
                                      ONE launch: lvdgs_blend_forward_batch / lvdgs_blend_backward_fused_loss_batch (the views
                                      of a mapping window; the results are the single calls', bit for bit) */
    LVDGS_FLAG_SUPER_TILES = 16,   /* R: a HINT for frames whose Gaussians are listed on many tiles each (opaque surfaces of large flat Gaussians: 70-80
                                      tiles per Gaussian): the (Gaussian, tile) pairs are grouped and depth-sorted per 64 x 64-pixel super-tile -- a tenth of
                                      the keys to scatter and sort there -- and every tile's list is read off its super-tile's sorted list.  point_list,
                                      ranges and every output are the same bits with and without it; worth setting when num_rendered exceeds ~16 pairs per
                                      Gaussian (lvdgs.rasterizer decides from the previous frame's count).  Ignored with LVDGS_FLAG_LIST_ALL_TILES, with a
                                      band of tile rows, on frames of fewer than 64 tiles and by lvdgs_forward_render; the views of lvdgs_forward_batch must agree on it.
                                      The super-tile lists share pair_capacity and may hold more pairs than the tile lists (a Gaussian whose rectangle spans more
                                      than 64 super-tiles is listed on all of them); when they outgrow the capacity and the tile lists do not, lvdgs_forward,
                                      lvdgs_forward_batch (per view) and lvdgs_forward_backward_fused_loss redo the view without the hint inside the call and
                                      return LVDGS_OK with the tile pair count -- num_rendered and LVDGS_E_CAPACITY concern the tile lists alone.
                                      B: the per-Gaussian pass of lvdgs_backward*, lvdgs_forward_backward_fused_loss and lvdgs_gaussian_backward_batch runs with helper waves (workgroups of eight waves: the second half of a
                                      large-footprint wave's pair records is summed beside the first) -- the same sums in the same order, sooner. */
    LVDGS_FLAG_POSE_ONLY = 4,      /* B: only the camera-pose gradient (dL_dtau, or its partial sums for lvdgs_tracking_tail) and --
                                      lvdgs_backward_fused_loss -- the loss value and exposure gradients are produced.  The
                                      reference's tracking optimiser holds the pose and the exposure alone
                                      (utils/slam_frontend.py:1468-1490, stepped at :1520); the Gaussian gradients autograd
                                      computes beside them are dropped.  With this flag they are not computed: the dL_d*
                                      outputs other than dL_dtau are ignored (may be NULL) and NOT written, the backward blend
                                      pass leaves out the sums that feed only colours and opacities, the per-Gaussian pass
                                      neither reads opacities / SH coefficients nor writes N x 14 gradients.  dL_dtau is bit for
                                      bit the full backward's.  Needs sh_degree 0 or colors_precomp (a view-dependent colour
                                      feeds the pose gradient through the colour gradient): LVDGS_E_INVALID otherwise */
    LVDGS_FLAG_ACCUMULATE_PARAM_GRADS = 2 /* B: the gradients w.r.t. the Gaussian parameters (dL_dmeans3D, dL_dopacities,
                                      dL_dscales, dL_drotations, dL_dcov3D, dL_dshs / dL_dcolors) are ADDED to what their
                                      buffers hold -- a later view of a mapping iteration, whose losses are summed before one
                                      backward (reference utils/slam_backend.py:180-306) -- instead of written; dL_dmeans2D
                                      and dL_dtau (per view) are written as always */
};

/* ---- sizes ---- */
size_t lvdgs_geom_bytes(int32_t num_gaussians);
size_t lvdgs_prepare_scratch_bytes(int32_t num_gaussians);
size_t lvdgs_binning_bytes(int64_t num_rendered);
size_t lvdgs_image_bytes(int32_t width, int32_t height);
size_t lvdgs_render_scratch_bytes(int32_t num_gaussians, int64_t num_rendered, int32_t width, int32_t height);
size_t lvdgs_backward_scratch_bytes(int32_t num_gaussians, int64_t num_rendered);

/* ---- rasterizer ---- */
/* Projects the Gaussians and counts (Gaussian, tile) pairs.  Writes radii and
 * geom_state; returns the pair count D in *num_rendered (synchronises the stream once).
 * D counts the (Gaussian, tile) pairs that are listed: the tiles of the reference's 3-sigma rectangle
 * (forward.cu's getRect) on which the Gaussian can reach alpha >= 1/255.  Pairs that cannot are dropped
 * (they contribute to no pixel; outputs are unchanged), so D <= the reference's num_rendered.  With
 * LVDGS_FLAG_LIST_ALL_TILES in a->flags every tile of the rectangle is listed and D equals it. */
int lvdgs_forward_prepare(const lvdgs_args *a, int64_t *num_rendered, void *stream);
/* Groups the pairs by tile, orders each tile's list by (depth, id) and composites front to back.
 * Writes out_color / out_depth / out_opacity / n_touched, binning_state and image_state. */
int lvdgs_forward_render(const lvdgs_args *a, void *stream);
/* Single-call forward without a pipeline bubble.  The caller sizes binning_state and scratch for
 * `pair_capacity` pairs (scratch >= max(lvdgs_prepare_scratch_bytes(N), lvdgs_render_scratch_bytes(N,cap,W,H)));
 * all kernels are enqueued with the pair count left on the device, and only then does the host wait
 * for the count (the GPU is busy with the tile sort and the blend meanwhile).  Returns LVDGS_OK and
 * the count in *num_rendered, or LVDGS_E_CAPACITY when the count exceeds pair_capacity: outputs are
 * then invalid, geom_state is valid, and the caller re-runs lvdgs_forward_render with
 * num_rendered = *num_rendered and buffers of that size.  Results are identical to the two-call form. */
int lvdgs_forward(const lvdgs_args *a, int64_t *num_rendered, void *stream);
/* Gradient of the three images w.r.t. every Gaussian parameter and the camera pose. */
int lvdgs_backward(const lvdgs_args *a, void *stream);
/* present[i] = Gaussian i is in front of the near plane of the view (GaussianRasterizer.markVisible). */
int lvdgs_mark_visible(int32_t num_gaussians, const float *means3D, const float *viewmatrix,
                       const float *projmatrix, uint8_t *present, void *stream);

/* ---- views into the state buffers (parity tests read intermediates through these) ---- */
typedef struct lvdgs_state_layout {
    /* byte offsets into geom_state */
    size_t geom_rec;           /* N x geom_rec_floats float: x, y, conic a, b, c, opacity, r, g, b, view depth,
                                  (unused), i32 radius, then (16-float records) the tile rectangle x0 | x1 << 16,
                                  y0 | y1 << 16 and the 64-bit mask of its tiles that are listed */
    size_t geom_tiles_touched; /* N x u32 */
    size_t geom_slot_base;     /* N x u32: exclusive scan of tiles_touched in id order (first pair of a Gaussian) */
    /* byte offsets into binning_state */
    /* (binning_state is laid out by its SIZE: these offsets hold for a buffer of exactly lvdgs_binning_bytes(num_rendered) bytes;
     *  point_list always starts the buffer) */
    size_t bin_point_list;     /* D x u32: Gaussian ids, (tile, depth, id) ordered */
    size_t bin_tile_keys;      /* D x u32: tile id of each entry of point_list -- written only on the radix
                                  path (images above 16384 tiles); otherwise derive it from img_ranges */
    /* byte offsets into image_state */
    size_t img_ranges;         /* T x 2 u32: [begin, end) of each tile in point_list */
    size_t img_final_T;        /* P x float */
    size_t img_n_contrib;      /* P x u32 */
    size_t geom_rec_floats;    /* floats per record of geom_rec (16) */
} lvdgs_state_layout;
int lvdgs_state_layout_query(int32_t num_gaussians, int64_t num_rendered, int32_t width, int32_t height,
                             lvdgs_state_layout *out);

/* ---- other native dependencies of the SLAM loop ---- */
/* mean squared distance of every point to its 3 nearest neighbours (simple_knn.distCUDA2). */
size_t lvdgs_knn_scratch_bytes(int32_t num_points);
int lvdgs_dist2_knn3(int32_t num_points, const float *points /* P*3 */, float *mean_dist2 /* P */,
                     void *scratch, size_t scratch_bytes, void *stream);
/* in-place 2-D rotary embedding of tokens (B, N, H, D) with integer positions (B, N, 2)
 * (croco curope.rope_2d): first half of D rotates by y, second half by x; fwd = +1 or -1. */
int lvdgs_rope2d(float *tokens, const int64_t *positions, int32_t B, int32_t N, int32_t H, int32_t D,
                 float base, float fwd, void *stream);
/* The same rotation for f32 / f16 / bf16 tokens addressed through element strides (D contiguous): element (b, n, h, d)
 * lives at tokens + b*stride_b + n*stride_n + h*stride_h + d.  croco calls curope on q / k in their (B, H, N, D)
 * attention layout, i.e. stride_h = N*D, stride_n = D, under autocast in half precision; arithmetic is f32 and each
 * element is rounded once when stored.  `dtype` is one of the LVDGS_F32 / LVDGS_F16 / LVDGS_BF16 codes. */
enum { LVDGS_F32 = 0, LVDGS_F16 = 1, LVDGS_BF16 = 2 };
int lvdgs_rope2d_strided(void *tokens, int32_t dtype, const int64_t *positions, int32_t B, int32_t N, int32_t H, int32_t D,
                         int64_t stride_b, int64_t stride_n, int64_t stride_h, float base, float fwd, void *stream);
/* Multi-scale deformable attention (Deformable-DETR; GroundingDINO's groundingdino._C.ms_deform_attn_forward / _backward,
 * reference GroundingDINO-main/groundingdino/models/GroundingDINO/ms_deform_attn.py:53, :80), float32.  For level l of
 * size (h, w): x = loc_x * w - 0.5, y = loc_y * h - 0.5; a sample takes part only if y > -1 && x > -1 && y < h && x < w, each
 * of its four corners only if it lies inside the level, and
 *     out[b, q, h, :] = sum_{l, p} weight * sum_corners bilinear * value[b, start_l + yy * w + xx, h, :].
 * spatial_shapes and level_start are DEVICE memory and are read on the device; no call waits for the host.  A corner is read
 * (or, in the backward, added to) only if its flattened index is below S, and NaN, infinite or huge locations take no part:
 * shapes that do not add up to S give wrong numbers, never an access outside the tensors.  B * Q == 0 or S == 0: LVDGS_OK,
 * nothing launched (S == 0: the outputs are zero-filled).  The forward and the location / weight gradients are bitwise
 * reproducible; grad_value is summed by float atomics and may differ in its last bits from run to run. */
int lvdgs_ms_deform_attn_forward(const float *value,            /* (B, S, H, D) */
                                 const int64_t *spatial_shapes, /* (L, 2) = (h, w), device */
                                 const int64_t *level_start,    /* (L), device */
                                 const float *sampling_loc,     /* (B, Q, H, L, P, 2) = (x, y) in [0, 1] */
                                 const float *attn_weight,      /* (B, Q, H, L, P) */
                                 int32_t B, int32_t S, int32_t H, int32_t D, int32_t Q, int32_t L, int32_t P,
                                 float *out,                    /* (B, Q, H * D) */
                                 void *stream);
int lvdgs_ms_deform_attn_backward(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                  const float *sampling_loc, const float *attn_weight,
                                  int32_t B, int32_t S, int32_t H, int32_t D, int32_t Q, int32_t L, int32_t P,
                                  const float *grad_out,        /* (B, Q, H * D) */
                                  float *grad_value,            /* (B, S, H, D), zeroed by the call */
                                  float *grad_sampling_loc,     /* (B, Q, H, L, P, 2) */
                                  float *grad_attn_weight,      /* (B, Q, H, L, P) */
                                  void *stream);

/* ---- fused photometric losses (reference utils/slam_utils.py:42-121) ---- */
/*   loss = weight_rgb   * mean_{c,p} [ omega_p * |(e^a I_cp + b) m_p - G_cp m_p| ]
 *        + weight_depth * mean_p     [ |D_p k_p - Z_p k_p| ]
 *   m_p = (sum_c G_cp > rgb_boundary_threshold) [* grad_mask_p],  omega_p = opacity_p if weight_by_opacity else 1,
 *   k_p = (Z_p > 0.01) [* (opacity_p > 0.95) if depth_needs_opaque].
 * get_loss_tracking_rgb  (slam_utils.py:53-62):  weight_rgb 1, weight_by_opacity 1, grad_mask, no depth term;
 * get_loss_tracking_rgbd (:65-79):  weight_rgb alpha, weight_depth 1-alpha, depth_needs_opaque 1;
 * get_loss_mapping_rgb   (:95-104): weight_rgb 1;   get_loss_mapping_rgbd (:107-121): alpha, 1-alpha. */
typedef struct lvdgs_loss_args {
    int32_t width, height;
    const float *image;        /* 3*H*W rendered colour                       */
    const float *depth;        /* H*W rendered depth or NULL                  */
    const float *opacity;      /* H*W rendered opacity or NULL                */
    const float *gt_image;     /* 3*H*W                                       */
    const float *gt_depth;     /* H*W or NULL (no depth term)                 */
    const uint8_t *grad_mask;  /* H*W bytes (0 / non-0) or NULL               */
    const float *exposure_a;   /* 1 or NULL (no exposure correction)          */
    const float *exposure_b;   /* 1 or NULL                                   */
    float rgb_boundary_threshold, weight_rgb, weight_depth;
    int32_t weight_by_opacity, depth_needs_opaque;
    void *scratch; size_t scratch_bytes;   /* lvdgs_loss_scratch_bytes(W,H)   */
    float *loss;               /* forward out: 1                              */
    const float *grad_loss;    /* backward in: 1 (d objective / d loss)       */
    float *d_image;            /* backward out: 3*H*W                         */
    float *d_depth;            /* H*W or NULL                                 */
    float *d_opacity;          /* H*W or NULL                                 */
    float *d_exposure_a;       /* 1 or NULL                                   */
    float *d_exposure_b;       /* 1 or NULL                                   */
} lvdgs_loss_args;
size_t lvdgs_loss_scratch_bytes(int32_t width, int32_t height);
int lvdgs_photometric_loss_forward(const lvdgs_loss_args *a, void *stream);
int lvdgs_photometric_loss_backward(const lvdgs_loss_args *a, void *stream);
/* Value and every gradient in ONE pass over the images (for callers whose objective is this loss, so that
 * d objective / d loss is known up front): grad_loss may be NULL (= 1) or a device scalar.  Same results as the two
 * calls above. */
int lvdgs_photometric_loss_value_and_grad(const lvdgs_loss_args *a, void *stream);
/* The same pass WITHOUT the final reduction: d_image / d_depth / d_opacity are written, the per-workgroup partial sums
 * of the loss value and of the exposure gradients stay in `scratch` for lvdgs_tracking_tail (`loss`, `d_exposure_a/b`
 * are not written yet).  One launch. */
int lvdgs_photometric_loss_partials(const lvdgs_loss_args *a, void *stream);

/* ---- per-frame pose optimiser step (reference utils/slam_frontend.py:1518-1521, utils/pose_utils.py:70-87) ----
 * One launch = `pose_optimizer.step()` (torch.optim.Adam: betas, eps, one learning rate per group) on the frame's
 * cam_rot_delta, cam_trans_delta, exposure_a, exposure_b, then `update_pose`: T_w2c <- SE3_exp([trans, rot]) @ [R T],
 * deltas zeroed, and the matrices the next render reads (Camera.world_view_transform / full_proj_transform /
 * camera_center, utils/camera_utils.py:106-120).  `state` = 24 floats owned by the caller and zeroed before the first
 * step of a frame: [0..15] Adam's (exp_avg, exp_avg_sq) of the 8 scalars (rot xyz, trans xyz, exposure a, b), [16] calls
 * applied, [17] a STICKY converged flag (||tau|| < converged_threshold at some step), [18] the number of steps applied,
 * [19..22] the Adam step count of the rot / trans / exposure_a / exposure_b group (a group whose gradient pointer is NULL in
 * a call is skipped, moments and count, as torch.optim.Adam skips parameters without .grad).  Once the flag is set further
 * calls change nothing, so the host may enqueue iterations ahead and read the flag late. */
typedef struct lvdgs_pose_step_args {
    float *R;                      /* 9, row-major world-to-camera rotation (in / out)                */
    float *T;                      /* 3 (in / out)                                                    */
    float *cam_rot_delta;          /* 3 parameter values (in / out: stepped, consumed, zeroed)        */
    float *cam_trans_delta;        /* 3                                                               */
    float *exposure_a;             /* 1 or NULL                                                       */
    float *exposure_b;             /* 1 or NULL                                                       */
    const float *grad_tau;         /* 6: dL/d(trans, rot), as lvdgs_backward writes dL_dtau; NULL = 0 */
    const float *grad_exposure_a;  /* 1 or NULL                                                       */
    const float *grad_exposure_b;  /* 1 or NULL                                                       */
    float *state;                  /* 24 floats, see above                                            */
    double lr_rot, lr_trans, lr_exposure, beta1, beta2, eps;  /* doubles, like the Python floats torch.optim.Adam computes with */
    float converged_threshold;
    const float *projmatrix_raw;   /* 16: the camera's projection_matrix (row-vector layout) or NULL  */
    float *viewmatrix;             /* out 16 or NULL                                                  */
    float *projmatrix;             /* out 16 or NULL: viewmatrix @ projmatrix_raw                     */
    float *campos;                 /* out 3 or NULL                                                   */
    /* The mapping loop's keyframes (utils/slam_backend.py:381-389) hold their gradients in separate tensors and may
     * lack some: when grad_tau is NULL these are read instead, and a parameter whose gradient pointer is NULL is left
     * untouched, moments included -- torch.optim.Adam skips parameters without a gradient.  R == NULL (with T NULL)
     * steps the exposure only (keyframes outside the pose window).  converged_threshold < 0 never raises the flag. */
    const float *grad_rot;         /* 3 or NULL */
    const float *grad_trans;       /* 3 or NULL */
    /* Optional: 2 floats of pinned host memory as the DEVICE addresses them (lvdgs_host_device_pointer), zeroed by the caller
     * before a frame's first step.  Every step stores state[18] (steps applied) to [1] and, when it raises the converged flag,
     * 1 to [0]: the host watches the optimisation without enqueuing a device-to-host copy per iteration (on this stack such a
     * copy is a blit kernel of its own). */
    float *host_flags;
} lvdgs_pose_step_args;
int lvdgs_pose_step(const lvdgs_pose_step_args *a, void *stream);
/* The address under which the device sees `host` (page-locked, mapped host memory, e.g. a pinned PyTorch tensor); fails with
 * LVDGS_E_HIP when the memory is not mapped into the device's address space. */
int lvdgs_host_device_pointer(void *host, void **device);
/* `count` independent steps (distinct cameras: the keyframes of a mapping window) in one launch instead of `count`. */
int lvdgs_pose_step_batch(const lvdgs_pose_step_args *steps, int32_t count, void *stream);

/* lvdgs_backward with the photometric loss evaluated INSIDE the backward blend pass: every pixel's dL/d(colour, depth,
 * opacity) is computed from `loss` (the formulas and parameters of lvdgs_photometric_loss_value_and_grad; d objective /
 * d loss = *grad_loss, or 1 when NULL) as the pass reads its pixels -- no gradient images are written or read, and there
 * is no separate pass over the frame (at 1080p: one launch and ~80 MB of traffic less per iteration).  a->dL_dout_* and
 * loss->d_image / d_depth / d_opacity are ignored; the opacity image's gradient feeds the blend iff
 * propagate_opacity_grad.  The loss's four partial sums are left per TILE in loss->scratch
 * (lvdgs_loss_scratch_bytes covers that layout too) for lvdgs_tracking_tail(..., partials_per_tile = 1), which writes
 * loss->loss and loss->d_exposure_a / _b.  An empty map or a view that lists no pair (num_gaussians or num_rendered == 0) is
 * fine: the loss of the background image is evaluated, every Gaussian / pose gradient is zero. */
int lvdgs_backward_fused_loss(const lvdgs_args *a, const lvdgs_loss_args *loss, int32_t propagate_opacity_grad, void *stream);

/* lvdgs_forward followed by lvdgs_backward_fused_loss as ONE call (a view whose loss is the photometric one: the tracking iteration,
 * utils/slam_frontend.py:1492-1517; a mapping view without a static mask).  Same arguments as the two calls (a->pair_capacity sizes
 * binning_state; scratch >= max of the three scratch sizes AT the capacity: lvdgs_backward_scratch_bytes(N, pair_capacity)), same results,
 * bit for bit.  What it buys: on frames of up to 4096 tiles the forward and the backward blend pass of a tile run in one launch -- the
 * loss's gradient at a pixel depends on that pixel alone, so a tile's backward needs nothing but the tile's own forward -- and a frame
 * of KITTI's size, on which each blend kernel lasts as long as its few heaviest tiles while the chip runs dry, pays that tail once
 * (KITTI geometry, pose-only: 0.209 -> 0.19 ms per tracking iteration).  Larger frames: the two calls in turn.  Returns LVDGS_OK and
 * the pair count, or LVDGS_E_CAPACITY (geom_state valid, everything else invalid): the caller grows binning_state / scratch and calls
 * lvdgs_forward_render, then lvdgs_backward_fused_loss.  The per-tile partial sums of the loss and the pose-gradient partials are left
 * for lvdgs_tracking_tail / lvdgs_map_view_tail as by lvdgs_backward_fused_loss (with a->dL_dtau == NULL). */
int lvdgs_forward_backward_fused_loss(const lvdgs_args *a, const lvdgs_loss_args *loss, int32_t propagate_opacity_grad, int64_t *num_rendered,
                                      void *stream);

/* The blend passes of `count` views in one launch each (no counterpart upstream, which renders a mapping window's keyframes one
 * after the other: utils/slam_backend.py:175-266).  A frame of KITTI's size (1848 tiles) leaves a 256-CU chip's wave slots half
 * empty and ends in a tail of its heaviest tiles; the ten views of a mapping window together fill it (per view: forward blend
 * 54 -> 34 us, backward 105 -> 77).  views[k]: the argument block of a view that has been through lvdgs_forward /
 * lvdgs_forward_render (resp. is about to go through lvdgs_backward_fused_loss) with LVDGS_FLAG_NO_BLEND -- the same
 * block, every buffer its own; all views the same image size and band of tile rows, losses[k] as for
 * lvdgs_backward_fused_loss.  Each view's outputs are what its single call without the flag writes, bit for bit. */
int lvdgs_blend_forward_batch(const lvdgs_args *const *views, int32_t count, void *stream);
/* lvdgs_forward for `count` views of ONE map (the same Gaussian tensors, the same num_gaussians / activations) and ONE image size,
 * every stage of all views in one launch: projection + counting, the two scans, the scatter, the per-tile depth sort and (unless
 * LVDGS_FLAG_NO_BLEND is set in the views' flags) the forward blend -- 6 launches for a mapping window's ten views instead of 50
 * (upstream renders them one after the other, utils/slam_backend.py:180-184; at KITTI's frame size the five stages before the blend are
 * latency-bound launches of 6-16 us each, half a millisecond per window).  Every view brings its own argument block with buffers of its
 * own, sized for its own pair_capacity as for lvdgs_forward; images of at most 16384 tiles.  The host waits once, with everything
 * enqueued, for all the pair counts: num_rendered[k] = view k's.  Returns LVDGS_OK, or LVDGS_E_CAPACITY when some view's count exceeds
 * its capacity -- THAT view's outputs are invalid (its geom_state is valid) and the caller re-runs lvdgs_forward_render for it with
 * buffers of num_rendered[k] pairs; the other views are complete.  Each view's state and outputs are lvdgs_forward's, bit for bit. */
int lvdgs_forward_batch(const lvdgs_args *const *views, int32_t count, int64_t *num_rendered, void *stream);
int lvdgs_blend_backward_fused_loss_batch(const lvdgs_args *const *views, const lvdgs_loss_args *const *losses, int32_t count,
                                          int32_t propagate_opacity_grad, void *stream);

/* The end of a tracking iteration in ONE launch (instead of three at ~6 us each on the iteration's critical path):
 *   - finishes the loss: sums the partial sums lvdgs_photometric_loss_partials(loss) left per 1024 pixels
 *     (partials_per_tile = 0) or lvdgs_backward_fused_loss left per tile (1), writes loss->loss, loss->d_exposure_a / _b;
 *   - reduces the pose-gradient partials lvdgs_backward(bwd) / lvdgs_backward_fused_loss(bwd, ...) left in bwd->scratch
 *     when called with bwd->dL_dtau == NULL (same `bwd` block, untouched in between: num_gaussians, num_rendered,
 *     scratch) and writes dL_dtau (6 floats);
 *   - applies lvdgs_pose_step(pose) with those gradients (pose->grad_* are ignored: the pose deltas take dL_dtau, the
 *     exposure parameters that `pose` names take loss->d_exposure_a / _b).  pose == NULL: the two reductions only (a
 *     view of the mapping iteration, whose keyframe is stepped after all views).
 * Same additions in the same order as the separate launches: bit-identical results. */
int lvdgs_tracking_tail(const lvdgs_loss_args *loss, const lvdgs_args *bwd, const lvdgs_pose_step_args *pose, float *dL_dtau,
                        int32_t partials_per_tile, void *stream);

/* The end of one VIEW of the mapping iteration in one launch: lvdgs_tracking_tail(loss, bwd, NULL, dL_dtau, 1, ...) -- the
 * view's loss value, exposure gradients and pose gradient from the partial sums lvdgs_backward_fused_loss left -- and
 * lvdgs_view_stats on the view's outputs (bwd->radii, bwd->n_touched, bwd->dL_dmeans2D; see lvdgs_view_stats below for the
 * meaning of the fields, any of vis_count / touched_row / split_xy may be NULL).  loss == NULL: a view scored by
 * lvdgs_masked_loss_batch, whose loss value is finished already -- the pose gradient and the statistics only. */
typedef struct lvdgs_view_stats_args {
    int32_t *radii_max;   /* N   */
    float *norm_sum;      /* N   */
    float *vis_count;     /* N or NULL */
    uint8_t *touched_row; /* N or NULL */
    float *split_xy;      /* N*2 or NULL */
} lvdgs_view_stats_args;
int lvdgs_map_view_tail(const lvdgs_loss_args *loss, const lvdgs_args *bwd, float *dL_dtau, const lvdgs_view_stats_args *stats, void *stream);
/* lvdgs_map_view_tail for `count` views in ONE launch (a mapping window whose views were rendered and differentiated together:
 * lvdgs_forward_batch ... ): losses[k] may be NULL as above (losses itself too: no view has a loss block), stats[k] is required.  The
 * statistics are taken per Gaussian over the views IN ORDER: radii_max / norm_sum / vis_count receive what `count` single calls in
 * that order give them, bit for bit. */
int lvdgs_map_view_tail_batch(const lvdgs_loss_args *const *losses, const lvdgs_args *const *bwds, float *const *dL_dtau,
                              const lvdgs_view_stats_args *const *stats, int32_t count, void *stream);

/* ---- Adam step of the Gaussian map (reference utils/slam_backend.py:144, :378, :458: gaussians.optimizer.step()) ----
 * All parameter tensors in one launch, one pass over (grad, exp_avg, exp_avg_sq, param); torch.optim.Adam's arithmetic
 * (no weight decay, no amsgrad), `step` = that tensor's step count INCLUDING this step (bias corrections). */
#define LVDGS_ADAM_MAX_TENSORS 8
typedef struct lvdgs_adam_tensor {
    float *param; const float *grad; float *exp_avg; float *exp_avg_sq;
    int64_t numel; int64_t step; double lr;
} lvdgs_adam_tensor;
int lvdgs_adam_step(const lvdgs_adam_tensor *tensors, int32_t count, double beta1, double beta2, double eps, void *stream);

/* Isotropic regulariser of the mapping loss (reference utils/slam_backend.py:303-305):
 *   loss = weight * mean_{i,k} | s_ik - mean_k s_ik |,  s = exp(raw_scales)   (the model's scaling activation)
 * writes the value to *loss and ADDS its gradient w.r.t. the raw (log) scales to grad_raw_scales (NULL: value only). */
size_t lvdgs_isotropic_scratch_bytes(int32_t num_gaussians);
int lvdgs_isotropic_reg(int32_t num_gaussians, const float *raw_scales /* N*3 */, float *grad_raw_scales /* N*3 or NULL */,
                        float weight, void *scratch, size_t scratch_bytes, float *loss, void *stream);
/* What the back end derives from one view's render package (utils/slam_backend.py:311-315, :350-357), accumulated over
 * the views rendered so far: radii_max = max(radii_max, radii); for visible Gaussians (radii > 0) norm_sum += |viewspace
 * gradient xy| and vis_count += 1 (NULL: not counted); touched_row[i] = n_touched[i] > 0 (NULL for views outside the window).
 * A view rendered in bands by several GPUs (lvdgs_args.tile_row_*) holds only a share of the gradient on each: pass
 * split_xy (N x 2) and the band's xy is written THERE instead of its norm being added to norm_sum -- the caller sums the
 * bands (all-reduce) and lvdgs_map_stats_apply takes the norm of the sum; vis_count then goes with ONE of the bands. */
int lvdgs_view_stats(int32_t num_gaussians, const int32_t *radii, const int32_t *n_touched, const float *viewspace_grad /* N*3 or NULL */,
                     int32_t *radii_max, float *norm_sum, float *vis_count, uint8_t *touched_row, float *split_xy, void *stream);
/* ... and their way into the model, one launch (:350-357 on the reduced values):
 *   max_radii2D = max(max_radii2D, radii_max); xyz_gradient_accum += norm_sum + sum_k |split_xy[k]|; denom += vis_count
 * split_xy: n_split planes of N x 2 floats (the summed band gradients of the views that were split), or NULL with 0. */
int lvdgs_map_stats_apply(int32_t num_gaussians, const int32_t *radii_max, const float *norm_sum, const float *vis_count,
                          const float *split_xy, int32_t n_split, float *max_radii2D, float *xyz_gradient_accum, float *denom, void *stream);

/* ---- depth term of the static-mask mapping loss (reference utils/slam_backend.py:216-261) ----
 *   M    = static_mask & (mono_depth > 0) & (rendered depth > 0)          (static_mask NULL = every pixel)
 *   loss = depth_lambda-free mean over M of |D_p - Z_p|;  0 when M is empty (the reference then adds nothing)
 * The mean is over |M|, not over the image (that is what distinguishes it from lvdgs_loss_args' depth term).
 * forward writes out[0] = loss, out[1] = |M|; backward reads out[1] back and writes
 *   d_depth_p = grad_loss * sign(D_p - Z_p) / |M| on M, 0 elsewhere. */
typedef struct lvdgs_masked_depth_args {
    int32_t width, height;
    const float *depth;          /* H*W rendered depth                           */
    const float *gt_depth;       /* H*W mono depth                               */
    const uint8_t *static_mask;  /* H*W bytes (non-0 = static) or NULL           */
    void *scratch; size_t scratch_bytes;   /* lvdgs_masked_depth_scratch_bytes(W,H); forward only */
    float *out;                  /* 2 floats: loss, |M|  (forward writes, backward reads [1]) */
    const float *grad_loss;      /* backward in: 1                               */
    float *d_depth;              /* backward out: H*W                            */
} lvdgs_masked_depth_args;
size_t lvdgs_masked_depth_scratch_bytes(int32_t width, int32_t height);
int lvdgs_masked_depth_l1_forward(const lvdgs_masked_depth_args *a, void *stream);
int lvdgs_masked_depth_l1_backward(const lvdgs_masked_depth_args *a, void *stream);

/* ---- fused L1 + SSIM image loss (reference utils/slam_backend.py:199-215, 438-454) ----
 * The mapping and colour-refinement losses `(1 - lambda) * l1_loss(a, b) + lambda * (1 - ssim(a, b))` call
 * gaussian_splatting.utils.loss_utils.l1_loss / ssim (package absent from the checkout; 11-tap Gaussian window,
 * sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over pixels and channels).  One launch computes both
 * means and, when d_img1 is given, the combined gradient
 *     d_img1 = weight_l1 * d mean|a - b| / d a + weight_ssim * d mean SSIM(a, b) / d a.
 * With keep_mask, pixels whose mask byte is 0 are first replaced by bg[plane % channels] in BOTH images
 * (slam_backend.py:205-209); they receive zero gradient. */
typedef struct lvdgs_ssim_args {
    int32_t width, height;
    int32_t planes;            /* batch * channels image planes of H*W floats  */
    int32_t channels;          /* planes per image (bg index = plane % channels) */
    const float *img1;         /* planes*H*W (the differentiated image)        */
    const float *img2;         /* planes*H*W                                   */
    const uint8_t *keep_mask;  /* H*W bytes or NULL                            */
    const float *bg;           /* channels floats or NULL (0)                  */
    float weight_l1, weight_ssim;
    void *scratch; size_t scratch_bytes;   /* lvdgs_ssim_scratch_bytes(W,H,planes) */
    float *out;                /* 2: mean |a - b|, mean SSIM                   */
    float *d_img1;             /* planes*H*W or NULL (values only)             */
} lvdgs_ssim_args;
size_t lvdgs_ssim_scratch_bytes(int32_t width, int32_t height, int32_t planes);
int lvdgs_ssim_l1(const lvdgs_ssim_args *a, void *stream);

/* ---- the static-mask mapping loss as ONE object (reference utils/slam_backend.py:196-261; colour refinement :420-454) ----
 * LVD-GS's front end attaches a static_mask to every tracked frame and keyframe (utils/slam_frontend.py:1218,1309-1329,1429-1433:
 * dynamic_filtering.enabled defaults to True), so this -- not get_loss_mapping -- is the loss of every window keyframe of
 * BackEnd.map:
 *     loss = (1 - lambda) * mean|a - b| + lambda * (1 - mean SSIM(a, b)) + depth_lambda * mean_{p in M} |D_p - Z_p|
 *     a, b = rendered / target colour with bg[c] written under the dynamic pixels (static_mask byte 0) of both,
 *     M    = static_mask & (Z > 0) & (D > 0)     (no depth term when gt_depth is NULL, or M is empty)
 * lvdgs_masked_loss_batch evaluates it for `count` views of one size in TWO launches whatever the count: the fused L1 + SSIM
 * kernel over every plane of every view (it also takes the depth term's sum and exact pixel count per 32x32 tile), and a
 * finish (one workgroup per view).  Per view it writes d_image = d loss / d a (the SSIM gradient is not local, so it is an
 * image) and out[0..4] = loss, mean|a - b|, mean SSIM, depth term, |M|.  The depth term's gradient is NOT written anywhere:
 * lvdgs_backward_masked_loss / lvdgs_blend_backward_window_batch evaluate depth_lambda * sign(D - Z) / |M| per pixel from
 * depth / gt_depth / static_mask and out[4] as the backward blend pass reads its pixels.  Same numbers as lvdgs_ssim_l1 +
 * lvdgs_masked_depth_l1_forward / _backward + lvdgs_backward on their gradient images (d_image, d_depth: the same bits). */
typedef struct lvdgs_masked_loss_args {
    int32_t width, height;
    const float *image;          /* 3*H*W rendered colour                               */
    const float *gt_image;       /* 3*H*W                                               */
    const uint8_t *static_mask;  /* H*W bytes (non-0 = static) or NULL (every pixel)    */
    const float *bg;             /* 3 or NULL (0): colour written under the mask        */
    const float *depth;          /* H*W rendered depth, or NULL                         */
    const float *gt_depth;       /* H*W mono depth, or NULL: no depth term              */
    float lambda_dssim, depth_lambda;
    void *scratch; size_t scratch_bytes;   /* lvdgs_masked_loss_scratch_bytes(W,H)      */
    float *d_image;              /* out: 3*H*W                                          */
    float *out;                  /* out: 8 floats, [0..4] as above                      */
} lvdgs_masked_loss_args;
size_t lvdgs_masked_loss_scratch_bytes(int32_t width, int32_t height);
int lvdgs_masked_loss_batch(const lvdgs_masked_loss_args *const *views, int32_t count, void *stream);
/* lvdgs_backward for a view scored by lvdgs_masked_loss_batch: the backward blend pass reads loss->d_image and evaluates the
 * depth term's gradient itself (a->dL_dout_* are ignored, the opacity image gets no gradient), then the per-Gaussian pass.
 * With LVDGS_FLAG_NO_BLEND it starts behind the blend pass (lvdgs_blend_backward_window_batch has run it). */
int lvdgs_backward_masked_loss(const lvdgs_args *a, const lvdgs_masked_loss_args *loss, void *stream);
/* The backward blend passes of a mapping window in one launch, every view with the loss it is scored by: view k takes
 * masked[k] when that is non-NULL (a keyframe with a static mask, as lvdgs_backward_masked_loss) and losses[k] otherwise (the
 * two random older views, keyframes without a mask: as lvdgs_blend_backward_fused_loss_batch).  `masked` may be NULL (no view
 * is masked); `losses` may be NULL when every view is masked.  Each view's records are its single call's, bit for bit. */
int lvdgs_blend_backward_window_batch(const lvdgs_args *const *views, const lvdgs_loss_args *const *losses,
                                      const lvdgs_masked_loss_args *const *masked, int32_t count, int32_t propagate_opacity_grad,
                                      void *stream);

/* The per-Gaussian passes (what lvdgs_backward_fused_loss / lvdgs_backward_masked_loss do with LVDGS_FLAG_NO_BLEND) of `count`
 * views of one map in ONE launch, behind lvdgs_blend_backward_window_batch.  The views share the map and the gradient buffers
 * (views[0]'s LVDGS_FLAG_ACCUMULATE_PARAM_GRADS says whether the sums are added to what those hold; the later views carry the
 * flag); a thread walks its Gaussian through the views in order with the parameter gradients in registers and writes them once,
 * where the view-after-view calls read and write them per view -- the same additions in the same order, the same bits.
 * Every view keeps its own dL_dmeans2D and pose-gradient partials (dL_dtau NULL: left in its scratch for lvdgs_map_view_tail*).
 * For SH colours of one coefficient (sh_degree 0, sh_coeffs 1) with scales + rotations; LVDGS_E_INVALID otherwise.
 * Replaces: the reference's per-view loss.backward() accumulation into .grad (utils/slam_backend.py:262-306). */
int lvdgs_gaussian_backward_batch(const lvdgs_args *const *views, int32_t count, void *stream);

/* ---- patch-based scale alignment of a keyframe's mono depth (LVD-GS Algorithm 1: reference utils/depth_utils.py process_depth,
 * called for every keyframe after the first, utils/slam_frontend.py:1380-1405) ----
 * r = render_depth, m = mono_depth (H x W).  Patches tile the image from (0, 0) in steps of patch_size, edge patches clipped.
 * Iteration k = 0 .. max_iter-1 with the current scale s (1 at the start), ms = float32(m * s):
 *   top:  stop if |s - s_prev| < epsilon (float32) and s != 1; s_prev = s;
 *   a patch PASSES when |mean r - mean ms| < mean_threshold * mean ms and |std r - std ms| < std_threshold * std ms (population
 *   statistics, float64); in a passing patch a pixel is ACCURATE when
 *   |(r - mean r) / (std r + 1e-6) - (ms - mean ms) / (std ms + 1e-6)| < error_threshold (NaN: never);
 *   count < min (= int(min_accurate_pixels_ratio * H * W)) and k == 2 or k == 3: num_accurate = count, the caller's SCALE REMEDY
 *   gives the next s (k == 2: continue with k = 3; k == 3: stop);
 *   else num_accurate = 0, and if count > 0 and (k < 2 or count >= min): s = mean r[acc] / mean m[acc] (UNSCALED m), num_accurate = count.
 * Fill (float32, as NumPy): ms = m * s; error = |r - ms| / (ms + 1e-8) > final_error_threshold or r == 0; final = error ? ms : r.
 * lvdgs_depth_align enqueues max_iter iteration launches and the fill (an iteration whose state is not RUNNING stands down); no host
 * wait.  Every launch that changes the state copies it to host_state (a host block without a tag: "Host blocks" above;
 * LVDGS_DEPTH_ALIGN_STATE_WORDS int32 words: [0] s (float bits), [1] s_prev (float bits), [2] status, [3] k of the last iteration run, [4] num_accurate,
 * [5] passing patches of the last iteration run, [6] accurate pixels of the last iteration run, [7] 1 once the fill has run).  The
 * caller synchronises the stream once and reads it.  status LVDGS_DEPTH_ALIGN_REMEDY (final_depth / error_mask not written): the
 * caller evaluates the remedy and calls lvdgs_depth_align_resume with its scale, which enqueues iteration 3 and the fill (remedy at
 * k == 2) or the fill alone (k == 3), reading k from host_state, and synchronises again.  scratch: lvdgs_depth_align_scratch_bytes(W, H, patch_size) bytes,
 * ZERO-FILLED before its first use (every call leaves it so).  Bit-deterministic: the sums are taken in a fixed order.
 * LVDGS_E_INVALID: bad sizes, patch_size outside 1..LVDGS_DEPTH_ALIGN_MAX_PATCH, max_iter < 0, a NULL pointer, scratch too small. */
#define LVDGS_DEPTH_ALIGN_MAX_PATCH 64
#define LVDGS_DEPTH_ALIGN_STATE_WORDS 8
enum {
    LVDGS_DEPTH_ALIGN_RUNNING = 0,
    LVDGS_DEPTH_ALIGN_CONVERGED = 1,  /* the top-of-iteration test stopped the loop */
    LVDGS_DEPTH_ALIGN_EXHAUSTED = 2,  /* max_iter iterations ran (or the remedy at k == 3 ended them) */
    LVDGS_DEPTH_ALIGN_REMEDY = 3      /* too few accurate pixels at k == 2 or 3: the caller's remedy is due */
};
typedef struct lvdgs_depth_align_args {
    int32_t width, height, patch_size, max_iter;
    double mean_threshold, std_threshold, error_threshold, final_error_threshold, epsilon, min_accurate_pixels_ratio;
    const float *render_depth;   /* H*W                                             */
    const float *mono_depth;     /* H*W                                             */
    float *final_depth;          /* out H*W                                         */
    uint8_t *error_mask;         /* out H*W bytes (0 / 1)                           */
    int32_t *host_state;         /* LVDGS_DEPTH_ALIGN_STATE_WORDS, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_depth_align_args;
size_t lvdgs_depth_align_scratch_bytes(int32_t width, int32_t height, int32_t patch_size);
int lvdgs_depth_align(const lvdgs_depth_align_args *a, void *stream);
int lvdgs_depth_align_resume(const lvdgs_depth_align_args *a, float scale, void *stream);

/* ---- pose initialisation by PnP-RANSAC on the rendered depth (reference utils/init_pose.py get_pose :160-175: cv2.undistortPoints +
 * depth_to_3d + cv2.solvePnPRansac, called for every tracked frame, utils/slam_frontend.py:1448) ----
 * The unknown is the keyframe -> frame motion T = [R | t] (world = the keyframe's camera frame).  All arithmetic and every comparison
 * below is float64 from the float32 / int32 loads.
 * Gather.  Match i = (keyframe pixel (x, y) int32, frame pixel (u, v) float32) is VALID when 0 <= x < width, 0 <= y < height and
 *   Z = depth[y * width + x] is finite and > 0 (deviation: the reference back-projects zero depth to the origin and leaves it to RANSAC).
 *   Both pixels go to normalised coordinates by TEN fixed-point steps of the Brown model (cv2.undistortPoints' scheme, twice its
 *   default count): x0 = (u - cx) / fx, y0 = (v - cy) / fy, (x, y) = (x0, y0), then ten times r2 = x^2 + y^2,
 *   icd = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2), dx = 2 p1 x y + p2 (r2 + 2 x^2), dy = p1 (r2 + 2 y^2) + 2 p2 x y,
 *   (x, y) = ((x0 - dx) icd, (y0 - dy) icd).  Object point P = (x_n Z, y_n Z, Z); frame point q = (u_n, v_n).
 * Residual of a match under T: with (X, Y, Zc) = R P + t, r = (fx (X / Zc - u_n), fy (Y / Zc - v_n)) -- pixels of the undistorted image.
 *   It is an INLIER when it is valid, Zc > 0 and |r|^2 < reproj_error^2.
 * Gauss-Newton step on a set of matches: A = sum J^T J, g = sum J^T r with J = dr/dtau under the left perturbation T <- Exp(tau) T,
 *   tau = [rho; theta] (pose_utils.SE3_exp, series below 1e-5 rad); the diagonal of A is multiplied by 1 + 1e-3 (the damping);
 *   A tau = -g by Cholesky.  The step FAILS when a pivot is not > 0 or tau is not finite.
 * Hypotheses.  mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32).  Draw d of hypothesis h:
 *   mix32(mix32(mix32(seed ^ 0x9e3779b9) + h) + d) % num_matches.  Slot s = 0, 1, 2 takes the first of its draws d = 32 s .. 32 s + 31
 *   that is a valid match not taken by an earlier slot; a slot that finds none voids the hypothesis.  Eight steps on the three
 *   matches from the identity; void when a step fails or a sample point ends with Zc <= 0.  Score: the number of inliers.
 *   Winner: the highest score, ties to the lowest h.
 * Refinement.  Three rounds of: select the inliers under the current pose, five steps on them.  The inlier mask and count are taken
 *   under the final pose.  Sums over matches are taken in a fixed order: two calls give the same bits.
 * FAILED (the pose is the exact identity, the mask zero) with reason FEW_VALID (fewer than 6 valid matches), ALL_VOID, FEW_INLIERS
 *   (the winner's score < min_inliers) or SINGULAR (a refinement step fails).
 * Two launches, enqueued at once; no host wait.  host_state: a host block ("Host blocks" above) of LVDGS_PNP_HOST_BYTES bytes:
 * LVDGS_PNP_STATE_WORDS int32 words -- [0] status, the tag, [1] valid matches, [2] inliers under the final pose, [3] the winning
 * hypothesis (-1: none), [4] its score, [5] reason, [6] [7] zero -- then the pose as 12 doubles, row-major [R | t].  scratch: lvdgs_pnp_scratch_bytes(num_matches, hypotheses) bytes, no initialisation needed.
 * LVDGS_E_INVALID: args NULL, a NULL pointer, bad raster size, num_matches < 0, hypotheses outside 1..LVDGS_PNP_MAX_HYPOTHESES,
 * reproj_error / fx / fy not > 0, scratch too small. */
#define LVDGS_PNP_MAX_HYPOTHESES 4096
#define LVDGS_PNP_STATE_WORDS 8
#define LVDGS_PNP_HOST_BYTES 128
enum {
    LVDGS_PNP_OK = 1,
    LVDGS_PNP_FAILED = 2
};
enum {
    LVDGS_PNP_FAIL_NONE = 0,
    LVDGS_PNP_FAIL_FEW_VALID = 1,
    LVDGS_PNP_FAIL_ALL_VOID = 2,
    LVDGS_PNP_FAIL_FEW_INLIERS = 3,
    LVDGS_PNP_FAIL_SINGULAR = 4
};
typedef struct lvdgs_pnp_args {
    int32_t width, height;        /* the raster of depth (W1, H1)                   */
    int32_t num_matches, hypotheses, min_inliers;
    uint32_t seed;
    double fx, fy, cx, cy;        /* intrinsics at that raster                      */
    double dist[5];               /* k1 k2 p1 p2 k3 (all zero: no distortion)       */
    double reproj_error;          /* pixels                                         */
    const float *depth;           /* H1*W1                                          */
    const int32_t *matches_im1;   /* M*2 (x, y) in the keyframe's raster            */
    const float *matches_im2;     /* M*2 (u, v) in the frame                        */
    uint8_t *inlier_mask;         /* out M bytes (0 / 1)                            */
    int32_t *host_state;          /* LVDGS_PNP_HOST_BYTES, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_pnp_args;
size_t lvdgs_pnp_scratch_bytes(int32_t num_matches, int32_t hypotheses);
int lvdgs_pnp_ransac(const lvdgs_pnp_args *a, void *stream);

/* ---- matching two descriptor maps by reciprocal nearest neighbours (what the reference's get_pose calls first:
 * fast_reciprocal_NNs(desc1, desc2, subsample_or_initxy1=8, dist='dot') over MASt3R descriptors; the network itself is out of scope) ----
 * desc1: (height1, width1, dim), desc2: (height2, width2, dim), float32, contiguous.  The score of a pair is the float32 dot product,
 * summed in ascending component order by one fmaf chain from zero -- the same arithmetic for every row of a map, so bit-identical rows
 * score bit-identically.  Flat index of a pixel: x + width * y.  arg-max ties go to the LOWEST flat index.
 * Seeds.  The grid y = S/2, S/2 + S, ... < height1, x = S/2, S/2 + S, ... < width1 (S = subsample, integer division), row-major: seed
 *   k starts at xy1 = its flat index, xy2 = -1, old1 = xy1, old2 = -1, active.
 * One round, active seeds only: (1) xy2 <- argmax_j <desc1[xy1], desc2[j]>; (2) xy2 == old2: the seed becomes inactive;
 *   (3) still active: xy1 <- argmax_i <desc2[xy2], desc1[i]>; (4) xy1 == old1: inactive; (5) old2 <- xy2, old1 <- xy1.
 * Rounds run until no seed is active, at most max_iter of them.  A seed still active then is UNCONVERGED and dropped.  A seed's
 * trajectory depends on no other seed.
 * Output.  The distinct pairs (xy1, xy2) of the inactive seeds, ascending by xy1, then xy2, as pixels: matches_im1 (M, 2) int32 (x, y)
 *   in map 1, matches_im2 (M, 2) float32 (x, y) in map 2 -- what lvdgs_pnp_ransac takes.  Both need room for `capacity` >= seeds pairs.
 *   seed_state (optional, may be NULL): 3 int32 per seed -- its final xy1, xy2 and 1 (inactive: it contributed its pair) / 0 (unconverged).
 * Every index written lies inside its map whatever the descriptors hold; with non-finite descriptors the result is otherwise unspecified.
 * Two calls on the same inputs give the same bytes.
 * 2 + 4 max_iter launches, enqueued at once; no host wait (the active set lives on the device; a search launch without active seeds
 * does nothing).  host_state: a host block ("Host blocks" above) of LVDGS_RNN_STATE_WORDS int32 words: [0] status, the tag
 * (LVDGS_RNN_OK once the call has run), [1] seeds, [2] matches M, [3] unconverged seeds, [4] rounds that had an active seed, [5..7] zero.
 * scratch: lvdgs_recip_nn_scratch_bytes(...) bytes, no initialisation needed.
 * LVDGS_E_INVALID: args NULL, a NULL pointer, a size not > 0, a map of more than 2^31 - 1 floats, dim outside 1..LVDGS_RNN_MAX_DIM,
 * subsample < 1, max_iter < 1, more than LVDGS_RNN_MAX_SEEDS seeds, capacity below the seed count, scratch too small. */
#define LVDGS_RNN_MAX_DIM 64
#define LVDGS_RNN_MAX_SEEDS 8192
#define LVDGS_RNN_STATE_WORDS 8
enum {
    LVDGS_RNN_OK = 1
};
typedef struct lvdgs_recip_nn_args {
    int32_t width1, height1, width2, height2;
    int32_t dim, subsample, max_iter;
    int32_t capacity;             /* pairs matches_im1 / matches_im2 have room for (>= seeds) */
    const float *desc1;           /* height1*width1*dim                             */
    const float *desc2;           /* height2*width2*dim                             */
    int32_t *matches_im1;         /* out capacity*2 (x, y) in map 1                 */
    float *matches_im2;           /* out capacity*2 (x, y) in map 2                 */
    int32_t *seed_state;          /* out seeds*3 (xy1, xy2, converged), or NULL     */
    int32_t *host_state;          /* LVDGS_RNN_STATE_WORDS, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_recip_nn_args;
/* the scratch a call with this seed grid needs (0 when an argument is not > 0) */
size_t lvdgs_recip_nn_scratch_bytes(int32_t width1, int32_t height1, int32_t subsample);
int lvdgs_reciprocal_nn(const lvdgs_recip_nn_args *a, void *stream);

/* ---- the matcher's image formatting (reference utils/init_pose.py torch_images_to_dust3r_format :35-75, the first statement of
 * get_pose, get_depth and find_scale: a device-to-host copy, PIL's resize and crop, torchvision's normalisation, an upload) ----
 * image: (3, height, width) float32, contiguous.  out: (3, H1, W1) float32 with (W1, H1) the matcher's raster of size `size`.
 * Quantise.  q = uint8(trunc(float32(x) * 255.0f)); a product outside [0, 255] clamps and NaN gives 0 (deviation: NumPy wraps).
 * Resize to (w, h) = (round(W size / S), round(H size / S)), S = max(W, H), halves to even, by PIL's 8-bit resampling with the
 *   LANCZOS filter (sinc(x) sinc(x / 3) on [-3, 3), support 3) when S > size, else BICUBIC (Keys, a = -0.5, support 2): a horizontal
 *   pass to uint8, then a vertical pass to uint8; a pass whose edge does not change is skipped.  Output sample xx of a pass from `in`
 *   to `out` samples, float64: scale = in / out, fs = max(scale, 1), support = filter support * fs, center = (xx + 0.5) scale,
 *   xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in) - xmin,
 *   w[x] = filter((x + xmin - center + 0.5) * (1 / fs)), divided by their sum ww when ww != 0,
 *   k[x] = int(w[x] 2^22 + 0.5) for w[x] >= 0, int(w[x] 2^22 - 0.5) below; sample = clamp((2^21 + sum k[x] pixel[xmin + x]) >> 22, 0, 255)
 *   in int32.
 * Crop.  cx = w / 2, cy = h / 2 (integer division), halfw = ((2 cx) / 16) 8, halfh likewise, halfh = 3 halfw / 4 when w == h; the
 *   columns cx - halfw .. cx + halfw - 1 and the rows cy - halfh .. cy + halfh - 1: (W1, H1) = (2 halfw, 2 halfh).  Only these are
 *   computed, and the horizontal pass runs over the image rows the vertical pass reads.
 * Normalise.  (float32(q) / 255.0f - 0.5f) / 0.5f, IEEE float32.  quantised (optional, may be NULL): the cropped uint8 image,
 *   (H1, W1, 3), before the normalisation.
 * lvdgs_format_plan_query gives the sizes of a call; lvdgs_format_table makes the entries first .. first + count - 1 of a pass' table on
 * the HOST (no GPU involved): per entry 2 + taps int32 words -- xmin, n, then the n coefficients, zero-filled to `taps`
 * (plan.taps_x / taps_y; a skipped pass has one tap: xmin = xx, n = 1, k = 2^22).  The caller keeps the tables of an image size on the
 * device: table_x = entries crop_x .. crop_x + W1 - 1 of the pass width -> w, table_y = entries crop_y .. crop_y + H1 - 1 of the pass
 * height -> h.  A kernel reads no image or scratch element outside its buffers whatever a table holds.
 * lvdgs_format_image: two launches, enqueued at once; no host wait, no copy.  scratch: lvdgs_format_scratch_bytes(W, H, size) bytes
 * (0: the sizes are refused), no initialisation needed.  Two calls give the same bytes.
 * LVDGS_E_INVALID: args / plan / table NULL, a NULL pointer, an edge not in 1..LVDGS_FORMAT_MAX_EDGE, size 224 (the reference's other
 * crop rule, which it never uses) or outside 16..LVDGS_FORMAT_MAX_SIZE, an empty raster, an unknown filter, table entries outside the
 * pass, scratch too small. */
#define LVDGS_FORMAT_MAX_EDGE 16384
#define LVDGS_FORMAT_MAX_SIZE 4096
enum {
    LVDGS_FORMAT_BICUBIC = 0,
    LVDGS_FORMAT_LANCZOS = 1
};
typedef struct lvdgs_format_plan {
    int32_t resized_width, resized_height;   /* (w, h)                                */
    int32_t filter;                          /* LVDGS_FORMAT_LANCZOS / _BICUBIC       */
    int32_t crop_x, crop_y;                  /* the crop's first column and row in the resized image */
    int32_t out_width, out_height;           /* (W1, H1)                              */
    int32_t taps_x, taps_y;                  /* coefficient slots per table entry     */
    int32_t row_first, row_count;            /* the image rows the vertical pass reads */
} lvdgs_format_plan;
typedef struct lvdgs_format_image_args {
    int32_t width, height, size;
    const float *image;           /* 3*H*W                                          */
    const int32_t *table_x;       /* W1*(2 + taps_x), device                        */
    const int32_t *table_y;       /* H1*(2 + taps_y), device                        */
    float *out;                   /* out 3*H1*W1                                    */
    uint8_t *quantised;           /* out H1*W1*3, or NULL                           */
    void *scratch; size_t scratch_bytes;
} lvdgs_format_image_args;
int lvdgs_format_plan_query(int32_t width, int32_t height, int32_t size, lvdgs_format_plan *plan);
int lvdgs_format_table(int32_t in, int32_t out, int32_t filter, int32_t first, int32_t count, int32_t *table);
size_t lvdgs_format_scratch_bytes(int32_t width, int32_t height, int32_t size);
int lvdgs_format_image(const lvdgs_format_image_args *a, void *stream);

/* ---- the scale between two depth maps at matched pixels (reference utils/depth_utils.py find_scale :31-55: cv2.resize of both maps
 * to the matcher's raster on the host, a gather at the matches, a ratio of means -- the scale remedy of LVD-GS Algorithm 1) ----
 * Match i = (map-1 pixel (x, y) int32, map-2 pixel (u, v) float32, truncated toward zero) at the raster (raster_width, raster_height),
 * as lvdgs_reciprocal_nn writes them.  depth1: (height1, width1), depth2: (height2, width2), float32; the sizes may differ from each
 * other and from the raster.
 * Sampling.  A match takes depth1 at its map-1 pixel and depth2 at its map-2 pixel as if each map had been resized bilinearly to the
 *   raster.  Per axis, pixel i of n_dst from n_src samples: f = (i + 0.5) (n_src / n_dst) - 0.5, s = floor(f), t = f - s;
 *   s < 0: (s, t) = (0, 0); s >= n_src - 1: (s, t) = (n_src - 1, 0); the neighbour s + 1 is clamped to n_src - 1.  With a, b the
 *   samples of row sy at sx and its neighbour and c, d those of the next row:
 *   value = (1 - ty) ((1 - tx) a + tx b) + ty ((1 - tx) c + tx d).  All arithmetic is float64 from the float32 loads, as written.
 *   UNPINNED against cv2.resize(INTER_LINEAR), which interpolates in float32.
 * A match is VALID when 0 <= x < raster_width, 0 <= y < raster_height, -1 < u < raster_width, -1 < v < raster_height (NaN: not) and both
 *   values are finite and > 0 (deviations: the reference lets +inf through, and its out-of-raster indices wrap or raise).
 * scale = float32((sum1 / n) / (sum2 / n)) over the n valid matches, the sums in float64 in a fixed order: two calls give the same bits.
 * One launch; no host wait.  host_state: a host block ("Host blocks" above) of LVDGS_MATCH_SCALE_HOST_BYTES bytes:
 * LVDGS_MATCH_SCALE_STATE_WORDS int32 words -- [0] status, the tag, [1] num_matches, [2] n, [3] the scale's float bits (0 when n == 0),
 * [4..7] zero -- then sum1 and sum2 as two doubles.
 * LVDGS_E_INVALID: args NULL, a NULL pointer (the matches may be NULL when num_matches == 0), num_matches < 0, a size not > 0. */
#define LVDGS_MATCH_SCALE_STATE_WORDS 8
#define LVDGS_MATCH_SCALE_HOST_BYTES 64
enum {
    LVDGS_MATCH_SCALE_OK = 1,
    LVDGS_MATCH_SCALE_NO_VALID = 2   /* no valid match: there is no scale */
};
typedef struct lvdgs_match_scale_args {
    int32_t num_matches;
    int32_t raster_width, raster_height;   /* (W1, H1) of the matches                */
    int32_t width1, height1, width2, height2;
    const int32_t *matches_im1;   /* M*2 (x, y) in map 1's raster                   */
    const float *matches_im2;     /* M*2 (u, v) in map 2's raster                   */
    const float *depth1;          /* height1*width1                                 */
    const float *depth2;          /* height2*width2                                 */
    int32_t *host_state;          /* LVDGS_MATCH_SCALE_HOST_BYTES, pinned host (the host address) */
} lvdgs_match_scale_args;
int lvdgs_match_depth_scale(const lvdgs_match_scale_args *a, void *stream);

/* ---- the edge mask of the tracking loss (reference utils/camera_utils.py compute_grad_mask :126-155: a channel mean, two reflect
 * pads, the Scharr gradients and the validity mask as convolutions, a magnitude, and a full sort of the image for its median) ----
 * image: (3, height, width) float32, contiguous, channels r, g, b.  All arithmetic is IEEE float32 in exactly this order, no
 * contraction, division and square root correctly rounded:
 *   gray = ((r + g) + b) / 3;  p = gray with ONE reflected pixel on each side (NumPy's pad mode "reflect": p[-1] = gray[1],
 *   p[n] = gray[n - 2]), so width and height must be at least 2.  With p[row][col] the 3 x 3 window around a pixel:
 *   gv = (((((p00*3 + p01*10) + p02*3) + p20*(-3)) + p21*(-10)) + p22*(-3)) * (1/32)
 *   gh = (((((p00*3 + p02*(-3)) + p10*10) + p12*(-10)) + p20*3) + p22*(-3)) * (1/32)
 *   full = |p| > 0.01f at all nine taps;  gv, gh are multiplied by full as 0 / 1;  mag = sqrtf(gv*gv + gh*gh).
 * The MEDIAN of n values is the (n - 1) / 2-th smallest (integer division; torch.median's lower median), found by radix selection on
 * the bit patterns: the bits a sort would give.  A NaN magnitude (a non-finite image) is outside the contract.
 * mode LVDGS_EDGE_MASK_MEDIAN: cut = median(mag) * (float)edge_threshold; mask: height*width bytes, 1 where mag > cut, else 0 -- a
 *   torch.bool tensor's storage, and the bytes the photometric loss takes as grad_mask.
 * mode LVDGS_EDGE_MASK_BLOCKS (the reference's rule for the "replica" dataset type): bh = height / 32, bw = width / 32 (integer
 *   division; width and height must be at least 32); block (i, j), 0 <= i, j < 32, is rows i bh .. i bh + bh - 1, columns j bw ..
 *   j bw + bw - 1, and has its own cut = median(its bh bw magnitudes) * (float)edge_threshold.  mask: height*width FLOAT32; inside
 *   the grid v = mag > cut ? 1 : mag, then v <= cut ? 0 : v (the reference's two assignments in their order: a cut of 1 or more
 *   clears the ones again); the rows and columns outside the grid keep their magnitude.
 * loss_mask (optional, may be NULL): height*width bytes, result != 0 -- the photometric loss' grad_mask in either mode (mode MEDIAN:
 *   the same bytes as mask).  magnitude (optional): mag, height*width float32.  stats (optional): (median, cut) as two float32, in
 *   mode BLOCKS per block: 2 * 1024 float32, block i * 32 + j at [2 (32 i + j)].  Both are for tests.
 * Mode MEDIAN: a clear of the selection state and six launches; mode BLOCKS: two launches.  All enqueued at once; no host wait, no copy.
 * scratch: the bytes lvdgs_edge_mask_scratch_bytes gives for (width, height) (0: the size is refused), no initialisation needed.
 * Two calls give the same bytes.
 * LVDGS_E_INVALID: args NULL, an unknown mode, image / mask / scratch NULL, scratch too small; LVDGS_E_RANGE: width or height below 2
 * (mode BLOCKS: below 32), or more than 2^31 - 1 pixels. */
enum {
    LVDGS_EDGE_MASK_MEDIAN = 0,
    LVDGS_EDGE_MASK_BLOCKS = 1
};
typedef struct lvdgs_edge_mask_args {
    int32_t width, height, mode;
    double edge_threshold;        /* config Training.edge_threshold; rounded to float32  */
    const float *image;           /* 3*H*W                                          */
    void *mask;                   /* out: H*W bytes (MEDIAN) / H*W float32 (BLOCKS)  */
    uint8_t *loss_mask;           /* out H*W bytes, or NULL                         */
    float *magnitude;             /* out H*W, or NULL                               */
    float *stats;                 /* out 2 (MEDIAN) / 2*1024 (BLOCKS) float32, or NULL */
    void *scratch; size_t scratch_bytes;
} lvdgs_edge_mask_args;
size_t lvdgs_edge_mask_scratch_bytes(int32_t width, int32_t height);
int lvdgs_edge_mask(const lvdgs_edge_mask_args *a, void *stream);

/* ---- what the front end reads after a frame's last tracking iteration (reference utils/slam_utils.py get_median_depth :124-134: a
 * boolean gather and a sort; utils/slam_frontend.py is_keyframe / add_to_window :1579-1674: two counts read per keyframe) ----
 * Median depth.  Pixel i of num_pixels is SELECTED when depth[i] > 0, opacity[i] > opacity_bar (opacity NULL: no such test) and
 *   mask[i] != 0 (mask NULL: no such test); NaN fails every test.  The result is the (n - 1) / 2-th smallest of the n selected depths
 *   (integer division), by radix selection on the bit patterns: the bits torch.median gives.  n == 0: the quiet NaN 0x7fc00000.
 * Covisibility.  cur[g] = n_touched[g] > 0 for Gaussian g of num_gaussians.  For row r of num_rows (rows[r]: num_gaussians bytes,
 *   nonzero = visible from that keyframe): intersection = #(cur & row), union = #(cur | row), own = #row.  visible = #cur.
 * mask_count = the nonzero bytes of count_mask (num_pixels bytes; NULL: 0).
 * A clear of the state and six launches, enqueued at once; no host wait.  host_state: a host block ("Host blocks" above) of
 * LVDGS_FRAME_SUMMARY_HOST_BYTES bytes: [LVDGS_FRAME_SUMMARY_SEQ] the call's `seq`, the tag,
 * [_MEDIAN] the median's float bits, [_SELECTED] n, [_VISIBLE], [_MASK_COUNT], zeros up to LVDGS_FRAME_SUMMARY_ROWS, then three
 * words per row, LVDGS_FRAME_SUMMARY_MAX_ROWS of them: intersection, union, own (zero for the rows not passed).
 * scratch: the bytes lvdgs_frame_summary_scratch_bytes gives, no initialisation needed.  Integer sums only: two calls give the same bytes.
 * LVDGS_E_RANGE: num_rows outside 0..LVDGS_FRAME_SUMMARY_MAX_ROWS, num_gaussians < 0, num_pixels < 0; LVDGS_E_INVALID: args NULL,
 * host_state / scratch NULL, depth NULL with num_pixels > 0, n_touched or one of the rows NULL with num_gaussians > 0, scratch too
 * small -- all before any launch. */
#define LVDGS_FRAME_SUMMARY_MAX_ROWS 16
#define LVDGS_FRAME_SUMMARY_HOST_BYTES 256
enum {
    LVDGS_FRAME_SUMMARY_SEQ = 0,
    LVDGS_FRAME_SUMMARY_MEDIAN = 1,
    LVDGS_FRAME_SUMMARY_SELECTED = 2,
    LVDGS_FRAME_SUMMARY_VISIBLE = 3,
    LVDGS_FRAME_SUMMARY_MASK_COUNT = 4,
    LVDGS_FRAME_SUMMARY_ROWS = 8
};
typedef struct lvdgs_frame_summary_args {
    int32_t num_pixels, num_gaussians, num_rows;
    uint32_t seq;
    float opacity_bar;            /* get_median_depth's 0.95                        */
    const float *depth;           /* num_pixels                                     */
    const float *opacity;         /* num_pixels, or NULL                            */
    const uint8_t *mask;          /* num_pixels bytes, or NULL                      */
    const int32_t *n_touched;     /* num_gaussians                                  */
    const uint8_t *rows[LVDGS_FRAME_SUMMARY_MAX_ROWS];   /* num_rows of num_gaussians bytes */
    const uint8_t *count_mask;    /* num_pixels bytes, or NULL                      */
    int32_t *host_state;          /* LVDGS_FRAME_SUMMARY_HOST_BYTES, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_frame_summary_args;
size_t lvdgs_frame_summary_scratch_bytes(void);
int lvdgs_frame_summary(const lvdgs_frame_summary_args *a, void *stream);

/* ---- dynamic-object masks from the detector's boxes and the segmenter's masks (reference utils/slam_frontend.py
 * EnhancedDynamicObjectMasker.detect_and_segment :906-1056 after its two networks, _temporal_consistency :1168-1182,
 * FrontEnd._expand_dynamic_mask :1260-1266, add_new_keyframe :1290-1323 and :1367-1369: NumPy rectangle fills, np.median over a
 * history, two cv2.dilate, two uploads and two waited-for means) ----
 * (h, w) = (height, width).  first_frame: detect_and_segment's own flag, frame_idx == 0 or not first_frame_processed (host state).
 * 1. Boxes.  num_boxes rows of four float32.  LVDGS_DYNAMIC_MASK_BOXES_XYXY: (x1, y1, x2, y2) in pixels, as
 *    GroundingDINODetector.detect returns them.  LVDGS_DYNAMIC_MASK_BOXES_CXCYWH: the model's normalised (cx, cy, bw, bh), taken
 *    through detect's float32 statements first (:364-382), in this order with no contraction: cx*w, cy*h, bw*w, bh*h; the two halves
 *    bw/2, bh/2; x1 = cx - bw/2, y1 = cy - bh/2, x2 = cx + bw/2, y2 = cy + bh/2; x clipped to [0, w], y to [0, h].
 *    Then the four values are truncated toward zero (astype(int)); x1, x2 are clamped to [0, w-1], y1, y2 to [0, h-1]; the box is
 *    DROPPED when x2 <= x1 or y2 <= y1.  vehicle[b] != 0 (a host-computed byte: the label contains one of the eight vehicle keywords,
 *    :926; vehicle NULL: none does) widens a surviving box: ew = (int)((double)(x2-x1) * r), eh = (int)((double)(y2-y1) * r), r = 0.15
 *    on a first frame, else 0.1 (one float64 product, truncated); x1 = max(0, x1-ew), y1 = max(0, y1-eh), x2 = min(w, x2+ew),
 *    y2 = min(h, y2+eh).  Rows y1..y2-1, columns x1..x2-1 of the box mask are set.  vehicle_detected: some surviving box is a vehicle's.
 *    Non-finite coordinates are outside the contract (every store stays inside the frame).
 * 2. The segmenter.  sam_masks: num_sam_masks masks of h*w bytes each, contiguous, nonzero = object; `union` is their OR.
 *    use_sam_result = (union has a set pixel) -- data on the device.  final = use_sam_result ? union : box mask (replaced, not merged).
 * 3. The reference's motion refinement is an identity (logical_and with ~ of a uint8 array, :1134) and is not computed.
 * 4. Temporal consistency, only when the frame is not first and use_sam_result is 0: final (before any dilation) is appended to the
 *    history in `state`, the oldest entry dropped when it then holds more than history_length entries; with n >= 3 entries a pixel
 *    stays set exactly when more than n / 2 of the n entries have it set (np.median(...).astype(uint8); a tie gives 0); with fewer,
 *    final is unchanged.  The history keeps the unfiltered inputs.
 * 5. When vehicle_detected, final is dilated by a k x k square of ones, k = vehicle_kernel_first on a first frame, else
 *    vehicle_kernel (7 and 5 in the reference).  DILATION: a pixel is set when any pixel of its centred k x k window that lies inside
 *    the image is set.  dynamic = final, static = 1 - dynamic.
 * 6. expand_kernel != 0 (keyframes: 9 for frame 0, else 7): expanded_dynamic = dynamic dilated by expand_kernel, expanded_static its
 *    complement, valid_rgb = ((r + g) + b > (float)rgb_boundary_threshold) & expanded_static with image (3, h, w) float32 and the
 *    float32 sum in that order; depth_out (optional) = depth_in where valid_rgb, else 0.
 * With num_boxes == 0 the steps run as stated on an empty box mask; the reference's fallback branch (:887-904) is the caller's.
 * Outputs: h*w bytes of 0 / 1 each -- a torch.bool tensor's storage, the bytes the masked loss reads --, each may be NULL.
 * info: LVDGS_DYNAMIC_MASK_INFO_WORDS int32 on the device (required; nobody has to read them): [_BOXES] surviving boxes, [_VEHICLE]
 *   vehicle_detected, [_USE_SAM], [_FILTERED] step 4 ran, [_HISTORY] entries in the history after the call, then the set pixels of
 *   [_BOX_PIXELS] the box mask, [_SAM_PIXELS] the union, [_DYNAMIC_PIXELS], [_STATIC_PIXELS], [_EXPANDED_PIXELS] expanded_dynamic,
 *   [_VALID_PIXELS] valid_rgb, [_DEPTH_PIXELS] the pixels of the masked depth above 0 (depth_in given); the rest 0.
 * state: the persistent history, caller-owned, lvdgs_dynamic_mask_state_bytes bytes: a header (frame size, ring length, entries,
 *   head) and history_length bit planes.  A zeroed block -- and a block left by another frame size or ring length -- is an empty history.
 * scratch: lvdgs_dynamic_mask_scratch_bytes bytes, no initialisation needed.  Either size query gives 0 for sizes the call refuses.
 * A clear of info and four launches (three when expand_kernel == 0), enqueued at once: their number does not depend on the boxes, on
 * use_sam_result or on the history.  No host wait, no copy.  Integer work only: equal inputs and equal state give equal bytes.
 * LVDGS_E_INVALID: args NULL; state / scratch / info NULL; boxes or sam_masks NULL with a count above 0; image NULL with
 * expand_kernel != 0; depth_out without depth_in; an unknown box_format; a vehicle kernel that is even or outside 1..15, an
 * expand_kernel that is neither 0 nor odd in 1..15; state or scratch too small.  LVDGS_E_RANGE: width or height below 1, more than
 * 2^31 - 1 pixels, a negative count, history_length outside 1..8.  All before any launch. */
enum {
    LVDGS_DYNAMIC_MASK_BOXES_XYXY = 0,
    LVDGS_DYNAMIC_MASK_BOXES_CXCYWH = 1
};
#define LVDGS_DYNAMIC_MASK_INFO_WORDS 16
enum {
    LVDGS_DYNAMIC_MASK_INFO_BOXES = 0,
    LVDGS_DYNAMIC_MASK_INFO_VEHICLE = 1,
    LVDGS_DYNAMIC_MASK_INFO_USE_SAM = 2,
    LVDGS_DYNAMIC_MASK_INFO_FILTERED = 3,
    LVDGS_DYNAMIC_MASK_INFO_HISTORY = 4,
    LVDGS_DYNAMIC_MASK_INFO_BOX_PIXELS = 5,
    LVDGS_DYNAMIC_MASK_INFO_SAM_PIXELS = 6,
    LVDGS_DYNAMIC_MASK_INFO_DYNAMIC_PIXELS = 7,
    LVDGS_DYNAMIC_MASK_INFO_STATIC_PIXELS = 8,
    LVDGS_DYNAMIC_MASK_INFO_EXPANDED_PIXELS = 9,
    LVDGS_DYNAMIC_MASK_INFO_VALID_PIXELS = 10,
    LVDGS_DYNAMIC_MASK_INFO_DEPTH_PIXELS = 11
};
typedef struct lvdgs_dynamic_mask_args {
    int32_t width, height;
    int32_t first_frame;          /* detect_and_segment's is_first_frame                */
    int32_t box_format, num_boxes;
    const float *boxes;           /* num_boxes * 4                                  */
    const uint8_t *vehicle;       /* num_boxes bytes, or NULL                       */
    int32_t num_sam_masks;
    const uint8_t *sam_masks;     /* num_sam_masks * H*W bytes                      */
    int32_t history_length;       /* 1..8; the reference's 5                        */
    int32_t vehicle_kernel_first, vehicle_kernel;   /* 7, 5                         */
    int32_t expand_kernel;        /* 0: no step 6                                   */
    const float *image;           /* 3*H*W; may be NULL when expand_kernel == 0     */
    double rgb_boundary_threshold;  /* config Training.rgb_boundary_threshold; rounded to float32 */
    const float *depth_in;        /* H*W, or NULL                                   */
    float *depth_out;             /* out H*W, or NULL                               */
    uint8_t *static_mask, *dynamic_mask, *expanded_dynamic, *expanded_static, *valid_rgb;   /* out H*W bytes each, or NULL */
    int32_t *info;                /* out LVDGS_DYNAMIC_MASK_INFO_WORDS              */
    void *state; size_t state_bytes;
    void *scratch; size_t scratch_bytes;
} lvdgs_dynamic_mask_args;
size_t lvdgs_dynamic_mask_state_bytes(int32_t width, int32_t height, int32_t history_length);
size_t lvdgs_dynamic_mask_scratch_bytes(int32_t width, int32_t height);
int lvdgs_dynamic_mask(const lvdgs_dynamic_mask_args *a, void *stream);

/* ---- dense Farneback optical flow and the motion mask of the masker's fallback branch (reference utils/slam_frontend.py
 * _fallback_detection :651-672: cv2.cvtColor, cv2.calcOpticalFlowFarneback(prev, cur, None, pyr_scale=0.5, levels=3, winsize=15,
 * iterations=3, poly_n=5, poly_sigma=1.2, flags=0), magnitude > motion_threshold, a 7 x 7 cv2.dilate) ----
 * THE TEXT BELOW IS THE DEFINITION.  It restates OpenCV's Farneback with the box window (flags = 0, no initial flow); parity with
 * the real cv2 -- calcOpticalFlowFarneback, the grey conversion, dilate -- is UNPINNED: OpenCV is not installed where this is built.
 * (h, w) is a level's size, (H, W) = (height, width) the frame's.  float = float32; every float expression is evaluated as written,
 * without contraction; a sum over taps adds one product at a time, taps ascending.  "On the host in double" values reach the device
 * rounded to float32.  The flow of a second frame that is the first one shifted by +d is +d.
 * GREY (lvdgs_motion_mask).  image is (3, H, W) float32.  Per channel q = (uint8)min(max(c * 255.0f, 0), 255), truncated (the
 *   reference's (img * 255).astype(np.uint8); NaN is outside the contract); grey = (4899 R + 9617 G + 1868 B + 8192) >> 14 in integers.
 * PYRAMID.  k = 0, s = 1; while k < levels: s *= pyr_scale; stop when W s < 32 or H s < 32; else k++.  Levels k .. 0 are processed,
 *   coarse to fine.  Level k: scale = the product of k factors pyr_scale, sigma = (1 / scale - 1) / 2, ksize = max(rint(5 sigma) | 1, 3),
 *   w = rint(W scale), h = rint(H scale), rint rounding half to even (261 x 259: 130 x 130, 65 x 65, 33 x 32).  Each of the two grey
 *   images is converted to float, blurred at FULL resolution -- along the rows, then along the columns, border reflect-101 -- by ksize
 *   taps ([1/4, 1/2, 1/4] when sigma == 0, else exp(-x^2 / (2 sigma^2)) normalised to sum 1, on the host in double), and resized to
 *   w x h bilinearly: source coordinate s = (i + 0.5) * (n_in / n_out) - 0.5 in double, i0 = floor(s), f = (float)(s - i0), the indices
 *   i0 and i0 + 1 clamped to the image, value (a (1 - fx) + b fx) (1 - fy) + (c (1 - fx) + d fx) fy with a, b the upper pair.  The
 *   flow of the coarser level is resized the same way, component by component, and multiplied by (float)(1 / pyr_scale); the coarsest
 *   level starts from zero.
 * POLYNOMIAL EXPANSION (n = poly_n, taps -n .. n), on the host in double: g[x] = exp(-x^2 / (2 poly_sigma^2)) rounded to float32, then
 *   divided by its sum; xg = x g, xxg = x^2 g; the 6 x 6 moment matrix G with G00 = sum g[y] g[x], G11 = sum g g x^2, G33 = sum g g x^4,
 *   G55 = sum g g x^2 y^2 over the (2n + 1)^2 window, G22 = G03 = G04 = G30 = G40 = G11, G44 = G33, G34 = G43 = G55, the rest 0;
 *   ig11 = inv(G)[1][1], ig03 = inv(G)[0][3], ig33 = inv(G)[3][3], ig55 = inv(G)[5][5].  Correlations of the level image along the
 *   columns with g, xg, xxg give v0, v1, v2; along the rows then b1 = v0*g, b2 = v0*xg, b4 = v0*xxg, b3 = v1*g, b5 = v1*xg, b6 = v2*g;
 *   both passes replicate the edge.  R = [b3 ig11, b2 ig11, b1 ig03 + b6 ig33, b1 ig03 + b4 ig33, b5 ig55]: (y, x, yy, xx, xy).
 * MATRICES at pixel (x, y) with flow (dx, dy): fx = (float)x + dx, fy = (float)y + dy, x1 = floor(fx), y1 = floor(fy).  If 0 <= x1 <
 *   w - 1 and 0 <= y1 < h - 1: with fx -= x1, fy -= y1 the five channels of R1 are interpolated into r2 .. r6 as a00 R1[y1][x1] +
 *   a01 R1[y1][x1+1] + a10 R1[y1+1][x1] + a11 R1[y1+1][x1+1], a00 = (1-fx)(1-fy), a01 = fx (1-fy), a10 = (1-fx) fy, a11 = fx fy; then
 *   r4 = (R0[2] + r4) 0.5, r5 = (R0[3] + r5) 0.5, r6 = (R0[4] + r6) 0.25, r2 = (R0[0] - r2) 0.5 + (r4 dy + r6 dx),
 *   r3 = (R0[1] - r3) 0.5 + (r6 dy + r5 dx).  Otherwise r2 = r3 = 0, r4 = R0[2], r5 = R0[3], r6 = R0[4] 0.5.  All five are multiplied by
 *   bx by, where bx = B[min(x, 5)] B[min(w - 1 - x, 5)] (by likewise with y, h), B = {0.14, 0.14, 0.4472, 0.4472, 0.4472, 1}.
 *   M = [r4 r4 + r6 r6, (r4 + r5) r6, r5 r5 + r6 r6, r4 r2 + r6 r3, r6 r2 + r5 r3].
 * UPDATE.  S = the sum of M over the winsize x winsize window -- along the rows, then along the columns, both replicating the edge --
 *   times (float)(1 / winsize^2).  With [g11, g12, g22, h1, h2] = S: idet = 1 / (g11 g22 - g12 g12 + 1e-3f),
 *   flow_x = (g11 h2 - g12 h1) idet, flow_y = (g22 h1 - g12 h2) idet.  A level runs `iterations` updates; M is recomputed from the
 *   new flow after every update but the last.
 * lvdgs_farneback_flow: prev, next: H*W grey bytes each on the device; flow: (H, W, 2) float32, x then y.  scratch:
 *   lvdgs_farneback_scratch_bytes bytes, no initialisation needed (0 for sizes the call refuses).  Per level one launch that blurs and
 *   resizes both images, one that expands both, one that resizes the flow and forms M, and one per update (it sums M, solves and forms
 *   the next M): 3 + iterations launches a level, enqueued at once, their number a function of the sizes and parameters only.
 * LVDGS_E_INVALID: args, prev, next, flow or scratch NULL; winsize even or outside 3..31; poly_n neither 5 nor 7; scratch too small.
 * LVDGS_E_RANGE: width or height outside 1..16384; pyr_scale not inside (0, 1); levels outside 0..8; iterations outside 1..10;
 * poly_sigma not above 0; a pyramid level whose blur has more than LVDGS_FARNEBACK_MAX_BLUR_TAPS taps.  All before any launch.
 *
 * lvdgs_motion_mask: the fallback's statements around the flow, stateful.  state: lvdgs_motion_mask_state_bytes bytes, caller-owned: a
 *   header and the stored grey plane; a zeroed block -- and a block left by another frame size -- holds no previous frame.  mode:
 *   LVDGS_MOTION_OBSERVE alone: the grey plane of image becomes the stored frame, nothing else is written (one launch).
 *   LVDGS_MOTION_MASK: the flow from the stored frame to the grey plane of image; moving = sqrtf(fx fx + fy fy) > (float)motion_threshold;
 *     mask = moving dilated by dilate_kernel (odd, 1..15) by the DILATION rule of lvdgs_dynamic_mask's step 5 (the same bit-plane code),
 *     written as H*W bytes of 0 / 1.  With no stored frame the mask is all zero.  The stored frame is unchanged, unless
 *   LVDGS_MOTION_ADVANCE is set as well: then the grey plane of image is the stored frame after the call.
 *   info: LVDGS_MOTION_INFO_WORDS int32 on the device (required by MASK; nobody has to read them): [_HAS_PREV] a frame was stored, [_LEVELS]
 *   the pyramid's levels, [_MOVING_PIXELS] set pixels before the dilation, [_MASK_PIXELS] after it; the rest 0 (OBSERVE writes none).
 *   flow: optional output as above (undefined content when no frame was stored).  scratch: lvdgs_motion_mask_scratch_bytes bytes.
 *   A clear of info, the grey launch, the flow's launches, one launch for the threshold and one for the dilation: enqueued at once,
 *   their number a function of the sizes and parameters only -- never of whether a frame is stored.  No host wait, no copy, no float
 *   atomics: equal inputs and equal state give equal bytes.
 * LVDGS_E_INVALID, beyond the flow's: image or state NULL; mask, info or scratch NULL in a MASK call; a mode other than OBSERVE,
 * MASK or MASK | ADVANCE; a dilate_kernel that is even or outside 1..15; state -- in a MASK call: or scratch -- too small.  LVDGS_E_RANGE: the flow's.  All
 * before any launch. */
#define LVDGS_FARNEBACK_MAX_BLUR_TAPS 127
enum {
    LVDGS_MOTION_OBSERVE = 1,
    LVDGS_MOTION_MASK = 2,
    LVDGS_MOTION_ADVANCE = 4
};
#define LVDGS_MOTION_INFO_WORDS 8
enum {
    LVDGS_MOTION_INFO_HAS_PREV = 0,
    LVDGS_MOTION_INFO_LEVELS = 1,
    LVDGS_MOTION_INFO_MOVING_PIXELS = 2,
    LVDGS_MOTION_INFO_MASK_PIXELS = 3
};
typedef struct lvdgs_farneback_params {
    double pyr_scale;             /* (0, 1); the reference's 0.5                    */
    int32_t levels;               /* 0..8; 3                                        */
    int32_t winsize;              /* odd, 3..31; 15                                 */
    int32_t iterations;           /* 1..10; 3                                       */
    int32_t poly_n;               /* 5 or 7; 5                                      */
    double poly_sigma;            /* > 0; 1.2                                       */
} lvdgs_farneback_params;
typedef struct lvdgs_farneback_args {
    int32_t width, height;
    lvdgs_farneback_params params;
    const uint8_t *prev, *next;   /* H*W grey bytes each                            */
    float *flow;                  /* out H*W*2                                      */
    void *scratch; size_t scratch_bytes;
} lvdgs_farneback_args;
typedef struct lvdgs_motion_mask_args {
    int32_t width, height;
    int32_t mode;                 /* LVDGS_MOTION_*                                 */
    int32_t dilate_kernel;        /* odd, 1..15; the reference's 7                  */
    lvdgs_farneback_params params;
    double motion_threshold;      /* the reference's 3.0; rounded to float32        */
    const float *image;           /* 3*H*W                                          */
    uint8_t *mask;                /* out H*W bytes (MASK)                           */
    float *flow;                  /* out H*W*2, or NULL                             */
    int32_t *info;                /* out LVDGS_MOTION_INFO_WORDS                    */
    void *state; size_t state_bytes;
    void *scratch; size_t scratch_bytes;
} lvdgs_motion_mask_args;
size_t lvdgs_farneback_scratch_bytes(int32_t width, int32_t height);
int lvdgs_farneback_flow(const lvdgs_farneback_args *a, void *stream);
size_t lvdgs_motion_mask_state_bytes(int32_t width, int32_t height);
size_t lvdgs_motion_mask_scratch_bytes(int32_t width, int32_t height);
int lvdgs_motion_mask(const lvdgs_motion_mask_args *a, void *stream);

/* ---- seeding a keyframe's Gaussians (GaussianModel.create_pcd_from_image_and_depth: a full sort for the median, nonzero, a host
 * draw, an upload and about fifteen gathers, with two host waits) ----
 * Pixel i = v*width + u is VALID when depth[i] > 0 && depth[i] <= depth_trunc (NaN fails).  n_valid = the number of valid pixels;
 * n_keep = (int64)((double)n_valid * inv_downsample), on the device, in double (Python's int(n_valid * (1.0 / downsample))).
 * Every pixel has a 32-bit key, all arithmetic uint32 with wrap-around:
 *   fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16
 *   key(i)   = fmix32( fmix32((uint32)i + seed_lo) ^ seed_hi )              seed = seed_hi:seed_lo
 * fmix32, the addition and the xor are bijections of uint32, so for one seed all keys of an image are distinct: no ties.
 * SELECTED are the n_keep valid pixels with the smallest keys, {i valid : key(i) <= t} with t the key of rank n_keep - 1 among the
 * valid keys; n_keep == 0 selects nothing.  Output rows are in ascending pixel index.  For selected pixel i with z = depth[i], in
 * float32, evaluated as written with no contraction:
 *   cam = ( ((float)u - cx) * z / fx, ((float)v - cy) * z / fy, z )
 *   xyz[j] = (cam[0]-T[0])*R[0][j] + (cam[1]-T[1])*R[1][j] + (cam[2]-T[2])*R[2][j], summed in that order (p_cam = R p_world + T)
 *   per channel c = min(max(gain * image[ch][i] + offset, 0), 1), q = (uint8)(c * 255) by truncation, rgb = (float)q * (1.0f / 255.0f)
 *   -- the bits of `uint8.float() / 255.0` in PyTorch on a GPU, which multiplies by the float32 reciprocal of a scalar divisor; a true
 *   division differs in the last bit for 126 of the 256 values --, f_dc = (rgb - 0.5f) / 0.28209479177387814f.  A NaN colour is
 *   outside the contract.
 * gain, offset: one float each ON THE DEVICE (NULL: 1 and 0); the caller's exp(exposure_a) and exposure_b.
 * want_median: the (P - 1) / 2-th smallest of all P = width*height depth values, the bits of torch.median (a NaN depth is outside
 * that contract, as for lvdgs_frame_summary).
 * A clear of the state and eight launches (twelve with the median), enqueued at once; no host wait.  host_state: a host block
 * ("Host blocks" above) of LVDGS_SEED_HOST_BYTES bytes: [LVDGS_SEED_SEQ] the call's `seq`, the tag; [_N_VALID]; [_N_KEEP], the rows written; [_MEDIAN] the float bits, or the quiet NaN 0x7fc00000 when not asked
 * for; [_THRESHOLD] the key t, for diagnosis; zeros after it.  scratch: the bytes lvdgs_seed_scratch_bytes gives (0: the size is
 * refused), no initialisation needed.  No atomic decides an output position: two calls give the same bytes.
 * Before any launch -- LVDGS_E_RANGE: width or height below 1, more than 2^31 - 1 pixels, inv_downsample NaN or outside (0, 1],
 * capacity < (int64)((double)(width*height) * inv_downsample) (the host-side bound of n_keep); LVDGS_E_INVALID: args, depth, R, T, xyz,
 * host_state or scratch NULL, rgb or f_dc NULL with an image, scratch too small. */
#define LVDGS_SEED_HOST_BYTES 64
enum {
    LVDGS_SEED_SEQ = 0,
    LVDGS_SEED_N_VALID = 1,
    LVDGS_SEED_N_KEEP = 2,
    LVDGS_SEED_MEDIAN = 3,
    LVDGS_SEED_THRESHOLD = 4
};
typedef struct lvdgs_seed_args {
    int32_t width, height;
    float fx, fy, cx, cy, depth_trunc;
    int32_t want_median;
    double inv_downsample;        /* in (0, 1]                                      */
    uint64_t seed;
    uint32_t seq;
    int32_t capacity;             /* rows the outputs hold                          */
    const float *image;           /* 3*H*W planar, or NULL: no colours              */
    const float *gain, *offset;   /* one float each on the device, or NULL: 1 and 0 */
    const float *depth;           /* H*W                                            */
    const float *R, *T;           /* 9 row-major and 3, on the device               */
    float *xyz, *rgb, *f_dc;      /* out capacity*3 each (rgb, f_dc may be NULL without an image) */
    int32_t *pixel;               /* out capacity: the rows' pixel indices, or NULL */
    int32_t *host_state;          /* LVDGS_SEED_HOST_BYTES, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_seed_args;
size_t lvdgs_seed_scratch_bytes(int32_t width, int32_t height);
int lvdgs_seed_points(const lvdgs_seed_args *a, void *stream);

/* ---- editing the map: prune_points, densify_and_prune and the pruning pass's rule as ONE plan, then one launch that moves every
 * per-Gaussian array (GaussianModel: three map edits in a row, each a nonzero the host waits for, an index copy to the CPU and 21
 * index_select / cat launches) ----
 * lvdgs_map_edit_plan decides, counts and lays out; it moves no row.  For N = num_gaussians source rows it writes, per OUTPUT row r,
 *   src[r] (the source row), kind[r] (LVDGS_EDIT_KEEP / _CLONE / _SPLIT0 / _SPLIT1) and noise_row[r] (-1 unless a split child),
 * and into host_state -- a host block ("Host blocks" above) of host_bytes >= 4 (LVDGS_EDIT_HOST_SRC + 2 N) bytes --
 *   [LVDGS_EDIT_SEQ] the call's `seq`, the tag; [_N_OUT] output rows; [_N_KEEP] those of kind KEEP; [_N_CLONE] those of kind
 *   CLONE; [_N_SPLIT_SEL] the split SOURCES, pruned or not (the noise tensor has 2 n_split_sel rows); [_N_PRUNED_FINAL] the rows the
 *   final prune took (prune mode: N - n_out); zeros up to [LVDGS_EDIT_HOST_SRC]; then src[0 .. n_out), and in prune mode with rule (b)
 *   n_obs[src[r]] for r in [0, n_out) behind it.
 * src, kind, noise_row hold `capacity` rows: at least N in prune mode, 2 N in densify mode (every source gives at most two rows).
 *
 * mode LVDGS_EDIT_PRUNE: the rows of [0, N) that survive, ascending, all of kind KEEP.  Row i is REMOVED
 *   (a) remove != NULL:  when remove[i] != 0                                   (GaussianModel.prune_points(mask));
 *   (b) remove == NULL:  n_obs[i] = the number of k < num_vis_rows with vis_rows[k][i] != 0, written to n_obs (int32, N) -- the rows'
 *       elements are 0 or 1, vis_stride (1, 4 or 8; 0 means 1) bytes apart, little-endian: their first byte is read --, and the row
 *       is removed when n_obs[i] <= prune_num && kf_id[i] >= min_kf_id      (the pruning pass of the mapping loop; its `odometry`
 *       mode, n_obs < 3, is prune_num = 2 and min_kf_id = INT32_MIN).
 * mode LVDGS_EDIT_DENSIFY: GaussianModel.densify_and_prune's three stages -- clone, split-then-prune, final prune -- as one
 * classification per source row, in float32, evaluated as written.  With s = the row's scale_dims (1 or 3) raw scales, o its raw opacity:
 *   g      = grad_accum[i] / denom[i], NaN -> 0                                (0/0 is 0; x/0 stays +-inf)
 *   big(t) = the maximum of expf(t[j]) over j, a NaN propagating               (torch.max)
 *   clone  = |g| >= grad_threshold && big(s) <= dense_extent                   (the clone stage takes the norm of g, the split stage g itself)
 *   split  =  g  >= grad_threshold && big(s) >  dense_extent
 *   child(t)[j] = logf(expf(t[j]) / 1.6f), the raw scale of both split children -- the SAME device expression in plan and apply
 *   gone(t) = 1 / (1 + expf(-o)) < min_opacity || (max_screen_size != 0 && (0 > max_screen_size || big(t) > world_extent))
 * The list before the final prune is the host path's: originals that were not split, ascending; then the clones, ascending by source;
 * then SPLIT0 of every split source, ascending; then SPLIT1 likewise.  The final prune drops a KEEP or CLONE row of source i when
 * gone(s) and a split child when gone(child(s)).  The screen-size term reads NO max_radii2D: densification_postfix has set that
 * statistic to zero before the final prune looks at it, in every call, so `max_radii2D > max_screen_size` is `0 > max_screen_size` -- what
 * the code does, not what the name suggests; and the world-size term applies only with max_screen_size != 0, as in the code.  The
 * field max_radii2D is accepted and never read.  noise_row of a SPLITk child = k * n_split_sel + (the rank of its source among the
 * split sources): the row of the host path's randn((2 n_split_sel, 3)) draw, whether the child survives or not.
 * Four launches, enqueued at once, no host wait; no atomic decides a position: two calls give the same bytes.  scratch: the bytes
 * lvdgs_map_edit_scratch_bytes(N) gives (0: N < 0), no initialisation needed.
 * Before any launch -- LVDGS_E_INVALID: args, src, kind, noise_row, host_state or scratch NULL; a mode's inputs NULL (prune (b):
 * kf_id, n_obs, a vis row; densify: grad_accum, denom, scaling, opacity); scratch too small; LVDGS_E_RANGE: N < 0, an unknown mode,
 * num_vis_rows outside [0, LVDGS_EDIT_MAX_VIS_ROWS], a vis_stride other than 0, 1, 4, 8, scale_dims not 1 or 3, capacity or host_bytes too small.
 *
 * lvdgs_map_edit_apply moves the rows of up to LVDGS_EDIT_MAX_COLUMNS columns in one launch and does not wait: for every column and
 * every r < n_out, out row r (row_bytes bytes, any value >= 1) is
 *   kind KEEP, or new_rows LVDGS_EDIT_COPY:   the bytes of in row src[r]          (parameters, kf ids, n_obs, visibility rows)
 *   new_rows LVDGS_EDIT_ZERO, kind != KEEP:   zeros                                (Adam moments of new rows)
 *   new_rows LVDGS_EDIT_XYZ,   a split child: R(q) (noise[noise_row[r]] * expf(s)) + xyz, of the source's rows of `in` (xyz, 12
 *     bytes), `rotation` (q = (r, x, y, z), 16 bytes, as stored: normalised here) and `scaling` (s; one value serves the three axes
 *     when scale_dims is 1).  n = sqrtf(((r r + x x) + y y) + z z); r, x, y, z /= n; R as build_rotation states it:
 *       R0 = (1 - 2 (y y + z z), 2 (x y - r z), 2 (x z + r y));  R1 = (2 (x y + r z), 1 - 2 (x x + z z), 2 (y z - r x));
 *       R2 = (2 (x z - r y), 2 (y z + r x), 1 - 2 (x x + y y));   v[k] = noise[..][k] * expf(s[k]);
 *       out[j] = ((Rj[0] v[0] + Rj[1] v[1]) + Rj[2] v[2]) + xyz[j], no contraction.   (CLONE rows copy.)
 *   new_rows LVDGS_EDIT_SCALE, a split child: child(s) of the source's row of `in` (4 scale_dims bytes).   (CLONE rows copy.)
 * Rows at and beyond n_out of an `out` array are not written.  in and out must not overlap.  src, kind, noise_row: a plan's outputs;
 * n_out, n_split_sel: what the plan reported.  _XYZ and _SCALE columns are for densify mode.
 * LVDGS_E_INVALID: args, src or kind NULL, a column's in or out NULL, row_bytes < 1, an unknown new_rows, an _XYZ column without noise_row,
 * noise, scaling and rotation or whose row_bytes is not 12, a _SCALE column whose row_bytes is not 4 scale_dims; LVDGS_E_RANGE: more
 * than LVDGS_EDIT_MAX_COLUMNS columns or fewer than 0, n_out or N < 0, scale_dims not 1 or 3. */
#define LVDGS_EDIT_MAX_COLUMNS 48
#define LVDGS_EDIT_MAX_VIS_ROWS 16
enum { LVDGS_EDIT_PRUNE = 0, LVDGS_EDIT_DENSIFY = 1 };                                               /* mode     */
enum { LVDGS_EDIT_KEEP = 0, LVDGS_EDIT_CLONE = 1, LVDGS_EDIT_SPLIT0 = 2, LVDGS_EDIT_SPLIT1 = 3 };   /* kind     */
enum { LVDGS_EDIT_COPY = 0, LVDGS_EDIT_ZERO = 1, LVDGS_EDIT_XYZ = 2, LVDGS_EDIT_SCALE = 3 };        /* new_rows */
enum {
    LVDGS_EDIT_SEQ = 0,
    LVDGS_EDIT_N_OUT = 1,
    LVDGS_EDIT_N_KEEP = 2,
    LVDGS_EDIT_N_CLONE = 3,
    LVDGS_EDIT_N_SPLIT_SEL = 4,
    LVDGS_EDIT_N_PRUNED_FINAL = 5,
    LVDGS_EDIT_HOST_SRC = 16
};
typedef struct lvdgs_map_edit_plan_args {
    int32_t mode;                 /* LVDGS_EDIT_PRUNE / _DENSIFY                    */
    int32_t num_gaussians;        /* N source rows                                  */
    uint32_t seq;
    int32_t scale_dims;           /* densify: 1 or 3 raw scales per row             */
    const uint8_t *remove;        /* prune (a): N bytes, or NULL: rule (b)          */
    int32_t num_vis_rows;         /* prune (b): rows of vis_rows in use             */
    int32_t prune_num;
    int32_t min_kf_id;
    int32_t capacity;             /* rows src / kind / noise_row hold               */
    const uint8_t *vis_rows[LVDGS_EDIT_MAX_VIS_ROWS];   /* prune (b): N bytes each */
    const int32_t *kf_id;         /* prune (b): N                                   */
    int32_t *n_obs;               /* prune (b): out N                               */
    const float *grad_accum, *denom;      /* densify: N each                        */
    const float *scaling;         /* densify: N*scale_dims, raw                     */
    const float *opacity;         /* densify: N, raw                                */
    const float *max_radii2D;     /* never read (see above); may be NULL            */
    float grad_threshold;
    float dense_extent;           /* percent_dense * extent                         */
    float min_opacity;
    float max_screen_size;        /* 0: off                                         */
    float world_extent;           /* 0.1 * extent                                   */
    int32_t vis_stride;           /* prune (b): bytes per element of a vis row: 1, 4 or 8 (0: 1) */
    int32_t *src;                 /* out capacity                                   */
    uint8_t *kind;                /* out capacity                                   */
    int32_t *noise_row;           /* out capacity                                   */
    int32_t *host_state;          /* pinned host (the host address)                 */
    size_t host_bytes;
    void *scratch; size_t scratch_bytes;
} lvdgs_map_edit_plan_args;
typedef struct lvdgs_map_edit_column {
    const void *in;               /* N rows                                         */
    void *out;                    /* at least n_out rows                            */
    int32_t row_bytes;            /* >= 1                                           */
    int32_t new_rows;             /* LVDGS_EDIT_COPY / _ZERO / _XYZ / _SCALE        */
} lvdgs_map_edit_column;
typedef struct lvdgs_map_edit_apply_args {
    int32_t num_gaussians;        /* N source rows                                  */
    int32_t n_out;                /* the plan's output rows                         */
    int32_t n_split_sel;          /* the plan's split sources: noise has twice as many rows */
    int32_t scale_dims;
    int32_t num_columns;
    int32_t reserved;
    const int32_t *src;           /* the plan's outputs                             */
    const uint8_t *kind;
    const int32_t *noise_row;     /* may be NULL without an _XYZ column             */
    const float *noise;           /* 2 n_split_sel * 3, or NULL                     */
    const float *scaling;         /* N*scale_dims raw: the _XYZ column's scales, or NULL */
    const float *rotation;        /* N*4 as stored: the _XYZ column's quaternions, or NULL */
    lvdgs_map_edit_column columns[LVDGS_EDIT_MAX_COLUMNS];
} lvdgs_map_edit_apply_args;
size_t lvdgs_map_edit_scratch_bytes(int32_t num_gaussians);
int lvdgs_map_edit_plan(const lvdgs_map_edit_plan_args *a, void *stream);
int lvdgs_map_edit_apply(const lvdgs_map_edit_apply_args *a, void *stream);

/* ---- a decoded frame's way onto the device (reference utils/dataset.py MonocularDataset.__getitem__ :321-344: per frame, on the
 * host, cv2.remap(INTER_LINEAR) over the whole frame when the calibration is distorted, image / 255.0 as a float64 array, a clamp, a
 * permute, and an upload of float32; the map comes from cv2.initUndistortRectifyMap(K, dist, I, K, (W, H), CV_32FC1) in __init__) ----
 * The arithmetic below is the contract of both the device entry points and the package's host mode (lvdgs.dataset, ingest="host"):
 * the same bits.
 * Conversion.  image[c][v][u] = (float)((double)byte / 255.0): what a float64 division followed by a cast to float32 gives.  The
 *   reference's clamp to [0, 1] is a no-op on bytes.
 * Undistortion map, all float64, evaluated as written (no contraction), for destination pixel (u, v), dist = (k1, k2, p1, p2, k3):
 *   x = (u - cx) / fx;  y = (v - cy) / fy;  r2 = x*x + y*y;
 *   kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2;
 *   xd = x*kr + 2*p1*x*y + p2*(r2 + 2*x*x);
 *   yd = y*kr + p1*(r2 + 2*y*y) + 2*p2*x*y;
 *   mapx = (float)(fx*xd + cx);  mapy = (float)(fy*yd + cy);
 *   sx = rint(mapx * 32), ties to even, as int32; sy likewise.  A coordinate that is not finite or whose magnitude is >= 2^20 is
 *   stored as INT32_MIN and means "outside".
 * Remap.  ix = sx >> 5 (floor, negatives too), ax = sx & 31; iy, ay likewise.  The neighbours (ix, iy), (ix+1, iy), (ix, iy+1),
 *   (ix+1, iy+1) carry the weights (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay; a neighbour outside the image counts as 0 on its own
 *   (a constant border), a pixel with an "outside" coordinate is 0.  out = (sum + 512) >> 10 per channel, in integers.
 *   Parity with the real cv2.remap is UNPINNED: OpenCV is not installed where this was written.  As recalled, it rounds these products
 *   into 15-bit weight tables and builds the map incrementally along a row; a grey level of difference in rare pixels is possible and
 *   has not been measured.
 * lvdgs_undistort_map: sx, sy: height*width int32 each, device.  dist: five doubles on the HOST, read during the call (nothing the
 *   caller must keep).  One launch, no wait.
 * lvdgs_ingest_frame: one launch, no host wait, no copy.  src: device bytes, row v at src + v * src_row_bytes, 3 bytes per pixel
 *   (src_row_bytes >= 3 * width; no alignment is assumed).  map_sx / map_sy: both NULL = no remap.  image_u8 (optional): the bytes
 *   after the remap, height*width*3 without a row gap -- what a detector or the matcher's formatting would take.  A map entry
 *   addresses no byte outside src whatever it holds.  Two calls give the same bytes.
 * LVDGS_E_INVALID, before anything is enqueued: args NULL, width or height not > 0 (an empty frame is refused, as by
 *   lvdgs_format_image), src / image / dist / sx / sy NULL, exactly one of map_sx / map_sy NULL, src_row_bytes < 3 * width, fx or fy
 *   zero or a non-finite intrinsic.  LVDGS_E_RANGE: a raster beyond 2^31 workgroups. */
typedef struct lvdgs_ingest_args {
    int32_t width, height;
    const uint8_t *src;           /* height rows of src_row_bytes, 3 bytes per pixel */
    int64_t src_row_bytes;
    const int32_t *map_sx;        /* height*width, or NULL                          */
    const int32_t *map_sy;        /* height*width, or NULL                          */
    float *image;                 /* out 3*height*width                             */
    uint8_t *image_u8;            /* out height*width*3, or NULL                    */
} lvdgs_ingest_args;
int lvdgs_undistort_map(int32_t width, int32_t height, double fx, double fy, double cx, double cy, const double dist[5],
                        int32_t *sx, int32_t *sy, void *stream);
int lvdgs_ingest_frame(const lvdgs_ingest_args *a, void *stream);

/* ---- a depth file's samples to the float32 plane (reference utils/dataset.py :331-335: the first channel of the depth and mono-depth
 * files divided by depth_scale and depth_scale * 5 as float64 arrays on the host; every consumer then casts to float32 and uploads) ----
 * out[v][u] = (float)((double)sample / divisor): the float64 division followed by the cast, as lvdgs.dataset.convert_depth_host
 * states it on the host.  The sample of pixel (u, v) lies at src + v * src_row_bytes + u * pixel_stride: an unsigned byte
 * (LVDGS_DEPTH_SAMPLE_BYTE) or an unsigned 16-bit word in the machine's byte order (LVDGS_DEPTH_SAMPLE_WORD).  pixel_stride is in
 * bytes: 1 for a byte plane, 3 for the first channel of a frame's colour bytes already on the device (a dataset whose depth path is
 * its colour path), 2 for a 16-bit plane; any stride not below the sample's size is taken.  The call reads no byte outside the
 * height rows of width * pixel_stride bytes each, and writes height*width floats without a row gap.  One launch, no host wait, no
 * copy; out needs float alignment only (16-byte stores are used where it has 16).  Two calls give the same bytes.
 * LVDGS_E_INVALID, before anything is enqueued: args / src / out NULL, width or height not > 0, a divisor that is zero or not
 * finite, an unknown sample_type, pixel_stride below the sample's size, src_row_bytes < width * pixel_stride, and for 16-bit samples
 * an odd src, an odd src_row_bytes or an odd pixel_stride.  LVDGS_E_RANGE: a raster beyond 2^31 workgroups. */
enum { LVDGS_DEPTH_SAMPLE_BYTE = 1, LVDGS_DEPTH_SAMPLE_WORD = 2 };
typedef struct lvdgs_ingest_depth_args {
    int32_t width, height;
    const void *src;              /* device: height rows of src_row_bytes           */
    int32_t sample_type;          /* LVDGS_DEPTH_SAMPLE_*                           */
    int32_t pixel_stride;         /* bytes from one pixel's sample to the next      */
    int64_t src_row_bytes;
    double divisor;
    float *out;                   /* out height*width                               */
} lvdgs_ingest_depth_args;
int lvdgs_ingest_depth(const lvdgs_ingest_depth_args *a, void *stream);

/* ---- Frame evaluation: the per-frame block of eval_rendering (reference utils/eval_utils_0806.py:216-312: two boolean masks, four
 * boolean gathers, two PSNRs, two SSIMs, and a copy of both images and the depth to the host for the 8-bit images it saves) ----
 * One call per rendered frame, enqueued on the caller's stream: no host wait, no copy.  render, gt_image: 3*height*width float32
 * (render unclamped, gt_image in [0, 1]); static_mask: height*width bytes (non-0 = static) or NULL; bg: 3 floats or NULL (= 0); depth:
 * height*width float32 or NULL.  Element by element, for channel c and pixel p, all float32 unless said otherwise, no contraction:
 *   a = min(max(render, 0), 1);   basic = gt > 0 (per channel element);   keep = basic & (static_mask[p] != 0)
 *   sum_sq_full = sum over basic of (a - gt) * (a - gt);  n_basic = |basic|;   sum_sq_static, n_keep: the same over keep.
 *     Each difference and square is float32; the sums are float64, taken per 32x32 tile of a plane by its workgroup (its waves'
 *     butterfly sums, the waves from 0 up) and then over the workgroups by one finishing workgroup (thread t takes partials t, t + 512,
 *     ...): a fixed order, no float atomics; the counts are integers.  PSNR is the caller's 10 log10(n / sum).
 *   ssim_full = mean over the 3*height*width elements of m(a, gt): SSIM as lvdgs_ssim_l1 states it -- 11 taps, sigma 1.5, the float32
 *     window g[k] = exp(-(k - 5)^2 / 4.5) divided by (float)(the float64 sum of the eleven g[k]) = 3.75923276, which is torch's g.sum(), zero padding, A = w*x, B = w*y, S = w*(x^2 + y^2), Z = w*(xy) by fmaf chains,
 *     m = ((2AB + C1)(2(Z - AB) + C2)) * (rcp(A^2 + B^2 + C1) * rcp(S - (A^2 + B^2) + C2)), C1 = 0.01^2, C2 = 0.03^2 -- each m float32,
 *     their sum float64 in the order above, divided by the count in float64.
 *   ssim_static = the same mean of m(a', gt') with a'[c][p] = keep[c][p] ? a[c][p] : bg[c], gt'[c][p] = keep[c][p] ? gt[c][p] : bg[c]:
 *     the mask is per channel element, which the single-plane keep_mask of lvdgs_ssim_l1 cannot express.
 *   static_mask NULL: keep = basic; the static quantities are not computed and the row reports them equal to the full ones.
 *   depth_min, depth_max: over the frame (fminf / fmaxf; non-finite depth is the caller's precondition and is not handled).
 * The row (64 bytes, written by the finishing launch to the DEVICE address out_row; the caller owns a table of them and reads it
 * when it likes):
 *   double sum_sq_full, sum_sq_static; uint64 n_basic, n_keep; double ssim_full, ssim_static; float depth_min, depth_max (0 without
 *   depth); uint32 flags (LVDGS_FRAME_EVAL_HAS_MASK, _HAS_DEPTH, _DEPTH_CONSTANT); uint32 reserved (0).
 * Optional byte outputs (each pointer may be NULL), what the reference hands to Image.fromarray:
 *   pred8, gt8, residual8: height*width*3 interleaved;  pred8 = (uint8)(a * 255.0f), gt8 = (uint8)(gt * 255.0f), a float32 product
 *     truncated;  residual8 = |pred8 - gt8|.
 *   depth8: height*width;  (uint8)(((d - depth_min) / (depth_max - depth_min)) * 255.0f), float32 in that order with an IEEE-rounded
 *     division.  A third launch of the same call reads the extrema from the row on the device.
 *   A constant depth map: the reference divides by zero and casts NaN to uint8, which is undefined.  BY DEFINITION the library writes
 *     depth8 = 0 everywhere and sets LVDGS_FRAME_EVAL_DEPTH_CONSTANT in the row.
 * Launches: one over 32x32 tiles x 3 planes (sums, counts, both SSIM sums, extrema, colour bytes), the finishing one, and depth8's
 * when asked for.  scratch: the bytes lvdgs_frame_eval_scratch_bytes gives (0: a size not > 0), no initialisation needed.
 * out_row and scratch hold doubles: both must be 8-byte aligned.
 * LVDGS_E_INVALID, before anything is enqueued: args NULL, width or height not > 0, render / gt_image / out_row / scratch NULL, depth8
 * without depth, scratch too small, out_row or scratch not 8-byte aligned.  LVDGS_E_RANGE: more than 65535 tile rows, or more than
 * 2^31 - 1 workgroups (tiles x 3). */
enum { LVDGS_FRAME_EVAL_HAS_MASK = 1, LVDGS_FRAME_EVAL_HAS_DEPTH = 2, LVDGS_FRAME_EVAL_DEPTH_CONSTANT = 4 };
typedef struct lvdgs_frame_eval_row {
    double sum_sq_full, sum_sq_static;
    uint64_t n_basic, n_keep;
    double ssim_full, ssim_static;
    float depth_min, depth_max;
    uint32_t flags;
    uint32_t reserved;
} lvdgs_frame_eval_row;
typedef struct lvdgs_frame_eval_args {
    int32_t width, height;
    const float *render;          /* 3*height*width, unclamped                      */
    const float *gt_image;        /* 3*height*width in [0, 1]                       */
    const uint8_t *static_mask;   /* height*width, non-0 = static, or NULL          */
    const float *bg;              /* 3, or NULL: 0                                  */
    const float *depth;           /* height*width, or NULL                          */
    void *out_row;                /* device: one lvdgs_frame_eval_row               */
    uint8_t *pred8;               /* out height*width*3, or NULL                    */
    uint8_t *gt8;                 /* out height*width*3, or NULL                    */
    uint8_t *residual8;           /* out height*width*3, or NULL                    */
    uint8_t *depth8;              /* out height*width, or NULL; needs depth         */
    void *scratch; size_t scratch_bytes;
} lvdgs_frame_eval_args;
size_t lvdgs_frame_eval_scratch_bytes(int32_t width, int32_t height);
int lvdgs_frame_eval(const lvdgs_frame_eval_args *a, void *stream);

/* ---- TSDF fusion of depth maps and a mesh by surface nets (what an Open3D-style ScalableTSDFVolume.integrate /
 * extract_triangle_mesh does on the host, after a copy of every depth map and image) ----
 * THE VOLUME: nx*ny*nz samples at the lattice points p[a] = origin[a] + voxel_size * (float)i_a (one float32 product, one float32
 * sum), linear index s = i + nx * (j + ny * k) in int64, in caller-owned planes: tsdf and weight, float32, and optionally r, g, b,
 * float32 running means (all three or none).  A zeroed block is an empty volume; there is no clear call.
 *
 * lvdgs_tsdf_integrate applies, to every voxel, views[0 .. count-1] in list order (count 0: nothing to do; at most
 * LVDGS_TSDF_MAX_VIEWS).  A view: width, height; fx, fy, cx, cy; R (9, row-major) and T (3) ON THE DEVICE, p_c = R p_w + T as for
 * lvdgs_seed_points; depth, height*width float32; image, 3*height*width planar float32, or NULL; mask, height*width bytes, non-0 =
 * use, or NULL; depth_min, depth_trunc (may be +inf).  Per voxel and view, all float32, evaluated as written, no contraction:
 *   1. x = ((R[0]*px + R[1]*py) + R[2]*pz) + T[0],  y and z alike with rows 1 and 2.  Skip unless z > depth_min.
 *   2. u = fx * (x / z) + cx,  v = fy * (y / z) + cy;  uf = floorf(u + 0.5f), vf alike.  Skip unless 0 <= uf < width and
 *      0 <= vf < height (float comparisons: a NaN or a value beyond int32 skips);  ui = (int)uf, vi = (int)vf.
 *   3. d = depth[vi*width + ui].  Skip unless d > 0 && d <= depth_trunc (NaN fails), and unless mask is NULL or mask[vi*width+ui] != 0.
 *   4. sdf = d - z.  Skip if sdf < -trunc.  t = fminf(1.0f, sdf / trunc).
 *   5. w1 = w + 1.0f;  tsdf = (tsdf * w + t) / w1;  with an image, per colour plane c = (c * w + image[ch][vi][ui]) / w1 (the colour
 *      as it is, not clamped; a view without an image leaves the colour planes alone);  w = fminf(w1, max_weight).
 * One thread owns four voxels along x and keeps them in registers across the views: the planes are read and written once per call
 * (16 bytes per lane when nx is a multiple of 4 and the planes are 16-byte aligned, element by element otherwise; rows that no
 * view changes are not written back).  A workgroup owns a brick of 64 x 4 x 4 voxels and first decides, per view, from the
 * brick's eight corner voxels alone whether the view can touch it: not when every z is at or below depth_min, when every z lies
 * beyond depth_trunc + trunc, or -- for a brick wholly in front of the camera -- when all of it projects left of, right of, above
 * or below the image; each test carries a margin above the rounding of steps 1 and 2, so only voxels the rule skips are skipped,
 * and a brick no view can touch is not read.  No atomics: two calls give the same bytes.  One launch, no host wait, no copy.
 * Before the launch -- LVDGS_E_INVALID: vol, its tsdf or weight NULL, r, g, b neither all set nor all NULL, views NULL with count >
 * 0, a view, its R, T or depth NULL, count outside 0 .. LVDGS_TSDF_MAX_VIEWS, an image on a volume without colour planes;
 * LVDGS_E_RANGE: a dimension below 1, more than 2^31 - 1 samples, ny or nz beyond 262140 (65535 bricks), voxel_size, trunc or
 * max_weight not finite and > 0, a view's width or height below 1 or more than 2^31 - 1 pixels.
 *
 * lvdgs_tsdf_mesh: surface nets over the same planes.  A sample is OBSERVED when weight > 0 and INSIDE when tsdf < 0.  Cell (i, j, k),
 * i < nx-1, j < ny-1, k < nz-1, with the samples (i+dx, j+dy, k+dz) as corners, is ACTIVE when all eight are observed and they are
 * not all on one side.
 *   Vertex of an active cell: over its 12 edges in the order x edges (dy,dz) = (0,0) (1,0) (0,1) (1,1), y edges (dx,dz) = (0,0) (1,0)
 *   (0,1) (1,1), z edges (dx,dy) = (0,0) (1,0) (0,1) (1,1), each from its low end f0 to its high end f1: where the ends differ in
 *   side, q = f0 / (f0 - f1), the crossing is the low corner's offset with q added along the edge's axis, and its colour is
 *   c0 + q * (c1 - c0) per plane.  The three coordinates and three colours are summed in that order starting from 0.0f and divided
 *   by (float)(the number of crossings);  position[a] = origin[a] + voxel_size * ((float)cell_a + mean[a]).  Vertices are numbered in
 *   the order of their cells' low-corner sample index s.
 *   Faces: for the lattice edge from sample (i, j, k) to its neighbour along axis a, (a, b, c) a cyclic permutation of (x, y, z),
 *   whose ends differ in side and whose four surrounding cells -- the sample's coordinates with (b, c) offset by c0 = (-1,-1),
 *   c1 = (0,-1), c2 = (0,0), c3 = (-1,0) -- exist and are active: the low end inside gives (c0,c1,c2), (c0,c2,c3), otherwise
 *   (c0,c2,c1), (c0,c3,c2), as vertex numbers (int32); normals point from inside to outside.  Faces are ordered by s, within a
 *   sample by axis x, y, z, the two triangles as written.
 * Launches, enqueued at once: classify (a byte per sample: active, inside, observed; vertices per span of samples), the edges (a
 * byte per sample; faces per span), one workgroup's scan of both counts, the vertices with the cell-to-vertex numbers in scratch,
 * the faces, and the publish.  No atomic decides a position: two calls give the same bytes.  vertices, colors: vertex_capacity*3
 * float32 (colors NULL: none; it needs the volume's colour planes); faces: face_capacity*3 int32.  Rows beyond a capacity are
 * not written -- nothing behind capacity*3 elements is touched -- and the counts reported are the exact ones, so one retry sized
 * by them succeeds.  host_state: a host block ("Host blocks" above) of LVDGS_TSDF_HOST_BYTES bytes: [LVDGS_TSDF_SEQ] the call's
 * `seq`, the tag; [_N_VERTICES]; [_N_FACES], saturated at 2^31 - 1; [_OVERFLOW] bit 0: more vertices than vertex_capacity, bit 1:
 * more faces than face_capacity, bit 2: more than 2^31 - 1 faces (no retry can hold them); zeros after it.  scratch: the bytes
 * lvdgs_tsdf_mesh_scratch_bytes gives (0: the size is refused), no initialisation needed.
 * Before any launch -- LVDGS_E_INVALID: args, tsdf, weight, vertices, faces, host_state or scratch NULL, r, g, b neither all set nor
 * all NULL, colors without colour planes, scratch too small; LVDGS_E_RANGE: a dimension below 2, more than 2^31 - 1 samples,
 * voxel_size not finite and > 0, a negative capacity. */
#define LVDGS_TSDF_MAX_VIEWS 16
#define LVDGS_TSDF_HOST_BYTES 64
enum {
    LVDGS_TSDF_SEQ = 0,
    LVDGS_TSDF_N_VERTICES = 1,
    LVDGS_TSDF_N_FACES = 2,
    LVDGS_TSDF_OVERFLOW = 3
};
typedef struct lvdgs_tsdf_volume {
    int32_t nx, ny, nz;
    float origin[3];
    float voxel_size, trunc, max_weight;   /* lvdgs_tsdf_mesh reads voxel_size only  */
    float *tsdf, *weight;         /* nx*ny*nz each                                  */
    float *r, *g, *b;             /* nx*ny*nz each, or all NULL: no colour          */
} lvdgs_tsdf_volume;
typedef struct lvdgs_tsdf_view {
    int32_t width, height;
    float fx, fy, cx, cy;
    float depth_min, depth_trunc;
    const float *R, *T;           /* 9 row-major and 3, on the device               */
    const float *depth;           /* height*width                                   */
    const float *image;           /* 3*height*width planar, or NULL                 */
    const uint8_t *mask;          /* height*width, non-0 = use, or NULL             */
} lvdgs_tsdf_view;
typedef struct lvdgs_tsdf_mesh_args {
    lvdgs_tsdf_volume vol;
    uint32_t seq;
    int32_t vertex_capacity, face_capacity;   /* rows the outputs hold               */
    float *vertices;              /* out vertex_capacity*3                          */
    float *colors;                /* out vertex_capacity*3, or NULL                 */
    int32_t *faces;               /* out face_capacity*3                            */
    int32_t *host_state;          /* LVDGS_TSDF_HOST_BYTES, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_tsdf_mesh_args;
int lvdgs_tsdf_integrate(const lvdgs_tsdf_volume *vol, const lvdgs_tsdf_view *const *views, int32_t count, void *stream);
size_t lvdgs_tsdf_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int lvdgs_tsdf_mesh(const lvdgs_tsdf_mesh_args *a, void *stream);

/* ---- Block-sparse TSDF volume: the fusion rule and the surface nets of "TSDF fusion" on an unbounded lattice of which only the
 * blocks near a surface are stored (what an Open3D-style ScalableTSDFVolume keeps in a host hash map) ----
 * THE LATTICE: samples at p[a] = origin[a] + voxel_size * (float)g_a, g a SIGNED global index (one float32 product, one float32 sum,
 * as for the dense volume).  A BLOCK is 8 x 8 x 8 samples: block coordinate b_a = floor(g_a / 8), each in [-2^20, 2^20), local
 * index l = i + 8 * (j + 8 * k) with g_a = 8 * b_a + (i, j, k)_a.  THE KEY of a block, never 0:
 *   key = 1 << 63 | (uint64)(bz + 2^20) << 42 | (uint64)(by + 2^20) << 21 | (uint64)(bx + 2^20)      -- ascending key = ascending (bz, by, bx).
 * STORAGE, all caller-owned, on the device, and an empty volume when zeroed (there is no clear call): a pool of pool_blocks blocks
 * in planes tsdf, weight and optionally r, g, b (all three or none), pool_blocks * 512 float32 each, block p at [512 p, 512 p + 512);
 * block_key, pool_blocks int64 (the key of pool block p, 0: unused; a key is negative as an int64, so a signed ascending sort puts
 * the unused entries last); an open-addressing table of table_slots (a power of two, >= 2 * pool_blocks) 64-bit keys and int32
 * values (key 0: empty slot; value: the pool index, or -1 for a key that found the pool exhausted -- ABSENT to every reader), probed
 * linearly from (mix(key) & (table_slots - 1)), mix = MurmurHash3's 64-bit finalizer; and a header of LVDGS_TSDF_BLOCKS_HEADER_WORDS
 * int32: [_HEADER_USED] blocks in use, [_HEADER_DROPPED] keys entered with -1, [_HEADER_OUT_OF_RANGE] samples skipped for their
 * coordinate (wraps at 2^32), [_HEADER_FLAGS] bit 0 (LVDGS_TSDF_BLOCKS_TABLE_FULL): a key found no slot.  Every kernel brings what it
 * reads from the header, from `order` and from the table into range before it indexes with it.
 *
 * lvdgs_tsdf_blocks_integrate(vol, views, count): views as for lvdgs_tsdf_integrate.  Three launches, no host wait, no copy.
 * ALLOCATION, for every view and every pixel (ui, vi), a thread each; all float32 as written, no contraction:
 *   1. d = depth[vi*width + ui].  Skip unless d > 0 && d <= depth_trunc, and unless mask is NULL or mask[vi*width + ui] != 0.
 *   2. The host computes, in float32, n_steps = 2 * (int)ceilf((trunc + voxel_size) / (0.5f * voxel_size)) + 1 (refused above
 *      LVDGS_TSDF_BLOCKS_MAX_STEPS) and step = 0.5f * voxel_size.
 *   3. For s = 0 .. n_steps-1:  zs = (d - (float)(n_steps / 2) * step) + (float)s * step;  skip the sample unless zs > depth_min;
 *      xc = ((float)ui - cx) / fx * zs,  yc = ((float)vi - cy) / fy * zs;  q = (xc - T[0], yc - T[1], zs - T[2]);
 *      p[a] = ((R[0*3+a] * q[0] + R[1*3+a] * q[1]) + R[2*3+a] * q[2])  (R^T q);  c[a] = floorf((p[a] - origin[a]) / (8.0f * voxel_size)).
 *      Unless -1048576.0f <= c[a] < 1048576.0f for every a (a NaN fails) the sample is skipped and counted in [_HEADER_OUT_OF_RANGE].
 *      Otherwise b = (int)c and the block is inserted if it is absent (a lane does not probe for the key of its previous sample).
 *   A key is entered by a 64-bit atomicCAS on the slot's key -- the only atomic that decides anything; the winner takes the next
 *   pool index from a counter and then writes the slot's value and block_key[index], or -1 and one count of [_HEADER_DROPPED] when
 *   the pool is exhausted: exact while the table has room; a key that finds every slot taken sets TABLE_FULL.  The values are read
 *   by later launches only.  Which pool index a block gets is not part of the contract; the SET of blocks is, while none is dropped.
 * INTEGRATION: every sample of every block in use -- those of earlier calls and those of this call -- gets steps 1-5 of "TSDF
 * fusion", views in list order: the dense rule on the global lattice restricted to the allocated blocks, the free-space updates
 * inside them included.  A block allocated by a later call starts from zero at that call.  One workgroup of 256 threads per block,
 * a thread owns the samples l and l + 256 and keeps them in registers across the views; per view the block's eight corner samples
 * decide (brick_may_touch, the dense kernel's test, one lane per view and a ballot) whether the view is walked; planes are read
 * once and written once, when a view changed them.  No atomics on plane data.
 * Before any launch -- LVDGS_E_INVALID: vol, tsdf, weight, block_key, table_keys, table_values or header NULL, r, g, b neither all
 * set nor all NULL, views NULL with count > 0, a view, its R, T or depth NULL, count outside 0 .. LVDGS_TSDF_MAX_VIEWS, an image on a
 * volume without colour planes; LVDGS_E_RANGE: pool_blocks outside 1 .. LVDGS_TSDF_BLOCKS_MAX_POOL, table_slots not a power of two,
 * below 2 * pool_blocks or above 2^30, voxel_size, trunc or max_weight not finite and > 0, more than LVDGS_TSDF_BLOCKS_MAX_STEPS
 * steps, a view's width or height below 1 or more than 2^31 - 1 pixels.
 *
 * lvdgs_tsdf_blocks_mesh: surface nets with the definitions of lvdgs_tsdf_mesh -- observed, inside, active cell, vertex, colour,
 * faces, winding -- on the global lattice; a sample of a block that is not in use is UNOBSERVED, so cells and faces cross block
 * borders through the neighbours' samples.  position[a] = origin[a] + voxel_size * ((float)g_a + mean[a]), g the cell's low corner.
 * Only cells with cell_lo[a] <= g_a < cell_hi[a] for every a can be active (INT32_MIN and INT32_MAX: all of them): with cell_lo = 0
 * and cell_hi = n - 1 the mesh is that of a dense volume of n samples per axis on the same lattice.
 * `order`: pool_blocks int32 on the device, the pool indices sorted by ascending key, the blocks in use first (plumbing: a sort of
 * block_key).  Vertices are ordered by (block in `order`, l of the cell's low corner), faces by (block in `order`, l, axis x, y, z),
 * the two triangles as written.  No atomic decides a position: two calls give the same bytes.  Launches, enqueued at once: the rank
 * of every pool block; the 27 neighbours of every block by table lookup; classify per block (the block and its +1 shell, 9^3
 * samples, in LDS: a 512-bit mask of active cells and their count); the edges (a byte per sample, the face count per block); one
 * workgroup's scan of both counts over the blocks; the vertices (a cell's vertex number = its block's base + the active cells of
 * the mask below l); the faces; the publish.  Capacities, rows beyond them and the retry: as for lvdgs_tsdf_mesh.  host_state: a
 * host block of LVDGS_TSDF_BLOCKS_HOST_BYTES bytes: [LVDGS_TSDF_BLOCKS_SEQ] the call's `seq`, the tag; [_N_VERTICES]; [_N_FACES],
 * saturated at 2^31 - 1; [_OVERFLOW], the bits of [LVDGS_TSDF_OVERFLOW]; [_USED], [_DROPPED], [_OUT_OF_RANGE], [_FLAGS]: the header;
 * zeros after it.  scratch: the bytes lvdgs_tsdf_blocks_mesh_scratch_bytes(pool_blocks) gives (0: refused), 8-byte aligned, no
 * initialisation needed.
 * Before any launch -- as for the integration, and LVDGS_E_INVALID: args, order, vertices, faces, host_state or scratch NULL, colors
 * without colour planes, scratch too small or misaligned; LVDGS_E_RANGE: a negative capacity.
 *
 * lvdgs_tsdf_blocks_rehash(vol): enters block_key[0 .. used-1] with their indices into vol's table, which the caller has zeroed (a
 * larger one, after the planes and keys were copied into a larger pool); keys that were dropped are forgotten: [_HEADER_DROPPED]
 * and [_HEADER_FLAGS] are reset.  One launch, no wait.  Refusals: those of the integration that concern vol. */
#define LVDGS_TSDF_BLOCKS_HEADER_WORDS 8
#define LVDGS_TSDF_BLOCKS_HOST_BYTES 64
#define LVDGS_TSDF_BLOCKS_MAX_POOL 4194304
#define LVDGS_TSDF_BLOCKS_MAX_STEPS 1025
enum {
    LVDGS_TSDF_BLOCKS_HEADER_USED = 0,
    LVDGS_TSDF_BLOCKS_HEADER_DROPPED = 1,
    LVDGS_TSDF_BLOCKS_HEADER_OUT_OF_RANGE = 2,
    LVDGS_TSDF_BLOCKS_HEADER_FLAGS = 3
};
enum { LVDGS_TSDF_BLOCKS_TABLE_FULL = 1 };
enum {
    LVDGS_TSDF_BLOCKS_SEQ = 0,
    LVDGS_TSDF_BLOCKS_N_VERTICES = 1,
    LVDGS_TSDF_BLOCKS_N_FACES = 2,
    LVDGS_TSDF_BLOCKS_OVERFLOW = 3,
    LVDGS_TSDF_BLOCKS_USED = 4,
    LVDGS_TSDF_BLOCKS_DROPPED = 5,
    LVDGS_TSDF_BLOCKS_OUT_OF_RANGE = 6,
    LVDGS_TSDF_BLOCKS_FLAGS = 7
};
typedef struct lvdgs_tsdf_blocks {
    int32_t pool_blocks, table_slots;
    float origin[3];
    float voxel_size, trunc, max_weight;
    float *tsdf, *weight;         /* pool_blocks*512 each                           */
    float *r, *g, *b;             /* pool_blocks*512 each, or all NULL: no colour   */
    int64_t *block_key;           /* pool_blocks                                    */
    uint64_t *table_keys;         /* table_slots                                    */
    int32_t *table_values;        /* table_slots                                    */
    int32_t *header;              /* LVDGS_TSDF_BLOCKS_HEADER_WORDS, on the device  */
} lvdgs_tsdf_blocks;
typedef struct lvdgs_tsdf_blocks_mesh_args {
    lvdgs_tsdf_blocks vol;
    uint32_t seq;
    int32_t vertex_capacity, face_capacity;   /* rows the outputs hold               */
    int32_t cell_lo[3], cell_hi[3];           /* cells with cell_lo <= g < cell_hi   */
    const int32_t *order;         /* pool_blocks: pool indices by ascending key     */
    float *vertices;              /* out vertex_capacity*3                          */
    float *colors;                /* out vertex_capacity*3, or NULL                 */
    int32_t *faces;               /* out face_capacity*3                            */
    int32_t *host_state;          /* LVDGS_TSDF_BLOCKS_HOST_BYTES, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_tsdf_blocks_mesh_args;
int lvdgs_tsdf_blocks_integrate(const lvdgs_tsdf_blocks *vol, const lvdgs_tsdf_view *const *views, int32_t count, void *stream);
size_t lvdgs_tsdf_blocks_mesh_scratch_bytes(int32_t pool_blocks);
int lvdgs_tsdf_blocks_mesh(const lvdgs_tsdf_blocks_mesh_args *a, void *stream);
int lvdgs_tsdf_blocks_rehash(const lvdgs_tsdf_blocks *vol, void *stream);

/* ---- Mesh scoring: area-weighted samples of a mesh and exact nearest neighbours between two clouds (what NICE-SLAM's eval_recon
 * does with trimesh.sample.sample_surface and a SciPy KD-tree on the host, after copying both meshes there) ----
 * lvdgs_mesh_sample draws num_samples points from (vertices (V,3) float32, faces (F,3) int32).  A function of (mesh, seed, sample
 * index) alone: no generator state, the same bytes on every call.  In the order evaluated:
 *   1. Area of face f with corners a, b, c = vertices[faces[f][0..2]], float64 from the float32 coordinates, no contraction:
 *      e1 = b - a, e2 = c - a;  n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);  A_f = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz).
 *      A face with an index outside 0 .. V-1, or whose A_f is not finite and > 0, has weight 0 (A_f := 0).
 *   2. A_max = the maximum of the A_f (order-free).  q_f = (uint64) floor(A_f / A_max * 4294967296.0), float64: the largest face
 *      gets 2^32, a weighted face may get 0 when it is 2^32 times smaller.  n_weighted = |{f: A_f > 0}|.
 *   3. prefix[f] = q_0 + ... + q_f in uint64 (integers: exact in any order);  total = prefix[F-1] < 2^63.
 *   4. Sample k:  k_j = key(3k + j), j = 0, 1, 2, with i = 3k + j in uint64 and seeding's fmix32:
 *        key(i) = fmix32( fmix32((uint32)i + seed_lo) ^ (seed_hi + (uint32)(i >> 32)) ),   seed = seed_hi:seed_lo.
 *      t = (uint64)(((k_0 << 32 | k_1) * total) >> 64) (the high half of the 128-bit product);  face = the first f with prefix[f] > t
 *      (a face with q_f = 0 is never chosen);  u1 = k_2 >> 8,  u2 = k_1 & 0xFFFFFF (the low bits of k_1 move t by less than one
 *      part in 2^32 of a face's interval);  if (u1 + u2 > 2^24) { u1 = 2^24 - u1; u2 = 2^24 - u2; } -- the fold, in integers, so
 *      that no rounding of a sum decides it;  r1 = (float)u1 * 2^-24,  r2 = (float)u2 * 2^-24, both exact;
 *      point[x] = (a[x] + r1 * (b[x] - a[x])) + r2 * (c[x] - a[x]) in float32 as written, y and z alike; colors, when vertex_colors
 *      is given, by the same expression over the corners' colours;  face_index[k] = face.
 * Outputs: points num_samples*3 float32; face_index num_samples int32 or NULL; colors num_samples*3 float32 or NULL (needs
 * vertex_colors, V*3 float32).  info: the DEVICE address of one lvdgs_mesh_sample_info, 16 bytes: flags (LVDGS_MESH_SAMPLE_NO_AREA:
 * no face has a positive weight -- nothing is sampled, points / face_index / colors are left untouched), n_weighted, total.
 * Five launches, enqueued at once: areas with a maximum per span of faces, the weights with a sum per span, one workgroup's scan of
 * the spans, the prefix (one workgroup scan per 256 faces, seeding's ordered compaction), the samples (a binary search each).  No
 * atomics, no host wait, no copy.  scratch: the bytes lvdgs_mesh_sample_scratch_bytes(num_faces) gives (0: the size is refused), 8-byte
 * aligned, no initialisation needed.  num_samples == 0: nothing to do.
 * Before any launch -- LVDGS_E_INVALID: args, vertices, faces, points, info or scratch NULL; colors without vertex_colors; a negative
 * count; num_vertices, num_faces or num_samples above 2^31 - 1; num_faces == 0; scratch too small or misaligned.
 *
 * lvdgs_cloud_distance: for each of num_queries points q_i the nearest of num_reference points r_j, EXACTLY:
 *   d2_i = min over j of ((dx*dx + dy*dy) + dz*dz),  dx = q_i[x] - r_j[x], dy, dz alike, float32 as written, no contraction;
 *   idx_i = the lowest j that attains it.
 * A reference point with a non-finite coordinate never wins.  A query with a non-finite coordinate gets d2 = +inf, idx = -1 and is
 * SKIPPED; with no usable reference point every query is skipped and LVDGS_CLOUD_DISTANCE_NO_REFERENCE is set.  Every other query
 * is COUNTED.  The result does not depend on the grid below, on points_per_cell or on the order atomics arrive in.
 * How it is found: the usable reference points' bounding box (a reduction), a uniform grid over it whose resolution one thread
 * decides on the device from their number, the box, points_per_cell (<= 0: LVDGS_CLOUD_DISTANCE_POINTS_PER_CELL) and the cell
 * budget of the scratch, at most LVDGS_CLOUD_DISTANCE_MAX_DIM cells along an axis; a counting sort of the reference points and of
 * the queries (a query outside the box goes to the nearest cell) by cell -- integer atomic counts, workgroup scans, scatter.  A
 * workgroup of one wave then takes one cell's queries and stages the reference points of the cell's 3 x 3 x 3 neighbourhood in LDS,
 * 512 (8 KiB) at a time, once for up to 64 queries.  A query whose best is not below the neighbourhood's reach goes on alone: planes of
 * cells outward from its own, rows outward within a plane, the row's run of cells that can still hold a nearer point.  A cell, row
 * or plane is skipped only when it holds no point, or when L * 0.99999f > best, L = the float32 sum of squares of its per-axis gaps
 * to the query, each gap taken to the cell's planes moved outward by slop[a] = h[a] / 256 + 1e-6f * (|lo[a]| + |hi[a]|): the cell
 * index of a point, (p[a] - lo[a]) * (n[a] / extent[a]) truncated and clamped, is off by less than 1024 * 3 * 2^-24 < 1/256 of a
 * cell, the planes lo[a] + c * h[a] by less than 3 * 2^-24 of |lo| + |hi|, and the per-point expression and L by less than 6 * 2^-24
 * relative together -- so a skipped point's d2 is above the best, never equal to it.
 * Outputs: d2 num_queries float32 or NULL; idx num_queries int32 or NULL; out_row: the DEVICE address of one lvdgs_cloud_distance_row,
 * LVDGS_CLOUD_DISTANCE_ROW_BYTES bytes of the caller's table, written by the finishing launch:
 *   sum_distance = the float64 sum of (double)sqrtf(d2) over the counted queries, sum_squared = of (double)d2, in a fixed order
 *   (thread t of workgroup b takes queries b * chunk + t, + 256, ...; butterfly sums of the waves, the waves from 0 up, then thread
 *   t of one finishing workgroup takes partials t, t + 256, ...): two calls give the same bits;  n_counted, n_skipped;
 *   n_below[t] = |{counted: sqrtf(d2) < thresholds[t]}| for t < num_thresholds (0 beyond);  max_distance = the largest sqrtf(d2)
 *   (0 when nothing is counted);  flags;  n_reference = the usable reference points;  reserved (0).
 * num_queries == 0: nothing to do, the row is not written.  scratch: the bytes lvdgs_cloud_distance_scratch_bytes(num_queries,
 * num_reference) gives (0: a count is refused), 16-byte aligned, no initialisation needed; out_row 8-byte aligned.  No host wait,
 * no copy.
 * Before any launch -- LVDGS_E_INVALID: args, queries, out_row or scratch NULL, reference NULL with num_reference > 0; a negative
 * count or one above 2^31 - 1; num_thresholds outside 0 .. LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS; a threshold not finite and >= 0;
 * scratch too small or misaligned. */
#define LVDGS_MESH_SAMPLE_INFO_BYTES 16
#define LVDGS_CLOUD_DISTANCE_ROW_BYTES 64
#define LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS 4
#define LVDGS_CLOUD_DISTANCE_POINTS_PER_CELL 8
#define LVDGS_CLOUD_DISTANCE_MAX_DIM 1024
enum { LVDGS_MESH_SAMPLE_NO_AREA = 1 };
enum { LVDGS_CLOUD_DISTANCE_NO_REFERENCE = 1 };
typedef struct lvdgs_mesh_sample_info {
    uint32_t flags;
    uint32_t n_weighted;
    uint64_t total;
} lvdgs_mesh_sample_info;
typedef struct lvdgs_mesh_sample_args {
    int64_t num_vertices, num_faces, num_samples;
    uint64_t seed;
    const float *vertices;        /* num_vertices*3                                 */
    const int32_t *faces;         /* num_faces*3                                    */
    const float *vertex_colors;   /* num_vertices*3, or NULL                        */
    float *points;                /* out num_samples*3                              */
    int32_t *face_index;          /* out num_samples, or NULL                       */
    float *colors;                /* out num_samples*3, or NULL; needs vertex_colors */
    void *info;                   /* device: one lvdgs_mesh_sample_info             */
    void *scratch; size_t scratch_bytes;
} lvdgs_mesh_sample_args;
typedef struct lvdgs_cloud_distance_row {
    double sum_distance, sum_squared;
    uint32_t n_counted, n_skipped;
    uint32_t n_below[LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS];
    float max_distance;
    uint32_t flags;
    uint32_t n_reference;
    uint32_t reserved[3];
} lvdgs_cloud_distance_row;
typedef struct lvdgs_cloud_distance_args {
    int64_t num_queries, num_reference;
    const float *queries;         /* num_queries*3                                  */
    const float *reference;       /* num_reference*3                                */
    int32_t num_thresholds;
    int32_t points_per_cell;      /* <= 0: LVDGS_CLOUD_DISTANCE_POINTS_PER_CELL     */
    float thresholds[LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS];
    float *d2;                    /* out num_queries, or NULL                       */
    int32_t *idx;                 /* out num_queries, or NULL                       */
    void *out_row;                /* device: one lvdgs_cloud_distance_row           */
    void *scratch; size_t scratch_bytes;
} lvdgs_cloud_distance_args;
size_t lvdgs_mesh_sample_scratch_bytes(int64_t num_faces);
int lvdgs_mesh_sample(const lvdgs_mesh_sample_args *a, void *stream);
size_t lvdgs_cloud_distance_scratch_bytes(int64_t num_queries, int64_t num_reference);
int lvdgs_cloud_distance(const lvdgs_cloud_distance_args *a, void *stream);

/* Culling a mesh to what the evaluated frames observed, before it is scored (what NICE-SLAM-style evaluations do on the host with
 * trimesh and a Python loop over the frames, after copying the meshes and every depth map there).
 *
 * lvdgs_mesh_visibility marks the vertices that some view sees: seen, num_vertices bytes, IN AND OUT -- a byte that is non-0 on entry
 * is left as it is, a byte that is 0 becomes 1 when a view of this call sees the vertex (seen[v] |= ...): any number of frames goes
 * through in calls of up to LVDGS_TSDF_MAX_VIEWS views and the caller zeroes the plane once.  views: the lvdgs_tsdf_view of "TSDF
 * fusion" (R, T, depth, mask on the device; image is ignored), count 0 .. LVDGS_TSDF_MAX_VIEWS.  Per vertex p = (px, py, pz) and view,
 * all float32, evaluated as written, no contraction:
 *   - steps 1 and 2 of "TSDF fusion" as they stand: x, y, z, skip unless z > depth_min; u, v, uf, vf, skip unless the half-up pixel
 *     (ui, vi) lies inside the image;
 *   - a view with depth == NULL is FRUSTUM ONLY: the vertex is seen when z <= depth_trunc;
 *   - with a depth plane, d = depth[vi*width + ui] and the vertex is seen when the tests of steps 3 and 4 hold with occlusion_eps in
 *     the place of trunc: d > 0 && d <= depth_trunc, mask NULL or mask[vi*width + ui] != 0, and !(d - z < -occlusion_eps) -- the
 *     condition under which a fusion with the truncation distance occlusion_eps would have updated a voxel at p.
 * A vertex with a non-finite coordinate is never seen: a NaN makes z a NaN, an infinity makes x, y and z each infinite or NaN, and
 * then either z > depth_min fails or x / z is a NaN and the float comparisons of step 2 fail.
 * One thread per vertex; the views are walked with their pose and intrinsics in scalar registers, a view is skipped by a whole wave
 * none of whose vertices passes steps 1 and 2, and a wave whose vertices are all seen stops.  One launch, no scratch, no atomics, no
 * host wait.  num_vertices == 0 or count == 0: nothing to do.
 * Before the launch -- LVDGS_E_INVALID: args NULL; a negative num_vertices or one above 2^31 - 1; count outside 0 ..
 * LVDGS_TSDF_MAX_VIEWS; vertices or seen NULL with num_vertices > 0; views NULL with count > 0; a view, its R or its T NULL;
 * LVDGS_E_RANGE: occlusion_eps not finite or negative; a view's width or height below 1 or more than 2^31 - 1 pixels.
 * THE FLOAT32 RULE AGAINST EXACT ARITHMETIC, u = 2^-24: x, y, z of step 1 are each within 4u * M of their exact values, M = |R0 px| +
 * |R1 py| + |R2 pz| + |T| of the row (three products and three sums, every partial sum at most M).  So the decision of a view can
 * differ from the one exact arithmetic takes only for a vertex that lies
 *   - within 4u Mz of z = depth_min, or (frustum only) of z = depth_trunc;
 *   - within 5u (Mz + |d|) of d - z = -occlusion_eps (z as above, and the difference rounds by u |d - z| <= u (|d| + Mz); d, the mask
 *     and occlusion_eps are float32 values that both read alike, so d > 0 and d <= depth_trunc never differ);
 *   - with u + 0.5 (v + 0.5) within  fx (4u Mx + |x / z| 4u Mz) / |z|  +  4u (|u| + |cx| + 1)  of an integer 0 .. width (height), a
 *     pixel edge: the quotient x / z inherits the errors of x and z and rounds once, the product with fx, the sum with cx and the sum
 *     with 0.5 round once each.
 * tests/test_mesh_cull.py excludes exactly those vertices, with the factors doubled, and requires equality on the rest.
 *
 * lvdgs_mesh_cull writes the kept part of a mesh (vertices (V,3) float32, vertex_colors (V,3) float32 or NULL, faces (F,3) int32) in
 * the original order.  seen: V bytes, non-0 = seen (lvdgs_mesh_visibility's plane, or any other).  A face is KEPT when all three of
 * its indices lie in 0 .. V-1 and, face_rule LVDGS_MESH_CULL_ALL: all three vertices are seen, LVDGS_MESH_CULL_ANY: at least one is.
 * A vertex is KEPT exactly when a kept face references it (under ANY that includes unseen vertices; a seen vertex that no kept face
 * references goes).  Kept vertices keep their relative order and so do kept faces; kept faces are rewritten through the old-to-new
 * vertex numbers.  Outputs, of the inputs' capacity, so that nothing can overflow: out_vertices V*3; out_colors V*3 or NULL (needs
 * vertex_colors); out_faces F*3; vertex_origin V int32 or NULL: the old index of each kept vertex; face_origin F int32 or NULL:
 * likewise.  Rows beyond the counts are not touched.  Coordinates and colours are copied bit for bit.
 * Launches, enqueued at once: a clear of the used-vertex plane; the face flags, the kept faces per span of faces and a plain store
 * of 1 per referenced vertex; the used vertices per span of vertices; one workgroup's scan of both counts; the vertices and colours,
 * with the old-to-new numbers in scratch; the faces; the publish.  No atomic decides a position: two calls give the same bytes.
 * host_state: a host block ("Host blocks" above) of LVDGS_MESH_CULL_HOST_BYTES bytes: [LVDGS_MESH_CULL_SEQ] the call's `seq`, the
 * tag; [_N_VERTICES]; [_N_FACES]; zeros after it.  scratch: the bytes lvdgs_mesh_cull_scratch_bytes(num_vertices, num_faces) gives
 * (0: a count is refused), no initialisation needed.  One wait, at the caller.
 * Before any launch -- LVDGS_E_INVALID: args NULL; a negative count or one above 2^31 - 1; a face_rule that is neither; vertices, seen
 * or out_vertices NULL with V > 0; faces or out_faces NULL with F > 0; host_state or scratch NULL; out_colors without vertex_colors;
 * scratch too small or not 4-byte aligned; an output that overlaps an input, the scratch or another output. */
#define LVDGS_MESH_CULL_HOST_BYTES 64
enum {
    LVDGS_MESH_CULL_SEQ = 0,
    LVDGS_MESH_CULL_N_VERTICES = 1,
    LVDGS_MESH_CULL_N_FACES = 2
};
enum {
    LVDGS_MESH_CULL_ALL = 0,
    LVDGS_MESH_CULL_ANY = 1
};
typedef struct lvdgs_mesh_visibility_args {
    int64_t num_vertices;
    const float *vertices;        /* num_vertices*3                                 */
    const lvdgs_tsdf_view *const *views;   /* count views; image ignored, depth may be NULL: frustum only */
    int32_t count;
    float occlusion_eps;          /* finite, >= 0                                   */
    uint8_t *seen;                /* in/out num_vertices                            */
} lvdgs_mesh_visibility_args;
typedef struct lvdgs_mesh_cull_args {
    int64_t num_vertices, num_faces;
    const float *vertices;        /* num_vertices*3                                 */
    const float *vertex_colors;   /* num_vertices*3, or NULL                        */
    const int32_t *faces;         /* num_faces*3                                    */
    const uint8_t *seen;          /* num_vertices, non-0 = seen                     */
    int32_t face_rule;            /* LVDGS_MESH_CULL_ALL or _ANY                    */
    uint32_t seq;
    float *out_vertices;          /* out num_vertices*3                             */
    float *out_colors;            /* out num_vertices*3, or NULL; needs vertex_colors */
    int32_t *out_faces;           /* out num_faces*3                                */
    int32_t *vertex_origin;       /* out num_vertices, or NULL                      */
    int32_t *face_origin;         /* out num_faces, or NULL                         */
    int32_t *host_state;          /* LVDGS_MESH_CULL_HOST_BYTES, pinned host (the host address) */
    void *scratch; size_t scratch_bytes;
} lvdgs_mesh_cull_args;
int lvdgs_mesh_visibility(const lvdgs_mesh_visibility_args *a, void *stream);
size_t lvdgs_mesh_cull_scratch_bytes(int64_t num_vertices, int64_t num_faces);
int lvdgs_mesh_cull(const lvdgs_mesh_cull_args *a, void *stream);

/* Depth and face indices rendered from a mesh: a triangle rasteriser with a depth buffer (what NICE-SLAM-style evaluations do on the
 * host with pyrender, after copying the mesh there, to cull a mesh against itself and to report a depth L1).
 *
 * lvdgs_mesh_depth renders views[0 .. count-1] (count 0 .. LVDGS_TSDF_MAX_VIEWS) of (vertices (V,3) float32, faces (F,3) int32).  A view
 * is the lvdgs_tsdf_view of "TSDF fusion": R and T on the device; depth, image and mask are ignored and may be NULL.  Per view v it
 * writes depth[v], height*width float32: the camera z of the nearest covering face, or 0.0f where no face covers (the "no depth"
 * every consumer of a depth plane here understands: d > 0), and, when face_index is not NULL, face_index[v], height*width int32: the
 * index of that face, or -1.  depth and face_index are HOST arrays of count device addresses; face_index NULL: no face planes,
 * otherwise every one of its entries is set.  All float32, evaluated as written, no contraction:
 *   VERTICES.  x, y, z of step 1 of "TSDF fusion"; u = fx * (x / z) + cx, v = fy * (y / z) + cy, the expressions of step 2, continuous
 *     and not rounded.  Pixel (i, j) has its centre at u = i, v = j (the half-up pixel of step 2 is the one whose centre is nearest).
 *     dm = fmaxf(depth_min, 0.0f) stands for depth_min throughout: the planes hold positive depths only.
 *   WHICH FACES TAKE PART.  Face f = (a0, a1, a2) takes part in a view when all three indices lie in 0 .. V-1; all three z > dm -- a
 *     face that crosses the near plane is dropped WHOLE, there is no clipping --; fabsf(u) < +inf and fabsf(v) < +inf for all three (u and v
 *     finite: a NaN fails); and its area is not 0:  ar = (u1 - u0) * (v2 - v0) - (v1 - v0) * (u2 - u0),  ar > 0 || ar < 0.  A vertex with a
 *     non-finite coordinate drops its faces by these comparisons failing, as in the visibility rule.
 *   PIXEL BOX.  lo = ceilf(fminf(fminf(u0, u1), u2)), hi = floorf(fmaxf(fmaxf(u0, u1), u2)); no pixel unless lo < (float)width && hi >=
 *     0.0f && lo <= hi (float comparisons first, as in step 2); then i runs from (lo > 0.0f ? (int)lo : 0) to (hi < (float)width ?
 *     (int)hi : width - 1), which is max(0, lo) .. min(width - 1, hi).  j alike from v and height.
 *   EDGE VALUES, watertight by construction.  The edge of a face between its vertices a and b: order the two by VERTEX INDEX, lo the
 *     smaller one (equal indices: either, the value is 0 both ways), and
 *         s = (u_hi - u_lo) * ((float)j - v_lo) - (v_hi - v_lo) * ((float)i - u_lo).
 *     The edge value is s when the face lists the edge as lo -> hi and -s otherwise (negation is exact).  E_k is the value of the
 *     edge opposite vertex k, listed as a1 -> a2, a2 -> a0, a0 -> a1 for k = 0, 1, 2.  The pixel is COVERED when all three E_k >= 0 or
 *     all three <= 0: both windings count and edges are inclusive (scene meshes have no reliable winding, and an occluder occludes
 *     from both sides).  Two faces that share an edge compute the same s for it, so at every pixel at least one of them passes
 *     that edge: a welded surface has no pinholes from rounding, and double coverage is harmless under a minimum.
 *   DEPTH of a covered pixel, perspective-correct (linear in 1/z):  A = (E0 + E1) + E2;  w_k = E_k / A;
 *         inv = (w0 * (1.0f / z0) + w1 * (1.0f / z1)) + w2 * (1.0f / z2);  zp = 1.0f / inv.
 *     The candidate is skipped unless zp > dm && zp <= depth_trunc (a NaN -- A == 0 gives one -- fails).
 *   WINNER.  The smallest zp; among equal zp the smallest face index.  One 64-bit key per pixel, (uint64)float_bits(zp) << 32 |
 *     (uint32)f -- the bits of positive floats order as unsigned integers --, reduced by an unsigned 64-bit atomic minimum in a
 *     scratch plane.  A minimum does not depend on arrival order: two calls give the same bytes.  It is the only atomic of the call
 *     and decides a value, never a position.
 * Launches, enqueued at once, no host wait, no copy: the fill of the scratch keys with all ones; the raster launch -- one lane owns
 * one face and loads its three vertices once per call; the views are walked with their pose and intrinsics in scalar registers, and
 * a view in which no face of a wave has a pixel box is skipped by the wave; a lane walks its own box while the box holds at most 16
 * pixels, a larger box is handed to the whole wave, one face at a time, whose 64 lanes walk it in tiles of 8 x 8 pixels (the result
 * does not depend on that threshold: it is a minimum); a plain load of the key in front of the atomic could skip a candidate that is not smaller (a stale
 * value is only ever larger, so the skip would be safe), but measured it costs more than it saves and is compiled out --; the resolve launch, which turns each key into the depth float and the face index, 0.0f and
 * -1 for an untouched key, and writes height*width elements per plane, nothing behind them.  num_faces == 0 or num_vertices == 0
 * still writes the empty planes.  scratch: the bytes lvdgs_mesh_depth_scratch_bytes(total_pixels) gives for the sum of height*width
 * over the views of the call -- 8 bytes per pixel, rounded up to a multiple of 256, of which the call needs the 8 per pixel -- (0: the size is refused: negative, or more than 2^31 - 1 pixels a view times
 * LVDGS_TSDF_MAX_VIEWS), 8-byte aligned, no initialisation needed.
 * Before any launch -- LVDGS_E_INVALID: args NULL; a negative count or one above 2^31 - 1; vertices NULL with V > 0, faces NULL with
 * F > 0; count outside 0 .. LVDGS_TSDF_MAX_VIEWS; views or depth NULL with count > 0; a view, its R, its T or its depth output
 * NULL; a face_index list with a NULL entry; scratch NULL, too small or not 8-byte aligned (count > 0); an output that overlaps an
 * input (vertices, faces, a view's R or T), the scratch or another output;  LVDGS_E_RANGE: a view's width or height below 1 or more
 * than 2^31 - 1 pixels.
 * THE FLOAT32 RULE AGAINST EXACT ARITHMETIC, u = 2^-24, with the float32 u, v, z of the vertices as the operands (both read them
 * alike; the box follows from them without rounding):
 *   - an edge value: the two differences of each product round once each, the product once, the final difference once, so s is
 *     within  4u (|u_hi - u_lo| |j - v_lo| + |v_hi - v_lo| |i - u_lo|)  of its exact value (first order in u; (float)i and (float)j
 *     are exact for images below 2^24 pixels a side).  Coverage can differ from exact arithmetic only at a pixel where an edge
 *     value of a face lies within that bound of 0.
 *   - zp of a covered pixel: the E_k have one sign, so A, the w_k and inv are sums and quotients of like-signed terms without
 *     cancellation -- two sums, a quotient, the reciprocal of z_k, a product, two sums and the last reciprocal: 8u relative --, and an
 *     error e_k of E_k moves inv by at most e_k / |A| times the spread of the 1 / z_k.  zp is within
 *         (8u + ((e_0 + e_1 + e_2) / |A|) * (z_max / z_min - 1)) * zp
 *     of its exact value, e_k the edge bound above, z_max and z_min over the face's three vertices.
 * tests/test_mesh_depth.py takes both bounds doubled: pixels where an edge value lies within the first of 0, or two candidate depths
 * (or a candidate and dm or depth_trunc) within the second of each other, are set aside, at most 1 % of the covered ones, and the rest
 * must agree. */
typedef struct lvdgs_mesh_depth_args {
    int64_t num_vertices, num_faces;
    const float *vertices;        /* num_vertices*3                                 */
    const int32_t *faces;         /* num_faces*3                                    */
    const lvdgs_tsdf_view *const *views;   /* count views; depth, image and mask ignored */
    int32_t count;
    float *const *depth;          /* host: count device addresses, out height*width each */
    int32_t *const *face_index;   /* host: count device addresses, out height*width each, or NULL */
    void *scratch; size_t scratch_bytes;
} lvdgs_mesh_depth_args;
size_t lvdgs_mesh_depth_scratch_bytes(int64_t total_pixels);
int lvdgs_mesh_depth(const lvdgs_mesh_depth_args *a, void *stream);

/* ---- diagnostics ---- */
const char *lvdgs_last_error(void);
const char *lvdgs_version(void);
/* Optional per-kernel timing with HIP events recorded on the caller's stream around each
 * launch.  Off by default; enabling it does not change results. */
void lvdgs_profile_enable(int on);
void lvdgs_profile_reset(void);
/* Synchronises outstanding events, then fills up to `cap` entries; returns the entry count. */
typedef struct lvdgs_kernel_time {
    char name[48];
    int64_t launches;
    double total_ms;
} lvdgs_kernel_time;
int lvdgs_profile_read(lvdgs_kernel_time *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* LVDGS_H */
