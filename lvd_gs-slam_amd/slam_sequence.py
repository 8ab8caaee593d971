"""The front end's and the back end's loops run as ONE sequence, in one process: ``SlamSequence``.

The reference runs ``FrontEnd.run`` (utils/slam_frontend.py:1740-1899) and ``BackEnd.run`` (utils/slam_backend.py:485-609) as two
OS processes that exchange messages over queues ("init", "keyframe", "sync_backend", "color_refinement").  The queues, the GUI and
the MASt3R / GroundingDINO models are out of scope; what IS the path is the order in which the loops
of this package are called on one another's results as a sequence advances, with the map growing and shrinking under them:

    frame 0      FrontEnd.initialize (:1702-1738)      pose := ground truth, ``add_new_keyframe(init=True)`` -> depth map
                 BackEnd "init" (:514-528)             reset, ``extend_from_pcd_seq(init=True)``, ``initialize_map``
    frame i      FrontEnd.tracking (:1416-1536)        pose := previous frame's (the "no estimate" branch, :1460-1462), ``track_frame``
                 keyframe test (:1822-1846)            ``is_keyframe`` / the covisibility rule while the window fills
      keyframe:  ``add_to_window`` (:1621-1674), ``add_new_keyframe`` (:1268-1414) -> depth map
                 BackEnd "keyframe" (:530-601)         ``extend_from_pcd_seq``, a fresh keyframe Adam, ``map(iters)``, ``map(prune=True)``
      else:      ``cleanup`` (:1697-1700)
      idle:      BackEnd's free-running branch (:487-499): ``map(window)``; every 10 iterations ``map(prune=True, iters=10)`` + push
    end          ``eval_ate`` (:1773-1776), ``eval_rendering`` before / after ``color_refinement`` (utils/eval_utils_0806.py:172-437)

This class is that order, statement for statement, as method calls: the "messages" are direct calls; ``push_to_frontend`` /
``sync_backend`` hand the front end a detached COPY of the map (``clone_obj``, utils/multiprocessing_utils.py:21-31) together with the
visibility rows of the window -- the front end tracks against the map as of the last push, which is what keeps its per-Gaussian
visibility vectors the size of the map it renders while the back end densifies and prunes the live one.  It is the schedule of the reference's
``single_thread`` mode (the front end waits for every keyframe's mapping) plus a FIXED number of the back end's free-running
iterations per tracked frame (``idle_map_iters``; in the reference that number is whatever the wall clock allows).

Stand-ins for what is out of scope, all injectable:
  * the pose initialisation: by default the previous frame's pose -- the reference's own branch for "MASt3R returned the identity".
    ``pose_init="pnp"`` follows ``FrontEnd.tracking`` (:1442-1465): ``init_pose.get_pose`` (PnP-RANSAC on the last keyframe's rendered
    depth, HIP) gives the keyframe -> frame motion, ``pose_init = rel_pose @ pose_last_kf``, the previous pose when that is the identity;
    only the matcher's descriptor network needs MASt3R -- ``matcher`` is injectable: ``init_pose.DescriptorMatcher(describe)`` matches
    descriptor maps on the device (``synthetic.WorldDescriptors`` stands in for the network), ``synthetic.GroundTruthMatcher`` makes
    matches from the ground truth without matching anything;
  * ``keyframe_depth``: the depth map a new keyframe seeds Gaussians from.  Default: the keyframe's mono depth under the valid-pixel
    mask, i.e. ``add_new_keyframe``'s own statements for the first keyframe (:1364-1382) applied to every keyframe.  For later
    keyframes the reference blends rendered and mono depth patch by patch and rescales the mono depth (``process_depth``,
    utils/depth_utils.py, :1383-1405): ``keyframe_depth="patch_align"`` does that (``depth_utils.process_depth``, HIP); only the
    algorithm's scale remedy is injectable as ``scale_remedy``, by default the current scale is kept; ``scale_remedy="matches"`` is
    the reference's ``find_scale`` on ``matcher``'s matches (``depth_utils.MatchScaleRemedy``: only the descriptor network behind the
    matcher needs MASt3R);
  * ``dataset.static_mask(idx)`` for the GroundingDINO + SAM masks (``dynamic_masker.get_static_mask_for_gaussian_init``).
    ``dynamic_masks="detections"`` runs that call instead: ``masker`` (a ``dynamic_mask.DynamicMasker``; only the two networks behind
    its seats are out of scope) assembles the masks from boxes, labels and SAM masks on every tracked frame and again on every
    keyframe, as the reference does (``lvdgs_dynamic_mask``, HIP, or the masker's PyTorch chain).

``render_fn`` / ``view_loss_fn`` / ``refine_loss_fn`` / ``knn_fn`` default to the HIP paths; the CPU tests pass the dense float64
renderer and the loss oracle so that the same harness runs at toy size without a GPU.
"""
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .gaussian_renderer import render
from .graphics_utils import getProjectionMatrix2
from .keyframe_utils import add_to_window, covisibility, is_keyframe
from .slam_loops import color_refinement, initialize_map, track_frame


def expand_dynamic_mask(dynamic_mask, kernel_size=5):
    """``FrontEnd._expand_dynamic_mask`` (utils/slam_frontend.py:1260-1266): dilation by a ``kernel_size`` square of ones
    (cv2.dilate there; a max-pool with the border left out of the maximum here -- the same set)."""
    m = dynamic_mask.to(torch.float32)[None, None]
    return F.max_pool2d(m, kernel_size, stride=1, padding=kernel_size // 2)[0, 0] > 0.5


def clone_map(gaussians):
    """``clone_obj(self.gaussians)`` of ``push_to_frontend`` (utils/slam_backend.py:478; utils/multiprocessing_utils.py:21-31): the same
    object with every tensor attribute a detached copy (no gradients flow into it, no optimiser comes with it)."""
    import copy
    snap = copy.copy(gaussians)
    for name, value in vars(gaussians).items():
        if torch.is_tensor(value):
            setattr(snap, name, value.detach().clone())
    snap.optimizer = None
    return snap


def make_backend(config, gaussians, pipeline_params, background, cameras_extent=6.0):
    """A BackEnd-shaped object: the attributes ``BackEnd.__init__`` / ``set_hyperparams`` set (utils/slam_backend.py:21-72)."""
    T = config["Training"]
    opt = config["opt_params"]
    return SimpleNamespace(
        config=config, gaussians=gaussians, pipeline_params=pipeline_params, background=background,
        opt_params=SimpleNamespace(**opt) if isinstance(opt, dict) else opt, cameras_extent=cameras_extent, live_mode=False,
        monocular=T["monocular"], iteration_count=0, last_sent=0, occ_aware_visibility={}, viewpoints={}, current_window=[],
        initialized=not T["monocular"], keyframe_optimizers=None, theta=0,
        init_itr_num=T["init_itr_num"], init_gaussian_update=T["init_gaussian_update"], init_gaussian_reset=T["init_gaussian_reset"],
        init_gaussian_th=T["init_gaussian_th"], init_gaussian_extent=cameras_extent * T["init_gaussian_extent"],
        mapping_itr_num=T["mapping_itr_num"], gaussian_update_every=T["gaussian_update_every"],
        gaussian_update_offset=T["gaussian_update_offset"], gaussian_th=T["gaussian_th"],
        gaussian_extent=cameras_extent * T["gaussian_extent"], gaussian_reset=T["gaussian_reset"], size_threshold=T["size_threshold"],
        window_size=T["window_size"], single_thread=config["Dataset"].get("single_thread", False))


def make_keyframe_optimizer(config, viewpoints, current_window, frames_to_optimize):
    """The Adam the back end builds when a keyframe arrives (utils/slam_backend.py:545-598): pose deltas of the newest
    ``frames_to_optimize`` window keyframes at half the tracking learning rates, exposure of every window keyframe; frame 0 fixed."""
    lr = config["Training"]["lr"]
    groups = []
    for cam_idx, kf in enumerate(current_window):
        if kf == 0:
            continue
        vp = viewpoints[kf]
        if cam_idx < frames_to_optimize:
            groups.append({"params": [vp.cam_rot_delta], "lr": lr["cam_rot_delta"] * 0.5, "name": "rot_{}".format(vp.uid)})
            groups.append({"params": [vp.cam_trans_delta], "lr": lr["cam_trans_delta"] * 0.5, "name": "trans_{}".format(vp.uid)})
        groups.append({"params": [vp.exposure_a], "lr": 0.01, "name": "exposure_a_{}".format(vp.uid)})
        groups.append({"params": [vp.exposure_b], "lr": 0.01, "name": "exposure_b_{}".format(vp.uid)})
    return torch.optim.Adam(groups) if groups else None


class SlamSequence:
    """See the module's docstring.  ``run()`` processes the whole dataset and returns the record ``summary()`` builds."""

    def __init__(self, config, dataset, gaussians, pipeline_params, background, *, fused="auto", render_fn=render, view_loss_fn=None,
                 refine_loss_fn=None, keyframe_depth=None, idle_map_iters=0, camera_cls=None, cameras_extent=6.0, on_event=None,
                 group=None, aux_group=None, bands_ok=None, depth_align_fn=None, scale_remedy=None, depth_align_params=None,
                 pose_init=None, matcher=None, pose_init_params=None, frame_stats="torch", edge_mask="torch", dynamic_masks="dataset",
                 masker=None, seeding="host", map_edit="host", prefetch=0):
        from .backend_map import map_window
        if camera_cls is None:
            from .camera_utils import Camera as camera_cls
        self.config, self.dataset, self.gaussians = config, dataset, gaussians
        self.pipeline_params, self.background = pipeline_params, background
        self.fused, self.render_fn, self.view_loss_fn, self.refine_loss_fn = fused, render_fn, view_loss_fn, refine_loss_fn
        # keyframe_depth: None / "mono" (the default), "patch_align" (Algorithm 1 for every keyframe after the first), or a callable.
        # depth_align_fn: process_depth's signature (default depth_utils.process_depth); depth_align_params: its keyword parameters
        # (patch_size, thresholds, ...: the reference's config["depth"]); scale_remedy: find_scale's arguments -> a scale, or None to keep it
        self.patch_align = keyframe_depth == "patch_align"
        if keyframe_depth is None or keyframe_depth == "mono":
            self.keyframe_depth = self.default_keyframe_depth
        elif self.patch_align:
            self.keyframe_depth = self.patch_align_keyframe_depth
        elif callable(keyframe_depth):
            self.keyframe_depth = keyframe_depth
        else:
            raise ValueError(f"keyframe_depth: None, 'mono', 'patch_align' or a callable, not {keyframe_depth!r}")
        # scale_remedy="matches": the reference's find_scale on `matcher`'s matches (depth_utils.MatchScaleRemedy)
        if isinstance(scale_remedy, str):
            if scale_remedy != "matches":
                raise ValueError(f"scale_remedy: None, 'matches' or a callable, not {scale_remedy!r}")
            if matcher is None:
                raise TypeError("SlamSequence(scale_remedy='matches') needs the `matcher` argument (depth_utils.find_scale's matcher)")
            from .depth_utils import MatchScaleRemedy
            scale_remedy = MatchScaleRemedy(matcher)
        self.depth_align_fn, self.scale_remedy = depth_align_fn, scale_remedy
        self.depth_align_params = dict(depth_align_params or {})
        self.depth_align_log = []      # per aligned keyframe: frame, scale_factor, num_accurate_pixels, error_pixel_share, remedy_fired
        # pose_init: None (the default: the previous frame's pose, nothing logged), "previous" (the same poses, with the per-frame log),
        # "pnp" (init_pose.get_pose with `matcher`), or a callable (last_kf, viewpoint, kf_idx, frame_idx) -> (4, 4) keyframe -> frame motion
        # (the identity: no estimate).  pose_init_params: get_pose's keyword parameters (hypotheses, reproj_error, seed, min_inliers).
        if pose_init == "pnp":
            if matcher is None:
                raise TypeError("SlamSequence(pose_init='pnp') needs the `matcher` argument (init_pose.get_pose's matcher)")
            self.pose_init_fn = self.pnp_pose_init
        elif pose_init is None or pose_init == "previous":
            self.pose_init_fn = None
        elif callable(pose_init):
            self.pose_init_fn = pose_init
        else:
            raise ValueError(f"pose_init: None, 'previous', 'pnp' or a callable, not {pose_init!r}")
        self.pose_init, self.matcher, self.pose_init_params = pose_init, matcher, dict(pose_init_params or {})
        self.pose_init_log = []        # per tracked frame (pose_init not None): see `tracking`
        # frame_stats: "torch" (the default: get_median_depth and covisibility, a host wait per count) or "fused" (frame_stats.frame_summary:
        # the median depth and every count the keyframe test, add_to_window and the frame log read, in one call and one wait per tracked
        # frame -- the same bits and counts).  edge_mask: "torch" (Camera.compute_grad_mask's PyTorch statements) or "fused"
        # (frame_stats.edge_mask).  Both fused paths need the frames on a GPU; frames elsewhere keep the PyTorch path.
        for name, value in (("frame_stats", frame_stats), ("edge_mask", edge_mask)):
            if value not in ("torch", "fused"):
                raise ValueError(f"{name}: 'torch' or 'fused', not {value!r}")
        self.frame_stats, self.edge_mask = frame_stats, edge_mask
        # seeding: "host" (the default: GaussianModel's PyTorch statements and its host draw) or "fused" (seeding.seed_points: one call and
        # one wait per keyframe, another subsample).  Set on the map; the front end's copies (clone_map) never seed.
        if seeding not in ("host", "fused"):
            raise ValueError(f"seeding: 'host' or 'fused', not {seeding!r}")
        self.seeding = seeding
        # map_edit: "host" (the default: GaussianModel's PyTorch statements) or "fused" (map_edit: prune_points, densify_and_prune and the
        # pruning pass as one plan, one wait and one launch each).  Set on the map.
        if map_edit not in ("host", "fused"):
            raise ValueError(f"map_edit: 'host' or 'fused', not {map_edit!r}")
        self.map_edit = map_edit
        # prefetch: 0 (the default: every frame read by `dataset[idx]` at its turn) or the number of frames dataset.FramePrefetcher reads
        # ahead of `run` on its worker threads -- the same frames, so the same poses and the same map
        if int(prefetch) < 0:
            raise ValueError(f"prefetch: a number of frames >= 0, not {prefetch!r}")
        self.prefetch, self._frames = int(prefetch), None
        # dynamic_masks: "dataset" (the default: dataset.static_mask's finished masks) or "detections" (`masker`, a
        # dynamic_mask.DynamicMasker: the masks, add_new_keyframe's dilation and valid_rgb come from its calls)
        if dynamic_masks not in ("dataset", "detections"):
            raise ValueError(f"dynamic_masks: 'dataset' or 'detections', not {dynamic_masks!r}")
        if dynamic_masks == "detections" and masker is None:
            raise TypeError("SlamSequence(dynamic_masks='detections') needs the `masker` argument (a dynamic_mask.DynamicMasker)")
        self.dynamic_masks, self.masker = dynamic_masks, masker if dynamic_masks == "detections" else None
        self._summary = None           # the tracked frame's FrameSummary (frame_stats="fused"), else None
        self.idle_map_iters, self.camera_cls, self.on_event = int(idle_map_iters), camera_cls, on_event
        self._map_window = map_window
        # several ranks (torch.distributed initialised): every rank runs the whole sequence -- tracking, map initialisation and colour
        # refinement are one view per iteration: replicas -- and the mapping windows' views are sharded over
        # `group` (backend_map.map_window); the replicas stay bit-identical, so every rank ends with the same map and trajectory
        self.group, self.aux_group, self.bands_ok = group, aux_group, bands_ok
        T = config["Training"]
        self.monocular = T["monocular"]
        self.tracking_itr_num, self.kf_interval, self.window_size = T["tracking_itr_num"], T["kf_interval"], T["window_size"]
        self.single_thread = T.get("single_thread", False)
        df = config.get("dynamic_filtering", {})
        self.enable_dynamic_filtering = df.get("enabled", True) and (self.masker is not None or hasattr(dataset, "static_mask"))
        self.filter_initialization = df.get("filter_initialization", True)
        # front-end state (FrontEnd.__init__, utils/slam_frontend.py:1184-1213)
        self.initialized = False
        self.kf_indices, self.current_window, self.occ_aware_visibility, self.cameras = [], [], {}, {}
        self.median_depth, self.theta = None, 0
        self.frontend_gaussians = gaussians      # the front end's copy of the map as of the last push (``_sync_backend``)
        gaussians.seeding = self.seeding
        gaussians.map_edit = self.map_edit
        self.backend = make_backend(config, gaussians, pipeline_params, background, cameras_extent)
        self.projection_matrix = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=dataset.fx, fy=dataset.fy, cx=dataset.cx, cy=dataset.cy,
                                                      W=dataset.width, H=dataset.height).transpose(0, 1).to(device=dataset.device)
        self.counts = dict(frames=0, keyframes=0, tracking_iterations=0, mapping_iterations=0, init_iterations=0, prune_passes=0,
                           refinement_iterations=0)
        self.gaussian_counts = []      # (event, N) whenever the map's size may have changed
        self.seconds = dict(tracking=0.0, mapping=0.0, init=0.0, seeding=0.0, refinement=0.0, other=0.0)
        if self.patch_align:
            self.seconds["depth_align"] = 0.0
        if self.pose_init_fn is not None:
            self.seconds["pose_init"] = 0.0
        self.window_log = []           # the window after every keyframe
        self.frame_log = []            # per tracked frame: tracking iterations, the keyframe test's inputs and its outcome
        self.batched_sizes = []        # the map's size at every mapping call that went through the batched window (MapWindowBatch)

    # ------------------------------------------------------------------ helpers
    def _n(self):
        return int(self.gaussians.get_xyz.shape[0])

    def _note(self, event):
        self.gaussian_counts.append((event, self._n()))
        if self.on_event is not None:
            self.on_event(event, self)

    def _sync(self):
        dev = self.gaussians.get_xyz.device
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    def _timed(self, key):
        seq = self

        class _T:
            def __enter__(self):
                seq._sync()
                self.t = time.perf_counter()

            def __exit__(self, *exc):
                seq._sync()
                seq.seconds[key] += time.perf_counter() - self.t
                return False
        return _T()

    def _map(self, window, **kw):
        be = self.backend
        it0, n0 = be.iteration_count, self._n()
        if self.view_loss_fn is not None:
            kw["view_loss_fn"] = self.view_loss_fn
        if self.group is not None or self.aux_group is not None or self.bands_ok is not None:
            kw.update(group=self.group, aux_group=self.aux_group, bands_ok=self.bands_ok)
        runs0 = getattr(getattr(be, "_lvdgs_window_batch", None), "runs", 0)
        out = self._map_window(be, window, render_fn=self.render_fn, fused=self.fused is not False, **kw)
        if getattr(getattr(be, "_lvdgs_window_batch", None), "runs", 0) > runs0:
            self.batched_sizes.append(n0)
        if kw.get("prune"):
            self.counts["prune_passes"] += 1
        else:
            self.counts["mapping_iterations"] += be.iteration_count - it0
        if self._n() != n0:
            self._note("prune" if kw.get("prune") else "densify")
        return out

    # ------------------------------------------------------------------ front end
    def new_viewpoint(self, idx):
        """``Camera.init_from_dataset`` + ``compute_grad_mask`` (utils/slam_frontend.py:1794-1798)."""
        vp = self.camera_cls.init_from_dataset(self.dataset if self._frames is None else self._frames, idx, self.projection_matrix)
        if self.edge_mask == "fused" and torch.is_tensor(vp.original_image) and vp.original_image.is_cuda:
            vp.compute_grad_mask(self.config, fused=True)
        else:
            vp.compute_grad_mask(self.config)
        return vp

    def _attach_masks(self, viewpoint, idx, first):
        """What ``add_new_keyframe`` / ``tracking`` store on the viewpoint from the detector's mask (:1306-1329, :1419-1436)."""
        if self.masker is not None:
            static = self.masker.get_static_mask_for_gaussian_init(viewpoint.original_image, idx)
            viewpoint.static_mask, viewpoint.dynamic_mask = static, self.masker.last.dynamic_mask
            return static
        static = self.dataset.static_mask(idx)
        if static is None:
            return None
        dev = viewpoint.original_image.device
        static = static.to(dev).bool()
        viewpoint.static_mask, viewpoint.dynamic_mask = static, ~static
        return static

    def default_keyframe_depth(self, viewpoint, render_pkg, valid_rgb, init):
        """``add_new_keyframe``'s monocular statements for the first keyframe (:1364-1382): the mono depth, zero where invalid."""
        d = torch.from_numpy(np.asarray(viewpoint.mono_depth)).clone().unsqueeze(0)
        d[~valid_rgb.cpu()] = 0
        return d[0].numpy()

    def patch_align_keyframe_depth(self, viewpoint, render_pkg, valid_rgb, init):
        """``add_new_keyframe``'s statements for every keyframe after the first (:1383-1405): ``process_depth`` on the tracking render's
        depth and the keyframe's mono depth (the previous keyframe's mono depth and image go to the scale remedy), the mono depth
        rescaled by the scale found, the result zero where invalid.  The first keyframe keeps the mono path (``init``)."""
        if init or render_pkg is None or len(self.kf_indices) < 2:
            return self.default_keyframe_depth(viewpoint, render_pkg, valid_rgb, init)
        from . import depth_utils
        fn = self.depth_align_fn or depth_utils.process_depth
        prev = self.cameras[self.kf_indices[-2]]
        fired = []

        def remedy(im1, im2, last_depth, mono_depth, model):
            fired.append(True)
            if self.scale_remedy is None:
                return None
            if hasattr(self.scale_remedy, "set_frames"):      # a matcher that works from the dataset, not from the images
                self.scale_remedy.set_frames(self.kf_indices[-2], self.kf_indices[-1])
            return self.scale_remedy(im1, im2, last_depth, mono_depth, model)

        with self._timed("depth_align"):
            final, scale, error_mask, num_accurate = fn(render_pkg["depth"].detach(), viewpoint.mono_depth, last_depth=prev.mono_depth,
                                                        im1=prev.original_image, im2=viewpoint.original_image, model=None,
                                                        scale_remedy=remedy, **self.depth_align_params)
            viewpoint.mono_depth = (np.asarray(viewpoint.mono_depth, dtype=np.float32) * np.float32(scale)).astype(np.float32)
            if torch.is_tensor(final):
                final = final.clone()
                final[~valid_rgb[0].to(final.device)] = 0
                share = float(error_mask.float().mean())
            else:
                final = np.array(final, dtype=np.float32)
                final[~valid_rgb[0].cpu().numpy()] = 0
                share = float(np.mean(error_mask))
        self.depth_align_log.append(dict(frame=int(self.kf_indices[-1]), scale_factor=float(scale), num_accurate_pixels=int(num_accurate),
                                         error_pixel_share=share, remedy_fired=bool(fired)))
        return final

    def add_new_keyframe(self, cur_frame_idx, render_pkg=None, init=False):
        """utils/slam_frontend.py:1268-1414 without the detector and MASt3R: rotation to the last keyframe, the valid-pixel mask
        (non-black pixels minus the dilated dynamic mask: 9 x 9 on frame 0, 7 x 7 after), the depth map the seeds come from."""
        thr = self.config["Training"]["rgb_boundary_threshold"]
        viewpoint = self.cameras[cur_frame_idx]
        if len(self.kf_indices) > 0:
            R_last = self.cameras[self.kf_indices[-1]].R.to(torch.float32)
            R_diff = R_last.T @ viewpoint.R.to(torch.float32)
            self.theta = torch.rad2deg(torch.acos(((torch.trace(R_diff) - 1) / 2).clamp(-1.0, 1.0)))
        self.kf_indices.append(cur_frame_idx)
        gt_img = viewpoint.original_image
        valid_rgb = (gt_img.sum(dim=0) > thr)[None]
        if self.masker is not None and self.enable_dynamic_filtering and (not init or self.filter_initialization):
            valid_rgb = self.masker.keyframe_masks(viewpoint, cur_frame_idx, thr).valid_rgb[None]
        elif self.enable_dynamic_filtering and (not init or self.filter_initialization):
            static = self._attach_masks(viewpoint, cur_frame_idx, cur_frame_idx == 0)
            if static is not None:
                expanded_dynamic = expand_dynamic_mask(viewpoint.dynamic_mask, 9 if cur_frame_idx == 0 else 7)
                viewpoint.expanded_dynamic_mask, viewpoint.expanded_static_mask = expanded_dynamic, ~expanded_dynamic
                valid_rgb = valid_rgb & viewpoint.expanded_static_mask[None]
        if not self.monocular and getattr(viewpoint, "depth", None) is not None:   # (:1409-1414)
            d = torch.from_numpy(np.asarray(viewpoint.depth)).clone().unsqueeze(0)
            d[~valid_rgb.cpu()] = 0
            return d[0].numpy()
        return self.keyframe_depth(viewpoint, render_pkg, valid_rgb, init)

    def initialize(self, cur_frame_idx, viewpoint):
        """FrontEnd.initialize (:1702-1738) + the back end's "init" message (utils/slam_backend.py:514-528)."""
        self.initialized = not self.monocular
        self.kf_indices, self.occ_aware_visibility, self.current_window = [], {}, []
        # (a dataset read from disk hands its poses over in float64, as the reference's does; upstream's getWorld2View2 narrows them where
        # it fills its float32 matrix, here the estimate's own dtype does: a no-op for float32 poses)
        viewpoint.update_RT(viewpoint.R_gt.to(viewpoint.R.dtype), viewpoint.T_gt.to(viewpoint.T.dtype))
        depth_map = self.add_new_keyframe(cur_frame_idx, init=True)
        be = self.backend
        # BackEnd.reset (:80-92)
        be.iteration_count, be.occ_aware_visibility, be.viewpoints, be.current_window = 0, {}, {}, []
        be.initialized, be.keyframe_optimizers = not be.monocular, None
        if self._n():
            self.gaussians.prune_points(self.gaussians.unique_kfIDs >= 0)
        be.viewpoints[cur_frame_idx] = viewpoint
        with self._timed("seeding"):
            self.gaussians.extend_from_pcd_seq(viewpoint, kf_id=cur_frame_idx, init=True, scale=2.0, depthmap=depth_map)
        self._note("seed")
        with self._timed("init"):
            initialize_map(be, cur_frame_idx, viewpoint, render_fn=self.render_fn, fused=self.fused)
        self.counts["init_iterations"] += be.init_itr_num
        self._note("initialize_map")
        self._sync_backend()
        self.current_window.append(cur_frame_idx)
        self.counts["keyframes"] += 1
        self.window_log.append(list(self.current_window))

    def _sync_backend(self):
        """``push_to_frontend`` + ``sync_backend`` (utils/slam_backend.py:470-480, utils/slam_frontend.py:1688-1695): a detached copy
        of the map and the window's visibility rows (the keyframes are shared objects here: their poses need no copying back)."""
        self.backend.last_sent = 0
        self.frontend_gaussians = clone_map(self.gaussians)
        self.occ_aware_visibility = dict(self.backend.occ_aware_visibility)

    def pnp_pose_init(self, last_kf, viewpoint, kf_idx, cur_frame_idx):
        """``get_pose`` as ``FrontEnd.tracking`` calls it (:1445-1453): the last keyframe rendered from the front end's copy of the map."""
        from . import init_pose
        if hasattr(self.matcher, "set_frames"):      # a stand-in that works from the dataset, not from the images
            self.matcher.set_frames(kf_idx, cur_frame_idx)
        rel_pose, _ = init_pose.get_pose(last_kf.original_image, viewpoint.original_image, None, getattr(self.dataset, "dist_coeffs", None),
                                         last_kf, self.frontend_gaussians, self.pipeline_params, self.background, matcher=self.matcher,
                                         **self.pose_init_params)
        return rel_pose

    @staticmethod
    def _pose_error(R, T, viewpoint):
        """(distance of the camera centres, rotation angle in degrees) of the pose (R, T) against the viewpoint's ground truth."""
        R, T = R.detach().double().cpu(), T.detach().double().cpu()
        Rg, Tg = viewpoint.R_gt.detach().double().cpu(), viewpoint.T_gt.detach().double().cpu()
        cos = ((torch.trace(R @ Rg.T) - 1.0) / 2.0).clamp(-1.0, 1.0)
        return float((R.T @ T - Rg.T @ Tg).norm()), float(torch.rad2deg(torch.acos(cos)))

    def tracking(self, cur_frame_idx, viewpoint):
        """FrontEnd.tracking (:1416-1536).  The initial estimate: the previous frame's pose, or (``pose_init``) :1442-1465."""
        if self.enable_dynamic_filtering:
            self._attach_masks(viewpoint, cur_frame_idx, False)
        prev = self.cameras[cur_frame_idx - 1]
        record = None
        if self.pose_init_fn is None:
            viewpoint.update_RT(prev.R, prev.T)
        else:
            kf_idx = self.current_window[0]
            last_kf = self.cameras[kf_idx]
            with self._timed("pose_init"):
                rel_pose = np.asarray(self.pose_init_fn(last_kf, viewpoint, kf_idx, cur_frame_idx), dtype=np.float64)
            estimated = not np.allclose(rel_pose, np.eye(4), atol=1e-6)
            if estimated:
                pose_last_kf = torch.eye(4, dtype=torch.float64)
                pose_last_kf[:3, :3], pose_last_kf[:3, 3] = last_kf.R.detach().double().cpu(), last_kf.T.detach().double().cpu()
                init = torch.from_numpy(rel_pose) @ pose_last_kf
                viewpoint.update_RT(init[:3, :3].to(prev.R.dtype), init[:3, 3].to(prev.T.dtype))
            else:
                viewpoint.update_RT(prev.R, prev.T)
            record = dict(frame=cur_frame_idx, keyframe=int(kf_idx), estimated=bool(estimated))
            if self.pose_init == "pnp":
                from . import init_pose
                lc = init_pose.last_call
                record.update(matches=lc.matches, valid_matches=lc.valid_matches, inliers=lc.inliers)
        if self.pose_init is not None:
            record = record or dict(frame=cur_frame_idx, keyframe=int(self.current_window[0]), estimated=False)
            record["init_translation_error"], record["init_rotation_error_deg"] = self._pose_error(viewpoint.R, viewpoint.T, viewpoint)
            record["previous_translation_error"], record["previous_rotation_error_deg"] = self._pose_error(prev.R, prev.T, viewpoint)
        fused_stats = self.frame_stats == "fused" and self.frontend_gaussians.get_xyz.is_cuda
        self._summary = None
        with self._timed("tracking"):
            render_pkg, median_depth, its = track_frame(viewpoint, self.frontend_gaussians, self.config, self.pipeline_params, self.background,
                                                        tracking_itr_num=self.tracking_itr_num, render_fn=self.render_fn, fused=self.fused,
                                                        **({"median_depth": False} if fused_stats else {}))
            if fused_stats:
                from .frame_stats import frame_summary
                depth, opacity = render_pkg["depth"], render_pkg["opacity"]
                if _lib.is_f32(depth) and _lib.is_f32(opacity, depth.device) and render_pkg["n_touched"].dtype is torch.int32:
                    self._summary = frame_summary(dict(depth=depth.detach(), opacity=opacity.detach(), n_touched=render_pkg["n_touched"]),
                                                  {k: self.occ_aware_visibility[k] for k in self.current_window},
                                                  count_mask=getattr(viewpoint, "expanded_static_mask", None))
                    median_depth = self._summary.median_depth
                else:   # (a renderer that leaves something else than the HIP path's buffers)
                    from .slam_utils import get_median_depth
                    median_depth = get_median_depth(depth, opacity)
        self.median_depth = median_depth
        self.counts["tracking_iterations"] += int(its)
        self._last_tracking_iterations = int(its)
        if record is not None:
            record["tracking_iterations"] = int(its)
            self.pose_init_log.append(record)
        return render_pkg

    def handle_keyframe(self, cur_frame_idx, viewpoint, depth_map):
        """The back end's "keyframe" message (utils/slam_backend.py:530-601)."""
        be, cfg = self.backend, self.config
        be.viewpoints[cur_frame_idx] = viewpoint
        be.current_window = self.current_window
        be.theta = self.theta
        with self._timed("seeding"):
            self.gaussians.extend_from_pcd_seq(viewpoint, kf_id=cur_frame_idx, init=False, scale=2.0, depthmap=depth_map)
        self._note("seed")
        frames_to_optimize = cfg["Training"]["pose_window"]
        iter_per_kf = be.mapping_itr_num if be.single_thread else cfg["Training"]["mapping_itr_nosingle"]
        if not be.initialized:
            if len(self.current_window) == cfg["Training"]["window_size"]:
                frames_to_optimize = cfg["Training"]["window_size"] - 1
                iter_per_kf = 50 if be.live_mode else cfg["Training"].get("initial_ba_itr_num", 300)
            else:
                iter_per_kf = be.mapping_itr_num
        be.keyframe_optimizers = make_keyframe_optimizer(cfg, be.viewpoints, self.current_window, frames_to_optimize)
        with self._timed("mapping"):
            self._map(self.current_window, iters=iter_per_kf, up_pose=True)
            self._map(self.current_window, prune=True)
        self._sync_backend()

    def idle_mapping(self, iterations):
        """The back end between messages (utils/slam_backend.py:487-499)."""
        be = self.backend
        if len(self.current_window) == 0 or be.single_thread:
            return
        with self._timed("mapping"):
            for _ in range(iterations):
                self._map(self.current_window)
                if be.last_sent >= 10:
                    self._map(self.current_window, prune=True, iters=10)
                    self._sync_backend()

    def step(self, cur_frame_idx):
        """One pass of FrontEnd.run's body for frame ``cur_frame_idx`` (:1794-1893).  Returns True for a keyframe."""
        viewpoint = self.new_viewpoint(cur_frame_idx)
        self.cameras[cur_frame_idx] = viewpoint
        self.counts["frames"] += 1
        if cur_frame_idx == 0 or not self.current_window:
            self.initialize(cur_frame_idx, viewpoint)
            return True
        self.initialized = self.initialized or (len(self.current_window) == self.window_size)
        render_pkg = self.tracking(cur_frame_idx, viewpoint)
        last_keyframe_idx = self.current_window[0]
        check_time = (cur_frame_idx - last_keyframe_idx) >= self.kf_interval
        curr_visibility = (render_pkg["n_touched"] > 0).long()
        fs = self._summary
        covis = None if fs is None else fs.covis
        create_kf = is_keyframe(self.config, self.cameras, cur_frame_idx, last_keyframe_idx, curr_visibility, self.occ_aware_visibility,
                                self.median_depth, covis=covis, mask_share=None if fs is None else fs.mask_share)
        inter, union, _, _ = covis[last_keyframe_idx] if fs is not None else covisibility(curr_visibility, self.occ_aware_visibility[last_keyframe_idx])
        point_ratio = inter / union if union else float("nan")
        if len(self.current_window) < self.window_size:
            create_kf = check_time and point_ratio < self.config["Training"]["kf_overlap"]
        if self.single_thread:
            create_kf = check_time and create_kf
        self.frame_log.append(dict(frame=cur_frame_idx, tracking_iterations=self._last_tracking_iterations, median_depth=float(self.median_depth),
                                   covisibility=point_ratio, visible=fs.visible if fs is not None else int(curr_visibility.count_nonzero()), keyframe=bool(create_kf),
                                   gaussians_tracked_against=int(self.frontend_gaussians.get_xyz.shape[0])))
        if create_kf:
            self.current_window, removed = add_to_window(self.config, self.cameras, cur_frame_idx, curr_visibility,
                                                         self.occ_aware_visibility, self.current_window, initialized=self.initialized, covis=covis)
            depth_map = self.add_new_keyframe(cur_frame_idx, render_pkg=render_pkg, init=False)
            self.handle_keyframe(cur_frame_idx, viewpoint, depth_map)
            self.counts["keyframes"] += 1
            self.window_log.append(list(self.current_window))
        else:
            viewpoint.clean()                      # FrontEnd.cleanup (:1697-1700): the pose stays, the images go
        self.idle_mapping(self.idle_map_iters)
        return create_kf

    def run(self, n_frames=None):
        t0 = time.perf_counter()
        n = len(self.dataset) if n_frames is None else min(n_frames, len(self.dataset))
        if self.prefetch > 0:
            from .dataset import FramePrefetcher
            self._frames = FramePrefetcher(self.dataset, range(n), depth=self.prefetch)
        try:
            with _lib.quiet_gc():
                for idx in range(n):
                    self.step(idx)
        finally:
            if self._frames is not None:      # at the end of the run and on an exception: no worker thread outlives it
                self._frames.close()
                self._frames = None
        self._sync()
        self.seconds["wall"] = time.perf_counter() - t0
        return self

    # ------------------------------------------------------------------ after the sequence
    def refine(self, iterations):
        """The "color_refinement" message (utils/slam_backend.py:510-512)."""
        kw = {} if self.refine_loss_fn is None else {"loss_fn": self.refine_loss_fn}
        with self._timed("refinement"):
            color_refinement(self.backend, iteration_total=iterations, render_fn=self.render_fn, fused=self.fused, **kw)
        self.counts["refinement_iterations"] += iterations
        self._sync_backend()

    def eval_ate(self):
        """``eval_ate`` over the keyframes (utils/eval_utils_0806.py:101-169); None with fewer than three."""
        from .eval_utils import eval_ate
        return eval_ate(self.cameras, self.kf_indices, monocular=self.monocular)

    def pose_errors(self):
        """Distance between estimated and ground-truth camera centres, frame by frame, WITHOUT any alignment (frame 0 starts at its
        ground-truth pose): what ``eval_ate``'s similarity alignment -- with scale for monocular runs -- can hide, e.g. a tracker that
        follows only a fraction of the motion.  -> {frame: error}."""
        out = {}
        for i, cam in self.cameras.items():
            c = lambda R, T: -(R.detach().double().cpu().T @ T.detach().double().cpu())
            out[i] = float((c(cam.R, cam.T) - c(cam.R_gt, cam.T_gt)).norm())
        return out

    def eval_rendering(self, metrics_fn=None, *, fused=False):
        """``eval_rendering``'s numbers (utils/eval_utils_0806.py:172-306): every NON-keyframe frame rendered from its tracked pose
        against the dataset's image; means of PSNR (and of whatever else ``metrics_fn`` returns: default ``eval_utils.frame_metrics``,
        which needs the GPU for SSIM).  ``fused``: one ``eval_utils.FrameEvaluator`` over the loop -- one library call per frame, no
        wait -- and one read of its table at the end (``metrics_fn`` is then not used)."""
        if metrics_fn is None:
            from .eval_utils import frame_metrics as metrics_fn
        rows, evaluator = [], None
        for idx in range(0, len(self.cameras) - 1):      # (`end_idx = len(frames) - 1`, :184)
            if idx in self.kf_indices:
                continue
            frame = self.cameras[idx]
            gt_image = self.dataset[idx][0]
            with torch.no_grad():
                pkg = self.render_fn(frame, self.frontend_gaussians, self.pipeline_params, self.background)
            static = getattr(frame, "expanded_static_mask", None)
            if static is None:
                static = getattr(frame, "static_mask", None)
            if fused:
                if evaluator is None:
                    from .eval_utils import FrameEvaluator
                    evaluator = FrameEvaluator(pkg["render"].shape[-2], pkg["render"].shape[-1], pkg["render"].device, len(self.cameras))
                evaluator.add(pkg["render"], gt_image.to(pkg["render"].device), static, self.background)
                continue
            rows.append(metrics_fn(pkg["render"], gt_image.to(pkg["render"].device), static, self.background))
        if evaluator is not None:
            rows = [{k: v for k, v in r.items() if k not in ("depth_min", "depth_max")} for r in evaluator.results()]
        if not rows:
            return {}
        return {k: float(np.mean([r[k] for r in rows if r.get(k) is not None])) for k in rows[0] if any(r.get(k) is not None for r in rows)}

    def fuse_mesh(self, voxel_size, bounds=None, frames="keyframes", mask="static", depth_trunc=None, max_voxels=1 << 26, volume="dense",
                  pool_blocks=None):
        """A surface of the finished map: the chosen frames rendered at their estimated poses with the run's ``render_fn``, their depth,
        colour and -- ``mask="static"``, where a frame has one -- static mask fused into a TSDF volume (``tsdf.TsdfVolume``, 16 views per
        library call, no wait), and the volume's surface-nets mesh (one wait).  What the reference's evaluation does with Open3D on the
        host after copying every rendered depth map and image.

        ``bounds``: (lo, hi) of the volume; default: the extent of the Gaussians with opacity at least 0.5 (all of them when none has),
        padded by the truncation distance ``4 * voxel_size``.  ``frames``: "keyframes", "all" or frame indices.  ``mask``: "static" or None.
        ``depth_trunc``: rendered depth beyond it is not fused (None: no limit).  ``max_voxels``: a volume that would hold more samples gets
        a larger voxel size (``TsdfVolume.from_bounds``; the record says so).  -> (``tsdf.Mesh`` on the device, a record: dims, the
        voxel size used and asked for, frames fused, vertex and face counts).

        ``volume="blocks"``: a ``tsdf_blocks.TsdfBlockVolume`` with its origin at the low corner of ``bounds`` instead -- only the blocks
        the rendered surfaces cross are stored, the voxel size asked for is always the one used and ``max_voxels`` is not consulted.
        ``pool_blocks``: the pool to start with (default 4096); when the fusion had to drop blocks the pool is doubled once and the
        frames are fused again.  The record then carries blocks, dropped and pool_blocks in place of dims (one more wait: the stats)."""
        from .tsdf import TsdfVolume
        from .tsdf_blocks import TsdfBlockVolume
        if volume not in ("dense", "blocks"):
            raise ValueError(f"fuse_mesh: volume 'dense' or 'blocks', not {volume!r}")
        gaussians = self.frontend_gaussians
        if frames == "keyframes":
            chosen = list(self.kf_indices)
        elif frames == "all":
            chosen = sorted(self.cameras)
        else:
            chosen = [int(i) for i in frames]
        if mask not in ("static", None):
            raise ValueError(f"fuse_mesh: mask 'static' or None, not {mask!r}")
        with torch.no_grad():
            xyz = gaussians.get_xyz.detach()
            if bounds is None:
                opaque = gaussians.get_opacity.detach().reshape(-1) >= 0.5
                points = xyz[opaque] if bool(opaque.any()) else xyz
                pad = 4.0 * float(voxel_size)
                bounds = ((points.min(0).values - pad).tolist(), (points.max(0).values + pad).tolist())
            if volume == "blocks":
                vol = TsdfBlockVolume(bounds[0], voxel_size, 4096 if pool_blocks is None else int(pool_blocks), device=xyz.device)
            else:
                vol = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel_size, max_voxels=max_voxels, device=xyz.device)

            def fuse():
                views = []
                for idx in chosen:
                    frame = self.cameras[idx]
                    pkg = self.render_fn(frame, gaussians, self.pipeline_params, self.background)
                    static = None
                    if mask == "static":
                        static = getattr(frame, "expanded_static_mask", None)
                        if static is None:
                            static = getattr(frame, "static_mask", None)
                        if static is not None:
                            static = static.to(xyz.device)
                    depth = pkg["depth"].detach()
                    views.append(dict(depth=depth.reshape(depth.shape[-2], depth.shape[-1]).contiguous(), R=frame.R, T=frame.T,
                                      intrinsics=(frame.fx, frame.fy, frame.cx, frame.cy), image=pkg["render"].detach().contiguous(), mask=static,
                                      depth_trunc=float("inf") if depth_trunc is None else float(depth_trunc)))
                    if len(views) == 16:
                        vol.integrate_views(views)
                        views = []
                if views:
                    vol.integrate_views(views)

            fuse()
            if volume == "blocks" and vol.stats()["dropped"]:
                vol.grow(2 * vol.pool_blocks)
                vol.reset()
                fuse()
        if volume == "blocks":      # the cells of the dense volume over ``bounds`` at this voxel size: nothing outside the box is meshed
            cells = [max(int(math.ceil((b - a) / float(voxel_size))) + 1, 2) - 1 for a, b in zip(bounds[0], bounds[1])]
            mesh = vol.extract_mesh(cell_range=((0, 0, 0), cells))
        else:
            mesh = vol.extract_mesh()
        record = dict(voxel_size=vol.voxel_size, voxel_size_requested=vol.voxel_size_requested,
                      frames=len(chosen), vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]))
        if volume == "blocks":
            record.update(volume="blocks", blocks=vol.last_stats["blocks"], dropped=vol.last_stats["dropped"], pool_blocks=vol.pool_blocks)
        else:
            record.update(dims=list(vol.dims))
        return mesh, record

    def _chosen_frames(self, frames):
        if frames == "keyframes":
            return list(self.kf_indices)
        return sorted(self.cameras) if frames == "all" else [int(i) for i in frames]

    def _dataset_depth_plane(self, idx, dev):
        """Frame ``idx``'s dataset depth (``Camera.depth32``, or ``Camera.depth`` / the dataset's plane uploaded once) as an (H, W) float32 tensor
        on ``dev``; None for a frame without one."""
        frame = self.cameras[idx]
        depth = getattr(frame, "depth32", None)
        if depth is None:
            depth = getattr(frame, "depth", None)
        if depth is None:      # a finished frame has given its planes back (Camera.clean): the dataset still has them
            record = self.dataset.frame(idx) if hasattr(self.dataset, "frame") else None
            depth = None if record is None else record.depth32
            if depth is None:
                depth = (self.dataset[idx] if record is None else record.frame)[1]
        if depth is None:
            return None
        depth = torch.as_tensor(np.asarray(depth) if not torch.is_tensor(depth) else depth, dtype=torch.float32, device=dev)
        return depth.detach().to(dev).reshape(int(frame.image_height), int(frame.image_width)).contiguous()

    def _frame_views(self, chosen, poses, depth_trunc, dev, depth="dataset"):
        """The chosen frames as the view dicts of ``TsdfVolume.integrate_views`` / ``mesh_eval.visibility``, at the ground-truth poses
        (``poses="gt"``) or the estimated ones.  ``depth="dataset"``: with the frame's dataset depth plane, a frame without one left out;
        ``depth=None``: every frame, frustum only (``size`` in the plane's place)."""
        views = []
        for idx in chosen:
            frame = self.cameras[idx]
            R, T = (frame.R_gt, frame.T_gt) if poses == "gt" else (frame.R, frame.T)
            view = dict(R=R.detach().to(dev), T=T.detach().to(dev), intrinsics=(frame.fx, frame.fy, frame.cx, frame.cy),
                        depth_trunc=float("inf") if depth_trunc is None else float(depth_trunc))
            if depth == "dataset":
                plane = self._dataset_depth_plane(idx, dev)
                if plane is None:
                    continue
                view["depth"] = plane
            else:
                view.update(depth=None, size=(int(frame.image_height), int(frame.image_width)))
            views.append(view)
        return views

    def _fuse_dataset_depth(self, volume, chosen, poses, depth_trunc):
        """The chosen frames' dataset depth fused into ``volume`` at the ground-truth poses (``poses="gt"``) or the estimated ones; a frame
        without depth is left out.  -> the frames fused."""
        views = self._frame_views(chosen, poses, depth_trunc, volume.device)
        for first in range(0, len(views), 16):
            volume.integrate_views(views[first:first + 16])
        return len(views)

    def eval_mesh(self, voxel_size, bounds=None, frames="keyframes", n_samples=200_000, threshold=None, seed=0, seed_gt=None, mask="static",
                  depth_trunc=None, max_voxels=1 << 26, est_depth="render", volume="dense", pool_blocks=None, gt_mesh=None, cull=None,
                  cull_eps=None, face_rule="all", depth_l1=False):
        """The finished map's surface scored against ground-truth geometry (``mesh_eval.score``: accuracy, completion, completion ratio,
        precision, recall, F-score, chamfer -- NICE-SLAM's ``eval_recon`` protocol), everything on the device.

        The estimate is ``fuse_mesh``'s mesh as it stands (``est_depth="dataset"``: the dataset's depth fused at the ESTIMATED poses
        instead of the rendered depth -- what the trajectory alone costs the surface).  The ground truth is a second volume of the same
        bounds and voxel size, fused from the same frames' dataset depth at ``R_gt``, ``T_gt``.  ``threshold``: default twice the voxel
        size actually used.  A dataset without metric depth (all-zero planes: the KITTI / dl3dv placeholders) gives an empty
        ground-truth mesh, which raises ``LvdgsError``.  Three waits: one per mesh, one for the score.
        ``volume="blocks"``, ``pool_blocks``: the estimate's rendered depth goes into a block-sparse volume (``fuse_mesh``); the ground
        truth and ``est_depth="dataset"`` stay dense.

        ``gt_mesh``: a ``tsdf.Mesh`` on the device or the path of a PLY (``mesh_eval.load_mesh_ply``) in the ground-truth poses' world
        frame -- a dataset's own scene mesh --, used as the ground truth in place of the second volume (one wait fewer); the dataset then
        needs metric depth only for ``cull="visible"``.
        ``cull``: None, or both meshes culled to what the chosen frames observed before they are scored (``mesh_eval.cull_mesh``, one more
        wait per mesh): "frustum" -- the estimate by the frames at their estimated ``R``, ``T``, the ground truth by the same frames at
        ``R_gt``, ``T_gt``, a vertex seen when it lies inside some frame's image and not beyond ``depth_trunc`` --; "visible" -- the ground
        truth is also tested against the frames' dataset depth planes (``_fuse_dataset_depth``'s), a vertex more than ``cull_eps`` behind
        its pixel's depth is not seen; the estimate stays frustum-culled, its surface being what those frames rendered.  ``cull_eps``:
        default the truncation distance ``4 * voxel_size`` actually used -- a fused surface lies within that band of the depth that
        produced it.  ``face_rule``: "all" or "any" of a face's vertices seen.
        "occlusion" -- each mesh is culled against the depth rendered from ITSELF (``mesh_eval.render_depth``) at the chosen frames, the
        estimate at the estimated ``R``, ``T``, the ground truth at ``R_gt``, ``T_gt``, both with ``cull_eps``: a second wall, or the inside of
        a fused shell, goes from either mesh.  No dataset depth is read, so with ``gt_mesh`` a dataset without metric depth can be scored
        this way.
        ``depth_l1``: both final meshes are rendered at the chosen frames (each at its own poses, as above) and the record gains
        ``depth_l1`` -- the mean over the frames of the frame's mean ``|d_est - d_gt|`` over the pixels where both depths are ``> 0`` and, with
        ``depth_trunc``, not beyond it (``mesh_eval.depth_l1_terms``; a frame without such a pixel is left out, NaN when there is none) --
        and ``depth_l1_pixels``, the pixels counted; ``last_eval_depths`` keeps the planes.  One more wait, taken at the end.
        -> (the score's dict, a record: both meshes' counts, the voxel size, the threshold, the samples and seeds; with ``cull`` per mesh
        also vertices_before, faces_before, cull and cull_eps)."""
        from . import mesh_eval
        from .tsdf import Mesh, TsdfVolume
        if est_depth not in ("render", "dataset"):
            raise ValueError(f"eval_mesh: est_depth 'render' or 'dataset', not {est_depth!r}")
        if cull not in (None, "frustum", "visible", "occlusion"):
            raise ValueError(f"eval_mesh: cull None, 'frustum', 'visible' or 'occlusion', not {cull!r}")
        if face_rule not in mesh_eval.FACE_RULES:
            raise ValueError(f"eval_mesh: face_rule 'all' or 'any', not {face_rule!r}")
        chosen = self._chosen_frames(frames)
        gaussians = self.frontend_gaussians
        with torch.no_grad():
            xyz = gaussians.get_xyz.detach()
            if bounds is None:      # fuse_mesh's default, taken here so that both volumes share it
                opaque = gaussians.get_opacity.detach().reshape(-1) >= 0.5
                points = xyz[opaque] if bool(opaque.any()) else xyz
                pad = 4.0 * float(voxel_size)
                bounds = ((points.min(0).values - pad).tolist(), (points.max(0).values + pad).tolist())
            if est_depth == "render":
                est, est_record = self.fuse_mesh(voxel_size, bounds=bounds, frames=chosen, mask=mask, depth_trunc=depth_trunc, max_voxels=max_voxels,
                                                 volume=volume, pool_blocks=pool_blocks)
            else:
                volume = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel_size, max_voxels=max_voxels, color=False, device=xyz.device)
                fused = self._fuse_dataset_depth(volume, chosen, "estimated", depth_trunc)
                est = volume.extract_mesh()
                est_record = dict(dims=list(volume.dims), voxel_size=volume.voxel_size, voxel_size_requested=volume.voxel_size_requested,
                                  frames=fused, vertices=int(est.vertices.shape[0]), faces=int(est.faces.shape[0]))
            if gt_mesh is None:
                truth = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel_size, max_voxels=max_voxels, color=False, device=xyz.device)
                fused = self._fuse_dataset_depth(truth, chosen, "gt", depth_trunc)
                gt = truth.extract_mesh()
                gt_record = dict(dims=list(truth.dims), voxel_size=truth.voxel_size, frames=fused, vertices=int(gt.vertices.shape[0]),
                                 faces=int(gt.faces.shape[0]))
                used = float(truth.voxel_size)
            else:
                gt = gt_mesh if isinstance(gt_mesh, Mesh) else mesh_eval.load_mesh_ply(os.fspath(gt_mesh), device=xyz.device)
                gt_record = dict(source="mesh" if isinstance(gt_mesh, Mesh) else os.fspath(gt_mesh), vertices=int(gt.vertices.shape[0]),
                                 faces=int(gt.faces.shape[0]))
                used = float(est_record["voxel_size"])
        if gt_record["faces"] == 0:
            if gt_mesh is not None:
                raise _lib.LvdgsError("eval_mesh: the ground-truth mesh has no faces")
            raise _lib.LvdgsError(f"eval_mesh: the ground-truth mesh is empty ({fused} of {len(chosen)} frames have a depth plane and none of it "
                                  "lies in the volume): a dataset without metric depth cannot score a mesh")
        if est_record["faces"] == 0:
            raise _lib.LvdgsError("eval_mesh: the estimated mesh is empty")
        if cull is not None:
            eps = 4.0 * used if cull_eps is None else float(cull_eps)
            dev = xyz.device
            gt_views = self._frame_views(chosen, "gt", depth_trunc, dev, depth="dataset" if cull == "visible" else None)
            if not gt_views:
                raise _lib.LvdgsError(f"eval_mesh: cull='visible' needs the frames' dataset depth and none of the {len(chosen)} frames has a plane")
            occlusion = "self" if cull == "occlusion" else None
            for name, mesh, record, views, how in (("estimated", est, est_record, self._frame_views(chosen, "estimated", depth_trunc, dev, depth=None),
                                                    "occlusion" if occlusion else "frustum"),
                                                   ("ground-truth", gt, gt_record, gt_views, cull)):
                kept, counts = mesh_eval.cull_mesh(mesh, views=views, occlusion_eps=eps, face_rule=face_rule, occlusion=occlusion)
                record.update(counts, cull=how, cull_eps=eps)
                if counts["faces"] == 0:
                    raise _lib.LvdgsError(f"eval_mesh: the {name} mesh has no face that the {len(views)} frames saw (cull={how!r})")
                if name == "estimated":
                    est = kept
                else:
                    gt = kept
        threshold = 2.0 * used if threshold is None else float(threshold)
        result = mesh_eval.score(est, gt, n_samples=n_samples, threshold=threshold, seed=seed, seed_gt=seed_gt)
        self.last_eval_meshes = (est, gt)
        record = dict(est=est_record, gt=gt_record, est_depth=est_depth, voxel_size=used, threshold=threshold, n_samples=int(n_samples),
                      seed=int(seed), seed_gt=int(seed) + 1 if seed_gt is None else int(seed_gt))
        if depth_l1:
            dev = xyz.device
            planes = [mesh_eval.render_depth(mesh, self._frame_views(chosen, poses, depth_trunc, dev, depth=None))
                      for mesh, poses in ((est, "estimated"), (gt, "gt"))]
            terms = [torch.stack([total, pixels.to(torch.float64)])      # per frame: (sum, pixels)
                     for total, pixels in (mesh_eval.depth_l1_terms(a, b, depth_trunc) for a, b in zip(*planes))]
            table = torch.stack(terms) if terms else torch.zeros((0, 2), dtype=torch.float64, device=dev)
            host = torch.empty(table.shape, dtype=torch.float64).pin_memory()
            host.copy_(table, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()      # the one wait of the depth L1
            sums, pixels = host.numpy()[:, 0], host.numpy()[:, 1]
            counted = pixels > 0
            record.update(depth_l1=float((sums[counted] / pixels[counted]).mean()) if counted.any() else math.nan,
                          depth_l1_pixels=int(pixels.sum()))
            self.last_eval_depths = tuple(planes)
        return result, record

    def summary(self):
        c, s = dict(self.counts), dict(self.seconds)
        ns = [n for _, n in self.gaussian_counts]
        loops = s.get("tracking", 0.0) + s.get("mapping", 0.0)
        its = c["tracking_iterations"] + c["mapping_iterations"]
        return dict(**c, gaussians_first=ns[0] if ns else 0, gaussians_last=self._n(), gaussians_max=max(ns) if ns else 0,
                    size_changes_by_densification=sum(1 for e, _ in self.gaussian_counts if e == "densify"),
                    size_changes_by_pruning=sum(1 for e, _ in self.gaussian_counts if e == "prune"),
                    seconds={k: round(v, 4) for k, v in s.items()},
                    frames_per_s=None if not s.get("wall") else round(c["frames"] / s["wall"], 3),
                    tracking_plus_mapping_iterations_per_s=None if not loops else round(its / loops, 2),
                    tracking_iterations_per_s=None if not s.get("tracking") else round(c["tracking_iterations"] / s["tracking"], 2),
                    mapping_iterations_per_s=None if not s.get("mapping") else round(c["mapping_iterations"] / s["mapping"], 2),
                    **({"depth_align": list(self.depth_align_log)} if self.patch_align else {}),
                    **({"pose_init": list(self.pose_init_log)} if self.pose_init is not None else {}))
