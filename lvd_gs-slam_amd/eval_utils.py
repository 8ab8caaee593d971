"""Trajectory and rendering metrics of the evaluation harness, without its plotting / logging dependencies.

Counterpart of the numbers ``utils/eval_utils_0806.py`` produces (it needs ``evo``, ``wandb``, ``lpips``,
``cv2`` and ``matplotlib``, none of which is part of the hot path):

* ``evaluate_ate`` -- ``evaluate_evo`` (:33-98): Umeyama alignment of the estimated keyframe trajectory onto
  the ground truth (with scale for monocular runs), falling back to aligning the first poses when either
  trajectory spans less than 0.1 m (:42-56); APE on the translation part; ``rmse`` and evo's other statistics.
  ``evo`` is not installed, so the alignment follows the published algorithm (Umeyama, PAMI 1991) [unpinned].
* ``eval_ate`` -- (:101-169): camera-to-world poses from the keyframes' ``R, T`` / ``R_gt, T_gt``.
* ``frame_metrics`` -- the per-frame block of ``eval_rendering`` (:231-306): PSNR on non-black pixels, SSIM on
  the full frame, and the static-region variants (mask = non-black & static; SSIM with the dynamic pixels of
  both images overwritten by the background colour).  SSIM runs on the fused HIP kernel.
* ``FrameEvaluator`` -- the same block as ONE library call per frame and no host wait (``lvdgs_frame_eval``): the sums, counts, both
  SSIM means and the depth extrema land in a row of a device table that ``results()`` reads once; optionally the 8-bit images the
  reference saves (:221-230, :309-312) are left on the device.  ``frame_metrics(fused=True)`` is a one-row evaluator.
* ``eval_rendering`` -- the reference's function (:172-437) by its positional signature and its loop: keyframes skipped,
  ``end_idx = len(frames) - 1``, the static means, ``psnr/<iteration>/final_result.json``.  LPIPS has no weights here: its keys
  appear only with ``lpips_fn``.  The matplotlib figure, wandb and ``Log`` are not restated.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import torch


class AlignmentError(ValueError):
    pass


def umeyama_alignment(x, y, with_scale=False):
    """Least-squares similarity (r, t, c) with ``y ~ c * r @ x + t`` for point sets ``x, y`` of shape (m, n)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != y.shape:
        raise AlignmentError("point sets must have the same shape")
    m, n = x.shape
    mean_x, mean_y = x.mean(axis=1), y.mean(axis=1)
    sigma_x = ((x - mean_x[:, None]) ** 2).sum() / n
    cov = (y - mean_y[:, None]) @ (x - mean_x[:, None]).T / n
    u, d, vt = np.linalg.svd(cov)
    if np.count_nonzero(d > np.finfo(d.dtype).eps) < m - 1:
        raise AlignmentError("degenerate covariance rank, Umeyama alignment is not possible")
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        s[m - 1, m - 1] = -1.0
    r = u @ s @ vt
    c = float(np.trace(np.diag(d) @ s) / sigma_x) if with_scale else 1.0
    t = mean_y - c * (r @ mean_x)
    return r, t, c


def trajectory_has_diversity(poses, min_translation=0.1):
    """utils/eval_utils_0806.py:42-48."""
    if len(poses) < 3:
        return False
    positions = np.array([p[:3, 3] for p in poses])
    return float(np.sqrt(np.sum(np.ptp(positions, axis=0) ** 2))) > min_translation


def align_trajectory(poses_est, poses_ref, correct_scale=False):
    """Similarity-align estimated camera-to-world poses onto the reference ones (positions drive the fit)."""
    est = [np.asarray(p, np.float64).copy() for p in poses_est]
    ref = [np.asarray(p, np.float64) for p in poses_ref]
    r, t, c = umeyama_alignment(np.array([p[:3, 3] for p in est]).T, np.array([p[:3, 3] for p in ref]).T, correct_scale)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = r, t
    out = []
    for p in est:
        p[:3, 3] *= c
        out.append(T @ p)
    return out


def align_trajectory_origin(poses_est, poses_ref):
    """Rigidly move the estimate so that its first pose coincides with the reference's first pose."""
    to_ref = np.asarray(poses_ref[0], np.float64) @ np.linalg.inv(np.asarray(poses_est[0], np.float64))
    return [to_ref @ np.asarray(p, np.float64) for p in poses_est]


def evaluate_ate(poses_gt, poses_est, monocular=False):
    """-> (rmse, statistics dict, aligned estimate); mirrors evaluate_evo's choice of alignment."""
    try:
        if not trajectory_has_diversity(poses_gt) or not trajectory_has_diversity(poses_est):
            aligned = align_trajectory_origin(poses_est, poses_gt)
        else:
            aligned = align_trajectory(poses_est, poses_gt, correct_scale=monocular)
    except AlignmentError:
        aligned = [np.asarray(p, np.float64) for p in poses_est]
    err = np.array([np.linalg.norm(a[:3, 3] - np.asarray(g, np.float64)[:3, 3]) for a, g in zip(aligned, poses_gt)])
    stats = {"rmse": float(np.sqrt(np.mean(err ** 2))), "mean": float(err.mean()), "median": float(np.median(err)),
             "std": float(err.std()), "min": float(err.min()), "max": float(err.max()), "sse": float(np.sum(err ** 2))}
    return stats["rmse"], stats, aligned


def eval_ate(frames, kf_ids, monocular=False):
    """ATE RMSE over the keyframes (utils/eval_utils_0806.py:101-169); None with fewer than 3."""
    if len(frames) < 3 or len(kf_ids) < 3:
        return None

    def c2w(R, T):
        pose = np.eye(4)
        pose[:3, :3] = R.detach().cpu().numpy()
        pose[:3, 3] = T.detach().cpu().numpy()
        return np.linalg.inv(pose)

    est = [c2w(frames[k].R, frames[k].T) for k in kf_ids]
    gt = [c2w(frames[k].R_gt, frames[k].T_gt) for k in kf_ids]
    return evaluate_ate(gt, est, monocular=monocular)[0]


def frame_metrics(rendering, gt_image, static_mask=None, background=None, fused=False):
    """PSNR / SSIM of one rendered frame and their static-region variants (utils/eval_utils_0806.py:231-306).  ``fused``: one
    ``lvdgs_frame_eval`` call and one read of its row instead of the statements below."""
    if fused:
        key = (int(rendering.shape[-2]), int(rendering.shape[-1]), rendering.device)
        ev = _single_row.get(key)
        if ev is None:
            _single_row.clear()      # one evaluator, of the last size asked for: nothing piles up on the device
            ev = _single_row[key] = FrameEvaluator(key[0], key[1], key[2], 1)
        ev.reset()
        ev.add(rendering, gt_image, static_mask, background)
        row = ev.results()[0]
        return {k: row[k] for k in ("psnr", "ssim", "psnr_static", "ssim_static", "static_ratio")}
    from .image_utils import psnr
    from .loss_utils import ssim

    image = torch.clamp(rendering.detach(), 0.0, 1.0)
    basic = gt_image > 0
    out = {"psnr": float(psnr(image[basic].unsqueeze(0), gt_image[basic].unsqueeze(0))),
           "ssim": float(ssim(image.unsqueeze(0), gt_image.unsqueeze(0)))}
    out["psnr_static"], out["ssim_static"], out["static_ratio"] = out["psnr"], out["ssim"], None
    if static_mask is not None:
        m = static_mask
        if m.dim() == 3:
            m = m.squeeze(-1) if m.shape[-1] == 1 else m.squeeze(0)
        if m.dim() == 2:
            m = m.unsqueeze(0).expand(3, -1, -1)
        keep = basic & m.to(device=image.device, dtype=torch.bool)
        if bool(keep.any()):
            bg = torch.zeros(3, device=image.device) if background is None else background.to(image.device)
            fill = bg.view(3, 1, 1).expand_as(image)
            out["psnr_static"] = float(psnr(image[keep].unsqueeze(0), gt_image[keep].unsqueeze(0)))
            out["ssim_static"] = float(ssim(torch.where(keep, image, fill).unsqueeze(0), torch.where(keep, gt_image, fill).unsqueeze(0)))
            out["static_ratio"] = float(keep.float().mean())
    return out


_single_row = {}      # (H, W, device) -> the one-row evaluator of frame_metrics(fused=True); holds the last key only


def _psnr_of_sum(n, total):
    """10 log10(n / sum) in float64: the reference's 20 log10(1 / sqrt(mse)) with mse = sum / n; inf for a zero sum, nan without elements."""
    n, total = float(n), float(total)
    if n == 0.0:
        return float("nan")
    return float("inf") if total == 0.0 else 10.0 * math.log10(n / total)


class FrameEvaluator:
    """The per-frame block of ``eval_rendering`` on the device: ``add`` enqueues one ``lvdgs_frame_eval`` call on the current stream
    and returns at once; ``results`` reads the table of rows in one device-to-host copy.  ``want_images``: the call also leaves
    ``pred8`` / ``gt8`` / ``residual8`` (H, W, 3) and, with a depth map, ``depth8`` (H, W) on the device (``images``)."""

    def __init__(self, height, width, device, capacity, want_images=False):
        from . import _lib
        self.height, self.width, self.device, self.capacity = int(height), int(width), torch.device(device), int(capacity)
        if self.height <= 0 or self.width <= 0 or self.capacity <= 0:
            raise ValueError("FrameEvaluator: height, width and capacity must be positive")
        if self.device.type != "cuda":
            raise _lib.LvdgsError("FrameEvaluator needs a GPU device: there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.rows = torch.zeros((self.capacity, _lib.FRAME_EVAL_ROW_BYTES), dtype=torch.uint8, device=self.device)
        self.scratch = _lib.DeviceScratch()
        self.scratch_bytes = int(_lib.lib().lvdgs_frame_eval_scratch_bytes(self.width, self.height))
        self.want_images, self.count, self.last_had_depth = bool(want_images), 0, False
        self.buffers = None
        if self.want_images:
            mk = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=self.device)
            self.buffers = dict(pred8=mk(self.height, self.width, 3), gt8=mk(self.height, self.width, 3),
                                residual8=mk(self.height, self.width, 3), depth8=mk(self.height, self.width))
        self._fn = _lib.lib().lvdgs_frame_eval

    def reset(self):
        """Start the table over (rows already written are overwritten by the next calls)."""
        self.count = 0

    def _image(self, t, name, planes):
        if not torch.is_tensor(t) or t.device != self.device:
            raise ValueError(f"FrameEvaluator.add: {name} must be a tensor on {self.device}")
        if t.dtype is not torch.float32:
            raise TypeError(f"FrameEvaluator.add: {name} must be float32, got {t.dtype}")
        t = t.detach()
        if planes == 1 and t.dim() == 3 and 1 in (t.shape[0], t.shape[-1]):
            t = t.squeeze(0) if t.shape[0] == 1 else t.squeeze(-1)
        want = (planes, self.height, self.width) if planes == 3 else (self.height, self.width)
        if tuple(t.shape) != want:
            raise ValueError(f"FrameEvaluator.add: {name} has shape {tuple(t.shape)}, expected {want}")
        return t.contiguous()

    def _mask(self, m):
        if not torch.is_tensor(m) or m.device != self.device:
            raise ValueError(f"FrameEvaluator.add: static_mask must be a tensor on {self.device}")
        if m.dim() == 3:      # the shapes frame_metrics accepts: (H, W), (1, H, W), (H, W, 1)
            m = m.squeeze(-1) if m.shape[-1] == 1 else m.squeeze(0)
        if tuple(m.shape) != (self.height, self.width):
            raise ValueError(f"FrameEvaluator.add: static_mask has shape {tuple(m.shape)}, expected one plane of {(self.height, self.width)}")
        if m.dtype is torch.bool:
            return m.contiguous().view(torch.uint8)
        if m.dtype is torch.uint8:
            return m.contiguous()
        return (m != 0).view(torch.uint8)

    def add(self, rendering, gt_image, static_mask=None, background=None, depth=None):
        """Enqueue the evaluation of one frame -> its row index.  No wait.  Raises when the table is full or a tensor is on another
        device or of another dtype than the call takes (float32 images and depth; a bool, uint8 or numeric mask)."""
        from . import _lib
        if self.count >= self.capacity:
            raise IndexError(f"FrameEvaluator.add: the table of {self.capacity} rows is full")
        render = self._image(rendering, "rendering", 3)
        gt = self._image(gt_image, "gt_image", 3)
        mask = None if static_mask is None else self._mask(static_mask)
        bg = None
        if background is not None:
            if not torch.is_tensor(background) or background.device != self.device or background.numel() != 3:
                raise ValueError(f"FrameEvaluator.add: background must be 3 values on {self.device}")
            bg = _lib.f32(background, self.device)
        d = None if depth is None else self._image(depth, "depth", 1)
        scratch = self.scratch.get(self.device, self.scratch_bytes)
        index = self.count
        a = _lib.FrameEvalArgs()
        a.width, a.height = self.width, self.height
        a.render, a.gt_image, a.static_mask, a.bg, a.depth = _lib.ptr(render), _lib.ptr(gt), _lib.ptr(mask), _lib.ptr(bg), _lib.ptr(d)
        a.out_row = C.c_void_p(self.rows.data_ptr() + index * _lib.FRAME_EVAL_ROW_BYTES)
        if self.want_images:
            b = self.buffers
            a.pred8, a.gt8, a.residual8 = _lib.ptr(b["pred8"]), _lib.ptr(b["gt8"]), _lib.ptr(b["residual8"])
            a.depth8 = _lib.ptr(b["depth8"]) if d is not None else None
        a.scratch, a.scratch_bytes = _lib.ptr(scratch), scratch.numel()
        with _lib.on_device(self.device):
            _lib.check(self._fn(C.byref(a), _lib.raw_stream(self.device)), "lvdgs_frame_eval")
        self.count, self.last_had_depth = index + 1, d is not None
        return index

    def images(self, index):
        """The device uint8 tensors of the LAST ``add`` (which must be ``index``): pred8, gt8, residual8 and, when that frame had a
        depth map, depth8.  The next ``add`` overwrites them."""
        if not self.want_images:
            raise ValueError("FrameEvaluator.images: built without want_images")
        if index != self.count - 1:
            raise IndexError(f"FrameEvaluator.images: only the last frame's images are held (row {self.count - 1}), asked for {index}")
        return {k: v for k, v in self.buffers.items() if k != "depth8" or self.last_had_depth}

    def read_table(self):
        """The rows written so far as a NumPy record array: THE one device-to-host read."""
        from . import _lib
        return self.rows[:self.count].cpu().numpy().view(_lib.FRAME_EVAL_ROW_DTYPE).reshape(-1)

    def results(self):
        """-> one dict per added frame, in order: ``frame_metrics``'s keys plus ``depth_min`` / ``depth_max`` (None without a depth map).
        PSNR = 10 log10(n / sum) in float64; with no mask, or a mask that keeps nothing, the static values are the full ones and
        ``static_ratio`` is None (utils/eval_utils_0806.py:273, :302-306)."""
        from . import _lib
        out = []
        elements = 3.0 * self.height * self.width
        for r in self.read_table():
            flags = int(r["flags"])
            m = {"psnr": _psnr_of_sum(r["n_basic"], r["sum_sq_full"]), "ssim": float(r["ssim_full"])}
            m["psnr_static"], m["ssim_static"], m["static_ratio"] = m["psnr"], m["ssim"], None
            if flags & _lib.FRAME_EVAL_HAS_MASK and int(r["n_keep"]) > 0:
                m["psnr_static"] = _psnr_of_sum(r["n_keep"], r["sum_sq_static"])
                m["ssim_static"] = float(r["ssim_static"])
                m["static_ratio"] = float(r["n_keep"]) / elements
            has_depth = bool(flags & _lib.FRAME_EVAL_HAS_DEPTH)
            m["depth_min"] = float(r["depth_min"]) if has_depth else None
            m["depth_max"] = float(r["depth_max"]) if has_depth else None
            out.append(m)
        return out


def quantised_images(image, gt_image, depth=None):
    """The reference's own host statements for what it saves (utils/eval_utils_0806.py:221-225, :309-312), NumPy float32 in its order:
    -> dict(pred8, gt8, residual8[, depth8, depth]).  ``image``: already clamped."""
    gt = (gt_image.detach().cpu().numpy().transpose((1, 2, 0)) * 255).astype(np.uint8)
    pred = (image.detach().cpu().numpy().transpose((1, 2, 0)) * 255).astype(np.uint8)
    residual = np.abs(pred.astype(np.float32) - gt.astype(np.float32))
    out = dict(pred8=pred, gt8=gt, residual8=np.clip(residual, 0, 255).astype(np.uint8))
    if depth is not None:
        depth_np = depth.detach().squeeze().cpu().numpy()
        depth_max, depth_min = depth_np.max(), depth_np.min()
        if depth_max == depth_min:      # the reference divides by zero here; the library's definition: zeros
            out["depth8"] = np.zeros(depth_np.shape, np.uint8)
        else:
            out["depth8"] = (((depth_np - depth_min) / (depth_max - depth_min)) * 255).astype(np.uint8)
        out["depth"] = depth_np
    return out


def _frame_static_mask(frame):
    """utils/eval_utils_0806.py:246-250: ``expanded_static_mask`` is looked at only when ``static_mask`` is set."""
    static = getattr(frame, "static_mask", None)
    if static is not None and getattr(frame, "expanded_static_mask", None) is not None:
        static = frame.expanded_static_mask
    return static


def eval_rendering(frames, gaussians, dataset, save_dir, pipe, background, datatype, kf_indices, iteration="final", *, render_fn=None,
                   fused=True, save_images=False, lpips_fn=None, metrics_fn=None, prefetch=0):
    """The reference's ``eval_rendering`` (utils/eval_utils_0806.py:172-437): every non-keyframe frame in ``range(len(frames) - 1)``
    rendered and scored -> the ``mean_*`` dict, also written to ``<save_dir>/psnr/<iteration>/final_result.json``.

    ``fused``: one ``FrameEvaluator`` over the loop and one read at the end; otherwise ``frame_metrics`` per frame.  ``metrics_fn``
    ``(rendering, gt_image, static_mask, background) -> frame_metrics's dict`` replaces either.  ``save_images``: also
    ``render_rgb/{idx}_pred.png``, ``render_depth/{idx}_pred.png`` and ``render_depth_npy/{idx}_pred.npy`` (the fused path writes the
    device bytes).  ``lpips_fn(image, gt) -> 0-dim tensor``: adds the ``mean_lpips*`` keys; its values stay on the device until the
    end.  ``prefetch``: that many frames read ahead on ``dataset.FramePrefetcher``'s threads, in the order they are scored
    (``dataset`` is then a ``lvdgs.dataset`` one); the numbers and files are the same.  ``datatype`` is accepted and unused, as in the
    reference."""
    from .image_utils import mkdir_p
    if render_fn is None:
        from .gaussian_renderer import render as render_fn
    end_idx = len(frames) - 1      # (:185: `iteration == "final" or "before_opt"` is always true)
    if save_images:
        from PIL import Image
        for sub in ("render_rgb", "render_depth", "render_depth_npy"):
            mkdir_p(os.path.join(save_dir, sub))
    evaluator, rows, lpips_full, lpips_static = None, [], [], []
    scored = [idx for idx in range(0, end_idx) if idx not in kf_indices]
    source = dataset
    if prefetch > 0 and scored:
        from .dataset import FramePrefetcher
        source = FramePrefetcher(dataset, scored, depth=prefetch)
    try:
        for idx in scored:
            frame = frames[idx]
            gt_image = source[idx][0]
            with torch.no_grad():
                pkg = render_fn(frame, gaussians, pipe, background)
            rendering, depth = pkg["render"].detach(), pkg.get("depth")
            gt_image = gt_image.to(rendering.device)
            static = _frame_static_mask(frame)
            use_fused = fused and metrics_fn is None
            if use_fused:
                if evaluator is None:
                    evaluator = FrameEvaluator(rendering.shape[-2], rendering.shape[-1], rendering.device, max(end_idx, 1), want_images=save_images)
                # the reference moves the mask to the device itself (:247-250), as frame_metrics does; the evaluator takes device tensors only
                dev_static = None if static is None else static.to(rendering.device)
                dev_bg = background.to(rendering.device) if torch.is_tensor(background) else background
                row = evaluator.add(rendering, gt_image, dev_static, dev_bg, depth if save_images else None)
            else:
                rows.append((metrics_fn or frame_metrics)(rendering, gt_image, static, background))
            if lpips_fn is not None:
                image = torch.clamp(rendering, 0.0, 1.0)
                lpips_full.append(lpips_fn(image, gt_image).detach().reshape(()))
                m = static
                if m is not None:
                    if m.dim() == 3:
                        m = m.squeeze(-1) if m.shape[-1] == 1 else m.squeeze(0)
                    keep = (gt_image > 0) & m.to(device=image.device, dtype=torch.bool)
                    bg = torch.zeros(3, device=image.device) if background is None else background.to(image.device)
                    fill = bg.view(3, 1, 1).expand_as(image)
                    masked = lpips_fn(torch.where(keep, image, fill), torch.where(keep, gt_image, fill)).detach().reshape(())
                    # (:273, :302-306: a mask that keeps nothing scores the full frame) -- chosen on the device, no wait
                    lpips_static.append(torch.where(keep.any(), masked, lpips_full[-1]))
                else:
                    lpips_static.append(lpips_full[-1])
            if save_images:
                if use_fused:
                    q = {k: v.cpu().numpy() for k, v in evaluator.images(row).items()}
                    if depth is not None:
                        q["depth"] = depth.detach().squeeze().cpu().numpy()
                else:
                    q = quantised_images(torch.clamp(rendering, 0.0, 1.0), gt_image, depth)
                if "depth8" in q:
                    Image.fromarray(q["depth8"]).save(os.path.join(save_dir, "render_depth", f"{idx}_pred.png"), dpi=(300, 300))
                    np.save(os.path.join(save_dir, "render_depth_npy", f"{idx}_pred.npy"), q["depth"])
                Image.fromarray(q["pred8"]).save(os.path.join(save_dir, "render_rgb", f"{idx}_pred.png"), dpi=(300, 300))
    finally:
        if source is not dataset:
            source.close()
    if evaluator is not None:
        rows = evaluator.results()
    output = dict()
    mean = lambda key: float(np.mean([r[key] for r in rows])) if rows else float("nan")
    output["mean_psnr"], output["mean_ssim"] = mean("psnr"), mean("ssim")
    if lpips_fn is not None:
        output["mean_lpips"] = float(torch.stack(lpips_full).mean()) if lpips_full else float("nan")
    # (:304-306, :411-415) a frame without a mask, or whose mask keeps nothing, enters the static means with its full values: with no
    # masked frame at all the static means are the full ones
    output["mean_psnr_static"], output["mean_ssim_static"] = mean("psnr_static"), mean("ssim_static")
    if lpips_fn is not None:
        output["mean_lpips_static"] = float(torch.stack(lpips_static).mean()) if lpips_static else float("nan")
    psnr_save_dir = os.path.join(save_dir, "psnr", str(iteration))
    mkdir_p(psnr_save_dir)
    with open(os.path.join(psnr_save_dir, "final_result.json"), "w", encoding="utf-8") as f:
        json.dump(output, f, indent=4)
    return output
