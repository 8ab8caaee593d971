"""The per-frame block of the reference's ``eval_rendering`` (utils/eval_utils_0806.py:216-312), restated on the CPU as the yardstick of
``lvdgs_frame_eval``: float64 for the sums and for SSIM (oracle/loss_oracle.py, imported, not changed), and the reference's NumPy
float32 statements, verbatim in their order, for the 8-bit images."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import loss_oracle as lo  # noqa: E402


def plane_mask(static_mask):
    """The mask shapes the reference accepts (:253-254) -> (H, W) bool, or None."""
    if static_mask is None:
        return None
    m = np.asarray(static_mask)
    if m.ndim == 3:
        m = m.squeeze(-1) if m.shape[-1] == 1 else m.squeeze(0)
    assert m.ndim == 2
    return m != 0


def frame_eval(render, gt, static_mask=None, bg=None, depth=None):
    """render, gt: (3, H, W) float32 arrays; static_mask: one plane or None; bg: 3 values or None; depth: (H, W) float32 or None.
    -> what a row of the library holds (sums and SSIM in float64, exact counts) and the byte images."""
    render, gt = np.asarray(render, np.float32), np.asarray(gt, np.float32)
    a = np.minimum(np.maximum(render, np.float32(0)), np.float32(1))      # torch.clamp(rendering, 0.0, 1.0): exact in float32
    basic = gt > 0
    m = plane_mask(static_mask)
    keep = basic if m is None else basic & m[None]
    sq = (a.astype(np.float64) - gt.astype(np.float64)) ** 2
    out = dict(has_mask=m is not None, n_basic=int(basic.sum()), n_keep=int(keep.sum()),
               sum_sq_full=float(sq[basic].sum()), sum_sq_static=float(sq[keep].sum()),
               ssim_full=float(lo.ssim(torch.from_numpy(a), torch.from_numpy(gt))))
    if m is None:
        out["ssim_static"] = out["ssim_full"]
    else:
        fill = np.broadcast_to((np.zeros(3, np.float32) if bg is None else np.asarray(bg, np.float32)).reshape(3, 1, 1), a.shape)
        out["ssim_static"] = float(lo.ssim(torch.from_numpy(np.where(keep, a, fill)), torch.from_numpy(np.where(keep, gt, fill))))
    # :309-312, verbatim in order (NumPy float32; `* 255` keeps float32)
    gt8 = (gt.transpose((1, 2, 0)) * 255).astype(np.uint8)
    pred8 = (a.transpose((1, 2, 0)) * 255).astype(np.uint8)
    residual = np.abs(pred8.astype(np.float32) - gt8.astype(np.float32))
    out.update(pred8=pred8, gt8=gt8, residual8=np.clip(residual, 0, 255).astype(np.uint8))
    if depth is not None:
        depth_np = np.asarray(depth, np.float32)
        depth_np = depth_np.reshape(gt.shape[1:])      # (the reference's squeeze(), which would also drop the axes of a 1 x 1 frame)
        depth_max = depth_np.max()      # :222-225
        depth_min = depth_np.min()
        out.update(depth_min=float(depth_min), depth_max=float(depth_max), depth_constant=bool(depth_max == depth_min))
        if depth_max == depth_min:      # the reference's 0 / 0 cast to uint8 is undefined; the library's definition is 0
            out["depth8"] = np.zeros(depth_np.shape, np.uint8)
        else:
            depth_nor = (depth_np - depth_min) / (depth_max - depth_min)
            out["depth8"] = (depth_nor * 255).astype(np.uint8)
    return out


def psnr_of_sum(n, total):
    if n == 0:
        return float("nan")
    return float("inf") if total == 0.0 else 10.0 * math.log10(n / total)


def metrics(o, elements):
    """``frame_metrics``'s dict from ``frame_eval``'s output, with the reference's fallback (:273, :302-306)."""
    out = {"psnr": psnr_of_sum(o["n_basic"], o["sum_sq_full"]), "ssim": o["ssim_full"]}
    out["psnr_static"], out["ssim_static"], out["static_ratio"] = out["psnr"], out["ssim"], None
    if o["has_mask"] and o["n_keep"] > 0:
        out.update(psnr_static=psnr_of_sum(o["n_keep"], o["sum_sq_static"]), ssim_static=o["ssim_static"], static_ratio=o["n_keep"] / elements)
    return out


# ---- the fixture of tests/golden/make_eval_golden.py (the reference's own eval_rendering on five frames of the toy scene)
PSNR_TOL, SSIM_TOL = 1e-3, 2e-6      # the bounds tests/test_gpu_ssim.py::test_frame_metrics_of_the_eval_harness holds this path to


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "eval_rendering.npz"))
    frames = []
    for idx in z["evaluated"].tolist():
        static = z[f"static_mask_{idx}"] if f"static_mask_{idx}" in z.files else None
        expanded = z[f"expanded_static_mask_{idx}"] if f"expanded_static_mask_{idx}" in z.files else None
        # utils/eval_utils_0806.py:246-250: the expanded mask is looked at only when static_mask is set
        used = None if static is None else (expanded if expanded is not None else static)
        frames.append(dict(idx=idx, render=z[f"render_{idx}"], gt=z[f"gt_{idx}"], depth=z[f"depth_{idx}"], static_mask=static,
                           expanded_static_mask=expanded, used_mask=used, png_rgb=z[f"png_rgb_{idx}"], png_depth=z[f"png_depth_{idx}"],
                           npy_depth=z[f"npy_depth_{idx}"]))
    return dict(frames=frames, background=z["background"], result=json.loads(str(z["result"])), json=json.loads(str(z["json"])),
                files=json.loads(str(z["files"])), kf_indices=z["kf_indices"].tolist(), num_frames=int(z["num_frames"]))


def check_means(rows, result):
    """``rows``: frame_metrics-shaped dicts of the fixture's frames -> the reference's means within the bounds."""
    for key, tol in (("psnr", PSNR_TOL), ("ssim", SSIM_TOL), ("psnr_static", PSNR_TOL), ("ssim_static", SSIM_TOL)):
        got = float(np.mean([r[key] for r in rows]))
        print(f"mean_{key}: got {got!r} reference {result['mean_' + key]!r}")
        assert abs(got - result["mean_" + key]) < tol, key
