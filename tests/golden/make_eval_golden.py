#!/usr/bin/env python3
"""Run the reference's OWN ``eval_rendering`` (utils/eval_utils_0806.py:172-437) on a few frames of the toy scene and store its inputs
and what it returned and wrote, as the fixture ``lvdgs_frame_eval`` and ``eval_utils.eval_rendering`` are held to.

Run in the authoring container only (needs the reference checkout; never on the GPU box):

    python -B tests/golden/make_eval_golden.py

How the reference's function is made to run here (CPU, no CUDA), following make_loop_golden.py:
  * ``torch.Tensor.cuda`` is the identity; ``evo`` (and the submodules the file imports), ``wandb``, ``cv2`` and
    ``torchmetrics.image.lpip`` are empty stand-in modules, the LPIPS class returns a constant;
  * ``gaussian_splatting.*`` resolves to the drop-in shims (lvd_gs-slam_amd/dropin);
  * ``render`` in its namespace is the dense renderer of tests/dense_render.py, pushed outside [0, 1] (x 1.8 - 0.25) so that the
    clamp matters; ``ssim`` is the float64 statement of oracle/loss_oracle.py; the save directory is temporary.
The evaluated frames cover: no mask; ``static_mask`` only; both masks (the expanded one wins); a mask that keeps nothing; a
(1, H, W) mask.  The ground-truth images carry black pixels in single channels.
Nothing of the reference's text is stored: only the inputs and the numbers / bytes its function produced.

Fixture: tests/golden/eval_rendering.npz.
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LVDGS_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "lvd_gs-slam_amd", "dropin"), REF):
    sys.path.insert(0, p)

import lvdgs  # noqa: E402,F401
import loss_oracle as lo  # noqa: E402
from dense_render import dense_render  # noqa: E402
from loop_scene import H, W, build_scene  # noqa: E402

LPIPS_CONSTANT = 0.25
KF_INDICES = [0, 3]
BACKGROUND = [0.1, 0.6, 0.3]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class _Lpips:
    def __init__(self, *a, **k):
        pass

    def to(self, *a, **k):
        return self

    def __call__(self, a, b):
        return torch.tensor(LPIPS_CONSTANT)


def load_reference():
    torch.Tensor.cuda = lambda self, *a, **k: self
    _stub("cv2")
    _stub("wandb", log=lambda *a, **k: None)
    anything = type("Anything", (), {})
    evo = _stub("evo")
    evo.core = _stub("evo.core")
    evo.core.metrics = _stub("evo.core.metrics", PoseRelation=anything, Unit=anything)
    evo.core.trajectory = _stub("evo.core.trajectory", PosePath3D=anything, PoseTrajectory3D=anything)
    evo.core.geometry = _stub("evo.core.geometry", GeometryException=Exception)
    evo.tools = _stub("evo.tools")
    evo.tools.plot = _stub("evo.tools.plot", PlotMode=anything)
    evo.tools.settings = _stub("evo.tools.settings", SETTINGS=anything())
    tm = _stub("torchmetrics")
    tm.image = _stub("torchmetrics.image")
    tm.image.lpip = _stub("torchmetrics.image.lpip", LearnedPerceptualImagePatchSimilarity=_Lpips)
    mod = importlib.import_module("utils.eval_utils_0806")
    mod.ssim = lambda a, b: lo.ssim(a, b)
    return mod


def main():
    mod = load_reference()
    sc = build_scene("cpu")
    frames = {i: c for i, c in enumerate(sc["cameras"] + [sc["track_camera"]])}      # 8 frames: end_idx = 7
    background = torch.tensor(BACKGROUND)
    gen = torch.Generator().manual_seed(5)
    gts = []
    for i in range(len(frames)):
        gt = frames[i].original_image.clone().clamp(0, 1)
        for c in range(3):      # black pixels in single channels, elsewhere strictly positive
            gt[c] = torch.where(torch.rand(H, W, generator=gen) < 0.08, torch.zeros(()), gt[c].clamp(min=1.0 / 512))
        gt[:, :3, :] = 0.0      # and a black border in all three
        gts.append(gt)
    dataset = [(g, None, None, None) for g in gts]
    for f in frames.values():
        f.static_mask = None
        f.expanded_static_mask = None
    m2 = torch.rand(H, W, generator=gen) > 0.3
    frames[2].static_mask = m2
    frames[4].static_mask = torch.rand(H, W, generator=gen) > 0.2
    frames[4].expanded_static_mask = frames[4].static_mask & (torch.rand(H, W, generator=gen) > 0.3)
    frames[5].static_mask = torch.zeros(H, W, dtype=torch.bool)
    frames[6].static_mask = (torch.rand(H, W, generator=gen) > 0.5)[None]
    frames[1].expanded_static_mask = torch.zeros(H, W, dtype=torch.bool)      # not looked at: static_mask is None (:246)

    seen = {}

    def render(frame, gaussians, pipe, bg):
        with torch.no_grad():
            pkg = dense_render(frame, gaussians, pipe, bg)
        pkg = dict(pkg)
        pkg["render"] = (pkg["render"] * 1.8 - 0.25).float().contiguous()
        seen[int(frame.uid)] = (pkg["render"].numpy().copy(), pkg["depth"].numpy().copy())
        return pkg
    mod.render = render

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        result = mod.eval_rendering(frames, sc["gaussians"], dataset, tmp, sc["pipe"], background, "monocular", KF_INDICES, iteration="before_opt")
        from PIL import Image
        evaluated = sorted(seen)
        for idx in evaluated:
            out[f"png_rgb_{idx}"] = np.array(Image.open(os.path.join(tmp, "render_rgb", f"{idx}_pred.png")))
            out[f"png_depth_{idx}"] = np.array(Image.open(os.path.join(tmp, "render_depth", f"{idx}_pred.png")))
            out[f"npy_depth_{idx}"] = np.load(os.path.join(tmp, "render_depth_npy", f"{idx}_pred.npy"))
        out["json"] = np.array(json.dumps(json.load(open(os.path.join(tmp, "psnr", "before_opt", "final_result.json")))))
        out["files"] = np.array(json.dumps(sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)))
    assert evaluated == [i for i in range(len(frames) - 1) if i not in KF_INDICES], evaluated
    out["evaluated"] = np.array(evaluated)
    out["kf_indices"] = np.array(KF_INDICES)
    out["num_frames"] = np.array(len(frames))
    out["background"] = background.numpy()
    out["result"] = np.array(json.dumps(result))
    for idx in evaluated:
        out[f"render_{idx}"], out[f"depth_{idx}"] = seen[idx]
        out[f"gt_{idx}"] = gts[idx].numpy()
        f = frames[idx]
        if f.static_mask is not None:
            out[f"static_mask_{idx}"] = f.static_mask.numpy()
        if f.expanded_static_mask is not None:
            out[f"expanded_static_mask_{idx}"] = f.expanded_static_mask.numpy()
    np.savez_compressed(os.path.join(HERE, "eval_rendering.npz"), **out)
    print("wrote eval_rendering.npz:", result, "frames", evaluated, os.path.getsize(os.path.join(HERE, "eval_rendering.npz")), "bytes")


if __name__ == "__main__":
    main()
