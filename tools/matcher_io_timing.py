"""Times the matcher I/O -- ``init_pose.format_image`` (one ``lvdgs_format_image`` call) and ``depth_utils.scale_from_matches`` (one
``lvdgs_match_depth_scale`` call) -- against restatements of the reference's routes on the same machine and inputs.

A. The image formatting, on a KITTI frame (1226 x 370 -> 512 x 144, LANCZOS), its half size (613 x 185) and a small frame that grows
   (320 x 240 -> 512 x 384, BICUBIC).  The baseline is the reference's own route (utils/init_pose.py:49-72): device-to-host copy, uint8,
   ``PIL.Image.resize``, crop, normalise, upload.  It needs PIL; where PIL does not import the baseline is reported as unavailable.
   The two results must be bit-identical.
B. The depth scale at the matches, 1152 matches (the seeds' grid of a 512 x 144 raster) over two 1226 x 370 depth maps and over two
   613 x 185 ones.  The baseline is PyTorch on the same GPU, as the reference resizes WHOLE maps: ``F.interpolate(bilinear,
   align_corners=False)`` of both to the raster, a gather at the matches, masked means, one read-back.  The two scales must agree to
   1e-5 relative.

Every call is timed with device events on the current stream around the whole call (the baselines' host work included: the second
event is recorded when the host gets there) after a warm-up; the two sides alternate in one loop; medians are reported.
``--only hip --calls N`` just makes N calls of each HIP entry point (for a kernel trace: ``rocprofv3 --kernel-trace --stats -d DIR --
python tools/matcher_io_timing.py --only hip --calls 20``).  One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import depth_utils, init_pose  # noqa: E402

try:
    import PIL.Image
except ImportError:
    PIL = None


def reference_format(image, size=512):
    """The reference's route for one frame: (3, H, W) float tensor on the GPU -> (1, 3, H1, W1) float32 on the GPU, through the host."""
    dev = image.device
    q = (image.permute(1, 2, 0).cpu().numpy() * 255).clip(0, 255).astype(np.uint8)      # (the clamp: formatting's stated deviation)
    img = PIL.Image.fromarray(q, "RGB")
    S = max(img.size)
    img = img.resize(tuple(int(round(x * size / S)) for x in img.size), PIL.Image.LANCZOS if S > size else PIL.Image.BICUBIC)
    W, H = img.size
    cx, cy = W // 2, H // 2
    halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    if W == H:
        halfh = 3 * halfw // 4
    img = img.crop((cx - halfw, cy - halfh, cx + halfw, cy + halfh))
    t = torch.from_numpy(np.asarray(img)).permute(2, 0, 1).contiguous().float().div(255)      # ToTensor
    return t.sub_(0.5).div_(0.5)[None].to(dev)                                                    # Normalize, upload


def torch_scale(m1, m2, d1, d2, raster):
    """``find_scale``'s arithmetic on whole maps in PyTorch -> float (NaN without a valid match)."""
    W1, H1 = raster
    a = F.interpolate(d1[None, None], size=(H1, W1), mode="bilinear", align_corners=False)[0, 0]
    b = F.interpolate(d2[None, None], size=(H1, W1), mode="bilinear", align_corners=False)[0, 0]
    x2, y2 = m2[:, 0].long(), m2[:, 1].long()
    va, vb = a[m1[:, 1].long(), m1[:, 0].long()], b[y2, x2]
    ok = (va > 0) & torch.isfinite(va) & (vb > 0) & torch.isfinite(vb)
    va, vb = va.double(), vb.double()
    zero = torch.zeros_like(va)
    return float((torch.where(ok, va, zero).sum() / ok.sum()) / (torch.where(ok, vb, zero).sum() / ok.sum()))


def time_calls(fns, calls, warmup, dev):
    """Median / min / max milliseconds of each callable, alternating them, by device events around the whole call."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), calls=len(v)) for k, v in ms.items()}


def smooth_image(H, W, dev, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, H // 8 + 2, W // 8 + 2), generator=g)
    img = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)[0] + 0.05 * torch.rand((3, H, W), generator=g)
    return img.clamp(0, 1).to(dev)


def depth_map(H, W, dev, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 1, H // 16 + 2, W // 16 + 2), generator=g) * 30 + 4
    d = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)[0, 0]
    d[torch.rand((H, W), generator=g) < 0.05] = 0.0      # holes, as a rendered or masked depth has them
    return d.contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["hip"], default=None, help="hip: only make --calls calls of each HIP entry point (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for (W, H) in ((1226, 370), (613, 185), (320, 240)):
        img = smooth_image(H, W, dev, W)
        hip = lambda: init_pose.format_image(img, 512)
        if a.only == "hip":
            for _ in range(a.calls):
                hip()
            torch.cuda.synchronize(dev)
            continue
        fns = {"hip": hip}
        rec = dict(what="format_image", frame=f"{H}x{W}", raster="{1}x{0}".format(*init_pose.matcher_raster(W, H)), pil=None if PIL is None else PIL.__version__)
        if PIL is not None:
            fns["reference_route"] = lambda: reference_format(img, 512)
            rec["bit_identical"] = bool(torch.equal(hip(), reference_format(img, 512)))
        else:
            rec["note"] = "PIL does not import here: no baseline"
        out = time_calls(fns, a.calls, a.warmup, dev)
        if PIL is not None:
            rec["baseline_over_hip"] = round(out["reference_route"]["median_ms"] / out["hip"]["median_ms"], 2)
        print(json.dumps(dict(rec, **out)), flush=True)
    raster = (512, 144)
    ys, xs = torch.meshgrid(torch.arange(4, raster[1], 8), torch.arange(4, raster[0], 8), indexing="ij")
    m1 = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).int().to(dev)
    g = torch.Generator().manual_seed(1)
    m2 = (m1.cpu().float() + (torch.rand(m1.shape, generator=g) * 6 - 3)).clamp_(min=0)
    m2[:, 0].clamp_(max=raster[0] - 1)
    m2[:, 1].clamp_(max=raster[1] - 1)
    m2 = m2.to(dev)
    for (W, H) in ((1226, 370), (613, 185)):
        d1, d2 = depth_map(H, W, dev, 2), depth_map(H, W, dev, 3) * 0.7
        hip = lambda: depth_utils.scale_from_matches(m1, m2, d1, d2, raster)
        if a.only == "hip":
            for _ in range(a.calls):
                hip()
            continue
        s_hip, s_torch = hip(), torch_scale(m1, m2, d1, d2, raster)
        ls = depth_utils.last_scale
        out = time_calls({"hip": hip, "torch_baseline": lambda: torch_scale(m1, m2, d1, d2, raster)}, a.calls, a.warmup, dev)
        print(json.dumps(dict(what="scale_from_matches", maps=f"{H}x{W}", raster=f"{raster[1]}x{raster[0]}", matches=ls.matches, valid=ls.valid,
                              scale=s_hip, torch_scale=s_torch, relative_difference=abs(s_hip - s_torch) / abs(s_torch),
                              agree_to_1e_5=bool(abs(s_hip - s_torch) <= 1e-5 * abs(s_torch)),
                              baseline_over_hip=round(out["torch_baseline"]["median_ms"] / out["hip"]["median_ms"], 2), **out)), flush=True)


if __name__ == "__main__":
    main()
