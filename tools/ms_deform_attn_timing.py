"""Times ``lvdgs.ms_deform_attn`` (one ``lvdgs_ms_deform_attn_forward`` / ``_backward`` call) against a PyTorch restatement of the
operator's ``grid_sample`` formulation on the same GPU and inputs.

Shapes: the feature pyramids of the project's two frame sizes at strides 8 / 16 / 32 / 64 (the strides are recalled from
upstream's Swin-T config, which is not in the reference tree: UNVERIFIED), each with ``Q = S`` (an encoder layer) and ``Q = 900``
(a decoder layer); ``B = 1, H = 8, D = 32, P = 4``.  Locations are a reference point per query plus N(0, 2 px) offsets per
sample, weights a softmax over the 16 samples.

The baseline (``torch_ms_deform_attn``) states the operator the way GroundingDINO's ``multi_scale_deformable_attn_pytorch`` does:
per level a ``grid_sample(bilinear, zeros, align_corners=False)`` of the level's (B * H, D, h, w) image, then the weighted sum over
levels and points; its backward is autograd's.  It is the yardstick, not the code under test.

Every call is timed with device events on the current stream after a warm-up; the sides alternate in one loop; medians are
reported, with the forward's gathered bytes per second (``B Q H L P 4 D 4`` bytes per call).  ``--only hip --calls N`` just makes N
calls of each (for a kernel trace).  One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import ms_deform_attn as mda  # noqa: E402

FRAMES = {
    "kitti_1226x370": ((47, 154), (24, 77), (12, 39), (6, 20)),          # S = 9674
    "1920x1080": ((135, 240), (68, 120), (34, 60), (17, 30)),            # S = 43110
}
H, D, P = 8, 32, 4


def torch_ms_deform_attn(value, levels, loc, weights):
    B, S, Hh, Dd = value.shape
    _, Q, _, L, Pp, _ = loc.shape
    grids = 2 * loc - 1
    sampled, start = [], 0
    for l, (h, w) in enumerate(levels):
        img = value[:, start:start + h * w].flatten(2).transpose(1, 2).reshape(B * Hh, Dd, h, w)
        grid = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)                       # (B * H, Q, P, 2)
        sampled.append(F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False))
        start += h * w
    w_ = weights.transpose(1, 2).reshape(B * Hh, 1, Q, L * Pp)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * w_).sum(-1).view(B, Hh * Dd, Q)
    return out.transpose(1, 2).contiguous()


def make_inputs(levels, Q, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = len(levels)
    S = sum(h * w for h, w in levels)
    value = torch.randn((1, S, H, D), generator=g)
    ref = torch.rand((1, Q, 1, 1, 1, 2), generator=g)
    wh = torch.tensor([[w, h] for h, w in levels], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref + 2.0 * torch.randn((1, Q, H, L, P, 2), generator=g) / wh
    weights = torch.softmax(torch.randn((1, Q, H, L * P), generator=g), -1).view(1, Q, H, L, P)
    grad_out = torch.randn((1, Q, H * D), generator=g)
    shapes = torch.tensor(levels, dtype=torch.int64)
    starts = torch.cumsum(shapes[:, 0] * shapes[:, 1], 0) - shapes[:, 0] * shapes[:, 1]
    return [t.to(dev) for t in (value, shapes, starts, loc, weights, grad_out)]


def time_calls(fns, calls, warmup, dev):
    """Median / min / max milliseconds of each callable, alternating them, by device events."""
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


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["hip"], default=None, help="hip: only make --calls forward and backward calls per shape (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for frame, levels in FRAMES.items():
        S = sum(h * w for h, w in levels)
        for layer, Q in (("encoder", S), ("decoder", 900)):
            value, shapes, starts, loc, weights, grad_out = make_inputs(levels, Q, dev, seed=S + Q)
            hip_fwd = lambda: mda.ms_deform_attn_forward(value, shapes, starts, loc, weights, 64)
            hip_bwd = lambda: mda.ms_deform_attn_backward(value, shapes, starts, loc, weights, grad_out, 64)
            if a.only == "hip":
                for _ in range(a.calls):
                    hip_fwd()
                    hip_bwd()
                torch.cuda.synchronize(dev)
                continue
            v, lo, w = (t.clone().requires_grad_(True) for t in (value, loc, weights))

            def torch_fwd():
                with torch.no_grad():
                    return torch_ms_deform_attn(value, levels, loc, weights)

            def torch_fwd_bwd():
                out = torch_ms_deform_attn(v, levels, lo, w)
                return torch.autograd.grad(out, (v, lo, w), grad_out)

            def hip_fwd_bwd():
                return hip_fwd(), hip_bwd()

            base_out, base_grads = torch_fwd(), torch_fwd_bwd()
            grads = hip_bwd()
            agree = dict(out=rel_l2(hip_fwd(), base_out), grad_value=rel_l2(grads[0], base_grads[0]),
                         grad_weights=rel_l2(grads[2], base_grads[2]))
            out = time_calls({"hip_forward": hip_fwd, "torch_forward": torch_fwd, "hip_forward_backward": hip_fwd_bwd,
                              "torch_forward_backward": torch_fwd_bwd}, a.calls, a.warmup, dev)
            gathered = Q * H * len(levels) * P * 4 * D * 4
            print(json.dumps(dict(what="ms_deform_attn", frame=frame, layer=layer, S=S, Q=Q, H=H, D=D, L=len(levels), P=P,
                                  rel_l2_against_baseline={k: float(f"{x:.3e}") for k, x in agree.items()},
                                  forward_gathered_bytes=gathered,
                                  forward_gathered_TBps=round(gathered / (out["hip_forward"]["median_ms"] * 1e-3) / 1e12, 3),
                                  forward_speedup=round(out["torch_forward"]["median_ms"] / out["hip_forward"]["median_ms"], 2),
                                  forward_backward_speedup=round(out["torch_forward_backward"]["median_ms"] / out["hip_forward_backward"]["median_ms"], 2),
                                  **out)), flush=True)


if __name__ == "__main__":
    main()
