"""Float64 oracle of multi-scale deformable attention, written from the rule and not from any implementation's text:

    level l of size (h, w):  x = loc_x * w - 0.5,  y = loc_y * h - 0.5
    a sample takes part only if  y > -1 and x > -1 and y < h and x < w
    each of its four corners (floor(y) + {0, 1}, floor(x) + {0, 1}) takes part only if it lies inside the level
    out[b, q, h, :] = sum_{l, p} weight * sum_corners bilinear * value[b, start_l + yy * w + xx, h, :]

PyTorch float64 on the CPU; the gradients are autograd's through this statement (the cell of a sample is a constant of the
differentiation, as it is for every location that is not on a cell boundary).  Inputs are NumPy arrays; float32 inputs are taken
at their exact values.
"""
import numpy as np
import torch


def _forward(value, levels, loc, weights):
    B, S, H, D = value.shape
    _, Q, _, L, P, _ = loc.shape
    table = value.permute(0, 2, 1, 3)                                    # (B, H, S, D)
    out = torch.zeros((B, Q, H, D), dtype=torch.float64)
    start = 0
    for l, (h, w) in enumerate(levels):
        x = loc[:, :, :, l, :, 0] * w - 0.5                              # (B, Q, H, P)
        y = loc[:, :, :, l, :, 1] * h - 0.5
        valid = (y > -1) & (x > -1) & (y < h) & (x < w)                  # False for NaN
        x = torch.where(valid, x, torch.zeros_like(x))
        y = torch.where(valid, y, torch.zeros_like(y))
        x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
        lx, ly = x - x0, y - y0
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = (y0 + dy).long(), (x0 + dx).long()
                inside = valid & (yy >= 0) & (xx >= 0) & (yy < h) & (xx < w)
                idx = torch.where(inside, start + yy * w + xx, torch.zeros_like(yy))
                rows = idx.permute(0, 2, 1, 3).reshape(B, H, Q * P, 1).expand(-1, -1, -1, D)
                corner = torch.gather(table, 2, rows).reshape(B, H, Q, P, D).permute(0, 2, 1, 3, 4)   # (B, Q, H, P, D)
                bilinear = (ly if dy else 1.0 - ly) * (lx if dx else 1.0 - lx) * inside
                out = out + ((weights[:, :, :, l, :] * bilinear)[..., None] * corner).sum(3)
        start += h * w
    return out.reshape(B, Q, H * D)


def _levels(shapes):
    return [(int(h), int(w)) for h, w in np.asarray(shapes).reshape(-1, 2)]


def forward(value, shapes, loc, weights):
    """-> out (B, Q, H * D) float64."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    with torch.no_grad():
        return _forward(t(value), _levels(shapes), t(loc), t(weights)).numpy()


def forward_backward(value, shapes, loc, weights, grad_out):
    """-> out, grad_value, grad_loc, grad_weights of sum(out * grad_out), float64."""
    t = lambda a: torch.from_numpy(np.array(a, np.float64)).requires_grad_(True)
    v, lo, w = t(value), t(loc), t(weights)
    out = _forward(v, _levels(shapes), lo, w)
    (out * torch.from_numpy(np.asarray(grad_out, np.float64)).reshape(out.shape)).sum().backward()
    return out.detach().numpy(), v.grad.numpy(), lo.grad.numpy(), w.grad.numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))


def max_abs(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max()) if a.size else 0.0
