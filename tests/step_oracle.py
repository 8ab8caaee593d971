"""TEST INFRASTRUCTURE -- float64 NumPy restatements of the four small kernel families of a tracking / mapping iteration, written from
``include/lvdgs.h`` and the statements it cites (reference utils/slam_utils.py:42-121, utils/slam_backend.py:303-305, :311-315, :350-357,
``torch.optim.Adam``'s single-tensor statements), not from the kernels:

* ``photometric``      lvdgs_photometric_loss_forward / _backward / _value_and_grad
* ``isotropic``        lvdgs_isotropic_reg
* ``adam``             lvdgs_adam_step, one tensor
* ``view_stats``, ``map_stats_apply``   lvdgs_view_stats (and the statistics half of lvdgs_map_view_tail / _batch), lvdgs_map_stats_apply

Inputs are the float32 / integer arrays the device sees; every operation on them is float64, so what is returned carries none of float32's
roundings.  The only float32 values are the ones the header itself states in float32: the three thresholds of the loss (the comparison
is made between the float32 input and the float32 constant -- exact on every side) and Adam's scalars (doubles, rounded to float32 where
they meet a tensor).  Next to each result the oracles return the magnitudes the tests' a-priori error bounds are made of.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
DEPTH_MIN, OPAQUE_MIN = f32(0.01), f32(0.95)      # k_p = (Z_p > 0.01) [* (opacity_p > 0.95)], float32 constants


def _d(a):
    return None if a is None else np.asarray(a).astype(f64)


def sign(x):
    """sign(0) = 0."""
    return (x > 0).astype(f64) - (x < 0).astype(f64)


def photometric(image, gt_image, depth=None, gt_depth=None, opacity=None, grad_mask=None, exposure_a=None, exposure_b=None, grad_loss=None,
                rgb_thr=0.01, weight_rgb=1.0, weight_depth=0.0, weight_by_opacity=0, depth_needs_opaque=0):
    """``image``, ``gt_image``: (3, P) float32; ``depth``, ``gt_depth``, ``opacity``: (P,) float32 or None; ``grad_mask``: (P,) bytes or None;
    ``exposure_a`` / ``_b`` / ``grad_loss``: a float32 scalar or None (identity / 1).

        loss = weight_rgb * mean_{c,p} [omega_p |(e^a I_cp + b) m_p - G_cp m_p|] + weight_depth * mean_p [|D_p k_p - Z_p k_p|]

    Returns a dict: value, d_image (3, P), d_depth, d_opacity (P,), d_a, d_b -- the gradients of grad_loss * loss -- and, for the error
    bounds, ``operands`` (3, P) = m (|e^a I| + |b| + |G|), ``omega`` (P,), ``abs_rd`` (P,) = |D k - Z k|, ``Wr`` = grad_loss weight_rgb / (3 P),
    ``abs_a`` / ``abs_b`` = the sums of the absolute values of d_a's / d_b's terms."""
    I, G = _d(image), _d(gt_image)
    P = I.shape[1]
    assert I.shape == G.shape == (3, P)
    if (weight_by_opacity or depth_needs_opaque) and opacity is None:
        raise ValueError("the flags need the opacity image")
    w_rgb = float(f32(weight_rgb))
    w_d = float(f32(weight_depth)) if (depth is not None and gt_depth is not None) else 0.0
    ea = math.exp(float(exposure_a)) if exposure_a is not None else 1.0
    eb = float(exposure_b) if exposure_b is not None else 0.0
    g = float(grad_loss) if grad_loss is not None else 1.0
    m = (G.sum(0) > float(f32(rgb_thr))).astype(f64)
    if grad_mask is not None:
        m = m * (np.asarray(grad_mask) != 0)
    om = _d(opacity) if weight_by_opacity else np.ones(P)
    r = (ea * I + eb) * m - G * m
    out = {}
    rd = kd = np.zeros(P)
    if depth is not None and gt_depth is not None:
        kd = (np.asarray(gt_depth, f32) > DEPTH_MIN).astype(f64)
        if depth_needs_opaque:
            kd = kd * (np.asarray(opacity, f32) > OPAQUE_MIN)
        rd = _d(depth) * kd - _d(gt_depth) * kd
    out["value"] = w_rgb * (om * np.abs(r)).sum() / (3.0 * P) + w_d * np.abs(rd).sum() / P
    Wr, Wd = g * w_rgb / (3.0 * P), g * w_d / P
    q = Wr * om * sign(r) * m                      # d objective / d (e^a I + b), per channel and pixel
    out["d_image"] = ea * q
    out["d_opacity"] = Wr * np.abs(r).sum(0) if weight_by_opacity else np.zeros(P)
    out["d_depth"] = Wd * sign(rd) * kd
    out["d_a"] = float((q * ea * I).sum())
    out["d_b"] = float(q.sum())
    out.update(operands=m * (np.abs(ea * I) + abs(eb) + np.abs(G)), omega=om, abs_rd=np.abs(rd), Wr=Wr, w_rgb=w_rgb, w_d=w_d, P=P,
               abs_a=float(np.abs(q * ea * I).sum()), abs_b=float(np.abs(q).sum()))
    return out


def isotropic(raw, weight, grad_in=None):
    """loss = weight * mean_{i,k} |s_ik - mean_k s_ik|, s = exp(raw); ``raw`` (N, 3) float32.  Returns (value, grad_in + d loss / d raw or
    None, extras).  A row whose three raw scales are bit-equal has s_ik = mean exactly: it adds nothing to either."""
    raw = np.asarray(raw, f32).reshape(-1, 3)
    N = raw.shape[0]
    extras = dict(sum_s=0.0, scale=0.0, s=np.zeros((0, 3)))
    if N == 0:
        return 0.0, (None if grad_in is None else _d(grad_in).reshape(0, 3)), extras
    s = np.exp(raw.astype(f64))
    d = s - s.mean(1, keepdims=True)
    equal = (raw[:, 0] == raw[:, 1]) & (raw[:, 1] == raw[:, 2])
    d[equal] = 0.0
    scale = float(f32(weight)) / (3.0 * N)
    value = scale * np.abs(d).sum()
    sg = sign(d)
    grad = scale * (sg - sg.mean(1, keepdims=True)) * s
    extras = dict(sum_s=float(s.sum()), scale=scale, s=s, equal=equal)
    return value, (None if grad_in is None else _d(grad_in).reshape(-1, 3) + grad), extras


def adam_scalars(step, lr, beta1, beta2, eps, round_scalars=True):
    """The six scalars of a step as the header gives them: doubles, rounded to float32 where they meet a tensor."""
    rnd = (lambda x: float(f32(x))) if round_scalars else float
    return dict(w1=rnd(1.0 - beta1), b2=rnd(beta2), w2=rnd(1.0 - beta2), eps=rnd(eps),
                step_size=rnd(lr / (1.0 - beta1 ** float(step))), bc2_sqrt=rnd(math.sqrt(1.0 - beta2 ** float(step))))


def adam(param, grad, m, v, step, lr, beta1, beta2, eps, round_scalars=True):
    """torch.optim.Adam (no weight decay, no amsgrad), ``step`` including this one:
        exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        denom = (exp_avg_sq.sqrt() / sqrt(1 - beta2^t)).add_(eps); param.addcdiv_(exp_avg, denom, value=-lr / (1 - beta1^t))
    Returns (param', exp_avg', exp_avg_sq', extras) in float64."""
    k = adam_scalars(step, lr, beta1, beta2, eps, round_scalars)
    p, g, m, v = _d(param), _d(grad), _d(m), _d(v)
    m1 = m + k["w1"] * (g - m)
    v1 = v * k["b2"] + k["w2"] * (g * g)
    denom = np.sqrt(v1) / k["bc2_sqrt"] + k["eps"]
    u = k["step_size"] * (m1 / denom)
    extras = dict(k, update=u, denom=denom, m_terms=np.abs(m) + np.abs(k["w1"] * g) + np.abs(k["w1"] * m))
    return p - u, m1, v1, extras


def view_stats(radii, n_touched, viewspace_grad, state, use_split=False):
    """One view into the accumulators.  ``state``: dict with radii_max (int), norm_sum, vis_count (float64 or None), norm_err (the
    accumulated a-priori bound of norm_sum in units of eps).  Returns the new state plus this view's ``touched_row`` (or None without
    n_touched) and ``split_xy`` (N, 2) when ``use_split`` -- the band's xy instead of its norm.
        radii_max = max(radii_max, radii); visible (radii > 0): norm_sum += |grad xy|, vis_count += 1; touched_row = n_touched > 0"""
    radii = np.asarray(radii, np.int64)
    vis = radii > 0
    new = dict(state)
    new["radii_max"] = np.maximum(np.asarray(state["radii_max"], np.int64), radii)
    xy = np.zeros((radii.size, 2))
    if viewspace_grad is not None:
        xy = np.where(vis[:, None], _d(viewspace_grad).reshape(-1, 3)[:, :2], 0.0)       # the third column is never read
    split = None
    if use_split:
        split = xy
    elif state.get("norm_sum") is not None:
        t = np.sqrt(xy[:, 0] ** 2 + xy[:, 1] ** 2)
        new["norm_sum"] = state["norm_sum"] + t
        new["norm_err"] = state.get("norm_err", np.zeros(radii.size)) + np.where(t > 0, 3.0 * t + np.abs(new["norm_sum"]), 0.0)
    if state.get("vis_count") is not None:
        new["vis_count"] = state["vis_count"] + vis
    touched = None if n_touched is None else (np.asarray(n_touched) > 0).astype(np.uint8)
    return new, touched, split


def map_stats_apply(radii_max, norm_sum, vis_count, split_planes, max_radii2D, grad_accum, denom):
    """max_radii2D = max(max_radii2D, radii_max); xyz_gradient_accum += norm_sum + sum_k |split_xy[k]|; denom += vis_count.
    ``split_planes``: (n_split, N, 2).  Returns (max_radii2D, grad_accum, denom, err) with err the a-priori bound of grad_accum in eps."""
    mr = np.maximum(_d(max_radii2D), _d(radii_max))
    g = _d(norm_sum).copy()
    err = np.zeros_like(g)
    planes = np.asarray(split_planes, f64)
    for plane in planes.reshape(planes.shape[0] if planes.ndim == 3 else 0, g.size, 2):
        t = np.sqrt(plane[:, 0] ** 2 + plane[:, 1] ** 2)
        g = g + t
        err += 3.0 * t + np.abs(g)
    acc = _d(grad_accum) + g
    return mr, acc, _d(denom) + _d(vis_count), err + np.abs(acc)


# ------------------------------------------------------------------------------------------------ a-priori bounds of a float32 evaluation
# eps = 2^-24: half an ulp, relative -- one rounding of +, -, *, /, sqrt.  expf: 2 eps (one ulp, what the device library documents and what
# PyTorch's CPU exp keeps).  First order throughout.  The derivations are in tests/test_gpu_step_kernels.py's docstring.
EPS = 2.0 ** -24


def summed_allowance(n_terms, roundings, sum_abs):
    """(ceil(log2 n) + 8 + r) eps sum|t|: pairwise summation of n terms that carry r roundings each, plus eight for short serial runs."""
    return (math.ceil(math.log2(max(int(n_terms), 1))) + 8 + roundings) * EPS * sum_abs


def photometric_bounds(o):
    """Bounds for every output of a float32 evaluation, from the oracle's dict ``o``."""
    P = o["P"]
    A = o["operands"]
    return dict(
        value=o["w_rgb"] / (3.0 * P) * summed_allowance(3 * P, 12, float((o["omega"] * A).sum())) + o["w_d"] / P * summed_allowance(P, 5, float(o["abs_rd"].sum())),
        d_a=summed_allowance(3 * P, 10, o["abs_a"]), d_b=summed_allowance(3 * P, 6, o["abs_b"]),
        d_image=8 * EPS * np.abs(o["d_image"]), d_depth=8 * EPS * np.abs(o["d_depth"]),
        d_opacity=8 * EPS * np.abs(o["d_opacity"]) + 5 * EPS * abs(o["Wr"]) * A.sum(0) * (o["d_opacity"] != 0))


def isotropic_bounds(extras, n, grad_in):
    value = extras["scale"] * summed_allowance(3 * n, 14, extras["sum_s"])
    grad = None if grad_in is None else EPS * (np.abs(_d(grad_in).reshape(-1, 3)) + 12.0 * extras["scale"] * extras["s"])
    return value, grad


def adam_bounds(p1, m1, v1, extras):
    """-> bounds of (param', exp_avg', exp_avg_sq')."""
    bm = 3 * EPS * extras["m_terms"]
    bv = 4 * EPS * v1
    bp = EPS * np.abs(p1) + 8 * EPS * np.abs(extras["update"]) + np.abs(extras["step_size"] / extras["denom"]) * bm
    return bp, bm, bv


# ------------------------------------------------------------------------------------------------ the statements in PyTorch, in any dtype
# What the reference runs (utils/slam_utils.py:42-121, utils/slam_backend.py:303-305, :350-357 with GaussianModel.add_densification_stats,
# torch.optim.Adam), on the CPU: in float64 + autograd they pin the oracles, in float32 they are the check of the bounds above.
def torch_photometric(dtype, image, gt_image, depth=None, gt_depth=None, opacity=None, grad_mask=None, exposure_a=None, exposure_b=None, grad_loss=None,
                      rgb_thr=0.01, weight_rgb=1.0, weight_depth=0.0, weight_by_opacity=0, depth_needs_opaque=0):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    leaf = lambda a: t(a).requires_grad_(True)
    img, gt = leaf(image), t(gt_image)
    a, b = leaf(np.array([0.0 if exposure_a is None else exposure_a], f32)), leaf(np.array([0.0 if exposure_b is None else exposure_b], f32))
    dep = leaf(depth) if depth is not None else None
    opa = leaf(opacity) if opacity is not None else None
    image_ab = torch.exp(a) * img + b
    mask = torch.from_numpy(np.ascontiguousarray(gt_image)).sum(dim=0) > torch.tensor(rgb_thr, dtype=torch.float32)     # decided on the float32 inputs
    if grad_mask is not None:
        mask = mask * torch.from_numpy(np.asarray(grad_mask) != 0)
    l1 = torch.abs(image_ab * mask - gt * mask)
    if weight_by_opacity:
        l1 = opa * l1
    loss = float(f32(weight_rgb)) * l1.mean()
    if dep is not None and gt_depth is not None:
        gtd32 = torch.from_numpy(np.ascontiguousarray(gt_depth))
        dm = gtd32 > torch.tensor(0.01, dtype=torch.float32)
        if depth_needs_opaque:
            dm = dm * (torch.from_numpy(np.ascontiguousarray(opacity)) > torch.tensor(0.95, dtype=torch.float32))
        loss = loss + float(f32(weight_depth)) * torch.abs(dep * dm - gtd32.to(dtype) * dm).mean()
    loss.backward(torch.tensor(1.0 if grad_loss is None else float(grad_loss), dtype=dtype))
    z = lambda x, like: (np.zeros(like.shape) if x is None or x.grad is None else x.grad.numpy().astype(f64))
    return dict(value=float(loss.detach()), d_image=z(img, image), d_depth=z(dep, image[0]), d_opacity=z(opa, image[0]),
                d_a=float(a.grad), d_b=float(b.grad))


def torch_isotropic(dtype, raw, weight, grad_in=None):
    import torch
    r = torch.from_numpy(np.ascontiguousarray(raw)).to(dtype).reshape(-1, 3).requires_grad_(True)
    if r.shape[0] == 0:
        return 0.0, None if grad_in is None else np.zeros((0, 3))
    if grad_in is not None:
        r.grad = torch.from_numpy(np.ascontiguousarray(grad_in)).to(dtype).reshape(-1, 3).clone()
    scaling = torch.exp(r)
    loss = weight * torch.abs(scaling - scaling.mean(dim=1).view(-1, 1)).mean()
    loss.backward()
    return float(loss.detach()), (None if grad_in is None else r.grad.numpy().astype(f64))


def torch_adam(dtype, param, grad, m, v, step, lr, beta1, beta2, eps):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    p = torch.nn.Parameter(t(param))
    p.grad = t(grad)
    opt = torch.optim.Adam([p], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=t(m), exp_avg_sq=t(v))
    opt.step()
    st = opt.state[p]
    return p.detach().numpy().astype(f64), st["exp_avg"].numpy().astype(f64), st["exp_avg_sq"].numpy().astype(f64)


def torch_norm_sum(dtype, norm_sum0, views):
    """GaussianModel.add_densification_stats over the views: xyz_gradient_accum[vis] += norm(grad[vis, :2], dim=-1)."""
    import torch
    acc = torch.from_numpy(np.ascontiguousarray(norm_sum0)).to(dtype).clone()
    for v in views:
        vis = torch.from_numpy(v["radii"] > 0)
        g = torch.from_numpy(v["grad"]).to(dtype)
        acc[vis] += torch.norm(g[vis, :2], dim=-1)
    return acc.numpy().astype(f64)
