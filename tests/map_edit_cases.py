"""Inputs for the map-edit tests: small maps whose densification decisions cannot depend on the last bit of an exponential.

``make_case(kind, n, S, sh_degree)`` -> a dict of float32 / int arrays (the six parameters, two Adam moments each, the three statistics,
kf ids, n_obs) and the thresholds of one ``densify_and_prune`` call.  Asserted in float64 on the way out (``assert_gaps``): no activated
value -- ``exp(s)``, ``exp(s) / 1.6``, ``sigmoid(o)`` -- lies within 2^-20 relative of the threshold it is compared with.  That is a
condition on the inputs, so ``expf`` on the device, NumPy's and PyTorch's exponentials all decide alike.  The gradient comparison
``accum / denom >= thr`` is exact IEEE arithmetic on every side, so ties (``g == thr`` to the bit), ``0 / 0`` and ``x / 0`` rows ARE here.

``build_model(case, device, map_edit)`` -> a ``GaussianModel`` in that state, Adam moments included.
"""
import numpy as np

SIZES = (0, 1, 63, 64, 65, 1023, 1025, 70_001)
# above 1024 x 256 rows, the most spans of a plan times a tile: a span is two tiles long and the write pass carries its rows across them
# (for kind "mixed" only -- the span scan is blind to what the rows are steered to)
LONG_SPANS = 262_401
# kind -> what the rows are steered to
KINDS = ("mixed", "mixed_no_screen", "none", "all_clone", "all_split", "all_pruned", "children_pruned")
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY, MAX_SCREEN = 6.0, 0.01, 0.0002, 0.05, 20.0
GAP = 2.0 ** -20
f32 = np.float32


def thresholds(case):
    """The float32 thresholds the activated values meet, as float64: (dense_extent, world_extent, min_opacity)."""
    return (float(f32(case["percent_dense"] * case["extent"])), float(f32(0.1 * case["extent"])), float(f32(case["min_opacity"])))


def gap_violations(scaling, opacity, case):
    """Boolean arrays (per scale entry, per opacity) of values within GAP relative of a threshold, in float64."""
    dense, world, min_op = thresholds(case)
    e = np.exp(scaling.astype(np.float64))
    near = lambda v, t: np.abs(v - t) <= GAP * t
    sig = 1.0 / (1.0 + np.exp(-opacity.astype(np.float64)))
    return near(e, dense) | near(e, world) | near(e / 1.6, world) | near(e / 1.6, dense), near(sig, min_op)


def assert_gaps(scaling, opacity, case):
    bad_s, bad_o = gap_violations(scaling, opacity, case)
    assert not bad_s.any() and not bad_o.any(), "an activated value lies within 2^-20 relative of its threshold"


def make_case(kind, n, S=3, sh_degree=0, seed=0):
    rng = np.random.default_rng([seed, n, S, KINDS.index(kind)])
    case = dict(kind=kind, n=n, S=S, sh_degree=sh_degree, extent=EXTENT, percent_dense=PERCENT_DENSE, max_grad=MAX_GRAD,
                min_opacity=MIN_OPACITY, max_screen_size=0.0 if kind == "mixed_no_screen" else MAX_SCREEN)
    dense, world, _ = thresholds(case)
    thr = f32(MAX_GRAD)
    # gradients: a sixth of the rows each -- far below, far above, exactly the threshold (denominators 1, 2, 4: exact quotients), 0 / 0,
    # x / 0, and one ulp below the threshold
    denom = rng.integers(1, 6, n).astype(f32)
    g = np.exp(rng.uniform(np.log(1e-5), np.log(1e-2), n)).astype(f32)
    accum = (g * denom).astype(f32)
    which = rng.integers(0, 6, n)
    tie = which == 2
    denom[tie] = f32(2.0) ** rng.integers(0, 3, int(tie.sum()))
    accum[tie] = thr * denom[tie]
    below = which == 5
    denom[below] = 1.0
    accum[below] = np.nextafter(thr, f32(0))
    accum[which == 3], denom[which == 3] = 0.0, 0.0
    denom[which == 4] = 0.0
    # activated scales log-uniform over [0.005, 2]: both sides of dense_extent (0.06), of world_extent (0.6) and of 1.6 world_extent
    scaling = rng.uniform(np.log(0.005), np.log(2.0), (n, S)).astype(f32)
    opacity = rng.normal(0.0, 3.0, (n, 1)).astype(f32)
    if kind == "none":
        accum[:] = 0.0
    elif kind == "all_clone":          # every gradient over the threshold, every scale small
        accum, denom = np.full(n, 1.0, f32), np.ones(n, f32)
        scaling = rng.uniform(np.log(0.005), np.log(0.05), (n, S)).astype(f32)
    elif kind == "all_split":          # ... every scale large, children below world_extent
        accum, denom = np.full(n, 1.0, f32), np.ones(n, f32)
        scaling = rng.uniform(np.log(0.1), np.log(0.5), (n, S)).astype(f32)
    elif kind == "all_pruned":         # every opacity below the bar: originals, clones and children all go
        opacity = rng.uniform(-9.0, -4.0, (n, 1)).astype(f32)
    elif kind == "children_pruned":    # split sources so large that exp(s) / 1.6 is still over world_extent: their children go, by that term alone
        accum, denom = np.full(n, 1.0, f32), np.ones(n, f32)
        scaling = rng.uniform(np.log(1.7 * world), np.log(3.0 * world), (n, S)).astype(f32)
        opacity = rng.uniform(1.0, 4.0, (n, 1)).astype(f32)
    for _ in range(8):                 # move what sits on a threshold off it
        bad_s, bad_o = gap_violations(scaling, opacity, case)
        if not bad_s.any() and not bad_o.any():
            break
        scaling[bad_s] += f32(0.001)
        opacity[bad_o] += f32(0.001)
    assert_gaps(scaling, opacity, case)
    rest = (sh_degree + 1) ** 2 - 1
    q = rng.normal(0.0, 1.0, (n, 4)).astype(f32)
    q[:, 0] += f32(2.0) * np.sign(q[:, 0] + f32(1e-3))       # unnormalised, away from zero norm
    case.update(
        grad_accum=accum.reshape(n, 1), denom=denom.reshape(n, 1), max_radii2D=rng.uniform(0.0, 40.0, n).astype(f32),
        xyz=rng.normal(0.0, 5.0, (n, 3)).astype(f32), f_dc=rng.normal(0.0, 1.0, (n, 1, 3)).astype(f32),
        f_rest=rng.normal(0.0, 1.0, (n, rest, 3)).astype(f32), opacity=opacity, scaling=scaling, rotation=q,
        kf_ids=rng.integers(0, 12, n).astype(np.int32), n_obs=rng.integers(0, 9, n).astype(np.int32))
    case["f_dc"][:, 0, 0] = np.arange(n, dtype=f32)         # a row's identity travels with it (exact below 2^24)
    for name in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"):
        shape = case[name].shape
        case["exp_avg_" + name] = (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(f32) * f32(1e-3)   # never zero
        case["exp_avg_sq_" + name] = rng.uniform(0.5, 1.5, shape).astype(f32) * f32(1e-6)
    return case


OPT = dict(percent_dense=PERCENT_DENSE, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
           position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001)
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def build_model(case, device, map_edit="host", moments=True):
    """A GaussianModel holding the case: parameters, statistics, kf ids, n_obs, an optimiser with the case's Adam moments."""
    import torch
    from torch import nn
    from lvdgs.gaussian_model import GaussianModel
    m = GaussianModel(case["sh_degree"], device=device)
    m.map_edit = map_edit
    m.isotropic = case["S"] == 1
    p = lambda a: nn.Parameter(torch.from_numpy(a.copy()).to(device).requires_grad_(True))
    m._xyz, m._features_dc, m._features_rest = p(case["xyz"]), p(case["f_dc"]), p(case["f_rest"])
    m._opacity, m._scaling, m._rotation = p(case["opacity"]), p(case["scaling"]), p(case["rotation"])
    m.init_lr(EXTENT)
    m.training_setup(OPT)
    m.xyz_gradient_accum = torch.from_numpy(case["grad_accum"].copy()).to(device)
    m.denom = torch.from_numpy(case["denom"].copy()).to(device)
    m.max_radii2D = torch.from_numpy(case["max_radii2D"].copy()).to(device)
    m.unique_kfIDs = torch.from_numpy(case["kf_ids"].copy())
    m.n_obs = torch.from_numpy(case["n_obs"].copy())
    if moments:
        for group in m.optimizer.param_groups:
            name = group["name"]
            m.optimizer.state[group["params"][0]] = dict(step=torch.tensor(3.0), exp_avg=torch.from_numpy(case["exp_avg_" + name].copy()).to(device),
                                                         exp_avg_sq=torch.from_numpy(case["exp_avg_sq_" + name].copy()).to(device))
    return m


def model_tensors(m):
    """Every per-Gaussian tensor of a model, by name, on the CPU."""
    out = {}
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        out[group["name"]] = p.detach().cpu()
        st = m.optimizer.state.get(p)
        if st:
            out["exp_avg_" + group["name"]] = st["exp_avg"].cpu()
            out["exp_avg_sq_" + group["name"]] = st["exp_avg_sq"].cpu()
    out.update(grad_accum=m.xyz_gradient_accum.cpu(), denom=m.denom.cpu(), max_radii2D=m.max_radii2D.cpu(), kf_ids=m.unique_kfIDs, n_obs=m.n_obs)
    return out
