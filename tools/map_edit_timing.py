"""Times the map edits, ``GaussianModel.map_edit = "host"`` (the PyTorch statements) against ``"fused"`` (one ``lvdgs_map_edit_plan``, one wait,
one ``lvdgs_map_edit_apply``), in one process and on the same state:

* ``densify_and_prune`` on a map with Adam moments, about a tenth of the rows cloned, a tenth split, a twentieth pruned;
* ``prune_points`` with 5 % of the rows removed;
* the pruning pass of the mapping loop (``backend_map._pruning_pass``, ``slam`` mode) with 8 visibility rows on the device.

Sizes: 16 k Gaussians (where the synthetic drive lives), 200 k and 2 M, SH degree 0.  Wall time per call with a device synchronisation on
either side, the two modes alternating inside one loop after a warm-up, a fresh copy of the state for every call made outside the clock;
medians and minima of 30.  One JSON line on stdout and in ``profiles/map_edit_timing.json``.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import backend_map  # noqa: E402
from lvdgs.gaussian_model import GaussianModel  # noqa: E402

SIZES = (16_000, 200_000, 2_000_000)
OPT = dict(position_lr_init=0.0016, position_lr_final=0.00016, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
           feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001, percent_dense=0.01)
EXTENT, MAX_GRAD, MIN_OPACITY, MAX_SCREEN = 6.0, 0.0002, 0.05, 20.0
WINDOW = [11, 9, 8, 6, 5, 3, 2, 0]


def base_state(n, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    which = r(n)
    # exp(scale): a tenth of the rows large and selected (split), a tenth small and selected (cloned); a twentieth transparent
    scaling = torch.log(0.005 + 0.04 * r(n, 3))
    scaling[which < 0.1] = torch.log(0.1 + 0.3 * r(n, 3))[which < 0.1]
    accum = torch.where(which < 0.2, torch.ones(n, device=dev), torch.zeros(n, device=dev)).reshape(n, 1)
    opacity = (2.0 + r(n, 1))
    opacity[r(n) < 0.05] = -6.0
    params = dict(xyz=10 * r(n, 3), f_dc=r(n, 1, 3), f_rest=torch.empty(n, 0, 3, device=dev), opacity=opacity, scaling=scaling,
                  rotation=r(n, 4) + 0.1)
    return dict(params=params, accum=accum, denom=torch.ones(n, 1, device=dev), radii=40 * r(n), kf=torch.randint(0, 12, (n,), dtype=torch.int32),
                prune_mask=r(n) < 0.05, vis=(r(8, n) < 0.3).long())


def model(mode, st, dev):
    m = GaussianModel(0, device=str(dev))
    m.map_edit = mode
    p = lambda t: nn.Parameter(t.clone().requires_grad_(True))
    m._set_params({k: p(v) for k, v in st["params"].items()})
    m.init_lr(EXTENT)
    m.training_setup(OPT)
    for group in m.optimizer.param_groups:
        q = group["params"][0]
        m.optimizer.state[q] = dict(step=torch.tensor(3.0), exp_avg=torch.full_like(q, 1e-3), exp_avg_sq=torch.full_like(q, 1e-6))
    m.xyz_gradient_accum, m.denom, m.max_radii2D = st["accum"].clone(), st["denom"].clone(), st["radii"].clone()
    m.unique_kfIDs, m.n_obs = st["kf"].clone(), torch.zeros(st["kf"].shape[0], dtype=torch.int32)
    if mode == "fused":
        m.kf_ids_on_device()      # (the mirror travels with a fused model's edits; its first upload is not an edit's cost)
    return m


def wall_ms(fn, modes, calls, warmup, dev, before):
    ms = {k: [] for k in modes}
    for it in range(warmup + calls):
        for k in modes:
            arg = before(k)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(arg)
            torch.cuda.synchronize(dev)
            if it >= warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return ms


def stats(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), calls=len(v))


def measure(n, dev, calls, warmup):
    st = base_state(n, dev)
    modes = ("host", "fused")
    out = dict(gaussians=n)
    sizes = {}

    def densify(m):
        m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN)
        sizes["densify_and_prune"] = m.get_xyz.shape[0]

    def prune(m):
        m.prune_points(st["prune_mask"])
        sizes["prune_points"] = m.get_xyz.shape[0]

    def pass_ctx(mode):
        G = model(mode, st, dev)
        vis = st["vis"].clone()
        backend = types.SimpleNamespace(occ_aware_visibility={k: vis[i] for i, k in enumerate(WINDOW)}, initialized=True, monocular=True)
        return types.SimpleNamespace(backend=backend, G=G, sharder=None, n_window=8, window=list(WINDOW),
                                     cfg={"Training": {"window_size": 8, "prune_mode": "slam", "prune_num": 2}})

    def pruning_pass(c):
        backend_map._pruning_pass(c)
        sizes["pruning_pass"] = c.G.get_xyz.shape[0]

    for name, fn, before in (("densify_and_prune", densify, lambda mode: model(mode, st, dev)), ("prune_points", prune, lambda mode: model(mode, st, dev)),
                             ("pruning_pass", pruning_pass, pass_ctx)):
        ms = wall_ms(fn, modes, calls, warmup, dev, before)
        out[name] = {k: stats(v) for k, v in ms.items()}
        out[name]["rows_after"] = sizes[name]
        print(f"  N = {n}: {name}: host {out[name]['host']['median_ms']} ms, fused {out[name]['fused']['median_ms']} ms "
              f"(minima {out[name]['host']['min_ms']} / {out[name]['fused']['min_ms']}), {sizes[name]} rows after", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_edit_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("map_edit_timing needs a GPU")
    dev = torch.device("cuda", 0)
    out = dict(what="map_edit", device=torch.cuda.get_device_name(dev), calls=a.calls, warmup=a.warmup,
               cases=[measure(n, dev, a.calls, a.warmup) for n in a.sizes])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
