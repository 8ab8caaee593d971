"""Regenerates tests/golden/ms_deform_attn.npz from GroundingDINO's own PyTorch formulation of the operator.

    python tests/golden/make_ms_deform_attn_golden.py /path/to/GroundingDINO-main

Loads ``groundingdino/models/GroundingDINO/ms_deform_attn.py`` of that checkout by file path (it imports with torch alone; its
guarded import of ``_C`` fails with a warning) and runs ``multi_scale_deformable_attn_pytorch`` on the CPU over the cases of
tests/ms_deform_attn_cases.py.  Stored, as data only:

* for the small cases (``cases.SMALL``): the float64 outputs on both location sets, and the float64 autograd gradients of
  ``sum(out * grad_out)`` on the generic set -- ``<case>/out_snapped``, ``<case>/out_generic``, ``<case>/grad_value``,
  ``<case>/grad_loc``, ``<case>/grad_weights``;
* for every case, ``<case>/f32_error`` (5, 2): the function's own float32 error -- relative L2 and max-abs of its float32 run
  against its float64 run at the same float32-rounded inputs -- for, in this order, ``ERROR_ROWS``.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ms_deform_attn_cases as cases  # noqa: E402

ERROR_ROWS = ("out_snapped", "out_generic", "grad_value", "grad_loc", "grad_weights")


def load_reference(checkout):
    path = os.path.join(checkout, "groundingdino", "models", "GroundingDINO", "ms_deform_attn.py")
    spec = importlib.util.spec_from_file_location("reference_ms_deform_attn", path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod.multi_scale_deformable_attn_pytorch


def run(fn, c, loc, dtype, grads):
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype).requires_grad_(grads)
    v, lo, w = t(c.value), t(loc), t(c.weights)
    out = fn(v, [tuple(int(n) for n in hw) for hw in c.shapes], lo, w)
    if not grads:
        return (out.detach().double().numpy(),)
    (out * torch.from_numpy(np.array(c.grad_out)).to(dtype)).sum().backward()
    return tuple(a.detach().double().numpy() for a in (out, v.grad, lo.grad, w.grad))


def error(a32, a64):
    d, n = a32 - a64, np.linalg.norm(a64)
    return [float(np.linalg.norm(d) / n) if n > 0 else float(np.linalg.norm(d)), float(np.abs(d).max())]


def main():
    fn = load_reference(sys.argv[1])
    data = {}
    for name in cases.CASES:
        c = cases.case(name)
        snapped64, = run(fn, c, c.loc_snapped, torch.float64, False)
        snapped32, = run(fn, c, c.loc_snapped, torch.float32, False)
        generic64 = run(fn, c, c.loc_generic, torch.float64, True)
        generic32 = run(fn, c, c.loc_generic, torch.float32, True)
        data[f"{name}/f32_error"] = np.array([error(snapped32, snapped64)] + [error(a, b) for a, b in zip(generic32, generic64)], np.float64)
        print(name, dict(zip(ERROR_ROWS, data[f"{name}/f32_error"].tolist())))
        if name in cases.SMALL:
            data[f"{name}/out_snapped"] = snapped64
            for key, a in zip(("out_generic", "grad_value", "grad_loc", "grad_weights"), generic64):
                data[f"{name}/{key}"] = a
    out = os.path.join(HERE, "ms_deform_attn.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
