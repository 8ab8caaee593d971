"""The HIP multi-scale deformable attention (``lvdgs.ms_deform_attn`` -> ``lvdgs_ms_deform_attn_forward`` / ``_backward``) against the
float64 oracle (tests/ms_deform_attn_oracle.py) on the seeded cases (tests/ms_deform_attn_cases.py).

Tolerances.  Per case and tensor, relative L2 <= 4 x max(e, 2^-23), where e is the relative L2 the reference's own PyTorch function
makes in float32 against its float64 run on the same inputs (tests/golden/ms_deform_attn.npz, ``<case>/f32_error``); max-abs
<= 4 x max(that function's recorded max-abs error, 2^-23 x the largest oracle element).  The factor 4 allows one more rounding of
x / y than the reference takes and another summation order over the 64 corner terms.  No element is excluded anywhere.
"""
import functools
import os

import numpy as np
import pytest
import torch

import ms_deform_attn_cases as cases
import ms_deform_attn_oracle as orc
import parity_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERROR_ROWS = ("out_snapped", "out_generic", "grad_value", "grad_loc", "grad_weights")
EPS = 2.0 ** -23


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype, device=torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ms_deform_attn.npz"))


@functools.lru_cache(maxsize=None)
def oracle_forward(name, which):
    c = cases.case(name)
    out = orc.forward(c.value, c.shapes, cases.locations(c, which), c.weights)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_backward(name):
    c = cases.case(name)
    res = orc.forward_backward(c.value, c.shapes, c.loc_generic, c.weights, c.grad_out)
    for a in res:
        a.setflags(write=False)
    return res


def check(name, row, got, ref, what):
    """The tolerance rule of the module docstring; prints each figure before it asserts."""
    e_l2, e_abs = golden()[f"{name}/f32_error"][ERROR_ROWS.index(row)]
    got = got.detach().cpu().numpy().reshape(ref.shape)
    parity_stats.record(what, got, ref)
    l2, ma = orc.rel_l2(got, ref), orc.max_abs(got, ref)
    tol_l2, tol_abs = 4.0 * max(e_l2, EPS), 4.0 * max(e_abs, EPS * float(np.abs(ref).max()))
    print(f"{name} {what}: rel_l2 {l2:.3e} (bound {tol_l2:.3e}, reference's own {e_l2:.3e})  max_abs {ma:.3e} (bound {tol_abs:.3e}, reference's own {e_abs:.3e})")
    assert np.isfinite(got).all(), what
    assert l2 <= tol_l2, (name, what, l2, tol_l2)
    assert ma <= tol_abs, (name, what, ma, tol_abs)


def inputs(name, which):
    c = cases.case(name)
    return c, dev(c.value), dev(c.shapes), dev(c.starts), dev(cases.locations(c, which)), dev(c.weights)


@pytest.mark.parametrize("which", cases.LOCATION_SETS)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_forward_matches_the_oracle(name, which):
    from lvdgs import ms_deform_attn as mda
    c, v, shapes, starts, loc, w = inputs(name, which)
    out = mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    assert tuple(out.shape) == (c.B, c.Q, c.H * c.D) and out.dtype is torch.float32 and out.is_contiguous()
    check(name, "out_" + which, out, oracle_forward(name, which), "out " + which)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_backward_matches_the_oracle_through_autograd(name):
    from lvdgs import ms_deform_attn as mda
    c, v, shapes, starts, loc, w = inputs(name, "generic")
    for t in (v, loc, w):
        t.requires_grad_(True)
    out = mda.MultiScaleDeformableAttnFunction.apply(v, shapes, starts, loc, w, 64)
    out.backward(dev(c.grad_out))
    ref_out, ref_v, ref_loc, ref_w = oracle_backward(name)
    check(name, "out_generic", out, ref_out, "out generic (autograd)")
    check(name, "grad_value", v.grad, ref_v, "grad value")
    check(name, "grad_loc", loc.grad, ref_loc, "grad locations")
    check(name, "grad_weights", w.grad, ref_w, "grad weights")
    assert shapes.grad is None and starts.grad is None


def test_backward_called_directly():
    from lvdgs import ms_deform_attn as mda
    name = "odd"
    c, v, shapes, starts, loc, w = inputs(name, "generic")
    gv, gl, gw = mda.ms_deform_attn_backward(v, shapes, starts, loc, w, dev(c.grad_out), 64)
    assert tuple(gv.shape) == c.value.shape and tuple(gl.shape) == c.loc_generic.shape and tuple(gw.shape) == c.weights.shape
    _, ref_v, ref_loc, ref_w = oracle_backward(name)
    check(name, "grad_value", gv, ref_v, "grad value")
    check(name, "grad_loc", gl, ref_loc, "grad locations")
    check(name, "grad_weights", gw, ref_w, "grad weights")


def bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["odd", "dino_rows"])
def test_two_calls_give_the_same_bits(name):
    """Forward, location and weight gradients: bit for bit.  grad_value is summed by float atomics: within the tolerance only."""
    from lvdgs import ms_deform_attn as mda
    c, v, shapes, starts, loc, w = inputs(name, "generic")
    g = dev(c.grad_out)
    a = mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    ga = mda.ms_deform_attn_backward(v, shapes, starts, loc, w, g, 64)
    b = mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    gb = mda.ms_deform_attn_backward(v, shapes, starts, loc, w, g, 64)
    assert bits(a) == bits(b) and bits(ga[1]) == bits(gb[1]) and bits(ga[2]) == bits(gb[2])
    ref_v = oracle_backward(name)[1]
    check(name, "grad_value", ga[0], ref_v, "grad value, first call")
    check(name, "grad_value", gb[0], ref_v, "grad value, second call")


def test_non_finite_and_far_locations_take_no_part():
    """A tenth of dino_small's samples get NaN, +inf, -inf, 1e30 or -1e30 in x, in y or in both.  The output is, bit for bit, that of
    the run with those samples' weights zero and their locations 0.5; their own location and weight gradients are exactly zero; every
    other location and weight gradient has the bits of the zero-weight run, and grad_value (float atomics) agrees within the
    case's tolerance."""
    from lvdgs import ms_deform_attn as mda
    name = "dino_small"
    c = cases.case(name)
    rng = np.random.default_rng(7)
    hit = rng.random(c.weights.shape) < 0.1
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)[rng.integers(0, 5, c.weights.shape)]
    where = rng.integers(0, 3, c.weights.shape)                     # 0: x, 1: y, 2: both
    loc_bad, loc_clean, w_clean = c.loc_generic.copy(), c.loc_generic.copy(), c.weights.copy()
    loc_bad[..., 0] = np.where(hit & (where != 1), bad, loc_bad[..., 0])
    loc_bad[..., 1] = np.where(hit & (where != 0), bad, loc_bad[..., 1])
    loc_clean[hit] = 0.5
    w_clean[hit] = 0.0
    assert 50 < hit.sum() < hit.size // 5
    v, shapes, starts, g = dev(c.value), dev(c.shapes), dev(c.starts), dev(c.grad_out)
    out_bad = mda.ms_deform_attn_forward(v, shapes, starts, dev(loc_bad), dev(c.weights), 64)
    out_clean = mda.ms_deform_attn_forward(v, shapes, starts, dev(loc_clean), dev(w_clean), 64)
    assert bool(torch.isfinite(out_bad).all()) and bits(out_bad) == bits(out_clean)
    gv_bad, gl_bad, gw_bad = mda.ms_deform_attn_backward(v, shapes, starts, dev(loc_bad), dev(c.weights), g, 64)
    gv_clean, gl_clean, gw_clean = mda.ms_deform_attn_backward(v, shapes, starts, dev(loc_clean), dev(w_clean), g, 64)
    gl_bad, gw_bad, gl_clean, gw_clean = (t.cpu().numpy() for t in (gl_bad, gw_bad, gl_clean, gw_clean))
    assert np.isfinite(gl_bad).all() and np.isfinite(gw_bad).all() and bool(torch.isfinite(gv_bad).all())
    assert (gl_bad[hit] == 0).all() and (gw_bad[hit] == 0).all()
    assert gl_bad[~hit].tobytes() == gl_clean[~hit].tobytes() and gw_bad[~hit].tobytes() == gw_clean[~hit].tobytes()
    assert np.abs(gl_bad[~hit]).max() > 0 and np.abs(gw_bad[~hit]).max() > 0
    check(name, "grad_value", gv_bad, gv_clean.cpu().numpy().astype(np.float64), "grad value against the zero-weight run")


def test_shapes_that_exceed_the_value_table_read_nothing_outside_it():
    """dino_small with its last level enlarged by one row (sum of h * w = S + 1): the kernels' guard (a corner is read or added to only
    if its flattened index is below S: ``msda_locate`` in csrc/ms_deform_attn.hip) keeps every access inside the tensors.  The call
    returns and its outputs are finite; the numbers themselves are not specified."""
    from lvdgs import ms_deform_attn as mda
    c, v, _, starts, loc, w = inputs("dino_small", "snapped")
    grown = c.shapes.copy()
    grown[-1, 0] += 1
    assert int((grown[:, 0] * grown[:, 1]).sum()) == c.S + 1
    shapes = dev(grown)
    out = mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    grads = mda.ms_deform_attn_backward(v, shapes, starts, loc, w, dev(c.grad_out), 64)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (out,) + tuple(grads))


def test_layouts_dtypes_and_streams():
    from lvdgs import ms_deform_attn as mda
    c, v, shapes, starts, loc, w = inputs("dino_small", "generic")
    g = dev(c.grad_out)
    plain = mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    plain_grads = mda.ms_deform_attn_backward(v, shapes, starts, loc, w, g, 64)
    view = v.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)          # (B, S, H, D) over a (B, H, S, D) buffer
    assert not view.is_contiguous() and torch.equal(view, v)
    assert bits(mda.ms_deform_attn_forward(view, shapes, None, loc, w, 64)) == bits(plain)
    assert bits(mda.ms_deform_attn_forward(v, shapes.int(), starts.int(), loc, w, 64)) == bits(plain)
    gv, gl, gw = mda.ms_deform_attn_backward(view, shapes.int(), None, loc, w, g, 64)
    assert bits(gl) == bits(plain_grads[1]) and bits(gw) == bits(plain_grads[2])
    check("dino_small", "grad_value", gv, plain_grads[0].cpu().numpy().astype(np.float64), "grad value from the view")
    side = torch.cuda.Stream(device=v.device)
    side.wait_stream(torch.cuda.current_stream(v.device))
    with torch.cuda.stream(side):
        out = mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
        gl2 = mda.ms_deform_attn_backward(v, shapes, starts, loc, w, g, 64)[1]
    side.synchronize()
    assert bits(out) == bits(plain) and bits(gl2) == bits(plain_grads[1])
    # an unaligned value table (a view one float into a buffer) takes the scalar path
    buf = torch.zeros(v.numel() + 1, device=v.device)
    buf[1:] = v.reshape(-1)
    off = buf[1:].view(v.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    check("dino_small", "out_generic", mda.ms_deform_attn_forward(off, shapes, starts, loc, w, 64), oracle_forward("dino_small", "generic"),
          "out generic, unaligned value")


def test_empty_work():
    from lvdgs import ms_deform_attn as mda
    c, v, shapes, starts, loc, w = inputs("dino_small", "generic")
    out = mda.ms_deform_attn_forward(v, shapes, starts, loc[:, :0], w[:, :0], 64)
    assert tuple(out.shape) == (c.B, 0, c.H * c.D)
    gv, gl, gw = mda.ms_deform_attn_backward(v, shapes, starts, loc[:, :0], w[:, :0], dev(c.grad_out)[:, :0], 64)
    assert tuple(gv.shape) == c.value.shape and not bool(gv.any()) and tuple(gl.shape) == (c.B, 0, c.H, c.L, c.P, 2) and tuple(gw.shape) == (c.B, 0, c.H, c.L, c.P)
    out = mda.ms_deform_attn_forward(v[:0], shapes, starts, loc[:0], w[:0], 64)
    assert tuple(out.shape) == (0, c.Q, c.H * c.D)
    gv, gl, gw = mda.ms_deform_attn_backward(v[:0], shapes, starts, loc[:0], w[:0], dev(c.grad_out)[:0], 64)
    assert tuple(gv.shape) == (0, c.S, c.H, c.D) and tuple(gl.shape) == (0, c.Q, c.H, c.L, c.P, 2) and tuple(gw.shape) == (0, c.Q, c.H, c.L, c.P)
