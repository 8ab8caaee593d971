"""Multi-scale deformable attention without a GPU: the float64 oracle against the reference's own function (golden file), the
C ABI's refusals, ``install()`` against a stub ``groundingdino`` package, and the Python wrapper's refusals."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import ms_deform_attn_cases as cases
import ms_deform_attn_oracle as orc

from lvdgs import _lib


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ms_deform_attn.npz"))


@pytest.mark.parametrize("name", cases.SMALL)
def test_oracle_equals_the_reference_function(golden, name):
    """Outputs on both location sets and the gradients on the generic one: 1e-12 relative L2, no element excluded."""
    c = cases.case(name)
    assert orc.rel_l2(orc.forward(c.value, c.shapes, c.loc_snapped, c.weights), golden[f"{name}/out_snapped"]) <= 1e-12
    out, gv, gl, gw = orc.forward_backward(c.value, c.shapes, c.loc_generic, c.weights, c.grad_out)
    for key, a in (("out_generic", out), ("grad_value", gv), ("grad_loc", gl), ("grad_weights", gw)):
        ref = golden[f"{name}/{key}"]
        assert a.shape == ref.shape and np.abs(ref).max() > 0, key          # (no comparison of nothing with nothing)
        assert orc.rel_l2(a, ref) <= 1e-12, (key, orc.rel_l2(a, ref))


def test_every_case_has_its_reference_float32_error(golden):
    for name in cases.CASES:
        e = golden[f"{name}/f32_error"]
        assert e.shape == (5, 2) and np.isfinite(e).all() and (e >= 0).all() and (e[:, 0] < 1e-5).all(), (name, e)


def test_c_abi_argument_validation_without_gpu():
    L = _lib.lib()
    p = [C.c_void_p(256 * (i + 1)) for i in range(9)]   # never dereferenced: every call below is rejected, or has nothing to do, before a launch
    fwd = lambda B, S, H, D, Q, Lv, P, ptrs=p: L.lvdgs_ms_deform_attn_forward(*ptrs[:5], B, S, H, D, Q, Lv, P, ptrs[5], None)
    bwd = lambda B, S, H, D, Q, Lv, P, ptrs=p: L.lvdgs_ms_deform_attn_backward(*ptrs[:5], B, S, H, D, Q, Lv, P, *ptrs[5:9], None)
    for call in (fwd, bwd):
        for k in range(7):
            sizes = [1, 24, 8, 32, 6, 4, 4]
            sizes[k] = -1
            assert call(*sizes) == _lib.E_INVALID and b"negative size" in L.lvdgs_last_error(), k
        assert call(1, 24, 8, 32, 6, 0, 4) == _lib.E_INVALID and b"L and P" in L.lvdgs_last_error()
        assert call(1, 24, 8, 32, 6, 4, 0) == _lib.E_INVALID and b"L and P" in L.lvdgs_last_error()
        assert call(1, 24, 0, 32, 6, 4, 4) == _lib.E_INVALID and b"H and D" in L.lvdgs_last_error()
        assert call(2, 1 << 20, 8, 256, 6, 4, 4) == _lib.E_INVALID and b"int32" in L.lvdgs_last_error()          # value: 2^32 elements
        assert call(1, 24, 8, 32, 1 << 24, 4, 4) == _lib.E_INVALID and b"int32" in L.lvdgs_last_error()          # locations: 2^32
        for k in range(6 if call is fwd else 9):                                                                 # each tensor in turn NULL
            ptrs = list(p)
            ptrs[k] = None
            assert call(1, 24, 8, 32, 6, 4, 4, ptrs) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error(), k
        none = [None] * 9
        assert call(0, 24, 8, 32, 6, 4, 4, none) == _lib.OK                                                       # B * Q == 0: nothing to do
        assert call(3, 0, 8, 32, 0, 4, 4, none) == _lib.OK
        assert call(1, 24, 8, 32, 0, 0, 0, none) == _lib.OK                                                       # L = P = 0 without queries


STUB = "try:\n    from groundingdino import _C\nexcept:\n    pass\n"


@pytest.fixture
def stub_groundingdino(tmp_path):
    """A ``groundingdino`` package with an empty ``__init__`` and a ``models/GroundingDINO/ms_deform_attn.py`` that holds just the
    guarded import; ``sys.modules`` and ``sys.path`` are restored afterwards."""
    pkg = tmp_path / "groundingdino"
    (pkg / "models" / "GroundingDINO").mkdir(parents=True)
    for d in (pkg, pkg / "models", pkg / "models" / "GroundingDINO"):
        (d / "__init__.py").write_text("")
    (pkg / "models" / "GroundingDINO" / "ms_deform_attn.py").write_text(STUB)
    saved = {k: v for k, v in sys.modules.items() if k == "groundingdino" or k.startswith("groundingdino.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, str(tmp_path))
    importlib.invalidate_caches()
    yield
    sys.path.remove(str(tmp_path))
    for k in [k for k in sys.modules if k == "groundingdino" or k.startswith("groundingdino.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    importlib.invalidate_caches()


def test_install_before_the_import(stub_groundingdino):
    from lvdgs import ms_deform_attn as mda
    assert mda.install() is mda
    from groundingdino import _C
    assert _C is mda and sys.modules["groundingdino._C"] is mda
    mod = importlib.import_module("groundingdino.models.GroundingDINO.ms_deform_attn")
    assert mod._C is mda and callable(mod._C.ms_deform_attn_forward) and callable(mod._C.ms_deform_attn_backward)


def test_install_repairs_a_failed_import_and_is_idempotent(stub_groundingdino):
    from lvdgs import ms_deform_attn as mda
    mod = importlib.import_module("groundingdino.models.GroundingDINO.ms_deform_attn")
    assert not hasattr(mod, "_C")                                    # the guarded import failed silently
    assert mda.install() is mda and mod._C is mda
    import groundingdino
    assert groundingdino._C is mda and sys.modules["groundingdino._C"] is mda
    before = {k: id(v) for k, v in sys.modules.items() if k.startswith("groundingdino")}
    assert mda.install() is mda and mod._C is mda and groundingdino._C is mda
    assert before == {k: id(v) for k, v in sys.modules.items() if k.startswith("groundingdino")}


def test_install_leaves_a_real_extension_alone_unless_forced(stub_groundingdino, tmp_path):
    from lvdgs import ms_deform_attn as mda
    (tmp_path / "groundingdino" / "_C.py").write_text("ms_deform_attn_forward = ms_deform_attn_backward = None\n")
    importlib.invalidate_caches()
    mod = importlib.import_module("groundingdino.models.GroundingDINO.ms_deform_attn")
    real = mod._C
    assert real is not mda and mda.install() is real and mod._C is real and sys.modules["groundingdino._C"] is real
    assert mda.install(force=True) is mda and mod._C is mda and sys.modules["groundingdino._C"] is mda


def test_wrapper_refuses_cpu_and_half_tensors():
    from lvdgs import ms_deform_attn as mda
    c = cases.case("tiny")
    v, lo, w = torch.from_numpy(c.value.copy()), torch.from_numpy(c.loc_generic.copy()), torch.from_numpy(c.weights.copy())
    shapes, starts = torch.from_numpy(c.shapes.copy()), torch.from_numpy(c.starts.copy())
    with pytest.raises(_lib.LvdgsError, match="GPU"):
        mda.ms_deform_attn_forward(v, shapes, starts, lo, w, 64)
    with pytest.raises(_lib.LvdgsError, match="GPU"):
        mda.ms_deform_attn_backward(v, shapes, starts, lo, w, torch.from_numpy(c.grad_out.copy()), 64)
    with pytest.raises(_lib.LvdgsError, match="GPU"):
        mda.MultiScaleDeformableAttnFunction.apply(v, shapes, None, lo, w, 64)
    with pytest.raises(TypeError, match="float32"):
        mda.ms_deform_attn_forward(v.half(), shapes, starts, lo, w, 64)
    with pytest.raises(TypeError, match="float32"):
        mda.ms_deform_attn_backward(v, shapes, starts, lo.half(), w, torch.from_numpy(c.grad_out.copy()), 64)
