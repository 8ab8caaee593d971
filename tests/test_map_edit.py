"""Map edit without a GPU: the provenance oracle against the project's own host path, the refusals (the argument blocks' layouts: tests/test_abi.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_edit_cases as cases
import map_edit_oracle as orc
from lvdgs import _lib
from lvdgs.gaussian_model import build_rotation

CPU_SIZES = (0, 1, 65, 1025)      # (the oracle and the host path are size-blind: the large sizes are the GPU tests')
CASES = [(k, n, S, d) for k in cases.KINDS for n in CPU_SIZES for S, d in ((3, 3), (1, 0))] + [("mixed", 1023, 3, 0)]


def expected_after_densify(case, o, seed):
    """Every tensor of the model after densify_and_prune, from the oracle's provenance and the host statements for the children."""
    src, kind, noise_row = o["src"], o["kind"], o["noise_row"]
    out = {}
    for name in cases.GROUPS:
        out[name] = torch.from_numpy(orc.materialise(case[name], src, kind))
        out["exp_avg_" + name] = torch.from_numpy(orc.materialise(case["exp_avg_" + name], src, kind, zero_new=True))
        out["exp_avg_sq_" + name] = torch.from_numpy(orc.materialise(case["exp_avg_sq_" + name], src, kind, zero_new=True))
    child = kind >= orc.SPLIT0
    if child.any() or o["n_split_sel"]:
        noise = torch.randn((2 * o["n_split_sel"], 3), generator=torch.Generator().manual_seed(seed))
        s = torch.from_numpy(case["scaling"][src[child]])
        samples = noise[torch.from_numpy(noise_row[child])] * torch.exp(s)
        R = build_rotation(torch.from_numpy(case["rotation"][src[child]]))
        out["xyz"][torch.from_numpy(child)] = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + torch.from_numpy(case["xyz"][src[child]])
        out["scaling"][torch.from_numpy(child)] = torch.log(torch.exp(s) / (0.8 * 2))
    n = src.size
    out.update(grad_accum=torch.zeros(n, 1), denom=torch.zeros(n, 1), max_radii2D=torch.zeros(n),
               kf_ids=torch.from_numpy(case["kf_ids"][src]), n_obs=torch.from_numpy(case["n_obs"][src]))
    return out


@pytest.mark.parametrize("kind,n,S,degree", CASES)
def test_oracle_is_the_host_path(kind, n, S, degree):
    """The oracle's (src, kind, noise_row) give the tensors GaussianModel's host statements leave, on the CPU, bit for bit.  Row
    identities travel in f_dc, KEEP rows alone keep non-zero moments, clones keep the source's scale and children show their noise row in
    their position: equal tensors are equal src / kind / noise_row lists."""
    case = cases.make_case(kind, n, S, degree)
    m = cases.build_model(case, "cpu")
    o = orc.densify_and_prune(case["scaling"], case["opacity"], case["max_radii2D"], case["grad_accum"], case["denom"], case["max_grad"],
                              case["min_opacity"], case["extent"], case["max_screen_size"], case["percent_dense"])
    assert o["n_out"] == o["n_keep"] + o["n_clone"] + int((o["kind"] >= orc.SPLIT0).sum())
    if kind == "all_clone":
        assert o["n_split_sel"] == 0 and o["n_keep"] == o["n_clone"] and o["n_keep"] + o["n_pruned_final"] // 2 == n    # an original and its clone stay or go together
    if kind == "all_split":
        assert o["n_split_sel"] == n and o["n_keep"] == 0
    if kind == "all_pruned":
        assert o["n_out"] == 0
    if kind == "children_pruned":
        assert o["n_split_sel"] == n and o["n_out"] == 0 and o["n_pruned_final"] == 2 * n
    if kind == "none":
        assert o["n_clone"] == 0 and o["n_split_sel"] == 0
    if S == 1:
        # the host statements cannot split an isotropic map at all: bmm of (b, 3, 3) with the (b, 1, 1) samples raises, selected rows or
        # not.  What the host path CAN do with such a map is prune it.
        with pytest.raises(RuntimeError):
            m.densify_and_prune(case["max_grad"], case["min_opacity"], case["extent"], case["max_screen_size"])
        m = cases.build_model(case, "cpu")
        mask = np.random.default_rng(n).random(n) < 0.3
        m.prune_points(torch.from_numpy(mask))
        p = orc.prune_points(n, mask)
        got = cases.model_tensors(m)
        for name in cases.GROUPS:
            assert torch.equal(got[name], torch.from_numpy(orc.materialise(case[name], p["src"], p["kind"]))), name
            assert torch.equal(got["exp_avg_" + name], torch.from_numpy(orc.materialise(case["exp_avg_" + name], p["src"], p["kind"]))), name
        assert torch.equal(got["kf_ids"], torch.from_numpy(case["kf_ids"][p["src"]])) and torch.equal(got["max_radii2D"], torch.from_numpy(case["max_radii2D"][p["src"]]))
        return
    m.generator = torch.Generator().manual_seed(11)
    m.densify_and_prune(case["max_grad"], case["min_opacity"], case["extent"], case["max_screen_size"])
    got, want = cases.model_tensors(m), expected_after_densify(case, o, 11)
    assert got["xyz"].shape[0] == o["n_out"]
    for name, t in want.items():
        assert got[name].shape == t.shape and torch.equal(got[name], t), name


def test_cases_cover_what_the_issue_names():
    """Ties at the threshold, 0 / 0 and x / 0 rows are in the mixed case, and both decisions of every comparison occur."""
    case = cases.make_case("mixed", 1025, 3, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = case["grad_accum"] / case["denom"]
    assert (g == np.float32(case["max_grad"])).sum() > 50 and np.isnan(g).sum() > 50 and np.isinf(g).sum() > 50
    o = orc.densify_and_prune(case["scaling"], case["opacity"], case["max_radii2D"], case["grad_accum"], case["denom"], case["max_grad"],
                              case["min_opacity"], case["extent"], case["max_screen_size"], case["percent_dense"])
    assert all((o["kind"] == k).sum() > 10 for k in range(4)) and o["n_pruned_final"] > 10
    ties = np.nonzero((g == np.float32(case["max_grad"]))[:, 0])[0]
    assert np.isin(ties, o["src"][o["kind"] != orc.KEEP]).any()        # a tie is selected: >= at equality


def _plan_args():
    a = _lib.MapEditPlanArgs(mode=_lib.EDIT_PRUNE, num_gaussians=100, capacity=100)
    # (never dereferenced: every call here is refused before a launch)
    a.src = a.kind = a.noise_row = a.host_state = a.scratch = a.remove = 256
    a.host_bytes = 4 * (_lib.EDIT_HOST_SRC + 200)
    a.scratch_bytes = _lib.lib().lvdgs_map_edit_scratch_bytes(100)
    return a


def test_plan_refusals_without_gpu():
    L = _lib.lib()
    err = lambda: L.lvdgs_last_error()
    assert L.lvdgs_map_edit_scratch_bytes(-1) == 0
    assert 0 < L.lvdgs_map_edit_scratch_bytes(0) <= L.lvdgs_map_edit_scratch_bytes(70_001) and L.lvdgs_map_edit_scratch_bytes(70_001) >= 70_001
    assert L.lvdgs_map_edit_plan(None, None) == _lib.E_INVALID and b"NULL" in err()
    for field in ("src", "kind", "noise_row", "host_state", "scratch"):
        a = _plan_args()
        setattr(a, field, None)
        assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_INVALID and b"NULL" in err(), field
    a = _plan_args()
    a.scratch_bytes -= 1
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_INVALID and b"scratch too small" in err()
    a = _plan_args()
    a.num_gaussians = -1
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE
    a = _plan_args()
    a.mode = 2
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"mode" in err()
    a = _plan_args()
    a.capacity = 99
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"capacity" in err()
    a = _plan_args()
    a.host_bytes -= 4
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"host_state" in err()
    # rule (b): more than 16 rows, a NULL row, no kf ids, an element size it has no read for
    a = _plan_args()
    a.remove, a.kf_id, a.n_obs, a.num_vis_rows = None, 256, 256, 17
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"visibility rows" in err()
    a.num_vis_rows = 2
    a.vis_rows[0] = 256
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_INVALID and b"row 1 is NULL" in err()
    a.vis_rows[1], a.vis_stride = 256, 2
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"vis_stride" in err()
    a.vis_stride, a.kf_id = 1, None
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_INVALID and b"kf_id" in err()
    # densify: twice the rows, the scale width, the inputs
    a = _plan_args()
    a.mode, a.scale_dims = _lib.EDIT_DENSIFY, 3
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"capacity" in err()
    a.capacity = 200
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_INVALID and b"grad_accum" in err()
    a.grad_accum = a.denom = a.scaling = a.opacity = 256
    a.scale_dims = 2
    assert L.lvdgs_map_edit_plan(C.byref(a), None) == _lib.E_RANGE and b"scale_dims" in err()


def _apply_args(columns=1):
    a = _lib.MapEditApplyArgs(num_gaussians=10, n_out=10, scale_dims=3, num_columns=columns)
    a.src = a.kind = 256
    for k in range(min(columns, _lib.EDIT_MAX_COLUMNS)):
        a.columns[k].in_, a.columns[k].out, a.columns[k].row_bytes, a.columns[k].new_rows = 256, 512, 4, _lib.EDIT_COPY
    return a


def test_apply_refusals_without_gpu():
    L = _lib.lib()
    err = lambda: L.lvdgs_last_error()
    assert L.lvdgs_map_edit_apply(None, None) == _lib.E_INVALID
    a = _apply_args(49)
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_RANGE and b"columns" in err()
    a = _apply_args(-1)
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_RANGE
    for field in ("src", "kind"):
        a = _apply_args()
        setattr(a, field, None)
        assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"NULL" in err()
    for field in ("in_", "out"):
        a = _apply_args(3)
        setattr(a.columns[2], field, None)
        assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"column 2" in err()
    for bad in (0, -4):
        a = _apply_args(2)
        a.columns[1].row_bytes = bad
        assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"row_bytes" in err()
    a = _apply_args()
    a.columns[0].new_rows = 4
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"new_rows" in err()
    a = _apply_args()
    a.columns[0].new_rows, a.columns[0].row_bytes = _lib.EDIT_XYZ, 12
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"noise_row" in err()      # no noise_row / scaling / rotation
    a.columns[0].row_bytes = 16
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"12 bytes" in err()
    a.columns[0].new_rows, a.columns[0].row_bytes = _lib.EDIT_SCALE, 4
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_INVALID and b"scale row" in err()
    a.scale_dims = 2
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.E_RANGE and b"scale_dims" in err()
    a = _apply_args(0)
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.OK                                      # nothing to move
    a = _apply_args(48)
    a.n_out = 0
    assert L.lvdgs_map_edit_apply(C.byref(a), None) == _lib.OK


def test_model_refuses_an_unknown_mode_and_stays_on_the_host_off_gpu():
    case = cases.make_case("mixed", 65, 3, 0)
    m = cases.build_model(case, "cpu", map_edit="fused")        # no GPU under the model: the host statements, as for fused seeding
    assert not m._edits_fused()
    m.prune_points(torch.zeros(65, dtype=torch.bool))
    m.map_edit = "device"
    with pytest.raises(ValueError):
        m.prune_points(torch.zeros(65, dtype=torch.bool))
