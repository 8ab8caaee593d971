"""Editing the map on the device (HIP, ``csrc/map_edit.hip``; semantics: ``include/lvdgs.h``, DESIGN.md section "Map edit").

``plan_prune``    which rows survive: an explicit mask (``GaussianModel.prune_points``) or the pruning pass's rule evaluated on the
                  device from the window's visibility rows (``backend_map._pruning_pass``).
``plan_densify``  ``GaussianModel.densify_and_prune``'s clone, split-then-prune and final prune as one classification per row.
``apply``         moves the rows of every per-Gaussian array a caller names -- parameters, Adam moments, statistics, visibility rows --
                  in one launch, and computes the split children's positions and scales.

A plan is one library call and ONE wait (``_plan``, a ``_lib.HostCall``) on a block of pinned host memory that then holds the counts and
the source row of every output row; ``apply`` does not wait.  The noise of the split children is the caller's: it is drawn between plan and apply, with
the shape the plan reports, so a model that edits its map this way consumes its generator as the host statements do.

A ``Plan``'s device arrays belong to the per-device outputs and are valid until the next plan on that device.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_plan = _lib.HostCall("lvdgs_map_edit_plan", tag=_lib.EDIT_SEQ, headroom=True)     # the block grows with the map: half as much again when it does
_outputs = {}     # device index -> {"src", "kind", "noise_row": the plan's device buffers; "block", "scratch": what _plan lends the plan being made}
INT32_MIN = -2 ** 31
COPY, ZERO, XYZ, SCALE = _lib.EDIT_COPY, _lib.EDIT_ZERO, _lib.EDIT_XYZ, _lib.EDIT_SCALE


class Plan:
    """What one ``lvdgs_map_edit_plan`` call leaves.  ``src`` (n_out,) int32, ``kind`` (n_out,) uint8, ``noise_row`` (n_out,) int32 on
    the device; ``src_cpu`` (n_out,) int64 and, for the pruning rule, ``n_obs_cpu`` (n_out,) int32 on the host, copied out of the pinned
    block; ``n_obs`` (n_in,) int32 on the device for the pruning rule; the counts of the header."""
    __slots__ = ("mode", "device", "n_in", "n_out", "n_keep", "n_clone", "n_split_sel", "n_pruned_final", "scale_dims",
                 "src", "kind", "noise_row", "src_cpu", "n_obs", "n_obs_cpu")


def _device_state(device, n, rows):
    """The per-device buffers, grown on demand: the pinned block for 2 ``n`` rows, scratch for ``n``, plan outputs for ``rows``."""
    st = _outputs.setdefault(device.index, {"src": None})
    st["block"], st["scratch"] = _plan.resources(device, 4 * max(_lib.EDIT_HOST_SRC + 2 * n, 4096), _lib.lib().lvdgs_map_edit_scratch_bytes(n))
    if st["src"] is None or st["src"].numel() < rows:
        cap = max(rows + rows // 2, 1024)
        st["src"] = torch.empty(cap, dtype=torch.int32, device=device)
        st["kind"] = torch.empty(cap, dtype=torch.uint8, device=device)
        st["noise_row"] = torch.empty(cap, dtype=torch.int32, device=device)
    return st


def _device_of(t):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.LvdgsError("map edit: tensors must be on a GPU (there is no CPU path)")
    return t.device


def _run_plan(a, st, device, n, rule):
    block = st["block"]
    a.num_gaussians = n
    a.src, a.kind, a.noise_row = st["src"].data_ptr(), st["kind"].data_ptr(), st["noise_row"].data_ptr()
    a.capacity = st["src"].numel()
    a.host_state, a.host_bytes = block.data_ptr(), block.numel()
    a.scratch, a.scratch_bytes = st["scratch"].data_ptr(), st["scratch"].numel()
    words = _plan.run(device, a)      # the one wait of the plan; a view of the block: what leaves here is copied out of it below
    p = Plan()
    p.mode, p.device, p.n_in, p.scale_dims = a.mode, device, n, a.scale_dims
    p.n_out, p.n_keep, p.n_clone = int(words[_lib.EDIT_N_OUT]), int(words[_lib.EDIT_N_KEEP]), int(words[_lib.EDIT_N_CLONE])
    p.n_split_sel, p.n_pruned_final = int(words[_lib.EDIT_N_SPLIT_SEL]), int(words[_lib.EDIT_N_PRUNED_FINAL])
    m, h = p.n_out, _lib.EDIT_HOST_SRC
    p.src, p.kind, p.noise_row = st["src"][:m], st["kind"][:m], st["noise_row"][:m]
    p.src_cpu = torch.from_numpy(words[h:h + m].astype(np.int64))
    p.n_obs = p.n_obs_cpu = None
    if rule:
        p.n_obs_cpu = torch.from_numpy(words[h + m:h + 2 * m].copy())
    return p


def plan_prune(n, device, mask=None, *, vis_rows=None, kf_id=None, prune_num=0, min_kf_id=INT32_MIN) -> Plan:
    """The rows of ``[0, n)`` that survive, ascending.  Either ``mask`` -- (n,) bool / uint8 on ``device``, True: remove -- or the rule of
    the pruning pass: ``vis_rows`` (up to 16 (n,) tensors of 0 / 1 on the device: bool, uint8, int32 or int64, all of one type) and ``kf_id`` ((n,) int32 on the device); row i
    goes when ``sum_k vis_rows[k][i] <= prune_num and kf_id[i] >= min_kf_id``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.LvdgsError("map edit: plans are made on a GPU (there is no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device()) if device.index is None else device
    n = int(n)
    st = _device_state(device, n, n)
    a = _lib.MapEditPlanArgs(mode=_lib.EDIT_PRUNE)
    byte_row = lambda t, what: _byte_row(t, n, device, what)
    n_obs = None
    if mask is not None:
        mask = byte_row(mask, "mask")
        a.remove = mask.data_ptr() if n else st["kind"].data_ptr()    # (an empty tensor has no address: any non-NULL one, never read)
    else:
        rows = list(vis_rows or [])
        stride = rows[0].element_size() if rows else 1
        for r in rows:
            if not (torch.is_tensor(r) and r.device == device and r.dtype in (torch.bool, torch.uint8, torch.int32, torch.int64) and r.is_contiguous()
                    and r.numel() == n and r.element_size() == stride):
                raise _lib.LvdgsError(f"map edit: visibility rows must be contiguous ({n},) bool, uint8, int32 or int64 tensors of one type on {device}")
        if len(rows) > _lib.EDIT_MAX_VIS_ROWS:
            raise _lib.LvdgsError(f"map edit: {len(rows)} visibility rows (at most {_lib.EDIT_MAX_VIS_ROWS})")
        if not (torch.is_tensor(kf_id) and kf_id.device == device and kf_id.dtype is torch.int32 and kf_id.is_contiguous() and kf_id.numel() == n):
            raise _lib.LvdgsError("map edit: kf_id must be a contiguous (n,) int32 tensor on the device")
        n_obs = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        a.num_vis_rows, a.vis_stride, a.prune_num, a.min_kf_id = len(rows), stride, int(prune_num), int(min_kf_id)
        for k, r in enumerate(rows):
            a.vis_rows[k] = r.data_ptr() if n else st["kind"].data_ptr()
        a.kf_id, a.n_obs = (kf_id.data_ptr() if n else st["kind"].data_ptr()), n_obs.data_ptr()
    p = _run_plan(a, st, device, n, rule=mask is None)
    p.n_obs = None if n_obs is None else n_obs[:n]
    return p


def _byte_row(t, n, device, what):
    if not (torch.is_tensor(t) and t.device == device and t.dtype in (torch.bool, torch.uint8) and t.is_contiguous() and t.numel() == n):
        raise _lib.LvdgsError(f"map edit: {what} must be a contiguous ({n},) bool or uint8 tensor on {device}")
    return t


def plan_densify(grad_accum, denom, scaling, opacity, grad_threshold, dense_extent, min_opacity, max_screen_size, world_extent) -> Plan:
    """``densify_and_prune`` as one classification: ``grad_accum``, ``denom`` (n, 1), raw ``scaling`` (n, 1 or 3) and raw ``opacity``
    (n, 1), float32 on one GPU; ``dense_extent`` = percent_dense * extent, ``world_extent`` = 0.1 * extent, ``max_screen_size`` 0 or
    None: off."""
    device = _device_of(scaling)
    n, dims = int(scaling.shape[0]), int(scaling.shape[1]) if scaling.ndim == 2 else 0
    if dims not in (1, 3):
        raise _lib.LvdgsError("map edit: scaling must be (n, 1) or (n, 3)")
    for t, what in ((grad_accum, "grad_accum"), (denom, "denom"), (opacity, "opacity")):
        if not _lib.is_f32(t, device) or t.numel() != n:
            raise _lib.LvdgsError(f"map edit: {what} must be a contiguous float32 tensor of {n} values on {device}")
    if not _lib.is_f32(scaling, device):
        raise _lib.LvdgsError("map edit: scaling must be a contiguous float32 tensor")
    st = _device_state(device, n, 2 * n)
    a = _lib.MapEditPlanArgs(mode=_lib.EDIT_DENSIFY, scale_dims=dims, grad_threshold=grad_threshold, dense_extent=dense_extent,
                             min_opacity=min_opacity, max_screen_size=float(max_screen_size or 0.0), world_extent=world_extent)
    spare = st["kind"].data_ptr()      # (an empty tensor has no address: any non-NULL one, never read)
    a.grad_accum, a.denom = grad_accum.data_ptr() or spare, denom.data_ptr() or spare
    a.scaling, a.opacity = scaling.data_ptr() or spare, opacity.data_ptr() or spare
    return _run_plan(a, st, device, n, rule=False)


def apply(plan, columns, noise=None, scaling=None, rotation=None):
    """Move the rows: ``columns`` is a list of ``(in, out, new_rows)`` -- contiguous tensors of plan.n_in and at least plan.n_out rows
    with the same row size, ``new_rows`` one of ``COPY``, ``ZERO``, ``XYZ``, ``SCALE``.  Columns whose rows have no bytes are passed
    over.  ``noise`` (2 plan.n_split_sel, 3) float32, ``scaling`` and ``rotation`` (the sources' raw values): for an ``XYZ`` column.
    No wait."""
    L = _lib.lib()
    device = plan.device
    a = _lib.MapEditApplyArgs(num_gaussians=plan.n_in, n_out=plan.n_out, n_split_sel=plan.n_split_sel, scale_dims=plan.scale_dims or 3)
    a.src, a.kind, a.noise_row = plan.src.data_ptr() or None, plan.kind.data_ptr() or None, plan.noise_row.data_ptr() or None
    if plan.n_out == 0:
        return
    k = 0
    for t_in, t_out, new_rows in columns:
        if t_in.device != device or t_out.device != device or not t_in.is_contiguous() or not t_out.is_contiguous():
            raise _lib.LvdgsError("map edit: columns must be contiguous tensors on the plan's device")
        row_bytes = t_in.element_size() * int(np.prod(t_in.shape[1:], dtype=np.int64))
        if t_in.shape[0] != plan.n_in or t_out.shape[0] < plan.n_out or t_out.element_size() * int(np.prod(t_out.shape[1:], dtype=np.int64)) != row_bytes:
            raise _lib.LvdgsError(f"map edit: column {k}: {tuple(t_in.shape)} -> {tuple(t_out.shape)} for {plan.n_in} -> {plan.n_out} rows")
        if row_bytes == 0:
            continue
        if k >= _lib.EDIT_MAX_COLUMNS:
            raise _lib.LvdgsError(f"map edit: more than {_lib.EDIT_MAX_COLUMNS} columns")
        c = a.columns[k]
        c.in_, c.out, c.row_bytes, c.new_rows = t_in.data_ptr(), t_out.data_ptr(), row_bytes, int(new_rows)
        k += 1
    a.num_columns = k
    if noise is not None:
        if not _lib.is_f32(noise, device) or tuple(noise.shape) != (2 * plan.n_split_sel, 3):
            raise _lib.LvdgsError(f"map edit: noise must be a contiguous ({2 * plan.n_split_sel}, 3) float32 tensor on the plan's device")
        a.noise = noise.data_ptr() or None
    if scaling is not None:
        a.scaling = _lib.f32(scaling, device).data_ptr()
    if rotation is not None:
        a.rotation = _lib.f32(rotation, device).data_ptr()
    with _lib.on_device(device):
        _lib.check(L.lvdgs_map_edit_apply(C.byref(a), _lib.raw_stream(device)), "lvdgs_map_edit_apply")
