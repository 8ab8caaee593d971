"""NumPy restatement of the map edits of ``lvdgs.gaussian_model.GaussianModel`` that carries PROVENANCE through them.

Every stage is written as ``gaussian_model.py`` states it -- ``densify_and_clone``, ``densify_and_split`` (with its ``prune_points`` of the
split sources), the final prune, each through ``densification_postfix`` / ``prune_points`` -- on a list of rows, and every ``cat`` and
``index_select`` moves three provenance arrays with the rows:

``src``        the row of the ORIGINAL map the row's bytes come from;
``kind``       KEEP (an original), CLONE, SPLIT0 / SPLIT1 (the first / second child of a split);
``noise_row``  for a split child, the row of the ``randn((2 n_split_sel, 3))`` draw of ``densify_and_split`` it was made with; else -1.

Nothing here composes the stages into one formula: what the device plan must reproduce is what falls out of running them in a row.
Decisions are float32 (NumPy's ``exp`` / ``log``); the cases (``map_edit_cases``) keep every activated value away from its threshold,
so a last-bit difference between exponentials cannot flip one.
"""
import numpy as np

KEEP, CLONE, SPLIT0, SPLIT1 = 0, 1, 2, 3
f32 = np.float32


def sigmoid(x):
    return (f32(1) / (f32(1) + np.exp(-x.astype(f32)))).astype(f32)


class Rows:
    """The per-row state the decisions read -- raw ``scaling`` (n, S), raw ``opacity`` (n, 1), ``max_radii2D`` (n,) -- and provenance."""

    def __init__(self, scaling, opacity, max_radii2D):
        n = scaling.shape[0]
        self.scaling, self.opacity, self.max_radii2D = scaling.astype(f32), opacity.astype(f32).reshape(n, 1), max_radii2D.astype(f32)
        self.src = np.arange(n, dtype=np.int64)
        self.kind = np.full(n, KEEP, dtype=np.int64)
        self.noise_row = np.full(n, -1, dtype=np.int64)

    @property
    def get_scaling(self):
        return np.exp(self.scaling)

    def index_select(self, idx):
        for k in ("scaling", "opacity", "max_radii2D", "src", "kind", "noise_row"):
            setattr(self, k, getattr(self, k)[idx])

    def prune_points(self, mask):
        self.index_select(np.nonzero(~mask)[0])

    def densification_postfix(self, new_scaling, new_opacity, new_src, new_kind, new_noise_row):
        self.scaling = np.concatenate((self.scaling, new_scaling))
        self.opacity = np.concatenate((self.opacity, new_opacity))
        self.src = np.concatenate((self.src, new_src))
        self.kind = np.concatenate((self.kind, new_kind))
        self.noise_row = np.concatenate((self.noise_row, new_noise_row))
        self.max_radii2D = np.zeros(self.scaling.shape[0], dtype=f32)     # the statistics start again at the new size

    def densify_and_clone(self, grads, grad_threshold, scene_extent, percent_dense):
        norm = np.abs(grads[:, 0])                                       # torch.norm over a dimension of one element
        sel = (norm >= f32(grad_threshold)) & (self.get_scaling.max(axis=1) <= f32(percent_dense * scene_extent))
        idx = np.nonzero(sel)[0]
        self.densification_postfix(self.scaling[idx], self.opacity[idx], self.src[idx], np.full(idx.size, CLONE), np.full(idx.size, -1))
        return idx.size

    def densify_and_split(self, grads, grad_threshold, scene_extent, percent_dense, N=2):
        n_init = self.scaling.shape[0]
        padded = np.zeros(n_init, dtype=f32)
        padded[:grads.shape[0]] = grads[:, 0]
        sel = (padded >= f32(grad_threshold)) & (self.get_scaling.max(axis=1) > f32(percent_dense * scene_extent))
        idx = np.nonzero(sel)[0]
        scaling_sel = self.get_scaling[idx]
        new_scaling = np.log(np.tile(scaling_sel, (N, 1)) / f32(0.8 * N)).astype(f32)
        kinds = np.concatenate([np.full(idx.size, SPLIT0 + k) for k in range(N)])
        # samples = randn((N * n_sel, 3)) * stds: child j of the postfix's new rows takes row j of the draw
        self.densification_postfix(new_scaling, np.tile(self.opacity[idx], (N, 1)), np.tile(self.src[idx], N), kinds, np.arange(N * idx.size))
        self.prune_points(np.concatenate((sel, np.zeros(N * idx.size, dtype=bool))))
        return idx.size


def densify_and_prune(scaling, opacity, max_radii2D, grad_accum, denom, max_grad, min_opacity, extent, max_screen_size, percent_dense):
    """-> dict(src, kind, noise_row, n_out, n_keep, n_clone, n_split_sel, n_pruned_final) of ``GaussianModel.densify_and_prune``."""
    rows = Rows(scaling, opacity, max_radii2D)
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = (grad_accum.astype(f32) / denom.astype(f32)).reshape(-1, 1)
    grads = np.where(np.isnan(grads), f32(0), grads)
    rows.densify_and_clone(grads, max_grad, extent, percent_dense)
    n_split_sel = rows.densify_and_split(grads, max_grad, extent, percent_dense)
    prune = sigmoid(rows.opacity)[:, 0] < f32(min_opacity)
    if max_screen_size:
        big_vs = rows.max_radii2D > f32(max_screen_size)
        big_ws = rows.get_scaling.max(axis=1) > f32(0.1 * extent)
        prune = prune | big_vs | big_ws
    before = rows.src.size
    rows.prune_points(prune)
    return dict(src=rows.src, kind=rows.kind, noise_row=rows.noise_row, n_out=rows.src.size, n_keep=int((rows.kind == KEEP).sum()),
                n_clone=int((rows.kind == CLONE).sum()), n_split_sel=n_split_sel, n_pruned_final=before - rows.src.size)


def prune_points(n, mask):
    """-> the same dict for ``GaussianModel.prune_points(mask)``."""
    src = np.nonzero(~np.asarray(mask, dtype=bool))[0]
    return dict(src=src, kind=np.full(src.size, KEEP), noise_row=np.full(src.size, -1), n_out=src.size, n_keep=src.size, n_clone=0,
                n_split_sel=0, n_pruned_final=n - src.size)


def pruning_pass(vis_rows, kf_id, prune_mode, prune_num, window, initialized):
    """``backend_map._pruning_pass``'s rule: -> (the dict, n_obs of every row before the prune)."""
    n = kf_id.shape[0]
    n_obs = np.zeros(n, dtype=np.int32)
    for r in vis_rows:
        n_obs += r.astype(np.int32)
    if prune_mode == "odometry":
        to_prune = n_obs < 3
    else:
        mask = kf_id >= sorted(window, reverse=True)[2]
        if not initialized:
            mask = kf_id >= 0
        to_prune = (n_obs <= prune_num) & mask
    return prune_points(n, to_prune), n_obs


def materialise(column, src, kind, zero_new=False):
    """A COPY (``zero_new=False``) or ZERO column after the edit."""
    out = column[src]
    if zero_new:
        out = out.copy()
        out[kind != KEEP] = 0
    return out
