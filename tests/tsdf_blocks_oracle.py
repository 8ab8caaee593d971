"""The block-sparse TSDF rules of include/lvdgs.h ("Block-sparse TSDF volume") in NumPy.

``allocation_keys_f32``   the allocation, float32, operation for operation: the sorted keys and the samples out of range;
``allocation_keys_f64``   the allocation stated independently in float64 (rays as matrix products): used to REPORT how many keys a
                          rounding moves, never to gate;
``BlockMirror``           a dense mirror volume (a ``tsdf_oracle`` dict) over a box of blocks, of which only the samples of allocated
                          blocks count: ``integrate_blocks_f32`` per call, ``block_planes``, ``mesh_blocks_f32``.

The box is ``nb`` blocks per axis from block ``lo``; dense index + 8 * lo = the signed global index, and positions are evaluated
from the global index (``lo`` = 0: exactly ``tsdf_oracle.integrate_f32``).
"""
import numpy as np

import tsdf_oracle as orc

F = np.float32
BIAS = 1 << 20


def pack_key(bx, by, bz):
    for b in (bx, by, bz):
        assert -BIAS <= int(b) < BIAS, b
    return 1 << 63 | (int(bz) + BIAS) << 42 | (int(by) + BIAS) << 21 | (int(bx) + BIAS)


def unpack_key(key):
    key = int(key)
    return tuple(((key >> s) & 0x1FFFFF) - BIAS for s in (0, 21, 42))


def pack_keys(b):
    """(n, 3) integer block coordinates -> uint64 keys."""
    b = np.asarray(b, np.int64) + BIAS
    return (np.uint64(1 << 63) | (b[:, 2].astype(np.uint64) << np.uint64(42)) | (b[:, 1].astype(np.uint64) << np.uint64(21))
            | b[:, 0].astype(np.uint64))


def unpack_keys(keys):
    keys = np.asarray(keys, np.uint64)
    return np.stack([((keys >> np.uint64(s)) & np.uint64(0x1FFFFF)).astype(np.int64) - BIAS for s in (0, 21, 42)], 1)


def ray_steps(voxel_size, trunc):
    """(n_steps, step) as the library's host code computes them, in float32."""
    vs, tr = F(voxel_size), F(trunc)
    return 2 * int(np.ceil((tr + vs) / (F(0.5) * vs))) + 1, F(0.5) * vs


def allocation_keys_f32(origin, voxel_size, trunc, views):
    """-> (sorted unique uint64 keys, samples out of range): steps 1-3 of the allocation for every view and pixel."""
    vs = F(voxel_size)
    o = np.asarray(origin, F)
    n_steps, step = ray_steps(voxel_size, trunc)
    edge = F(8.0) * vs
    keys, outside = [], 0
    with np.errstate(all="ignore"):
        for V in views:
            H, W = V["depth"].shape
            R, T = V["R"].astype(F), V["T"].astype(F)
            fx, fy, cx, cy = (F(v) for v in V["intrinsics"])
            vi, ui = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            d = V["depth"]
            use = (d > 0) & (d <= F(V["depth_trunc"]))
            if V["mask"] is not None:
                use &= V["mask"].reshape(H, W) != 0
            d, ui, vi = d[use], ui[use], vi[use]
            xn, yn = (ui.astype(F) - cx) / fx, (vi.astype(F) - cy) / fy
            z0 = d - F(n_steps // 2) * step
            assert xn.dtype == F and z0.dtype == F
            for s in range(n_steps):
                zs = z0 + F(s) * step
                front = zs > F(V["depth_min"])
                q = (xn * zs - T[0], yn * zs - T[1], zs - T[2])
                c = []
                for a in range(3):
                    pw = (R[0, a] * q[0] + R[1, a] * q[1]) + R[2, a] * q[2]
                    c.append(np.floor((pw - o[a]) / edge))
                    assert c[-1].dtype == F
                inside = np.logical_and.reduce([(x >= F(-1048576.0)) & (x < F(1048576.0)) for x in c])
                outside += int((front & ~inside).sum())
                sel = front & inside
                keys.append(pack_keys(np.stack([x[sel].astype(np.int64) for x in c], 1)))
    keys = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.uint64)
    return keys, outside


def allocation_keys_f64(origin, voxel_size, trunc, views):
    """The same allocation in float64, from the float32 inputs: every pixel's ray as a matrix product."""
    vs = np.float64(F(voxel_size))
    o = np.asarray(origin, F).astype(np.float64)
    n_steps, step = ray_steps(voxel_size, trunc)
    offsets = (np.arange(n_steps) - n_steps // 2) * np.float64(step)
    blocks = []
    with np.errstate(all="ignore"):
        for V in views:
            H, W = V["depth"].shape
            R, T = V["R"].astype(np.float64), V["T"].astype(np.float64)
            fx, fy, cx, cy = V["intrinsics"]
            d = V["depth"].astype(np.float64)
            use = (d > 0) & (d <= np.float64(V["depth_trunc"]))
            if V["mask"] is not None:
                use &= V["mask"].reshape(H, W) != 0
            vi, ui = np.nonzero(use)
            rays = np.stack([(ui - cx) / fx, (vi - cy) / fy, np.ones(len(ui))], 1)            # (n, 3), unit camera z
            zs = d[use][:, None] + offsets[None, :]                                          # (n, steps)
            pc = rays[:, None, :] * zs[:, :, None]
            pw = (pc - T) @ R                                                                # R^T (p_c - T), row vectors
            b = np.floor((pw - o) / (8.0 * vs))
            ok = (zs > np.float64(V["depth_min"])) & np.all((b >= -BIAS) & (b < BIAS), -1)
            blocks.append(b[ok].astype(np.int64))
    return np.unique(pack_keys(np.concatenate(blocks))) if blocks else np.zeros(0, np.uint64)


def _integrate_f32_at(vol, views, index_lo):
    """``tsdf_oracle.integrate_f32`` with the lattice indices moved by ``index_lo``: positions from the signed global index."""
    real = orc.lattice_indices
    orc.lattice_indices = lambda dims: tuple(a + int(l) for a, l in zip(real(dims), index_lo))
    try:
        return orc.integrate_f32(vol, views)
    finally:
        orc.lattice_indices = real


class BlockMirror:
    def __init__(self, origin, voxel_size, lo, nb, trunc=None, max_weight=64.0, color=True):
        self.lo, self.nb = tuple(int(v) for v in lo), tuple(int(v) for v in nb)
        self.vol = orc.empty_volume(tuple(8 * n for n in self.nb), origin, voxel_size, trunc=trunc, max_weight=max_weight, color=color)
        self.keys = np.zeros(0, np.uint64)
        self.out_of_range = 0

    @classmethod
    def around(cls, origin, voxel_size, views, trunc=None, **kw):
        """The mirror whose box is the bounding box of everything ``views`` allocate."""
        tr = 4.0 * float(voxel_size) if trunc is None else trunc
        b = unpack_keys(allocation_keys_f32(origin, voxel_size, tr, views)[0])
        lo, hi = b.min(0), b.max(0)
        return cls(origin, voxel_size, lo, hi - lo + 1, trunc=trunc, **kw)

    def allocated_samples(self, keys=None):
        """(nz, ny, nx) bool: the samples of the allocated blocks."""
        b = unpack_keys(self.keys if keys is None else keys) - np.asarray(self.lo)
        assert ((b >= 0) & (b < np.asarray(self.nb))).all(), "a block outside the mirror's box"
        grid = np.zeros(self.nb[::-1], bool)
        grid[b[:, 2], b[:, 1], b[:, 0]] = True
        return np.repeat(np.repeat(np.repeat(grid, 8, 0), 8, 1), 8, 2)

    def integrate_blocks_f32(self, views, keys=None):
        """One library call: the call's keys join the set (``keys``: the set the device allocated, where a pool dropped some), the dense
        rule runs on a copy of the box and only the samples of allocated blocks are kept."""
        new, outside = allocation_keys_f32(self.vol["origin"], self.vol["voxel_size"], self.vol["trunc"], views)
        self.out_of_range += outside
        self.keys = np.union1d(self.keys, new) if keys is None else np.asarray(keys, np.uint64)
        tmp = orc.copy_volume(self.vol)
        _integrate_f32_at(tmp, views, tuple(8 * l for l in self.lo))
        keep = self.allocated_samples().reshape(-1)
        for name in orc.PLANES:
            if name in self.vol:
                self.vol[name] = np.where(keep, tmp[name], self.vol[name])
        return new

    def block_planes(self, name, keys=None):
        """(n, 8, 8, 8) indexed [block in key order, k, j, i]."""
        return self.block_planes_unsorted(name, np.sort(self.keys if keys is None else np.asarray(keys, np.uint64)))

    def block_planes_unsorted(self, name, keys):
        """(n, 8, 8, 8) indexed [block in the order of ``keys``, k, j, i]."""
        b = unpack_keys(keys) - np.asarray(self.lo)
        nz, ny, nx = self.nb[::-1]
        grid = self.vol[name].reshape(nz, 8, ny, 8, nx, 8).transpose(0, 2, 4, 1, 3, 5)
        return grid[b[:, 2], b[:, 1], b[:, 0]]

    def masked_volume(self):
        """The box as the extraction sees it: samples of blocks that are not allocated are unobserved."""
        vol = orc.copy_volume(self.vol)
        vol["weight"] = np.where(self.allocated_samples().reshape(-1), vol["weight"], F(0))
        return vol

    def mesh_blocks_f32(self):
        """``tsdf_oracle.mesh_f32`` of the box (``lo`` must be 0: its positions come from the dense index), vertices re-ordered to
        (key, l) and faces to (key, l, axis), vertex numbers remapped."""
        assert self.lo == (0, 0, 0), "mesh_blocks_f32 needs a box that starts at block 0"
        vol = self.masked_volume()
        vertices, colors, faces = orc.mesh_f32(vol)
        cells = active_cells(vol)                                   # (V, 3) (i, j, k) in mesh_f32's vertex order
        assert len(cells) == len(vertices)
        rank_key = cell_order_key(cells)
        perm = np.argsort(rank_key, kind="stable")                  # new position -> old number
        number = np.empty(len(perm), np.int64)
        number[perm] = np.arange(len(perm))
        # a pair of triangles belongs to the sample of its own cell c2 -- the vertex both triangles hold besides v0 -- and the pairs of
        # one sample already stand in axis order: a stable sort by the sample's (key, l) is the order of the header
        a, b = faces[0::2].astype(np.int64), faces[1::2].astype(np.int64)
        v2 = np.where((a[:, 1] == b[:, 1]) | (a[:, 1] == b[:, 2]), a[:, 1], a[:, 2])
        order = np.argsort(rank_key[v2], kind="stable")
        pairs = np.stack([a[order], b[order]], 1).reshape(-1, 3)
        return vertices[perm], None if colors is None else colors[perm], number[pairs].astype(np.int32)


def active_cells(vol):
    """(V, 3) low corners (i, j, k) of the active cells in the order of their sample index (``mesh_f32``'s vertex order)."""
    nx, ny, nz = vol["dims"]
    obs = vol["weight"].reshape(nz, ny, nx) > 0
    ins = vol["tsdf"].reshape(nz, ny, nx) < 0
    corner = lambda a, d: a[d[2]:d[2] + nz - 1, d[1]:d[1] + ny - 1, d[0]:d[0] + nx - 1]
    corners = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    n_in = sum(corner(ins, d).astype(np.int32) for d in corners)
    active = np.logical_and.reduce([corner(obs, d) for d in corners]) & (n_in > 0) & (n_in < 8)
    kk, jj, ii = np.nonzero(active)
    return np.stack([ii, jj, kk], 1)


def cell_order_key(cells):
    """A sortable integer per cell: (bz, by, bx, l) for non-negative cells of a box that starts at block 0."""
    b, l = cells // 8, cells % 8
    return ((b[:, 2] * (1 << 21) + b[:, 1]) * (1 << 21) + b[:, 0]) * 512 + (l[:, 0] + 8 * (l[:, 1] + 8 * l[:, 2]))


def mesh_as_sets(vertices, colors, faces):
    """(the set of vertex rows with their colours, the set of faces as triples of vertex rows): equality whatever the numbering."""
    rows = np.asarray(vertices, F) if colors is None else np.concatenate([np.asarray(vertices, F), np.asarray(colors, F)], 1)
    rows = [r.tobytes() for r in rows]
    return set(rows), {(rows[a], rows[b], rows[c]) for a, b, c in np.asarray(faces)}
