"""A block-sparse TSDF volume on the device: the fusion rule and the surface nets of ``tsdf.TsdfVolume`` on an unbounded lattice of
which only the 8 x 8 x 8 blocks near a surface are stored (HIP, ``csrc/tsdf_blocks.hip``; the rules: ``include/lvdgs.h``, "Block-sparse
TSDF volume").

``TsdfBlockVolume.integrate*``   ``lvdgs_tsdf_blocks_integrate``: allocates the blocks the views' depth bands cross, then fuses up to 16
                                 views per call into every block in use; no wait, no copy.
``TsdfBlockVolume.extract_mesh`` ``lvdgs_tsdf_blocks_mesh``: ONE wait, a second only when the guessed capacities were too small.
``TsdfBlockVolume.stats``        blocks in use, keys dropped for want of pool space, samples out of range, table full: one wait.
``TsdfBlockVolume.grow``         a larger pool and table (``lvdgs_tsdf_blocks_rehash``); dropped keys are forgotten.

A volume holds what its pool holds: ``stats()["dropped"]`` > 0 says that surface was left out -- ``grow``, ``reset`` and fuse again.
There is no CPU path: tensors that are not on a GPU raise ``LvdgsError``.
"""
import ctypes as C

import torch

from . import _lib
from .tsdf import Mesh, TsdfVolume, _TsdfBase

_mesh_call = _lib.HostCall("lvdgs_tsdf_blocks_mesh", tag=_lib.TSDF_BLOCKS_SEQ)
_INT32_MAX = 2 ** 31 - 1
BLOCK_EDGE, BLOCK_SAMPLES, COORD_BIAS = 8, 512, 1 << 20
_PLANES = ("tsdf", "weight", "r", "g", "b")


def pack_key(bx, by, bz):
    """The key of block (bx, by, bz), each in [-2^20, 2^20), as the unsigned 64-bit integer of the header."""
    for b in (bx, by, bz):
        if not -COORD_BIAS <= int(b) < COORD_BIAS:
            raise ValueError(f"block coordinate {b} outside [-2^20, 2^20)")
    return 1 << 63 | (int(bz) + COORD_BIAS) << 42 | (int(by) + COORD_BIAS) << 21 | (int(bx) + COORD_BIAS)


def unpack_key(key):
    key = int(key) & (2 ** 64 - 1)
    return tuple(((key >> shift) & 0x1FFFFF) - COORD_BIAS for shift in (0, 21, 42))


def table_slots_for(pool_blocks):
    """The smallest table the library takes for a pool: a power of two, at least twice the pool."""
    return 1 << max(1, (2 * int(pool_blocks) - 1).bit_length())


class TsdfBlockVolume(_TsdfBase):
    """Samples at ``origin + voxel_size * g`` for signed global indices ``g``; block ``b = floor(g / 8)`` per axis, stored when a view's
    depth band crossed it.  ``pool_blocks`` blocks of 512 samples per plane (``tsdf``, ``weight`` and, with ``color``, ``r``, ``g``,
    ``b``), ``block_key`` (pool_blocks int64), the table (``table_slots`` keys and values) and the header.  Fusion (``integrate*``) is
    the dense volume's, into ``lvdgs_tsdf_blocks_integrate``."""
    _integrate = "lvdgs_tsdf_blocks_integrate"

    def __init__(self, origin, voxel_size, pool_blocks, trunc=None, max_weight=64.0, color=True, device="cuda", table_slots=None):
        super().__init__(origin, voxel_size, trunc, max_weight, color, device)
        if len(self.origin) != 3:
            raise _lib.LvdgsError("TsdfBlockVolume: origin has three entries")
        self._allocate(pool_blocks, table_slots)

    def _allocate(self, pool_blocks, table_slots=None):
        pool = int(pool_blocks)
        if not 1 <= pool <= _lib.TSDF_BLOCKS_MAX_POOL:
            raise _lib.LvdgsError(f"TsdfBlockVolume: pool_blocks {pool} outside 1 .. {_lib.TSDF_BLOCKS_MAX_POOL}")
        slots = table_slots_for(pool) if table_slots is None else int(table_slots)
        dev = self.device
        names = _PLANES[:5 if self.color else 2]
        self.pool_blocks, self.table_slots = pool, slots
        self.planes = torch.zeros((len(names), pool * BLOCK_SAMPLES), dtype=torch.float32, device=dev)      # zeroed: an empty volume
        for row, name in enumerate(names):
            setattr(self, name, self.planes[row])
        self.block_key = torch.zeros(pool, dtype=torch.int64, device=dev)
        self.table_keys = torch.zeros(slots, dtype=torch.int64, device=dev)
        self.table_values = torch.zeros(slots, dtype=torch.int32, device=dev)
        self.header = torch.zeros(_lib.TSDF_BLOCKS_HEADER_WORDS, dtype=torch.int32, device=dev)
        self._vol = _lib.TsdfBlocksArgs(
            pool_blocks=pool, table_slots=slots, origin=(C.c_float * 3)(*self.origin), voxel_size=self.voxel_size, trunc=self.trunc,
            max_weight=self.max_weight, tsdf=self.tsdf.data_ptr(), weight=self.weight.data_ptr(),
            r=self.r.data_ptr() if self.color else None, g=self.g.data_ptr() if self.color else None,
            b=self.b.data_ptr() if self.color else None, block_key=self.block_key.data_ptr(), table_keys=self.table_keys.data_ptr(),
            table_values=self.table_values.data_ptr(), header=self.header.data_ptr())

    def bytes_held(self):
        return sum(t.numel() * t.element_size() for t in (self.planes, self.block_key, self.table_keys, self.table_values, self.header))

    def reset(self):
        for t in (self.planes, self.block_key, self.table_keys, self.table_values, self.header):
            t.zero_()
        self.frames = 0

    # ---- what the volume holds -------------------------------------------------------------------
    def stats(self):
        """{blocks, dropped, out_of_range, table_full} of the header: one wait."""
        h = self.header.cpu().numpy()
        return dict(blocks=min(max(int(h[_lib.TSDF_BLOCKS_HEADER_USED]), 0), self.pool_blocks), dropped=int(h[_lib.TSDF_BLOCKS_HEADER_DROPPED]),
                    out_of_range=int(h[_lib.TSDF_BLOCKS_HEADER_OUT_OF_RANGE]) & 0xFFFFFFFF,
                    table_full=bool(int(h[_lib.TSDF_BLOCKS_HEADER_FLAGS]) & _lib.TSDF_BLOCKS_TABLE_FULL))

    def _order(self):
        """The pool indices by ascending key.  A key is negative as an int64 and an unused entry 0: the signed sort puts the blocks in
        use first, in the unsigned order of their keys."""
        return torch.sort(self.block_key).indices

    def blocks(self):
        """(n, 3) int32 block coordinates (bx, by, bz) of the blocks in use, in key order."""
        n = self.stats()["blocks"]
        keys = self.block_key[self._order()[:n]]
        return torch.stack([((keys >> shift) & 0x1FFFFF) - COORD_BIAS for shift in (0, 21, 42)], 1).to(torch.int32)

    def block_planes(self, name):
        """(n, 8, 8, 8) float32, indexed [block in key order, k, j, i]: plane ``name`` of the blocks in use."""
        n = self.stats()["blocks"]
        return getattr(self, name).view(self.pool_blocks, BLOCK_EDGE, BLOCK_EDGE, BLOCK_EDGE)[self._order()[:n]]

    def grow(self, pool_blocks):
        """A pool of ``pool_blocks`` >= the present size and a table to match; what the volume holds is kept, the keys that were
        dropped are forgotten (fuse their views again)."""
        pool = int(pool_blocks)
        if pool < self.pool_blocks:
            raise _lib.LvdgsError(f"TsdfBlockVolume.grow: {pool} blocks is below the present {self.pool_blocks}")
        old = (self.planes, self.block_key, self.header, self.pool_blocks)
        self._allocate(pool)
        self.planes[:, :old[3] * BLOCK_SAMPLES].copy_(old[0])
        self.block_key[:old[3]].copy_(old[1])
        self.header.copy_(old[2])
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().lvdgs_tsdf_blocks_rehash(C.byref(self._vol), _lib.raw_stream(self.device)), "lvdgs_tsdf_blocks_rehash")

    def to_dense(self):
        """A ``TsdfVolume`` over the bounding box of the blocks in use, filled with their samples.  The box starts at block
        min(0, lowest coordinate) per axis: while no block coordinate is negative the dense lattice IS this lattice -- the same origin,
        dense index = global index --, otherwise its origin is ``origin + voxel_size * 8 * lowest``.  Raises when the box exceeds what
        a dense volume holds."""
        b = self.blocks().to(torch.int64)
        if b.shape[0] == 0:
            raise _lib.LvdgsError("TsdfBlockVolume.to_dense: the volume holds no block")
        lo = torch.clamp(b.min(0).values, max=0)
        hi = b.max(0).values
        lo_l, nb = lo.tolist(), (hi - lo + 1).tolist()
        dims = tuple(BLOCK_EDGE * n for n in nb)
        if dims[0] * dims[1] * dims[2] > _INT32_MAX:
            raise _lib.LvdgsError(f"TsdfBlockVolume.to_dense: the blocks span {dims} samples, more than a dense volume holds")
        origin = tuple(o + self.voxel_size * BLOCK_EDGE * l for o, l in zip(self.origin, lo_l))
        dense = TsdfVolume(origin, self.voxel_size, dims, trunc=self.trunc, max_weight=self.max_weight, color=self.color, device=self.device)
        at = b - lo
        for name in _PLANES[:5 if self.color else 2]:
            grid = dense.plane(name).view(nb[2], BLOCK_EDGE, nb[1], BLOCK_EDGE, nb[0], BLOCK_EDGE).permute(0, 2, 4, 1, 3, 5)
            grid[at[:, 2], at[:, 1], at[:, 0]] = self.block_planes(name)
        dense.frames = self.frames
        dense.index_offset = tuple(BLOCK_EDGE * l for l in lo_l)
        return dense

    # ---- extraction ------------------------------------------------------------------------------
    def _mesh_once(self, vcap, fcap, cell_range=None):
        dev = self.device
        lo, hi = ((-2 ** 31,) * 3, (_INT32_MAX,) * 3) if cell_range is None else cell_range
        L = _lib.lib()
        block, scratch = _mesh_call.resources(dev, _lib.TSDF_BLOCKS_HOST_BYTES, L.lvdgs_tsdf_blocks_mesh_scratch_bytes(self.pool_blocks))
        order = self._order().to(torch.int32)
        vertices, colors, faces = out = self._mesh_buffers(vcap, fcap)
        a = _lib.TsdfBlocksMeshArgs(vol=self._vol, vertex_capacity=vcap, face_capacity=fcap, cell_lo=(C.c_int32 * 3)(*[int(v) for v in lo]),
                                    cell_hi=(C.c_int32 * 3)(*[int(v) for v in hi]), order=order.data_ptr(), vertices=vertices.data_ptr(),
                                    colors=None if colors is None else colors.data_ptr(), faces=faces.data_ptr(), host_state=block.data_ptr(),
                                    scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        w = _mesh_call.run(dev, a).copy()      # the one wait of the call
        self.last_stats = dict(blocks=int(w[_lib.TSDF_BLOCKS_USED]), dropped=int(w[_lib.TSDF_BLOCKS_DROPPED]),
                               out_of_range=int(w[_lib.TSDF_BLOCKS_OUT_OF_RANGE]) & 0xFFFFFFFF,
                               table_full=bool(int(w[_lib.TSDF_BLOCKS_FLAGS]) & _lib.TSDF_BLOCKS_TABLE_FULL))
        return out, int(w[_lib.TSDF_BLOCKS_N_VERTICES]), int(w[_lib.TSDF_BLOCKS_N_FACES]), int(w[_lib.TSDF_BLOCKS_OVERFLOW])

    def extract_mesh(self, vertex_capacity=None, face_capacity=None, cell_range=None) -> Mesh:
        """The surface-nets mesh of the volume as it stands, vertices in (key, l) order.  The capacities default to the last
        extraction's counts with headroom (the first time: a sheet across every block of the pool); a call that overflows them is
        repeated once with the exact counts.  ``last_stats`` holds the header as the call saw it.  ``cell_range`` = (lo, hi): only cells
        whose low corner's global index lies in lo <= g < hi per axis -- ((0, 0, 0), (nx - 1, ny - 1, nz - 1)) gives the mesh of a dense
        volume of (nx, ny, nz) samples on this lattice."""
        return self._extract(min(self.pool_blocks * 96, _INT32_MAX // 4), self.pool_blocks * BLOCK_SAMPLES, vertex_capacity, face_capacity, cell_range)
