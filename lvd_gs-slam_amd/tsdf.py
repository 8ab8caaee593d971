"""A dense TSDF volume on the device: fusion of depth maps and a mesh of the result by surface nets (HIP, ``csrc/tsdf.hip``; the rules:
``include/lvdgs.h``, "TSDF fusion").

``TsdfVolume.integrate*``  ``lvdgs_tsdf_integrate``: up to 16 views per call, the planes read and written once per call; no wait, no copy.
``TsdfVolume.extract_mesh`` ``lvdgs_tsdf_mesh``: vertices, colours and faces on the device; ONE wait, a second only when the capacities
                           guessed for the first call were too small (the call reports the exact counts either way).
``save_mesh_ply``          the mesh as a binary little-endian PLY.

What an Open3D-style host fusion does after copying every depth map and image to the host.  There is no CPU path: tensors that are
not on a GPU raise ``LvdgsError``.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

Mesh = namedtuple("Mesh", "vertices colors faces")      # (V, 3) float32, (V, 3) float32 or None, (F, 3) int32 -- on the device
_mesh_call = _lib.HostCall("lvdgs_tsdf_mesh", tag=_lib.TSDF_SEQ)
_INT32_MAX = 2 ** 31 - 1


def view_block(name, dev, color, depth, R, T, intrinsics, image=None, mask=None, depth_min=0.0, depth_trunc=math.inf, size=None):
    """One view's argument block (``lvdgs_tsdf_view``) and the tensors it points into, for the call ``name`` on the GPU ``dev``.
    ``color``: an image is acceptable.  ``size``: None -- a depth plane is required --, or the (height, width) of a view that may come
    without one (``depth=None``: the view is frustum only, ``mesh_eval.visibility``)."""
    if torch.is_tensor(depth) and depth.ndim == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth is None and size is not None:
        H, W = (int(v) for v in size)
    else:
        if not _lib.is_f32(depth, dev) or depth.ndim != 2:
            raise _lib.LvdgsError(f"{name}: depth must be a contiguous (H, W) float32 tensor on the volume's GPU (there is no CPU path)")
        H, W = depth.shape
        if size is not None and (int(size[0]), int(size[1])) != (H, W):
            raise _lib.LvdgsError(f"{name}: the view's size {tuple(size)} is not its depth plane's {(H, W)}")
    if image is not None:
        if not color:
            raise _lib.LvdgsError(f"{name}: an image on a volume made with color=False")
        if not _lib.is_f32(image, dev) or tuple(image.shape) != (3, H, W):
            raise _lib.LvdgsError(f"{name}: image must be a contiguous (3, H, W) float32 tensor of the depth's size on its device")
    if mask is not None:
        if not torch.is_tensor(mask) or mask.device != dev:
            raise _lib.LvdgsError(f"{name}: mask must be a tensor on the volume's GPU")
        mask = mask.reshape(-1) if mask.numel() == H * W else mask
        if mask.numel() != H * W:
            raise _lib.LvdgsError(f"{name}: mask must have the depth's H * W elements")
        mask = (mask if mask.dtype in (torch.uint8, torch.bool) else mask != 0).contiguous()
        mask = mask.view(torch.uint8) if mask.dtype is torch.bool else mask
    for what, t in (("R", R), ("T", T)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.LvdgsError(f"{name}: {what} must be a tensor on the volume's GPU")
    R, T = _lib.f32(R, dev), _lib.f32(T, dev)
    if R.numel() != 9 or T.numel() != 3:
        raise _lib.LvdgsError(f"{name}: R must be (3, 3) and T (3,)")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    a = _lib.TsdfViewArgs(width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy, depth_min=float(depth_min), depth_trunc=float(depth_trunc),
                          R=R.data_ptr(), T=T.data_ptr(), depth=None if depth is None else depth.data_ptr(),
                          image=None if image is None else image.data_ptr(), mask=None if mask is None else mask.data_ptr())
    return a, (depth, R, T, image, mask)


class _TsdfBase:
    """What the dense and the block-sparse volume share: the lattice and the constants of the rule, a view's argument block, the fusion
    calls, and the capacities of a mesh call with their one retry.  A volume supplies ``_vol`` (its argument struct), ``_integrate``
    (the library entry's name), ``_mesh_once(vcap, fcap, *extra)`` and the first capacity guess of its ``extract_mesh``."""

    def __init__(self, origin, voxel_size, trunc, max_weight, color, device):
        self._name = type(self).__name__
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LvdgsError(f"{self._name}: the volume lives on a GPU (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        self.voxel_size_requested = self.voxel_size      # from_bounds: what the caller asked for, when the volume had to be coarser
        self.color = bool(color)
        self.frames = 0
        self._capacity = None      # (vertices, faces) of the last extraction, with headroom

    # ---- fusion ----------------------------------------------------------------------------------
    def _view(self, depth, R, T, intrinsics, image=None, mask=None, depth_min=0.0, depth_trunc=math.inf):
        """One view's argument block and the tensors it points into."""
        return view_block(f"{self._name}.integrate", self.device, self.color, depth, R, T, intrinsics, image=image, mask=mask,
                          depth_min=depth_min, depth_trunc=depth_trunc)

    def integrate_views(self, views):
        """``views``: dicts of ``integrate``'s arguments, fused in list order, 16 per library call.  No wait."""
        blocks = [self._view(**v) for v in views]
        L = _lib.lib()
        stream = _lib.raw_stream(self.device)
        with _lib.on_device(self.device):
            for first in range(0, len(blocks), _lib.TSDF_MAX_VIEWS):
                chunk = blocks[first:first + _lib.TSDF_MAX_VIEWS]
                ptrs = (C.POINTER(_lib.TsdfViewArgs) * len(chunk))(*[C.pointer(a) for a, _ in chunk])
                _lib.check(getattr(L, self._integrate)(C.byref(self._vol), ptrs, len(chunk), stream), self._integrate)
        self.frames += len(blocks)

    def integrate(self, depth, R, T, intrinsics, image=None, mask=None, depth_min=0.0, depth_trunc=math.inf):
        """Fuse one view: ``depth`` (H, W), ``R`` (3, 3), ``T`` (3,) with ``p_cam = R p_world + T``, ``intrinsics`` (fx, fy, cx, cy),
        ``image`` (3, H, W) or None, ``mask`` (H, W) non-zero = use, or None."""
        self.integrate_views([dict(depth=depth, R=R, T=T, intrinsics=intrinsics, image=image, mask=mask, depth_min=depth_min,
                                   depth_trunc=depth_trunc)])

    def integrate_camera(self, viewpoint, depth, image=None, mask=None, depth_min=0.0, depth_trunc=math.inf):
        """``integrate`` with ``R``, ``T`` and the intrinsics of a ``camera_utils.Camera``."""
        self.integrate(depth, viewpoint.R, viewpoint.T, (viewpoint.fx, viewpoint.fy, viewpoint.cx, viewpoint.cy), image=image, mask=mask,
                       depth_min=depth_min, depth_trunc=depth_trunc)

    # ---- extraction ------------------------------------------------------------------------------
    def _mesh_buffers(self, vcap, fcap):
        """The outputs of one mesh call: vertices, colours (None without colour planes) and faces, at least one row each."""
        dev = self.device
        vertices = torch.empty((max(vcap, 1), 3), dtype=torch.float32, device=dev)
        colors = torch.empty((max(vcap, 1), 3), dtype=torch.float32, device=dev) if self.color else None
        faces = torch.empty((max(fcap, 1), 3), dtype=torch.int32, device=dev)
        return vertices, colors, faces

    def _extract(self, first, most_vertices, vertex_capacity, face_capacity, *extra):
        """``extract_mesh``: the capacities default to the last extraction's counts with headroom (the first time: ``first``), the
        vertices' to at most ``most_vertices``; a call that overflows them is repeated once with the exact counts.  ``extra``: what
        ``_mesh_once`` takes after the capacities."""
        guess = self._capacity or (first,) * 2
        vcap = min(most_vertices, guess[0]) if vertex_capacity is None else int(vertex_capacity)
        fcap = min(_INT32_MAX, 2 * guess[1]) if face_capacity is None else int(face_capacity)
        out, nv, nf, overflow = self._mesh_once(vcap, fcap, *extra)
        if overflow & _lib.TSDF_OVERFLOW_INT32:
            raise _lib.LvdgsError(f"{self._name}.extract_mesh: more than 2^31 - 1 faces")
        if overflow:
            out, nv, nf, overflow = self._mesh_once(nv, nf, *extra)
            if overflow:
                raise _lib.LvdgsError(f"{self._name}.extract_mesh: the retry with the exact counts overflowed ({overflow})")
        self._capacity = (nv + nv // 4 + 64, nf // 2 + nf // 8 + 64)
        self.last_counts = (nv, nf)
        vertices, colors, faces = out
        return Mesh(vertices[:nv], None if colors is None else colors[:nv], faces[:nf])


class TsdfVolume(_TsdfBase):
    """``dims`` = (nx, ny, nz) samples at ``origin + voxel_size * (i, j, k)``; planes ``tsdf``, ``weight`` and, with ``color``, ``r``,
    ``g``, ``b``, each a flat float32 tensor indexed ``i + nx * (j + ny * k)`` (``plane(name)`` gives the (nz, ny, nx) view)."""
    _integrate = "lvdgs_tsdf_integrate"

    def __init__(self, origin, voxel_size, dims, trunc=None, max_weight=64.0, color=True, device="cuda"):
        super().__init__(origin, voxel_size, trunc, max_weight, color, device)
        self.dims = tuple(int(v) for v in dims)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise _lib.LvdgsError("TsdfVolume: origin and dims have three entries")
        n = self.dims[0] * self.dims[1] * self.dims[2]
        if min(self.dims) < 1 or n > _INT32_MAX:
            raise _lib.LvdgsError(f"TsdfVolume: dims {self.dims}: every dimension at least 1, at most 2^31 - 1 samples")
        names = ("tsdf", "weight") + (("r", "g", "b") if color else ())
        self.planes = torch.zeros((len(names), n), dtype=torch.float32, device=self.device)      # one zeroed block: an empty volume
        for row, name in enumerate(names):
            setattr(self, name, self.planes[row])
        self._vol = _lib.TsdfVolumeArgs(nx=self.dims[0], ny=self.dims[1], nz=self.dims[2], origin=(C.c_float * 3)(*self.origin),
                                        voxel_size=self.voxel_size, trunc=self.trunc, max_weight=self.max_weight,
                                        tsdf=self.tsdf.data_ptr(), weight=self.weight.data_ptr(),
                                        r=self.r.data_ptr() if color else None, g=self.g.data_ptr() if color else None,
                                        b=self.b.data_ptr() if color else None)

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, max_voxels=1 << 28, **kw):
        """The volume that covers the box ``lo .. hi``; a ``voxel_size`` that would need more than ``max_voxels`` samples is raised
        until it fits (``voxel_size_requested`` keeps what was asked for)."""
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
        asked = size = float(voxel_size)
        if not (size > 0 and math.isfinite(size)) or any(not (b >= a) for a, b in zip(lo, hi)):
            raise _lib.LvdgsError("TsdfVolume.from_bounds: voxel_size must be positive and hi >= lo")
        max_voxels = min(int(max_voxels), _INT32_MAX)
        dims_of = lambda s: tuple(max(int(math.ceil((b - a) / s)) + 1, 2) for a, b in zip(lo, hi))
        while dims_of(size)[0] * dims_of(size)[1] * dims_of(size)[2] > max_voxels:
            size *= 1.05
        vol = cls(lo, size, dims_of(size), **kw)
        vol.voxel_size_requested = asked
        return vol

    def plane(self, name):
        return getattr(self, name).view(self.dims[2], self.dims[1], self.dims[0])

    def reset(self):
        self.planes.zero_()
        self.frames = 0

    # ---- extraction ------------------------------------------------------------------------------
    def _mesh_once(self, vcap, fcap):
        dev = self.device
        L = _lib.lib()
        block, scratch = _mesh_call.resources(dev, _lib.TSDF_HOST_BYTES, L.lvdgs_tsdf_mesh_scratch_bytes(*self.dims))
        vertices, colors, faces = out = self._mesh_buffers(vcap, fcap)
        a = _lib.TsdfMeshArgs(vol=self._vol, vertex_capacity=vcap, face_capacity=fcap, vertices=vertices.data_ptr(),
                              colors=None if colors is None else colors.data_ptr(), faces=faces.data_ptr(), host_state=block.data_ptr(),
                              scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        w = _mesh_call.run(dev, a).copy()      # the one wait of the call
        return out, int(w[_lib.TSDF_N_VERTICES]), int(w[_lib.TSDF_N_FACES]), int(w[_lib.TSDF_OVERFLOW])

    def extract_mesh(self, vertex_capacity=None, face_capacity=None) -> Mesh:
        """The surface-nets mesh of the volume as it stands.  The capacities default to the last extraction's counts with headroom
        (the first time: room for a few sheets across the volume); a call that overflows them is repeated once with the exact counts."""
        nx, ny, nz = self.dims
        if min(self.dims) < 2:
            raise _lib.LvdgsError(f"TsdfVolume.extract_mesh: dims {self.dims}: a mesh needs at least 2 samples along every axis")
        cells = (nx - 1) * (ny - 1) * (nz - 1)
        return self._extract(min(cells, 4 * (nx * ny + ny * nz + nz * nx)), cells, vertex_capacity, face_capacity)


def save_mesh_ply(path, mesh):
    """Binary little-endian PLY: per vertex ``x y z`` float32 and, with colours, ``red green blue`` as ``(uint8)(clamp(c, 0, 1) * 255)``;
    per face ``list uchar int vertex_indices``."""
    v = mesh.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if mesh.colors is not None:
        c = mesh.colors.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
        c8 = (np.clip(c, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(len(v), dtype=np.dtype(fields))
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if mesh.colors is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"], frec["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
