"""A mesh scored against ground-truth geometry on the device: area-weighted samples of both surfaces and the exact nearest neighbour
of every sample in the other cloud (HIP, ``csrc/mesh_eval.hip``; the rules: ``include/lvdgs.h``, "Mesh scoring").

``sample_mesh``    ``lvdgs_mesh_sample``: ``n`` points as a function of (mesh, seed, sample index); no generator state, no wait.
``nearest``        ``lvdgs_cloud_distance``: ``d2``, ``idx`` and one row of sums and counts in a device table; no wait, no copy.
``score``          both samplings, both directed searches and ONE read of the table (one ``Stream.synchronize``): accuracy, completion,
                   completion ratio, precision, recall, F-score, chamfer -- NICE-SLAM's ``eval_recon`` protocol.
``load_mesh_ply``  what ``tsdf.save_mesh_ply`` wrote.
``visibility``     ``lvdgs_mesh_visibility``: the vertices that some view sees -- inside a frustum and, where the view has a depth plane, not
                   behind what it shows --, 16 views per call into one byte plane; no wait.
``cull_mesh``      ``lvdgs_mesh_cull``: the part of a mesh whose faces' vertices were seen, in the original order (HIP,
                   ``csrc/mesh_cull.hip``); ONE wait, for the two counts.  ``occlusion="self"``: the views' depth
                   planes are first rendered from the mesh itself.
``render_depth``   ``lvdgs_mesh_depth``: per view the depth plane -- and the face-index plane -- a rasteriser with a depth buffer gives of a
                   mesh (HIP, ``csrc/mesh_depth.hip``), 16 views per call; no wait.
``depth_l1_terms`` the sum and the count of one frame's "Depth L1" between two rendered planes, as torch statements.

What trimesh's ``sample_surface`` and a SciPy KD-tree do on the host after a copy of both meshes.  There is no CPU path: tensors that
are not on a GPU raise ``LvdgsError``.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .tsdf import Mesh, view_block

_INT32_MAX = 2 ** 31 - 1
_sample_scratch = _lib.DeviceScratch()
_distance_scratch = _lib.DeviceScratch()
_ROW, _INFO = _lib.CLOUD_DISTANCE_ROW_BYTES, _lib.MESH_SAMPLE_INFO_BYTES
_score_tables = {}      # device index -> the Table of ``score``
_cull_call = _lib.HostCall("lvdgs_mesh_cull", tag=_lib.MESH_CULL_SEQ)
_depth_scratch = _lib.DeviceScratch()
FACE_RULES = {"all": _lib.MESH_CULL_ALL, "any": _lib.MESH_CULL_ANY}


def _cuda_device(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.LvdgsError(f"{what} must be a tensor on a GPU (there is no CPU path)")
    return t.device


def _points(t, what, device=None):
    """``t`` as a contiguous (P, 3) float32 tensor on its GPU."""
    dev = _cuda_device(t, what)
    if device is not None and dev != device:
        raise _lib.LvdgsError(f"{what} is on {dev}, expected {device}")
    if t.ndim != 2 or t.shape[1] != 3:
        raise _lib.LvdgsError(f"{what} must have the shape (P, 3), not {tuple(t.shape)}")
    if t.shape[0] > _INT32_MAX:
        raise _lib.LvdgsError(f"{what}: more than 2^31 - 1 rows")
    return _lib.f32(t, dev)


def _mesh_parts(mesh):
    """(vertices (V, 3) float32, faces (F, 3) int32, colours (V, 3) float32 or None) of a ``tsdf.Mesh`` or a (vertices, faces) pair."""
    if isinstance(mesh, Mesh):
        vertices, colors, faces = mesh
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        (vertices, faces), colors = mesh, None
    else:
        raise _lib.LvdgsError("a mesh is a tsdf.Mesh or a (vertices, faces) pair")
    vertices = _points(vertices, "mesh vertices")
    dev = vertices.device
    if not torch.is_tensor(faces) or faces.device != dev or faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise _lib.LvdgsError("mesh faces must be an (F, 3) integer tensor on the vertices' GPU")
    faces = faces.detach()
    if faces.dtype is not torch.int32 or not faces.is_contiguous():
        faces = faces.to(torch.int32).contiguous()
    if colors is not None:
        colors = _points(colors, "mesh colours", dev)
        if colors.shape[0] != vertices.shape[0]:
            raise _lib.LvdgsError("mesh colours must have one row per vertex")
    return vertices, faces, colors


class Table:
    """``rows`` cloud-distance rows followed by ``infos`` sampling info rows in ONE device buffer, and its one read."""

    def __init__(self, device, rows=1, infos=0):
        self.device, self.rows, self.infos = device, int(rows), int(infos)
        self.buffer = torch.zeros(self.rows * _ROW + self.infos * _INFO, dtype=torch.uint8, device=device)
        self.host = None      # pinned, made by the first read

    def row_ptr(self, i):
        assert 0 <= i < self.rows
        return C.c_void_p(self.buffer.data_ptr() + i * _ROW)

    def info_ptr(self, i):
        assert 0 <= i < self.infos
        return C.c_void_p(self.buffer.data_ptr() + self.rows * _ROW + i * _INFO)

    def read(self):
        """-> (the rows, the infos) as NumPy record arrays: one copy to pinned memory and THE one wait (``Stream.synchronize``)."""
        if self.host is None:
            self.host = torch.zeros(self.buffer.numel(), dtype=torch.uint8).pin_memory()
        self.host.copy_(self.buffer, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        raw = self.host.numpy()
        rows = raw[:self.rows * _ROW].view(_lib.CLOUD_DISTANCE_ROW_DTYPE).copy()
        infos = raw[self.rows * _ROW:].view(_lib.MESH_SAMPLE_INFO_DTYPE).copy()
        return rows, infos


def sample_raw(vertices, faces, n, seed, points, info_ptr, vertex_colors=None, colors=None, face_index=None):
    """One ``lvdgs_mesh_sample`` call into the caller's tensors; ``info_ptr``: a device address (``Table.info_ptr``).  No wait."""
    dev = vertices.device
    L = _lib.lib()
    need = int(L.lvdgs_mesh_sample_scratch_bytes(int(faces.shape[0])))
    scratch = _sample_scratch.get(dev, need)
    a = _lib.MeshSampleArgs(num_vertices=int(vertices.shape[0]), num_faces=int(faces.shape[0]), num_samples=int(n),
                            seed=int(seed) & (2 ** 64 - 1), vertices=vertices.data_ptr(), faces=faces.data_ptr(),
                            vertex_colors=None if vertex_colors is None else vertex_colors.data_ptr(), points=points.data_ptr(),
                            face_index=None if face_index is None else face_index.data_ptr(),
                            colors=None if colors is None else colors.data_ptr(), info=info_ptr,
                            scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    with _lib.on_device(dev):
        _lib.check(L.lvdgs_mesh_sample(C.byref(a), _lib.raw_stream(dev)), "lvdgs_mesh_sample")


def _sample(mesh, n, seed, info_ptr, want_colors=True):
    vertices, faces, vcolors = _mesh_parts(mesh)
    n = int(n)
    if n < 0 or n > _INT32_MAX:
        raise _lib.LvdgsError(f"sample_mesh: n = {n} is outside 0 .. 2^31 - 1")
    if faces.shape[0] == 0:
        raise _lib.LvdgsError("sample_mesh: the mesh has no faces")
    dev = vertices.device
    # NaN rows: a mesh without area leaves them, and the search skips them
    points = torch.full((n, 3), math.nan, dtype=torch.float32, device=dev)
    colors = torch.full((n, 3), math.nan, dtype=torch.float32, device=dev) if (vcolors is not None and want_colors) else None
    sample_raw(vertices, faces, n, seed, points, info_ptr, vertex_colors=vcolors if colors is not None else None, colors=colors)
    return points, colors


def sample_mesh(mesh, n, seed=0):
    """``n`` area-weighted samples of ``mesh`` (a ``tsdf.Mesh`` or a (vertices, faces) pair on a GPU): (n, 3) float32 points, and for a
    mesh with vertex colours ``(points, colors)``.  The same bytes for the same (mesh, seed); no wait.  A mesh without any area
    leaves every row NaN."""
    vertices = mesh[0]
    table = Table(_cuda_device(vertices, "mesh vertices"), rows=0, infos=1)
    points, colors = _sample(mesh, n, seed, table.info_ptr(0))
    return points if colors is None else (points, colors)


def nearest(query, reference, thresholds=(), points_per_cell=0, want_d2=True, want_idx=True, table=None, row=0):
    """For every row of ``query`` (M, 3) the nearest row of ``reference`` (N, 3): -> (``d2`` (M,) float32, ``idx`` (M,) int32, the
    ``Table`` whose row ``row`` the call fills -- ``table.read()`` is the wait).  ``thresholds``: up to four distances whose counts
    the row reports.  ``want_d2`` / ``want_idx`` False: None in their place, only the row is written."""
    query = _points(query, "nearest: query")
    dev = query.device
    reference = _points(reference, "nearest: reference", dev)
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > _lib.CLOUD_DISTANCE_MAX_THRESHOLDS:
        raise _lib.LvdgsError(f"nearest: at most {_lib.CLOUD_DISTANCE_MAX_THRESHOLDS} thresholds")
    M, N = int(query.shape[0]), int(reference.shape[0])
    L = _lib.lib()
    scratch = _distance_scratch.get(dev, int(L.lvdgs_cloud_distance_scratch_bytes(M, N)))
    table = Table(dev, rows=row + 1) if table is None else table
    d2 = torch.empty(M, dtype=torch.float32, device=dev) if want_d2 else None
    idx = torch.empty(M, dtype=torch.int32, device=dev) if want_idx else None
    a = _lib.CloudDistanceArgs(num_queries=M, num_reference=N, queries=query.data_ptr(), reference=reference.data_ptr() if N else None,
                               num_thresholds=len(thresholds), points_per_cell=int(points_per_cell),
                               thresholds=(C.c_float * _lib.CLOUD_DISTANCE_MAX_THRESHOLDS)(*thresholds),
                               d2=None if d2 is None else d2.data_ptr(), idx=None if idx is None else idx.data_ptr(),
                               out_row=table.row_ptr(row), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    with _lib.on_device(dev):
        _lib.check(L.lvdgs_cloud_distance(C.byref(a), _lib.raw_stream(dev)), "lvdgs_cloud_distance")
    return d2, idx, table


def _ratio(a, b):
    return float(a) / float(b) if b else math.nan


def score_from_rows(est_to_gt, gt_to_est, threshold=None):
    """The score's numbers from the two rows (records of ``CLOUD_DISTANCE_ROW_DTYPE``; ``n_below[0]`` counts the threshold).  A
    direction in which nothing was counted gives NaN, not an exception."""
    ne, ng = int(est_to_gt["n_counted"]), int(gt_to_est["n_counted"])
    accuracy = _ratio(est_to_gt["sum_distance"], ne)
    completion = _ratio(gt_to_est["sum_distance"], ng)
    precision = _ratio(int(est_to_gt["n_below"][0]), ne)
    recall = _ratio(int(gt_to_est["n_below"][0]), ng)
    both = precision + recall
    fscore = 2.0 * precision * recall / both if both > 0 else (math.nan if math.isnan(both) else 0.0)
    return dict(accuracy=accuracy, completion=completion, completion_ratio=recall, precision=precision, recall=recall, fscore=fscore,
                chamfer=0.5 * (accuracy + completion), n_est=ne, n_gt=ng,
                skipped_est=int(est_to_gt["n_skipped"]), skipped_gt=int(gt_to_est["n_skipped"]),
                flags_est=int(est_to_gt["flags"]), flags_gt=int(gt_to_est["flags"]),
                max_est=float(est_to_gt["max_distance"]), max_gt=float(gt_to_est["max_distance"]),
                threshold=None if threshold is None else float(threshold))


MeshScore = dict      # what ``score`` returns: the keys of ``score_from_rows``


def _is_cloud(x):
    return torch.is_tensor(x)


def score(est, gt, n_samples=200_000, threshold=0.05, seed=0, seed_gt=None, points_per_cell=0) -> MeshScore:
    """``est`` against ``gt``, each a mesh (sampled: ``n_samples`` points, seeds ``seed`` and ``seed_gt``, default ``seed + 1``) or a
    (P, 3) cloud (used as given).  accuracy: mean distance est -> gt; completion: gt -> est; completion_ratio = recall: the share of
    gt samples nearer than ``threshold``; precision: the share of est samples; fscore; chamfer: the mean of the two means.  One
    ``Stream.synchronize``, at the end, and no other wait."""
    first = est if _is_cloud(est) else est[0]
    dev = _cuda_device(first, "score: est")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    table = _score_tables.get(dev.index)
    if table is None:
        table = _score_tables[dev.index] = Table(dev, rows=2, infos=2)
    table.buffer.zero_()      # a cloud given as such leaves its info row alone
    seeds = (int(seed), int(seed) + 1 if seed_gt is None else int(seed_gt))
    clouds = []
    for slot, (what, seed_) in enumerate(zip((est, gt), seeds)):
        if _is_cloud(what):
            clouds.append(_points(what, "score: a cloud", dev))
        else:
            clouds.append(_sample(what, n_samples, seed_, table.info_ptr(slot), want_colors=False)[0])
        if clouds[-1].shape[0] == 0:
            raise _lib.LvdgsError("score: a cloud without points")
    nearest(clouds[0], clouds[1], (threshold,), points_per_cell, want_d2=False, want_idx=False, table=table, row=0)
    nearest(clouds[1], clouds[0], (threshold,), points_per_cell, want_d2=False, want_idx=False, table=table, row=1)
    rows, infos = table.read()
    for slot, name in enumerate(("est", "gt")):
        if int(infos[slot]["flags"]) & _lib.MESH_SAMPLE_NO_AREA:
            raise _lib.LvdgsError(f"score: the {name} mesh has no face with a positive area")
    return score_from_rows(rows[0], rows[1], threshold)


def visibility(vertices, views, occlusion_eps=0.0, seen=None):
    """Which of ``vertices`` (V, 3) some view sees -> ``seen``, (V,) uint8 on the vertices' GPU.  ``views``: the dicts that
    ``TsdfVolume.integrate_views`` takes -- ``depth`` (H, W), ``R``, ``T``, ``intrinsics``, ``mask``, ``depth_min``, ``depth_trunc``; an
    ``image`` is ignored.  A view with ``depth=None`` carries ``size=(H, W)`` and is frustum only: a vertex in front of ``depth_min``,
    inside the image and not beyond ``depth_trunc`` is seen.  With a depth plane the vertex must also not lie more than ``occlusion_eps``
    behind the pixel's depth, which must be positive, not beyond ``depth_trunc`` and unmasked.  ``seen``: a plane to accumulate into (it
    is written in place; bytes that are set stay set); default: a zeroed one.  16 views per library call, no wait."""
    vertices = _points(vertices, "visibility: vertices")
    dev = vertices.device
    V = int(vertices.shape[0])
    if seen is None:
        seen = torch.zeros(V, dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(seen) or seen.device != dev or seen.dtype is not torch.uint8 or tuple(seen.shape) != (V,) or not seen.is_contiguous():
        raise _lib.LvdgsError("visibility: seen must be a contiguous (V,) uint8 tensor on the vertices' GPU")
    blocks = []
    for v in views:
        v = {k: x for k, x in v.items() if k != "image"}
        depth, size = v.pop("depth", None), v.pop("size", None)
        if depth is None and size is None:
            raise _lib.LvdgsError("visibility: a view without a depth plane needs size=(H, W)")
        blocks.append(view_block("visibility", dev, False, depth, size=size, **v))
    L = _lib.lib()
    stream = _lib.raw_stream(dev)
    with _lib.on_device(dev):
        for first in range(0, len(blocks), _lib.TSDF_MAX_VIEWS):
            chunk = blocks[first:first + _lib.TSDF_MAX_VIEWS]
            ptrs = (C.POINTER(_lib.TsdfViewArgs) * len(chunk))(*[C.pointer(a) for a, _ in chunk])
            a = _lib.MeshVisibilityArgs(num_vertices=V, vertices=vertices.data_ptr(), views=C.cast(ptrs, C.c_void_p), count=len(chunk),
                                        occlusion_eps=float(occlusion_eps), seen=seen.data_ptr())
            _lib.check(L.lvdgs_mesh_visibility(C.byref(a), stream), "lvdgs_mesh_visibility")
    return seen


def cull_raw(vertices, faces, seen, face_rule, out_vertices, out_faces, vertex_colors=None, out_colors=None, vertex_origin=None, face_origin=None):
    """One ``lvdgs_mesh_cull`` call into the caller's tensors and its one wait -> (kept vertices, kept faces).  Rows beyond the counts
    are not touched."""
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    L = _lib.lib()
    block, scratch = _cull_call.resources(dev, _lib.MESH_CULL_HOST_BYTES, L.lvdgs_mesh_cull_scratch_bytes(V, F))
    a = _lib.MeshCullArgs(num_vertices=V, num_faces=F, vertices=_lib.ptr(vertices), vertex_colors=_lib.ptr(vertex_colors), faces=_lib.ptr(faces),
                          seen=_lib.ptr(seen), face_rule=int(face_rule), out_vertices=_lib.ptr(out_vertices), out_colors=_lib.ptr(out_colors),
                          out_faces=_lib.ptr(out_faces), vertex_origin=_lib.ptr(vertex_origin), face_origin=_lib.ptr(face_origin),
                          host_state=block.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    w = _cull_call.run(dev, a)      # the one wait of the call
    return int(w[_lib.MESH_CULL_N_VERTICES]), int(w[_lib.MESH_CULL_N_FACES])


def _size_of_view(v, what):
    size, depth = v.get("size"), v.get("depth")
    if size is None and torch.is_tensor(depth) and depth.ndim >= 2:
        size = depth.shape[-2:]
    if size is None:
        raise _lib.LvdgsError(f"{what}: a view needs size=(H, W)")
    return int(size[0]), int(size[1])


def render_depth(mesh, views, want_faces=False):
    """``mesh`` (a ``tsdf.Mesh`` or a (vertices, faces) pair on a GPU) seen from ``views`` -> a list of (H, W) float32 depth planes on the
    mesh's GPU: per pixel the camera z of the nearest face that covers the pixel's centre, 0 where none does.  ``want_faces``: ->
    (the depth planes, the (H, W) int32 planes of the winning faces' indices, -1 where none).  ``views``: the dicts ``visibility`` takes
    -- ``R``, ``T``, ``intrinsics``, ``depth_min``, ``depth_trunc`` and ``size=(H, W)``, which is required unless the view carries a depth
    plane of that size; ``depth``, ``image`` and ``mask`` are ignored.  Both windings of a face cover, edges are inclusive, a face with a
    vertex at or in front of ``depth_min`` is dropped whole (include/lvdgs.h, "Mesh scoring").  16 views per library call, no wait."""
    vertices, faces, _ = _mesh_parts(mesh)
    dev = vertices.device
    blocks, sizes = [], []
    for v in views:
        size = _size_of_view(v, "render_depth")
        v = {k: x for k, x in v.items() if k not in ("image", "depth", "mask", "size")}
        blocks.append(view_block("render_depth", dev, False, None, size=size, **v))
        sizes.append(size)
    depth = [torch.empty(size, dtype=torch.float32, device=dev) for size in sizes]
    index = [torch.empty(size, dtype=torch.int32, device=dev) for size in sizes] if want_faces else None
    L = _lib.lib()
    stream = _lib.raw_stream(dev)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    with _lib.on_device(dev):
        for first in range(0, len(blocks), _lib.TSDF_MAX_VIEWS):
            chunk = blocks[first:first + _lib.TSDF_MAX_VIEWS]
            n = len(chunk)
            ptrs = (C.POINTER(_lib.TsdfViewArgs) * n)(*[C.pointer(a) for a, _ in chunk])
            planes = (C.c_void_p * n)(*[d.data_ptr() for d in depth[first:first + n]])
            indices = (C.c_void_p * n)(*[d.data_ptr() for d in index[first:first + n]]) if want_faces else None
            scratch = _depth_scratch.get(dev, L.lvdgs_mesh_depth_scratch_bytes(sum(h * w for h, w in sizes[first:first + n])))
            a = _lib.MeshDepthArgs(num_vertices=V, num_faces=F, vertices=vertices.data_ptr() if V else None, faces=faces.data_ptr() if F else None,
                                   views=C.cast(ptrs, C.c_void_p), count=n, depth=C.cast(planes, C.c_void_p),
                                   face_index=None if indices is None else C.cast(indices, C.c_void_p),
                                   scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
            _lib.check(L.lvdgs_mesh_depth(C.byref(a), stream), "lvdgs_mesh_depth")
    return (depth, index) if want_faces else depth


def depth_l1_terms(d_est, d_gt, depth_trunc=None):
    """One frame's terms of the "Depth L1" between two depth planes of one size, as torch statements on the planes' device -> (the sum of
    ``|d_est - d_gt|`` in float64, the number of pixels, int64) over the pixels where both are ``> 0`` and, with ``depth_trunc``, not beyond
    it.  No wait."""
    both = (d_est > 0) & (d_gt > 0)
    if depth_trunc is not None:
        both = both & (d_est <= float(depth_trunc)) & (d_gt <= float(depth_trunc))
    diff = (d_est.to(torch.float64) - d_gt.to(torch.float64)).abs()
    return torch.where(both, diff, torch.zeros_like(diff)).sum(), both.sum()


def cull_mesh(mesh, views=None, seen=None, occlusion_eps=0.0, face_rule="all", want_origin=False, occlusion=None):
    """``mesh`` (a ``tsdf.Mesh`` or a (vertices, faces) pair on a GPU) without the faces that were not seen -> (a ``tsdf.Mesh`` on the
    device, a record).  ``views``: what ``visibility`` takes, with ``occlusion_eps``; ``seen``: a (V,) uint8 plane to start from, or
    the whole decision when there are no views.  ``face_rule``: "all" -- a face stays when its three vertices are seen -- or "any".  A
    vertex stays exactly when a kept face references it; vertices and faces keep their order.  An empty result is a mesh with zero
    faces.  The record: vertices_before, faces_before, vertices, faces, and with ``want_origin`` vertex_origin and face_origin, the
    old index of each kept row (int32, on the device).  ``occlusion="self"``: every view's depth plane is replaced by the depth rendered
    from the mesh itself (``render_depth``; a view needs no plane of its own, ``size`` is enough), so a vertex more than ``occlusion_eps``
    behind the mesh's first surface in a view is not seen by it.  ONE wait."""
    vertices, faces, colors = _mesh_parts(mesh)
    if face_rule not in FACE_RULES:
        raise _lib.LvdgsError(f"cull_mesh: face_rule 'all' or 'any', not {face_rule!r}")
    if occlusion not in (None, "self"):
        raise _lib.LvdgsError(f"cull_mesh: occlusion None or 'self', not {occlusion!r}")
    if views is None and seen is None:
        raise _lib.LvdgsError("cull_mesh: give the views, a seen plane, or both")
    if occlusion is not None and views is None:
        raise _lib.LvdgsError("cull_mesh: occlusion='self' needs the views")
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if occlusion is not None:
        views = list(views)
        planes = render_depth((vertices, faces), views)
        views = [dict({k: x for k, x in v.items() if k not in ("size", "image")}, depth=plane) for v, plane in zip(views, planes)]
    if views is not None:
        seen = visibility(vertices, views, occlusion_eps, seen=seen)
    elif not torch.is_tensor(seen) or seen.device != dev or seen.dtype is not torch.uint8 or tuple(seen.shape) != (V,) or not seen.is_contiguous():
        raise _lib.LvdgsError("cull_mesh: seen must be a contiguous (V,) uint8 tensor on the mesh's GPU")
    out_vertices = torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev)
    out_colors = None if colors is None else torch.empty((max(V, 1), 3), dtype=torch.float32, device=dev)
    out_faces = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)
    vertex_origin = torch.empty(max(V, 1), dtype=torch.int32, device=dev) if want_origin else None
    face_origin = torch.empty(max(F, 1), dtype=torch.int32, device=dev) if want_origin else None
    nv, nf = cull_raw(vertices, faces, seen, FACE_RULES[face_rule], out_vertices, out_faces, vertex_colors=colors, out_colors=out_colors,
                      vertex_origin=vertex_origin, face_origin=face_origin)
    record = dict(vertices_before=V, faces_before=F, vertices=nv, faces=nf)
    if want_origin:
        record.update(vertex_origin=vertex_origin[:nv], face_origin=face_origin[:nf])
    return Mesh(out_vertices[:nv], None if out_colors is None else out_colors[:nv], out_faces[:nf]), record


def load_mesh_ply(path, device="cuda") -> Mesh:
    """The binary little-endian PLY that ``tsdf.save_mesh_ply`` writes, as a ``tsdf.Mesh`` on ``device``: vertices float32, colours (the
    file's bytes / 255) or None, faces int32."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise _lib.LvdgsError(f"{path}: not a PLY file")
    header = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if "format binary_little_endian 1.0" not in header:
        raise _lib.LvdgsError(f"{path}: only binary little-endian PLY is read")
    counts, props, element = {}, {}, None
    for line in header:
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            counts[element], props[element] = int(w[2]), []
        elif w[:1] == ["property"] and element is not None:
            props[element].append(w[1:])
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    try:
        vdt = np.dtype([(p[-1], kinds[p[0]]) for p in props["vertex"]])
        face_ok = props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    except KeyError as e:
        raise _lib.LvdgsError(f"{path}: an element or property type save_mesh_ply does not write ({e})") from None
    if not face_ok or not {"x", "y", "z"} <= set(vdt.names):
        raise _lib.LvdgsError(f"{path}: not the layout save_mesh_ply writes")
    nv, nf = counts["vertex"], counts["face"]
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(body) < nv * vdt.itemsize + nf * fdt.itemsize:
        raise _lib.LvdgsError(f"{path}: the file is shorter than its header says")
    v = np.frombuffer(body, dtype=vdt, count=nv)
    f = np.frombuffer(body, dtype=fdt, count=nf, offset=nv * vdt.itemsize)
    if nf and not (f["n"] == 3).all():
        raise _lib.LvdgsError(f"{path}: a face that is no triangle")
    vertices = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32)
    colors = None
    if {"red", "green", "blue"} <= set(vdt.names):
        colors = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.float32) / np.float32(255)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return Mesh(to(vertices), None if colors is None else to(colors), to(f["i"].astype(np.int32).reshape(-1, 3)))
