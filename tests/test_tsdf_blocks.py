"""The block-sparse TSDF volume without a GPU: the layouts of its two structs against a C probe, every refusal with its status, the
key packing, and the NumPy mirror (tests/tsdf_blocks_oracle.py) on a fronto-parallel plane and on the six-view sphere of the dense
tests: there the mesh of the allocated blocks must be the mesh of the dense rule on the same lattice, exactly.

Why it should be: the allocation band is the truncation band widened by one voxel and sampled every half voxel along each pixel's ray,
and a pixel's footprint at the surface is below half a voxel.  A corner sample of an active cell lies within two voxels of the
surface, three voxels inside the band; the part of the band inside that sample's block therefore holds a ball of more than a voxel's
radius, and a ball of that size holds a ray sample.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refusal_recording
import tsdf_blocks_oracle as borc
import tsdf_cases as cases
import tsdf_oracle as orc
from lvdgs import _lib, tsdf_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096      # a non-NULL pointer value; every call below is refused before a launch, so it is never dereferenced
_recorded = None      # of the refusal test that is running: files what _integrate and _mesh see (refusal_recording.Numbered)


# ---------------------------------------------------------------- the ABI ----
def test_struct_layouts_against_a_c_probe(tmp_path):
    structs = {"lvdgs_tsdf_blocks": _lib.TsdfBlocksArgs, "lvdgs_tsdf_blocks_mesh_args": _lib.TsdfBlocksMeshArgs}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} . %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0; }\n'
                   % (os.path.join(ROOT, "include", "lvdgs.h"), "\n".join(lines)))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "probe"), str(src)], check=True)
    seen = 0
    for line in subprocess.check_output([str(tmp_path / "probe")]).decode().splitlines():
        cname, field, value = line.split()
        cls = structs[cname]
        assert int(value) == (C.sizeof(cls) if field == "." else getattr(cls, field).offset), line
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in structs.values())
    assert _lib.TSDF_BLOCKS_HOST_BYTES >= 4 * (_lib.TSDF_BLOCKS_FLAGS + 1) and _lib.TSDF_BLOCKS_HEADER_WORDS > _lib.TSDF_BLOCKS_HEADER_FLAGS


def _volume(**kw):
    fields = dict(pool_blocks=8, table_slots=16, origin=(C.c_float * 3)(0, 0, 0), voxel_size=0.1, trunc=0.4, max_weight=64.0,
                  tsdf=FAKE, weight=FAKE, r=FAKE, g=FAKE, b=FAKE, block_key=FAKE, table_keys=FAKE, table_values=FAKE, header=FAKE)
    fields.update(kw)
    return _lib.TsdfBlocksArgs(**fields)


def _view(**kw):
    fields = dict(width=40, height=30, fx=40.0, fy=40.0, cx=20.0, cy=15.0, depth_min=0.0, depth_trunc=10.0, R=FAKE, T=FAKE, depth=FAKE)
    fields.update(kw)
    return _lib.TsdfViewArgs(**fields)


def _integrate(vol, views, count=None):
    L = _lib.lib()
    ptrs = (C.POINTER(_lib.TsdfViewArgs) * max(len(views), 1))(*[C.pointer(v) if v is not None else None for v in views])
    status = L.lvdgs_tsdf_blocks_integrate(None if vol is None else C.byref(vol), ptrs, len(views) if count is None else count, None)
    _recorded(status, L.lvdgs_last_error())
    return status, L.lvdgs_last_error().decode()


VOLUME_REFUSALS = [
    (dict(tsdf=None), _lib.E_INVALID, "tsdf / weight plane is NULL"),
    (dict(weight=None), _lib.E_INVALID, "tsdf / weight plane is NULL"),
    (dict(g=None), _lib.E_INVALID, "all set or all NULL"),
    (dict(block_key=None), _lib.E_INVALID, "header is NULL"),
    (dict(table_keys=None), _lib.E_INVALID, "header is NULL"),
    (dict(table_values=None), _lib.E_INVALID, "header is NULL"),
    (dict(header=None), _lib.E_INVALID, "header is NULL"),
    (dict(pool_blocks=0), _lib.E_RANGE, "pool_blocks 0 is outside"),
    (dict(pool_blocks=_lib.TSDF_BLOCKS_MAX_POOL + 1, table_slots=1 << 24), _lib.E_RANGE, "is outside 1 .."),
    (dict(table_slots=24), _lib.E_RANGE, "must be a power of two"),
    (dict(table_slots=8), _lib.E_RANGE, "at least 2 * pool_blocks"),
    (dict(table_slots=0), _lib.E_RANGE, "must be a power of two"),
] + [(dict(**{field: bad}), _lib.E_RANGE, "must be finite and positive")
     for field in ("voxel_size", "trunc", "max_weight") for bad in (0.0, -1.0, float("inf"), float("nan"))]


def test_integrate_refusals_without_gpu():
    global _recorded
    _recorded = refusal_recording.Numbered("test_tsdf_blocks::integrate")
    L = _lib.lib()
    ok = _view()
    assert _integrate(None, [ok]) == (_lib.E_INVALID, "tsdf blocks integrate: volume is NULL")
    assert L.lvdgs_tsdf_blocks_integrate(C.byref(_volume()), None, 0, None) == _lib.OK      # nothing to do
    assert L.lvdgs_tsdf_blocks_integrate(C.byref(_volume()), None, 1, None) == _lib.E_INVALID and b"view list is NULL" in L.lvdgs_last_error()
    for count in (-1, _lib.TSDF_MAX_VIEWS + 1):
        status, msg = _integrate(_volume(), [ok], count=count)
        assert status == _lib.E_INVALID and f"count {count} is outside 0 .. 16" in msg
    for kw, want, words in VOLUME_REFUSALS:
        status, msg = _integrate(_volume(**kw), [ok])
        assert status == want and words in msg, (kw, status, msg)
    status, msg = _integrate(_volume(trunc=100.0, voxel_size=0.1), [ok])
    assert status == _lib.E_RANGE and "steps along a ray" in msg
    status, msg = _integrate(_volume(), [ok, None])
    assert status == _lib.E_INVALID and "view 1 is NULL" in msg
    for kw in (dict(width=0), dict(height=0), dict(width=65536, height=32768)):
        status, msg = _integrate(_volume(), [ok, _view(**kw)])
        assert status == _lib.E_RANGE and "view 1: image size" in msg, kw
    for field in ("R", "T", "depth"):
        status, msg = _integrate(_volume(), [_view(**{field: None})])
        assert status == _lib.E_INVALID and "view 0: R / T / depth is NULL" in msg
    status, msg = _integrate(_volume(r=None, g=None, b=None), [_view(image=FAKE)])
    assert status == _lib.E_INVALID and "no colour planes" in msg


def _mesh_args(vol=None, **kw):
    fields = dict(vol=vol or _volume(), vertex_capacity=16, face_capacity=16, order=FAKE, vertices=FAKE, faces=FAKE, host_state=FAKE,
                  scratch=FAKE, scratch_bytes=1 << 30)
    fields.update(kw)
    return _lib.TsdfBlocksMeshArgs(**fields)


def _mesh(a):
    L = _lib.lib()
    status = L.lvdgs_tsdf_blocks_mesh(None if a is None else C.byref(a), None)
    _recorded(status, L.lvdgs_last_error())
    return status, L.lvdgs_last_error().decode()


def test_mesh_and_rehash_refusals_without_gpu():
    global _recorded
    _recorded = refusal_recording.Numbered("test_tsdf_blocks::mesh")
    L = _lib.lib()
    assert _mesh(None) == (_lib.E_INVALID, "tsdf blocks mesh: args is NULL")
    for kw, want, words in VOLUME_REFUSALS:
        status, msg = _mesh(_mesh_args(vol=_volume(**kw)))
        assert status == want and words in msg, (kw, status, msg)
        assert L.lvdgs_tsdf_blocks_rehash(C.byref(_volume(**kw)), None) == want and words.encode() in L.lvdgs_last_error()
        _recorded(want, L.lvdgs_last_error())
    assert L.lvdgs_tsdf_blocks_rehash(None, None) == _lib.E_INVALID
    for kw in (dict(vertex_capacity=-1), dict(face_capacity=-1)):
        status, msg = _mesh(_mesh_args(**kw))
        assert status == _lib.E_RANGE and "negative capacity" in msg
    for field in ("order", "vertices", "faces", "host_state", "scratch"):
        status, msg = _mesh(_mesh_args(**{field: None}))
        assert status == _lib.E_INVALID and "order / vertices / faces / host_state / scratch is NULL" in msg
    status, msg = _mesh(_mesh_args(vol=_volume(r=None, g=None, b=None), colors=FAKE))
    assert status == _lib.E_INVALID and "no colour planes" in msg
    need = L.lvdgs_tsdf_blocks_mesh_scratch_bytes(8)
    assert need > 8 * (512 + 64 + 108) and need % 256 == 0
    status, msg = _mesh(_mesh_args(scratch_bytes=need - 1))
    assert status == _lib.E_INVALID and "scratch too small" in msg
    status, msg = _mesh(_mesh_args(scratch=FAKE + 4))
    assert status == _lib.E_INVALID and "8-byte aligned" in msg
    assert L.lvdgs_tsdf_blocks_mesh_scratch_bytes(0) == 0 and L.lvdgs_tsdf_blocks_mesh_scratch_bytes(_lib.TSDF_BLOCKS_MAX_POOL + 1) == 0
    assert L.lvdgs_tsdf_blocks_mesh_scratch_bytes(1000) > L.lvdgs_tsdf_blocks_mesh_scratch_bytes(999) - 1


def test_python_refusals_without_gpu():
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        tsdf_blocks.TsdfBlockVolume((0, 0, 0), 0.1, 8, device="cpu")
    assert [tsdf_blocks.table_slots_for(n) for n in (1, 8, 9, 32, 33)] == [2, 16, 32, 64, 128]


# ---------------------------------------------------------------- the keys ----
def test_key_packing_round_trip_at_the_range_ends():
    lo, hi = -(1 << 20), (1 << 20) - 1
    corners = [(x, y, z) for x in (lo, -1, 0, hi) for y in (lo, -1, 0, hi) for z in (lo, -1, 0, hi)]
    keys = []
    for b in corners:
        key = tsdf_blocks.pack_key(*b)
        assert key == borc.pack_key(*b) and key >> 63 == 1 and key < 1 << 64 and key != 0
        assert tsdf_blocks.unpack_key(key) == b == borc.unpack_key(key)
        assert tsdf_blocks.unpack_key(key - (1 << 64)) == b      # as torch holds it: a negative int64
        keys.append(key)
    assert np.array_equal(borc.pack_keys(np.asarray(corners)), np.asarray(keys, np.uint64))
    assert np.array_equal(borc.unpack_keys(np.asarray(keys, np.uint64)), np.asarray(corners))
    by_key = [b for _, b in sorted(zip(keys, corners))]
    assert by_key == sorted(corners, key=lambda b: (b[2], b[1], b[0]))      # ascending key = ascending (bz, by, bx)
    assert tsdf_blocks.pack_key(lo, lo, lo) == 1 << 63 and tsdf_blocks.pack_key(hi, hi, hi) == (1 << 64) - 1
    for bad in (lo - 1, hi + 1):
        with pytest.raises(ValueError):
            tsdf_blocks.pack_key(0, bad, 0)


# ---------------------------------------------------------------- the mirror ----
def plane_scene():
    """tests/tsdf_cases.py's fronto-parallel plane (5 cm voxels, footprint 1.31 / 67 = 0.39 voxels) on a lattice whose origin puts
    every allocated block at a non-negative coordinate."""
    case = cases.plane_case()
    return dict(origin=np.array([-1.2, -0.8, -0.4], np.float32), voxel_size=0.05, views=case["views"], color=False)


FAR = 1.4      # the enclosing sphere of the mirror's sphere scene


def sphere_scene():
    """The dense tests' sphere from its six axis views at 4 m inside an enclosing sphere of radius 1.4 m, so that the free space around
    it is observed (the dense case's own enclosing sphere, 8 m, would allocate thousands of blocks).  A ray that misses the sphere ends
    on the far wall at up to 5.4 m: 144 x 144 pixels at f = 150 keep the footprint there at 0.36 voxels of 0.1 m."""
    S = cases.SPHERE
    c = np.asarray(S["centre"])
    views = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            cam = c.copy()
            cam[axis] += sign * S["distance"]
            cam += np.array([0.0137, -0.0091, 0.0113])
            views.append(cases.sphere_view(cam, c, S["radius"], (150.0, 150.0, 71.3, 71.7), 144, 144, far=FAR))
    return dict(origin=np.full(3, -1.6, np.float32), voxel_size=S["voxel_size"], views=views, color=True)


def fused_mirror(scene):
    m = borc.BlockMirror.around(scene["origin"], scene["voxel_size"], scene["views"], color=scene["color"])
    m = borc.BlockMirror(scene["origin"], scene["voxel_size"], (0, 0, 0), tuple(l + n for l, n in zip(m.lo, m.nb)), color=scene["color"])
    m.integrate_blocks_f32(scene["views"])
    return m


def differing_cells(mirror, dense):
    a = {tuple(c) for c in borc.active_cells(mirror.masked_volume())}
    b = {tuple(c) for c in borc.active_cells(dense)}
    return sorted(a ^ b)


@pytest.mark.parametrize("scene", [plane_scene, sphere_scene], ids=["plane", "sphere"])
def test_blocks_mirror_mesh_is_the_dense_mirror_mesh(scene):
    scene = scene()
    mirror = fused_mirror(scene)
    assert mirror.lo == (0, 0, 0) and len(mirror.keys) > 4
    assert (borc.unpack_keys(mirror.keys) >= 0).all()
    n64 = borc.allocation_keys_f64(scene["origin"], scene["voxel_size"], mirror.vol["trunc"], scene["views"])
    print(f"{len(mirror.keys)} blocks; the float64 statement differs in {len(np.setxor1d(n64, mirror.keys))} keys")
    dense = orc.copy_volume(orc.empty_volume(mirror.vol["dims"], scene["origin"], scene["voxel_size"], color=scene["color"]))
    orc.integrate_f32(dense, scene["views"])
    keep = mirror.allocated_samples().reshape(-1)
    for name in orc.PLANES:      # the blocks hold the dense rule's values, bit for bit
        if name in dense:
            assert np.array_equal(mirror.vol[name][keep].view(np.uint32), dense[name][keep].view(np.uint32)), name
    assert differing_cells(mirror, dense) == []
    vb, cb, fb = mirror.mesh_blocks_f32()
    vd, cd, fd = orc.mesh_f32(dense)
    assert len(vb) == len(vd) > 50 and len(fb) == len(fd) > 50
    assert borc.mesh_as_sets(vb, cb, fb) == borc.mesh_as_sets(vd, cd, fd)
    # (key, l) order: the blocks ascend, and the cells inside a block
    order_key = borc.cell_order_key(borc.active_cells(mirror.masked_volume()))
    assert len(np.unique(order_key)) == len(vb)
    if scene["color"]:      # the sphere (the part of the mesh inside the far wall's band): closed, oriented outward, Euler characteristic 2
        near = np.linalg.norm(vb.astype(np.float64) - np.asarray(cases.SPHERE["centre"]), axis=1) < 0.75
        inner = near[fb].all(1)
        assert np.array_equal(inner, near[fb].any(1)) and inner.sum() > 100
        number = np.cumsum(near) - 1
        closed, euler = orc.manifold_report(number[fb[inner]], int(near.sum()))
        assert closed and euler == 2
        assert orc.signed_volume(vb, fb[inner]) > 0.8 * 4.0 / 3.0 * np.pi * cases.SPHERE["radius"] ** 3


def test_mirror_with_signed_indices():
    """The sphere on a lattice whose origin puts its blocks at negative coordinates: the mirror evaluates positions from the signed
    global indices, observes the sphere's surface band and nothing outside the allocated blocks."""
    views = sphere_scene()["views"][:2]
    signed = borc.BlockMirror.around(np.full(3, 2.0, np.float32), 0.1, views, color=True)
    assert max(signed.lo) < 0
    signed.integrate_blocks_f32(views)
    seen = signed.vol["weight"] > 0
    assert seen.sum() > 1000 and not (seen & ~signed.allocated_samples().reshape(-1)).any()
    assert (signed.vol["tsdf"][seen] < 0).any() and (signed.vol["tsdf"][seen] > 0).any()
