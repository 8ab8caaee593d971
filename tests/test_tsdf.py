"""TSDF fusion and surface nets without a GPU: the ABI of the new entry points, every refusal, and the NumPy statements of the rules
(tests/tsdf_oracle.py) checked against each other and against geometry they must reproduce.

FRAGILE voxels.  A voxel is fragile for a view if, in float64, ``u + 0.5`` or ``v + 0.5`` lies within 1e-4 of an integer, ``z`` within 1e-6
relative of ``depth_min``, or ``sdf`` within 1e-6 * trunc of ``-trunc``: a float32 rounding may take another pixel or another branch there.
They are left out of the comparisons and capped at 0.5 % of the voxels any view touches -- a condition on the cases (the cameras of
tests/tsdf_cases.py carry odd fractions for it), asserted below.

The float32 mirror against the float64 statement on the non-fragile voxels of these cases, measured: every decision (the weights)
equal; tsdf within 8.2e-7 (general case; sphere 5.1e-7, plane 2.7e-7), colours within 8.0e-8.  The bound asserted is 2e-6 / 5e-7: a
running mean of values in [-1, 1] over at most six views, a handful of float32 roundings (2^-24 each) per view on top of the
rounding of ``sdf / trunc``, whose inputs ``d`` and ``z`` of magnitude 4 carry 2.4e-7 each against a trunc of 0.3-0.4.  Twice the measured
difference is the tolerance a GPU comparison falls back on should bit equality with the mirror not hold (tests/test_gpu_tsdf.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import refusal_recording
import tsdf_cases as cases
import tsdf_oracle as orc
from lvdgs import _lib

FRAGILE_CAP = 0.005
TSDF_F64_TOL, COLOR_F64_TOL = 2e-6, 5e-7


def test_the_module_and_the_exports_exist():
    from lvdgs import tsdf
    for name in ("lvdgs_tsdf_integrate", "lvdgs_tsdf_mesh", "lvdgs_tsdf_mesh_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert callable(tsdf.TsdfVolume) and callable(tsdf.save_mesh_ply) and tsdf.Mesh._fields == ("vertices", "colors", "faces")


FAKE = 4096      # a non-NULL pointer value; every call below is refused before a launch, so it is never dereferenced
_recorded = None      # of the refusal test that is running: files what _integrate and _mesh see (refusal_recording.Numbered)


def _volume(color=False, **kw):
    v = _lib.TsdfVolumeArgs(nx=8, ny=8, nz=8, origin=(C.c_float * 3)(0, 0, 0), voxel_size=0.1, trunc=0.4, max_weight=64.0, tsdf=FAKE, weight=FAKE)
    if color:
        v.r = v.g = v.b = FAKE
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def _view(**kw):
    a = _lib.TsdfViewArgs(width=64, height=48, fx=50, fy=50, cx=32, cy=24, depth_min=0, depth_trunc=10, R=FAKE, T=FAKE, depth=FAKE)
    for k, val in kw.items():
        setattr(a, k, val)
    return a


def _integrate(vol, views, count=None):
    L = _lib.lib()
    ptrs = (C.POINTER(_lib.TsdfViewArgs) * max(len(views), 1))(*[C.pointer(v) if v is not None else None for v in views])
    status = L.lvdgs_tsdf_integrate(C.byref(vol) if vol is not None else None, ptrs, len(views) if count is None else count, None)
    _recorded(status, L.lvdgs_last_error())
    return status, L.lvdgs_last_error().decode()


def test_integrate_refusals_without_gpu():
    global _recorded
    _recorded = refusal_recording.Numbered("test_tsdf::integrate")
    L = _lib.lib()
    inf, nan = float("inf"), float("nan")
    ok = _view()
    assert _integrate(None, [ok]) == (_lib.E_INVALID, "tsdf integrate: volume is NULL")
    assert L.lvdgs_tsdf_integrate(C.byref(_volume()), None, 0, None) == _lib.OK                     # nothing to do
    assert L.lvdgs_tsdf_integrate(C.byref(_volume()), None, 1, None) == _lib.E_INVALID and b"view list is NULL" in L.lvdgs_last_error()
    for count in (-1, 17):
        status, msg = _integrate(_volume(), [ok], count)
        assert status == _lib.E_INVALID and f"count {count} is outside 0 .. 16" in msg
    for plane in ("tsdf", "weight"):
        status, msg = _integrate(_volume(**{plane: None}), [ok])
        assert status == _lib.E_INVALID and "tsdf / weight plane is NULL" in msg
    status, msg = _integrate(_volume(r=FAKE), [ok])
    assert status == _lib.E_INVALID and "all set or all NULL" in msg
    for dim in ("nx", "ny", "nz"):
        status, msg = _integrate(_volume(**{dim: 0}), [ok])
        assert status == _lib.E_RANGE and "every dimension must be at least 1" in msg
    status, msg = _integrate(_volume(nx=2048, ny=1024, nz=1024), [ok])
    assert status == _lib.E_RANGE and "more than 2^31 - 1 cells" in msg
    status, msg = _integrate(_volume(nx=1 << 16, ny=1 << 16, nz=1), [ok])
    assert status == _lib.E_RANGE and "more than 2^31 - 1 cells" in msg
    for field in ("voxel_size", "trunc", "max_weight"):
        for bad in (0.0, -1.0, inf, nan):
            status, msg = _integrate(_volume(**{field: bad}), [ok])
            assert status == _lib.E_RANGE and "must be finite and positive" in msg, (field, bad)
    status, msg = _integrate(_volume(), [ok, None])
    assert status == _lib.E_INVALID and "view 1 is NULL" in msg
    for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 16, height=1 << 16)):
        status, msg = _integrate(_volume(), [ok, _view(**kw)])
        assert status == _lib.E_RANGE and "view 1: image size" in msg, kw
    for field in ("R", "T", "depth"):
        status, msg = _integrate(_volume(), [_view(**{field: None})])
        assert status == _lib.E_INVALID and "view 0: R / T / depth is NULL" in msg
    status, msg = _integrate(_volume(color=False), [_view(image=FAKE)])
    assert status == _lib.E_INVALID and "no colour planes" in msg


def _mesh_args(vol=None, **kw):
    a = _lib.TsdfMeshArgs(vol=vol or _volume(), seq=1, vertex_capacity=10, face_capacity=10, vertices=FAKE, faces=FAKE, host_state=FAKE,
                          scratch=FAKE, scratch_bytes=1 << 40)
    for k, val in kw.items():
        setattr(a, k, val)
    return a


def _mesh(a):
    L = _lib.lib()
    status = L.lvdgs_tsdf_mesh(C.byref(a) if a is not None else None, None)
    _recorded(status, L.lvdgs_last_error())
    return status, L.lvdgs_last_error().decode()


def test_mesh_refusals_without_gpu():
    global _recorded
    _recorded = refusal_recording.Numbered("test_tsdf::mesh")
    L = _lib.lib()
    assert _mesh(None) == (_lib.E_INVALID, "tsdf mesh: args is NULL")
    for plane in ("tsdf", "weight"):
        status, msg = _mesh(_mesh_args(_volume(**{plane: None})))
        assert status == _lib.E_INVALID and "tsdf / weight plane is NULL" in msg
    status, msg = _mesh(_mesh_args(_volume(g=FAKE)))
    assert status == _lib.E_INVALID and "all set or all NULL" in msg
    for dims in ((1, 8, 8), (8, 1, 8), (5, 1, 3), (8, 8, 1), (0, 8, 8)):
        status, msg = _mesh(_mesh_args(_volume(nx=dims[0], ny=dims[1], nz=dims[2])))
        assert status == _lib.E_RANGE and "every dimension must be at least 2" in msg, dims
        assert L.lvdgs_tsdf_mesh_scratch_bytes(*dims) == 0
    status, msg = _mesh(_mesh_args(_volume(nx=2048, ny=1024, nz=1024)))
    assert status == _lib.E_RANGE and "more than 2^31 - 1 cells" in msg
    assert L.lvdgs_tsdf_mesh_scratch_bytes(2048, 1024, 1024) == 0
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        status, msg = _mesh(_mesh_args(_volume(voxel_size=bad)))
        assert status == _lib.E_RANGE and "must be finite and positive" in msg
    for field in ("vertex_capacity", "face_capacity"):
        status, msg = _mesh(_mesh_args(**{field: -1}))
        assert status == _lib.E_RANGE and "negative capacity" in msg
    for field in ("vertices", "faces", "host_state", "scratch"):
        status, msg = _mesh(_mesh_args(**{field: None}))
        assert status == _lib.E_INVALID and "vertices / faces / host_state / scratch is NULL" in msg
    status, msg = _mesh(_mesh_args(colors=FAKE))
    assert status == _lib.E_INVALID and "no colour planes" in msg
    need = L.lvdgs_tsdf_mesh_scratch_bytes(8, 8, 8)
    assert need % 256 == 0 and need >= 8 * 8 * 8 * 6      # two bytes and one word per sample, and the span counts
    status, msg = _mesh(_mesh_args(scratch_bytes=need - 1))
    assert status == _lib.E_INVALID and "scratch too small" in msg
    assert L.lvdgs_tsdf_mesh_scratch_bytes(1290, 1290, 1290) > L.lvdgs_tsdf_mesh_scratch_bytes(256, 256, 256) > need


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from lvdgs.tsdf import TsdfVolume
    with pytest.raises(_lib.LvdgsError):
        TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    if not torch.cuda.is_available():
        return
    vol = TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), color=False)
    with pytest.raises(_lib.LvdgsError):
        vol.integrate(torch.ones(4, 4), torch.eye(3, device="cuda"), torch.zeros(3, device="cuda"), (1, 1, 0, 0))


# ---------------------------------------------------------------- the oracles against each other ----
def _both(case):
    v32, v64 = orc.copy_volume(case["vol"]), orc.copy_volume(case["vol"], np.float64)
    t32 = orc.integrate_f32(v32, case["views"])
    t64, fragile = orc.integrate_f64(v64, case["views"])
    return v32, v64, t32, t64, fragile


@pytest.mark.parametrize("name", ["plane", "sphere", "general", "general_no_colour"])
def test_float32_mirror_against_the_float64_statement(name):
    case = {"plane": cases.plane_case, "sphere": cases.sphere_case, "general": lambda: cases.general_case(True),
            "general_no_colour": lambda: cases.general_case(False)}[name]()
    v32, v64, t32, t64, fragile = _both(case)
    touched = (t32 | t64).any(0)
    skip = fragile.any(0)
    share = skip.sum() / touched.sum()
    print(name, "voxels", touched.size, "touched", int(touched.sum()), "fragile", int(skip.sum()), "share", share)
    assert touched.sum() > 0.3 * touched.size and share <= FRAGILE_CAP
    good = ~skip
    assert np.array_equal(t32[:, good], t64[:, good])
    assert np.array_equal(v32["weight"][good], v64["weight"][good])
    for plane, tol in (("tsdf", TSDF_F64_TOL), ("r", COLOR_F64_TOL), ("g", COLOR_F64_TOL), ("b", COLOR_F64_TOL)):
        if plane in v32:
            diff = float(np.abs(v32[plane][good] - v64[plane][good]).max())
            print(name, plane, diff)
            assert diff <= tol, (plane, diff)
    if name.startswith("general"):      # the case does hold what it is there for
        views, vol = case["views"], case["vol"]
        assert any((v["depth"] == 0).any() for v in views) and views[0]["mask"] is not None and not views[0]["mask"].all()
        assert (views[0]["depth"] > views[0]["depth_trunc"]).any() and views[2]["depth_min"] > 0
        assert not t64.any(0).all() and all(t.any() for t in t64) and all(d % 4 for d in vol["dims"])
        assert (v64["weight"] == 3).any() and (v64["weight"] == 1).any()


@pytest.mark.parametrize("name", ["sphere", "slanted", "blobs", "holes"])
def test_mesh_mirror_against_the_float64_statement(name):
    vol = _extraction()[name]
    v32, c32, f32 = orc.mesh_f32(vol)
    v64, c64, f64 = orc.mesh_f64(vol)
    assert len(v32) > 100 and len(f32) > 100 and v32.dtype == np.float32 and f32.dtype == np.int32
    assert np.array_equal(f32, f64) and len(v32) == len(v64)
    assert np.abs(v32 - v64).max() <= 4e-7 * max(1.0, np.abs(v64).max())
    if c32 is not None:
        assert np.abs(c32 - c64).max() <= 4e-7
    if name == "holes":
        closed, _ = orc.manifold_report(f32, len(v32))
        assert not closed and (vol["weight"] == 0).sum() > 20


_EXTRACTION = {}


def _extraction():
    if not _EXTRACTION:
        _EXTRACTION.update(cases.extraction_cases())
    return _EXTRACTION


# ---------------------------------------------------------------- geometry ----
def test_plane_case():
    """Every vertex at the plane's depth to 1e-5 relative (the projective distance is linear in z along the camera's axis, so its
    interpolation is exact up to rounding), all normals along one direction of z: from inside -- behind the plane -- to outside."""
    case = cases.plane_case()
    vol = orc.copy_volume(case["vol"])
    orc.integrate_f32(vol, case["views"])
    vertices, colors, faces = orc.mesh_f32(vol)
    assert len(vertices) >= 50 and len(faces) >= 80 and colors is None
    z_cam = vertices[:, 2].astype(np.float64) + 1.0      # the camera sits at z = -1 and looks along +z
    assert np.abs(z_cam - case["d0"]).max() <= 1e-5 * case["d0"]
    normals = orc.face_normals(vertices, faces)
    assert np.abs(normals[:, :2]).max() <= 1e-6 * np.abs(normals[:, 2]).min()
    assert (normals[:, 2] < 0).all() or (normals[:, 2] > 0).all()
    assert (normals[:, 2] < 0).all()      # inside is behind the plane, at larger z


def test_sphere_case():
    """The fused sphere: a closed oriented manifold of genus 0 with positive volume, between the spheres of radius r -+ 2 voxels (one
    cell diagonal, 1.74 voxels, plus the half-voxel footprint of a pixel)."""
    case = cases.sphere_case()
    vol = _extraction()["sphere"]
    vertices, colors, faces = orc.mesh_f32(vol)
    closed, euler = orc.manifold_report(faces, len(vertices))
    assert closed and euler == 2
    volume = orc.signed_volume(vertices, faces)
    ball = lambda r: 4.0 / 3.0 * np.pi * r ** 3
    r, vs = case["radius"], vol["voxel_size"]
    print("sphere volume", volume, "radius of the same volume", (3 * volume / (4 * np.pi)) ** (1 / 3))
    assert volume > 0 and ball(r - 2 * vs) <= volume <= ball(r + 2 * vs)
    dist = np.linalg.norm(vertices.astype(np.float64) - case["centre"], axis=1)
    assert np.abs(dist - r).max() <= 2 * vs
    assert colors.min() >= 0 and colors.max() <= 1


def test_save_mesh_ply_round_trip(tmp_path):
    from lvdgs.tsdf import Mesh, save_mesh_ply
    vertices, colors, faces = orc.mesh_f32(_extraction()["blobs"])
    colors = colors * np.float32(1.3) - np.float32(0.1)      # beyond [0, 1]: clamped
    path = tmp_path / "mesh.ply"
    save_mesh_ply(str(path), Mesh(torch.from_numpy(vertices), torch.from_numpy(colors), torch.from_numpy(faces)))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    nv, nf = (int(next(l for l in lines if l.startswith(f"element {k}")).split()[2]) for k in ("vertex", "face"))
    assert [l.split()[-1] for l in lines if l.startswith("property")] == ["x", "y", "z", "red", "green", "blue", "vertex_indices"]
    assert "property list uchar int vertex_indices" in lines
    vrec = np.frombuffer(body, np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))]), nv)
    frec = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nf, offset=nv * 15)
    assert len(body) == nv * 15 + nf * 13 and nv == len(vertices) and nf == len(faces)
    assert np.array_equal(vrec["p"], vertices) and np.array_equal(frec["i"], faces) and (frec["n"] == 3).all()
    assert np.array_equal(vrec["c"], (np.clip(colors, 0, 1) * np.float32(255)).astype(np.uint8))
    save_mesh_ply(str(path), Mesh(torch.from_numpy(vertices), None, torch.from_numpy(faces)))
    assert len(open(path, "rb").read().split(b"end_header\n", 1)[1]) == nv * 12 + nf * 13
