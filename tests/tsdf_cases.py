"""The cases of tests/test_tsdf.py and tests/test_gpu_tsdf.py: volumes, cameras and analytically rendered depth maps (NumPy only).

Cameras look at a point from a point; ``R`` has the camera's right, down and forward axes as rows and ``T = -R C`` (``p_cam = R p_world +
T``).  Pixel (ui, vi) is the ray through ``((ui - cx) / fx, (vi - cy) / fy, 1)``: a voxel's nearest pixel is ``floor(u + 0.5)``.
The principal points and camera centres carry odd fractions on purpose, so that the lattice does not project onto pixel borders
(the fragile-voxel cap of tests/test_tsdf.py).
"""
import functools

import numpy as np

import tsdf_oracle as orc


def look_at(centre, target, up=(0.0, 0.0, 1.0)):
    centre, target = np.asarray(centre, np.float64), np.asarray(target, np.float64)
    fwd = target - centre
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64))
    if np.linalg.norm(right) < 1e-6:
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return R.astype(np.float32), (-R @ centre).astype(np.float32)


def pixel_rays(R, T, intrinsics, H, W):
    """Camera centre and the world direction of every pixel's ray with unit camera z: depth = the ray parameter."""
    fx, fy, cx, cy = intrinsics
    R64, T64 = R.astype(np.float64), T.astype(np.float64)
    vi, ui = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d_cam = np.stack([(ui - cx) / fx, (vi - cy) / fy, np.ones((H, W))], -1)
    return -R64.T @ T64, d_cam @ R64


def ray_sphere(origin, dirs, centre, radius, first=True):
    """Ray parameter of the first (or last) intersection with a sphere; 0 where the ray misses or the hit lies behind."""
    oc = origin - np.asarray(centre, np.float64)
    a = (dirs * dirs).sum(-1)
    b = 2.0 * (dirs * oc).sum(-1)
    c = (oc * oc).sum() - radius * radius
    disc = b * b - 4 * a * c
    root = np.sqrt(np.maximum(disc, 0.0))
    s = (-b - root) / (2 * a) if first else (-b + root) / (2 * a)
    return np.where((disc > 0) & (s > 0), s, 0.0)


def sphere_view(centre_cam, sphere_c, radius, intrinsics, H, W, far=None):
    """Depth and colour (0.5 + 0.5 normal) of a sphere; rays that miss it get the inside of a sphere of radius ``far`` (None: 0)."""
    R, T = look_at(centre_cam, sphere_c, up=(0.0, 0.0, 1.0) if abs(centre_cam[2] - sphere_c[2]) < 1e-9 else (0.0, 1.0, 0.0))
    C, dirs = pixel_rays(R, T, intrinsics, H, W)
    s = ray_sphere(C, dirs, sphere_c, radius)
    hit = s > 0
    point = C + s[..., None] * dirs
    normal = (point - np.asarray(sphere_c)) / radius
    image = np.where(hit[None], 0.5 + 0.5 * np.moveaxis(normal, -1, 0), 0.25)
    if far is not None:
        s = np.where(hit, s, ray_sphere(C, dirs, sphere_c, far, first=False))
    return orc.make_view(s.astype(np.float32), R, T, intrinsics, image=image.astype(np.float32))


# ---------------------------------------------------------------- the CPU cases ----
@functools.lru_cache(maxsize=None)
def plane_case():
    """A fronto-parallel plane at depth d0 in front of one camera that looks along the volume's +z axis: constant depth."""
    dims, vs = (12, 10, 14), 0.05
    origin = np.array([-0.3, -0.25, 0.0], np.float32)
    d0 = 1.3137
    R, T = np.eye(3, dtype=np.float32), np.array([0.013, -0.007, 1.0], np.float32)      # z_cam = z_world + 1
    H, W = 48, 64
    view = orc.make_view(np.full((H, W), d0, np.float32), R, T, (67.0, 67.0, 31.3, 23.7))
    vol = orc.empty_volume(dims, origin, vs, color=False)
    return dict(vol=vol, views=[view], d0=float(np.float32(d0)), z_world=float(np.float32(d0)) - 1.0)


SPHERE = dict(dims=(24, 20, 16), voxel_size=0.1, radius=0.5, centre=(1.163, 0.957, 0.771), distance=4.0, far=8.0,
              intrinsics=(100.0, 100.0, 47.3, 47.7), size=(96, 96))


@functools.lru_cache(maxsize=None)
def sphere_case():
    """A sphere of radius r inside a far enclosing sphere (so that free space is observed), seen from six axis views.  The footprint of
    a pixel at the surface is z / fx <= 4.0 / 100 = 0.4 voxels."""
    S = SPHERE
    c = np.asarray(S["centre"])
    H, W = S["size"]
    views = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            cam = c.copy()
            cam[axis] += sign * S["distance"]
            cam += np.array([0.0137, -0.0091, 0.0113])      # off the lattice's planes of symmetry
            views.append(sphere_view(cam, c, S["radius"], S["intrinsics"], H, W, far=S["far"]))
    vol = orc.empty_volume(S["dims"], np.zeros(3, np.float32), S["voxel_size"], color=True)
    return dict(vol=vol, views=views, radius=S["radius"], centre=c)


@functools.lru_cache(maxsize=None)
def general_case(color=True):
    """The GPU integration case: 37 x 22 x 19 voxels (no dimension a multiple of a brick edge or of 4), 64 x 48 images, three views --
    one beside the volume that leaves part of it behind the camera, one with a mask and a depth_trunc that cuts the far pixels, one with
    a depth_min inside the volume -- over depth maps with zero patches."""
    dims, vs = (37, 22, 19), 0.08
    origin = np.array([-1.41, -0.83, 0.21], np.float32)
    H, W = 48, 64
    rng = np.random.default_rng(5)
    vi, ui = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    centre = origin.astype(np.float64) + 0.5 * vs * np.asarray(dims)

    def depth_map(base, seed):
        d = base + 0.35 * np.sin(ui / 9.0 + seed) * np.cos(vi / 7.0 - seed) + 0.02 * rng.standard_normal((H, W))
        d[rng.random((H, W)) < 0.06] = 0.0
        d[5:9, 40:52] = 0.0
        return d.astype(np.float32)

    image = lambda: rng.random((3, H, W)).astype(np.float32) * 1.2 - 0.1 if color else None
    views = []
    R, T = look_at(centre + np.array([0.31, -0.27, -2.6]), centre + np.array([0.05, 0.02, 0.0]), up=(0.0, 1.0, 0.0))
    views.append(orc.make_view(depth_map(2.5, 0.3), R, T, (58.0, 61.0, 30.7, 24.3), image=image(), mask=rng.random((H, W)) > 0.2,
                               depth_trunc=2.7))
    R, T = look_at(centre + np.array([-0.9, 0.1, 0.05]), centre + np.array([1.0, 0.2, 0.3]), up=(0.0, 0.0, 1.0))      # inside the volume
    views.append(orc.make_view(depth_map(1.4, 1.1), R, T, (45.0, 44.0, 33.1, 22.9), image=image()))
    R, T = look_at(centre + np.array([2.2, 1.9, 1.3]), centre, up=(0.0, 0.0, 1.0))
    views.append(orc.make_view(depth_map(3.0, 2.2), R, T, (75.0, 75.0, 20.9, 30.2), image=None, depth_min=2.6))      # looks past the image's edge
    vol = orc.empty_volume(dims, origin, vs, trunc=0.3, color=color)
    return dict(vol=vol, views=views)


# ---------------------------------------------------------------- volumes for the extraction ----
def analytic_volume(dims, sdf, voxel_size=0.1, origin=(0.0, 0.0, 0.0), color=True, holes=0.0, seed=0):
    """A volume whose tsdf plane is ``sdf(points)`` clipped to [-1, 1], weight 1 (0 at a share ``holes`` of the samples), smooth colours."""
    vol = orc.empty_volume(dims, np.asarray(origin, np.float32), voxel_size, color=color)
    i, j, k = orc.lattice_indices(vol["dims"])
    p = np.asarray(origin, np.float64)[None] + voxel_size * np.stack([i, j, k], 1)
    vol["tsdf"] = np.clip(sdf(p) / (4 * voxel_size), -1.0, 1.0).astype(np.float32)
    rng = np.random.default_rng(seed)
    vol["weight"] = (rng.random(len(p)) >= holes).astype(np.float32) * (1.0 + (i % 3)).astype(np.float32)
    if color:
        for n, name in enumerate("rgb"):
            vol[name] = (0.5 + 0.5 * np.sin(p[:, n] * (3.0 + n) + n)).astype(np.float32)
    return vol


def two_spheres(dims, seed):
    """Two overlapping spheres across the middle of the volume, 1 % of the samples unobserved: a surface that crosses many spans."""
    extent = 0.1 * np.asarray(dims, np.float64)
    r = 0.3 * extent.min()
    a, b = extent * np.array([0.38, 0.45, 0.5]), extent * np.array([0.64, 0.55, 0.48])
    return analytic_volume(dims, lambda p: np.minimum(np.linalg.norm(p - a, axis=1) - r, np.linalg.norm(p - b, axis=1) - 0.9 * r),
                           holes=0.01, seed=seed)


def extraction_cases():
    """name -> volume: the fused sphere, a slanted plane, two blobs that touch the boundary, a volume with unobserved holes, and two
    volumes sized for the span scan of the extraction (256 samples to a tile, 256 spans to a round of the scan, at most 2048 spans):
    ``rounds`` has 69 120 samples = 270 spans of one tile, so the scan of the span counts carries into a second round; ``tiles`` has
    540 000 samples = 2110 tiles, above 2048, so a span is two tiles long (1055 spans, five rounds) and the write passes carry their
    row from the first tile into the second."""
    s = sphere_case()
    fused = orc.copy_volume(s["vol"])
    orc.integrate_f32(fused, s["views"])
    n = np.array([0.31, -0.52, 0.8])
    n /= np.linalg.norm(n)
    slanted = analytic_volume((13, 9, 11), lambda p: p @ n - 0.47, color=False)
    blobs = analytic_volume((19, 12, 10), lambda p: np.minimum(np.linalg.norm(p - np.array([0.55, 0.5, 0.45]), axis=1) - 0.33,
                                                               np.linalg.norm(p - np.array([1.5, 0.7, 0.2]), axis=1) - 0.41))
    holes = analytic_volume((17, 15, 9), lambda p: np.linalg.norm(p - np.array([0.8, 0.7, 0.4]), axis=1) - 0.55, holes=0.03, seed=3)
    return dict(sphere=fused, slanted=slanted, blobs=blobs, holes=holes, rounds=two_spheres((48, 40, 36), 7), tiles=two_spheres((90, 80, 75), 8))
