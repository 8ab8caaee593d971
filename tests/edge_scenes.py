"""Seeded scenes that put many Gaussians into one of the regimes where a splatting backward has its special cases, and
``regime_counts``, which counts from the oracle's outputs how much of each regime a scene actually reaches (test
infrastructure: tests/test_oracle_edges.py runs them at toy sizes against the float64 autograd statement, tests/test_gpu_edge_regimes.py
at moderate sizes through the kernels against the float32 oracle).

Every generator returns ``(g, cam)``: the dict of float32 CPU tensors ``synthetic.make_gaussians`` returns and a
``synthetic.make_camera`` camera.  Placements keep a relative margin of at least 2 % from the guard band and the near plane, so
that float32 inputs read in float64 fall on the side the formula puts them; exact-threshold placements belong to the GPU test
against the float32 oracle.

Pixel convention of ``synthetic.make_camera``'s projection: view-space (x, y, z) lands on pixel (fx x / z + cx - 0.5,
fy y / z + cy - 0.5), pixel (i, j) being evaluated at (i, j); the guard band clamps x / z beyond 1.3 tan(fov_x / 2) = 0.65 W / fx,
i.e. more than 0.65 W pixels from cx - 0.5 (y: 0.65 H from cy - 0.5), whatever the focal length."""
import math

import numpy as np
import torch

from lvdgs import synthetic

NEAR_CULL = 0.2      # view z at or below is culled (csrc/common.hpp, oracle/lvdgs_oracle.c)
FOV_GUARD = 1.3      # x/z, y/z clamp in the EWA Jacobian, times tan(fov/2)
LOWPASS = 0.3        # added to the 2-D covariance diagonal
ALPHA_MAX = 0.99
ALPHA_MIN = 1.0 / 255.0
NEAR_Z = 0.35        # "near": view z in (0.2, 0.35]
TILE = 16


def _camera(W, H, kind="centred", pose_seed=3):
    """"centred": fx = fy = W, principal point at the centre; "offcentre": cx = 0.22 W, cy = 0.78 H, so that centres INSIDE the
    frame are clamped on a band along the right edge (x > 0.87 W) and one along the top (y < 0.13 H); "wide": tan(fov/2) = 1.25 on
    both axes."""
    if kind == "centred":
        return synthetic.make_camera(W, H, pose_seed=pose_seed)
    if kind == "offcentre":
        return synthetic.make_camera(W, H, pose_seed=pose_seed, cx=0.22 * W, cy=0.78 * H)
    if kind == "wide":
        return synthetic.make_camera(W, H, pose_seed=pose_seed, fx=W / 2.5, fy=H / 2.5)
    raise ValueError(kind)


def _random_quats(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _assemble(cam, px, py, z, sigma, opac, rng, sh_degree=0, rotations=None, scales=None):
    """Gaussians whose view-space centres project to pixel (px, py) at view depth z (taken to the world through the camera's
    pose), footprints of about ``sigma`` pixels (per-axis scale z sigma / fx x U[0.7, 1.3], random orientation) unless
    ``scales`` / ``rotations`` are given.  Returns the dict of ``synthetic.make_gaussians``."""
    n = len(px)
    x = (px - cam.cx + 0.5) * z / cam.fx
    y = (py - cam.cy + 0.5) * z / cam.fy
    p_cam = np.stack([x, y, z], 1)
    R, T = cam.R.double().numpy(), cam.T.double().numpy()
    means = (p_cam - T) @ R                        # R^T (p - T), row by row
    if scales is None:
        scales = (z * sigma / cam.fx)[:, None] * rng.uniform(0.7, 1.3, (n, 3))
    if rotations is None:
        rotations = _random_quats(rng, n)
    rgb = rng.uniform(0.0, 1.0, (n, 3))
    K = (sh_degree + 1) ** 2
    shs = np.zeros((n, K, 3))
    shs[:, 0] = (rgb - 0.5) / synthetic.SH_C0
    if K > 1:
        shs[:, 1:] = 0.1 * rng.standard_normal((n, K - 1, 3))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(means3D=t(means), scales=t(scales), rotations=t(rotations), opacities=t(np.reshape(opac, (n, 1))), shs=t(shs),
                colors=t(rgb))


def _concat(*parts):
    return {k: torch.cat([p[k] for p in parts], 0).contiguous() for k in parts[0]}


def _ordinary(cam, W, H, n, rng, sh_degree=0, z=(1.5, 8.0), sigma=(1.0, 5.0)):
    """Small blobs over the frame (opacity sigmoid(N(0, 1.5)) below 0.95: never capped)."""
    px, py = rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)
    zz = np.exp(rng.uniform(math.log(z[0]), math.log(z[1]), n))
    s = np.exp(rng.uniform(math.log(sigma[0]), math.log(sigma[1]), n))
    o = np.minimum(1.0 / (1.0 + np.exp(-1.5 * rng.standard_normal(n))), 0.95)
    return _assemble(cam, px, py, zz, s, o, rng, sh_degree)


def cap_scene(N, W, H, seed=0, pose_seed=3, sh_degree=0):
    """**cap**: three in four Gaussians with opacity in [0.995, 0.99999] centred within 0.05 px of a pixel centre, footprints of
    1.5-4.5 px: o G > 0.99 on that pixel.  Every such Gaussian has a pixel of its own (a footprint under 10 px cannot reach
    G > 0.995 one pixel away), so two capped alphas never meet on a pixel -- (1 - 0.99)^2 would put T exactly on the 1e-4
    stop.  The rest are ordinary blobs."""
    rng = np.random.default_rng(seed)
    cam = _camera(W, H, "centred", pose_seed)
    n_cap = (3 * N) // 4
    cells = rng.choice((W - 4) * (H - 4), size=n_cap, replace=False)
    px = 2 + cells % (W - 4) + rng.uniform(-0.05, 0.05, n_cap)
    py = 2 + cells // (W - 4) + rng.uniform(-0.05, 0.05, n_cap)
    z = np.exp(rng.uniform(math.log(1.5), math.log(8.0), n_cap))
    sigma = rng.uniform(1.5, 4.5, n_cap)
    opac = rng.uniform(0.995, 0.99999, n_cap)
    caps = _assemble(cam, px, py, z, sigma, opac, rng, sh_degree)
    return _concat(caps, _ordinary(cam, W, H, N - n_cap, rng, sh_degree)), cam


def _off_threshold(r, margin=0.03):
    """Guard ratios (x/z over the band's limit) moved out of [1 - margin, 1 + margin] in magnitude."""
    a = np.abs(r)
    a = np.where((a > 1 - margin) & (a <= 1), 1 - margin, np.where((a > 1) & (a < 1 + margin), 1 + margin, a))
    return np.sign(r) * a


def guard_scene(N, W, H, seed=0, camera="centred", pose_seed=3, sh_degree=0):
    """**guard**: three in five Gaussians beyond the EWA guard band -- left, right, above, below and in the four corners, at
    1.04-1.45 times the band's limit -- with footprints large enough to reach well into the frame; the rest ordinary blobs.
    ``camera`` (``_camera``): with "offcentre" a third of the clamped ones are centred INSIDE the frame, on the bands where that
    principal point puts the limit in the image; "wide" has tan(fov/2) = 1.25."""
    rng = np.random.default_rng(seed)
    cam = _camera(W, H, camera, pose_seed)
    n_g = (3 * N) // 5
    ox, oy = cam.cx - 0.5, cam.cy - 0.5                 # pixel of the optical axis
    limx, limy = 0.65 * W, 0.65 * H                      # the band's limit, in pixels from it
    # guard ratios of the frame's pixels (x / z over the limit): the non-clamped axis is drawn among them
    rx = (rng.uniform(0, W - 1, n_g) - ox) / limx
    ry = (rng.uniform(0, H - 1, n_g) - oy) / limy
    kind = rng.integers(0, 8, n_g)                       # 0-1 x -/+, 2-3 y -/+, 4-7 corners
    beyond = lambda s, n: s * rng.uniform(1.04, 1.45, n)
    sx = np.where(kind % 2 == 0, -1.0, 1.0)
    sy = np.where((kind // 2) % 2 == 0, -1.0, 1.0)
    is_x = (kind < 2) | (kind >= 4)
    is_y = ((kind >= 2) & (kind < 4)) | (kind >= 4)
    rx = np.where(is_x, beyond(sx, n_g), rx)
    ry = np.where(is_y, beyond(sy, n_g), ry)
    if camera == "offcentre":
        # a third on the in-frame bands: right edge (x) and top edge (y), at 1.03 to 0.98 of the frame's own extent beyond the limit
        inside = rng.uniform(0, 1, n_g) < 1.0 / 3.0
        hi_x, lo_y = (W - 1 - ox) / limx, (0 - oy) / limy
        half = rng.uniform(0, 1, n_g) < 0.5
        rx = np.where(inside & half, rng.uniform(1.03, 0.98 * hi_x, n_g), rx)
        ry = np.where(inside & ~half, -rng.uniform(1.03, 0.98 * -lo_y, n_g), ry)
        ry = np.where(inside & half, (rng.uniform(0, H - 1, n_g) - oy) / limy, ry)
        rx = np.where(inside & ~half, (rng.uniform(0, W - 1, n_g) - ox) / limx, rx)
    rx, ry = _off_threshold(rx), _off_threshold(ry)
    px, py = ox + rx * limx, oy + ry * limy
    dist = np.maximum(np.maximum(-px, px - (W - 1)), np.maximum(-py, py - (H - 1)))
    dist = np.maximum(dist, 0.0)
    sigma = dist / rng.uniform(1.0, 1.6, n_g) + rng.uniform(2.0, 5.0, n_g)
    z = np.exp(rng.uniform(math.log(1.5), math.log(6.0), n_g))
    opac = rng.uniform(0.3, 0.9, n_g)
    guard = _assemble(cam, px, py, z, sigma, opac, rng, sh_degree)
    return _concat(guard, _ordinary(cam, W, H, N - n_g, rng, sh_degree)), cam


def near_scene(N, W, H, seed=0, pose_seed=3, n_behind=4, big_frac=0.15):
    """**near**: view z in [0.205, 0.35] (log-uniform), centres over the frame, footprints of 1-6 px and, for ``big_frac`` of them,
    up to W / 4 px (at 200 px wide and more: rectangles of more than 64 tiles, so block culling and two-level grouping take part);
    plus ``n_behind`` Gaussians just behind the plane (z in [0.190, 0.198]), which must be culled and get exactly zero gradient
    (they are the LAST ``n_behind`` rows)."""
    rng = np.random.default_rng(seed)
    cam = _camera(W, H, "centred", pose_seed)
    n = N - n_behind
    px, py = rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)
    z = np.exp(rng.uniform(math.log(0.205), math.log(NEAR_Z), n))
    big = rng.uniform(0, 1, n) < big_frac
    sigma = np.where(big, np.exp(rng.uniform(math.log(8.0), math.log(max(W / 4.0, 9.0)), n)),
                     np.exp(rng.uniform(0.0, math.log(6.0), n)))
    opac = np.where(big, rng.uniform(0.1, 0.4, n), rng.uniform(0.2, 0.9, n))
    near = _assemble(cam, px, py, z, sigma, opac, rng)
    bx, by = rng.uniform(0, W - 1, n_behind), rng.uniform(0, H - 1, n_behind)
    behind = _assemble(cam, bx, by, rng.uniform(0.190, 0.198, n_behind), rng.uniform(2.0, 6.0, n_behind),
                       rng.uniform(0.5, 0.9, n_behind), rng)
    return _concat(near, behind), cam


def stop_scene(N, W, H, seed=0, pose_seed=3, layers=12):
    """**stop**: ``layers`` (10 or more) sheets of opaque Gaussians (opacity in [0.9, 0.98]: never capped) over the whole frame,
    each a jittered grid whose footprints are 0.75 of its spacing, the sheets at depths 1.5, 1.9, 2.3, ...: most pixels end at
    T < 1e-4 a few sheets in, with the rest of the list behind them."""
    assert layers >= 10
    rng = np.random.default_rng(seed)
    cam = _camera(W, H, "centred", pose_seed)
    per = N // layers
    nx = max(int(round(math.sqrt(per * W / H))), 1)
    ny = max(per // nx, 1)
    parts = []
    for l in range(layers):
        n = per if l < layers - 1 else N - per * (layers - 1)
        cell = rng.integers(0, nx * ny, n) if n > nx * ny else rng.permutation(nx * ny)[:n]
        sx, sy = W / nx, H / ny
        px = (cell % nx + 0.5 + rng.uniform(-0.3, 0.3, n)) * sx - 0.5
        py = (cell // nx + 0.5 + rng.uniform(-0.3, 0.3, n)) * sy - 0.5
        z = (1.5 + 0.4 * l) * (1.0 + 0.02 * rng.uniform(-1, 1, n))
        parts.append(_assemble(cam, px, py, z, 0.75 * min(sx, sy) * np.ones(n), rng.uniform(0.9, 0.98, n), rng))
    return _concat(*parts), cam


def _quat_mul(a, b):
    aw, ax, ay, az = a.T
    bw, bx, by, bz = b.T
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1)


def thin_scene(N, W, H, seed=0, pose_seed=3):
    """**thin**: surface-like Gaussians -- in-plane footprints of 2-10 px, the third scale 1e-3 of the others -- whose thin axis
    is 0.3-2 degrees from perpendicular to the line of sight (seen nearly edge-on): across the projected line the 2-D covariance
    is the +0.3 low-pass term's.  Opacity sigmoid(2 + N(0, 1)) below 0.985 (the surface workloads' law, never capped)."""
    rng = np.random.default_rng(seed)
    cam = _camera(W, H, "centred", pose_seed)
    px, py = rng.uniform(0, W - 1, N), rng.uniform(0, H - 1, N)
    z = np.exp(rng.uniform(math.log(1.5), math.log(8.0), N))
    s_in = z * np.exp(rng.uniform(math.log(2.0), math.log(10.0), N)) / cam.fx
    scales = np.stack([s_in * rng.uniform(0.7, 1.3, N), s_in * rng.uniform(0.7, 1.3, N), 1e-3 * s_in], 1)
    g = _assemble(cam, px, py, z, np.ones(N), np.ones(N), rng, scales=scales, rotations=np.tile([1.0, 0, 0, 0], (N, 1)))
    # thin axis n: perpendicular to the line of sight d, tilted towards it by 0.3-2 degrees; q takes e_z to n, after a random
    # turn about e_z (the in-plane orientation)
    campos = torch.linalg.inv(cam.world_view_transform.double())[3, :3].numpy()
    d = g["means3D"].double().numpy() - campos
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perp = np.cross(d, rng.standard_normal((N, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    tilt = np.radians(rng.uniform(0.3, 2.0, N))
    n = perp * np.cos(tilt)[:, None] + d * np.sin(tilt)[:, None]
    n = np.where(n[:, 2:3] < 0, -n, n)                   # (the same plane) keeps 1 + n_z away from 0
    q_align = np.stack([1.0 + n[:, 2], -n[:, 1], n[:, 0], np.zeros(N)], 1)
    q_align /= np.linalg.norm(q_align, axis=1, keepdims=True)
    phi = rng.uniform(0, 2 * math.pi, N)
    q = _quat_mul(q_align, np.stack([np.cos(phi / 2), np.zeros(N), np.zeros(N), np.sin(phi / 2)], 1))
    g["rotations"] = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32))
    g["opacities"] = torch.from_numpy(np.minimum(1.0 / (1.0 + np.exp(-(2.0 + rng.standard_normal(N)))), 0.985)
                                      .astype(np.float32).reshape(N, 1))
    return g, cam


SCENES = {"cap": cap_scene, "guard": guard_scene, "near": near_scene, "stop": stop_scene, "thin": thin_scene}


def regime_counts(fwd, g, cam):
    """What each regime is about, counted from an oracle forward (``oracle.Oracle.forward``'s dict, either precision) of ``g``
    seen by ``cam``.  "Composited": alpha >= 1/255 on at least one pixel in front of that pixel's stop.

      capped_pairs     composited (pixel, Gaussian) pairs with o G >= 0.99 (the alpha cap active);
      clamped_x / _y   composited Gaussians whose x / z (y / z) lies beyond the guard band; per side clamped_x_neg, clamped_x_pos,
                       clamped_y_neg, clamped_y_pos; clamped_inside: clamped ones centred inside the frame;
      near             composited Gaussians with view z < 0.35;
      stopped_pixels   pixels whose loop ended at T < 1e-4 (an entry with alpha >= 1/255 follows the last contributor);
      lowpass          composited Gaussians whose 2-D covariance has its smaller eigenvalue below 2 x 0.3 (the low-pass term
                       dominates across them);
      composited       composited Gaussians."""
    H, W = fwd["n_contrib"].shape
    N = fwd["radii"].shape[0]
    gx = (W + TILE - 1) // TILE
    m2 = fwd["means2D"].astype(np.float64)
    co = fwd["conic_opacity"].astype(np.float64)
    ids = fwd["ids_sorted"].astype(np.int64)
    ranges = fwd["ranges"].astype(np.int64)
    n_contrib = fwd["n_contrib"].astype(np.int64)
    composited = np.zeros(N, bool)
    capped = stopped = 0
    for t in range(ranges.shape[0]):
        b, e = ranges[t]
        if e <= b:
            continue
        ty, tx = divmod(t, gx)
        ys, xs = np.mgrid[ty * TILE:min(ty * TILE + TILE, H), tx * TILE:min(tx * TILE + TILE, W)]
        xs, ys = xs.ravel(), ys.ravel()
        gid = ids[b:e]
        dx = m2[gid, 0][None] - xs[:, None]
        dy = m2[gid, 1][None] - ys[:, None]
        power = -0.5 * (co[gid, 0][None] * dx * dx + co[gid, 2][None] * dy * dy) - co[gid, 1][None] * dx * dy
        raw = co[gid, 3][None] * np.exp(np.minimum(power, 0.0))
        valid = (power <= 0) & (np.minimum(raw, ALPHA_MAX) >= ALPHA_MIN)
        inside = np.arange(e - b)[None] < n_contrib[ys, xs][:, None]
        comp = valid & inside
        capped += int((comp & (raw >= ALPHA_MAX)).sum())
        stopped += int((valid & ~inside).any(1).sum())
        composited[gid[comp.any(0)]] = True
    V = cam.world_view_transform.double().numpy()
    pv = g["means3D"].double().numpy() @ V[:3, :3] + V[3, :3]
    rx = pv[:, 0] / pv[:, 2] / (FOV_GUARD * cam.tanfovx)
    ry = pv[:, 1] / pv[:, 2] / (FOV_GUARD * cam.tanfovy)
    in_frame = (m2[:, 0] >= 0) & (m2[:, 0] <= W - 1) & (m2[:, 1] >= 0) & (m2[:, 1] <= H - 1)
    a, b_, c = co[:, 0], co[:, 1], co[:, 2]
    conic_max = 0.5 * (a + c) + np.sqrt(0.25 * (a - c) ** 2 + b_ * b_)
    with np.errstate(divide="ignore"):
        minor = np.where(composited, 1.0 / np.where(conic_max > 0, conic_max, np.inf), np.inf)
    cx_, cy_ = composited & (np.abs(rx) > 1), composited & (np.abs(ry) > 1)
    return dict(capped_pairs=capped, clamped_x=int(cx_.sum()), clamped_y=int(cy_.sum()),
                clamped_x_neg=int((cx_ & (rx < 0)).sum()), clamped_x_pos=int((cx_ & (rx > 0)).sum()),
                clamped_y_neg=int((cy_ & (ry < 0)).sum()), clamped_y_pos=int((cy_ & (ry > 0)).sum()),
                clamped_inside=int(((cx_ | cy_) & in_frame).sum()),
                near=int((composited & (pv[:, 2] < NEAR_Z)).sum()), stopped_pixels=stopped,
                lowpass=int((minor < 2 * LOWPASS).sum()), composited=int(composited.sum()))
