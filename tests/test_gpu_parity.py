"""Parity of the HIP rasterizer (through the C ABI) against the CPU oracle (float32 build) on the
same seeded inputs.  Integers derived from per-Gaussian float maths (radii, tile rectangles,
sorted tile/depth/id lists, tile ranges) must be bit-exact; rendered images and gradients must
agree within 1e-4 relative (BASELINE.json north_star).  Blend-time counters (n_contrib,
n_touched) depend on exp() rounding at the 1/255, 1e-4 and 0.5 thresholds, so they are required
to be exact wherever the oracle did not flag a comparison as within 1e-5 of its threshold."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # north_star tolerance for float outputs


def _mods():
    import oracle as orc
    import hip_runner
    from lvdgs import synthetic
    return orc, hip_runner, synthetic


def _scene(synthetic, N, W, H, seed, pose_seed=None, sh_degree=0, **kw):
    g = synthetic.make_gaussians(N, W, H, seed=seed, sh_degree=sh_degree, **kw)
    cam = synthetic.make_camera(W, H, pose_seed=pose_seed)
    return g, cam


def _close(a, b, rtol=RTOL, atol_scale=1e-5, what="", rel_l2=2e-5, max_rel_sig=1e-3):
    """Three requirements (achieved errors of every call go to gpurun_out/parity_report.*, see parity_stats.py):
      * |a-b| <= rtol*|b| + atol_scale*max|b| elementwise;
      * ||a-b||_2 <= rel_l2 * ||b||_2 (the tensor as a whole is far inside the north star's 1e-4);
      * elements that are not cancellation residues (|b| >= 1e-3 max|b|) are within max_rel_sig of their own value."""
    import parity_stats
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    st = parity_stats.record(what, a, b)
    tol = rtol * np.abs(b) + atol_scale * max(np.abs(b).max(), 1e-30)
    bad = np.abs(a - b) > tol
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outside tolerance, worst {np.abs(a - b).max():.3e} (scale {np.abs(b).max():.3e})"
    if st is not None and st["scale"] > 0:
        assert st["rel_l2"] <= rel_l2, f"{what}: relative L2 error {st['rel_l2']:.3e}"
        assert st["max_rel_sig"] <= max_rel_sig, f"{what}: max relative error on significant elements {st['max_rel_sig']:.3e}"


def _check_forward(f_hip, f_ora, W, H):
    import hip_runner
    N = f_ora["radii"].shape[0]
    # ---- bit-exact integer / index state ----
    np.testing.assert_array_equal(f_hip["radii"], f_ora["radii"])
    vis = f_ora["radii"] > 0
    rec = f_hip["rec"]
    # per-Gaussian projection: same float32 operations in the same order -> identical bits
    np.testing.assert_array_equal(rec[vis, 0:2], f_ora["means2D"][vis])
    np.testing.assert_array_equal(rec[vis, 9], f_ora["depths"][vis])
    np.testing.assert_array_equal(rec[vis, 2:5], f_ora["conic_opacity"][vis, 0:3])
    np.testing.assert_array_equal(rec[vis, 11].view(np.int32), f_ora["radii"][vis])
    _close(rec[vis, 6:9], f_ora["rgb"][vis], rtol=1e-6, what="rgb")
    # sorted (tile, depth, id) list and per-tile ranges: the reference's, or (tile culling, the default) the reference's
    # minus pairs that provably contribute to no pixel
    hip_runner.check_pair_lists(f_hip, f_ora, W, H)
    if len(f_hip["point_list"]):
        depth_bits = rec[:, 9].view(np.uint32)[f_hip["point_list"]]
        keys64 = (f_hip["tile_keys"].astype(np.uint64) << np.uint64(32)) | depth_bits.astype(np.uint64)
        np.testing.assert_array_equal(keys64, f_ora["keys_sorted"][f_hip["kept_in_oracle_list"]])
    # ---- images ----
    # A pixel is "fragile" when the oracle saw alpha within 1e-5 of 1/255 (or T within 1e-5 of 1e-4 / 0.5):
    # there exp() rounding may include or drop one faint Gaussian, which moves the pixel by at most
    # alpha ~ 4e-3 of its remaining transmittance.  Everywhere else the 1e-4 tolerance applies.
    solid = f_ora["fragile"] == 0
    assert solid.mean() > 0.98
    for k in ("color", "depth", "opacity"):
        m = np.broadcast_to(solid, f_ora[k].shape)
        _close(np.where(m, f_hip[k], 0), np.where(m, f_ora[k], 0), what=k)
        scale = max(np.abs(f_ora[k]).max(), 1e-30)
        assert np.abs(f_hip[k] - f_ora[k]).max() <= 5e-3 * scale, k + " (fragile pixels)"
    _close(np.where(solid, f_hip["final_T"], 0), np.where(solid, f_ora["final_T"], 0), what="final_T")
    # ---- blend-time counters ----
    np.testing.assert_array_equal(f_hip["n_contrib"][solid], hip_runner.expected_n_contrib(f_hip, f_ora)[solid])
    # ... and on the fragile pixels: between the oracle's own bounds -- its last contributor with every comparison that was within
    # 1e-5 of its threshold (alpha against 1/255, T against 1e-4) gone the other way (oracle/lvdgs_oracle.c: n_contrib_lo / _hi)
    if (~solid).any():
        lo, hi = (hip_runner.expected_n_contrib(f_hip, f_ora, k)[~solid].astype(np.int64) for k in ("n_contrib_lo", "n_contrib_hi"))
        got = f_hip["n_contrib"][~solid].astype(np.int64)
        assert ((lo <= got) & (got <= hi)).all(), f"n_contrib outside the oracle's bounds on {int(((got < lo) | (got > hi)).sum())} of {got.size} fragile pixels"
    n_fragile = int((~solid).sum())
    diff = np.abs(f_hip["n_touched"].astype(np.int64) - f_ora["n_touched"].astype(np.int64))
    assert diff.sum() <= 4 * n_fragile + 0, (diff.sum(), n_fragile)
    assert not f_hip["n_touched"][~vis].any()


def gaussians_away_from_fragile_pixels(f_ora, W, H):
    """Boolean (N,): Gaussians whose support holds no fragile pixel.

    A pixel is fragile when the oracle saw a threshold comparison (alpha vs 1/255, T vs 1e-4 or 0.5) within 1e-5
    relative: there exp() rounding may composite one faint Gaussian on one side and not on the other, which perturbs
    that pixel's contribution (by alpha ~ 4e-3 of it) to EVERY Gaussian composited at that pixel.  A Gaussian can reach
    alpha >= 1/255 only where its exponent is above -ln(255): within sqrt(2 ln 255) = 3.33 sigma of its centre, i.e.
    inside the square of half-width 1.12 * radius + 1 around it (radius = ceil(3 sigma_max))."""
    frag = f_ora["fragile"] != 0
    N = f_ora["radii"].shape[0]
    if not frag.any():
        return np.ones(N, bool)
    cum = np.zeros((H + 1, W + 1), np.int64)
    cum[1:, 1:] = frag.cumsum(0).cumsum(1)
    r = np.ceil(1.12 * f_ora["radii"].astype(np.float64) + 1.0)
    m = f_ora["means2D"].astype(np.float64)
    x0 = np.clip(np.floor(m[:, 0] - r), 0, W).astype(np.int64); x1 = np.clip(np.ceil(m[:, 0] + r) + 1, 0, W).astype(np.int64)
    y0 = np.clip(np.floor(m[:, 1] - r), 0, H).astype(np.int64); y1 = np.clip(np.ceil(m[:, 1] + r) + 1, 0, H).astype(np.int64)
    x1, y1 = np.maximum(x1, x0), np.maximum(y1, y0)
    n = cum[y1, x1] - cum[y0, x1] - cum[y1, x0] + cum[y0, x0]
    return (n == 0) | (f_ora["radii"] <= 0)


def masked_rerun(hr, orc, g, cam, W, H, bg, grads, **run_kw):
    """For _check_backward(rerun=...): both sides again with the image gradients of the given pixels zeroed -- returns
    (HIP backward, float32-oracle backward, a function that runs the float64 oracle on the same problem when asked)."""
    def rerun(solid):
        keep = torch.from_numpy(np.ascontiguousarray(solid.reshape(H, W)))[None]
        masked = tuple(None if t is None else torch.where(keep, t, torch.zeros_like(t)) for t in grads)
        _, bh = hr.run_hip(g, cam, W, H, bg, grads=masked, **run_kw)
        ora_kw = {k: v for k, v in run_kw.items() if k in ("use_sh", "sh_degree", "cov_precomp", "scale_modifier")}
        _, bo = hr.run_oracle(orc, g, cam, W, H, bg, grads=masked, **ora_kw)
        return bh, bo, lambda: hr.run_oracle(orc, g, cam, W, H, bg, grads=masked, prec="f64", **ora_kw)[1]
    return rerun


def _no_farther_from_float64_than_the_float32_oracle(n, hip, ref32, ref64, why):
    """The rule of tests/test_gpu_fuzz.py for sums float32 cannot hold to the strict bounds (large cancelling terms): the
    kernels are no farther from the float64 result than the float32 restatement is (x 1.5), plus the strict tolerance."""
    import parity_stats
    hip, ref32, ref64 = (np.asarray(x, np.float64).reshape(np.shape(hip)) for x in (hip, ref32, ref64))
    norm = max(np.linalg.norm(ref64), 1e-300)
    scale = max(np.abs(ref64).max(), 1e-300)
    e_hip, e_ora = np.linalg.norm(hip - ref64) / norm, np.linalg.norm(ref32 - ref64) / norm
    m_hip, m_ora = np.abs(hip - ref64).max(), np.abs(ref32 - ref64).max()
    parity_stats.record(f"grad {n} vs the FLOAT64 oracle (float32 oracle: rel_l2 {e_ora:.2e}, max {m_ora / scale:.2e} of scale)", hip, ref64)
    assert e_hip <= 2e-5 + 1.5 * e_ora, f"{n}: kernels {e_hip:.3e} from float64, float32 oracle {e_ora:.3e} | strict check said: {why}"
    strict = 1e-4 * np.abs(ref64) + 1e-5 * scale
    assert (np.abs(hip - ref64) <= 1.5 * m_ora + strict).all(), f"{n}: max error {m_hip:.3e} vs the float32 oracle's {m_ora:.3e} (scale {scale:.3e}) | {why}"


def _check_backward(b_hip, b_ora, names, f_ora=None, W=None, H=None, rerun=None):
    """Every gradient within the tolerances of _close.

    Fragile pixels (the oracle saw a threshold comparison within 1e-5 relative: exp() rounding may composite one faint
    Gaussian on one side and not on the other) perturb the contribution of THEIR pixel to every Gaussian composited there by
    alpha ~ 4e-3 of it.  With `rerun` (masked_rerun: the full-size cases) the statement that holds for EVERY Gaussian and the
    pose is made on the problem without them: the image gradients of the fragile pixels are zeroed, both sides run again,
    and every tensor must agree to the strict tolerances (1e-4 elementwise + 1e-5 of scale, 2e-5 relative L2; a tensor float32
    cannot hold to them -- the pose gradient of an opaque-surface scene, six sums of large cancelling terms -- must be no farther
    from the FLOAT64 oracle than the float32 oracle is, x 1.5).  On the problem as given: strict on the Gaussians no fragile
    pixel can reach, the perturbation's size on the others."""
    clean = None if f_ora is None else gaussians_away_from_fragile_pixels(f_ora, W, H)
    if rerun is not None and clean is not None and not clean.all():
        bh, bo, float64 = rerun(f_ora["fragile"] == 0)
        b64 = None
        for n in names:
            ref = bo[n].reshape(bh[n].shape)
            try:
                # (relative L2 asserted at five times what the full-size cases achieve, profiles/r04_parity_report.txt:
                # <= 1e-6 per-Gaussian tensors, <= 2.8e-6 the pose gradient)
                _close(bh[n], ref, what="grad " + n + " (image gradients of the fragile pixels zeroed: EVERY Gaussian)", rel_l2=1.5e-5 if n == "tau" else 5e-6)
            except AssertionError as why:
                b64 = float64() if b64 is None else b64
                _no_farther_from_float64_than_the_float32_oracle(n, bh[n], ref, b64[n], why)
    for n in names:
        ref = b_ora[n].reshape(b_hip[n].shape)
        if clean is None or clean.all():
            _close(b_hip[n], ref, what="grad " + n)
            continue
        if n == "tau":  # six sums over every Gaussian, the ones fragile pixels reach included
            if rerun is None:
                _close(b_hip[n], ref, what="grad tau", rel_l2=1e-4)
            else:   # (held strictly on the masked problem above; here to the size of the fragile pixels' perturbation)
                st = parity_stats_record("grad tau (fragile pixels included)", b_hip[n], ref)
                assert st["rel_l2"] <= 1e-3, st
            continue
        if clean.any():
            # (the other Gaussians take the reference's values, so the error of the clean ones is measured against the
            # norm and scale of the whole gradient, whatever the subset happens to contain)
            sel = clean.reshape((-1,) + (1,) * (ref.ndim - 1))
            _close(np.where(sel, b_hip[n], ref), ref, what="grad " + n + " (away from fragile pixels)")
        st = parity_stats_record("grad " + n + " (all Gaussians, fragile pixels included)", b_hip[n], ref)
        scale = max(np.abs(ref).max(), 1e-30)
        assert st["rel_l2"] <= 2e-4, (n, st)
        assert np.abs(b_hip[n] - ref).max() <= 2e-2 * scale, (n, st)


def parity_stats_record(what, a, b):
    import parity_stats
    return parity_stats.record(what, a, b)


@pytest.mark.parametrize("N,W,H,seed,pose", [(2000, 160, 96, 0, None), (5000, 256, 144, 1, 2), (300, 1226, 370, 2, 5)])
def test_forward_and_backward_match_oracle(N, W, H, seed, pose):
    orc, hr, syn = _mods()
    g, cam = _scene(syn, N, W, H, seed, pose_seed=pose)
    bg = torch.tensor([0.2, 0.4, 0.1])
    grads = syn.make_image_grads(W, H, seed)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


def test_config1_10k_640x480_forward():
    """BASELINE.json configs[0]: 10k Gaussians, 640x480, forward."""
    orc, hr, syn = _mods()
    g, cam = _scene(syn, 10_000, 640, 480, 0)
    bg = torch.zeros(3)
    f_hip, _ = hr.run_hip(g, cam, 640, 480, bg)
    f_ora, _ = hr.run_oracle(orc, g, cam, 640, 480, bg)
    _check_forward(f_hip, f_ora, 640, 480)


def test_config2_100k_640x480_forward_backward():
    """BASELINE.json configs[1]: 100k Gaussians, 640x480, forward + backward grad check."""
    orc, hr, syn = _mods()
    W, H = 640, 480
    g, cam = _scene(syn, 100_000, W, H, 0)
    bg = torch.zeros(3)
    grads = syn.make_image_grads(W, H, 0)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


def test_a_map_between_half_a_million_and_a_million_gaussians():
    """The grouping kernels take one Gaussian per thread up to 2^19, four above 2^20 (binning.hpp:
    group_per_thread_default); BASELINE's sizes (100k / 200k / 500k / 2M) never land on the two in between."""
    orc, hr, syn = _mods()
    W, H, N = 640, 480, (1 << 19) + 20_000
    g, cam = _scene(syn, N, W, H, 3)
    bg = torch.zeros(3)
    grads = syn.make_image_grads(W, H, 3)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_spherical_harmonics_degrees(deg):
    orc, hr, syn = _mods()
    W, H, N = 128, 96, 1500
    g, cam = _scene(syn, N, W, H, 10 + deg, pose_seed=1, sh_degree=deg)
    g["shs"][:, 0] -= 1.0  # exercise the clamp mask
    bg = torch.zeros(3)
    grads = syn.make_image_grads(W, H, deg)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, use_sh=True, sh_degree=deg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, use_sh=True, sh_degree=deg, grads=grads)
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "opacities", "scales", "rotations", "shs", "tau"], f_ora, W, H)


def test_precomputed_covariance_path():
    orc, hr, syn = _mods()
    W, H, N = 128, 96, 1200
    g, cam = _scene(syn, N, W, H, 30)
    q, s = g["rotations"].double(), g["scales"].double()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    M = R @ torch.diag_embed(s)
    S = M @ M.transpose(1, 2)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float().contiguous()
    bg = torch.tensor([1.0, 1.0, 1.0])
    grads = syn.make_image_grads(W, H, 3)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, cov_precomp=cov, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, cov_precomp=cov, grads=grads)
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "opacities", "cov3D", "colors", "tau"], f_ora, W, H)


def test_large_gaussians_far_from_their_tiles():
    """Footprints of 40-400 pixels: most (quadrant, Gaussian) pairs have the mean hundreds of pixels outside the
    quadrant, the regime where the backward pass's quadrant-local moments lose the most to cancellation."""
    orc, hr, syn = _mods()
    N, W, H = 400, 640, 480
    g, cam = _scene(syn, N, W, H, 7, pose_seed=3, r_min=40.0, r_max=400.0, z_min=2.0, z_max=20.0)
    with torch.no_grad():
        g["opacities"].mul_(0.25)  # faint enough that hundreds of them contribute to a pixel
    bg = torch.tensor([0.1, 0.2, 0.3])
    grads = syn.make_image_grads(W, H, 7)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    assert np.median(f_ora["radii"][f_ora["radii"] > 0]) > 100
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


def test_edge_cases_empty_culled_single_and_huge():
    orc, hr, syn = _mods()
    W, H = 96, 80
    cam = syn.make_camera(W, H)
    bg = torch.tensor([0.5, 0.25, 0.125])
    grads = syn.make_image_grads(W, H, 1)
    # all culled (behind the camera)
    g = syn.make_gaussians(50, W, H, seed=0)
    g["means3D"][:, 2] = -g["means3D"][:, 2]
    f, b = hr.run_hip(g, cam, W, H, bg, grads=grads)
    assert f["num_rendered"] == 0 and not f["radii"].any() and not f["n_touched"].any()
    assert np.all(f["color"][0] == 0.5) and np.all(f["color"][1] == 0.25) and not f["opacity"].any()
    assert not b["means3D"].any() and not b["tau"].any() and not b["colors"].any()
    # a single Gaussian, and one that covers every tile (many tiles per Gaussian, > 256 per tile below)
    g1 = syn.make_gaussians(1, W, H, seed=1)
    g1["means3D"][0] = torch.tensor([0.0, 0.0, 2.0]); g1["scales"][0] = torch.tensor([3.0, 2.0, 1.0]); g1["opacities"][0] = 0.9
    f_hip, b_hip = hr.run_hip(g1, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g1, cam, W, H, bg, grads=grads)
    assert f_hip["tiles_touched"][0] == ((W + 15) // 16) * ((H + 15) // 16)
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


@pytest.mark.parametrize("N", [1, 2048, 2049, 4099])
def test_slot_bases_are_the_exclusive_scan_of_tiles_touched(N):
    """scan_apply_kernel against numpy.  The kernel runs behind the projection of lvdgs_forward_prepare (the single-call forward of an
    image this small groups by counting and makes its slot bases in the scatter instead), so the test makes that call and reads
    tiles_touched, the slot bases and the pair count it returns.  A workgroup scans a chunk of 2048 Gaussians (256 threads x 8): 4099 is
    two full chunks and a ragged third of three elements -- the prefix from the earlier workgroups' block sums, the carry across waves
    and the tail guard all take part; 2048 and 2049 sit on either side of the chunk boundary."""
    import ctypes as C
    _, hr, syn = _mods()
    from lvdgs import _lib
    L = _lib.lib()
    W = H = 64
    g, cam = _scene(syn, N, W, H, seed=11)
    dev = torch.device("cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    t = {k: v.to(dev).contiguous() for k, v in g.items()}
    mats = [getattr(cam, k).to(dev).contiguous() for k in ("world_view_transform", "full_proj_transform", "projection_matrix", "camera_center")]
    buf = lambda n: torch.zeros(max(int(n), 256), dtype=torch.uint8, device=dev)
    bg, radii, n_touched = torch.zeros(3, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    color, depth, opacity = (torch.empty(c, H, W, device=dev) for c in (3, 1, 1))
    geom, image, scratch = buf(L.lvdgs_geom_bytes(N)), buf(L.lvdgs_image_bytes(W, H)), buf(L.lvdgs_prepare_scratch_bytes(N))
    a = _lib.Args()
    a.image_height, a.image_width, a.tanfovx, a.tanfovy, a.scale_modifier, a.sh_degree = H, W, cam.tanfovx, cam.tanfovy, 1.0, 0
    a.bg, a.viewmatrix, a.projmatrix, a.projmatrix_raw, a.campos = p(bg), p(mats[0]), p(mats[1]), p(mats[2]), p(mats[3])
    a.num_gaussians, a.sh_coeffs = N, 0
    a.means3D, a.opacities, a.scales, a.rotations, a.colors_precomp = p(t["means3D"]), p(t["opacities"]), p(t["scales"]), p(t["rotations"]), p(t["colors"])
    a.radii, a.n_touched, a.out_color, a.out_depth, a.out_opacity = p(radii), p(n_touched), p(color), p(depth), p(opacity)
    a.geom_state, a.geom_bytes, a.image_state, a.image_bytes = p(geom), geom.numel(), p(image), image.numel()
    a.scratch, a.scratch_bytes = p(scratch), scratch.numel()
    D = C.c_int64()
    _lib.check(L.lvdgs_forward_prepare(C.byref(a), C.byref(D), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "prepare")
    torch.cuda.synchronize()
    lay = _lib.StateLayout()
    _lib.check(L.lvdgs_state_layout_query(N, max(D.value, 1), W, H, C.byref(lay)), "layout")
    tt = hr._view(geom, lay.geom_tiles_touched, N, np.uint32).astype(np.uint64)
    slot_base = hr._view(geom, lay.geom_slot_base, N, np.uint32).astype(np.uint64)
    assert N == 1 or (tt[: N // 2].any() and tt[N // 2:].any()), "the scene lists nothing: the scan would be checked on zeros"
    np.testing.assert_array_equal(slot_base, np.concatenate([[0], np.cumsum(tt)[:-1]]))
    assert D.value == int(tt.sum())


def test_many_gaussians_per_tile_and_early_termination():
    """> 256 entries per tile (several staging rounds) and opaque stacks that hit the T < 1e-4 stop."""
    orc, hr, syn = _mods()
    W, H, N = 64, 48, 6000
    g, cam = _scene(syn, N, W, H, 50, r_min=2.0, r_max=6.0, z_min=1.0, z_max=4.0)
    g["opacities"][:] = torch.clamp(g["opacities"] * 2.0, max=0.999)
    bg = torch.zeros(3)
    grads = syn.make_image_grads(W, H, 4)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    assert (f_ora["ranges"][:, 1] - f_ora["ranges"][:, 0]).max() > 600
    assert (f_ora["final_T"] < 1e-3).mean() > 0.3
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


def test_more_than_2048_tiles_two_pass_tile_sort():
    orc, hr, syn = _mods()
    W, H, N = 1920, 1080, 4000
    g, cam = _scene(syn, N, W, H, 60)
    bg = torch.zeros(3)
    f_hip, _ = hr.run_hip(g, cam, W, H, bg)
    f_ora, _ = hr.run_oracle(orc, g, cam, W, H, bg)
    _check_forward(f_hip, f_ora, W, H)


def test_mark_visible_matches_oracle():
    orc, hr, syn = _mods()
    from lvdgs.rasterizer import GaussianRasterizer
    W, H = 64, 64
    cam = syn.make_camera(W, H, pose_seed=7)
    g = syn.make_gaussians(5000, W, H, seed=3, z_min=0.05, z_max=3.0)
    g["means3D"][::3, 2] *= -1
    vis = GaussianRasterizer(hr.settings_from_cam(cam, W, H, torch.zeros(3))).markVisible(g["means3D"].cuda())
    ref = orc.mark_visible(g["means3D"].numpy(), cam.world_view_transform.numpy())
    np.testing.assert_array_equal(vis.cpu().numpy(), ref)


def test_opacity_gradient_switch():
    """By default (PROPAGATE_OPACITY_GRAD = False, the backward binding INTEGRATION.md cites takes dL/dcolor and
    dL/ddepth only) a gradient arriving at the opacity image is dropped -- exactly that path and nothing else."""
    orc, hr, syn = _mods()
    from lvdgs import rasterizer
    assert rasterizer.PROPAGATE_OPACITY_GRAD is False
    W, H, N = 96, 64, 800
    g, cam = _scene(syn, N, W, H, 70)
    bg = torch.zeros(3)
    gc, gd, go = syn.make_image_grads(W, H, 5)
    _, b_off = hr.run_hip(g, cam, W, H, bg, grads=(gc, gd, go), propagate_opacity=False)
    assert rasterizer.PROPAGATE_OPACITY_GRAD is False
    _, b_ref = hr.run_oracle(orc, g, cam, W, H, bg, grads=(gc, gd, None))
    _check_backward(b_off, b_ref, ["means3D", "opacities", "scales", "tau"])


def test_pair_capacity_overflow_reruns_binning_with_identical_results():
    """lvdgs_forward with a capacity that is too small reports the pair count; the wrapper re-runs the
    binning + blend stage with exact sizes.  Outputs and gradients must equal the roomy-capacity run bit for bit."""
    orc, hr, syn = _mods()
    from lvdgs import rasterizer
    W, H, N = 256, 144, 5000
    g, cam = _scene(syn, N, W, H, 80, pose_seed=2)
    bg = torch.zeros(3)
    grads = syn.make_image_grads(W, H, 6)
    f_ok, b_ok = hr.run_hip(g, cam, W, H, bg, grads=grads)
    assert not f_ok["overflowed"]
    saved = (dict(rasterizer._PAIR_CAPACITY), rasterizer._MIN_PAIR_CAPACITY, rasterizer._PAIRS_PER_GAUSSIAN_GUESS)
    try:
        rasterizer._PAIR_CAPACITY.clear()
        rasterizer._MIN_PAIR_CAPACITY, rasterizer._PAIRS_PER_GAUSSIAN_GUESS = 1, 0
        f_small, b_small = hr.run_hip(g, cam, W, H, bg, grads=grads)
        assert f_small["overflowed"] and f_small["num_rendered"] == f_ok["num_rendered"] > 1
        # the capacity has been raised: the next frame fits
        f_next, _ = hr.run_hip(g, cam, W, H, bg)
        assert not f_next["overflowed"]
    finally:
        rasterizer._PAIR_CAPACITY.clear(); rasterizer._PAIR_CAPACITY.update(saved[0])
        rasterizer._MIN_PAIR_CAPACITY, rasterizer._PAIRS_PER_GAUSSIAN_GUESS = saved[1], saved[2]
    for k in ("color", "depth", "opacity", "radii", "n_touched", "point_list", "tile_keys", "ranges", "n_contrib"):
        np.testing.assert_array_equal(f_small[k], f_ok[k], err_msg=k)
    for k in b_ok:
        np.testing.assert_array_equal(b_small[k], b_ok[k], err_msg=k)


def test_fused_activations_match_the_accessor_path():
    """render() with the model's raw parameters (activations applied inside the kernels) against render()
    through get_scaling / get_rotation / get_opacity: same images, same gradients w.r.t. the raw parameters."""
    from types import SimpleNamespace
    from lvdgs import gaussian_renderer, synthetic
    from lvdgs.gaussian_model import GaussianModel
    from lvdgs.gaussian_renderer import render
    W, H, N = 256, 160, 6000
    g = synthetic.make_gaussians(N, W, H, seed=90)
    cam = synthetic.make_camera(W, H, pose_seed=4)
    for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
        setattr(cam, k, getattr(cam, k).cuda())
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)
    gc, gd, go = (t.cuda() for t in synthetic.make_image_grads(W, H, 7))
    out = {}
    for fused in (True, False):
        gaussian_renderer.FUSE_ACTIVATIONS = fused
        try:
            model = GaussianModel.from_activated(g["means3D"], g["scales"], g["rotations"] * 1.7, g["opacities"], shs=g["shs"])
            cam.cam_rot_delta = torch.nn.Parameter(torch.zeros(3, device="cuda"))
            cam.cam_trans_delta = torch.nn.Parameter(torch.zeros(3, device="cuda"))
            pkg = render(cam, model, pipe, torch.zeros(3, device="cuda"))
            ((pkg["render"] * gc).sum() + (pkg["depth"] * gd).sum() + (pkg["opacity"] * go).sum()).backward()
            out[fused] = dict(img=pkg["render"].detach().cpu().numpy(), radii=pkg["radii"].cpu().numpy(),
                              grads=[p.grad.cpu().numpy() for p in model.parameters() if p.grad is not None],
                              tau=np.concatenate([cam.cam_trans_delta.grad.cpu().numpy(), cam.cam_rot_delta.grad.cpu().numpy()]))
        finally:
            gaussian_renderer.FUSE_ACTIVATIONS = True
    a, b = out[True], out[False]
    assert (a["radii"] != b["radii"]).mean() < 1e-3  # exp / normalise rounding may move a radius by one in rare cases
    _close(a["img"], b["img"], rtol=1e-4, atol_scale=1e-4, what="image", rel_l2=1e-4, max_rel_sig=5e-2)
    assert len(a["grads"]) == len(b["grads"]) == 5
    for x, y in zip(a["grads"], b["grads"]):
        _close(x, y, rtol=1e-3, atol_scale=1e-4, what="raw-parameter gradient", rel_l2=1e-3, max_rel_sig=5e-2)
    _close(a["tau"], b["tau"], rtol=1e-3, atol_scale=1e-4, what="tau", rel_l2=1e-3, max_rel_sig=5e-2)


@pytest.mark.parametrize("opacity_scale,r_max", [(1.0, 12.0), (0.05, 25.0)])
def test_tile_culling_changes_no_output_bit_and_without_it_the_lists_are_the_references(opacity_scale, r_max):
    """The default path lists a (Gaussian, tile) pair only when the Gaussian can reach alpha >= 1/255 somewhere on the
    tile (common.hpp: reaches_rect / rect_keeps).  LVDGS_FLAG_LIST_ALL_TILES (lvdgs_args.flags) lists every tile of the 3-sigma rectangle, as the
    reference does.  (1) Without culling the pair list, ranges and n_contrib equal the oracle's bit for bit; (2) with it
    the list is the oracle's minus pairs that provably contribute nothing (hip_runner.check_pair_lists); (3) images,
    radii and n_touched are bitwise the same in the two modes, and the gradients agree to summation-order rounding."""
    orc, hr, syn = _mods()
    W, H, N = 333, 205, 4000
    g = syn.make_gaussians(N, W, H, seed=91, r_min=0.5, r_max=r_max)
    with torch.no_grad():
        g["opacities"].mul_(opacity_scale)
    cam = syn.make_camera(W, H, pose_seed=4)
    bg = torch.tensor([0.1, 0.2, 0.3])
    grads = syn.make_image_grads(W, H, 12)
    f_on, b_on = hr.run_hip(g, cam, W, H, bg, grads=grads, tile_cull=True)
    f_off, b_off = hr.run_hip(g, cam, W, H, bg, grads=grads, tile_cull=False)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    _check_forward(f_off, f_ora, W, H)
    assert f_off["num_rendered"] == f_ora["num_rendered"]
    dropped = hr.check_pair_lists(f_on, f_ora, W, H)
    assert dropped > 0.1, dropped
    _check_forward(f_on, f_ora, W, H)
    for k in ("color", "depth", "opacity", "final_T", "radii", "n_touched"):
        np.testing.assert_array_equal(f_on[k], f_off[k], err_msg=k)
    # gradients: the same terms, but a Gaussian's place in its batch of eight decides the order its 256 pixels are
    # summed in (blend_bwd3's row rotations), and the batches differ once pairs are dropped: rounding-level differences
    for k in b_on:
        _close(b_on[k], b_off[k], rtol=1e-4, what=f"cull on/off {k}")
    _check_backward(b_off, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)
    _check_backward(b_on, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


@pytest.mark.parametrize("tile_cull", [True, False])
def test_rectangles_of_more_than_64_tiles_are_culled_by_blocks_of_tiles(tile_cull):
    """A Gaussian whose 3-sigma square spans more than 64 tiles has one mask bit per BLOCK of tiles (an 8 x 8 grid of
    blocks over its rectangle, common.hpp: RectBlocks); its gradient slots follow the kept blocks, and the grouping
    kernels walk it with a whole wave.  Round blobs keep nearly everything, long thin ones -- the footprint of a wall seen
    at a grazing angle -- lose most of their square; small Gaussians beside them are culled per tile.  All kinds in one
    scene, forward and backward against the oracle; with LVDGS_FLAG_LIST_ALL_TILES every tile is listed again."""
    orc, hr, syn = _mods()
    W, H, N = 400, 304, 600                        # 25 x 19 = 475 tiles
    g = syn.make_gaussians(N, W, H, seed=33, r_min=0.5, r_max=6.0)
    with torch.no_grad():
        for i, z in ((0, 2.0), (1, 5.0), (2, 9.0)):   # three large round ones, faint enough not to hide the rest
            g["means3D"][i] = torch.tensor([0.02 * i, -0.01 * i, z])
            g["scales"][i] = torch.tensor([0.4, 0.3, 0.2]) * z
            g["opacities"][i] = 0.15
        for i, (z, ang) in enumerate(((3.0, 0.5), (4.0, -0.9), (6.0, 1.3), (2.5, 0.1)), start=3):   # long thin ones, at an angle
            g["means3D"][i] = torch.tensor([0.1 * (i - 4), 0.05 * (5 - i), z])
            g["scales"][i] = torch.tensor([0.45, 0.012, 0.012]) * z
            g["rotations"][i] = torch.tensor([math.cos(ang / 2), 0.0, 0.0, math.sin(ang / 2)])
            g["opacities"][i] = 0.6
    cam = syn.make_camera(W, H, pose_seed=6)
    bg = torch.tensor([0.2, 0.2, 0.2])
    grads = syn.make_image_grads(W, H, 5)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads, tile_cull=tile_cull)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    big = f_ora["tiles_touched"] > 64
    assert big.sum() >= 7
    if tile_cull:
        kept = f_hip["tiles_touched"][big].astype(np.float64) / f_ora["tiles_touched"][big]
        assert kept.min() < 0.45 and kept.max() > 0.8, kept          # the thin ones lose most of their square, the round ones little
        assert (f_hip["tiles_touched"][~big] < f_ora["tiles_touched"][~big]).any()                  # culled beside them
    else:
        np.testing.assert_array_equal(f_hip["tiles_touched"], f_ora["tiles_touched"])
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)


def test_image_regions_without_gradient_add_nothing():
    """blend_bwd lets a wave sit out the lists when all 64 pixels of its quadrant receive a zero gradient (loss masks).
    Gradient images that vanish on a band and on scattered 8x8 / 16x16 blocks, against the oracle fed the same images."""
    orc, hr, syn = _mods()
    W, H, N = 200, 136, 2500
    g, cam = _scene(syn, N, W, H, 57, pose_seed=3)
    bg = torch.tensor([0.3, 0.2, 0.1])
    gc, gd, go = syn.make_image_grads(W, H, 8)
    keep = torch.ones(H, W)
    keep[:, 40:123] = 0                      # a band that covers whole tiles and cuts through others
    blocks = torch.rand(H // 8, W // 8, generator=torch.Generator().manual_seed(5)) > 0.5
    keep *= blocks.repeat_interleave(8, 0).repeat_interleave(8, 1).float()[:H, :W]
    grads = (gc * keep, gd * keep, go * keep)
    f_hip, b_hip = hr.run_hip(g, cam, W, H, bg, grads=grads)
    f_ora, b_ora = hr.run_oracle(orc, g, cam, W, H, bg, grads=grads)
    assert 0.2 < float(keep.mean()) < 0.5
    _check_forward(f_hip, f_ora, W, H)
    _check_backward(b_hip, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H)
