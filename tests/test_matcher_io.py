"""What the matcher-I/O GPU tests (tests/test_gpu_matcher_io.py) hold the HIP kernels to, checked without a GPU: the NumPy restatement of
the image formatting against PIL (tests/golden/image_format.npz, and live PIL where it imports), the host-side coefficient tables of
``lvdgs_format_table`` against the restatement's, the normalisation against torch, and the float64 oracle of ``find_scale``'s
arithmetic against what its definition asks."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import image_format_oracle as fmt
import match_scale_oracle as mso
import matcher_io_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_KINDS = [(n, k) for n in mc.FORMAT_CASES for k in mc.KINDS]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_format.npz"))


@pytest.mark.parametrize("name,kind", CASE_KINDS)
def test_format_oracle_equals_pil_byte_for_byte(golden, name, kind):
    W, H, size, raster = mc.FORMAT_CASES[name]
    q = fmt.format_bytes(fmt.quantise(mc.image(name, kind)), size)
    assert q.shape == (raster[1], raster[0], 3) and q.dtype == np.uint8
    step = int(golden[f"{name}/{kind}/step"])
    rows = golden[f"{name}/{kind}/rows"]
    assert np.array_equal(q[::step], rows), int((q[::step] != rows).sum())
    assert hashlib.sha256(q.tobytes()).hexdigest() == str(golden[f"{name}/{kind}/sha256"])
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_image_format_golden as mk
    assert np.array_equal(q, mk.pil_format(fmt.quantise(mc.image(name, kind)), size))


def test_the_cases_cover_what_they_are_named_for():
    from lvdgs import init_pose
    for name, (W, H, size, raster) in mc.FORMAT_CASES.items():
        w, h, filt, x0, y0, W1, H1 = fmt.plan(W, H, size)
        assert (W1, H1) == raster == init_pose.matcher_raster(W, H, size), name
    assert fmt.plan(300, 90, 64)[2] == fmt.LANCZOS and 300 / 64 > 4.6
    co = fmt.coefficients(300, 64, fmt.LANCZOS)
    assert co[0][0] == 0 and len(co[0][1]) < len(co[32][1]) and co[-1][0] + len(co[-1][1]) == 300 and len(co[-1][1]) < len(co[32][1])   # clipped at both borders
    assert fmt.plan(97, 61, 128)[2] == fmt.BICUBIC and fmt.plan(50, 50, 64)[:2] == (64, 64)
    assert fmt.plan(512, 160, 512)[:2] == (512, 160) and fmt.plan(511, 300, 512)[:2] == (512, 301)
    x0, y0 = fmt.plan(200, 75, 90)[3:5]
    assert x0 % 2 == 1 and y0 % 2 == 1
    with pytest.raises(ValueError):
        fmt.plan(640, 480, 224)
    img = mc.image("square_rule", "noise")
    q = fmt.quantise(img)
    assert q[0, 0, 0] == 0 and q[25, 16, 1] == 255 and q[49, 49, 2] == 0 and q[16, 25, 0] == 255    # below 0, above 1, NaN, far above


def test_normalisation_equals_torch_bitwise():
    q = np.arange(256, dtype=np.uint8)
    want = (torch.from_numpy(q).float() / 255 - 0.5) / 0.5
    assert fmt.normalise(q).tobytes() == want.numpy().tobytes()
    via_ops = torch.from_numpy(q).float().div(255).sub_(0.5).div_(0.5)       # ToTensor + Normalize, as torchvision applies them
    assert fmt.normalise(q).tobytes() == via_ops.numpy().tobytes()


@pytest.mark.parametrize("name", list(mc.FORMAT_CASES))
def test_host_tables_and_plan_equal_the_oracle(name):
    """``lvdgs_format_plan_query`` and ``lvdgs_format_table`` run on the host: the raster, the crop and every integer coefficient are
    the restatement's (and so PIL's)."""
    from lvdgs import _lib
    L = _lib.lib()
    W, H, size, _ = mc.FORMAT_CASES[name]
    w, h, filt, x0, y0, W1, H1 = fmt.plan(W, H, size)
    p = _lib.FormatPlan()
    assert L.lvdgs_format_plan_query(W, H, size, C.byref(p)) == _lib.OK
    assert (p.resized_width, p.resized_height, p.crop_x, p.crop_y, p.out_width, p.out_height) == (w, h, x0, y0, W1, H1)
    assert p.filter == (_lib.FORMAT_LANCZOS if filt == fmt.LANCZOS else _lib.FORMAT_BICUBIC)
    rows = []
    for n_in, n_out, first, count, taps in ((W, w, x0, W1, p.taps_x), (H, h, y0, H1, p.taps_y)):
        t = np.full((count, 2 + taps), -7, dtype=np.int32)
        assert L.lvdgs_format_table(n_in, n_out, p.filter, first, count, t.ctypes.data) == _lib.OK
        if n_in == n_out:
            assert taps == 1 and np.array_equal(t[:, 0], np.arange(first, first + count)) and (t[:, 1] == 1).all() and (t[:, 2] == 1 << 22).all()
        else:
            co = fmt.coefficients(n_in, n_out, filt)
            assert taps >= max(len(k) for _, k in co)
            for j in range(count):
                xmin, k = co[first + j]
                assert t[j, 0] == xmin and t[j, 1] == len(k) and np.array_equal(t[j, 2:2 + len(k)], k) and not t[j, 2 + len(k):].any(), (name, j)
        rows.append((int(t[:, 0].min()), int((t[:, 0] + t[:, 1]).max())))
    assert (p.row_first, p.row_first + p.row_count) == rows[1]
    assert L.lvdgs_format_scratch_bytes(W, H, size) >= 3 * p.row_count * W1


def test_host_side_refusals():
    from lvdgs import _lib
    L = _lib.lib()
    p = _lib.FormatPlan()
    for (W, H, size), word in (((640, 480, 224), b"224"), ((0, 480, 512), b"image size"), ((640, 480, 8), b"size 8"),
                               ((640, 480, _lib.FORMAT_MAX_SIZE + 1), b"outside"), ((_lib.FORMAT_MAX_EDGE + 1, 480, 512), b"edge"),
                               ((4000, 20, 512), b"empty raster")):
        assert L.lvdgs_format_plan_query(W, H, size, C.byref(p)) == _lib.E_INVALID and word in L.lvdgs_last_error(), (W, H, size, L.lvdgs_last_error())
        assert L.lvdgs_format_scratch_bytes(W, H, size) == 0
    assert L.lvdgs_format_plan_query(640, 480, 512, None) == _lib.E_INVALID
    t = np.zeros(64, dtype=np.int32)
    assert L.lvdgs_format_table(0, 4, _lib.FORMAT_LANCZOS, 0, 1, t.ctypes.data) == _lib.E_INVALID
    assert L.lvdgs_format_table(8, 4, 5, 0, 1, t.ctypes.data) == _lib.E_INVALID and b"filter" in L.lvdgs_last_error()
    assert L.lvdgs_format_table(8, 4, _lib.FORMAT_LANCZOS, 3, 2, t.ctypes.data) == _lib.E_INVALID and b"outside" in L.lvdgs_last_error()
    assert L.lvdgs_format_table(8, 4, _lib.FORMAT_LANCZOS, 0, 1, None) == _lib.E_INVALID and not t.any()
    assert L.lvdgs_format_image(None, None) == _lib.E_INVALID and L.lvdgs_match_depth_scale(None, None) == _lib.E_INVALID


# ----------------------------------------------------------------------------------------------- the scale oracle
def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("shape", [(185, 613), (30, 100)])
def test_scale_oracle_recovers_a_known_scale(shape):
    """depth2 = depth1 / s sampled at the same places gives s to float32, whether the maps shrink (613 x 185) or grow (100 x 30) on
    their way to the 512 x 144 raster.  (depth2 is rounded to float32 pixel by pixel: 6e-8 relative each, averaged over 1152 samples.)"""
    s = 1.37
    d1, d2 = mc.scaled_pair(*shape, s)
    m1, m2 = mc.grid_matches(stride=8)
    o = mso.match_scale(m1, m2, d1, d2, mc.RASTER)
    assert o["status"] == mso.OK and o["valid"] == len(m1) == 1152
    assert ulps(o["scale"], np.float32(s)) <= 1, (o["scale"], s)


def test_scale_oracle_borders_and_outside():
    d1, d2 = mc.depth_map(185, 613, 1), mc.depth_map(90, 300, 2)
    m1, m2, inside = mc.border_matches()
    o = mso.match_scale(m1, m2, d1, d2, mc.RASTER)
    assert np.array_equal(o["mask"], inside) and o["valid"] == int(inside.sum())
    W1, H1 = mc.RASTER
    corner = np.array([0, W1 - 1]), np.array([0, H1 - 1])
    small = mc.depth_map(30, 100, 3)                                                      # upsizing: both raster corners fall outside the sample centres
    got = mso.sample(small, corner[0], corner[1], mc.RASTER)
    assert got[0] == np.float64(small[0, 0]) and got[1] == np.float64(small[-1, -1])     # the clamped branch: the corner samples themselves
    assert mso.match_scale(m1[~inside], m2[~inside], d1, d2, mc.RASTER)["scale"] is None
    none = mso.match_scale(np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), d1, d2, mc.RASTER)
    assert none["status"] == mso.NO_VALID and none["scale"] is None and none["valid"] == 0
    zero = mso.match_scale(*mc.grid_matches(), np.zeros_like(d1), d2, mc.RASTER)
    assert zero["status"] == mso.NO_VALID and zero["scale"] is None
    inf = d1.copy()
    inf[:] = np.inf
    assert mso.match_scale(*mc.grid_matches(), inf, d2, mc.RASTER)["valid"] == 0          # +inf is not a depth (deviation from the reference)


def test_scale_oracle_with_holes_and_under_permuted_sums():
    """30 % zeros in one map, 5 % NaNs in the other: a match whose bilinear window touches a NaN, or whose sample is 0, is dropped.  The
    float32 scale does not depend on the order of the float64 sums: 50 permutations, one result, clean and holed."""
    d1, d2 = mc.depth_map(185, 613, 3), mc.depth_map(185, 613, 4)
    m1, m2 = mc.grid_matches(jitter=3.0, seed=5)
    m1, m2 = np.concatenate([m1, mc.border_matches()[0]]), np.concatenate([m2, mc.border_matches()[1]])
    for a, b in ((d1, d2), mc.holes(d1, d2, 6)):
        o = mso.match_scale(m1, m2, a, b, mc.RASTER)
        assert 0 < o["valid"] <= len(m1) - 9 and np.isfinite(o["scale"])
        seen = set()
        for k in range(50):
            perm = np.random.default_rng(k).permutation(o["valid"])
            seen.add(mso.match_scale(m1, m2, a, b, mc.RASTER, order=perm)["scale"].tobytes())
        seen.add(o["scale"].tobytes())
        assert len(seen) == 1
    clean, holed = mso.match_scale(m1, m2, d1, d2, mc.RASTER)["valid"], o["valid"]
    assert holed < 0.95 * clean


def test_nearest_rule():
    z = np.arange(6 * 10, dtype=np.float32).reshape(6, 10)
    up = mso.nearest_resize(z, 25, 13)
    assert up.shape == (13, 25) and up[0, 0] == z[0, 0] and up[-1, -1] == z[-1, -1]
    assert np.array_equal(up[:, 3], z[(np.arange(13) * 6) // 13, (3 * 10) // 25])
    assert np.array_equal(mso.nearest_resize(z, 10, 6), z)
    down = mso.nearest_resize(z, 4, 3)
    assert np.array_equal(down, z[[0, 2, 4]][:, [0, 2, 5, 7]])
