"""CPU side of the fused seeding (lvdgs_seed_points; lvdgs.seeding): the NumPy oracle's invariants (tests/seeding_oracle.py), the
uniformity of the selection rule, and the library's ABI and argument validation without a GPU.  The kernels themselves:
tests/test_gpu_seeding.py."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seeding_cases as cases
import seeding_oracle as oracle
from lvdgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvdgs.h")
NEW_SYMBOLS = ("lvdgs_seed_scratch_bytes", "lvdgs_seed_points")


# ---------------------------------------------------------------- the oracle's invariants
@pytest.mark.parametrize("W,H", [(23, 37), (1226, 370), (1920, 1080)])
def test_keys_of_an_image_are_distinct(W, H):
    from lvdgs.seeding import call_seed
    for c in (0, 1):
        k = oracle.keys(W * H, call_seed(0, c))
        assert k.dtype == np.uint32 and np.unique(k).size == W * H


@pytest.mark.parametrize("ds", [1, 3, 32, 64])
def test_count_order_and_validity_of_the_selection(ds):
    from lvdgs.seeding import call_seed
    W, H = 211, 97
    d = cases.depth_map(W, H)
    valid = oracle.valid_mask(d)
    got = oracle.select(d, 1.0 / ds, call_seed(5, ds))
    assert got["n_valid"] == int(valid.sum()) and 0.5 < valid.mean() < 0.7
    assert got["n_keep"] == int(got["n_valid"] * (1.0 / ds)) == got["pixel"].size > 0
    assert np.all(np.diff(got["pixel"]) > 0)
    assert valid[got["pixel"]].all()
    flat = d.reshape(-1)
    special = {float(v): int(np.flatnonzero(flat == np.float32(v))[0]) for v in cases.SPECIALS if v == v and v not in (0.0,)}
    assert valid[special[100.0]] and not valid[special[cases.SPECIALS[1]]] and not valid[special[float("inf")]] and not valid[special[-1.0]]
    assert not valid[np.flatnonzero(np.isnan(flat))].any()
    if ds == 1:      # everything valid is kept, in raster order
        assert np.array_equal(got["pixel"], np.flatnonzero(valid))


def test_selection_is_uniform_over_pixels_and_neighbours():
    """48 x 64, all valid (P = 3072), a quarter kept, over the 512 consecutive call seeds call_seed(0, c): per pixel the selection
    count is Binomial(S, p)-like; z = (count - S p) / sqrt(S p (1 - p)).  Conditions: max |z| <= 5; |sum z^2 - P| <= 4 sqrt(2 P) (a
    chi-square with ~P degrees); the same max |z| for the co-selection of horizontally adjacent pixels against its hypergeometric
    mean S p (n_keep - 1) / (P - 1)."""
    from lvdgs.seeding import call_seed
    H, W, S = 48, 64, 512
    P, inv = H * W, 0.25
    d = np.ones((H, W), np.float32)
    count = np.zeros(P)
    pair = np.zeros((H, W - 1))
    n_keep = int(P * inv)
    for c in range(S):
        got = oracle.select(d, inv, call_seed(0, c))
        assert got["n_keep"] == n_keep
        sel = np.zeros(P, bool)
        sel[got["pixel"]] = True
        count += sel
        s2 = sel.reshape(H, W)
        pair += s2[:, 1:] & s2[:, :-1]
    p = n_keep / P
    z = (count - S * p) / np.sqrt(S * p * (1 - p))
    pp = p * (n_keep - 1) / (P - 1)
    zp = (pair - S * pp) / np.sqrt(S * pp * (1 - pp))
    print(f"max |z| {np.abs(z).max():.2f}, sum z^2 {np.sum(z * z):.0f} (P = {P}, allowed +- {4 * np.sqrt(2 * P):.0f}), adjacent pairs max |z| {np.abs(zp).max():.2f}")
    assert np.abs(z).max() <= 5
    assert abs(np.sum(z * z) - P) <= 4 * np.sqrt(2 * P)
    assert np.abs(zp).max() <= 5


@pytest.mark.parametrize("W,H", cases.SIZES[:2])
def test_marked_depth_map_has_a_negative_median_that_torch_agrees_on(W, H):
    d = cases.marked_depth_map(W, H)
    want = oracle.lower_median(d)
    assert not np.isnan(d).any() and np.isinf(d).any() and (d == -1.0).any() and np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
    assert want < 0 and want != -1.0 and 0.5 < (d < 0).mean() < 0.6
    assert float(torch.from_numpy(d).median()) == float(want)
    assert 0.2 < oracle.valid_mask(d).mean() < 0.5      # and there is something to seed


def test_call_seed_is_a_splitmix64_step():
    from lvdgs.seeding import call_seed
    # SplitMix64's first output for the seeds 0 and 1234567, and its second for the seed 0 (the state after one step is the increment)
    assert call_seed(0, 0) == 0xE220A8397B1DCDAF
    assert call_seed(1234567, 0) == 6457827717110365317
    assert call_seed(0, 0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4 == call_seed(0x9E3779B97F4A7C15, 0)
    assert call_seed((1 << 64) - 1, 1) == call_seed(0, 0)      # modulo 2^64
    for b, c in ((0, 0), (0, 1), (7, 5), (1 << 63, 3)):
        assert call_seed(b, c) == oracle.splitmix64((b + c) & oracle.MASK64)


def test_oracle_colours_are_the_torch_statements_with_the_gpu_division():
    """PyTorch's `x / 255.0` multiplies by the float32 reciprocal on a GPU and divides on a CPU; apart from that step the oracle is the
    model's statements."""
    img = cases.image(40, 30)
    pixel = np.arange(0, 1200, 7)
    rgb, f_dc = oracle.colours(img, pixel, cases.GAIN, cases.OFFSET)
    ab = (torch.tensor(np.float32(cases.GAIN)) * torch.from_numpy(img) + torch.tensor(np.float32(cases.OFFSET))).clamp(0.0, 1.0)
    q = (ab * 255).to(torch.uint8)
    want = q.to(torch.float32) * torch.tensor(np.float32(1) / np.float32(255))
    assert np.array_equal(rgb.view(np.uint32), want.reshape(3, -1)[:, pixel].t().contiguous().numpy().view(np.uint32))
    assert set(np.unique(q.numpy()).tolist()) >= {0, 255} and len(np.unique(q.numpy())) > 100
    assert np.allclose(f_dc, (rgb - 0.5) / 0.28209479177387814, rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------- the library without a GPU
def test_header_declares_and_library_exports_the_new_symbols():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(lvdgs_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert 4 * (_lib.SEED_THRESHOLD + 1) <= _lib.SEED_HOST_BYTES


def _refused(status, want):
    msg = _lib.lib().lvdgs_last_error()
    assert status == want and len(msg) > 0, (status, want, msg)
    return msg


def test_seed_points_refusals_without_gpu():
    L = _lib.lib()
    assert L.lvdgs_seed_scratch_bytes(0, 8) == 0 and L.lvdgs_seed_scratch_bytes(8, -1) == 0 and L.lvdgs_seed_scratch_bytes(65536, 65536) == 0
    need = L.lvdgs_seed_scratch_bytes(1226, 370)
    assert need % 256 == 0 and need >= 2 * 4 * 4 * 256
    p = C.c_void_p(256)      # never dereferenced: every call below is refused before a launch
    ok = dict(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, depth_trunc=100.0, want_median=1, inv_downsample=1.0 / 8, seed=1,
              seq=1, capacity=64 * 48 // 8, image=p, gain=p, offset=p, depth=p, R=p, T=p, xyz=p, rgb=p, f_dc=p, pixel=p, host_state=p,
              scratch=p, scratch_bytes=need)
    call = lambda **kw: L.lvdgs_seed_points(C.byref(_lib.SeedArgs(**{**ok, **kw})), None)
    _refused(L.lvdgs_seed_points(None, None), _lib.E_INVALID)
    for w, h in ((0, 48), (64, 0), (-3, 48), (65536, 65536)):
        assert b"image size" in _refused(call(width=w, height=h), _lib.E_RANGE)
    for inv in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert b"inv_downsample" in _refused(call(inv_downsample=inv), _lib.E_RANGE)
    assert b"capacity" in _refused(call(capacity=64 * 48 // 8 - 1), _lib.E_RANGE)
    assert b"capacity" in _refused(call(inv_downsample=1.0, capacity=64 * 48 - 1), _lib.E_RANGE)
    for name in ("depth", "R", "T", "xyz", "host_state", "scratch"):
        assert b"NULL" in _refused(call(**{name: None}), _lib.E_INVALID), name
    for name in ("rgb", "f_dc"):
        assert b"with an image" in _refused(call(**{name: None}), _lib.E_INVALID), name
    assert b"scratch too small" in _refused(call(scratch_bytes=need - 1), _lib.E_INVALID)


def test_seed_points_refuses_cpu_tensors():
    from lvdgs import seeding
    R, T = cases.pose()
    with pytest.raises(_lib.LvdgsError):
        seeding.seed_points(torch.zeros(3, 8, 8), torch.ones(8, 8), cases.INTRINSICS, torch.from_numpy(R), torch.from_numpy(T), 4, 1)


def test_fused_model_on_the_cpu_runs_the_host_statements(monkeypatch):
    """``seeding = "fused"`` away from a GPU: the host path, the same draw from the same generator (the kNN stands in: it has no CPU path)."""
    from lvdgs import simple_knn
    from lvdgs.gaussian_model import GaussianModel
    monkeypatch.setattr(simple_knn, "distCUDA2", lambda xyz: torch.ones(xyz.shape[0]))
    W, H = 40, 30
    R, T = cases.pose()
    cam = SimpleNamespace(original_image=torch.from_numpy(cases.image(W, H)), exposure_a=torch.tensor([0.08]), exposure_b=torch.tensor([-0.02]),
                          image_height=H, image_width=W, fx=50.0, fy=50.0, cx=20.0, cy=15.0, R=torch.from_numpy(R), T=torch.from_numpy(T), depth=None)
    cfg = {"Dataset": {"sensor_type": "depth", "pcd_downsample": 4, "pcd_downsample_init": 2, "point_size": 0.05, "adaptive_pointsize": True}}
    depth = cases.depth_map(W, H, specials=False)
    outs = {}
    for mode in ("host", "fused"):
        m = GaussianModel(0, config=cfg, device="cpu")
        assert (m.seeding, m.seed_base, m.seed_calls) == ("host", 0, 0)
        m.seeding = mode
        outs[mode] = m.create_pcd_from_image(cam, init=False, depthmap=depth)
        assert m.seed_calls == 0
    assert outs["host"][0].shape[0] == int(oracle.valid_mask(depth).sum() * 0.25)
    for a, b in zip(outs["host"], outs["fused"]):
        assert torch.equal(a, b)
    m.seeding = "device"
    with pytest.raises(ValueError):
        m.create_pcd_from_image(cam, init=False, depthmap=depth)
