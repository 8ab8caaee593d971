"""CPU side of the frame statistics (lvdgs_edge_mask, lvdgs_frame_summary; lvdgs.frame_stats): the NumPy oracle that pins the
kernels' arithmetic (tests/frame_stats_oracle.py) against the PyTorch statements it stands for, and the library's ABI and argument
validation without a GPU.  The kernels themselves: tests/test_gpu_frame_stats.py."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frame_stats_cases as cases
import frame_stats_oracle as oracle
from lvdgs import _lib
from lvdgs.camera_utils import Camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvdgs.h")
NEW_SYMBOLS = ("lvdgs_edge_mask_scratch_bytes", "lvdgs_edge_mask", "lvdgs_frame_summary_scratch_bytes", "lvdgs_frame_summary")


def torch_grad_mask(image, edge_threshold, dataset_type):
    """``Camera.compute_grad_mask`` as it stands (the CPU's conv2d path) on a NumPy image."""
    cam = SimpleNamespace(original_image=torch.from_numpy(image), grad_mask=None)
    Camera.compute_grad_mask(cam, {"Training": {"edge_threshold": edge_threshold}, "Dataset": {"type": dataset_type}})
    return cam.grad_mask.numpy()


@pytest.mark.parametrize("H,W", cases.MEDIAN_SIZES)
def test_oracle_mask_is_compute_grad_mask(H, W):
    img = cases.image(H, W)
    got = oracle.edge_mask_median(img, cases.EDGE_THRESHOLD)
    want = torch_grad_mask(img, cases.EDGE_THRESHOLD, "kitti")
    print(f"{H}x{W}: set {got['mask'].mean():.3f}, differing pixels {(got['mask'][None] != want).sum()}, invalid share {(got['mag'] == 0).mean():.3f}")
    assert want.dtype == bool and want.shape == (1, H, W)
    assert np.array_equal(got["mask"][None], want)
    assert 0.2 < got["mask"].mean() < 0.6 and (got["mag"] == 0).mean() > 0.03      # a real mask, and a real share of invalid pixels


@pytest.mark.parametrize("H,W", cases.BLOCK_SIZES)
@pytest.mark.parametrize("thr,gain", [(1.1, 1.0), (0.5, 1.0), (1.1, 40.0)])
def test_oracle_block_rule_is_the_replica_branch(H, W, thr, gain):
    img = cases.image(H, W, gain=gain)
    got = oracle.edge_mask_blocks(img, thr)
    want = torch_grad_mask(img, thr, "replica")
    assert want.dtype == np.float32 and want.shape == (1, H, W)
    bh, bw = H // 32, W // 32
    # inside the grid both hold zeros and ones: identical.  Outside it both keep the raw magnitude, which conv2d sums in another
    # order than the header fixes: a dozen float32 roundings of partial sums of at most 32 max|p| before the 1/32, and max|p| is
    # about `gain` -- under 2e-6 gain.
    assert np.array_equal(got["mask"][:32 * bh, :32 * bw].view(np.uint32), want[0, :32 * bh, :32 * bw].view(np.uint32))
    assert set(np.unique(got["mask"][:32 * bh, :32 * bw]).tolist()) <= {0.0, 1.0}
    assert np.abs(got["mask"] - want[0]).max() <= 2e-6 * gain
    if gain > 1.0:      # the quirk: blocks whose cut reaches 1 are cleared altogether, the others are not
        high = got["cuts"] >= 1.0
        assert high.any() and (~high).any()
        i, j = np.argwhere(high)[0]
        assert not got["mask"][i * bh:(i + 1) * bh, j * bw:(j + 1) * bw].any()
    else:
        assert (got["cuts"] < 1.0).all() and (got["mask"] == 1.0).any()
    if H % 32 or W % 32:      # outside the grid: the raw magnitude
        assert np.array_equal(got["mask"][32 * (H // 32):], got["mag"][32 * (H // 32):])
        assert np.array_equal(got["mask"][:, 32 * (W // 32):], got["mag"][:, 32 * (W // 32):])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257])
def test_oracle_median_is_torch_median(n):
    for pattern in cases.SELECT_PATTERNS:
        d = cases.depths(pattern, n)
        got, want = oracle.lower_median(d), torch.from_numpy(d).median().numpy()
        assert got.dtype == np.float32
        assert (np.isnan(got) and np.isnan(want)) if n == 0 else got.view(np.uint32) == want.view(np.uint32), (pattern, n)


def test_oracle_summary_is_get_median_depth_and_covisibility():
    from lvdgs.keyframe_utils import covisibility
    from lvdgs.slam_utils import get_median_depth
    n, N = 257, 65
    d, o = cases.depths("random", n), cases.opacities("third", n)
    m = cases.visibility("random", n, seed=5)
    touched = (cases.visibility("random", N, seed=1) * 3).astype(np.int32)
    rows = [cases.visibility(k, N, seed=2) for k in ("random", "true", "false")]
    got = oracle.summary(d, o, touched, rows, mask=m, count_mask=m)
    want = get_median_depth(torch.from_numpy(d), torch.from_numpy(o), torch.from_numpy(m))
    assert got["median"].view(np.uint32) == want.numpy().view(np.uint32) and got["selected"] == int(((d > 0) & (o > np.float32(0.95)) & m).sum())
    for r, row in enumerate(rows):
        inter, union, n_cur, n_kf = covisibility(torch.from_numpy(touched > 0), torch.from_numpy(row).long())
        assert got["rows"][r] == (inter, union, n_kf) and got["visible"] == n_cur
    assert got["mask_count"] == int(m.sum())


# ---------------------------------------------------------------- the library without a GPU
def test_header_declares_and_library_exports_the_new_symbols():
    declared = set(re.findall(r"\b(lvdgs_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert 4 * (_lib.FRAME_SUMMARY_ROWS + 3 * _lib.FRAME_SUMMARY_MAX_ROWS) <= _lib.FRAME_SUMMARY_HOST_BYTES


def _refused(status, want):
    msg = _lib.lib().lvdgs_last_error()
    assert status == want and len(msg) > 0, (status, want, msg)
    return msg


def test_edge_mask_refusals_without_gpu():
    L = _lib.lib()
    assert L.lvdgs_edge_mask_scratch_bytes(1, 64) == 0 and L.lvdgs_edge_mask_scratch_bytes(64, 1) == 0
    need = L.lvdgs_edge_mask_scratch_bytes(1226, 370)
    assert need % 256 == 0 and need >= 4 * 1226 * 370 + 4 * 4 * 256
    p = C.c_void_p(256)      # never dereferenced: every call below is refused before a launch
    ok = dict(width=64, height=48, mode=_lib.EDGE_MASK_MEDIAN, edge_threshold=1.1, image=p, mask=p, scratch=p, scratch_bytes=1 << 20)
    call = lambda **kw: L.lvdgs_edge_mask(C.byref(_lib.EdgeMaskArgs(**{**ok, **kw})), None)
    _refused(L.lvdgs_edge_mask(None, None), _lib.E_INVALID)
    assert b"mode" in _refused(call(mode=2), _lib.E_INVALID)
    for w, h in ((1, 48), (64, 1), (0, 0), (-5, 48)):
        assert b"image size" in _refused(call(width=w, height=h), _lib.E_RANGE)
    assert b"image size" in _refused(call(width=65536, height=65536), _lib.E_RANGE)
    for w, h in ((31, 48), (64, 31)):
        assert b"grid" in _refused(call(width=w, height=h, mode=_lib.EDGE_MASK_BLOCKS), _lib.E_RANGE)
        assert call(width=w, height=h, scratch_bytes=0) == _lib.E_INVALID      # (fine for the whole-image rule, but for its scratch)
    for name in ("image", "mask", "scratch"):
        assert b"NULL" in _refused(call(**{name: None}), _lib.E_INVALID)
    assert b"scratch too small" in _refused(call(scratch_bytes=L.lvdgs_edge_mask_scratch_bytes(64, 48) - 1), _lib.E_INVALID)


def test_frame_summary_refusals_without_gpu():
    L = _lib.lib()
    need = L.lvdgs_frame_summary_scratch_bytes()
    assert need % 256 == 0 and need >= 4 * 4 * 256
    p = C.c_void_p(256)      # never dereferenced
    rows = (C.c_void_p * _lib.FRAME_SUMMARY_MAX_ROWS)(*([256] * _lib.FRAME_SUMMARY_MAX_ROWS))
    ok = dict(num_pixels=100, num_gaussians=10, num_rows=3, seq=1, opacity_bar=0.95, depth=p, opacity=p, n_touched=p, rows=rows,
              host_state=p, scratch=p, scratch_bytes=need)
    call = lambda **kw: L.lvdgs_frame_summary(C.byref(_lib.FrameSummaryArgs(**{**ok, **kw})), None)
    _refused(L.lvdgs_frame_summary(None, None), _lib.E_INVALID)
    assert b"rows" in _refused(call(num_rows=17), _lib.E_RANGE)
    assert b"rows" in _refused(call(num_rows=-1), _lib.E_RANGE)
    assert b"negative" in _refused(call(num_gaussians=-1), _lib.E_RANGE)
    assert b"negative" in _refused(call(num_pixels=-1), _lib.E_RANGE)
    for name in ("host_state", "scratch", "depth", "n_touched"):
        assert b"NULL" in _refused(call(**{name: None}), _lib.E_INVALID), name
    holed = (C.c_void_p * _lib.FRAME_SUMMARY_MAX_ROWS)(256, None, 256)
    assert b"row 1 is NULL" in _refused(call(rows=holed), _lib.E_INVALID)
    assert b"scratch too small" in _refused(call(scratch_bytes=need - 1), _lib.E_INVALID)


def test_python_entry_points_refuse_cpu_tensors():
    from lvdgs import frame_stats
    with pytest.raises(_lib.LvdgsError):
        frame_stats.edge_mask(torch.zeros(3, 8, 8), 1.1, "kitti")
    with pytest.raises(_lib.LvdgsError):
        frame_stats.frame_summary(dict(depth=torch.zeros(1, 4, 4), opacity=torch.zeros(1, 4, 4), n_touched=torch.zeros(3, dtype=torch.int32)), {})


def test_keyframe_functions_take_the_counts_instead_of_the_rows():
    """``covis=`` / ``mask_share=`` replace the reads: the visibility arguments may then be anything."""
    from lvdgs.keyframe_utils import add_to_window, covisibility, is_keyframe
    cfg = {"Training": dict(kf_translation=0.08, kf_min_translation=0.05, kf_overlap=0.9, window_size=3, kf_cutoff=0.3)}
    rng = np.random.default_rng(0)
    cams = {}
    for i in range(5):
        cams[i] = SimpleNamespace(R=torch.eye(3), T=torch.tensor([0.0, 0.0, 0.3 * i]))
    cams[4].expanded_static_mask = torch.from_numpy(rng.random((6, 7)) < 0.25)
    cur = torch.from_numpy(cases.visibility("random", 200, seed=9)).long()
    occ = {i: torch.from_numpy(cases.visibility("random", 200, seed=10 + i)).long() for i in range(4)}
    covis = {i: covisibility(cur, occ[i]) for i in occ}
    share = float(cams[4].expanded_static_mask.float().mean())
    for last in range(4):
        for md in (0.5, 5.0, 50.0):
            assert is_keyframe(cfg, cams, 4, last, cur, occ, md) == is_keyframe(cfg, cams, 4, last, None, None, md, covis=covis, mask_share=share)
    for window in ([3, 2, 1, 0], [3, 2], [3, 1, 0]):
        assert add_to_window(cfg, cams, 4, cur, occ, window) == add_to_window(cfg, cams, 4, None, None, window, covis=covis)
