"""Frame evaluation without a GPU: the statement-level oracle (tests/frame_eval_oracle.py) against the fixture made by the reference's
own ``eval_rendering`` (tests/golden/make_eval_golden.py), the loop logic of ``eval_utils.eval_rendering`` with an injected per-frame
metrics function, and the C ABI of ``lvdgs_frame_eval`` (scratch size, argument validation)."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frame_eval_oracle as feo
from frame_eval_oracle import check_means, load_fixture
from lvdgs import _lib



def test_the_fixture_covers_the_cases(golden_dir):
    fx = load_fixture(golden_dir)
    fr = {f["idx"]: f for f in fx["frames"]}
    assert sorted(fr) == [i for i in range(fx["num_frames"] - 1) if i not in fx["kf_indices"]]
    assert any(f["used_mask"] is None for f in fx["frames"])
    assert any(f["static_mask"] is not None and f["expanded_static_mask"] is None for f in fx["frames"])
    assert any(f["static_mask"] is not None and f["expanded_static_mask"] is not None for f in fx["frames"])
    assert any(f["used_mask"] is not None and not f["used_mask"].any() for f in fx["frames"])
    for f in fx["frames"]:
        black = f["gt"] == 0
        assert (black.sum(0) == 1).any() and (black.sum(0) == 3).any()      # black in single channels, and black pixels
        assert f["render"].min() < 0 and f["render"].max() > 1
    assert fx["json"] == fx["result"]
    assert np.any(fx["background"] != 0)


def test_oracle_reproduces_the_reference_fixture(golden_dir):
    fx = load_fixture(golden_dir)
    rows = []
    for f in fx["frames"]:
        o = feo.frame_eval(f["render"], f["gt"], f["used_mask"], fx["background"], f["depth"])
        assert np.array_equal(o["pred8"], f["png_rgb"]), f["idx"]
        assert np.array_equal(o["depth8"], f["png_depth"]), f["idx"]
        assert np.array_equal(f["npy_depth"], np.asarray(f["depth"]).squeeze()), f["idx"]
        rows.append(feo.metrics(o, f["gt"].size))
    check_means(rows, fx["result"])
    none = [r for r, f in zip(rows, fx["frames"]) if f["used_mask"] is not None and not f["used_mask"].any()]
    assert none and all(r["static_ratio"] is None and r["psnr_static"] == r["psnr"] for r in none)


# ---------------------------------------------------------------- the loop of eval_utils.eval_rendering
def _loop_case(n=7, masks=True):
    H, W = 6, 8
    g = torch.Generator().manual_seed(3)
    frames = {i: SimpleNamespace(uid=i, static_mask=None, expanded_static_mask=None) for i in range(n)}
    if masks:
        frames[1].static_mask = torch.ones(H, W, dtype=torch.bool)
        frames[2].static_mask = torch.ones(H, W, dtype=torch.bool)
        frames[2].expanded_static_mask = torch.zeros(H, W, dtype=torch.bool)
        frames[4].expanded_static_mask = torch.zeros(H, W, dtype=torch.bool)      # ignored: static_mask is None
    dataset = [(torch.rand(3, H, W, generator=g), None, None, None) for _ in range(n)]
    rendered = []

    def render_fn(frame, gaussians, pipe, background):
        rendered.append(frame.uid)
        return {"render": torch.rand(3, H, W, generator=g) * 1.4 - 0.2, "depth": torch.rand(1, H, W, generator=g) + frame.uid}
    return frames, dataset, render_fn, rendered


def test_eval_rendering_loop_logic(tmp_path):
    from lvdgs.eval_utils import eval_rendering
    frames, dataset, render_fn, rendered = _loop_case()
    seen = []

    def metrics_fn(rendering, gt_image, static_mask, background):
        i = len(seen)
        seen.append(static_mask)
        masked = static_mask is not None and bool(static_mask.any())
        return {"psnr": 10.0 + i, "ssim": 0.1 * i, "psnr_static": 20.0 + i if masked else 10.0 + i, "ssim_static": 0.5 if masked else 0.1 * i,
                "static_ratio": 0.5 if masked else None}
    out = eval_rendering(frames, None, dataset, str(tmp_path), None, torch.zeros(3), "monocular", [0, 3], "before_opt", render_fn=render_fn,
                         metrics_fn=metrics_fn, save_images=True)
    assert rendered == [1, 2, 4, 5]      # keyframes 0 and 3 skipped; end_idx = len(frames) - 1 = 6 is exclusive, whatever `iteration` is
    assert seen[0] is frames[1].static_mask and seen[1] is frames[2].expanded_static_mask and seen[2] is None and seen[3] is None
    assert set(out) == {"mean_psnr", "mean_ssim", "mean_psnr_static", "mean_ssim_static"}      # no lpips_fn: no LPIPS keys
    assert out["mean_psnr"] == pytest.approx(np.mean([10, 11, 12, 13])) and out["mean_ssim"] == pytest.approx(0.15)
    assert out["mean_psnr_static"] == pytest.approx(np.mean([20, 11, 12, 13])) and out["mean_ssim_static"] == pytest.approx(np.mean([0.5, 0.1, 0.2, 0.3]))
    with open(tmp_path / "psnr" / "before_opt" / "final_result.json") as f:
        assert json.load(f) == out
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs)
    want = ["psnr/before_opt/final_result.json"] + [f"{sub}/{i}_pred.{ext}" for sub, ext in
                                                    (("render_depth", "png"), ("render_depth_npy", "npy"), ("render_rgb", "png")) for i in (1, 2, 4, 5)]
    assert files == sorted(want)
    from PIL import Image
    assert np.array(Image.open(tmp_path / "render_rgb" / "4_pred.png")).shape == (6, 8, 3)
    assert np.array(Image.open(tmp_path / "render_depth" / "4_pred.png")).dtype == np.uint8
    assert np.load(tmp_path / "render_depth_npy" / "4_pred.npy").shape == (6, 8)


def test_eval_rendering_static_means_fall_back_and_lpips_keys(tmp_path):
    from lvdgs.eval_utils import eval_rendering
    frames, dataset, render_fn, rendered = _loop_case(masks=False)
    metrics_fn = lambda r, g, m, b: {"psnr": float(len(rendered)), "ssim": 0.5, "psnr_static": float(len(rendered)), "ssim_static": 0.5, "static_ratio": None}
    out = eval_rendering(frames, None, dataset, str(tmp_path), None, torch.zeros(3), "monocular", [0], render_fn=render_fn, metrics_fn=metrics_fn,
                         lpips_fn=lambda a, b: (a - b).abs().mean())
    assert rendered == [1, 2, 3, 4, 5]
    assert out["mean_psnr_static"] == out["mean_psnr"] and out["mean_ssim_static"] == out["mean_ssim"]
    assert set(out) == {"mean_psnr", "mean_ssim", "mean_lpips", "mean_psnr_static", "mean_ssim_static", "mean_lpips_static"}
    assert out["mean_lpips_static"] == out["mean_lpips"] > 0
    assert os.path.exists(tmp_path / "psnr" / "final" / "final_result.json") and not os.path.exists(tmp_path / "render_rgb")


def test_eval_rendering_matches_the_reference_file_list(golden_dir, tmp_path):
    """The files the reference wrote, less its matplotlib figures (viz/), are the files ``save_images`` writes."""
    from lvdgs.eval_utils import eval_rendering
    fx = load_fixture(golden_dir)
    by_idx = {f["idx"]: f for f in fx["frames"]}
    frames = {i: SimpleNamespace(uid=i, static_mask=None) for i in range(fx["num_frames"])}
    zero = torch.zeros(3, 48, 64)
    dataset = [(torch.from_numpy(by_idx[i]["gt"]) if i in by_idx else zero, None, None, None) for i in range(fx["num_frames"])]
    render_fn = lambda frame, *a: {"render": torch.from_numpy(by_idx[frame.uid]["render"]), "depth": torch.from_numpy(by_idx[frame.uid]["depth"])}
    row = {"psnr": 1.0, "ssim": 1.0, "psnr_static": 1.0, "ssim_static": 1.0, "static_ratio": None}
    eval_rendering(frames, None, dataset, str(tmp_path), None, torch.zeros(3), "monocular", fx["kf_indices"], "before_opt", render_fn=render_fn,
                   metrics_fn=lambda *a: row, save_images=True)
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs)
    assert files == [f for f in fx["files"] if not f.startswith("viz")]
    from PIL import Image
    for i, f in by_idx.items():      # the host statements of the unfused path write the reference's bytes
        assert np.array_equal(np.array(Image.open(tmp_path / "render_rgb" / f"{i}_pred.png")), f["png_rgb"])
        assert np.array_equal(np.array(Image.open(tmp_path / "render_depth" / f"{i}_pred.png")), f["png_depth"])
        assert np.array_equal(np.load(tmp_path / "render_depth_npy" / f"{i}_pred.npy"), f["npy_depth"])
        assert Image.open(tmp_path / "render_rgb" / f"{i}_pred.png").info["dpi"] == pytest.approx((300, 300), abs=0.01)


# ---------------------------------------------------------------- the C ABI
def test_scratch_bytes_are_aligned_and_monotone():
    L = _lib.lib()
    prev = 0
    for w, h in ((1, 1), (32, 32), (33, 32), (64, 64), (1226, 370), (1920, 1280), (4000, 3000)):
        b = L.lvdgs_frame_eval_scratch_bytes(w, h)
        tiles = -(-w // 32) * -(-h // 32)
        assert b % 256 == 0 and b >= prev and b >= 3 * tiles * 48, (w, h, b)
        assert b > prev or (w, h) == (32, 32)
        prev = b
    assert L.lvdgs_frame_eval_scratch_bytes(0, 5) == 0 and L.lvdgs_frame_eval_scratch_bytes(5, -1) == 0


def test_argument_validation_without_gpu():
    L = _lib.lib()
    assert L.lvdgs_frame_eval(None, None) == _lib.E_INVALID and b"image size" in L.lvdgs_last_error()
    a = _lib.FrameEvalArgs()
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"image size" in L.lvdgs_last_error()
    a.width, a.height = 64, -1
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"image size" in L.lvdgs_last_error()
    a.height = 48
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    # (never dereferenced: every call here is rejected before a launch)
    a.render, a.gt_image, a.out_row = 256, 512, 768
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()      # scratch
    a.scratch, a.scratch_bytes = 1024, L.lvdgs_frame_eval_scratch_bytes(64, 48) - 1
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"scratch too small" in L.lvdgs_last_error()
    a.scratch_bytes += 1
    a.depth8 = 2048
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"depth8 without depth" in L.lvdgs_last_error()
    a.depth8 = None
    a.out_row = 772
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"8-byte aligned" in L.lvdgs_last_error()
    a.out_row, a.scratch = 768, 1028
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_INVALID and b"8-byte aligned" in L.lvdgs_last_error()
    a.scratch = 1024
    a.width, a.height = 32 * 11000, 32 * 65535      # 11000 x 65535 x 3 workgroups: past 2^31 - 1
    a.scratch_bytes = L.lvdgs_frame_eval_scratch_bytes(a.width, a.height)
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_RANGE and b"workgroups" in L.lvdgs_last_error()
    a.width, a.height = 8, 32 * 65536
    a.scratch_bytes = L.lvdgs_frame_eval_scratch_bytes(a.width, a.height)
    assert L.lvdgs_frame_eval(C.byref(a), None) == _lib.E_RANGE and b"tile rows" in L.lvdgs_last_error()


def test_frame_evaluator_needs_a_gpu_device():
    from lvdgs.eval_utils import FrameEvaluator
    with pytest.raises(_lib.LvdgsError):
        FrameEvaluator(8, 8, "cpu", 1)
    with pytest.raises(ValueError):
        FrameEvaluator(0, 8, "cuda", 1)
