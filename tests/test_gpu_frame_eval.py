"""``lvdgs_frame_eval`` / ``eval_utils.FrameEvaluator`` on the GPU against the statement-level oracle (tests/frame_eval_oracle.py) and the
fixture of the reference's own ``eval_rendering``: exact counts and bytes, SSIM within 2e-6, sums of squares within a relative 2^-21.

The sums' bound: every term is non-negative and carries at most three float32 roundings (the difference, the square; the clamp is
exact), under 2^-22 relative per term, hence per sum; the float64 accumulation adds nothing at that scale and the margin doubles it."""
import random

import numpy as np
import pytest
import torch

import frame_eval_oracle as feo
from lvdgs import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(7, 5), (9, 37), (33, 65), (40, 52), (64, 64), (1, 1)]
SUM_REL, SSIM_TOL, PSNR_TOL = 2.0 ** -21, 2e-6, 1e-3


def _frame(H, W, seed, mask="partial", depth="ordinary", identical=False):
    """Render below 0 and above 1; ground truth with zeros in single channels (and a zero pixel when there is room)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g).clamp(min=1.0 / 256)
    gt[1] = torch.where(torch.rand(H, W, generator=g) < 0.2, torch.zeros(()), gt[1])      # zeros in one channel only
    if H > 2:
        gt[:, 0, :] = 0.0
    render = gt.clone() if identical else (gt + 0.15 * torch.randn(3, H, W, generator=g)) * 1.3 - 0.1
    m = {"none": None, "partial": torch.rand(H, W, generator=g) > 0.35, "zero": torch.zeros(H, W, dtype=torch.bool)}[mask]
    d = {"none": None, "ordinary": torch.rand(H, W, generator=g) * 40 + 0.5, "constant": torch.full((H, W), 3.25)}[depth]
    return render.contiguous(), gt.contiguous(), m, d


def _run(ev, render, gt, mask, bg, depth):
    i = ev.add(render.to(DEV), gt.to(DEV), None if mask is None else mask.to(DEV), None if bg is None else bg.to(DEV),
               None if depth is None else depth.to(DEV))
    images = {k: v.cpu().numpy() for k, v in ev.images(i).items()} if ev.want_images else {}
    return i, images


def _check(row, images, o, what):
    print(what, {k: (row[k].item(), o.get(k)) for k in ("sum_sq_full", "sum_sq_static", "n_basic", "n_keep", "ssim_full", "ssim_static")})
    assert int(row["n_basic"]) == o["n_basic"], what
    assert int(row["n_keep"]) == (o["n_keep"] if o["has_mask"] else o["n_basic"]), what
    want_static = o["sum_sq_static"] if o["has_mask"] else o["sum_sq_full"]
    assert abs(float(row["sum_sq_full"]) - o["sum_sq_full"]) <= SUM_REL * o["sum_sq_full"], what
    assert abs(float(row["sum_sq_static"]) - want_static) <= SUM_REL * want_static, what
    assert abs(float(row["ssim_full"]) - o["ssim_full"]) < SSIM_TOL, what
    assert abs(float(row["ssim_static"]) - o["ssim_static"]) < SSIM_TOL, what
    flags = int(row["flags"])
    assert bool(flags & _lib.FRAME_EVAL_HAS_MASK) == o["has_mask"] and int(row["reserved"]) == 0
    assert bool(flags & _lib.FRAME_EVAL_HAS_DEPTH) == ("depth_min" in o)
    if "depth_min" in o:
        assert float(row["depth_min"]) == o["depth_min"] and float(row["depth_max"]) == o["depth_max"], what
        assert bool(flags & _lib.FRAME_EVAL_DEPTH_CONSTANT) == o["depth_constant"], what
    for k, v in images.items():
        assert v.shape == o[k].shape and np.array_equal(v, o[k]), (what, k, int((v != o[k]).sum()))


@pytest.mark.parametrize("H,W", SIZES)
def test_rows_and_bytes_against_the_oracle(H, W):
    bg = torch.tensor([0.1, 0.6, 0.3])
    cases = [("none", "none", None), ("partial", "ordinary", bg), ("zero", "constant", bg), ("partial", "none", None), ("none", "ordinary", None)]
    from lvdgs.eval_utils import FrameEvaluator
    ev = FrameEvaluator(H, W, DEV, len(cases), want_images=True)
    kept = []
    for n, (mask, depth, b) in enumerate(cases):
        render, gt, m, d = _frame(H, W, 100 * H + W + n, mask, depth)
        assert H * W == 1 or (float(render.min()) < 0 and float(render.max()) > 1)
        i, images = _run(ev, render, gt, m, b, d)
        assert i == n and (("depth8" in images) == (d is not None))
        kept.append((images, feo.frame_eval(render.numpy(), gt.numpy(), None if m is None else m.numpy(), None if b is None else b.numpy(),
                                            None if d is None else d.numpy())))
    table = ev.read_table()
    for n, (images, o) in enumerate(kept):
        _check(table[n], images, o, (H, W, cases[n][:2]))
    zero = ev.results()[2]      # a mask that keeps nothing: the static values are the full ones, by the host's fallback
    assert zero["static_ratio"] is None and zero["psnr_static"] == zero["psnr"] and zero["ssim_static"] == zero["ssim"]
    assert np.all(kept[2][0]["depth8"] == 0) and int(table[2]["flags"]) & _lib.FRAME_EVAL_DEPTH_CONSTANT


@pytest.mark.parametrize("shape", ["hw", "1hw", "hw1", "uint8", "float"])
def test_mask_shapes_and_dtypes(shape):
    from lvdgs.eval_utils import FrameEvaluator
    H, W = 40, 52
    render, gt, m, _ = _frame(H, W, 7)
    given = {"hw": m, "1hw": m[None], "hw1": m[..., None], "uint8": m.to(torch.uint8) * 200, "float": m.float() * 0.5}[shape]
    ev = FrameEvaluator(H, W, DEV, 1)
    _run(ev, render, gt, given, None, None)
    _check(ev.read_table()[0], {}, feo.frame_eval(render.numpy(), gt.numpy(), m.numpy()), shape)


def test_identical_images():
    from lvdgs.eval_utils import FrameEvaluator
    H, W = 40, 52
    render, gt, m, _ = _frame(H, W, 11, identical=True)
    ev = FrameEvaluator(H, W, DEV, 1)
    _run(ev, render, gt, m, torch.tensor([0.2, 0.3, 0.4]), None)
    r = ev.results()[0]
    assert r["psnr"] == float("inf") and r["psnr_static"] == float("inf")
    assert abs(r["ssim"] - 1.0) < 1e-6 and abs(r["ssim_static"] - 1.0) < 1e-6      # test_gpu_ssim.py's bound for identical images
    row = ev.read_table()[0]
    assert float(row["sum_sq_full"]) == 0.0 and float(row["sum_sq_static"]) == 0.0


def test_quantisation_edges():
    """Render and ground truth run through k / 255 and its two float32 neighbours for every k: the bytes are NumPy's."""
    from lvdgs.eval_utils import FrameEvaluator
    H, W = 33, 65
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.stack([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))], 1).reshape(-1).astype(np.float32)
    n = 3 * H * W
    idx = np.arange(n)
    render = vals[idx % vals.size].reshape(3, H, W)
    gt = vals[(idx * 7 + 3) % vals.size].reshape(3, H, W)      # 7 and 768 are coprime: every value is met, against varying partners
    assert set(np.unique(render)) == set(vals) == set(np.unique(gt))
    depth = vals[(idx[:H * W] * 5 + 1) % vals.size].reshape(H, W) * 37.0 + 2.0
    ev = FrameEvaluator(H, W, DEV, 1, want_images=True)
    _, images = _run(ev, torch.from_numpy(render), torch.from_numpy(gt), None, None, torch.from_numpy(depth))
    o = feo.frame_eval(render, gt, None, None, depth)
    for name in ("pred8", "gt8", "residual8", "depth8"):
        assert np.array_equal(images[name], o[name]), (name, int((images[name] != o[name]).sum()))


def test_same_call_twice_gives_the_same_bits_and_rows_are_distinct_and_in_order():
    from lvdgs.eval_utils import FrameEvaluator
    H, W = 33, 65
    a, b = _frame(H, W, 21), _frame(H, W, 22, mask="none")
    ev = FrameEvaluator(H, W, DEV, 4)
    bg = torch.tensor([0.3, 0.2, 0.1])
    for f in (a, a, b, a):
        _run(ev, f[0], f[1], f[2], bg, f[3])
    raw = ev.rows.cpu().numpy()
    assert np.array_equal(raw[0], raw[1]) and np.array_equal(raw[0], raw[3]) and not np.array_equal(raw[0], raw[2])
    rows = ev.results()
    assert len(rows) == 4 and rows[0] == rows[1] == rows[3] and rows[2] != rows[0]
    oa = feo.metrics(feo.frame_eval(a[0].numpy(), a[1].numpy(), a[2].numpy(), bg.numpy()), a[1].numel())
    ob = feo.metrics(feo.frame_eval(b[0].numpy(), b[1].numpy()), b[1].numel())
    for got, want in ((rows[0], oa), (rows[2], ob)):
        assert abs(got["psnr"] - want["psnr"]) < PSNR_TOL and abs(got["ssim"] - want["ssim"]) < SSIM_TOL
    assert rows[2]["static_ratio"] is None and abs(rows[0]["static_ratio"] - oa["static_ratio"]) < 1e-12
    assert rows[0]["depth_min"] == float(a[3].min()) and rows[2]["depth_max"] == float(b[3].max())
    with pytest.raises(IndexError):
        ev.add(a[0].to(DEV), a[1].to(DEV))


def test_the_fixture_frames(golden_dir):
    """The frames of the reference's own run through ``FrameEvaluator``: its PNG bytes exactly, its means within 1e-3 dB / 2e-6.
    (These frames are half smooth, which is where the window's normalisation shows: with the eleven values summed one by one in float32 the
    SSIM means came out 2.67e-6 and 2.36e-6 low; with torch's sum they are 6e-8 and 4e-7 off.)"""
    from lvdgs.eval_utils import FrameEvaluator
    fx = feo.load_fixture(golden_dir)
    H, W = fx["frames"][0]["gt"].shape[1:]
    ev = FrameEvaluator(H, W, DEV, len(fx["frames"]), want_images=True)
    bg = torch.from_numpy(fx["background"])
    for f in fx["frames"]:
        m = None if f["used_mask"] is None else torch.from_numpy(f["used_mask"])
        _, images = _run(ev, torch.from_numpy(f["render"]), torch.from_numpy(f["gt"]), m, bg, torch.from_numpy(f["depth"]))
        assert np.array_equal(images["pred8"], f["png_rgb"]) and np.array_equal(images["depth8"], f["png_depth"]), f["idx"]
    feo.check_means(ev.results(), fx["result"])


def test_eval_rendering_fused_over_the_fixture(golden_dir, tmp_path):
    """``eval_utils.eval_rendering`` on its default path (one ``FrameEvaluator`` over the loop, the files written from the device bytes, one
    read at the end) over the frames of the reference's own run, the masks left on the HOST as a dataset may hand them over: the
    reference's file list, its PNG bytes and ``.npy`` depths exactly, its means within 1e-3 dB / 2e-6."""
    import json
    import os
    from types import SimpleNamespace
    from PIL import Image
    from lvdgs.eval_utils import eval_rendering
    fx = feo.load_fixture(golden_dir)
    by_idx = {f["idx"]: f for f in fx["frames"]}
    frames = {}
    for i in range(fx["num_frames"]):
        f = by_idx.get(i)
        cpu = lambda m: None if m is None else torch.from_numpy(m)
        frames[i] = SimpleNamespace(uid=i, static_mask=cpu(f["static_mask"]) if f else None, expanded_static_mask=cpu(f["expanded_static_mask"]) if f else None)
    frames[6].static_mask = frames[6].static_mask.to(DEV)      # one mask on the device, the others on the host
    assert sum(1 for fr in frames.values() if fr.static_mask is not None and not fr.static_mask.is_cuda) >= 2
    zero = torch.zeros(3, 48, 64)
    dataset = [(torch.from_numpy(by_idx[i]["gt"]) if i in by_idx else zero, None, None, None) for i in range(fx["num_frames"])]      # host images too
    rendered = []

    def render_fn(frame, gaussians, pipe, background):
        rendered.append(frame.uid)
        return {"render": torch.from_numpy(by_idx[frame.uid]["render"]).to(DEV), "depth": torch.from_numpy(by_idx[frame.uid]["depth"]).to(DEV)}
    out = eval_rendering(frames, None, dataset, str(tmp_path), None, torch.from_numpy(fx["background"]), "monocular", fx["kf_indices"], "before_opt",
                         render_fn=render_fn, save_images=True)      # fused=True is the default; the background on the host as well
    assert rendered == sorted(by_idx)
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs)
    assert files == [f for f in fx["files"] if not f.startswith("viz")]
    for i, f in by_idx.items():
        assert np.array_equal(np.array(Image.open(tmp_path / "render_rgb" / f"{i}_pred.png")), f["png_rgb"]), i
        assert np.array_equal(np.array(Image.open(tmp_path / "render_depth" / f"{i}_pred.png")), f["png_depth"]), i
        assert np.array_equal(np.load(tmp_path / "render_depth_npy" / f"{i}_pred.npy"), f["npy_depth"]), i
    print(out, fx["result"])
    assert set(out) == {"mean_psnr", "mean_ssim", "mean_psnr_static", "mean_ssim_static"}
    for k in out:
        assert abs(out[k] - fx["result"][k]) < (PSNR_TOL if "psnr" in k else SSIM_TOL), k
    with open(tmp_path / "psnr" / "before_opt" / "final_result.json") as fh:
        assert json.load(fh) == out
    # with an lpips_fn the LPIPS keys appear, and the path still makes one read of the table
    out2 = eval_rendering(frames, None, dataset, str(tmp_path / "b"), None, torch.from_numpy(fx["background"]), "monocular", fx["kf_indices"],
                          render_fn=render_fn, lpips_fn=lambda a, b: (a - b).abs().mean())
    assert set(out2) == set(out) | {"mean_lpips", "mean_lpips_static"} and all(out2[k] == out[k] for k in out)
    assert not os.path.exists(tmp_path / "b" / "render_rgb") and os.path.exists(tmp_path / "b" / "psnr" / "final" / "final_result.json")


def test_frame_metrics_fused_agrees_with_the_host_path():
    from lvdgs.eval_utils import frame_metrics
    H, W = 70, 110
    render, gt, m, _ = _frame(H, W, 31)
    bg = torch.tensor([0.0, 0.25, 0.5])
    for mask, b in ((m, bg), (None, None), (torch.zeros(H, W, dtype=torch.bool), bg), (m[None], None)):
        args = (render.to(DEV), gt.to(DEV), None if mask is None else mask.to(DEV), None if b is None else b.to(DEV))
        host, fused = frame_metrics(*args), frame_metrics(*args, fused=True)
        print(host, fused)
        assert set(host) == set(fused)
        for k in ("psnr", "psnr_static"):
            assert abs(host[k] - fused[k]) < PSNR_TOL, k
        for k in ("ssim", "ssim_static"):
            assert abs(host[k] - fused[k]) < SSIM_TOL, k
        assert (host["static_ratio"] is None) == (fused["static_ratio"] is None)
        if host["static_ratio"] is not None:
            assert abs(host["static_ratio"] - fused["static_ratio"]) < 1e-6      # (the host path's mean is float32)


def _count_waits_and_reads(fn):
    """(calls of any HostCall.wait, of torch.cuda.synchronize / Stream.synchronize / Event.synchronize, of Tensor.cpu / .item / .tolist) while ``fn`` runs."""
    counts = {"wait": 0, "sync": 0, "read": 0}
    saved = [(_lib.HostCall, "wait", _lib.HostCall.wait), (torch.cuda, "synchronize", torch.cuda.synchronize),
             (torch.cuda.Stream, "synchronize", torch.cuda.Stream.synchronize), (torch.cuda.Event, "synchronize", torch.cuda.Event.synchronize),
             (torch.Tensor, "cpu", torch.Tensor.cpu), (torch.Tensor, "item", torch.Tensor.item), (torch.Tensor, "tolist", torch.Tensor.tolist)]

    def counting(kind, real):
        def f(*a, **k):
            counts[kind] += 1
            return real(*a, **k)
        return f
    for owner, name, real in saved:
        setattr(owner, name, counting("wait" if owner is _lib.HostCall else "sync" if name == "synchronize" else "read", real))
    try:
        fn()
    finally:
        for owner, name, real in saved:
            setattr(owner, name, real)
    return counts


def test_add_makes_no_wait_and_results_reads_once():
    from lvdgs.eval_utils import FrameEvaluator
    H, W, N = 40, 52, 5
    frames = [tuple(None if t is None else t.to(DEV) for t in _frame(H, W, 40 + i)) for i in range(N)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    ev = FrameEvaluator(H, W, DEV, N, want_images=True)
    ev.add(frames[0][0], frames[0][1], frames[0][2], bg, frames[0][3])      # (the first call allocates the scratch)
    ev.reset()
    c = _count_waits_and_reads(lambda: [ev.add(r, g, m, bg, d) for r, g, m, d in frames])
    assert c == {"wait": 0, "sync": 0, "read": 0}, c
    out = []
    c = _count_waits_and_reads(lambda: out.extend(ev.results()))
    assert c == {"wait": 0, "sync": 0, "read": 1}, c
    assert len(out) == N and len({r["psnr"] for r in out}) == N


def test_wrong_device_dtype_and_shape_are_refused_on_the_host():
    from lvdgs.eval_utils import FrameEvaluator
    H, W = 9, 37
    render, gt, m, d = (None if t is None else t.to(DEV) for t in _frame(H, W, 50))
    ev = FrameEvaluator(H, W, DEV, 2)
    with pytest.raises(ValueError):
        ev.add(render.cpu(), gt)
    with pytest.raises(TypeError):
        ev.add(render.double(), gt)
    with pytest.raises(TypeError):
        ev.add(render, gt, depth=d.half())
    with pytest.raises(ValueError):
        ev.add(render, gt, m.cpu())
    with pytest.raises(ValueError):
        ev.add(render, gt[:, :-1])
    with pytest.raises(ValueError):
        ev.add(render, gt, m[None].expand(3, -1, -1))
    with pytest.raises(ValueError):
        ev.images(0)
    assert ev.count == 0 and ev.add(render, gt, m) == 0


def test_toy_sequence_eval_rendering_fused_equals_the_default():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import sequence_scene as ss
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
    torch.manual_seed(0)
    random.seed(0)
    seq = SlamSequence(cfg, ds.to("cuda"), ss.empty_map(cfg, "cuda"), ss.PIPE, torch.zeros(3, device="cuda"), idle_map_iters=2).run()
    host, fused = seq.eval_rendering(), seq.eval_rendering(fused=True)
    print(host, fused)
    assert set(host) == set(fused) and "psnr" in host and "ssim" in host
    for k in host:
        assert abs(host[k] - fused[k]) < (PSNR_TOL if k.startswith("psnr") else SSIM_TOL if k.startswith("ssim") else 1e-6), k
