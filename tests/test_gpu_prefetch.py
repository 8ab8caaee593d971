"""``lvdgs_ingest_depth`` against its host statement, ``planes="device"``, ``FramePrefetcher``'s side stream under a busy consumer, and
the loops and the evaluation with frames read ahead against the plain runs -- on the GPU."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from lvdgs import _lib, dataset as D
from test_dataset import rebuild_tree, same_bits
from test_prefetch import DIVISORS, prefetch_threads

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
SHAPES = ((1, 1), (67, 35), (131, 3), (64, 64))        # (W, H): one pixel; odd, H*W = 2345 not a multiple of 4; three rows; whole groups only


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dataset.npz"))


def samples_of(dtype, W, H, seed):
    top = np.iinfo(dtype).max
    s = np.random.default_rng(seed).integers(0, top + 1, (H, W)).astype(dtype)
    s.reshape(-1)[:4] = np.array([0, 1, 255, top], dtype)[:s.size]       # the extreme samples lead
    s.reshape(-1)[-1] = top if s.size > 1 else s.reshape(-1)[-1]
    return s


def call_depth(dev, host_bytes, dtype, W, H, stride, pitch, divisor, src_offset=0, out_offset=0):
    """``lvdgs_ingest_depth`` on ``host_bytes`` (a flat uint8 array) uploaded ``src_offset`` bytes into a buffer, the output ``out_offset``
    floats into one that is filled with a sentinel -> (the H x W plane, the floats around it)."""
    buf = torch.zeros(src_offset + host_bytes.size + 16, dtype=torch.uint8, device=dev)
    buf[src_offset:src_offset + host_bytes.size] = torch.from_numpy(host_bytes).to(dev)
    out = torch.full((out_offset + W * H + 8,), -7.0, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    a = _lib.IngestDepthArgs(width=W, height=H, src=buf.data_ptr() + src_offset, sample_type=_lib.DEPTH_SAMPLE_BYTE if dtype == np.uint8 else _lib.DEPTH_SAMPLE_WORD,
                             pixel_stride=stride, src_row_bytes=pitch, divisor=divisor, out=out.data_ptr() + 4 * out_offset)
    _lib.check(_lib.lib().lvdgs_ingest_depth(C.byref(a), _lib.raw_stream(dev)), "lvdgs_ingest_depth")
    got = out.cpu().numpy()
    return got[out_offset:out_offset + W * H].reshape(H, W), np.concatenate([got[:out_offset], got[out_offset + W * H:]])


# ---- the kernel against convert_depth_host ----
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("W,H", SHAPES)
def test_ingest_depth_equals_the_host_statement(dev, W, H, dtype):
    size = np.dtype(dtype).itemsize
    for k, divisor in enumerate(DIVISORS):
        s = samples_of(dtype, W, H, 3 * k + W)
        want = D.convert_depth_host(s, divisor)
        flat = np.ascontiguousarray(s).view(np.uint8).reshape(-1)
        got, around = call_depth(dev, flat, dtype, W, H, size, W * size, divisor)              # rows without a gap, 16-byte aligned: the vector paths
        assert same_bits(got, want) and (around == -7.0).all(), (W, H, dtype, divisor)
        again, _ = call_depth(dev, flat, dtype, W, H, size, W * size, divisor)
        assert got.tobytes() == again.tobytes()                                                 # two calls, equal bytes
        got, around = call_depth(dev, flat, dtype, W, H, size, W * size, divisor, out_offset=1)  # the output 4 bytes off a 16-byte boundary
        assert same_bits(got, want) and (around == -7.0).all(), (W, H, dtype, divisor, "out + 4")
        got, around = call_depth(dev, flat, dtype, W, H, size, W * size, divisor, src_offset=2)  # the source off its vector alignment
        assert same_bits(got, want) and (around == -7.0).all(), (W, H, dtype, divisor, "src + 2")
        pad = 6                                                                                 # a row pitch: 6 bytes between the rows
        rows = np.full((H, W * size + pad), 0xAB, np.uint8)
        rows[:, :W * size] = np.ascontiguousarray(s).view(np.uint8).reshape(H, W * size)
        got, around = call_depth(dev, rows.reshape(-1), dtype, W, H, size, W * size + pad, divisor)
        assert same_bits(got, want) and (around == -7.0).all(), (W, H, dtype, divisor, "pitch")


@pytest.mark.parametrize("W,H", SHAPES)
def test_ingest_depth_reads_the_first_channel_of_colour_bytes(dev, W, H):
    """Stride 3 into H x W x 3 colour bytes: the dword path (rows without a gap, aligned), the byte path (an odd base, a row pitch), and
    the package's ``ingest_depth`` on the view ``frame[:, :, 0]``."""
    rgb = np.random.default_rng(W).integers(0, 256, (H, W, 3)).astype(np.uint8)
    rgb.reshape(-1, 3)[:4, 0] = np.array([0, 1, 255, 255], np.uint8)[:W * H]
    rgb[..., 1:] |= 0x80                                  # no other channel can pass for the first
    for divisor in DIVISORS:
        want = D.convert_depth_host(rgb[:, :, 0], divisor)
        for off in (0, 1):
            got, around = call_depth(dev, rgb.reshape(-1), np.uint8, W, H, 3, 3 * W, divisor, src_offset=off, out_offset=off)
            assert same_bits(got, want) and (around == -7.0).all(), (W, H, divisor, off)
        rows = np.zeros((H, 3 * W + 5), np.uint8)
        rows[:, :3 * W] = rgb.reshape(H, 3 * W)
        got, _ = call_depth(dev, rows.reshape(-1), np.uint8, W, H, 3, 3 * W + 5, divisor)
        assert same_bits(got, want), (W, H, divisor, "pitch")
        on_device = torch.from_numpy(rgb).to(dev)
        assert same_bits(D.ingest_depth(on_device[:, :, 0], divisor).cpu().numpy(), want)
    words = np.random.default_rng(1).integers(0, 65536, (H, W)).astype(np.uint16)
    as_int16 = torch.from_numpy(words.view(np.int16)).to(dev)                                    # the bits of a 16-bit file, read as unsigned
    assert same_bits(D.ingest_depth(as_int16, 6553.5).cpu().numpy(), D.convert_depth_host(words, 6553.5))
    with pytest.raises(ValueError):
        D.ingest_depth(on_device, 5000.0)                  # three dimensions
    with pytest.raises(_lib.LvdgsError):
        D.ingest_depth(on_device[:, :, 0], 0.0)            # the library's refusal, raised


# ---- planes="device" ----
@pytest.mark.parametrize("name", ["waymo", "kitti"])
def test_device_planes_equal_the_host_arrays_cast(golden, tmp_path, name, dev):
    from lvdgs.camera_utils import Camera
    from lvdgs.graphics_utils import getProjectionMatrix2
    from lvdgs.slam_utils import _mono_depth
    cfg = rebuild_tree(golden, name, tmp_path / name)
    plain = D.load_dataset(None, None, cfg, device=dev, ingest="fused")
    ds = D.load_dataset(None, None, cfg, device=dev, ingest="fused", planes="device")
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=ds.fx, fy=ds.fy, cx=ds.cx, cy=ds.cy, W=ds.width, H=ds.height).transpose(0, 1).to(dev)
    for i in range(len(ds)):
        rec = ds.frame(i)
        image, depth, pose, mono = rec.frame
        pi, pd, pp, pm = plain[i]
        assert torch.equal(image, pi) and torch.equal(pose, pp) and same_bits(depth, pd) and same_bits(mono, pm)     # the 4-tuple is unchanged
        assert same_bits(ds[i][1], pd) and plain.frame(i).depth32 is None
        for plane, host in ((rec.depth32, depth), (rec.mono_depth32, mono)):
            assert plane.dtype is torch.float32 and plane.device == dev and tuple(plane.shape) == (ds.height, ds.width)
            assert same_bits(plane.cpu().numpy(), host.astype(np.float32)), (name, i)
        cam = Camera.init_from_dataset(ds, i, proj)
        seeded = cam._lvdgs_mono_depth[1]
        assert _mono_depth(cam, cam.original_image) is seeded and cam._lvdgs_mono_depth[0] is cam.mono_depth      # no upload: the seeded tensor
        assert tuple(seeded.shape) == (1, ds.height, ds.width) and same_bits(seeded[0].cpu().numpy(), mono.astype(np.float32))
        assert same_bits(cam.depth32.cpu().numpy(), depth.astype(np.float32))
        uploaded = _mono_depth(Camera.init_from_dataset(plain, i, proj), cam.original_image)
        assert torch.equal(uploaded, seeded)                                                                      # what the upload gives
        cam.mono_depth = (np.asarray(cam.mono_depth, dtype=np.float32) * np.float32(1.25)).astype(np.float32)     # a rescaled array: not the cached one
        fresh = _mono_depth(cam, cam.original_image)
        assert fresh is not seeded and same_bits(fresh[0].cpu().numpy(), cam.mono_depth)
        cam.clean()
        assert cam.depth32 is None


# ---- the side stream under a busy consumer ----
def busy_tree(root, golden, n=12, W=640, H=480):
    """``n`` frames of noise in the waymo layout, 16-bit depth files, a small distortion -> the settings."""
    from PIL import Image
    cfg = json.loads(str(golden["waymo/config"]))
    cfg["Dataset"]["dataset_path"] = str(root)
    cfg["Dataset"]["Calibration"].update(width=W, height=H, fx=500.0, fy=500.0, cx=W / 2.0, cy=H / 2.0, distorted=True,
                                         k1=0.02, k2=-0.01, p1=0.0005, p2=-0.0003, k3=0.0)
    rng = np.random.default_rng(5)
    for sub in ("rgb", "depth", "mono_depth", "gt"):
        os.makedirs(os.path.join(root, sub))
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(root, "rgb", f"{i:04d}.png"), compress_level=1)
        for sub in ("depth", "mono_depth"):
            Image.fromarray(rng.integers(0, 65536, (H, W)).astype(np.uint16)).save(os.path.join(root, sub, f"{i:04d}.png"), compress_level=1)
        pose = np.eye(4)
        pose[:3, 3] = (0.1 * i, 0.0, 0.02 * i)
        np.savetxt(os.path.join(root, "gt", f"{i:04d}.txt"), pose.reshape(1, 16), delimiter=" ")
    return cfg


@pytest.mark.parametrize("planes", ["host", "device"])
def test_the_side_stream_hands_over_whole_frames_to_a_busy_consumer(golden, tmp_path, dev, planes):
    """12 frames through the prefetcher with two frames read ahead (so the ring's slots come round), a long elementwise job on the
    consumer's stream between the takes: a missing event or a slot reused early would hand out other bits than ``dataset[i]``."""
    cfg = busy_tree(str(tmp_path / "busy"), golden)
    ds = D.load_dataset(None, None, cfg, device=dev, ingest="fused", planes=planes)
    assert len(ds) == 12 and ds.disorted is True
    load = torch.ones(1 << 26, dtype=torch.float32, device=dev)
    taken = []
    with D.FramePrefetcher(ds, range(12), depth=2, workers=2) as pf:
        assert pf._side is not None
        for i in range(12):
            rec = pf.frame(i)
            taken.append((rec.frame, rec.depth32, rec.mono_depth32))
            check = rec.frame[0].sum()                     # the consumer reads the frame on its own stream at once ...
            for _ in range(24):
                load.mul_(1.0000001)                       # ... and keeps that stream busy while the next frames are staged
            taken[-1] += (check,)
        assert len(pf._ring) <= pf._ring_slots
    assert not prefetch_threads()
    torch.cuda.synchronize(dev)
    for i, ((image, depth, pose, mono), d32, m32, check) in enumerate(taken):
        wi, wd, wp, wm = ds[i]
        assert torch.equal(image, wi) and torch.equal(pose, wp) and pose.dtype is torch.float64, i
        assert same_bits(depth, wd) and same_bits(mono, wm), i
        assert torch.equal(check, wi.sum()), i
        if planes == "device":
            assert same_bits(d32.cpu().numpy(), wd.astype(np.float32)) and same_bits(m32.cpu().numpy(), wm.astype(np.float32)), i
        else:
            assert d32 is None and m32 is None


# ---- the loops and the evaluation with frames read ahead ----
@pytest.fixture(scope="module")
def drive_runs(tmp_path_factory, dev):
    """The six-frame exported drive of tests/test_gpu_dataset.py, run plainly (fused ingest) and with ``prefetch=3`` over ``planes="device"``."""
    import export_sequence_dir as ex
    import sequence as tool
    from lvdgs.slam_sequence import SlamSequence
    root = tmp_path_factory.mktemp("drive")
    cfg, ds, _ = tool.kitti_sequence(dev, frames=6, scale=0.25, cadence="short", masks=False)
    path = ex.export_dataset(ds, cfg, str(root / "drive"), dist=(0.02, -0.01, 0.0005, -0.0003, 0.0))
    runs = {}
    for name, planes, prefetch in (("plain", "host", 0), ("ahead", "device", 3)):
        torch.manual_seed(0)
        random.seed(0)
        c, d = tool.directory_sequence(dev, path, ingest="fused", planes=planes)
        seq = SlamSequence(c, d, tool.empty_map(c, dev), tool.PIPE, torch.zeros(3, device=dev), idle_map_iters=2, prefetch=prefetch)
        seq.run()
        assert seq._frames is None and not prefetch_threads()
        runs[name] = seq
    return runs


def test_the_loops_with_frames_read_ahead_equal_the_plain_run(drive_runs):
    p, a = drive_runs["plain"], drive_runs["ahead"]
    assert a.prefetch == 3 and a.dataset.planes == "device" and p.prefetch == 0
    assert p.kf_indices == a.kf_indices and sorted(p.cameras) == sorted(a.cameras) == list(range(6))
    for i in p.cameras:
        assert torch.equal(p.cameras[i].R, a.cameras[i].R) and torch.equal(p.cameras[i].T, a.cameras[i].T), i
    pp, pa = p.gaussians._params_by_name(), a.gaussians._params_by_name()
    assert pp.keys() == pa.keys() and p.gaussians.get_xyz.shape[0] == a.gaussians.get_xyz.shape[0] > 0
    for k in pp:
        assert torch.equal(pp[k], pa[k]), k
    kf = a.cameras[a.kf_indices[-1]]
    assert kf.depth32 is not None and kf._lvdgs_mono_depth[1].is_cuda          # the keyframes carried the device planes


def test_eval_rendering_with_frames_read_ahead_gives_the_same_dict_and_files(drive_runs, tmp_path, dev):
    import sequence as tool
    from lvdgs.eval_utils import eval_rendering
    seq = drive_runs["plain"]
    outs, files = {}, {}
    for name, prefetch in (("plain", 0), ("ahead", 3)):
        root = tmp_path / name
        outs[name] = eval_rendering(seq.cameras, seq.frontend_gaussians, seq.dataset, str(root), tool.PIPE, torch.zeros(3, device=dev), "monocular",
                                    seq.kf_indices, save_images=True, prefetch=prefetch)
        files[name] = {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}
        assert not prefetch_threads()
    assert outs["plain"] == outs["ahead"] and set(outs["plain"]) == {"mean_psnr", "mean_ssim", "mean_psnr_static", "mean_ssim_static"}
    assert files["plain"].keys() == files["ahead"].keys() and any(f.startswith("render_rgb") for f in files["plain"])
    for f in files["plain"]:
        assert files["plain"][f] == files["ahead"][f], f
