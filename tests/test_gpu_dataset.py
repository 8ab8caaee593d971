"""The HIP frame ingest (``lvdgs_undistort_map``, ``lvdgs_ingest_frame``: csrc/ingest.hip) against the independent oracle
(tests/ingest_oracle.py) on the cases of tests/ingest_cases.py -- ``sx``, ``sy``, ``image_u8`` and ``image`` bit for bit --, the dataset
classes with ``ingest="fused"`` against ``ingest="host"``, and the loops on an exported directory in both modes.  Reads nothing of the
reference."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import ingest_cases as ic
from lvdgs import _lib, dataset as D
from test_dataset import TREES, ingest_refusals, rebuild_tree, same_bits, valid_ingest_args

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dataset.npz"))


def device_source(name, kind, dev):
    """The case's source on the device as the (H, W, 3) view ``ingest_frame`` takes: its rows ``3 W + pad`` bytes apart."""
    c = ic.case(name)
    rows = torch.from_numpy(ic.source(name, kind).copy()).to(dev)
    return rows.as_strided((c["H"], c["W"], 3), (rows.stride(0), 3, 1))


def device_map(name, dev):
    c = ic.case(name)
    return D.undistort_map_device(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"], dev)


@pytest.mark.parametrize("name", sorted(ic.SMALL))
def test_undistort_map_equals_the_oracle(name, dev):
    sx, sy = device_map(name, dev)
    want_sx, want_sy = ic.reference_map(name)
    assert same_bits(sx.cpu().numpy(), want_sx), name
    assert same_bits(sy.cpu().numpy(), want_sy), name


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("name", sorted(ic.SMALL))
def test_ingest_with_a_remap_equals_the_oracle(name, kind, dev):
    src = device_source(name, kind, dev)
    sx, sy = device_map(name, dev)
    image, u8 = D.ingest_frame(src, sx, sy, want_u8=True)
    want_u8, want = ic.reference(name, kind, True)
    assert same_bits(u8.cpu().numpy(), want_u8), name
    assert same_bits(image.cpu().numpy(), want), name
    alone = D.ingest_frame(src, sx, sy)                        # image_u8 = NULL
    again, u8_again = D.ingest_frame(src, sx, sy, want_u8=True)
    assert torch.equal(alone, image) and torch.equal(again, image) and torch.equal(u8_again, u8)


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("name", sorted(ic.SMALL))
def test_ingest_without_a_remap_equals_the_oracle(name, kind, dev):
    src = device_source(name, kind, dev)
    image, u8 = D.ingest_frame(src, want_u8=True)
    want_u8, want = ic.reference(name, kind, False)
    assert same_bits(u8.cpu().numpy(), want_u8), name
    assert same_bits(image.cpu().numpy(), want), name
    assert torch.equal(D.ingest_frame(src), image)


def test_unaligned_buffers_take_the_scalar_paths(dev):
    """A source, a byte copy and an image that start on odd addresses: no wide access may be assumed."""
    name, kind = "64x64", "noise"
    c = ic.case(name)
    W, H = c["W"], c["H"]
    L = _lib.lib()
    flat = torch.from_numpy(ic.source(name, kind).copy().reshape(-1))
    src = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device=dev)
    src[1:1 + flat.numel()] = flat.to(dev)
    sx, sy = device_map(name, dev)
    msx, msy = torch.zeros(W * H + 4, dtype=torch.int32, device=dev), torch.zeros(W * H + 4, dtype=torch.int32, device=dev)
    msx[1:1 + W * H], msy[1:1 + W * H] = sx.reshape(-1), sy.reshape(-1)                     # 4 bytes off a 16-byte boundary
    image = torch.full((3 * H * W + 4,), -1.0, dtype=torch.float32, device=dev)
    u8 = torch.full((3 * H * W + 16,), 7, dtype=torch.uint8, device=dev)
    for remap in (False, True):
        a = _lib.IngestArgs(width=W, height=H, src=src.data_ptr() + 1, src_row_bytes=3 * W, map_sx=msx.data_ptr() + 4 if remap else None,
                            map_sy=msy.data_ptr() + 4 if remap else None, image=image.data_ptr() + 4, image_u8=u8.data_ptr() + 3)
        _lib.check(L.lvdgs_ingest_frame(C.byref(a), _lib.raw_stream(dev)), "lvdgs_ingest_frame")
        want_u8, want = ic.reference(name, kind, remap)
        assert same_bits(image[1:1 + 3 * H * W].cpu().numpy().reshape(3, H, W), want)
        assert same_bits(u8[3:3 + 3 * H * W].cpu().numpy().reshape(H, W, 3), want_u8)
        assert float(image[0]) == -1.0 and float(image[-1]) == -1.0 and int(u8[2]) == 7 and int(u8[3 + 3 * H * W]) == 7   # nothing beside the outputs


def test_a_full_waymo_frame_equals_the_oracle(dev):
    """1920 x 1280 with the coefficients of the committed 405841.yaml."""
    name = ic.FULL
    sx, sy = device_map(name, dev)
    assert same_bits(sx.cpu().numpy(), ic.reference_map(name)[0]) and same_bits(sy.cpu().numpy(), ic.reference_map(name)[1])
    src = device_source(name, "noise", dev)
    image, u8 = D.ingest_frame(src, sx, sy, want_u8=True)
    want_u8, want = ic.reference(name, "noise", True)
    assert same_bits(u8.cpu().numpy(), want_u8) and same_bits(image.cpu().numpy(), want)
    plain = D.ingest_frame(src)
    assert same_bits(plain.cpu().numpy(), ic.reference(name, "noise", False)[1])
    assert torch.equal(D.ingest_frame(src, sx, sy), image)


def test_refusals_on_the_device_leave_the_outputs_alone(dev):
    L = _lib.lib()
    stream = _lib.raw_stream(dev)
    src = torch.zeros((8, 16, 3), dtype=torch.uint8, device=dev)
    image = torch.full((3, 8, 16), -1.0, device=dev)
    m = torch.zeros((8, 16), dtype=torch.int32, device=dev)
    for what, over, word in ingest_refusals():
        over = {k: (m.data_ptr() if k in ("map_sx", "map_sy") else v) for k, v in over.items()}
        a = valid_ingest_args(**{**dict(src=src.data_ptr(), image=image.data_ptr()), **over})
        assert L.lvdgs_ingest_frame(C.byref(a), stream) == _lib.E_INVALID, what
    torch.cuda.synchronize()
    assert bool((image == -1.0).all())
    with pytest.raises(_lib.LvdgsError):
        D.ingest_frame(src.cpu())
    with pytest.raises(ValueError):
        D.ingest_frame(src, m)
    with pytest.raises(ValueError):
        D.ingest_frame(src, m[:4], m[:4])


# ---- the dataset classes: fused against host ----
def frames_equal(a, b):
    for k in range(len(a)):
        ia, da, pa, ma = a[k]
        ib, db, pb, mb = b[k]
        assert ia.is_cuda and ib.is_cuda and ia.dtype is torch.float32 and pa.is_cuda and pa.dtype is torch.float64
        assert torch.equal(ia, ib) and torch.equal(pa, pb), k
        assert same_bits(da, db) and same_bits(ma, mb), k


@pytest.mark.parametrize("name", TREES)
def test_fused_ingest_equals_host_ingest_on_the_golden_trees(golden, tmp_path, name, dev):
    cfg = rebuild_tree(golden, name, tmp_path / name)
    host = D.load_dataset(None, None, cfg, device=dev, ingest="host")
    fused = D.load_dataset(None, None, cfg, device=dev, ingest="fused")
    frames_equal(host, fused)
    assert same_bits(fused[0][0].cpu().numpy(), golden[f"{name}/image/0"])       # and both are the reference's bits


def test_fused_ingest_equals_host_ingest_on_a_distorted_tree(golden, tmp_path, dev):
    cfg = rebuild_tree(golden, "replica", tmp_path / "r")
    cfg["Dataset"]["Calibration"].update(distorted=True, k1=0.2, k2=-0.05, p1=0.01, p2=-0.004, k3=0.02)
    host = D.load_dataset(None, None, cfg, device=dev, ingest="host")
    fused = D.load_dataset(None, None, cfg, device=dev, ingest="fused")
    frames_equal(host, fused)
    plain = D.load_dataset(None, None, rebuild_tree(golden, "replica", tmp_path / "p"), device=dev, ingest="fused")
    assert not torch.equal(plain[0][0], fused[0][0])                              # the remap did something
    raw = host.decode_color(host.color_paths[1])
    (ih, uh), (i_f, uf) = host.ingest_image(raw, want_u8=True), fused.ingest_image(raw, want_u8=True)
    assert torch.equal(ih, i_f) and torch.equal(uh, uf)


# ---- the loops on an exported directory ----
def test_the_loops_on_an_exported_directory_agree_between_the_two_modes(tmp_path, dev):
    """Six frames of the synthetic drive at a quarter of KITTI's size, written as a waymo-layout directory with a small distortion, read back
    through load_config + load_dataset, run through SlamSequence with host and with fused ingest: the images are the same bits, so every
    pose and the whole map are."""
    import export_sequence_dir as ex
    import sequence as tool
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _ = tool.kitti_sequence(dev, frames=6, scale=0.25, cadence="short", masks=False)
    path = ex.export_dataset(ds, cfg, str(tmp_path / "drive"), dist=(0.02, -0.01, 0.0005, -0.0003, 0.0))
    for sub in ("rgb", "depth", "mono_depth", "gt"):
        assert len(os.listdir(tmp_path / "drive" / sub)) == 6
    runs = {}
    for mode in ("host", "fused"):
        torch.manual_seed(0)
        random.seed(0)
        c, d = tool.directory_sequence(dev, path, ingest=mode)
        assert d.disorted is True and len(d) == 6 and (d.width, d.height) == (ds.width, ds.height)
        seq = SlamSequence(c, d, tool.empty_map(c, dev), tool.PIPE, torch.zeros(3, device=dev), idle_map_iters=2)
        seq.run()
        runs[mode] = seq
    h, f = runs["host"], runs["fused"]
    assert h.kf_indices == f.kf_indices and sorted(h.cameras) == sorted(f.cameras) == list(range(6))
    for i in h.cameras:
        assert torch.equal(h.cameras[i].R, f.cameras[i].R) and torch.equal(h.cameras[i].T, f.cameras[i].T), i
    ph, pf = h.gaussians._params_by_name(), f.gaussians._params_by_name()
    assert ph.keys() == pf.keys() and h.gaussians.get_xyz.shape[0] == f.gaussians.get_xyz.shape[0] > 0
    for k in ph:
        assert torch.equal(ph[k], pf[k]), k
    print(json.dumps(dict(frames=6, keyframes=h.kf_indices, gaussians=int(h.gaussians.get_xyz.shape[0]))))
