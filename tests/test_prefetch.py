"""``lvdgs.dataset``'s split of a frame into its host half (``read``) and its device half (``assemble``), ``FramePrefetcher`` over the
golden 48 x 32 trees, the host statement of the depth conversion and the refusals of ``lvdgs_ingest_depth`` -- all without a GPU."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest
import torch

from lvdgs import _lib, dataset as D
from test_dataset import GOLDEN, rebuild_tree, same_bits

DIVISORS = (256.0, 5000.0, 6553.5, 5 * 6553.5)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dataset.npz"))


def host_set(golden, root, name):
    return D.load_dataset(None, None, rebuild_tree(golden, name, root / name), device="cpu", ingest="host")


def same_frame(a, b):
    (ia, da, pa, ma), (ib, db, pb, mb) = a, b
    return (same_bits(ia.numpy(), ib.numpy()) and same_bits(da, db) and same_bits(pa.numpy(), pb.numpy()) and same_bits(ma, mb)
            and pa.dtype is torch.float64 and ia.dtype is torch.float32)


def prefetch_threads():
    return [t for t in threading.enumerate() if t.name.startswith("lvdgs-prefetch")]


# ---- the split, and the prefetcher against dataset[i] ----
@pytest.mark.parametrize("name", ["waymo", "kitti", "replica"])
def test_assemble_of_read_is_getitem(golden, tmp_path, name):
    ds = host_set(golden, tmp_path, name)
    for i in range(len(ds)):
        rec = ds.read(i)
        assert isinstance(rec.raw, np.ndarray) and isinstance(rec.pose, np.ndarray) and rec.frame is None and rec.depth32 is None
        assert same_frame(ds.assemble(rec), ds[i]), (name, i)
        assert same_frame(ds.frame(i).frame, ds[i]), (name, i)


@pytest.mark.parametrize("workers", [1, 4])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", ["waymo", "kitti", "replica"])
def test_take_is_getitem(golden, tmp_path, name, depth, workers):
    ds = host_set(golden, tmp_path, name)
    with D.FramePrefetcher(ds, range(len(ds)), depth=depth, workers=workers) as pf:
        assert len(pf) == len(ds) and pf.fx == ds.fx and pf.device == "cpu" and pf.color_paths is ds.color_paths
        for i in range(len(ds)):
            assert same_frame(pf.take(i) if i % 2 else pf[i], ds[i]), (name, i)
    assert not prefetch_threads()


@pytest.mark.parametrize("depth", [1, 2])
def test_lookahead_is_bounded_and_a_file_is_decoded_once(golden, tmp_path, monkeypatch, depth):
    from PIL import Image
    ds = host_set(golden, tmp_path, "kitti")
    lock, reads, opened = threading.Lock(), [], []
    real_read, real_open = ds.read, Image.open

    def read(idx):
        with lock:
            reads.append(idx)
        return real_read(idx)

    def opening(p, *a, **k):
        with lock:
            opened.append(p)
        return real_open(p, *a, **k)

    ds.read = read
    monkeypatch.setattr(Image, "open", opening)
    n = len(ds)
    with D.FramePrefetcher(ds, range(n), depth=depth, workers=4) as pf:
        with lock:
            assert set(reads) <= set(range(depth))                 # nothing taken yet: the first `depth` frames at the most
        for i in range(n):
            pf.take(i)
            with lock:
                assert set(reads) <= set(range(i + depth + 1)), (i, sorted(reads))
    assert sorted(reads) == list(range(n))                          # every frame read once ...
    assert sorted(opened) == sorted(ds.color_paths)                 # ... and its one file (colour = both placeholders) opened once
    monkeypatch.undo()
    ws = host_set(golden, tmp_path, "waymo")
    monkeypatch.setattr(Image, "open", opening)
    del opened[:]
    with D.FramePrefetcher(ws, range(len(ws)), depth=depth, workers=2) as pf:
        for i in range(len(ws)):
            pf.take(i)
    assert sorted(opened) == sorted(ws.color_paths + ws.depth_paths + ws.mono_depth_paths)


def test_a_worker_s_error_is_raised_at_its_frame_s_turn(golden, tmp_path):
    from PIL import Image
    ds = host_set(golden, tmp_path, "waymo")
    Image.fromarray(np.zeros((32, 48), np.uint8)).save(ds.color_paths[2])                 # one channel
    with D.FramePrefetcher(ds, range(len(ds)), depth=3, workers=2) as pf:
        assert same_frame(pf.take(0), ds[0]) and same_frame(pf.take(1), ds[1])
        with pytest.raises(ValueError, match="three 8-bit channels"):
            pf.take(2)
        assert same_frame(pf.take(3), ds[3])                                              # the frames after it stay available
    assert not prefetch_threads()


def test_a_take_out_of_order_returns_the_right_frame(golden, tmp_path):
    ds = host_set(golden, tmp_path, "replica")
    with D.FramePrefetcher(ds, [0, 1, 2, 3], depth=2, workers=2) as pf:
        assert same_frame(pf.take(3), ds[3])          # not its turn: a direct read
        assert same_frame(pf.take(0), ds[0])
        assert same_frame(pf.take(2), ds[2])          # skipped 1
        assert same_frame(pf.take(1), ds[1])          # and back in order
        assert same_frame(pf.take(2), ds[2]) and same_frame(pf.take(3), ds[3])
        assert same_frame(pf.take(0), ds[0])          # past the end of the order
    with D.FramePrefetcher(ds, [2, 0], depth=1, workers=1) as pf:                         # any order, not only ascending
        assert same_frame(pf.take(2), ds[2]) and same_frame(pf.take(0), ds[0])


def test_no_thread_outlives_close_or_a_with_block_left_by_an_exception(golden, tmp_path):
    ds = host_set(golden, tmp_path, "kitti")
    pf = D.FramePrefetcher(ds, range(len(ds)), depth=2, workers=4)
    assert len(prefetch_threads()) == 4 and all(t.daemon for t in prefetch_threads())
    pf.take(0)
    pf.close()
    pf.close()
    assert not prefetch_threads()
    with pytest.raises(RuntimeError, match="close"):
        pf.take(1)
    with pytest.raises(KeyError):
        with D.FramePrefetcher(ds, range(len(ds)), depth=3, workers=3) as pf:
            pf.take(0)
            raise KeyError("the loop fails")
    assert not prefetch_threads()


def test_a_read_that_does_not_return_ends_in_a_timeout_not_a_hang(golden, tmp_path):
    ds = host_set(golden, tmp_path, "kitti")
    gate, real = threading.Event(), ds.read
    ds.read = lambda idx: (gate.wait(30), real(idx))[1]
    pf = D.FramePrefetcher(ds, range(len(ds)), depth=1, workers=1, timeout=0.05)
    with pytest.raises(TimeoutError, match="frame 0"):
        pf.take(0)
    gate.set()
    pf.close()
    assert not prefetch_threads()


def test_worker_count_and_depth_are_bounded(golden, tmp_path):
    ds = host_set(golden, tmp_path, "kitti")
    assert 1 <= D.PREFETCH_WORKERS <= 4 and D.PREFETCH_MAX_WORKERS == 16
    for kw in (dict(workers=0), dict(depth=0)):
        with pytest.raises(ValueError):
            D.FramePrefetcher(ds, range(len(ds)), **kw)
    with D.FramePrefetcher(ds, range(len(ds)), workers=40) as pf:       # capped, not refused
        assert len(prefetch_threads()) == 16 and same_frame(pf.take(0), ds[0])
    assert not prefetch_threads()
    with pytest.raises(TypeError, match="read / assemble"):
        D.FramePrefetcher([1, 2, 3], range(3))


# ---- the depth conversion on the host, and the C side without a GPU ----
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("divisor", DIVISORS)
def test_convert_depth_host_is_the_float64_division_and_the_cast(dtype, divisor):
    top = np.iinfo(dtype).max
    samples = np.arange(top + 1, dtype=np.int64).astype(dtype).reshape(-1, 16)      # every value of the type: 0, 1, 255 and 65535 among them
    got = D.convert_depth_host(samples, divisor)
    assert same_bits(got, (samples / divisor).astype(np.float32))           # NumPy: an integer array / a float is float64
    assert same_bits(got, (samples.astype(np.float64) / np.float64(divisor)).astype(np.float32))
    assert got.dtype == np.float32 and got[0, 0] == 0.0
    with pytest.raises(ValueError):
        D.convert_depth_host(samples.astype(np.int32), divisor)


def test_the_planes_of_a_tree_are_the_conversion_of_its_samples(golden, tmp_path):
    """What planes="device" computes from the samples is what the 4-tuple's float64 arrays give when cast: the two statements agree."""
    ds = host_set(golden, tmp_path, "waymo")
    rec = ds.read(1)
    samples = ds.load_image(ds.depth_paths[1])
    assert samples.dtype == np.uint16
    assert same_bits(D.convert_depth_host(samples, ds.depth_scale), rec.depth.astype(np.float32))
    assert same_bits(D.convert_depth_host(ds.load_image(ds.mono_depth_paths[1]), ds.depth_scale * 5), rec.mono_depth.astype(np.float32))


def valid_depth_args(**over):
    a = dict(width=16, height=8, src=256, sample_type=_lib.DEPTH_SAMPLE_BYTE, pixel_stride=1, src_row_bytes=16, divisor=5000.0, out=512)
    a.update(over)
    return _lib.IngestDepthArgs(**a)


def depth_refusals():
    """(what, changes to a valid argument block, a word of the message).  The pointers are never dereferenced: every call is refused
    before a launch."""
    word = dict(sample_type=_lib.DEPTH_SAMPLE_WORD, pixel_stride=2, src_row_bytes=32)
    return [("src NULL", dict(src=None), "NULL"), ("out NULL", dict(out=None), "NULL"),
            ("zero width", dict(width=0), "image size"), ("negative height", dict(height=-2), "image size"),
            ("zero divisor", dict(divisor=0.0), "divisor"), ("negative zero divisor", dict(divisor=-0.0), "divisor"),
            ("infinite divisor", dict(divisor=float("inf")), "divisor"), ("NaN divisor", dict(divisor=float("nan")), "divisor"),
            ("no sample type", dict(sample_type=0), "sample_type"), ("unknown sample type", dict(sample_type=3), "sample_type"),
            ("zero stride", dict(pixel_stride=0), "pixel_stride"), ("negative stride", dict(pixel_stride=-1), "pixel_stride"),
            ("byte stride for words", dict(word, pixel_stride=1), "pixel_stride"),
            ("short pitch", dict(src_row_bytes=15), "src_row_bytes"), ("short pitch, stride 3", dict(pixel_stride=3, src_row_bytes=47), "src_row_bytes"),
            ("short pitch, words", dict(word, src_row_bytes=30), "src_row_bytes"), ("negative pitch", dict(src_row_bytes=-16), "src_row_bytes"),
            ("odd address for words", dict(word, src=257), "even"), ("odd pitch for words", dict(word, src_row_bytes=33), "even"),
            ("odd stride for words", dict(word, pixel_stride=3, src_row_bytes=48), "even")]


def test_refusals_of_ingest_depth_without_a_gpu():
    L = _lib.lib()
    assert L.lvdgs_ingest_depth(None, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    for what, over, word in depth_refusals():
        assert L.lvdgs_ingest_depth(C.byref(valid_depth_args(**over)), None) == _lib.E_INVALID, what
        assert word.encode() in L.lvdgs_last_error(), (what, L.lvdgs_last_error())


def test_refusals_of_the_planes_mode(golden, tmp_path):
    cfg = rebuild_tree(golden, "waymo", tmp_path / "w")
    with pytest.raises(ValueError, match="ingest='fused'"):
        D.load_dataset(None, None, cfg, device="cpu", ingest="host", planes="device")
    with pytest.raises(ValueError, match="planes"):
        D.load_dataset(None, None, cfg, device="cpu", ingest="fused", planes="gpu")
    ds = D.load_dataset(None, None, cfg, device="cpu", ingest="fused", planes="device")   # no quiet fall-back to the host arrays
    with pytest.raises(_lib.LvdgsError, match="GPU"):
        ds[0]
    with pytest.raises(_lib.LvdgsError, match="GPU"):
        D.ingest_depth(torch.zeros((4, 4), dtype=torch.uint8), 5000.0)
    assert D.load_dataset(None, None, cfg, device="cpu").planes == "host"
    rec = ds.read(0)                                                                      # the host half needs no device
    assert rec.depth_samples.dtype == np.uint16 and rec.mono_samples.dtype == np.uint16 and rec.depth.dtype == np.float64
    kitti = D.load_dataset(None, None, rebuild_tree(golden, "kitti", tmp_path / "k"), device="cpu", ingest="fused", planes="device")
    rec = kitti.read(0)
    assert rec.depth_samples is None and rec.mono_samples is None                         # placeholders: the colour bytes serve
