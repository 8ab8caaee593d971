#!/usr/bin/env python3
"""Times a frame's way from decoded bytes to the (3, H, W) float32 tensor on the device, ``lvdgs.dataset``'s host mode (NumPy
undistortion and conversion, a float32 upload) against its fused mode (a byte upload and one ``lvdgs_ingest_frame`` call), with a device
synchronisation on either side of every timed call:

    python tools/ingest_timing.py [--repeats 20] [--out profiles/ingest_timing.json]

    python tools/ingest_timing.py --decode-scaling [--frames 16]      # no GPU: frames per second of ``dataset.read`` with 1, 2, 4 and 8 threads
    python tools/ingest_timing.py --prefetch [--frames 16] [--pause-ms 30] [--rounds 3]
                                                                      # a loop of ``dataset[i]`` against ``FramePrefetcher.take(i)``

The last two write their section of profiles/ingest_prefetch.json, over directories of patterned frames (rgb, 16-bit depth and mono-depth
PNGs) made in a temporary place.  ``--prefetch`` alternates the two loaders in one process, ``--rounds`` times each: the plain loop is
``dataset[i]`` with fused ingest; the other takes from a prefetcher (``--depth`` frames ahead, ``planes="device"``); after every frame the
loop synchronises and then sleeps ``--pause-ms``, which stands for the loops' own work.  Reported: the median milliseconds a frame's
fetch held the loop up.

Two frames: 1226 x 370 without distortion (KITTI-07) and 1920 x 1280 with the coefficients of tests/golden/configs/mono/waymo/405841.yaml.
Reported per frame: the PNG decode (PIL, the same in both modes, so outside both columns), each mode's milliseconds (median and best of
``--repeats``), and the call alone on bytes already on the device (wall time, and the launch by HIP events).  The host column is THIS
package's NumPy restatement of the remap, not ``cv2.remap``: OpenCV is not installed and its time cannot be measured here.  No time is
asserted anywhere."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lvdgs  # noqa: E402,F401
from lvdgs import _lib, dataset as D  # noqa: E402
from lvdgs.config_utils import load_config  # noqa: E402

WAYMO = os.path.join(ROOT, "tests", "golden", "configs", "mono", "waymo", "405841.yaml")
KITTI = os.path.join(ROOT, "tests", "golden", "configs", "mono", "KITTI", "07.yaml")


def timed(fn, repeats, dev):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=round(statistics.median(out), 4), best_ms=round(min(out), 4))


def frame_record(yaml_path, dev, repeats):
    cfg = load_config(yaml_path)
    cfg["Dataset"]["dataset_path"] = "."
    sets = {m: D.MonocularDataset(None, None, cfg, device=dev, ingest=m) for m in ("host", "fused")}
    W, H = sets["host"].width, sets["host"].height
    v, u = np.mgrid[0:H, 0:W]
    raw = np.stack([(u + v) % 256, (3 * u) % 256, (5 * v + u // 7) % 256], axis=-1).astype(np.uint8)
    raw = np.ascontiguousarray((raw + np.random.default_rng(0).integers(0, 32, raw.shape)).astype(np.uint8))
    buf = io.BytesIO()
    Image.fromarray(raw).save(buf, format="PNG")
    png = buf.getvalue()
    decode = []
    for _ in range(max(3, repeats // 4)):
        t0 = time.perf_counter()
        np.array(Image.open(io.BytesIO(png)))
        decode.append(1e3 * (time.perf_counter() - t0))
    for ds in sets.values():               # the map of the calibration, once per dataset: outside the per-frame time
        if ds.disorted:
            ds.undistort_map()
        ds.ingest_image(raw)
    assert torch.equal(sets["host"].ingest_image(raw), sets["fused"].ingest_image(raw))
    rec = dict(frame=f"{W}x{H}", distorted=bool(sets["host"].disorted), decode_png_ms=round(statistics.median(decode), 3),
               host=timed(lambda: sets["host"].ingest_image(raw), repeats, dev), fused=timed(lambda: sets["fused"].ingest_image(raw), repeats, dev))
    on_device = torch.from_numpy(raw).to(dev)
    sx, sy = sets["fused"].undistort_map() if sets["fused"].disorted else (None, None)
    rec["kernel_only"] = timed(lambda: D.ingest_frame(on_device, sx, sy), repeats, dev)
    _lib.profile_enable(True)            # the launch alone, by HIP events around it on the stream
    _lib.profile_reset()
    for _ in range(repeats):
        D.ingest_frame(on_device, sx, sy)
    torch.cuda.synchronize(dev)
    launches, total_ms = _lib.profile_read()["ingest_frame"]
    _lib.profile_enable(False)
    moved = (3 + 12 + (8 if sx is not None else 0)) * W * H
    rec["kernel_event_us"] = round(1e3 * total_ms / launches, 2)
    rec["kernel_bytes_moved"] = moved
    rec["kernel_tb_per_s"] = round(moved / (1e-3 * total_ms / launches) / 1e12, 2)
    rec["bytes_uploaded"] = dict(host=12 * W * H, fused=3 * W * H)
    rec["speedup_median"] = round(rec["host"]["median_ms"] / rec["fused"]["median_ms"], 2)
    return rec


def patterned_tree(root, yaml_path, frames):
    """``frames`` patterned frames of the calibration's size in the waymo layout under ``root`` -> the settings."""
    cfg = load_config(yaml_path)
    cal = cfg["Dataset"]["Calibration"]
    W, H = cal["width"], cal["height"]
    cfg["Dataset"].update(type="waymo", dataset_path=root)
    cal.setdefault("depth_scale", 256.0)
    for sub in ("rgb", "depth", "mono_depth", "gt"):
        os.makedirs(os.path.join(root, sub))
    v, u = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(0)
    for i in range(frames):
        raw = np.stack([(u + v + 3 * i) % 256, (3 * u + i) % 256, (5 * v + u // 7) % 256], axis=-1)
        Image.fromarray((raw + rng.integers(0, 32, raw.shape)).astype(np.uint8)).save(os.path.join(root, "rgb", f"{i:06d}.png"))
        z = (20000 + 8000 * np.sin(u / 97.0 + i) * np.cos(v / 61.0) + rng.integers(0, 64, (H, W))).astype(np.uint16)
        Image.fromarray(z).save(os.path.join(root, "mono_depth", f"{i:06d}.png"))
        Image.fromarray((z // 5).astype(np.uint16)).save(os.path.join(root, "depth", f"{i:06d}.png"))
        np.savetxt(os.path.join(root, "gt", f"{i:06d}.txt"), np.eye(4).reshape(1, 16), delimiter=" ")
    return cfg


def decode_scaling(frames):
    """Frames per second of ``dataset.read`` alone (decode and the two divisions) over 1, 2, 4 and 8 threads: no device is touched."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    out = []
    for yaml_path in (KITTI, WAYMO):
        with tempfile.TemporaryDirectory() as root:
            ds = D.load_dataset(None, None, patterned_tree(root, yaml_path, frames), device="cpu")
            ds.read(0)
            rec = dict(frame=f"{ds.width}x{ds.height}", frames=frames, files_per_frame=3)
            for workers in (1, 2, 4, 8):
                rates = []
                for _ in range(3):
                    with ThreadPoolExecutor(workers) as pool:
                        t0 = time.perf_counter()
                        list(pool.map(ds.read, range(frames)))
                        rates.append(frames / (time.perf_counter() - t0))
                rec[f"frames_per_s_{workers}"] = round(statistics.median(rates), 2)
            rec["ms_per_frame_1"] = round(1e3 / rec["frames_per_s_1"], 2)
            out.append(rec)
    return out


def prefetch_record(yaml_path, dev, frames, pause_ms, rounds, depth, workers):
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        cfg = patterned_tree(root, yaml_path, frames)
        plain = D.load_dataset(None, None, cfg, device=dev, ingest="fused")
        ahead = D.load_dataset(None, None, cfg, device=dev, ingest="fused", planes="device")
        plain[0], ahead[0]                                  # the calibration's map, the library, the allocator: outside the time

        def loop(take):
            held, t_all = [], time.perf_counter()
            for i in range(frames):
                t0 = time.perf_counter()
                frame = take(i)
                torch.cuda.synchronize(dev)
                held.append(1e3 * (time.perf_counter() - t0))
                del frame
                time.sleep(pause_ms * 1e-3)
            return held, 1e3 * (time.perf_counter() - t_all) / frames

        held = {"dataset[i]": [], "take(i)": []}
        wall = {"dataset[i]": [], "take(i)": []}
        for _ in range(rounds):
            h, w = loop(plain.__getitem__)
            held["dataset[i]"] += h[1:]
            wall["dataset[i]"].append(w)
            with D.FramePrefetcher(ahead, range(frames), depth=depth, workers=workers) as pf:
                time.sleep(pause_ms * 1e-3)                 # the loop's work on the frame before the first
                h, w = loop(pf.take)
            held["take(i)"] += h[1:]                        # (the first frame of a loop has nothing running ahead of it)
            wall["take(i)"].append(w)
        rec = dict(frame=f"{plain.width}x{plain.height}", distorted=bool(plain.disorted), frames=frames, pause_ms=pause_ms, rounds=rounds,
                   depth=depth, workers=workers)
        for k in held:
            rec[k] = dict(held_up_median_ms=round(statistics.median(held[k]), 3), held_up_worst_ms=round(max(held[k]), 3),
                          wall_ms_per_frame_median=round(statistics.median(wall[k]), 3))
        return rec


def merge_section(path, key, value, **head):
    out = {}
    if os.path.isfile(path):
        with open(path) as f:
            out = json.load(f)
    out.update(head)
    out[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({key: value}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--decode-scaling", action="store_true")
    ap.add_argument("--prefetch", action="store_true")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--pause-ms", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--workers", type=int, default=D.PREFETCH_WORKERS)
    a = ap.parse_args()
    if a.decode_scaling or a.prefetch:
        path = a.out or os.path.join(ROOT, "profiles", "ingest_prefetch.json")
        if a.decode_scaling:
            merge_section(path, "decode_scaling", decode_scaling(a.frames), decode_scaling_host_cpus_used="1, 2, 4, 8 threads of one process")
        if a.prefetch:
            dev = torch.device("cuda", 0)
            merge_section(path, "prefetch", [prefetch_record(y, dev, a.frames, a.pause_ms, a.rounds, a.depth, a.workers) for y in (KITTI, WAYMO)],
                          device=torch.cuda.get_device_name(dev))
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "ingest_timing.json")
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, numpy=np.__version__,
               note="host = lvdgs.dataset's NumPy restatement + float32 upload, not cv2.remap (OpenCV is not installed); decode is outside both columns",
               frames=[frame_record(KITTI, dev, a.repeats), frame_record(WAYMO, dev, a.repeats)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
