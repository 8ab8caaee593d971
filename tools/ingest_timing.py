#!/usr/bin/env python3
"""Times a frame's way from decoded bytes to the (3, H, W) float32 tensor on the device, ``lvdgs.dataset``'s host mode (NumPy
undistortion and conversion, a float32 upload) against its fused mode (a byte upload and one ``lvdgs_ingest_frame`` call), with a device
synchronisation on either side of every timed call:

    python tools/ingest_timing.py [--repeats 20] [--out profiles/ingest_timing.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_timing.json"))
    a = ap.parse_args()
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
