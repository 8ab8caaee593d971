#!/usr/bin/env python3
"""Write frames of the synthetic drive (tools/sequence.py, lvdgs.synthetic) as a directory in the reference's waymo layout -- ``rgb/``,
``depth/``, ``mono_depth/`` (PNG; the depths 16-bit), ``gt/`` (one 4 x 4 camera-to-world matrix per frame) -- plus the YAML that opens it,
so the whole path from files on disk (lvdgs.config_utils.load_config, lvdgs.dataset.load_dataset, the frame ingest) through the loops
can run where no dataset exists:

    python tools/export_sequence_dir.py OUT_DIR [--frames 20] [--scale 0.5] [--cadence short] [--distortion K1 K2 P1 P2 K3]
    python tools/sequence.py --config OUT_DIR/sequence.yaml --ingest fused

What the files hold is what the loader gives back, not the in-memory drive: the image goes through 8 bits, the mono depth through
16 bits at ``depth_scale * 5`` counts per unit (``depth_scale`` is chosen so the deepest pixel fits), the static masks of a drive with
dynamic objects are not part of the layout.  With non-zero ``--distortion`` the calibration says ``distorted: True`` and the loader
undistorts the rendered frames -- a small warp of an image that had none, there to run the remap, not to model a lens."""
import argparse
import os
import sys

import numpy as np
import torch
import yaml
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _plain(x):
    """A settings tree of built-in types only (what yaml.safe_dump takes)."""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, (np.generic,)):
        return x.item()
    return x


def export_dataset(ds, cfg, out_dir, dist=(0.0, 0.0, 0.0, 0.0, 0.0), frames=None, yaml_name="sequence.yaml"):
    """Frames 0 .. ``frames`` - 1 of the ``SequenceDataset`` ``ds`` into ``out_dir`` and ``cfg`` (a merged settings tree) as the YAML
    beside them, its ``Dataset`` block rewritten to type ``waymo`` with this calibration.  Returns the YAML's path."""
    n = len(ds) if frames is None else min(int(frames), len(ds))
    for sub in ("rgb", "depth", "mono_depth", "gt"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    monos = [np.asarray(ds[i][3], np.float64) for i in range(n)]
    deepest = max(float(m.max()) for m in monos)
    depth_scale = float(np.floor(65535.0 / (5.0 * max(deepest, 1e-6)) * 0.98))     # mono counts = depth * depth_scale * 5 <= 65535
    for i in range(n):
        image, _, pose, _ = ds[i]
        rgb = (image.detach().float().clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
        Image.fromarray(rgb).save(os.path.join(out_dir, "rgb", f"{i:06d}.png"))
        mono16 = np.clip(np.rint(monos[i] * depth_scale * 5.0), 0, 65535).astype(np.uint16)
        depth16 = np.clip(np.rint(monos[i] * depth_scale), 0, 65535).astype(np.uint16)
        Image.fromarray(mono16).save(os.path.join(out_dir, "mono_depth", f"{i:06d}.png"))
        Image.fromarray(depth16).save(os.path.join(out_dir, "depth", f"{i:06d}.png"))
        c2w = np.linalg.inv(torch.as_tensor(pose).detach().double().cpu().numpy())
        with open(os.path.join(out_dir, "gt", f"{i:06d}.txt"), "w") as f:
            f.write(" ".join(repr(float(x)) for x in c2w.reshape(-1)) + "\n")
    out = _plain(cfg)
    out.pop("inherit_from", None)
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    out["Dataset"].update(type="waymo", dataset_path=os.path.abspath(out_dir))
    out["Dataset"].pop("begin", None)
    out["Dataset"].pop("end", None)
    out["Dataset"]["Calibration"] = dict(fx=float(ds.fx), fy=float(ds.fy), cx=float(ds.cx), cy=float(ds.cy), k1=k1, k2=k2, p1=p1, p2=p2, k3=k3,
                                         width=int(ds.width), height=int(ds.height), depth_scale=depth_scale, distorted=bool(any(dist)))
    path = os.path.join(out_dir, yaml_name)
    with open(path, "w") as f:
        yaml.safe_dump(out, f, sort_keys=True)
    return path


def main():
    import sequence as tool
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--cadence", choices=["reference", "short"], default="short")
    ap.add_argument("--geometry", choices=sorted(tool.GEOMETRY), default="kitti07")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--distortion", type=float, nargs=5, default=[0.0] * 5, metavar=("K1", "K2", "P1", "P2", "K3"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, ds, _ = tool.kitti_sequence(dev, a.frames, a.scale, a.cadence, masks=False, seed=a.seed, geometry=a.geometry)
    print(export_dataset(ds, cfg, a.out_dir, dist=a.distortion))


if __name__ == "__main__":
    main()
