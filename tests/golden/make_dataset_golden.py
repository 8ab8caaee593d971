#!/usr/bin/env python3
"""Run the reference's OWN dataset classes -- ``KITTIDataset``, ``WaymoDataset``, ``dl3dvDataset``, ``ReplicaDataset``
(utils/dataset.py:25-163, :248-416) -- on tiny directory trees written here, and store the trees and what the classes returned as the
fixture ``lvdgs.dataset`` is held to.

Run in the authoring container only (needs the reference checkout; never on the GPU box):

    python -B tests/golden/make_dataset_golden.py

How the reference module is made to import and run here (CPU, no OpenCV):
  * ``gaussian_splatting`` resolves to the drop-in shims (lvd_gs-slam_amd/dropin), as in make_loop_golden.py;
  * ``cv2``, ``trimesh`` and ``pyrealsense2`` are stand-in modules: ``cv2.initUndistortRectifyMap`` returns ``(None, None)``,
    ``cv2.remap`` raises (every tree says ``distorted: False``, so it is never reached);
  * the constructed object's ``.device`` is set to ``"cpu"`` (the class hard-codes ``"cuda:0"``).
The TUM class is not run: its parser needs ``np.unicode_`` (gone in NumPy 2) and the real trimesh.

Fixture: tests/golden/dataset.npz.  Per tree ``<t>``:
  <t>/config            the settings the classes were given, as JSON (``dataset_path`` is relative: the tree's root)
  <t>/files             the relative names of every file of the tree; <t>/file/<i>: its bytes as uint8 (images as encoded, text as written),
                        so no encoder enters the comparison on another machine -- only PIL's decoder does
  <t>/color_order       the colour paths the class ended up with, relative to the root, in order (likewise depth_order, mono_order)
  <t>/image/<k>, <t>/depth/<k>, <t>/mono/<k>, <t>/pose/<k>    what ``dataset[k]`` returned
Nothing of the reference's text is stored."""
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LVDGS_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "lvd_gs-slam_amd", "dropin"), REF):
    sys.path.insert(0, p)

W, H, FRAMES = 48, 32, 4


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference():
    def no_remap(*a, **k):
        raise RuntimeError("cv2.remap is not available: the golden trees are undistorted")
    _stub("cv2", initUndistortRectifyMap=lambda *a, **k: (None, None), remap=no_remap, CV_32FC1=5, INTER_LINEAR=1)
    _stub("trimesh")
    _stub("pyrealsense2")
    import lvdgs  # noqa: F401  (the drop-in shims import it)
    return importlib.import_module("utils.dataset")


def encode(array, fmt, **kw):
    buf = io.BytesIO()
    Image.fromarray(array).save(buf, format=fmt, **kw)
    return buf.getvalue()


def colour(rng, i):
    """A frame with structure (so JPEG keeps some of it) and noise (so no two pixels decide alike)."""
    v, u = np.mgrid[0:H, 0:W]
    base = np.stack([(5 * u + 3 * v + 40 * i) % 256, (7 * v + 11 * i) % 256, (3 * u * v // 4 + 90 * i) % 256], axis=-1)
    return np.clip(base + rng.integers(-20, 21, size=(H, W, 3)), 0, 255).astype(np.uint8)


def depth16(rng, i):
    return rng.integers(0, 65536, size=(H, W)).astype(np.uint16)


def c2w(rng, first_translation):
    """A camera-to-world matrix: a small random rotation, a translation near ``first_translation``."""
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(0.2 * rng.standard_normal(3)).as_matrix()
    T[:3, 3] = np.asarray(first_translation) + rng.standard_normal(3)
    return T


def text(rows):
    return ("\n".join(" ".join(repr(float(x)) for x in r) for r in rows) + "\n").encode()


CAL = dict(fx=40.0, fy=41.0, cx=23.5, cy=15.25, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, width=W, height=H, distorted=False)


def tree_kitti(rng):
    files = {}
    for i in range(FRAMES + 2):                       # six frames; begin = 1, end = 5 keeps four
        files[f"image_2/{i:06d}.jpg"] = encode(colour(rng, i), "JPEG", quality=92)
        files[f"gt/{i:06d}.txt"] = (" ".join(repr(float(x)) for x in c2w(rng, (12.0, -3.0, 40.0))[:3].reshape(-1))).encode()
    cfg = {"Dataset": {"type": "KITTI", "begin": 1, "end": 5, "Calibration": dict(CAL, depth_scale=200.0)}}
    return files, cfg


def tree_dl3dv(rng):
    from scipy.spatial.transform import Rotation
    files, cams = {}, []
    for i in range(FRAMES + 3):                       # seven frames; begin = 2, end = 6 keeps four
        files[f"rgb/frame_{i:05d}.png"] = encode(colour(rng, i), "PNG")
        T = c2w(rng, (-7.0, 2.5, 1.0))
        cams.append({"cam_quat": [float(x) for x in Rotation.from_matrix(T[:3, :3]).as_quat()], "cam_trans": [float(x) for x in T[:3, 3]]})
    files["cameras.json"] = json.dumps(cams).encode()
    cfg = {"Dataset": {"type": "dl3dv", "begin": 2, "end": 6, "Calibration": dict(CAL, depth_scale=100.0)}}
    return files, cfg


def tree_waymo(rng):
    files = {}
    for i in range(FRAMES):
        files[f"rgb/{i:04d}.png"] = encode(colour(rng, i), "PNG")
        files[f"depth/{i:04d}.png"] = encode(depth16(rng, i), "PNG")
        files[f"mono_depth/{i:04d}.png"] = encode(depth16(rng, i), "PNG")
        files[f"gt/{i:04d}.txt"] = (" ".join(repr(float(x)) for x in c2w(rng, (3.0, 4.0, -5.0)).reshape(-1))).encode()
    cfg = {"Dataset": {"type": "waymo", "Calibration": dict(CAL, depth_scale=5000.0)}}
    return files, cfg


def tree_replica(rng):
    files, rows = {}, []
    for i in range(FRAMES):
        files[f"results/frame{i:06d}.png"] = encode(colour(rng, i), "PNG")
        files[f"results/depth{i:06d}.png"] = encode(depth16(rng, i), "PNG")
        files[f"results/mono{i:06d}.png"] = encode(colour(rng, i + 9), "PNG")      # a three-channel file: its first channel is read
        rows.append(c2w(rng, (0.5, -0.25, 2.0)).reshape(-1))
    files["traj.txt"] = text(rows)
    cfg = {"Dataset": {"type": "replica", "Calibration": dict(CAL, depth_scale=6553.5)}}
    return files, cfg


TREES = {"kitti": tree_kitti, "dl3dv": tree_dl3dv, "waymo": tree_waymo, "replica": tree_replica}


def write_tree(root, files):
    for name, data in files.items():
        path = os.path.join(root, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)


def main():
    ref = load_reference()
    out = {}
    for t, (tree_name, make) in enumerate(TREES.items()):
        rng = np.random.default_rng(4100 + t)
        files, cfg = make(rng)
        with tempfile.TemporaryDirectory() as tmp:
            root = os.path.join(tmp, tree_name) + "/"          # (the KITTI and replica parsers join "gt/" and "traj.txt" without a separator)
            write_tree(root, files)
            run_cfg = json.loads(json.dumps(cfg))
            run_cfg["Dataset"]["dataset_path"] = root
            ds = ref.load_dataset(None, None, run_cfg)
            ds.device = "cpu"
            assert len(ds) == FRAMES, (tree_name, len(ds))
            rel = lambda paths: np.array([os.path.relpath(p, root) for p in paths])
            out[f"{tree_name}/color_order"], out[f"{tree_name}/depth_order"], out[f"{tree_name}/mono_order"] = \
                rel(ds.color_paths), rel(ds.depth_paths), rel(ds.mono_depth_paths)
            for k in range(FRAMES):
                image, depth, pose, mono = ds[k]
                assert image.dtype.is_floating_point and tuple(image.shape) == (3, H, W)
                out[f"{tree_name}/image/{k}"] = image.numpy()
                out[f"{tree_name}/depth/{k}"] = np.asarray(depth)
                out[f"{tree_name}/mono/{k}"] = np.asarray(mono)
                out[f"{tree_name}/pose/{k}"] = pose.numpy()
        out[f"{tree_name}/config"] = np.array(json.dumps(cfg, sort_keys=True))
        names = sorted(files)
        out[f"{tree_name}/files"] = np.array(names)
        for i, name in enumerate(names):
            out[f"{tree_name}/file/{i}"] = np.frombuffer(files[name], dtype=np.uint8)
    path = os.path.join(HERE, "dataset.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
