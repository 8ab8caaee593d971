#!/usr/bin/env python3
"""Writes tests/golden/image_format.npz: what PIL gives on the image-formatting cases of tests/matcher_io_cases.py.

    python tests/golden/make_image_format_golden.py

The inputs are regenerated from seeds (tests/matcher_io_cases.py) and quantised as the reference quantises them
(tests/image_format_oracle.py ``quantise``); PIL then resizes and crops exactly as ``torch_images_to_dust3r_format`` does
(utils/init_pose.py:26-33, :59-69 of the reference).  Stored per case and kind: the SHA-256 of PIL's cropped uint8 image (what the
tests hold the oracle to), its rows 0, step, 2 step, ... (step 1: all of them, for outputs up to 40 KB; 32 above -- to see WHERE a
mismatch lies without carrying a megabyte of noise), and PIL's version."""
import hashlib
import os
import sys

import numpy as np
import PIL
import PIL.Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_format_oracle as fmt  # noqa: E402
import matcher_io_cases as mc  # noqa: E402


def pil_format(q, size):
    """(H, W, 3) uint8 -> the resized, cropped (H1, W1, 3) uint8, by PIL."""
    img = PIL.Image.fromarray(q, "RGB")
    S = max(img.size)
    interp = PIL.Image.LANCZOS if S > size else PIL.Image.BICUBIC
    img = img.resize(tuple(int(round(x * size / S)) for x in img.size), interp)
    W, H = img.size
    cx, cy = W // 2, H // 2
    halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    if W == H:
        halfh = 3 * halfw // 4
    return np.asarray(img.crop((cx - halfw, cy - halfh, cx + halfw, cy + halfh)))


def main():
    out = {"pil_version": np.array(PIL.__version__)}
    for name, (W, H, size, raster) in mc.FORMAT_CASES.items():
        for kind in mc.KINDS:
            got = pil_format(fmt.quantise(mc.image(name, kind)), size)
            assert got.shape == (raster[1], raster[0], 3), (name, got.shape)
            step = 1 if got.size <= 40_000 else 32
            out[f"{name}/{kind}/sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest())
            out[f"{name}/{kind}/step"] = np.array(step)
            out[f"{name}/{kind}/rows"] = np.ascontiguousarray(got[::step])
    path = os.path.join(HERE, "image_format.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
