#!/usr/bin/env python3
"""Records tests/golden/quadrant_test.npz: what the library computes on the quadrant-test scene (tests/quadrant_scene.py).

Run it on a GPU with the library of the commit BEFORE the change under test (LVDGS_LIB=<that build's liblvdgs.so>): the
fixture is what tests/test_gpu_quadrant_test.py holds the current build to, bit for bit.

    LVDGS_LIB=/path/to/parent/liblvdgs.so python3 tests/golden/make_quadrant_test_golden.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lvdgs  # noqa: E402,F401
import quadrant_scene  # noqa: E402

if __name__ == "__main__":
    from lvdgs import _lib
    results = quadrant_scene.collect()
    path = sys.argv[1] if len(sys.argv) > 1 else quadrant_scene.GOLDEN
    np.savez_compressed(path, **quadrant_scene.pack(results))
    lengths = results["calls/list_lengths"]
    print(f"{path}: {len(results)} arrays, {os.path.getsize(path)} bytes, library {_lib.LIB_PATH} {_lib.lib().lvdgs_version().decode()}; "
          f"pairs {int(results['calls/pairs'][0])}, tile lists {sorted(lengths.tolist())[-4:]} longest, "
          f"pixels with transmittance below 1e-4: {int((results['calls/final_T'] < 1e-4).sum())} of {lengths.size * 256}")
