#!/usr/bin/env python3
"""Run the reference's OWN ``process_depth`` (utils/depth_utils.py, LVD-GS Algorithm 1) on the cases of tests/depth_align_cases.py
and store what it computed, as the fixture the oracle (tests/test_depth_align.py) and the HIP path (tests/test_gpu_depth_align.py)
are checked against.

Run in the authoring container only (needs the reference checkout; never on the GPU box):

    python -B tests/golden/make_depth_align_golden.py

How the reference module is made to load here (CPU, no MASt3R / dust3r / cv2), as make_loop_golden.py does for the loops:
  * its imports of ``mast3r.*``, ``dust3r.*``, ``cv2`` and ``utils.init_pose`` resolve to empty stand-in modules;
  * ``find_scale`` in the module's namespace is replaced by ``depth_align_cases.RecordedRemedy``: the case's recorded scales, call
    after call (the remedy needs MASt3R, out of scope);
  * stdout is captured for the number of passing patches the function prints.
Nothing of the reference's text is stored: only the SHA-256 of the inputs (regenerated from seeds by the tests) and the numbers
and packed masks the function returned.

Fixture: tests/golden/depth_align.npz
"""
import contextlib
import importlib.util
import io
import json
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LVDGS_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_align_cases as dc  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference():
    nothing = lambda *a, **k: None  # noqa: E731
    for name in ("mast3r", "mast3r.utils", "mast3r.utils.path_to_dust3r", "dust3r", "cv2"):
        _stub(name)
    _stub("mast3r.model", AsymmetricMASt3R=object)
    _stub("mast3r.fast_nn", fast_reciprocal_NNs=nothing)
    _stub("dust3r.inference", inference=nothing)
    _stub("dust3r.cloud_opt", global_aligner=nothing, GlobalAlignerMode=object)
    pkg = _stub("utils")
    pkg.__path__ = [os.path.join(REF, "utils")]
    _stub("utils.init_pose", _resize_pil_image=nothing, torch_images_to_dust3r_format=nothing)
    spec = importlib.util.spec_from_file_location("utils.depth_utils", os.path.join(REF, "utils", "depth_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["utils.depth_utils"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    out, meta = {}, {}
    for name in dc.CASES:
        r, m, kw, remedy = dc.make_case(name)
        stand_in = dc.RecordedRemedy(remedy)
        ref.find_scale = stand_in
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            final, scale, err, num_acc = ref.process_depth(r, m, None, None, None, None, **kw)
        patch_num = [int(x) for x in re.findall(r"filtering:\s+(\d+)", buf.getvalue())]
        assert len(patch_num) == 1, buf.getvalue()
        err = np.asarray(err, bool)
        out[name + "/scale"] = np.float32(scale)
        out[name + "/ints"] = np.array([int(num_acc), patch_num[0], stand_in.calls], np.int64)
        out[name + "/error_mask"] = np.packbits(err.ravel())
        meta[name] = dict(shape=list(r.shape), kwargs=kw, remedy=remedy, input_sha256=dc.sha256(r, m),
                          final_depth_sha256=dc.sha256(np.asarray(final, np.float32)), scale_type=type(scale).__name__)
        print(f"{name:22s} {r.shape} scale {float(scale):.7f} accurate {int(num_acc)} patches {patch_num[0]} remedy calls {stand_in.calls}")
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    np.savez_compressed(os.path.join(HERE, "depth_align.npz"), **out)


if __name__ == "__main__":
    main()
