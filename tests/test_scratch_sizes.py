"""Every ``lvdgs_*_bytes`` function of include/lvdgs.h, byte for byte against a recording (``tests/golden/scratch_sizes.json``).

A size function and the pointer binding of its entry point are one statement of the buffer's layout (csrc/carve.hpp); the sizes are
part of the ABI -- callers allocate by them, and a caller built against an older library must still bring enough.  The argument
tuples of each function, generated from its parameter names and types as the header declares them:
  * every refused or degenerate value of each parameter in turn (-1, 0, and 2^31 for an ``int64_t`` count), the others mid-size;
  * 1 everywhere;
  * counts just below, at and just above a 256-byte rounding of every element width in use -- 63 / 64 / 65 words, 31 / 32 / 33
    doubles, 255 / 256 / 257 bytes -- in every parameter at once and in each parameter with the others 1;
  * the mid-size shape of tests/test_api_refusals.py (N = 1000, 64 x 48, D = 5000) and one large shape (2^21 Gaussians, 1920 x 1080,
    2^26 pairs);
  * the render scratch: image sizes on both sides of ``group_max_tiles()`` (16384 tiles of 16 x 16), so that both grouping branches
    of ``render_scratch_layout`` are in the table.

``python tests/test_scratch_sizes.py`` records the file anew from the library in place (a build known to be good).
"""
import json
import os
import re
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import lvdgs  # noqa: F401  (registers the package alias)

from lvdgs import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scratch_sizes.json")
HEADER = os.path.join(os.path.dirname(HERE), "include", "lvdgs.h")

# parameter name -> (mid-size, large)
SHAPES = {
    "num_gaussians": (1000, 1 << 21), "num_points": (1000, 1 << 21), "num_rendered": (5000, 1 << 26),
    "width": (64, 1920), "height": (48, 1080), "width1": (64, 1920), "height1": (48, 1080),
    "planes": (1, 3), "patch_size": (8, 32), "subsample": (2, 8), "size": (224, 512), "history_length": (3, 16),
    "num_matches": (1000, 1 << 21), "hypotheses": (64, 4096),
    "nx": (8, 512), "ny": (6, 512), "nz": (5, 256), "pool_blocks": (1000, 1 << 20),
    "num_vertices": (1000, 1 << 21), "num_faces": (1000, 1 << 21), "num_queries": (1000, 1 << 21), "num_reference": (5000, 1 << 26),
    "total_pixels": (64 * 48, 1920 * 1080 * 16),
}
ROUNDINGS = (63, 64, 65, 31, 32, 33, 255, 256, 257)


def declared():
    """name -> [(type, parameter name), ...] of every lvdgs_*_bytes function the header declares, in its order."""
    out = {}
    for name, params in re.findall(r"^size_t (lvdgs_\w+_bytes)\(([^)]*)\);", open(HEADER).read(), re.M):
        out[name] = [] if params.strip() == "void" else [tuple(p.split()) for p in params.split(",")]
    return out


def tuples(name, params):
    mid = [SHAPES[p][0] for _, p in params]
    rows = []
    for i, (ctype, _) in enumerate(params):
        for bad in (-1, 0) + ((1 << 31,) if ctype == "int64_t" else ()):
            rows.append(mid[:i] + [bad] + mid[i + 1:])
    rows.append([1] * len(params))
    for c in ROUNDINGS:
        rows.append([c] * len(params))
        if len(params) > 1:
            rows += [[1] * i + [c] + [1] * (len(params) - i - 1) for i in range(len(params))]
    rows.append(mid)
    rows.append([SHAPES[p][1] for _, p in params])
    if name == "lvdgs_render_scratch_bytes":      # 128 x 128 tiles are the last image the counting path groups
        for w, h in ((2048, 2048), (2049, 2048), (2048, 2064), (2032, 2048), (4096, 4096)):
            rows += [[1000, 5000, w, h], [1 << 21, 1 << 26, w, h]]
    seen, unique = set(), []
    for r in rows:
        if tuple(r) not in seen:
            seen.add(tuple(r))
            unique.append(r)
    return unique


def measure(name, params):
    f = getattr(_lib.lib(), name)
    return [[args, int(f(*args))] for args in tuples(name, params)]


def test_the_recording_holds_every_size_function_of_the_header():
    golden, names = json.load(open(GOLDEN)), declared()
    assert set(golden) == set(names) and len(names) >= 32
    for name, params in names.items():
        assert [args for args, _ in golden[name]] == tuples(name, params), name
        assert name in _lib.EXPORTS, name


@pytest.mark.parametrize("name", sorted(declared()))
def test_sizes_are_the_recorded_ones(name):
    # (with the counting path switched off every image takes the radix branch: other sizes, by design)
    if name == "lvdgs_render_scratch_bytes" and os.environ.get("LVDGS_FORCE_RADIX_GROUPING"):
        pytest.skip("the counting path is switched off in the environment")
    want = json.load(open(GOLDEN))[name]
    got = measure(name, declared()[name])
    assert got == want, [(g, w[1]) for g, w in zip(got, want) if g != w][:8]


def test_both_grouping_branches_are_recorded():
    if os.environ.get("LVDGS_FORCE_RADIX_GROUPING"):
        pytest.skip("the counting path is switched off in the environment")
    L = _lib.lib()
    # the radix branch's histograms do not depend on the image, the counting branch's counters grow with its tiles
    assert L.lvdgs_render_scratch_bytes(1000, 5000, 2049, 2048) == L.lvdgs_render_scratch_bytes(1000, 5000, 4096, 4096)
    assert L.lvdgs_render_scratch_bytes(1000, 5000, 2048, 2048) > L.lvdgs_render_scratch_bytes(1000, 5000, 2032, 2048)


if __name__ == "__main__":
    out = {name: measure(name, params) for name, params in declared().items()}
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": [\n  %s\n ]' % (n, ",\n  ".join(json.dumps(r) for r in rows)) for n, rows in sorted(out.items())) + "\n}\n")
    print(sum(len(r) for r in out.values()), "sizes of", len(out), "functions recorded from", _lib.LIB_PATH)
