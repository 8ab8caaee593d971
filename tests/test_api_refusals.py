"""Every refusal of the rasterizer's entry points (csrc/api.hip), status and full message, against a recording.

Each case starts from one valid-looking call -- fake non-NULL pointers, buffer sizes exactly what the library asks for -- and breaks
ONE thing; the library must refuse it before a launch or any HIP call (no pointer here is ever dereferenced), with the status and
the ``lvdgs_last_error()`` text recorded in ``tests/golden/api_refusals.json``.  One broken thing per case, so the order of the
checks inside an entry point is free to change; what is refused, and in which words, is not.

``python tests/test_api_refusals.py`` records the file anew from the library in place (a build known to be good).
"""
import ctypes as C
import json
import os
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import lvdgs  # noqa: F401  (registers the package alias)

from lvdgs import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_refusals.json")
N, W, H, CAP = 1000, 64, 48, 5000
ROOMY = 1 << 40   # a buffer size no case outgrows: for cases whose broken thing would make a size too small as well

_fake = [1 << 20]


def fake():
    _fake[0] += 4096
    return _fake[0]


def scratch_bytes(entry):
    L = _lib.lib()
    prep, render, bwd = L.lvdgs_prepare_scratch_bytes(N), L.lvdgs_render_scratch_bytes(N, CAP, W, H), L.lvdgs_backward_scratch_bytes(N, CAP)
    assert prep <= render
    if entry == "forward_prepare":
        return prep
    if entry in ("forward", "forward_render", "forward_batch", "blend_forward_batch"):
        return render
    return max(render, bwd) if entry == "forward_backward_fused_loss" else bwd


def valid_args(entry):
    L = _lib.lib()
    a = _lib.Args()
    a.image_width, a.image_height, a.tanfovx, a.tanfovy, a.scale_modifier = W, H, 1.0, 1.0, 1.0
    a.num_gaussians, a.sh_coeffs, a.num_rendered, a.pair_capacity = N, 1, CAP, CAP
    for f in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos", "means3D", "opacities", "scales", "rotations", "shs",
              "geom_state", "binning_state", "image_state", "scratch", "radii", "out_color", "out_depth", "out_opacity", "n_touched",
              "dL_dout_color", "dL_dmeans3D", "dL_dmeans2D", "dL_dopacities", "dL_dscales", "dL_drotations", "dL_dshs", "dL_dtau"):
        setattr(a, f, fake())
    a.geom_bytes, a.binning_bytes, a.image_bytes = L.lvdgs_geom_bytes(N), L.lvdgs_binning_bytes(CAP), L.lvdgs_image_bytes(W, H)
    a.scratch_bytes = scratch_bytes(entry)
    return a


def another_view(a):
    """A second view of the same map: the map's and the gradients' pointers shared, state and outputs its own."""
    b = _lib.Args.from_buffer_copy(a)
    for f in ("viewmatrix", "projmatrix", "projmatrix_raw", "campos", "geom_state", "binning_state", "image_state", "scratch", "radii",
              "out_color", "out_depth", "out_opacity", "n_touched", "dL_dmeans2D", "dL_dtau"):
        setattr(b, f, fake())
    return b


def valid_loss():
    lo = _lib.LossArgs()
    lo.width, lo.height, lo.weight_rgb = W, H, 1.0
    lo.image, lo.gt_image, lo.scratch = fake(), fake(), fake()
    lo.scratch_bytes = _lib.lib().lvdgs_loss_scratch_bytes(W, H)
    return lo


def valid_masked():
    m = _lib.MaskedLossArgs()
    m.width, m.height = W, H
    m.d_image, m.out = fake(), fake()
    return m


class Call:
    """The arguments of one call of `entry`, valid until a case breaks them."""

    def __init__(self, entry):
        self.entry = entry
        self.a = valid_args(entry)
        self.b = another_view(self.a)
        if entry == "gaussian_backward_batch":
            self.b.flags = _lib.FLAG_ACCUMULATE_PARAM_GRADS
        self.loss, self.loss_b = valid_loss(), valid_loss()
        self.masked, self.masked_b = valid_masked(), valid_masked()
        self.args_null = self.n_null = self.views_null = self.losses_null = False
        self.views = [self.a, self.b]          # (an entry None: a NULL view)
        self.losses = [self.loss, self.loss_b]   # (None: no lvdgs_loss_args list)
        self.maskeds = None                      # (a list: the views are scored by the static-mask loss)
        self.count = 2

    def run(self):
        L = _lib.lib()
        a = None if self.args_null else C.byref(self.a)
        n = (C.c_int64 * 2)(-1, -1)
        np_ = None if self.n_null else n
        ptrs = lambda cls, xs: None if xs is None else (C.POINTER(cls) * len(xs))(*[None if x is None else C.pointer(x) for x in xs])
        views = None if self.views_null else ptrs(_lib.Args, self.views)
        losses = None if self.losses_null else ptrs(_lib.LossArgs, self.losses)
        e = self.entry
        if e == "forward_prepare":
            st = L.lvdgs_forward_prepare(a, np_, None)
        elif e == "forward":
            st = L.lvdgs_forward(a, np_, None)
        elif e == "forward_render":
            st = L.lvdgs_forward_render(a, None)
        elif e == "forward_batch":
            st = L.lvdgs_forward_batch(views, self.count, np_, None)
        elif e == "forward_backward_fused_loss":
            st = L.lvdgs_forward_backward_fused_loss(a, C.byref(self.loss) if self.loss is not None else None, 0, np_, None)
        elif e == "backward":
            st = L.lvdgs_backward(a, None)
        elif e == "backward_fused_loss":
            st = L.lvdgs_backward_fused_loss(a, C.byref(self.loss) if self.loss is not None else None, 0, None)
        elif e == "backward_masked_loss":
            st = L.lvdgs_backward_masked_loss(a, C.byref(self.masked) if self.masked is not None else None, None)
        elif e == "blend_forward_batch":
            st = L.lvdgs_blend_forward_batch(views, self.count, None)
        elif e == "blend_backward_window_batch":
            st = L.lvdgs_blend_backward_window_batch(views, losses, ptrs(_lib.MaskedLossArgs, self.maskeds), self.count, 0, None)
        elif e == "gaussian_backward_batch":
            st = L.lvdgs_gaussian_backward_batch(views, self.count, None)
        else:
            raise KeyError(e)
        return int(st), L.lvdgs_last_error().decode()


def put(view, **fields):
    """The case that sets fields of c.<view> ('a', 'b', 'loss', 'loss_b', 'masked', 'masked_b') or of the call itself ('c')."""
    def mutate(c):
        target = c if view == "c" else getattr(c, view)
        for f, v in fields.items():
            setattr(target, f, v)
    return mutate


def both(**fields):
    return lambda c: (put("a", **fields)(c), put("b", **fields)(c))


def short(view, field):
    return lambda c: setattr(getattr(c, view), field, getattr(getattr(c, view), field) - 1)


def roomy(view, **fields):
    """... with every buffer of the view large enough for anything, so that only the fields set are wrong."""
    return put(view, geom_bytes=ROOMY, binning_bytes=ROOMY, image_bytes=ROOMY, scratch_bytes=ROOMY, **fields)


def chain(*ms):
    return lambda c: [m(c) for m in ms]


def view_list(i, v):
    def mutate(c):
        c.views[i] = v
    return mutate


POSE_ONLY, ACCUMULATE, NO_BLEND = _lib.FLAG_POSE_ONLY, _lib.FLAG_ACCUMULATE_PARAM_GRADS, _lib.FLAG_NO_BLEND

# what check_common and check_gaussians refuse, on view `v`
COMMON = lambda v: [
    ("width_0", put(v, image_width=0)), ("height_0", put(v, image_height=0)), ("negative_N", put(v, num_gaussians=-1)),
    ("tanfovx_0", put(v, tanfovx=0.0)), ("tanfovy_negative", put(v, tanfovy=-1.0)), ("sh_degree_4", put(v, sh_degree=4)),
    ("bg_null", put(v, bg=None)), ("viewmatrix_null", put(v, viewmatrix=None)), ("projmatrix_null", put(v, projmatrix=None)),
]
GAUSSIANS = lambda set_: [
    ("means3D_null", set_(means3D=None)), ("opacities_null", set_(opacities=None)), ("shs_and_colors", set_(colors_precomp=4096)),
    ("no_colour", set_(shs=None)), ("scales_without_rotations", set_(rotations=None)), ("scales_and_cov3D", set_(cov3D_precomp=4096)),
    ("campos_null", set_(campos=None)), ("sh_coeffs_too_few", set_(sh_degree=1)),
]
# the geometry half and the render half of "a forward with a pair capacity", on view `v`
FORWARD_GEOM = lambda v: [
    ("radii_null", put(v, radii=None)), ("geom_state_null", put(v, geom_state=None)), ("scratch_null", put(v, scratch=None)),
    ("geom_bytes_short", short(v, "geom_bytes")),
]
RENDER_BUFFERS = lambda v: [
    ("out_color_null", put(v, out_color=None)), ("out_depth_null", put(v, out_depth=None)), ("out_opacity_null", put(v, out_opacity=None)),
    ("image_state_null", put(v, image_state=None)), ("image_bytes_short", short(v, "image_bytes")), ("n_touched_null", put(v, n_touched=None)),
    ("binning_state_null", put(v, binning_state=None)), ("binning_bytes_short", short(v, "binning_bytes")),
    ("scratch_bytes_short", short(v, "scratch_bytes")),
]
CAPACITY = lambda v: [("capacity_0", put(v, pair_capacity=0)), ("capacity_2_31", roomy(v, pair_capacity=1 << 31))]
# what the check of a backward call refuses, on view `v` (pixel gradients supplied: dL_dout_color too)
BACKWARD = lambda v: [
    ("negative_num_rendered", put(v, num_rendered=-1)), ("image_state_null", put(v, image_state=None)), ("image_bytes_short", short(v, "image_bytes")),
    ("projmatrix_raw_null", put(v, projmatrix_raw=None)), ("radii_null", put(v, radii=None)),
    ("pose_only_view_dependent_colour", put(v, flags=POSE_ONLY, sh_degree=1, sh_coeffs=4)), ("pose_only_accumulate", put(v, flags=POSE_ONLY | ACCUMULATE)),
    ("dL_dmeans3D_null", put(v, dL_dmeans3D=None)), ("dL_dmeans2D_null", put(v, dL_dmeans2D=None)), ("dL_dopacities_null", put(v, dL_dopacities=None)),
    ("dL_dscales_null", put(v, dL_dscales=None)), ("dL_drotations_null", put(v, dL_drotations=None)),
    ("dL_dcov3D_null", put(v, scales=None, rotations=None, cov3D_precomp=4096)), ("dL_dshs_null", put(v, dL_dshs=None)),
    ("dL_dcolors_null", put(v, shs=None, colors_precomp=4096)),
    ("geom_state_null", put(v, geom_state=None)), ("scratch_null", put(v, scratch=None)), ("binning_state_null", put(v, binning_state=None)),
    ("geom_bytes_short", short(v, "geom_bytes")), ("binning_bytes_short", short(v, "binning_bytes")), ("scratch_bytes_short", short(v, "scratch_bytes")),
]
LOSS = lambda lo: [
    ("loss_image_null", put(lo, image=None)), ("loss_gt_image_null", put(lo, gt_image=None)), ("loss_scratch_null", put(lo, scratch=None)),
    ("loss_scratch_short", short(lo, "scratch_bytes")), ("loss_opacity_null", put(lo, weight_by_opacity=1)),
    ("loss_width_differs", put(lo, width=W + 1, scratch_bytes=ROOMY)), ("loss_height_differs", put(lo, height=H + 1, scratch_bytes=ROOMY)),
]
MASKED = lambda m, v: [
    ("masked_d_image_null", put(m, d_image=None)), ("masked_out_null", put(m, out=None)), ("masked_width_differs", put(m, width=W + 1)),
    ("masked_height_differs", put(m, height=H + 1)), ("masked_gt_depth_without_depth", put(m, gt_depth=4096)),
    ("masked_in_a_band", put(v, tile_row_begin=1, tile_row_end=2)), ("masked_pose_only", put(v, flags=POSE_ONLY)),
]
ONE_FRAME = lambda v: [   # views of one frame: what the second may not differ in
    ("width_differs", roomy(v, image_width=W + 16)), ("height_differs", roomy(v, image_height=H + 16)),
    ("row_begin_differs", put(v, tile_row_begin=1)), ("row_end_differs", put(v, tile_row_end=1)),
]
VIEW_LIST = [("count_negative", put("c", count=-1)), ("views_null", put("c", views_null=True)), ("view_0_null", view_list(0, None)),
             ("view_1_null", view_list(1, None))]

CASES = {}
for entry, cases in {
    "forward_prepare": [("args_null", put("c", args_null=True)), ("num_rendered_null", put("c", n_null=True)),
                        ("image_too_large", put("a", image_width=16 * 2049, image_height=16 * 2049)),
                        ("scratch_bytes_short", short("a", "scratch_bytes"))]
                       + COMMON("a") + GAUSSIANS(lambda **f: put("a", **f)) + FORWARD_GEOM("a"),
    "forward": [("args_null", put("c", args_null=True)), ("num_rendered_null", put("c", n_null=True)),
                ("empty_map_image_state_null", put("a", num_gaussians=0, image_state=None)), ("sh_degree_4", put("a", sh_degree=4)),
                ("means3D_null", put("a", means3D=None))]
               + CAPACITY("a") + FORWARD_GEOM("a") + RENDER_BUFFERS("a"),
    "forward_render": [("args_null", put("c", args_null=True)), ("negative_num_rendered", put("a", num_rendered=-1)), ("sh_degree_4", put("a", sh_degree=4)),
                       ("geom_state_null", put("a", geom_state=None)), ("scratch_null", put("a", scratch=None))]
                      + RENDER_BUFFERS("a"),
    "forward_batch": VIEW_LIST + [
        ("num_rendered_null", put("c", n_null=True)), ("empty_map", both(num_gaussians=0)), ("sh_degree_4", put("b", sh_degree=4)),
        ("means3D_null", both(means3D=None)),
        ("too_many_tiles", chain(roomy("a", image_width=4096, image_height=4096), roomy("b", image_width=4096, image_height=4096))),
        ("N_differs", put("b", num_gaussians=N - 1)), ("means3D_differs", put("b", means3D=4096)), ("opacities_differs", put("b", opacities=4096)),
        ("scales_differs", put("b", scales=4096)), ("rotations_differs", put("b", rotations=4096)),
        ("cov3D_differs", put("b", scales=None, rotations=None, cov3D_precomp=4096)), ("shs_differs", put("b", shs=4096)),
        ("colors_differs", put("b", shs=None, colors_precomp=4096)), ("sh_coeffs_differs", put("b", sh_coeffs=4)), ("activations_differs", put("b", activations=1)),
        ("list_all_tiles_differs", put("b", flags=_lib.FLAG_LIST_ALL_TILES)), ("no_blend_differs", put("b", flags=NO_BLEND)),
        ("super_tiles_differs", put("b", flags=_lib.FLAG_SUPER_TILES))]
        + ONE_FRAME("b") + CAPACITY("b") + FORWARD_GEOM("b") + RENDER_BUFFERS("b"),
    "forward_backward_fused_loss": [("args_null", put("c", args_null=True)), ("num_rendered_null", put("c", n_null=True)), ("loss_null", put("c", loss=None)),
                                    ("sh_degree_4", put("a", sh_degree=4)), ("means3D_null", put("a", means3D=None))]
                                   + CAPACITY("a") + LOSS("loss") + FORWARD_GEOM("a")
                                   + [c for c in RENDER_BUFFERS("a") if c[0] != "scratch_bytes_short"]   # (the backward's records are the larger need)
                                   + [c for c in BACKWARD("a") if c[0] not in ("negative_num_rendered", "image_state_null", "image_bytes_short", "radii_null",
                                                                               "geom_state_null", "scratch_null", "binning_state_null", "geom_bytes_short",
                                                                               "binning_bytes_short")],
    "backward": [("args_null", put("c", args_null=True)), ("no_blend", put("a", flags=NO_BLEND)), ("dL_dout_color_null", put("a", dL_dout_color=None)),
                 ("sh_degree_4", put("a", sh_degree=4)), ("means3D_null", put("a", means3D=None))] + BACKWARD("a"),
    "backward_fused_loss": [("args_null", put("c", args_null=True)), ("loss_null", put("c", loss=None))] + LOSS("loss") + BACKWARD("a"),
    "backward_masked_loss": [("args_null", put("c", args_null=True)), ("masked_null", put("c", masked=None))] + MASKED("masked", "a")
                            + [c for c in BACKWARD("a") if not c[0].startswith("pose_only")],
    "blend_forward_batch": VIEW_LIST + [("sh_degree_4", put("b", sh_degree=4)), ("negative_num_rendered", put("b", num_rendered=-1))]
                           + ONE_FRAME("b") + RENDER_BUFFERS("b"),
    "blend_backward_window_batch": VIEW_LIST + [
        ("no_loss_lists", put("c", losses_null=True)), ("view_1_without_loss", lambda c: c.losses.__setitem__(1, None)),
        ("pose_only_differs", put("b", flags=POSE_ONLY)),
        ("width_differs", chain(roomy("b", image_width=W + 16), put("loss_b", width=W + 16, scratch_bytes=ROOMY))),
        ("height_differs", chain(roomy("b", image_height=H + 16), put("loss_b", height=H + 16, scratch_bytes=ROOMY))),
        ("row_begin_differs", put("b", tile_row_begin=1)), ("row_end_differs", put("b", tile_row_end=1))]
        + LOSS("loss_b") + [c for c in BACKWARD("b") if not c[0].startswith("pose_only")]
        + [("pose_only_view_dependent_colour", both(flags=POSE_ONLY, sh_degree=1, sh_coeffs=4)), ("pose_only_accumulate", both(flags=POSE_ONLY | ACCUMULATE))]
        + [("as_" + n, chain(lambda c: (setattr(c, "maskeds", [c.masked, c.masked_b]), setattr(c, "losses_null", True)), m))
           for n, m in MASKED("masked_b", "b")[:5] + [("masked_in_a_band", both(tile_row_begin=1, tile_row_end=2)), ("masked_pose_only", both(flags=POSE_ONLY))]],
    "gaussian_backward_batch": VIEW_LIST + [
        ("pose_only", put("b", flags=POSE_ONLY | ACCUMULATE)), ("N_differs", put("b", num_gaussians=N - 1)), ("means3D_differs", put("b", means3D=4096)),
        ("opacities_differs", put("b", opacities=4096)), ("scales_differs", put("b", scales=4096)), ("rotations_differs", put("b", rotations=4096)),
        ("shs_differs", put("b", shs=4096)), ("activations_differs", put("b", activations=1)), ("dL_dmeans3D_differs", put("b", dL_dmeans3D=4096)),
        ("dL_dopacities_differs", put("b", dL_dopacities=4096)), ("dL_dscales_differs", put("b", dL_dscales=4096)),
        ("dL_drotations_differs", put("b", dL_drotations=4096)), ("dL_dshs_differs", put("b", dL_dshs=4096)),
        ("colors_precomp", both(colors_precomp=4096)), ("cov3D_precomp", both(cov3D_precomp=4096)), ("sh_coeffs_4", both(sh_coeffs=4)),
        ("view_1_does_not_accumulate", put("b", flags=0))]
        # (less what the checks above refuse in other words: pose-only views, other colour / covariance forms, gradient buffers of its own)
        + [c for c in BACKWARD("b") if c[0] not in ("pose_only_view_dependent_colour", "pose_only_accumulate", "dL_dcov3D_null", "dL_dcolors_null",
                                                    "dL_dmeans3D_null", "dL_dopacities_null", "dL_dscales_null", "dL_drotations_null", "dL_dshs_null")],
}.items():
    for name, mutate in cases:
        assert (entry + "." + name) not in CASES, name
        CASES[entry + "." + name] = (entry, mutate)


def refusal(case):
    entry, mutate = CASES[case]
    call = Call(entry)
    mutate(call)
    return call.run()


def test_the_recording_covers_the_cases():
    golden = json.load(open(GOLDEN))
    assert set(golden) == set(CASES) and len(CASES) >= 60
    # a refusal is a verdict on the arguments: never a HIP error (the call got as far as the runtime), never OK
    assert all(g["status"] in (_lib.E_INVALID, _lib.E_RANGE) and g["error"] for g in golden.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal(case):
    # (with the one-launch leg switched off the call is lvdgs_forward, then lvdgs_backward_fused_loss: what only the backward refuses
    # would be rendered first -- with these pointers)
    if case.startswith("forward_backward_fused_loss.") and (os.environ.get("LVDGS_NO_FUSED_BLEND") or os.environ.get("LVDGS_FORCE_RADIX_GROUPING")):
        pytest.skip("the fused forward + backward leg is switched off in the environment")
    want = json.load(open(GOLDEN))[case]
    status, error = refusal(case)
    assert (status, error) == (want["status"], want["error"])


if __name__ == "__main__":
    out = {}
    for case in sorted(CASES):
        status, error = refusal(case)
        assert status in (_lib.E_INVALID, _lib.E_RANGE), (case, status, error)
        out[case] = {"status": status, "error": error}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(out), "refusals recorded from", _lib.LIB_PATH)
