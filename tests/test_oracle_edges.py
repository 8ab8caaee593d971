"""The float64 C oracle against the dense float64 autograd statement (tests/ref_torch.py) in the regimes where a splatting
backward has its special cases (tests/edge_scenes.py): the alpha cap, the EWA guard band (centred, off-centre and wide-angle
cameras), the near plane, the early stop at T < 1e-4, thin Gaussians seen edge-on, and scale_modifier != 1.

test_oracle_pinning.py is the only independent anchor of the oracle's analytic backward, and its scenes reach none of these;
the HIP backward follows the oracle's derivation line by line, so a derivation error shared by the two is caught here or
nowhere.  Same rules as there: integers exact, images to 1e-10, gradients to rtol 1e-7 (atol 1e-9 of the tensor's largest
entry).  Every case first asserts that its scene reaches its regime (edge_scenes.regime_counts against a floor)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import edge_scenes  # noqa: E402
import oracle as orc  # noqa: E402
import ref_torch  # noqa: E402
from lvdgs import synthetic  # noqa: E402

# toy sizes (ref_torch is dense: pixels x Gaussians); floors at about half of what each scene reaches
CASES = {
    "cap": dict(scene="cap", N=160, W=62, H=46, seed=1, floor=dict(capped_pairs=45)),
    "guard": dict(scene="guard", N=150, W=64, H=48, seed=2, floor=dict(clamped_x_neg=8, clamped_x_pos=8, clamped_y_neg=8,
                                                                        clamped_y_pos=8)),
    "guard_offcentre": dict(scene="guard", camera="offcentre", N=150, W=64, H=48, seed=3,
                            floor=dict(clamped_x_pos=20, clamped_y_neg=15, clamped_inside=20)),
    "guard_wide": dict(scene="guard", camera="wide", N=150, W=60, H=44, seed=4, floor=dict(clamped_x=25, clamped_y=25)),
    "near": dict(scene="near", N=150, W=64, H=48, seed=5, floor=dict(near=70)),
    "stop": dict(scene="stop", N=192, W=64, H=48, seed=6, floor=dict(stopped_pixels=1500)),
    "thin": dict(scene="thin", N=160, W=62, H=46, seed=7, floor=dict(lowpass=80)),
}


def scene(case, sh_degree=0):
    c = CASES[case]
    kw = {"camera": c["camera"]} if "camera" in c else {}
    if sh_degree:
        kw["sh_degree"] = sh_degree
    g, cam = edge_scenes.SCENES[c["scene"]](c["N"], c["W"], c["H"], seed=c["seed"], **kw)
    return {k: v.double() for k, v in g.items()}, cam, c["W"], c["H"]


def _cov6(g):
    R = ref_torch.quat_to_rot(g["rotations"])
    M = R @ torch.diag_embed(g["scales"])
    S = M @ M.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()


def _oracle(g, cam, W, H, bg, use_sh, sh_degree, cov, scale_modifier):
    o = orc.Oracle("f64")
    view, proj_raw = cam.world_view_transform.double(), cam.projection_matrix.double()
    kw = dict(scales=g["scales"].numpy(), rotations=g["rotations"].numpy()) if cov is None else dict(cov3D_precomp=cov.numpy())
    out = o.forward(means3D=g["means3D"].numpy(), opacities=g["opacities"].numpy(), W=W, H=H, tanfovx=cam.tanfovx,
                    tanfovy=cam.tanfovy, viewmatrix=view.numpy(), projmatrix=(view @ proj_raw).numpy(),
                    projmatrix_raw=proj_raw.numpy(), campos=torch.linalg.inv(view)[3, :3].numpy(), bg=bg.numpy(),
                    shs=g["shs"].numpy() if use_sh else None, colors_precomp=None if use_sh else g["colors"].numpy(),
                    sh_degree=sh_degree, scale_modifier=scale_modifier, **kw)
    return o, out


def pin(g, cam, W, H, grad_seed, use_sh=False, sh_degree=0, cov=None, scale_modifier=1.0):
    """Forward and backward of the float64 oracle against ref_torch on (g, cam); returns (oracle forward, oracle backward)."""
    bg = torch.tensor([0.3, 0.1, 0.7], dtype=torch.float64)
    tau = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    names = ["means3D", "opacities", "shs" if use_sh else "colors"] + (["scales", "rotations"] if cov is None else [])
    leaves = {k: g[k].clone().requires_grad_(k in names) for k in g}
    view, proj, campos = ref_torch.camera_matrices(cam.R.double(), cam.T.double(), tau, cam.projection_matrix.double())
    kw = dict(scales=leaves["scales"], rotations=leaves["rotations"])
    if cov is not None:
        cov_leaf = cov.clone().requires_grad_(True)
        kw = dict(cov3D_precomp=cov_leaf)
    ref = ref_torch.render_dense(leaves["means3D"], leaves["opacities"], H, W, cam.tanfovx, cam.tanfovy, bg, view, proj, campos,
                                 shs=leaves["shs"] if use_sh else None, colors_precomp=None if use_sh else leaves["colors"],
                                 sh_degree=sh_degree, scale_modifier=scale_modifier, **kw)
    gc, gd, go = (t.double() for t in synthetic.make_image_grads(W, H, grad_seed))
    ((ref["color"] * gc).sum() + (ref["depth"] * gd).sum() + (ref["opacity"] * go).sum()).backward()

    o, out = _oracle(g, cam, W, H, bg, use_sh, sh_degree, cov, scale_modifier)
    assert out["num_rendered"] > 0
    for k in ("radii", "tiles_touched", "n_touched", "n_contrib"):
        np.testing.assert_array_equal(out[k], ref[k].numpy(), err_msg=k)
    for k in ("color", "depth", "opacity"):
        np.testing.assert_allclose(out[k], ref[k].detach().numpy(), rtol=1e-10, atol=1e-12, err_msg=k)

    gr = o.backward(gc.numpy(), gd.numpy(), go.numpy())
    o.free()
    want = {n: leaves[n].grad for n in names}
    want["tau"] = tau.grad
    if cov is not None:
        want["cov3D"] = cov_leaf.grad
    for n, r in want.items():
        b = r.numpy().reshape(gr[n].shape)
        np.testing.assert_allclose(gr[n], b, rtol=1e-7, atol=1e-9 * np.abs(b).max(), err_msg=n)
    # viewspace gradient = d loss / d NDC xy
    pix = ref["means2D_pix"].grad.numpy()
    for a, size in ((0, W), (1, H)):
        np.testing.assert_allclose(gr["means2D"][:, a], pix[:, a] * 0.5 * size, rtol=1e-7,
                                   atol=1e-9 * np.abs(pix).max() * size, err_msg="means2D")
    assert np.all(gr["means2D"][:, 2] == 0)
    dead = out["radii"] == 0
    for n in ("means3D", "means2D", "opacities", "scales", "rotations"):
        assert not np.any(gr[n][dead]), f"culled Gaussians with a {n} gradient"
    return out, gr


def _premise(case, out, g, cam, floor=None):
    counts = edge_scenes.regime_counts(out, g, cam)
    for k, v in (floor or CASES[case]["floor"]).items():
        assert counts[k] >= v, f"{case}: {k} = {counts[k]} < {v} ({counts})"
    return counts


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_matches_autograd_in_the_regime(case):
    g, cam, W, H = scene(case)
    out, gr = pin(g, cam, W, H, grad_seed=list(CASES).index(case))
    _premise(case, out, g, cam)
    if case == "near":
        behind = slice(-4, None)      # edge_scenes.near_scene: the last four are just behind the near plane
        assert (out["radii"][behind] == 0).all()
        for n in ("means3D", "opacities", "scales", "rotations", "colors"):
            assert not np.any(gr[n][behind]), n


def test_guard_band_with_spherical_harmonics_degree_3():
    """The shs path through the guard band with the off-centre principal point: the view direction of a clamped Gaussian feeds
    the colour (and with it means3D and dL/dtau) while its clamped coordinate feeds nothing; scales and rotations compared too."""
    g, cam, W, H = scene("guard_offcentre", sh_degree=3)
    g["shs"][:, 0] -= 1.2   # some channels below zero: the clamp mask too
    out, _ = pin(g, cam, W, H, grad_seed=31, use_sh=True, sh_degree=3)
    _premise("guard_offcentre", out, g, cam)
    assert out["clamped"].any()


def test_precomputed_covariance_of_thin_gaussians():
    """dL/dcov3D where the 3-D covariance is near singular (one scale 1e-3 of the others) and the 2-D one is the low-pass term's
    across the line."""
    g, cam, W, H = scene("thin")
    out, _ = pin(g, cam, W, H, grad_seed=32, cov=_cov6(g))
    _premise("thin", out, g, cam)


# scale_modifier multiplies every scale before the covariance (and dL/dscales by itself once)
@pytest.mark.parametrize("case", ["guard_offcentre", "near", "thin"])
@pytest.mark.parametrize("scale_modifier", [0.6, 1.7])
def test_scale_modifier(case, scale_modifier):
    g, cam, W, H = scene(case)
    out, _ = pin(g, cam, W, H, grad_seed=33, scale_modifier=scale_modifier)
    _premise(case, out, g, cam, {k: v // 2 for k, v in CASES[case]["floor"].items()})
    o, plain = _oracle(g, cam, W, H, torch.zeros(3, dtype=torch.float64), False, 0, None, 1.0)
    o.free()
    assert (plain["radii"] != out["radii"]).mean() > 0.3      # (the modifier reached the footprints)
