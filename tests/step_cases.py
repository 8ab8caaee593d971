"""Seeded inputs for the loss / Adam / isotropic / statistics tests, each with its conditions asserted in float64 on the way out (as
``map_edit_cases.assert_gaps`` does): a decision -- a threshold, the sign of a residual -- never depends on a float32 rounding, except on
the rows placed ON a threshold on purpose, where every side compares the same float32 numbers.
"""
import numpy as np

f32, f64 = np.float32, np.float64
GAP = 2.0 ** -18
RGB_THR = 0.01
DEPTH_MIN, OPAQUE_MIN = f32(0.01), f32(0.95)
up = lambda x: np.nextafter(f32(x), f32(np.inf))

# ------------------------------------------------------------------------------------------------ photometric loss
# W x H: P = 1, 3, 4, 5 (a lone lane, both paths); 1023, 1024, 1025 (the last lane of ONE workgroup, its 16-byte and scalar path, one
# pixel in a second workgroup); 258 workgroups on the 16-byte path (516 x 512) and on the scalar one (513 x 513): the smallest sizes at
# which a thread of the 256-thread finish kernels takes a second partial sum.
LOSS_SIZES = ((1, 1), (3, 1), (2, 2), (5, 1), (33, 31), (32, 32), (41, 25), (516, 512), (513, 513))
# what each configuration passes: the four the header names, then one optional pointer (group) absent at a time
_BASE = dict(weight_rgb=1.0, weight_depth=0.0, weight_by_opacity=0, depth_needs_opaque=0, opacity=True, depth=True, grad_mask=True,
             exposure=True, grad_loss=True, optional_outputs=True)
LOSS_CONFIGS = {
    "tracking_rgb": dict(_BASE, weight_by_opacity=1, depth=False),
    "tracking_rgbd": dict(_BASE, weight_rgb=0.9, weight_depth=0.1, weight_by_opacity=1, depth_needs_opaque=1),
    "mapping_rgb": dict(_BASE, depth=False, grad_mask=False, grad_loss=False),       # grad_loss NULL in value_and_grad: 1
    "mapping_rgbd": dict(_BASE, weight_rgb=0.95, weight_depth=0.05, grad_mask=False),
    "no_opacity": dict(_BASE, weight_rgb=0.95, weight_depth=0.05, opacity=False),
    "no_exposure": dict(_BASE, weight_rgb=0.9, weight_depth=0.1, weight_by_opacity=1, depth_needs_opaque=1, exposure=False),
    "no_grad_mask": dict(_BASE, weight_rgb=0.9, weight_depth=0.1, weight_by_opacity=1, depth_needs_opaque=1, grad_mask=False),
    "no_optional_outputs": dict(_BASE, weight_rgb=0.9, weight_depth=0.1, weight_by_opacity=1, depth_needs_opaque=1, optional_outputs=False),
}
PLACED = ("g_tie", "g_in", "z_tie", "z_in", "o_tie", "o_in", "i_eq_g", "mask0", "mask1", "mask2", "mask255")


def loss_condition(c):
    """Per channel and pixel: is |e^a I + b - G| >= GAP (|e^a I| + |b| + |G|)?  (float64)"""
    ea = np.exp(f64(c["exposure_a"])) if c["exposure_a"] is not None else 1.0
    eb = f64(c["exposure_b"]) if c["exposure_b"] is not None else 0.0
    I, G = c["image"].astype(f64), c["gt_image"].astype(f64)
    return np.abs(ea * I + eb - G) >= GAP * (np.abs(ea * I) + abs(eb) + np.abs(G))


def assert_loss_conditions(c):
    ok = loss_condition(c).all(0)
    exempt = np.zeros(ok.size, bool)
    if c["exposure_a"] is None:
        exempt[[p for name, p in c["placed"] if name == "i_eq_g"]] = True       # residual exactly zero on purpose
    assert (ok | exempt).all(), "a residual lies within 2^-18 of zero"
    G = c["gt_image"]
    s32 = (G[0] + G[1]) + G[2]
    assert s32.dtype == f32 and np.array_equal(s32 > f32(RGB_THR), G.astype(f64).sum(0) > f64(f32(RGB_THR))), "the float32 sum of G decides otherwise"
    for name, p in c["placed"]:
        if name == "g_tie":
            assert s32[p] == f32(RGB_THR) and G[0, p] == f32(RGB_THR)                # sums to the threshold exactly: out
        if name == "g_in":
            assert s32[p] == up(RGB_THR)
        if name == "i_eq_g":
            assert np.array_equal(c["image"][:, p], G[:, p]) and s32[p] > f32(RGB_THR)


def loss_case(W, H, config, seed=0):
    """-> dict of float32 / uint8 arrays (None where the configuration passes NULL), the scalars, and ``placed``: [(name, pixel)]."""
    cfg = LOSS_CONFIGS[config]
    P = W * H
    ci = list(LOSS_CONFIGS).index(config)
    rng = np.random.default_rng([seed, W, H, ci])
    I = rng.uniform(0.0, 1.0, (3, P)).astype(f32)
    G = rng.uniform(0.0, 1.0, (3, P)).astype(f32)
    dark = rng.random(P) < 0.1                                   # sums on both sides of the 0.01 threshold
    G[:, dark] = rng.uniform(0.0, 0.0066, (3, int(dark.sum()))).astype(f32)
    split = ((G[0] + G[1]) + G[2] > f32(RGB_THR)) != (G.astype(f64).sum(0) > f64(f32(RGB_THR)))      # a sum whose float32 rounding decides
    G[0, split] += f32(1e-4)
    D = rng.uniform(0.0, 10.0, P).astype(f32)
    Z = rng.uniform(0.0, 10.0, P).astype(f32)
    near = rng.random(P) < 0.1
    Z[near] = rng.uniform(0.0, 0.02, int(near.sum())).astype(f32)
    Z[rng.random(P) < 0.05] = 0.0
    O = rng.uniform(0.0, 1.0, P).astype(f32)
    opaque = rng.random(P) < 0.4
    O[opaque] = rng.uniform(0.9, 1.0, int(opaque.sum())).astype(f32)
    M = rng.choice(np.array([0, 0, 1, 1, 2, 255], np.uint8), P)
    c = dict(W=W, H=H, P=P, config=config, cfg=cfg, rgb_thr=RGB_THR,
             exposure_a=f32(0.13) if cfg["exposure"] else None, exposure_b=f32(-0.04) if cfg["exposure"] else None,
             grad_loss=f32(0.7) if cfg["grad_loss"] else None)
    # the placed rows: at the head of the image (rotated by the configuration, so that the 1- to 5-pixel images see all of them
    # between them) and, when there is room, once more at its end (the last workgroup, the scalar tail)
    placed = []
    order = PLACED[ci % len(PLACED):] + PLACED[:ci % len(PLACED)]
    slots = [(name, k) for k, name in enumerate(order) if k < P]
    if P >= 2 * len(PLACED):
        slots += [(name, P - 1 - k) for k, name in enumerate(order)]
    for name, p in slots:
        I[:, p], G[:, p], D[p], Z[p], O[p], M[p] = f32(0.5), f32(0.25), f32(3.0), f32(5.0), f32(0.99), 1    # a live pixel in every term
        if name in ("g_tie", "g_in"):
            G[:, p] = (f32(RGB_THR) if name == "g_tie" else up(RGB_THR), 0.0, 0.0)
        elif name in ("z_tie", "z_in"):
            Z[p] = DEPTH_MIN if name == "z_tie" else up(DEPTH_MIN)
        elif name in ("o_tie", "o_in"):
            O[p] = OPAQUE_MIN if name == "o_tie" else up(OPAQUE_MIN)
        elif name == "i_eq_g":
            I[:, p] = G[:, p] = (f32(0.3), f32(0.6), f32(0.9))
        else:
            M[p] = int(name[4:])
        placed.append((name, p))
    c.update(image=I, gt_image=G, depth=D if cfg["depth"] else None, gt_depth=Z if cfg["depth"] else None,
             opacity=O if cfg["opacity"] else None, grad_mask=M if cfg["grad_mask"] else None, placed=placed)
    keep = np.zeros(P, bool)
    keep[[p for _, p in placed]] = True
    for _ in range(8):                     # move a residual that sits on zero off it (never a placed row)
        bad = ~loss_condition(c) & ~keep[None]
        if not bad.any():
            break
        I[bad] += f32(0.01)
    assert_loss_conditions(c)
    return c


def loss_oracle_args(c):
    """The keyword arguments of step_oracle.photometric for a case."""
    cfg = c["cfg"]
    return dict(image=c["image"], gt_image=c["gt_image"], depth=c["depth"], gt_depth=c["gt_depth"], opacity=c["opacity"], grad_mask=c["grad_mask"],
                exposure_a=c["exposure_a"], exposure_b=c["exposure_b"], grad_loss=c["grad_loss"], rgb_thr=c["rgb_thr"],
                weight_rgb=cfg["weight_rgb"], weight_depth=cfg["weight_depth"], weight_by_opacity=cfg["weight_by_opacity"],
                depth_needs_opaque=cfg["depth_needs_opaque"])


# ------------------------------------------------------------------------------------------------ isotropic regulariser
ISO_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025, 70_001)       # 70 001: 274 workgroups, the finish kernel's strided loop
ISO_WEIGHT = 10.0


def iso_condition(raw):
    """Per row: all three scales bit-equal, or every |s_k - mean| >= GAP max s (float64)."""
    s = np.exp(raw.astype(f64))
    equal = (raw[:, 0] == raw[:, 1]) & (raw[:, 1] == raw[:, 2])
    d = np.abs(s - s.mean(1, keepdims=True))
    return equal | (d >= GAP * s.max(1, keepdims=True)).all(1)


def iso_case(n, seed=0):
    rng = np.random.default_rng([seed, n, 77])
    raw = rng.uniform(np.log(0.005), np.log(2.0), (n, 3)).astype(f32)
    kind = rng.integers(0, 10, n)
    raw[kind == 0] = raw[kind == 0][:, :1]                        # a tenth: three bit-equal scales
    two = kind == 1
    raw[two, 1] = raw[two, 0]                                     # a tenth: two equal
    for _ in range(8):
        bad = ~iso_condition(raw)
        if not bad.any():
            break
        raw[bad, 2] += f32(0.01)
    assert iso_condition(raw).all()
    if n >= 20:
        assert (kind == 0).any() and two.any()
    return dict(n=n, raw=raw, weight=ISO_WEIGHT, grad_in=rng.normal(0.0, 1e-3, (n, 3)).astype(f32))     # the term is ADDED to what is there


# ------------------------------------------------------------------------------------------------ Adam
ADAM_NUMELS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 10_007)
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-15
ADAM_GUARD, ADAM_GUARD_VALUE = 8, f32(-77.25)
ADAM_LISTS = tuple(f"single_{n}" for n in ADAM_NUMELS) + ("eight", "unaligned")


def adam_tensor(rng, numel, step, lr, offset=0):
    """One tensor's four buffers, each ``offset`` floats of lead, numel values and ADAM_GUARD guard elements."""
    sgn = lambda k: rng.choice(np.array([-1.0, 1.0]), k)
    g = (sgn(numel) * 10.0 ** rng.uniform(-12.0, 4.0, numel)).astype(f32)
    m = (g.astype(f64) * sgn(numel) * 10.0 ** rng.uniform(-1.0, 1.0, numel)).astype(f32)
    v = (g.astype(f64) ** 2 * 10.0 ** rng.uniform(-1.0, 1.0, numel)).astype(f32)
    kind = rng.integers(0, 10, numel)
    still = kind == 0                       # zero gradient, zero moments: the parameter must not move
    g[still], m[still], v[still] = 0.0, 0.0, 0.0
    first = kind == 1                       # a first step: moments still zero
    m[first], v[first] = 0.0, 0.0
    g[kind == 2] = 0.0                      # momentum alone
    p = rng.normal(0.0, 1.0, numel).astype(f32)
    assert ((g == 0) | ((np.abs(g) >= 1e-12) & (np.abs(g) <= 1e4))).all()

    def buf(a):
        b = np.full(offset + numel + ADAM_GUARD, ADAM_GUARD_VALUE, f32)
        b[offset:offset + numel] = a
        return b
    return dict(numel=numel, step=step, lr=lr, offset=offset, still=still, param=buf(p), grad=buf(g), exp_avg=buf(m), exp_avg_sq=buf(v))


def adam_list(name, seed=0):
    rng = np.random.default_rng([seed, ADAM_LISTS.index(name), 5])
    if name.startswith("single_"):
        return [adam_tensor(rng, int(name[7:]), 3, 1e-3)]
    if name == "unaligned":                  # four views one float into their buffers: data_ptr() % 16 == 4, numel % 4 == 0
        return [adam_tensor(rng, 1028, 7, 2.5e-3, offset=1)]
    numels = (70_001, 3, 1024, 0, 5, 1, 2049, 257)        # the longest first and an empty one in the middle
    steps = (1, 2, 1000, 5, 10 ** 6, 1, 2, 1000)
    lrs = (1.6e-4, 2.5e-3, 1.25e-4, 1.0, 0.05, 1e-3, 6e-3, 1e-5)
    return [adam_tensor(rng, n, s, lr) for n, s, lr in zip(numels, steps, lrs)]


# ------------------------------------------------------------------------------------------------ per-view statistics
STATS_SIZES = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2049)
STATS_VIEWS = 13                             # one more than a batched tail launch takes
UNREAD = f32(1e30)


def stats_case(n, views=STATS_VIEWS, seed=0):
    """``views`` render packages of one map of n Gaussians and the accumulators' starting values."""
    rng = np.random.default_rng([seed, n, views, 9])
    run = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 500, n)).astype(np.int32)
    c = dict(n=n, radii_max0=run.copy(), norm_sum0=np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.0, 1e-3, n)).astype(f32),
             vis_count0=rng.integers(0, 4, n).astype(f32), views=[])
    run = run.astype(np.int64)
    for _ in range(views):
        how = rng.integers(0, 5, n)          # invisible, below / equal to / above the running maximum, far above
        radii = np.select([how == 0, how == 1, how == 2, how == 3], [0, np.maximum(run - 1, 0), run, run + 1], rng.integers(1, 2 ** 24, n))
        radii = radii.astype(np.int32)
        assert (radii >= 0).all() and (radii < 2 ** 24).all()
        run = np.maximum(run, radii)
        grad = np.full((n, 3), UNREAD, f32)
        grad[:, :2] = (rng.choice(np.array([-1.0, 1.0]), (n, 2)) * 10.0 ** rng.uniform(-8.0, 0.0, (n, 2))).astype(f32)
        grad[rng.random(n) < 0.1, :2] = 0.0                       # visible or not, a gradient of exactly (0, 0)
        n_touched = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 1000, n)).astype(np.int32)
        c["views"].append(dict(radii=radii, n_touched=n_touched, grad=grad))
    if n >= 255:
        v0 = c["views"][0]
        assert ((v0["radii"] > 0) & (v0["grad"][:, :2] == 0).all(1)).any() and (v0["radii"] == 0).any()
    c.update(max_radii2D0=rng.uniform(0.0, 600.0, n).astype(f32), grad_accum0=rng.uniform(0.0, 1e-2, n).astype(f32),
             denom0=rng.integers(0, 50, n).astype(f32))
    return c
