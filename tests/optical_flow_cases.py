"""Scenes for the optical-flow tests: band-limited texture (a sum of 24 sinusoids of spatial frequency <= 0.35 rad/px), evaluated
at shifted coordinates -- so a shift is exact, whatever its fraction -- and quantised to bytes.

(a) ``whole_shift``: the second frame is the first one shifted by SHIFT_A.
(b) ``moving_rectangle``: the background shifted by SHIFT_BG; a centred rectangle, a third of the frame each way, of a second
    texture shifted by SHIFT_RECT.
A second frame that is the first one shifted by +d has flow +d: frame2(x) = frame1(x - d).
"""
import numpy as np

SIZES = ((64, 48), (130, 70), (261, 259), (9, 7))      # (W, H): one level | two | four, odd, both half-to-even roundings | tiny
SHIFT_A = (2.5, -1.25)
SHIFT_BG = (0.5, -0.25)
SHIFT_RECT = (5.0, 2.0)
WAVES, MAX_FREQ = 24, 0.35


def texture(seed):
    """-> f(x, y): float64 in about [0, 255], band-limited."""
    rng = np.random.default_rng(seed)
    freq = MAX_FREQ * np.sqrt(rng.uniform(0.05, 1.0, WAVES))
    angle = rng.uniform(0, 2 * np.pi, WAVES)
    kx, ky, phase = freq * np.cos(angle), freq * np.sin(angle), rng.uniform(0, 2 * np.pi, WAVES)
    amp = rng.uniform(0.5, 1.0, WAVES)
    amp = amp / amp.sum()

    def f(x, y):
        v = sum(a * np.sin(kx_ * x + ky_ * y + p) for a, kx_, ky_, p in zip(amp, kx, ky, phase))
        return 127.5 + 127.5 * 2.2 * v
    return f


def to_bytes(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def grid(W, H):
    return np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))


def whole_shift(W, H, shift=SHIFT_A, seed=11):
    """-> (frame1, frame2) uint8 (H, W)."""
    f = texture(seed)
    x, y = grid(W, H)
    return to_bytes(f(x, y)), to_bytes(f(x - shift[0], y - shift[1]))


def rectangle_of(W, H):
    """(x0, y0, x1, y1), exclusive ends: the centred third."""
    return W // 3, H // 3, W - W // 3, H - H // 3


def moving_rectangle(W, H, seed=23):
    """-> (frame1, frame2, inside): ``inside`` marks the rectangle's pixels in frame 1 that are still inside it in frame 2."""
    bg, fg = texture(seed), texture(seed + 1)
    x, y = grid(W, H)
    x0, y0, x1, y1 = rectangle_of(W, H)

    def frame(bg_shift, fg_shift):
        inside = (x - fg_shift[0] >= x0) & (x - fg_shift[0] < x1) & (y - fg_shift[1] >= y0) & (y - fg_shift[1] < y1)
        return np.where(inside, fg(x - fg_shift[0], y - fg_shift[1]), bg(x - bg_shift[0], y - bg_shift[1])), inside

    f1, in1 = frame((0.0, 0.0), (0.0, 0.0))
    f2, in2 = frame(SHIFT_BG, SHIFT_RECT)
    return to_bytes(f1), to_bytes(f2), in1 & in2


def as_image(grey):
    """A (3, H, W) float32 image whose grey plane (``optical_flow_oracle.grey_of``) is ``grey``: three equal channels at (g + 0.5) / 255."""
    c = ((grey.astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    return np.stack([c, c, c])


def golden():
    """tests/golden/motion_fallback.npz (made by tests/golden/make_motion_fallback_golden.py from the reference's own code) ->
    (W, H, conservative rectangle, sequences): per sequence a list of frames, each a dict of the scripted inputs (``frame_idx``,
    ``has_boxes``, ``image`` (H, W, 3) uint8, ``boxes``, ``labels``) and what the reference's call gave (``kind``: boxes | early |
    motion | none; ``stored``: the call replaced ``prev_frame``; ``dynamic`` (H, W) uint8)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_fallback.npz"))
    W, H = (int(v) for v in z["size"])
    seqs = []
    for s in range(int(z["sequences"])):
        frames = []
        for f, idx in enumerate(z[f"s{s}_frame_idx"]):
            frames.append(dict(frame_idx=int(idx), has_boxes=bool(z[f"s{s}_has_boxes"][f]), stored=bool(z[f"s{s}_stored"][f]),
                               kind=str(z[f"s{s}_kind"][f]), image=z[f"s{s}_images"][f], boxes=z[f"s{s}_f{f}_boxes"],
                               labels=[str(v) for v in z[f"s{s}_f{f}_labels"]],
                               dynamic=np.unpackbits(z[f"s{s}_f{f}_dynamic"])[:H * W].reshape(H, W)))
        seqs.append(frames)
    return W, H, tuple(int(v) for v in z["conservative"]), seqs


def image_of(rgb):
    """(H, W, 3) uint8 -> the (3, H, W) float32 frame that quantises back to it: (q + 0.5) / 255."""
    return np.ascontiguousarray(((rgb.astype(np.float64) + 0.5) / 255.0).astype(np.float32).transpose(2, 0, 1))
