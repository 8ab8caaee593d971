"""Dense Farneback optical flow and the motion mask of the masker's fallback branch, on the device (HIP, ``csrc/optical_flow.hip``;
semantics: ``include/lvdgs.h``).

When its detector returns no boxes the reference's masker falls back (utils/slam_frontend.py:887-904 -> ``_fallback_detection``,
:635-678): from frame 5 on a dense ``cv2.calcOpticalFlowFarneback`` between the stored grey frame and the current one on the host,
``magnitude > 3.0`` and a 7 x 7 dilation -- a download, tens of milliseconds of one core, an upload and a wait.  Here it is one
library call with a fixed number of launches and no host wait.  Parity with the real ``cv2`` (Farneback, the grey conversion, the
dilation) is UNPINNED -- OpenCV is not installed where this is built; the header's text is the definition.

``farneback``        the functional form: two grey byte planes on the GPU in, the flow out.
``farneback_torch``  the same text as PyTorch / NumPy statements on whatever device the planes live on (CPU tests, A/B runs).
``MotionFallback``   a callable for the ``fallback`` seat of ``DynamicMasker``: the reference's ``prev_frame`` and its fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

DEFAULTS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)     # the reference's call (flags=0)
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
MIN_SIZE = 32
EARLY_FRAMES = 5     # _fallback_detection: below this frame index the reference uses its colour / contour / Canny heuristic

_scratch = _lib.DeviceScratch()


def _params(params):
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"farneback: unknown parameters {sorted(unknown)} (known: {sorted(DEFAULTS)})")
    p = dict(DEFAULTS, **params)
    return _lib.FarnebackParams(pyr_scale=float(p["pyr_scale"]), levels=int(p["levels"]), winsize=int(p["winsize"]),
                                iterations=int(p["iterations"]), poly_n=int(p["poly_n"]), poly_sigma=float(p["poly_sigma"]))


def _grey_plane(t, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype is not torch.uint8 or t.dim() != 2:
        raise _lib.LvdgsError(f"farneback: {what} must be an (H, W) uint8 tensor on a GPU (there is no CPU path; farneback_torch is the PyTorch text)")
    return t.contiguous()


def farneback(prev_grey, next_grey, **params):
    """One ``lvdgs_farneback_flow`` call: (H, W) uint8 twice, on one GPU -> flow (H, W, 2) float32, [..., 0] along x, [..., 1] along y.
    ``params``: ``DEFAULTS``' names.  No host wait, no copy."""
    prev_grey, next_grey = _grey_plane(prev_grey, "prev_grey"), _grey_plane(next_grey, "next_grey")
    if prev_grey.shape != next_grey.shape or prev_grey.device != next_grey.device:
        raise _lib.LvdgsError("farneback: the two planes must have one size and one device")
    H, W = prev_grey.shape
    device = prev_grey.device
    L = _lib.lib()
    scratch = _scratch.get(device, L.lvdgs_farneback_scratch_bytes(W, H))
    flow = torch.empty((H, W, 2), dtype=torch.float32, device=device)
    a = _lib.FarnebackArgs(width=W, height=H, params=_params(params), prev=_lib.ptr(prev_grey), next=_lib.ptr(next_grey),
                           flow=_lib.ptr(flow), scratch=_lib.ptr(scratch), scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        _lib.check(L.lvdgs_farneback_flow(C.byref(a), _lib.raw_stream(device)), "lvdgs_farneback_flow")
    return flow


class MotionState:
    """The stored grey frame of ``lvdgs_motion_mask`` for one frame size: a zeroed block holds no frame."""

    def __init__(self, width, height, device="cuda"):
        self.width, self.height = int(width), int(height)
        nbytes = int(_lib.lib().lvdgs_motion_mask_state_bytes(self.width, self.height))
        if nbytes == 0:
            raise _lib.LvdgsError(f"motion mask: no state for a {width}x{height} frame (1..16384 each way)")
        self.block = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def reset(self):
        self.block.zero_()

    def stored(self):
        """The stored grey plane as an (H, W) uint8 NumPy array, or None (a device-to-host copy: for tests)."""
        raw = self.block.cpu().numpy()
        w, h, stored = (int(v) for v in raw[:12].view(np.int32))
        if (w, h, stored) != (self.width, self.height, 1):
            return None
        return raw[256:256 + w * h].reshape(h, w).copy()


def motion_mask(image, state, mode=None, *, motion_threshold=3.0, dilate_kernel=7, want_flow=False, **params):
    """One ``lvdgs_motion_mask`` call on ``image`` (3, H, W) float32 on the state's GPU.  ``mode``: ``_lib.MOTION_OBSERVE`` (-> None),
    ``_lib.MOTION_MASK`` (the default) or ``MOTION_MASK | MOTION_ADVANCE`` -> (mask (H, W) bool, info: 8 int32 on the device --
    ``_lib.MOTION_INFO`` names them --, flow (H, W, 2) or None).  No host wait, no copy."""
    mode = _lib.MOTION_MASK if mode is None else int(mode)
    device = state.block.device
    W, H = state.width, state.height
    if not _lib.is_f32(image, device) or tuple(image.shape) != (3, H, W):
        raise _lib.LvdgsError(f"motion mask: image must be a contiguous (3, {H}, {W}) float32 tensor on the state's GPU")
    L = _lib.lib()
    a = _lib.MotionMaskArgs(width=W, height=H, mode=mode, dilate_kernel=int(dilate_kernel), params=_params(params),
                            motion_threshold=float(motion_threshold), image=_lib.ptr(image), state=_lib.ptr(state.block),
                            state_bytes=state.block.numel())
    mask = info = flow = None
    if mode != _lib.MOTION_OBSERVE:
        scratch = _scratch.get(device, L.lvdgs_motion_mask_scratch_bytes(W, H))
        mask = torch.empty((H, W), dtype=torch.bool, device=device)
        info = torch.empty(_lib.MOTION_INFO_WORDS, dtype=torch.int32, device=device)
        flow = torch.empty((H, W, 2), dtype=torch.float32, device=device) if want_flow else None
        a.mask, a.info, a.flow, a.scratch, a.scratch_bytes = _lib.ptr(mask), _lib.ptr(info), _lib.ptr(flow), _lib.ptr(scratch), scratch.numel()
    with _lib.on_device(device):
        _lib.check(L.lvdgs_motion_mask(C.byref(a), _lib.raw_stream(device)), "lvdgs_motion_mask")
    return None if mode == _lib.MOTION_OBSERVE else (mask, info, flow)


# ------------------------------------------------------------------------------------------------------------------------------
# The same text as PyTorch statements (``MotionFallback(fused=False)``): one statement per sentence of the header.  What the header
# computes "on the host in double" is NumPy float64 here; sums run over their taps in ascending order, one product at a time.
# ------------------------------------------------------------------------------------------------------------------------------
def grey_torch(image):
    """(3, H, W) float32 -> (H, W) uint8: the reference's ``(img * 255).astype(np.uint8)`` and the integer grey."""
    q = (image.to(torch.float32) * 255.0).clamp(0.0, 255.0).to(torch.uint8).to(torch.int32)
    return ((4899 * q[0] + 9617 * q[1] + 1868 * q[2] + 8192) >> 14).to(torch.uint8)


def pyramid(W, H, pyr_scale, levels):
    """The levels, coarsest first: dicts of k, scale, w, h, sigma, ksize."""
    k, s = 0, 1.0
    while k < levels:
        s *= pyr_scale
        if W * s < MIN_SIZE or H * s < MIN_SIZE:
            break
        k += 1
    out = []
    for level in range(k, -1, -1):
        scale = 1.0
        for _ in range(level):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1.0) / 2.0
        out.append(dict(k=level, scale=scale, w=int(np.rint(W * scale)), h=int(np.rint(H * scale)), sigma=sigma,
                        ksize=max(int(np.rint(5.0 * sigma)) | 1, 3)))
    return out


def _blur_taps(sigma, ksize):
    if sigma == 0:
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ksize, dtype=np.float64) - ksize // 2
    w = np.exp(-x * x / (2.0 * sigma * sigma))
    return w / w.sum()


def _poly_taps(n, sigma):
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * sigma * sigma)).astype(np.float32).astype(np.float64)
    g = g / g.sum()
    gg = g[:, None] * g[None, :]
    X, Y = x[None, :], x[:, None]
    G = np.zeros((6, 6))
    G[0, 0] = gg.sum()
    G[1, 1] = (gg * X * X).sum()
    G[3, 3] = (gg * X ** 4).sum()
    G[5, 5] = (gg * X * X * Y * Y).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    inv = np.linalg.inv(G)
    return g, x * g, x * x * g, (inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5])


def _reflect101(i, n):
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    i = torch.remainder(i, p)
    return torch.where(i >= n, p - i, i)


def _replicate(i, n):
    return i.clamp(0, n - 1)


def _correlate(img, taps, axis, border):
    n, r = img.shape[axis], len(taps) // 2
    at = torch.arange(n, device=img.device)
    acc = torch.zeros_like(img)
    for j, t in enumerate(taps):
        acc = acc + float(t) * img.index_select(axis, border(at + (j - r), n))
    return acc


def _axis_taps(n_in, n_out, dtype, device):
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5
    i0 = np.floor(s)
    f = torch.from_numpy(s - i0).to(device=device, dtype=dtype)
    i0 = i0.astype(np.int64)
    return (torch.from_numpy(np.clip(i0, 0, n_in - 1)).to(device), torch.from_numpy(np.clip(i0 + 1, 0, n_in - 1)).to(device), f)


def _resize(img, w, h):
    y0, y1, fy = _axis_taps(img.shape[0], h, img.dtype, img.device)
    x0, x1, fx = _axis_taps(img.shape[1], w, img.dtype, img.device)
    fy, fx = fy[:, None], fx[None, :]
    top, bottom = img.index_select(0, y0), img.index_select(0, y1)
    a, b, c, d = top.index_select(1, x0), top.index_select(1, x1), bottom.index_select(1, x0), bottom.index_select(1, x1)
    return (a * (1.0 - fx) + b * fx) * (1.0 - fy) + (c * (1.0 - fx) + d * fx) * fy


def _level_image(grey, lv, dtype):
    taps = _blur_taps(lv["sigma"], lv["ksize"])
    img = _correlate(_correlate(grey.to(dtype), taps, 1, _reflect101), taps, 0, _reflect101)
    return _resize(img, lv["w"], lv["h"])


def _poly_exp(img, n, sigma):
    g, xg, xxg, (ig11, ig03, ig33, ig55) = _poly_taps(n, sigma)
    v0, v1, v2 = (_correlate(img, t, 0, _replicate) for t in (g, xg, xxg))
    b1, b2, b4 = (_correlate(v0, t, 1, _replicate) for t in (g, xg, xxg))
    b3, b5 = _correlate(v1, g, 1, _replicate), _correlate(v1, xg, 1, _replicate)
    b6 = _correlate(v2, g, 1, _replicate)
    return torch.stack([b3 * float(ig11), b2 * float(ig11), b1 * float(ig03) + b6 * float(ig33), b1 * float(ig03) + b4 * float(ig33),
                        b5 * float(ig55)], dim=2)


def _border_weight(n, dtype, device):
    c = torch.arange(n, device=device)
    wb = torch.tensor(BORDER + (1.0,), dtype=dtype, device=device)
    return wb[c.clamp(max=5)] * wb[(n - 1 - c).clamp(max=5)]


def _matrices(R0, R1, flow):
    h, w = flow.shape[:2]
    dtype, device = flow.dtype, flow.device
    x, y = torch.arange(w, device=device).to(dtype)[None, :], torch.arange(h, device=device).to(dtype)[:, None]
    dx, dy = flow[..., 0], flow[..., 1]
    fx, fy = x + dx, y + dy
    x1f, y1f = torch.floor(fx), torch.floor(fy)
    inside = (x1f >= 0) & (x1f < w - 1) & (y1f >= 0) & (y1f < h - 1)
    x1, y1 = torch.where(inside, x1f, torch.zeros_like(x1f)).long(), torch.where(inside, y1f, torch.zeros_like(y1f)).long()
    x2, y2 = (x1 + 1).clamp(max=w - 1), (y1 + 1).clamp(max=h - 1)
    fx, fy = (fx - x1f)[..., None], (fy - y1f)[..., None]
    a00, a01, a10, a11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
    r = a00 * R1[y1, x1] + a01 * R1[y1, x2] + a10 * R1[y2, x1] + a11 * R1[y2, x2]
    r4, r5, r6 = (R0[..., 2] + r[..., 2]) * 0.5, (R0[..., 3] + r[..., 3]) * 0.5, (R0[..., 4] + r[..., 4]) * 0.25
    r2 = (R0[..., 0] - r[..., 0]) * 0.5 + (r4 * dy + r6 * dx)
    r3 = (R0[..., 1] - r[..., 1]) * 0.5 + (r6 * dy + r5 * dx)
    zero = torch.zeros_like(r2)
    r2, r3 = torch.where(inside, r2, zero), torch.where(inside, r3, zero)
    r4, r5, r6 = torch.where(inside, r4, R0[..., 2]), torch.where(inside, r5, R0[..., 3]), torch.where(inside, r6, R0[..., 4] * 0.5)
    s = _border_weight(w, dtype, device)[None, :] * _border_weight(h, dtype, device)[:, None]
    r2, r3, r4, r5, r6 = r2 * s, r3 * s, r4 * s, r5 * s, r6 * s
    return torch.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], dim=2)


def _update(M, winsize):
    ones = np.ones(winsize)
    S = torch.stack([_correlate(_correlate(M[..., c], ones, 1, _replicate), ones, 0, _replicate) for c in range(5)], dim=2)
    S = S * (1.0 / (winsize * winsize))
    g11, g12, g22, h1, h2 = (S[..., c] for c in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return torch.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], dim=2)


def farneback_torch(prev_grey, next_grey, dtype=torch.float32, return_levels=False, **params):
    """``farneback`` as PyTorch statements on the planes' device: (H, W) uint8 twice -> flow (H, W, 2) of ``dtype``."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"farneback: unknown parameters {sorted(unknown)} (known: {sorted(DEFAULTS)})")
    p = dict(DEFAULTS, **params)
    H, W = prev_grey.shape
    levels = pyramid(W, H, p["pyr_scale"], p["levels"])
    flow = None
    for lv in levels:
        I0, I1 = _level_image(prev_grey, lv, dtype), _level_image(next_grey, lv, dtype)
        if flow is None:
            flow = torch.zeros((lv["h"], lv["w"], 2), dtype=dtype, device=prev_grey.device)
        else:
            flow = torch.stack([_resize(flow[..., c], lv["w"], lv["h"]) for c in range(2)], dim=2) * (1.0 / p["pyr_scale"])
        R0, R1 = _poly_exp(I0, p["poly_n"], p["poly_sigma"]), _poly_exp(I1, p["poly_n"], p["poly_sigma"])
        M = _matrices(R0, R1, flow)
        for i in range(p["iterations"]):
            flow = _update(M, p["winsize"])
            if i < p["iterations"] - 1:
                M = _matrices(R0, R1, flow)
    return (flow, len(levels)) if return_levels else flow


def motion_mask_torch(prev_grey, image, motion_threshold=3.0, dilate_kernel=7, **params):
    """The MASK statements in PyTorch: -> (mask (H, W) bool, moving (H, W) bool, flow, the image's grey plane)."""
    from .slam_sequence import expand_dynamic_mask
    grey = grey_torch(image)
    flow = farneback_torch(prev_grey, grey, **params)
    magnitude = torch.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1])
    moving = magnitude > float(np.float32(motion_threshold))
    return expand_dynamic_mask(moving, dilate_kernel), moving, flow, grey


class MotionFallback:
    """The reference masker's ``prev_frame`` and the motion branch of its ``_fallback_detection`` (utils/slam_frontend.py:651-672), as
    a callable for the ``fallback`` seat of ``DynamicMasker``: ``(image, frame_idx) -> (H, W) bool mask or None``.

    ``frame_idx is not None and frame_idx < 5``: ``early(image, frame_idx)`` when given, else None (the empty mask).  The reference's
    colour, contour and Canny heuristic for those frames (``_create_conservative_first_frame_mask``) stays OUT: it is a chain of OpenCV
    calls that cannot be stated without OpenCV; ``early`` is the seat for it.
    Otherwise: the motion mask between the stored frame and ``image`` -- flow magnitude above ``motion_threshold``, dilated by
    ``dilate_kernel`` --, or None when no frame is stored.
    ``observe(image)`` stores the frame.  ``DynamicMasker`` calls it where the reference sets ``prev_frame``: on a frame WITH boxes that
    is not a first frame (``_refine_with_motion``, :1109 and :1139) -- and only there: the reference's fallback branch never advances
    the stored frame, so consecutive fallback frames are all compared with the last frame that had boxes.
    ``advance_on_fallback=True`` is the opt-in alternative: a fallback frame from ``EARLY_FRAMES`` on becomes the stored frame itself.
    ``fused=True``: ``lvdgs_motion_mask`` (HIP; the frames must be on a GPU; no host wait).  ``fused=False``: ``motion_mask_torch`` on
    the image's device.  ``params``: ``DEFAULTS``' names."""

    def __init__(self, motion_threshold=3.0, dilate_kernel=7, early=None, advance_on_fallback=False, fused=True, **params):
        _params(params)
        if not (1 <= int(dilate_kernel) <= 15 and int(dilate_kernel) % 2):
            raise ValueError(f"dilate_kernel: odd, 1..15, not {dilate_kernel!r}")
        self.motion_threshold, self.dilate_kernel, self.early = float(motion_threshold), int(dilate_kernel), early
        self.advance_on_fallback, self.fused, self.params = bool(advance_on_fallback), bool(fused), dict(params)
        self.prev_frame = None          # fused=False: the stored grey plane
        self._state = None              # fused=True: the MotionState of the frames' size and device
        self._stored = False            # fused=True: a frame is stored (host knowledge: nothing is read back)
        self.last_info = None           # fused=True: the last mask call's info words, on the device

    def reset(self):
        self.prev_frame, self._stored = None, False
        if self._state is not None:
            self._state.reset()

    def _device_state(self, image):
        _, H, W = image.shape
        if not image.is_cuda:
            raise _lib.LvdgsError("MotionFallback(fused=True) needs the frames on a GPU (there is no CPU path; fused=False is the PyTorch text)")
        s = self._state
        if s is None or (s.width, s.height) != (W, H) or s.block.device != image.device:
            s, self._stored = MotionState(W, H, image.device), False
            self._state = s
        return s

    def observe(self, image):
        if self.fused:
            state = self._device_state(image)
            motion_mask(_lib.f32(image, image.device), state, _lib.MOTION_OBSERVE, **self.params)
            self._stored = True
        else:
            self.prev_frame = grey_torch(image)

    def __call__(self, image, frame_idx=None):
        if frame_idx is not None and frame_idx < EARLY_FRAMES:
            return None if self.early is None else self.early(image, frame_idx)
        if self.fused:
            state = self._device_state(image)
            if not self._stored:
                if self.advance_on_fallback:
                    self.observe(image)
                return None
            mode = _lib.MOTION_MASK | (_lib.MOTION_ADVANCE if self.advance_on_fallback else 0)
            mask, self.last_info, _ = motion_mask(_lib.f32(image, image.device), state, mode, motion_threshold=self.motion_threshold,
                                                  dilate_kernel=self.dilate_kernel, **self.params)
            return mask
        prev = self.prev_frame
        if prev is None or prev.shape != image.shape[1:] or prev.device != image.device:
            self.prev_frame = grey_torch(image) if self.advance_on_fallback else None
            return None
        mask, _, _, grey = motion_mask_torch(prev, image, self.motion_threshold, self.dilate_kernel, **self.params)
        if self.advance_on_fallback:
            self.prev_frame = grey
        return mask
