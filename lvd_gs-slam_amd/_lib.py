"""ctypes binding of ``lib/liblvdgs.so`` (C ABI: ``include/lvdgs.h``).

The library is the only compute path: if it is missing or fails to load, importing a symbol
from here raises -- there is no CPU or PyTorch fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

from ._abi import *  # noqa: F401,F403  (include/lvdgs.h as data: the structs, the constants, PROTOTYPES)

_HERE = os.path.dirname(os.path.abspath(__file__))
# LVDGS_LIB: another build of the library (same-box A/B of compile-time variants: `make OUT=../lib_b EXTRA=-D...`)
LIB_PATH = os.environ.get("LVDGS_LIB") or os.path.join(_HERE, "lib", "liblvdgs.so")

# every symbol include/lvdgs.h declares (checked by tests/test_abi.py)
EXPORTS = tuple(PROTOTYPES)  # noqa: F405

_lib = None


class LvdgsError(RuntimeError):
    pass


def lib():
    """The loaded library (loads on first use; raises if the HIP build is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LvdgsError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C lvd_gs-slam_amd/csrc`). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():  # noqa: F405
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def ptr(t):
    """A tensor's data as a pointer field of an argument block (None: NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def is_f32(t, device=None):
    """Is ``t`` a contiguous float32 tensor on ``device`` (None: on any GPU)?"""
    return (torch.is_tensor(t) and (t.is_cuda if device is None else t.device == device) and t.dtype is torch.float32
            and t.is_contiguous())


def f32(t, device):
    """``t`` detached, as a contiguous float32 tensor on ``device`` (itself when it is one: no conversion kernel, no dispatcher
    round trip through ``.to()``)."""
    t = t.detach()
    return t if is_f32(t, device) else t.to(device=device, dtype=torch.float32).contiguous()


def device_bytes(n, device):
    """A byte buffer of at least ``n`` bytes (and at least 256) on ``device``."""
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=device)


def raw_stream(device):
    """hipStream_t of PyTorch's current stream ON `device` (the tensor's device, which need not be the current one),
    as a c_void_p.  A direct C call: torch.cuda.current_stream() costs tens of microseconds of Python per call."""
    idx = device.index if (device is not None and device.index is not None) else torch.cuda.current_device()
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


class on_device:
    """Make `device` the current HIP device for the duration of a library call when it is not already (kernels are
    launched on the current device; a stream of another device would be rejected)."""
    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index

    def __enter__(self):
        self.prev = None
        if self.idx is not None:
            cur = torch.cuda.current_device()
            if cur != self.idx:
                self.prev = cur
                torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


class DeviceScratch:
    """A library call's scratch, one buffer per device: kept while large enough, replaced by a larger one on demand
    (``device_bytes``).  ``zeroed``: a new buffer is zero-filled once; ``headroom``: a new buffer gets half as much again."""

    def __init__(self, *, zeroed=False, headroom=False):
        self.zeroed, self.headroom, self.buffers = zeroed, headroom, {}

    def get(self, device, nbytes):
        nbytes = int(nbytes)
        buf = self.buffers.get(device.index)
        if buf is None or buf.numel() < nbytes:
            buf = self.buffers[device.index] = device_bytes(nbytes + (nbytes // 2 if self.headroom else 0), device)
            if self.zeroed:
                buf.zero_()
        return buf


def next_seq(seq):
    """The sequence number that follows ``seq``: 1 .. 0x7FFFFFFF round and round, never 0 -- what a cleared tag word holds."""
    return (int(seq) % 0x7FFFFFFF) + 1


def host_block_verdict(words, name, tag, seq=None, statuses=()):
    """The tag word of a host block after the call's one wait: returned when it is the call's sequence number or one of the statuses
    the call can end in; anything else -- the cleared word above all -- means the call wrote no state."""
    found = int(words[tag])
    if (seq is not None and found == seq) or found in statuses:
        return found
    expected = f"sequence number {seq}" if seq is not None else "status " + " or ".join(str(s) for s in statuses)
    raise LvdgsError(f"{name} left no state (word [{tag}] of its host block holds {found}, expected {expected})")


class HostCall:
    """One entry point of the library that reports through a block of pinned host memory (include/lvdgs.h, "Host blocks"): its
    per-device block, scratch and sequence counter, and the call with its one wait.

    ``name``: the library function.  ``statuses``: what its tag word -- ``[tag]`` of the block -- may hold after the call; None: the
    call is tagged with the ``seq`` of its argument block, which ``run`` fills in.  ``tag=None``: no tag (``lvdgs_depth_align``,
    whose block is a state that its resume call reads: ``run`` neither clears nor judges it)."""

    def __init__(self, name, *, statuses=None, tag=0, zeroed=False, headroom=False):
        self.name, self.statuses, self.tag, self.headroom = name, statuses, tag, headroom
        self.scratch = DeviceScratch(zeroed=zeroed, headroom=headroom)
        self.blocks, self.words, self.seq = {}, {}, {}      # device index -> pinned block; -> its int32 words; -> last sequence number
        self.fn = None

    def resources(self, device, block_bytes, scratch_bytes=None):
        """(the device's pinned block of at least ``block_bytes`` bytes -- the one of the call before while large enough --, its scratch
        of at least ``scratch_bytes``; None: the call takes no scratch)."""
        block_bytes = int(block_bytes)
        block = self.blocks.get(device.index)
        if block is None or block.numel() < block_bytes:
            block = self.blocks[device.index] = torch.zeros(block_bytes + (block_bytes // 2 if self.headroom else 0), dtype=torch.uint8).pin_memory()
            self.words[device.index] = block.numpy().view(np.int32)
        return block, None if scratch_bytes is None else self.scratch.get(device, scratch_bytes)

    def wait(self, device):
        """The one wait of the call: until everything enqueued on the device's current stream has run."""
        torch.cuda.current_stream(device).synchronize()

    def run(self, device, args, fn=None):
        """``fn(byref(args), stream)`` (default: the library function) on ``device``, whose block ``args.host_state`` is, and the
        wait -> the block as int32 words (a view: copy what is to outlive the next call)."""
        words = self.words[device.index]
        if fn is None:
            fn = self.fn = self.fn or getattr(lib(), self.name)
        seq = None
        if self.tag is not None:
            words[self.tag] = 0      # whatever the call before left: only this call's own tag counts
            if self.statuses is None:
                seq = args.seq = self.seq[device.index] = next_seq(self.seq.get(device.index, 0))
        with on_device(device):
            check(fn(C.byref(args), raw_stream(device)), self.name)
            self.wait(device)
        if self.tag is not None:
            host_block_verdict(words, self.name, self.tag, seq, self.statuses or ())
        return words


_gc_policy = None      # "scoped" | "process" | "off"; None: not decided yet (LVDGS_GC_FREEZE / set_gc_policy / first loop entry)
_gc_depth = 0


def set_gc_policy(policy):
    """How the product's loops keep CPython's full-heap garbage collections out of their iterations.

    The loops run at 0.2-2 ms per iteration and allocate a few hundred small Python objects in each, which makes CPython start a
    FULL collection every few dozen to few hundred iterations; with the whole heap of an application that has PyTorch imported
    (about a million objects) in the oldest generation that is one stall of 40-110 ms (measured: ``tools/side_stall_diag.py``) --
    20-60 iterations' worth of time.

    * ``"scoped"`` (the default): ``gc.freeze()`` when the outermost product loop is entered (``track_frame``, ``map_window``,
      ``initialize_map``, ``color_refinement``, ``slam_sequence``) -- everything alive moves to the permanent generation, two list
      splices, no collection -- and ``gc.unfreeze()`` when it returns: inside the loop the collector walks only what the loop itself
      allocated, and afterwards the host application's collector sees its heap exactly as before (``gc.get_freeze_count() == 0``).
      An application that calls ``gc.freeze()`` ITSELF should pick one of the other two: the scoped exit would thaw its objects too
      (a freeze found in place at the first loop entry of the process switches the policy to "off" by itself).
    * ``"process"`` (``LVDGS_GC_FREEZE=1``, what every round up to 5 did unasked): one ``gc.collect(); gc.freeze()`` at the first loop
      entry, for the life of the process.  Cyclic garbage among the objects alive at that moment is never reclaimed.
    * ``"off"`` (``LVDGS_GC_FREEZE=0``): the collector is left alone.
    """
    global _gc_policy
    if policy not in ("scoped", "process", "off"):
        raise ValueError("gc policy: 'scoped', 'process' or 'off'")
    if policy == "process" and _gc_policy != "process":
        import gc
        gc.collect()
        gc.freeze()
    _gc_policy = policy


class quiet_gc:
    """Context manager around a product loop: see ``set_gc_policy``.  Re-entrant (only the outermost scope acts)."""
    __slots__ = ("acted",)

    def __enter__(self):
        global _gc_policy, _gc_depth
        import gc
        self.acted = False
        if _gc_policy is None:
            env = os.environ.get("LVDGS_GC_FREEZE", "scoped")
            _gc_policy = {"0": "off", "1": "process"}.get(env, "scoped")
            if _gc_policy == "scoped" and gc.get_freeze_count() > 0:   # (walks the permanent generation: asked once per process)
                _gc_policy = "off"   # the host application manages a freeze of its own: hands off
            if _gc_policy == "process":
                gc.collect()
                gc.freeze()
        _gc_depth += 1
        if _gc_policy == "scoped" and _gc_depth == 1:
            gc.freeze()
            self.acted = True
        return self

    def __exit__(self, *exc):
        global _gc_depth
        _gc_depth -= 1
        if self.acted:
            import gc
            gc.unfreeze()
        return False


def check(status, what):
    if status != OK:
        raise LvdgsError(f"{what} failed ({status}): {lib().lvdgs_last_error().decode()}")


def profile_enable(on=True):
    lib().lvdgs_profile_enable(1 if on else 0)


def profile_reset():
    lib().lvdgs_profile_reset()


def profile_read():
    """{kernel name: (launches, total_ms)} measured with HIP events on the launch stream."""
    buf = (KernelTime * 64)()
    n = lib().lvdgs_profile_read(buf, 64)
    return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(n)}
