"""The probe library (tests/probe/primitives_probe.hip, built as liblvdgs_probe.so beside the product library) and plain NumPy references
for the primitives of csrc/device_utils.hpp, spans.hpp and select.hpp.  Used by tests/test_primitives_probe.py (no GPU) and
tests/test_gpu_primitives.py.

The references do not go through the headers' code: integers are cumsum / sum / max in Python or uint64 arithmetic, reduced modulo the
type; float reductions are emulated in the ORDER the headers' comments state, one float32 addition per statement; the select's answer
comes from a sort."""
import ctypes as C
import os

import numpy as np

from lvdgs import _lib

PROBE_PATH = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), "liblvdgs_probe.so")
E_INVALID = 1
QUIET_NAN = 0x7FC00000

# enum WaveOp of the probe, in its order
WAVE_OPS = ("sum_i32", "sum_u32", "sum_u64", "sum_f32", "sum_f64", "sum_lane63", "max_i32", "max_u32", "max_f32", "min_f32", "scan_u32", "scan_i32",
            "scan_dpp", "fold32", "fold16", "rot1", "rot4", "rot8", "rot15", "dpp_shr1", "dpp_shr8", "row_sums3", "write_lane")
# op -> (planes in, dtype in, planes out, dtype out)
WAVE_SHAPES = {name: (1, np.float32, 1, np.float32) for name in WAVE_OPS}
WAVE_SHAPES.update(sum_i32=(1, np.int32, 1, np.int32), sum_u32=(1, np.uint32, 1, np.uint32), sum_u64=(1, np.uint64, 1, np.uint64),
                   sum_f64=(1, np.float64, 1, np.float64), max_i32=(1, np.int32, 1, np.int32), max_u32=(1, np.uint32, 1, np.uint32),
                   scan_u32=(1, np.uint32, 1, np.uint32), scan_i32=(1, np.int32, 1, np.int32), scan_dpp=(1, np.uint32, 1, np.uint32),
                   fold32=(2, np.float32, 1, np.float32), fold16=(2, np.float32, 1, np.float32), row_sums3=(3, np.float32, 6, np.float32),
                   write_lane=(1, np.int32, 1, np.int32))
SCAN_DTYPES = {np.dtype(np.uint32): 0, np.dtype(np.int32): 1, np.dtype(np.uint64): 2}
# scan_span_counts forms of the probe: (THREADS, T, C)
SPAN_COUNT_FORMS = [(256, np.uint32, np.uint32), (256, np.uint32, np.uint64), (256, np.uint64, np.uint64), (1024, np.uint32, np.uint64)]

_vp, _sz, _i, _i64, _u32, _u64, _f64 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
_PROTOTYPES = {
    "lvdgs_probe_span_length": (_u32, [_u32, _u32, _u32]),
    "lvdgs_probe_make_spans": (None, [_i64, _i, _i, _u32, C.POINTER(_i), C.POINTER(_u32)]),
    "lvdgs_probe_select_key": (_u32, [_u32]),
    "lvdgs_probe_select_unkey": (_u32, [_u32]),
    "lvdgs_probe_select_keys": (_i, [_vp, _vp, _vp, _i64]),
    "lvdgs_probe_lower_median_rank": (_u32, [_u32]),
    "lvdgs_probe_select_rank_of": (_u32, [_i64, _f64, _u32]),
    "lvdgs_probe_select_blocks": (_i, [_i64]),
    "lvdgs_probe_select_state_bytes": (_sz, []),
    "lvdgs_probe_select_report_words": (_i, []),
    "lvdgs_probe_wave": (_i, [_i, _i, _i, _vp, _sz, _vp, _sz, _i, _i, _vp]),
    "lvdgs_probe_mask_bit": (_i, [_i, _u64, _i, _vp, _sz, _vp]),
    "lvdgs_probe_scan": (_i, [_i, _i, _i, _i, _vp, _sz, _vp, _sz, _i, _vp]),
    "lvdgs_probe_block_sum": (_i, [_i, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "lvdgs_probe_span_range": (_i, [_u32, _u32, _i, _vp, _sz, _vp]),
    "lvdgs_probe_span_counts": (_i, [_i, _vp, _sz, _vp, _sz, _i, _i, _vp, _sz, _vp]),
    "lvdgs_probe_compact": (_i, [_i, _vp, _sz, _i64, _i, _u64, _vp, _sz, _vp, _vp, _i64, _sz, _sz, _vp, _vp]),
    "lvdgs_probe_select": (_i, [_vp, _sz, _vp, _sz, _i64, _i, _i64, _f64, _vp, _sz, _vp, _sz, _i, _vp]),
    "lvdgs_probe_select_segment": (_i, [_vp, _vp, _i, _i, _sz, _sz, _vp, _sz, _vp]),
    "lvdgs_probe_hist_add": (_i, [_vp, _vp, _sz, _vp, _sz, _vp]),
}
_probe = None


def probe():
    """The loaded probe library (the product library first: the probe takes its error plumbing from it)."""
    global _probe
    if _probe is None:
        _lib.lib()
        if not os.path.exists(PROBE_PATH):
            raise _lib.LvdgsError(f"{PROBE_PATH} not found: `make -C lvd_gs-slam_amd/csrc` builds it beside the product library")
        L = C.CDLL(PROBE_PATH)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _probe = L
    return _probe


def last_error():
    return _lib.lib().lvdgs_last_error().decode()


# ---------------------------------------------------------------- host functions
def make_spans(n, threads, cap, min_span):
    blocks, span = C.c_int(-1), C.c_uint32(0)
    probe().lvdgs_probe_make_spans(n, threads, cap, min_span, C.byref(blocks), C.byref(span))
    return blocks.value, span.value


def select_keys(bits):
    """(select_key(bits), select_unkey(select_key(bits))) of a uint32 array."""
    bits = np.ascontiguousarray(bits, np.uint32)
    keys, back = np.empty_like(bits), np.empty_like(bits)
    status = probe().lvdgs_probe_select_keys(bits.ctypes.data, keys.ctypes.data, back.ctypes.data, bits.size)
    assert status == 0, last_error()
    return keys, back


# ---------------------------------------------------------------- device probes (torch tensors on the GPU in, NumPy out)
def _gpu(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:      # (torch has no arithmetic on the unsigned types, but it need not: the bytes travel)
        return torch.from_numpy(a.view(np.int32)).cuda()
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda()
    return torch.from_numpy(a).cuda()


to_gpu = _gpu


def _empty(count, dtype, fill=None):
    import torch
    nbytes = max(int(count) * np.dtype(dtype).itemsize, 8)
    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    t.fill_(0 if fill is None else fill)
    return t


def _host(t, dtype, count):
    return t.cpu().numpy().view(dtype)[:count].copy()


def _stream(t):
    return _lib.raw_stream(t.device)


def _ok(status, what):
    if status != 0:
        raise _lib.LvdgsError(f"{what} failed ({status}): {last_error()}")


def run_wave(op, threads, planes, a0=0, a1=0):
    """Op `op` over `planes` ((in planes, n) or (n,), n a multiple of `threads`) -> (out planes, n)."""
    p_in, d_in, p_out, d_out = WAVE_SHAPES[op]
    x = np.ascontiguousarray(planes, d_in).reshape(p_in, -1)
    n = x.shape[1]
    assert n % threads == 0
    src, dst = _gpu(x), _empty(p_out * n, d_out, 0xAB)
    _ok(probe().lvdgs_probe_wave(WAVE_OPS.index(op), threads, n // threads, src.data_ptr(), x.nbytes, dst.data_ptr(), dst.numel(), a0, a1, _stream(src)),
        "lvdgs_probe_wave " + op)
    return _host(dst, d_out, p_out * n).reshape(p_out, n)


def run_mask_bit(set_bit, mask, bit):
    dst = _empty(64, np.uint64, 0xAB)
    _ok(probe().lvdgs_probe_mask_bit(int(set_bit), int(mask), bit, dst.data_ptr(), dst.numel(), _stream(dst)), "lvdgs_probe_mask_bit")
    return _host(dst, np.uint64, 64)


def run_scan(threads, values):
    """scan_workgroup<threads, values.dtype> of (n,) values -> (exclusive, total), each (n,)."""
    x = np.ascontiguousarray(values)
    n = x.size
    src, dst = _gpu(x), _empty(2 * n, x.dtype, 0xAB)
    _ok(probe().lvdgs_probe_scan(0, SCAN_DTYPES[x.dtype], threads, n // threads, src.data_ptr(), x.nbytes, dst.data_ptr(), dst.numel(), 0, _stream(src)),
        "lvdgs_probe_scan")
    out = _host(dst, x.dtype, 2 * n).reshape(2, n)
    return out[0], out[1]


def run_scan_contract(threads, planes, trips):
    """The contract probe: planes (3 + trips, n) -> (5 + 2 trips, n) (the layout: primitives_probe.hip, scan_contract_kernel)."""
    x = np.ascontiguousarray(planes)
    n = x.shape[1]
    assert x.shape[0] == 3 + trips
    src, dst = _gpu(x), _empty((5 + 2 * trips) * n, x.dtype, 0xAB)
    _ok(probe().lvdgs_probe_scan(1, SCAN_DTYPES[x.dtype], threads, n // threads, src.data_ptr(), x.nbytes, dst.data_ptr(), dst.numel(), trips, _stream(src)),
        "lvdgs_probe_scan (contract)")
    return _host(dst, x.dtype, (5 + 2 * trips) * n).reshape(5 + 2 * trips, n)


def run_block_sum(waves, planes):
    """block_sum<waves> twice on one s: planes (2, n) float32 or int32 -> (2, n)."""
    x = np.ascontiguousarray(planes)
    n = x.shape[1]
    src, dst = _gpu(x), _empty(2 * n, x.dtype, 0xAB)
    _ok(probe().lvdgs_probe_block_sum(int(x.dtype == np.int32), waves, n // (64 * waves), src.data_ptr(), x.nbytes, dst.data_ptr(), dst.numel(), _stream(src)),
        "lvdgs_probe_block_sum")
    return _host(dst, x.dtype, 2 * n).reshape(2, n)


def run_span_range(n, span, blocks):
    dst = _empty(2 * blocks, np.uint32, 0xAB)
    _ok(probe().lvdgs_probe_span_range(n, span, blocks, dst.data_ptr(), dst.numel(), _stream(dst)), "lvdgs_probe_span_range")
    return _host(dst, np.uint32, 2 * blocks).reshape(blocks, 2)


def run_span_counts(form, counts, stride, in_place, before_fill=None):
    """scan_span_counts form `form` over the strided array `counts` ((blocks * stride,) of T, given whole: sentinels included; out of place `before_fill` is
    what the output array holds beforehand) -> (before array of C, whole; the total every thread got back, (THREADS,))."""
    threads, T, Cc = SPAN_COUNT_FORMS[form]
    x = np.ascontiguousarray(counts, T)
    blocks = x.size // stride
    src = _gpu(x) if x.size else _empty(1, T)
    if in_place:
        dst = src
    else:
        dst = _gpu(np.ascontiguousarray(before_fill, Cc)) if x.size else _empty(1, Cc)
    tot = _empty(threads, Cc, 0xAB)
    _ok(probe().lvdgs_probe_span_counts(form, src.data_ptr(), x.size * np.dtype(T).itemsize, dst.data_ptr(), x.size * np.dtype(Cc).itemsize, blocks, stride,
                                        tot.data_ptr(), tot.numel(), _stream(tot)), "lvdgs_probe_span_counts")
    return _host(dst, Cc, x.size), _host(tot, Cc, threads)


def run_compact(form, keep, blocks, row0=0):
    """The TileWalk compaction of flatnonzero(keep) by `blocks` workgroups -> (indices, rows, total); the outputs hold one word per element + 1, filled with
    0xAB bytes where nothing was stored."""
    keep = np.ascontiguousarray(keep, np.uint8)
    n = keep.size
    cap = n + 1
    src = _gpu(keep) if n else _empty(1, np.uint8)
    scratch, idx, rows, total = _empty(2 * blocks, np.uint64), _empty(cap, np.uint32, 0xAB), _empty(cap, np.uint64, 0xAB), _empty(1, np.uint64, 0xAB)
    _ok(probe().lvdgs_probe_compact(form, src.data_ptr(), src.numel(), n, blocks, row0, scratch.data_ptr(), scratch.numel(), idx.data_ptr(), rows.data_ptr(), cap, idx.numel(),
                                    rows.numel(), total.data_ptr(), _stream(src)), "lvdgs_probe_compact")
    return _host(idx, np.uint32, cap), _host(rows, np.uint64, cap), int(_host(total, np.uint64, 1)[0])


class Select:
    """One select state on the device, reused from call to call the way the product's callers reuse theirs."""

    def __init__(self):
        self.state = _empty(probe().lvdgs_probe_select_state_bytes(), np.uint8, 0xAB)      # (garbage: the probe clears it on the stream)
        self.words = probe().lvdgs_probe_select_report_words()
        self.report = _empty(self.words, np.uint32)

    def __call__(self, v, take, n, fixed=-1, fraction=0.0, keys=False, per_pass=False):
        """-> dict(bits, n, ticket, k, after=[ticket behind pass 0..3], only with per_pass).  v, take: device tensors (take None: all)."""
        _ok(probe().lvdgs_probe_select(None if v is None else v.data_ptr(), 0 if v is None else v.numel(), None if take is None else take.data_ptr(),
                                       0 if take is None else take.numel(), n, int(keys), fixed, fraction,
                                       self.state.data_ptr(), self.state.numel(), self.report.data_ptr(), self.report.numel(), int(per_pass),
                                       _stream(self.state)), "lvdgs_probe_select")
        w = _host(self.report, np.uint32, self.words)
        return dict(bits=int(w[0]), n=int(w[1]), ticket=int(w[2]), k=int(w[3]), after=[int(x) for x in w[4:8]])


def run_select_segment(v, take, n, segments):
    """v, take: (segments * n,) arrays -> (segments, 256) result bits."""
    v = np.ascontiguousarray(v, np.float32)
    src = _gpu(v) if v.size else _empty(1, np.float32)
    tk = None if take is None else (_gpu(np.ascontiguousarray(take, np.uint8)) if v.size else _empty(1, np.uint8))
    dst = _empty(segments * 256, np.uint32, 0xAB)
    _ok(probe().lvdgs_probe_select_segment(src.data_ptr(), None if tk is None else tk.data_ptr(), n, segments, v.size, 0 if tk is None else tk.numel(), dst.data_ptr(), dst.numel(), _stream(dst)),
        "lvdgs_probe_select_segment")
    return _host(dst, np.uint32, segments * 256).reshape(segments, 256)


def run_hist_add(ok, digit):
    a, d = _gpu(np.ascontiguousarray(ok, np.uint8)), _gpu(np.ascontiguousarray(digit, np.uint32))
    dst = _empty(256, np.uint32, 0xAB)
    _ok(probe().lvdgs_probe_hist_add(a.data_ptr(), d.data_ptr(), 64, dst.data_ptr(), dst.numel(), _stream(dst)), "lvdgs_probe_hist_add")
    return _host(dst, np.uint32, 256)


# ---------------------------------------------------------------- references
def waves(x):
    """(..., n) -> (..., n / 64, 64)."""
    x = np.asarray(x)
    return x.reshape(x.shape[:-1] + (-1, 64))


def _row_prefix(v):
    """In-row (16 lanes) inclusive prefix, Hillis-Steele: four statements v += (v moved up by 1, 2, 4, 8 lanes inside the row, zero filled).  A lane without
    a source adds +0 like the hardware does (so a -0 there becomes +0)."""
    rows = v.reshape(v.shape[:-1] + (4, 16))
    for s in (1, 2, 4, 8):
        moved = np.zeros_like(rows)
        moved[..., s:] = rows[..., :-s]
        rows = rows + moved
    return rows.reshape(v.shape)


def emulate_row_chain(v):
    """wave_sum_to_lane63 / wave_inclusive_scan_dpp statement by statement on (..., 64) of float32 (or uint32): the row prefixes, then lane 15 of rows 0 and 2
    into rows 1 and 3, then lane 31 into rows 2 and 3.  Every lane is the wave's inclusive prefix in that order; lane 63 the total."""
    v = _row_prefix(np.asarray(v))
    add = np.zeros_like(v)
    add[..., 16:32] = v[..., 15:16]
    add[..., 48:64] = v[..., 47:48]
    v = v + add
    add = np.zeros_like(v)
    add[..., 32:64] = v[..., 31:32]
    return v + add


def emulate_butterfly(v, op=np.add):
    """wave_sum / wave_max: v = op(v, v[lane ^ off]) for off = 32, 16, ... 1, on (..., 64)."""
    v = np.asarray(v)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lanes ^ off])
    return v


def emulate_block_sum(v, n_waves):
    """block_sum<4> / <8>(float) of (..., 64 * n_waves) float32: the row chain's lane 63 per wave, then left to right (4) or the pairwise tree (8)."""
    s = emulate_row_chain(waves(np.asarray(v, np.float32)))[..., 63]
    assert s.shape[-1] == n_waves and s.dtype == np.float32
    if n_waves == 4:
        return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]
    assert n_waves == 8
    return ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))


def emulate_row_sums3(v):
    """row_sums3 of one register: the in-row prefix of (..., 64) float32."""
    return _row_prefix(np.asarray(v, np.float32))


def float64_bound(values, depth):
    """(sum in float64, depth * 2^-24 * sum |v|) over the last axis: the first-order bound of a float32 summation tree whose longest path has `depth`
    additions (each addition's relative error is at most 2^-24)."""
    v = np.asarray(values, np.float64)
    return v.sum(axis=-1), depth * 2.0 ** -24 * np.abs(v).sum(axis=-1)


def order_case():
    """One wave built so that the order of summation shows: lane 0 holds 2^24, the others +1 and -1 in turn (true sum 2^24 - 1; the row chain gives it,
    the xor butterfly gives 2^24 - 2)."""
    v = np.where(np.arange(64) % 2, -1.0, 1.0).astype(np.float32)
    v[0] = 2.0 ** 24
    return v


WAVE_DEPTH, BLOCK_DEPTH = 6, 9      # additions on the longest path: a wave; block_sum<4> (6 + 3) and <8> (6 + 3)


def exclusive_scan(values, dtype):
    """Exclusive prefix and total over the last axis in Python-sized integers, reduced modulo the type."""
    bits = 8 * np.dtype(dtype).itemsize
    v = np.asarray(values).astype(object)
    inc = np.cumsum(v, axis=-1)
    mod = lambda a: np.vectorize(lambda z: int(z) % (1 << bits), otypes=[object])(a)      # noqa: E731
    excl, total = mod(inc - v), mod(inc[..., -1])
    if np.dtype(dtype).kind == "i":
        signed = lambda a: np.vectorize(lambda z: z - (1 << bits) if z >> (bits - 1) else z, otypes=[object])(a)      # noqa: E731
        excl, total = signed(excl), signed(total)
    return excl.astype(dtype), np.asarray(total).astype(dtype)


class SortedReference:
    """The order statistics of values[take] under the float order with -0 before +0 (no NaN), from a sort of the values: equal values have equal bits
    except the zeros, which lie together in the sorted array -- the negative ones first."""

    def __init__(self, values, take=None):
        v = np.asarray(values, np.float32)
        if take is not None:
            v = v[np.asarray(take, bool)]
        assert not np.isnan(v).any()
        self.sorted = np.sort(v)
        self.n = int(v.size)
        self.zeros_from = int(np.searchsorted(self.sorted, np.float32(0), "left"))
        self.zeros_upto = int(np.searchsorted(self.sorted, np.float32(0), "right"))
        self.negative_zeros = int(np.count_nonzero((v == 0) & np.signbit(v)))

    def bits(self, rank):
        """The 32 bits of the rank-th smallest; the quiet NaN when nothing takes part."""
        if self.n == 0:
            return QUIET_NAN
        if self.zeros_from <= rank < self.zeros_upto:
            return 0x80000000 if rank - self.zeros_from < self.negative_zeros else 0
        return int(self.sorted[rank].view(np.uint32))


def select_reference(values, take, rank):
    return SortedReference(values, take).bits(rank)


def fmix32(i):
    h = np.asarray(i, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.uint32)


def rank_of(fixed, fraction, n):
    """SelectRank::of in Python: the fixed rank; the lower median for fraction 0; else keep - 1 with keep = int(float(n) * fraction), 0 when keep == 0."""
    if fixed >= 0:
        return fixed & 0xFFFFFFFF
    if fraction == 0.0:
        return (n - 1) // 2 if n else 0
    keep = int(float(n) * fraction)
    return keep - 1 if keep > 0 else 0
