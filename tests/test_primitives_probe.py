"""The host side of the shared primitives (csrc/spans.hpp, select.hpp) through the probe library, and the NumPy references of
tests/primitives_probe.py against their float64 bound -- no GPU.  The device side: tests/test_gpu_primitives.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import primitives_probe as pp

THREADS = (64, 256, 1024)
CAPS = (1, 2, 512, 2048, 65536)
N_MAX = 2 ** 31 - 1


def _sizes(threads):
    rng = np.random.default_rng(threads)
    # half of the random sizes small (where the minimum span and the cap of one meet), half anywhere up to the contract's 2^31 - 1
    random = np.concatenate((rng.integers(0, 1 << 22, 1000), rng.integers(0, N_MAX, 1000, endpoint=True)))
    return [0, 1, threads - 1, threads, threads + 1, N_MAX] + [int(x) for x in random]


@pytest.mark.parametrize("threads", THREADS)
def test_span_length_and_make_spans_against_python_integers(threads):
    L = pp.probe()
    for cap, min_factor in itertools.product(CAPS, (1, 16)):
        min_span = min_factor * threads
        for n in _sizes(threads):
            # span_length: the smallest multiple of `threads` with cap * span >= n, at least `threads`
            tiles = max(-(-n // (cap * threads)), 1)
            fit = L.lvdgs_probe_span_length(n, cap, threads)
            assert fit == tiles * threads, (n, cap, threads)
            assert cap * fit >= n and (fit == threads or cap * (fit - threads) < n)
            # span_range's comment, a fixed grid over span_length's spans: blocks * span < n + blocks * threads (n == 0: the one minimal span each), in 32 bits
            assert cap * fit < max(n, 1) + cap * threads and cap * fit < 2 ** 32
            blocks, span = pp.make_spans(n, threads, cap, min_span)
            if n == 0:
                assert blocks == 0      # no span
                continue
            want_span = max(min_span, fit)
            assert (blocks, span) == (-(-n // want_span), want_span), (n, cap, threads, min_span)
            assert span % threads == 0 and span >= min_span
            assert (blocks - 1) * span < n <= blocks * span
            assert 1 <= blocks <= cap
            assert blocks * span < 2 ** 32      # span_range: block * span must fit 32 bits


def test_make_spans_of_nothing_and_of_a_negative_count():
    assert pp.make_spans(0, 256, 512, 4096) == (0, 4096)
    assert pp.make_spans(-5, 256, 512, 4096) == (0, 4096)


def _float_order(bits):
    """The indices that sort uint32 float patterns (no NaN) by value, -0 before +0."""
    v = bits.view(np.float32)
    return np.lexsort(((v == 0) & ~np.signbit(v), v))


def test_select_key_orders_floats_and_select_unkey_inverts_it():
    L = pp.probe()
    sweep = [(s << 31) | (e << 23) | m for s in (0, 1) for e in range(256) for m in (0, 1, 1 << 22, (1 << 23) - 1) if not (e == 255 and m)]
    assert len(sweep) == 2 * (255 * 4 + 1)      # every exponent, both signs, the four mantissas; of exponent 255 the infinities only
    rng = np.random.default_rng(5)
    random = rng.integers(0, 1 << 32, 1_100_000, dtype=np.uint64).astype(np.uint32)
    random = random[~np.isnan(random.view(np.float32))][:1_000_000]
    assert random.size == 1_000_000
    for bits in (np.asarray(sweep, np.uint32), random):
        keys, back = pp.select_keys(bits)
        assert np.array_equal(back, bits)
        by_key, by_value = np.argsort(keys, kind="stable"), _float_order(bits)
        assert np.array_equal(bits[by_key], bits[by_value])      # (equal patterns may swap places; the sequences of patterns may not differ)
        assert np.unique(keys).size == np.unique(bits).size
    # the scalar entry points are the same functions
    for b in (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000):
        k = L.lvdgs_probe_select_key(b)
        assert k == int(pp.select_keys([b])[0][0]) and L.lvdgs_probe_select_unkey(k) == b
    # -inf < -1 < -denormal < -0 < +0 < +denormal < 1 < +inf
    chain = [0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000]
    keys = [L.lvdgs_probe_select_key(b) for b in chain]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_select_rank_and_lower_median_against_python():
    L = pp.probe()
    for n in (0, 1, 2, 3, 2 ** 31 - 1, 2 ** 32 - 1):
        assert L.lvdgs_probe_lower_median_rank(n) == ((n - 1) // 2 if n else 0)
        assert L.lvdgs_probe_select_rank_of(-1, 0.0, n) == ((n - 1) // 2 if n else 0)
        for fraction in (1 / 4, 1 / 32, 1 / 3, 1.0, 1e-12):
            keep = int(float(n) * fraction)
            want = keep - 1 if keep > 0 else 0
            assert L.lvdgs_probe_select_rank_of(-1, fraction, n) == want == pp.rank_of(-1, fraction, n), (n, fraction)
        for fixed in (0, 1, 7, 2 ** 31 - 1, 2 ** 32 - 1):
            assert L.lvdgs_probe_select_rank_of(fixed, 0.5, n) == fixed
    assert L.lvdgs_probe_select_rank_of(-1, 1.0, 2 ** 32 - 1) == 2 ** 32 - 2 and L.lvdgs_probe_select_rank_of(-1, 1e-12, 2 ** 32 - 1) == 0


def test_select_blocks_at_its_two_clamps():
    L = pp.probe()
    per = 256 * 8      # SEL_THREADS * SEL_ITEMS_PER_THREAD
    assert [L.lvdgs_probe_select_blocks(n) for n in (0, 1, per, per + 1, 2 * per, 2 * per + 1)] == [1, 1, 1, 2, 2, 3]
    assert [L.lvdgs_probe_select_blocks(n) for n in (511 * per + 1, 512 * per, 512 * per + 1, 2 ** 31 - 1, 2 ** 40)] == [512] * 5
    assert L.lvdgs_probe_select_blocks(511 * per) == 511


# ---------------------------------------------------------------- the emulators against the float64 bound
def _random_waves(count, seed):
    """(count, 64) float32: mixed signs, magnitudes from 2^-20 to 2^20."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (count, 64)) * np.exp2(rng.uniform(-20, 20, (count, 64)))).astype(np.float32)


def test_wave_emulators_hold_the_float64_bound():
    v = _random_waves(1000, 11)
    total, bound = pp.float64_bound(v, pp.WAVE_DEPTH)
    chain = pp.emulate_row_chain(v)
    assert chain.dtype == np.float32 and (np.abs(chain[:, 63].astype(np.float64) - total) <= bound).all()
    # every lane of the chain is the inclusive prefix up to it
    for lane in (0, 15, 16, 31, 32, 47, 48, 62):
        t, b = pp.float64_bound(v[:, :lane + 1], pp.WAVE_DEPTH)
        assert (np.abs(chain[:, lane].astype(np.float64) - t) <= b).all(), lane
    fly = pp.emulate_butterfly(v)
    assert fly.dtype == np.float32 and (fly.view(np.uint32) == fly.view(np.uint32)[:, :1]).all()      # the same bits in every lane
    assert (np.abs(fly[:, 0].astype(np.float64) - total) <= bound).all()
    d = v.astype(np.float64)
    fly64 = pp.emulate_butterfly(d)
    assert (np.abs(fly64[:, 0] - d.sum(axis=1)) <= pp.WAVE_DEPTH * 2.0 ** -53 * np.abs(d).sum(axis=1)).all()
    rows = pp.emulate_row_sums3(v)
    for row in range(4):
        t, b = pp.float64_bound(v[:, 16 * row:16 * row + 16], 4)
        assert (np.abs(rows[:, 16 * row + 15].astype(np.float64) - t) <= b).all()
    # the two orders are different orders: on the case built for it they give different bits
    shows = pp.order_case()
    assert float(pp.emulate_row_chain(shows)[63]) == 2.0 ** 24 - 1 and float(pp.emulate_butterfly(shows)[0]) == 2.0 ** 24 - 2


@pytest.mark.parametrize("n_waves", [4, 8])
def test_block_sum_emulator_holds_the_float64_bound(n_waves):
    v = _random_waves(1000 * n_waves, 12 + n_waves).reshape(1000, 64 * n_waves)
    total, bound = pp.float64_bound(v, pp.BLOCK_DEPTH)
    got = pp.emulate_block_sum(v, n_waves)
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - total) <= bound).all()


def test_left_to_right_and_pairwise_differ_where_they_should():
    # wave totals (2^24, 1, 1, -2^24, ...): left to right loses both ones, the pairwise tree one of them
    totals = np.asarray([2.0 ** 24, 1, 1, -2.0 ** 24, 2.0 ** 24, 1, 1, -2.0 ** 24], np.float32)
    v = np.zeros((8, 64), np.float32)
    v[:, 63] = totals
    assert float(pp.emulate_block_sum(v[:4].reshape(-1), 4)) == 0.0
    assert float(pp.emulate_block_sum(v.reshape(-1), 8)) == 2.0      # ((2^24 + 1) + (1 - 2^24)) twice: 2^24 + (1 - 2^24) = 1 each
    assert float(v.astype(np.float64).sum()) == 4.0


def test_integer_reference_wraps_like_the_type():
    excl, total = pp.exclusive_scan(np.asarray([0xFFFFFFFF, 2, 3], np.uint32), np.uint32)
    assert excl.tolist() == [0, 0xFFFFFFFF, 1] and int(total) == 4
    excl, total = pp.exclusive_scan(np.asarray([0x7FFFFFFF, 1, -5], np.int32), np.int32)
    assert excl.tolist() == [0, 0x7FFFFFFF, -2 ** 31] and int(total) == 2 ** 31 - 5
    excl, total = pp.exclusive_scan(np.asarray([2 ** 63, 2 ** 63, 7], np.uint64), np.uint64)
    assert excl.tolist() == [0, 2 ** 63, 0] and int(total) == 7


def test_select_reference_orders_the_zeros_and_reports_nothing_as_nan():
    v = np.asarray([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], np.float32)
    assert [pp.select_reference(v, None, k) for k in range(6)] == [0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000]
    assert pp.select_reference(v, np.zeros(6, bool), 0) == pp.QUIET_NAN
    assert pp.select_reference(v, [0, 0, 1, 0, 0, 0], 0) == 0x3F800000
    assert pp.fmix32(np.arange(3)).tolist() == [0, 0x514E28B7, 0x30F4C306]      # MurmurHash3's finalizer on 0, 1, 2


# ---------------------------------------------------------------- refusals: nothing is launched on a mistake
def test_host_entry_points_refuse_bad_arguments_without_a_device():
    L = pp.probe()
    buf = (C.c_uint64 * 4096)()
    p, big = C.addressof(buf), C.sizeof(buf)
    state = L.lvdgs_probe_select_state_bytes()
    assert state % 256 == 0 and L.lvdgs_probe_select_report_words() == 8
    refused = [
        ("wave: no such op", lambda: L.lvdgs_probe_wave(99, 64, 1, p, big, p, big, 0, 0, None)),
        ("wave: negative op", lambda: L.lvdgs_probe_wave(-1, 64, 1, p, big, p, big, 0, 0, None)),
        ("wave: 128 threads", lambda: L.lvdgs_probe_wave(0, 128, 1, p, big, p, big, 0, 0, None)),
        ("wave: no workgroup", lambda: L.lvdgs_probe_wave(0, 64, 0, p, big, p, big, 0, 0, None)),
        ("wave: NULL in", lambda: L.lvdgs_probe_wave(0, 64, 1, None, big, p, big, 0, 0, None)),
        ("wave: NULL out", lambda: L.lvdgs_probe_wave(0, 64, 1, p, big, None, big, 0, 0, None)),
        ("wave: short in", lambda: L.lvdgs_probe_wave(0, 64, 1, p, 255, p, big, 0, 0, None)),
        ("wave: short out (six planes)", lambda: L.lvdgs_probe_wave(pp.WAVE_OPS.index("row_sums3"), 64, 1, p, big, p, 6 * 256 - 1, 0, 0, None)),
        ("wave: lane 64", lambda: L.lvdgs_probe_wave(pp.WAVE_OPS.index("write_lane"), 64, 1, p, big, p, big, 0, 64, None)),
        ("mask: bit 64", lambda: L.lvdgs_probe_mask_bit(1, 0, 64, p, big, None)),
        ("mask: NULL", lambda: L.lvdgs_probe_mask_bit(1, 0, 3, None, big, None)),
        ("mask: short", lambda: L.lvdgs_probe_mask_bit(1, 0, 3, p, 511, None)),
        ("scan: dtype", lambda: L.lvdgs_probe_scan(0, 3, 64, 1, p, big, p, big, 0, None)),
        ("scan: 512 threads", lambda: L.lvdgs_probe_scan(0, 0, 512, 1, p, big, p, big, 0, None)),
        ("scan: NULL", lambda: L.lvdgs_probe_scan(0, 0, 64, 1, None, big, p, big, 0, None)),
        ("scan: trips without the contract probe", lambda: L.lvdgs_probe_scan(0, 0, 64, 1, p, big, p, big, 1, None)),
        ("scan: four trips", lambda: L.lvdgs_probe_scan(1, 0, 64, 1, p, big, p, big, 4, None)),
        ("scan: short out", lambda: L.lvdgs_probe_scan(0, 2, 64, 1, p, big, p, 1023, 0, None)),
        ("scan: short in (contract)", lambda: L.lvdgs_probe_scan(1, 0, 64, 1, p, 6 * 256 - 1, p, big, 3, None)),
        ("block_sum: float of 16 waves", lambda: L.lvdgs_probe_block_sum(0, 16, 1, p, big, p, big, None)),
        ("block_sum: int of 8 waves", lambda: L.lvdgs_probe_block_sum(1, 8, 1, p, big, p, big, None)),
        ("block_sum: NULL", lambda: L.lvdgs_probe_block_sum(0, 4, 1, p, big, None, big, None)),
        ("block_sum: short", lambda: L.lvdgs_probe_block_sum(0, 4, 1, p, 2047, p, big, None)),
        ("span_range: NULL", lambda: L.lvdgs_probe_span_range(10, 256, 1, None, big, None)),
        ("span_range: short", lambda: L.lvdgs_probe_span_range(10, 256, 7, p, 55, None)),
        ("span_range: span 0", lambda: L.lvdgs_probe_span_range(10, 0, 1, p, big, None)),
        ("span_range: n beyond 2^31 - 1", lambda: L.lvdgs_probe_span_range(2 ** 31, 256, 1, p, big, None)),
        ("span_range: blocks * span beyond 32 bits", lambda: L.lvdgs_probe_span_range(10, 2 ** 31, 2, p, big, None)),
        ("span_counts: form", lambda: L.lvdgs_probe_span_counts(4, p, big, p, big, 1, 1, p, big, None)),
        ("span_counts: negative", lambda: L.lvdgs_probe_span_counts(0, p, big, p, big, -1, 1, p, big, None)),
        ("span_counts: stride 0", lambda: L.lvdgs_probe_span_counts(0, p, big, p, big, 1, 0, p, big, None)),
        ("span_counts: in place across types", lambda: L.lvdgs_probe_span_counts(1, p, big, p, big, 1, 1, p, big, None)),
        ("span_counts: short before", lambda: L.lvdgs_probe_span_counts(1, p, big, p + 1024, 8 * 10 * 5 - 1, 10, 5, p, big, None)),
        ("span_counts: short totals", lambda: L.lvdgs_probe_span_counts(3, p, big, p + 1024, big - 1024, 10, 1, p, 8 * 1024 - 1, None)),
        ("span_counts: NULL", lambda: L.lvdgs_probe_span_counts(0, None, big, p, big, 1, 1, p, big, None)),
        ("compact: form", lambda: L.lvdgs_probe_compact(4, p, big, 10, 1, 0, p, big, p, p, 11, big, big, p, None)),
        ("compact: negative n", lambda: L.lvdgs_probe_compact(0, p, big, -1, 1, 0, p, big, p, p, 11, big, big, p, None)),
        ("compact: no workgroup", lambda: L.lvdgs_probe_compact(0, p, big, 10, 0, 0, p, big, p, p, 11, big, big, p, None)),
        ("compact: NULL keep", lambda: L.lvdgs_probe_compact(0, None, big, 10, 1, 0, p, big, p, p, 11, big, big, p, None)),
        ("compact: short keep", lambda: L.lvdgs_probe_compact(0, p, 9, 10, 1, 0, p, big, p, p, 11, big, big, p, None)),
        ("compact: outputs below the capacity", lambda: L.lvdgs_probe_compact(0, p, big, 10, 1, 0, p, big, p, p, 11, 43, big, p, None)),
        ("compact: short scratch", lambda: L.lvdgs_probe_compact(0, p, big, 10, 7, 0, p, 111, p, p, 11, big, big, p, None)),
        ("compact: a 32-bit walk from above 2^32", lambda: L.lvdgs_probe_compact(0, p, big, 10, 1, 2 ** 32, p, big, p, p, 11, big, big, p, None)),
        ("select: negative n", lambda: L.lvdgs_probe_select(p, big, None, 0, -1, 0, -1, 0.0, p, big, p, big, 0, None)),
        ("select: NULL values", lambda: L.lvdgs_probe_select(None, 0, None, 0, 5, 0, -1, 0.0, p, big, p, big, 0, None)),
        ("select: NULL state", lambda: L.lvdgs_probe_select(p, big, None, 0, 5, 0, -1, 0.0, None, big, p, big, 0, None)),
        ("select: short state", lambda: L.lvdgs_probe_select(p, big, None, 0, 5, 0, -1, 0.0, p, state - 1, p, big, 0, None)),
        ("select: short report", lambda: L.lvdgs_probe_select(p, big, None, 0, 5, 0, -1, 0.0, p, big, p, 31, 0, None)),
        ("select: short values", lambda: L.lvdgs_probe_select(p, 4, None, 0, 5, 0, -1, 0.0, p, big, p, big, 0, None)),
        ("select: short take", lambda: L.lvdgs_probe_select(p, big, p, 4, 5, 0, -1, 0.0, p, big, p, big, 0, None)),
        ("select: short take with keys", lambda: L.lvdgs_probe_select(None, 0, p, 4, 5, 1, -1, 0.0, p, big, p, big, 0, None)),
        ("select: fraction 1.5", lambda: L.lvdgs_probe_select(p, big, None, 0, 5, 0, -1, 1.5, p, big, p, big, 0, None)),
        ("select_segment: negative n", lambda: L.lvdgs_probe_select_segment(p, None, -1, 1, 10, 0, p, big, None)),
        ("select_segment: no segment", lambda: L.lvdgs_probe_select_segment(p, None, 5, 0, 10, 0, p, big, None)),
        ("select_segment: NULL", lambda: L.lvdgs_probe_select_segment(None, None, 5, 1, 10, 0, p, big, None)),
        ("select_segment: short values", lambda: L.lvdgs_probe_select_segment(p, None, 5, 3, 14, 0, p, big, None)),
        ("select_segment: short take", lambda: L.lvdgs_probe_select_segment(p, p, 5, 3, 15, 14, p, big, None)),
        ("select_segment: short out", lambda: L.lvdgs_probe_select_segment(p, None, 5, 3, 15, 0, p, 3 * 1024 - 1, None)),
        ("hist_add: NULL", lambda: L.lvdgs_probe_hist_add(None, p, 64, p, big, None)),
        ("hist_add: 63 lanes", lambda: L.lvdgs_probe_hist_add(p, p, 63, p, big, None)),
        ("hist_add: short out", lambda: L.lvdgs_probe_hist_add(p, p, 64, p, 1023, None)),
        ("select_keys: NULL", lambda: L.lvdgs_probe_select_keys(None, p, p, 1)),
        ("select_keys: negative", lambda: L.lvdgs_probe_select_keys(p, p, p, -1)),
    ]
    for what, call in refused:
        assert call() == pp.E_INVALID, what
        assert pp.last_error().startswith("probe "), (what, pp.last_error())


def test_the_probe_is_not_part_of_the_product_library():
    from lvdgs import _lib
    assert not any(name.startswith("lvdgs_probe") for name in _lib.EXPORTS)
    assert not any(hasattr(_lib.lib(), name) for name in ("lvdgs_probe_wave", "lvdgs_probe_select"))
