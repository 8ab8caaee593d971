"""The shared wave, scan, span and select primitives (csrc/device_utils.hpp, spans.hpp, select.hpp) on the GPU, one at a time through the
probe library, against the NumPy references of tests/primitives_probe.py: integers exactly, float reductions bit for bit against an
emulation of the stated order AND within a float64 bound derived from the tree depth, the select against a sort.  The host side and the
references themselves: tests/test_primitives_probe.py."""
import numpy as np
import pytest

import primitives_probe as pp

pytestmark = pytest.mark.gpu

WORKGROUPS = (64, 256, 1024)
SEAMS = (0, 15, 16, 31, 32, 47, 48, 63)      # the first and last lane of every 16-lane row
FOUR_LANES = (0, 31, 32, 63)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def wave_run(op, threads, x, a0=0, a1=0):
    """Op over K waves ((K, 64) or (planes, K, 64)) in launches of TWO workgroups of `threads` threads (so `lane = threadIdx.x & 63` runs in every wave of a
    workgroup); the last launch is filled up with the first waves again -> (out planes, K, 64)."""
    x = np.asarray(x)
    x = x[None] if x.ndim == 2 else x
    K, per = x.shape[1], 2 * threads // 64
    padded = np.concatenate([x, x[:, np.arange((-K) % per) % K]], axis=1)
    out = [pp.run_wave(op, threads, padded[:, at:at + per].reshape(x.shape[0], -1), a0, a1) for at in range(0, padded.shape[1], per)]
    return np.concatenate([o.reshape(o.shape[0], per, 64) for o in out], axis=1)[:, :K]


def mixed_waves(count, seed):
    """(count, 64) float32: mixed signs, magnitudes from 2^-20 to 2^20."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (count, 64)) * np.exp2(rng.uniform(-20, 20, (count, 64)))).astype(np.float32)


def order_waves():
    """Waves in which the order of summation shows: one lane at 2^24, the others +-1."""
    rng = np.random.default_rng(21)
    out = [pp.order_case()]
    for lane in FOUR_LANES:
        v = rng.choice([-1.0, 1.0], 64).astype(np.float32)
        v[lane] = 2.0 ** 24
        out.append(v)
    return np.stack(out)


def wrapped_sum(x, dtype):
    """Sum over the last axis in Python integers, reduced to the type."""
    bits = 8 * np.dtype(dtype).itemsize
    total = np.asarray(x).astype(object).sum(axis=-1)
    wrap = np.vectorize(lambda z: (int(z) % (1 << bits)) - ((1 << bits) if np.dtype(dtype).kind == "i" and (int(z) % (1 << bits)) >> (bits - 1) else 0), otypes=[object])
    return wrap(total).astype(dtype)


# ================================================================ wave level
@pytest.mark.parametrize("threads", WORKGROUPS)
@pytest.mark.parametrize("op,dtype", [("sum_i32", np.int32), ("sum_u32", np.uint32), ("sum_u64", np.uint64)])
def test_wave_sum_of_integers_wraps(threads, op, dtype):
    rng = np.random.default_rng(31)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max, (33, 64), dtype=dtype, endpoint=True)
    x[1] = info.max      # every lane at the top: wraps 63 times
    want = wrapped_sum(x, dtype)
    assert int(np.abs(x[0].astype(object)).sum()) > info.max      # (the inputs do wrap)
    got = wave_run(op, threads, x)[0]
    assert np.array_equal(got, np.broadcast_to(want[:, None], got.shape))


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_wave_sum_of_floats_is_the_butterfly_bit_for_bit(threads):
    v = np.concatenate([mixed_waves(27, 32), order_waves()])
    got = wave_run("sum_f32", threads, v)[0]
    want = pp.emulate_butterfly(v)
    assert np.array_equal(u32(got), u32(want))      # (which says every lane holds the same bits: the emulation does)
    assert (u32(got) == u32(got)[:, :1]).all()
    total, bound = pp.float64_bound(v, pp.WAVE_DEPTH)
    assert (np.abs(got[:, 0].astype(np.float64) - total) <= bound).all()
    d = np.concatenate([mixed_waves(27, 33).astype(np.float64) * (1 + 2.0 ** -40), order_waves().astype(np.float64) * 2.0 ** 29])
    got = wave_run("sum_f64", threads, d)[0]
    assert np.array_equal(got.view(np.uint64), pp.emulate_butterfly(d).view(np.uint64))
    assert (np.abs(got[:, 0] - d.sum(axis=1)) <= pp.WAVE_DEPTH * 2.0 ** -53 * np.abs(d).sum(axis=1)).all()


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_wave_sum_to_lane63_is_the_row_chain_bit_for_bit(threads):
    v = np.concatenate([mixed_waves(27, 34), order_waves()])
    got = wave_run("sum_lane63", threads, v)[0][:, 63]      # lane 63 only: the other lanes are unspecified
    assert np.array_equal(u32(got), u32(pp.emulate_row_chain(v)[:, 63]))
    total, bound = pp.float64_bound(v, pp.WAVE_DEPTH)
    assert (np.abs(got.astype(np.float64) - total) <= bound).all()
    # the case built for it: this order keeps the 2^24 - 1 the butterfly loses
    assert float(got[27]) == 2.0 ** 24 - 1


def extreme_waves(rng, sign):
    """Float waves for max (sign +1) / min (-1): random, with infinities, a single extreme in each of four lanes, all lanes equal, both zeros."""
    out = [mixed_waves(1, 35)[0], np.full(64, 3.5, np.float32), np.full(64, -np.inf, np.float32), np.full(64, np.inf, np.float32)]
    v = mixed_waves(1, 36)[0]
    v[5], v[40] = np.inf, -np.inf
    out.append(v)
    v = np.full(64, -sign * np.inf, np.float32)      # one finite lane among infinities of the losing sign
    v[17] = 2.5
    out.append(v)
    out.append(np.where(rng.random(64) < 0.5, -0.0, 0.0).astype(np.float32))
    for lane in FOUR_LANES:
        v = -sign * np.abs(mixed_waves(1, 37 + lane)[0])
        v[lane] = sign * 2.0 ** 21
        out.append(v.astype(np.float32))
    return np.stack(out)


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_wave_max_and_min(threads):
    rng = np.random.default_rng(38)
    for op, dtype in (("max_i32", np.int32), ("max_u32", np.uint32)):
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max, (12, 64), dtype=dtype, endpoint=True)
        x[1] = 7      # all lanes equal
        x[2] = info.min
        for k, lane in enumerate(FOUR_LANES):      # a single extreme
            x[3 + k] = rng.integers(info.min, 0 if dtype == np.int32 else 1000, 64, dtype=dtype)
            x[3 + k, lane] = info.max
        got = wave_run(op, threads, x)[0]
        assert np.array_equal(got, np.broadcast_to(x.max(axis=1)[:, None], got.shape)), op
    for op, sign, reduce in (("max_f32", 1.0, np.max), ("min_f32", -1.0, np.min)):
        v = extreme_waves(rng, sign)
        got = wave_run(op, threads, v)[0]
        assert not np.isnan(got).any()
        assert np.array_equal(got, np.broadcast_to(reduce(v, axis=1)[:, None], got.shape)), op      # by value: -0 == +0


def scan_inputs():
    rng = np.random.default_rng(39)
    x = [rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    x.append(np.ones(64, np.uint32))
    x.append(np.full(64, 0xFFFFFFFF, np.uint32))      # near 2^32: wraps at every lane
    x.append((0xFFFFFF00 + rng.integers(0, 256, 64)).astype(np.uint32))
    x.append(np.zeros(64, np.uint32))
    for lane in SEAMS:
        for value in (1, 0x80000001):
            v = np.zeros(64, np.uint32)
            v[lane] = value
            x.append(v)
    return np.stack(x)


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_wave_scans_agree_with_each_other_and_with_cumsum(threads):
    x = scan_inputs()
    want = (np.cumsum(x.astype(np.uint64), axis=1) & 0xFFFFFFFF).astype(np.uint32)
    shuffles, dpp = wave_run("scan_u32", threads, x)[0], wave_run("scan_dpp", threads, x)[0]
    assert np.array_equal(shuffles, want) and np.array_equal(dpp, want)
    assert np.array_equal(pp.emulate_row_chain(x), want)      # (the order the header states, in integers)
    signed = np.concatenate([x.view(np.int32), np.random.default_rng(40).integers(-1000, 1000, (4, 64), dtype=np.int32), -np.ones((1, 64), np.int32)])
    assert (signed < 0).any()
    want = (np.cumsum(signed.astype(np.int64), axis=1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    assert np.array_equal(wave_run("scan_i32", threads, signed)[0], want)


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_folds_rotations_and_dpp_moves(threads):
    a, b = mixed_waves(5, 42), mixed_waves(5, 43)
    assert np.unique(a).size == a.size      # distinct values: a lane that reads the wrong source shows
    got = wave_run("fold32", threads, np.stack([a, b]))[0]
    want = np.concatenate([a[:, :32] + a[:, 32:], b[:, :32] + b[:, 32:]], axis=1)
    assert np.array_equal(u32(got), u32(want))
    got = wave_run("fold16", threads, np.stack([a, b]))[0]
    ra, rb = a.reshape(-1, 4, 16), b.reshape(-1, 4, 16)
    want = np.stack([ra[:, 0] + ra[:, 1], rb[:, 0] + rb[:, 1], ra[:, 2] + ra[:, 3], rb[:, 2] + rb[:, 3]], axis=1).reshape(-1, 64)
    assert np.array_equal(u32(got), u32(want))
    for n in (1, 4, 8, 15):      # lane i of a row gets lane (i - N) mod 16 of it
        got = wave_run(f"rot{n}", threads, a)[0]
        assert np.array_equal(u32(got), u32(np.roll(ra, n, axis=2).reshape(-1, 64))), n
    for op, shift in (("dpp_shr1", 1), ("dpp_shr8", 8)):      # lane i of a row gets lane i - shift, 0 where there is none
        want = np.zeros_like(ra)
        want[:, :, shift:] = ra[:, :, :-shift]
        assert np.array_equal(u32(wave_run(op, threads, a)[0]), u32(want.reshape(-1, 64))), op


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_row_sums3_twice_behind_a_dependent_valu_write(threads):
    planes = np.stack([mixed_waves(6, 44 + k) for k in range(3)])
    s0, s1 = np.float32(2.0), np.float32(0.5)      # (exact scalings: the probe multiplies right in front of each call)
    got = wave_run("row_sums3", threads, planes, int(s0.view(np.int32)), int(s1.view(np.int32)))
    first = pp.emulate_row_sums3(planes * s0)
    second = pp.emulate_row_sums3(first * s1)
    assert first.dtype == np.float32 and second.dtype == np.float32
    assert np.array_equal(u32(got[:3]), u32(first)) and np.array_equal(u32(got[3:]), u32(second))
    for row in range(4):      # lane 15 of a row: the row total, within the bound of a four-deep tree
        total, bound = pp.float64_bound(planes[..., 16 * row:16 * row + 16] * 2.0, 4)
        assert (np.abs(got[:3, :, 16 * row + 15].astype(np.float64) - total) <= bound).all()


def test_mask_set_bit_and_mask_clear_bit():
    masks = (0, 0xFFFFFFFFFFFFFFFF, int(np.random.default_rng(45).integers(0, 1 << 63)) | (1 << 63) | 1)
    for mask in masks + (masks[2] ^ 0xFFFFFFFFFFFFFFFF,):
        for bit in FOUR_LANES:
            got = pp.run_mask_bit(True, mask, bit)
            assert (got == np.uint64(mask | (1 << bit))).all(), (hex(mask), bit)
            got = pp.run_mask_bit(False, mask, bit)
            assert (got == np.uint64(mask & ~(1 << bit))).all(), (hex(mask), bit)


@pytest.mark.parametrize("threads", WORKGROUPS)
def test_write_lane_changes_one_lane(threads):
    v = np.random.default_rng(46).integers(-2 ** 31, 2 ** 31, (2 * threads // 64, 64), dtype=np.int64).astype(np.int32)
    for lane, x in zip(FOUR_LANES, (0x12345678, -1, -2 ** 31, 0)):
        got = wave_run("write_lane", threads, v, x, lane)[0]
        want = v.copy()
        want[:, lane] = x
        assert np.array_equal(got, want), lane


# ================================================================ workgroup level
def scan_cases(threads, dtype):
    """One workgroup per row: random values that wrap (32 bits) or sum past 2^32 (64 bits), negatives for int, zeros, a single 1 at the wave seams."""
    rng = np.random.default_rng(47 + threads)
    if dtype == np.uint64:
        rows = [rng.integers(1 << 31, 1 << 34, threads, dtype=np.uint64), rng.integers(0, 1 << 63, threads, dtype=np.uint64) * 2 + 1]
    elif dtype == np.uint32:
        rows = [rng.integers(0, 1 << 32, threads, dtype=np.uint64).astype(np.uint32), np.full(threads, 0xFFFFFFFF, np.uint32)]
    else:
        rows = [rng.integers(-2 ** 31, 2 ** 31, threads, dtype=np.int64).astype(np.int32), rng.integers(-9, 3, threads, dtype=np.int64).astype(np.int32)]
    rows += [np.zeros(threads, dtype), np.ones(threads, dtype)]
    for at in sorted({0, 63, 64 % threads, threads - 1}):
        v = np.zeros(threads, dtype)
        v[at] = 1
        rows.append(v)
    return np.stack(rows).astype(dtype)


@pytest.mark.parametrize("threads", WORKGROUPS)
@pytest.mark.parametrize("dtype", [np.uint32, np.int32, np.uint64])
def test_scan_workgroup(threads, dtype):
    x = scan_cases(threads, dtype)
    want_excl, want_total = pp.exclusive_scan(x, dtype)
    if dtype == np.uint64:
        assert int(x[0].astype(object).sum()) > 2 ** 32      # a 64-bit scan that a 32-bit shuffle would get wrong
    if dtype == np.uint32:
        assert int(x[0].astype(object).sum()) > 2 ** 32      # wraps
    excl, total = pp.run_scan(threads, x.reshape(-1))
    assert np.array_equal(excl.reshape(x.shape), want_excl)
    assert np.array_equal(total.reshape(x.shape), np.broadcast_to(want_total[:, None], x.shape))      # the total, in every thread


@pytest.mark.parametrize("threads", WORKGROUPS)
@pytest.mark.parametrize("dtype", [np.uint32, np.int32, np.uint64])
def test_scan_workgroup_barrier_contracts(threads, dtype):
    """No barrier of the caller's: (a) two calls back to back on one s_scan with different inputs, (b) a word every thread left in LDS before the first call is
    seen by thread t - 64 behind it, (c) three more scans in a loop with a uniform trip count, as scan_span_counts calls it."""
    trips, groups = 3, 3
    rng = np.random.default_rng(48 + threads)
    hi = 1 << 40 if dtype == np.uint64 else 1 << 31
    planes = rng.integers(0, hi, (3 + trips, groups, threads), dtype=np.int64).astype(dtype)
    out = pp.run_scan_contract(threads, planes.reshape(3 + trips, -1), trips).reshape(5 + 2 * trips, groups, threads)

    def check(values, excl, total, what):
        want_excl, want_total = pp.exclusive_scan(values, dtype)
        assert np.array_equal(excl, want_excl), what
        assert np.array_equal(total, np.broadcast_to(want_total[:, None], total.shape)), what

    check(planes[0], out[0], out[1], "the first call (no barrier in front)")
    assert np.array_equal(out[2], np.roll(planes[1], -64, axis=1)), "the caller's LDS word, published by the scan's barriers"
    check(planes[2], out[3], out[4], "the second call, back to back")
    for r in range(trips):
        check(planes[3 + r], out[5 + 2 * r], out[6 + 2 * r], f"trip {r} of the loop")


def block_sum_inputs(n_waves):
    """(2, groups, 64 * n_waves) float32: two different planes for the two calls."""
    groups = 6
    v = mixed_waves(2 * groups * n_waves, 49 + n_waves).reshape(2, groups, 64 * n_waves)
    # wave totals (2^24, 1, 1, -2^24, ...): left to right and the pairwise tree differ
    totals = np.resize(np.asarray([2.0 ** 24, 1, 1, -2.0 ** 24], np.float32), n_waves)
    v[0, 1] = 0
    v[0, 1, 63::64] = totals
    v[1, 2] = 0
    v[1, 2, 5::64] = totals[::-1]
    v[1, 3] = np.repeat(order_waves()[:4], n_waves // 4, axis=0).reshape(-1)      # the order inside the waves shows too
    return v


@pytest.mark.parametrize("n_waves", [4, 8])
def test_block_sum_of_floats_is_the_stated_order_bit_for_bit(n_waves):
    v = block_sum_inputs(n_waves)
    got = pp.run_block_sum(n_waves, v.reshape(2, -1)).reshape(v.shape)      # two calls back to back on one s
    want = pp.emulate_block_sum(v, n_waves)
    assert np.array_equal(u32(got), u32(np.broadcast_to(want[..., None], v.shape)))      # in every thread
    total, bound = pp.float64_bound(v, pp.BLOCK_DEPTH)
    assert (np.abs(got[..., 0].astype(np.float64) - total) <= bound).all()
    assert float(got[0, 1, 0]) == (0.0 if n_waves == 4 else 2.0)      # what each order makes of (2^24, 1, 1, -2^24, ...)


@pytest.mark.parametrize("n_waves", [1, 4, 16])
def test_block_sum_of_ints(n_waves):
    x = np.random.default_rng(50 + n_waves).integers(-2 ** 31, 2 ** 31, (2, 5, 64 * n_waves), dtype=np.int64).astype(np.int32)
    x[1, 0] = np.arange(64 * n_waves) - 700
    got = pp.run_block_sum(n_waves, x.reshape(2, -1)).reshape(x.shape)
    assert np.array_equal(got, np.broadcast_to(wrapped_sum(x, np.int32)[..., None], x.shape))


# ================================================================ spans
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70_001])
def test_span_range_tiles_the_elements(n):
    for blocks in (1, 2, 7, 300):
        span = pp.probe().lvdgs_probe_span_length(n, blocks, 256)
        r = pp.run_span_range(n, span, blocks).astype(np.int64)
        begin, end = r[:, 0], r[:, 1]
        assert begin[0] == 0 and end[-1] == n and np.array_equal(begin[1:], end[:-1])      # [0, n) exactly, in order
        want_begin = np.minimum(np.arange(blocks) * span, n)
        assert np.array_equal(begin, want_begin) and np.array_equal(end, np.minimum(want_begin + span, n))
        past = np.arange(blocks) * span >= n
        assert np.array_equal(begin[past], end[past])      # a workgroup past the end owns nothing
        assert (end - begin <= span).all()


def span_count_inputs(form, blocks, rng):
    """Counts for a form of scan_span_counts: every round's sum fits T; with a 64-bit carry over 32-bit rounds the total goes past 2^32 as soon as there are
    two rounds."""
    threads, T, Cc = pp.SPAN_COUNT_FORMS[form]
    if T == np.uint64:
        return rng.integers(0, 1 << 40, blocks, dtype=np.uint64)
    if Cc == np.uint32:
        return rng.integers(0, 1 << 16, blocks, dtype=np.uint64).astype(np.uint32)      # the total must fit C
    counts = np.zeros(blocks, np.uint64)
    for base in range(0, blocks, threads):
        w = rng.random(min(threads, blocks - base)) + 0.01
        counts[base:base + threads] = np.floor(w / w.sum() * 0.97 * 2 ** 32).astype(np.uint64)      # a round of about 0.97 * 2^32
    return counts.astype(np.uint32)


SENTINEL = 0xA5A5A5A5


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_scan_span_counts(form):
    threads, T, Cc = pp.SPAN_COUNT_FORMS[form]
    rng = np.random.default_rng(51 + form)
    for blocks in ((1023, 1024, 1025, 2048) if threads == 1024 else (0, 1, 255, 256, 257, 3 * 256 + 5)):
        counts = span_count_inputs(form, blocks, rng)
        rounds = [int(counts[b:b + threads].astype(object).sum()) for b in range(0, blocks, threads)]
        assert all(r < 2 ** (8 * np.dtype(T).itemsize) for r in rounds)      # the contract: a round's sum fits T
        want_total = sum(rounds)
        assert want_total < 2 ** (8 * np.dtype(Cc).itemsize)                  # ... and the total fits C
        if T == np.uint32 and Cc == np.uint64 and len(rounds) > 1:
            assert want_total > 2 ** 32      # the carry is what holds it
        want_before = np.concatenate([[0], np.cumsum(counts.astype(object))[:-1]]).astype(Cc) if blocks else np.zeros(0, Cc)
        for stride in (1, 5):
            strided = np.full(blocks * stride, SENTINEL, T)
            strided[::stride] = counts
            for in_place in ((True, False) if T == Cc else (False,)):
                want = np.full(blocks * stride, SENTINEL, Cc)
                want[::stride] = want_before
                before, totals = pp.run_span_counts(form, strided, stride, in_place, before_fill=np.full(blocks * stride, SENTINEL, Cc))
                what = (form, blocks, stride, in_place)
                assert np.array_equal(before, want), what      # the prefixes, and the four other words of every stride untouched
                assert totals.shape == (threads,) and (totals == Cc(want_total)).all(), what      # the same total in every thread


COMPACT_ROW0 = (1000, 2 ** 32 + 12345, 2 ** 33 + 7, 2 ** 40)      # where `row` starts, per form: above 2^32 where C has 64 bits
COMPACT_GRIDS = (1, 2, 7, 512)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4096, 70_001])
def test_tile_walk_compaction(form, n):
    rng = np.random.default_rng(52 + n)
    row0 = COMPACT_ROW0[form]
    for rate in (0.0, 1.0, 0.5, 1 / 256):
        keep = (rng.random(n) < rate).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)      # (any non-zero byte keeps)
        want = np.flatnonzero(keep)
        m = want.size
        first = None
        for blocks in COMPACT_GRIDS:
            idx, rows, total = pp.run_compact(form, keep, blocks, row0)
            what = (form, n, rate, blocks)
            assert total == m, what
            assert np.array_equal(idx[:m], want), what      # flatnonzero, in order
            assert np.array_equal(rows[:m], (row0 + np.arange(m, dtype=np.uint64)).astype(np.uint64)), what
            assert (idx[m:] == 0xABABABAB).all() and (rows[m:] == 0xABABABABABABABAB).all(), what      # nothing stored behind the last
            if first is None:
                first = (idx.tobytes(), rows.tobytes())
            assert (idx.tobytes(), rows.tobytes()) == first, what      # the same bytes however the elements are cut into spans


# ================================================================ select
def _from_bits(bits):
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def value_set(name, n, rng):
    if name == "uniform":
        return rng.uniform(-50, 50, n).astype(np.float32)
    if name == "negative":
        return (-rng.uniform(0.001, 50, n)).astype(np.float32)
    if name == "zeros":      # a mixture of -0 and +0, a few values either side
        return rng.choice(np.asarray([-0.0, 0.0, -0.0, 0.0, -1.5, 2.5], np.float32), n)
    if name == "infinities":
        return rng.choice(np.asarray([-np.inf, np.inf, -3.0, 0.0, 4.0, 1e30, -1e30], np.float32), n)
    if name == "denormals":
        return _from_bits(rng.integers(1, 1 << 23, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << 31))
    if name == "equal":
        return np.full(n, -3.25, np.float32)
    if name == "one_ulp":
        return rng.choice(np.asarray([1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), -1.0, np.nextafter(np.float32(-1.0), np.float32(-2.0))], np.float32), n)
    if name == "low_byte":      # the top three key bytes shared: only the last pass decides
        return _from_bits(0x42280000 | rng.integers(0, 256, n, dtype=np.uint64))
    if name == "low_byte_negative":
        return _from_bits(0xC2280000 | rng.integers(0, 256, n, dtype=np.uint64))
    assert name == "sign_only"
    return rng.choice(np.asarray([7.5, -7.5], np.float32), n)


VALUE_SETS = ("uniform", "negative", "zeros", "infinities", "denormals", "equal", "one_ulp", "low_byte", "low_byte_negative", "sign_only")
SELECT_SIZES = (0, 1, 2, 255, 256, 257, 2048, 2049, 100_003, 512 * 256 * 8 + 1)      # the last: past what 512 workgroups take in one stride
FRACTIONS = (1 / 4, 1 / 32, 1 / 3, 1.0, 1e-9)      # the last: keep == 0 at every size here


@pytest.fixture(scope="module")
def select():
    return pp.Select()


def participations(n, rng):
    one = np.zeros(n, np.uint8)
    if n:
        one[int(rng.integers(0, n))] = 1
    return [("all", None), ("none", np.zeros(n, np.uint8)), ("one", one), ("40 %", (rng.random(n) < 0.4).astype(np.uint8))]


@pytest.mark.parametrize("n", SELECT_SIZES)
@pytest.mark.parametrize("name", VALUE_SETS)
def test_select_against_a_sort(select, name, n):
    rng = np.random.default_rng(53 + n)
    v = value_set(name, n, rng)
    if name in ("zeros", "infinities", "sign_only", "one_ulp") and n > 8:
        assert np.signbit(v).any() and not np.signbit(v).all()
    dv = pp.to_gpu(v) if n else None
    if n == 0:
        dv = pp.to_gpu(np.zeros(1, np.float32))      # (a valid pointer; nothing of it is read)
    for label, take in participations(n, rng):
        ref = pp.SortedReference(v, take)
        m = ref.n
        dt = None if take is None else pp.to_gpu(take if n else np.zeros(1, np.uint8))
        ranks = [(-1, 0.0)] + [(-1, f) for f in FRACTIONS] + ([(0, 0.0), (m - 1, 0.0), (m // 3, 0.0)] if m else [(0, 0.0)])
        for k, (fixed, fraction) in enumerate(ranks):
            got = select(dv, dt, n, fixed, fraction, per_pass=(k == 0))
            what = (name, n, label, fixed, fraction)
            assert got["n"] == m and got["ticket"] == 0, what      # the elements that took part; the ticket back at zero
            assert got["bits"] == ref.bits(pp.rank_of(fixed, fraction, m)), (what, hex(got["bits"]))
            if k == 0:      # the lower median: the ticket behind every pass, and the four launches at once give the same state
                assert got["after"] == [0, 0, 0, 0], what
                again = select(dv, dt, n, fixed, fraction)
                assert (again["bits"], again["n"], again["k"], again["ticket"]) == (got["bits"], got["n"], got["k"], got["ticket"]), what
        if m:
            assert pp.rank_of(-1, FRACTIONS[-1], m) == 0 and int(m * FRACTIONS[-1]) == 0      # (keep == 0)


@pytest.mark.parametrize("n", [1, 257, 2049, 100_003])
def test_select_over_a_key_source(select, n):
    rng = np.random.default_rng(54 + n)
    keys = pp.fmix32(np.arange(n))
    for take in (None, (rng.random(n) < 0.4).astype(np.uint8)):
        mine = np.sort(keys if take is None else keys[take.astype(bool)])
        if mine.size == 0:
            continue
        dt = None if take is None else pp.to_gpu(take)
        for fixed, fraction in ((-1, 0.0), (-1, 1 / 8), (-1, 1.0), (0, 0.0)):
            got = select(None, dt, n, fixed, fraction, keys=True)
            assert got["n"] == mine.size and got["ticket"] == 0
            assert got["bits"] == int(mine[pp.rank_of(fixed, fraction, mine.size)]), (n, fixed, fraction)      # the key of that rank, as it stands


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_select_segment(n):
    rng = np.random.default_rng(55 + n)
    for name in VALUE_SETS:
        # three segments of one launch: every element, a random 40 %, and one none of whose elements take part
        v = np.concatenate([value_set(name, n, rng) for _ in range(3)])
        take = np.concatenate([np.ones(n, np.uint8), (rng.random(n) < 0.4).astype(np.uint8), np.zeros(n, np.uint8)])
        got = pp.run_select_segment(v, take, n, 3)
        assert (got == got[:, :1]).all(), name      # the same bits in every thread
        for seg in range(3):
            ref = pp.SortedReference(v[seg * n:(seg + 1) * n], take[seg * n:(seg + 1) * n])
            assert int(got[seg, 0]) == ref.bits(pp.rank_of(-1, 0.0, ref.n)), (name, n, seg, hex(int(got[seg, 0])))
        assert (got[2] == pp.QUIET_NAN).all()
        if n:
            assert np.array_equal(pp.run_select_segment(v[:n], None, n, 1)[0], got[0]), name      # no predicate: all take part


def test_hist_add():
    rng = np.random.default_rng(56)
    lanes = np.arange(64)
    every, nobody = np.ones(64, np.uint8), np.zeros(64, np.uint8)
    late = (lanes >= 9).astype(np.uint8)      # the first active lane is not lane 0
    cases = [(every, np.full(64, 200)), (every, lanes * 4 + 3), (late, np.where(lanes < 9, 77, 5)), (late, rng.integers(0, 256, 64)), (nobody, lanes),
             ((rng.random(64) < 0.5).astype(np.uint8), rng.integers(0, 4, 64)), ((lanes == 63).astype(np.uint8), np.full(64, 255)),
             (every, np.where(lanes % 2, 0, 255))]
    for ok, digit in cases:
        got = pp.run_hist_add(ok, digit)
        want = np.bincount(np.asarray(digit)[ok.astype(bool)], minlength=256)
        assert np.array_equal(got, want), (ok.tolist(), np.asarray(digit).tolist())
