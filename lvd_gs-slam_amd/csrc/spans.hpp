// The span scan: an ordered compaction (or prefix) of n elements with no atomic that decides a position ("Span scan").
//   1. Every workgroup owns one contiguous SPAN of elements (span_range) and leaves a count, or a sum, per span.
//   2. One workgroup turns the span counts into what lies in front of each span (scan_span_counts).
//   3. A write pass walks each span again in tiles of THREADS elements (TileWalk): an element's position is what lies in front of
//      its span + what lies in front of its tile + the exclusive prefix inside the tile.
// Integer decisions only: two calls give the same bytes, and no result depends on how the elements are cut into spans.
// The geometry compiles as plain C++ too (map_edit_host.hpp is part of a stand-alone host program); the device part needs hipcc.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include "device_utils.hpp"
#define LVDGS_SPANS_HD __host__ __device__
#else
#define LVDGS_SPANS_HD
#endif

namespace lvdgs {

// Elements per span when n (0 .. 2^31 - 1) elements go to `blocks` >= 1 workgroups of `threads` threads: the smallest multiple of
// `threads` with blocks * span >= n, at least `threads`.
LVDGS_SPANS_HD inline uint32_t span_length(uint32_t n, uint32_t blocks, uint32_t threads) {
    const uint64_t per = (uint64_t)blocks * threads;
    const uint64_t tiles = ((uint64_t)n + per - 1) / per;
    return (uint32_t)(tiles ? tiles : 1) * threads;
}

// The spans of n (0 .. 2^31 - 1) elements: at most `cap` of them, none shorter than min_span (a multiple of `threads`) but the last,
// and as many as are non-empty -- (blocks - 1) * span < n <= blocks * span; n == 0 gives no span.
struct Spans { int blocks; uint32_t span; };
inline Spans make_spans(int64_t n, int threads, int cap, uint32_t min_span) {
    Spans s{0, min_span};
    if (n <= 0) return s;
    const uint32_t fit = span_length((uint32_t)n, (uint32_t)cap, (uint32_t)threads);
    if (fit > s.span) s.span = fit;
    s.blocks = (int)((n + s.span - 1) / s.span);
    return s;
}

#ifdef __HIPCC__

// [begin, end) of workgroup `block`'s span; begin is clamped to n, so a workgroup past the end owns nothing.  I: the type the kernel
// indexes with (uint32_t keeps 32-bit scalar and address arithmetic).  block * span must fit 32 bits: it does for every grid of
// make_spans and for a fixed grid over span_length's spans, where blocks * span < n + blocks * threads, and n <= 2^31 - 1.
template <typename I>
struct SpanRange { I begin, end; };
template <typename I>
__device__ __forceinline__ SpanRange<I> span_range(I n, I span, uint32_t block) {
    const I first = (I)block * span;
    const I begin = first < n ? first : n;
    return {begin, n - begin < span ? n : begin + span};
}

// Step 2, called by ALL threads of ONE workgroup of THREADS threads: reads counts[j * stride] for j < blocks, writes what lies in
// front of span j to before[j * stride] (in place when before == counts) and returns the total, in every thread.  Rounds of THREADS
// spans, the last one padded with zeros, with a carry of type C across the rounds.  T is the type a round is scanned in: the sum of
// the THREADS counts of one round must fit T; the total need only fit C.  sh: SCAN_WORDS of LDS; calls may follow each other on it.
// (T, C) in use and tested: (uint32_t, uint32_t), (uint32_t, unsigned long long), (unsigned long long, unsigned long long).
template <int THREADS, typename T, typename C>
__device__ __forceinline__ C scan_span_counts(const T *counts, C *before, int blocks, int stride, T *sh) {
    C carry = 0;
    // The counts of the round after are loaded in front of a round's scan and waited for behind it, in front of the round's store:
    // neither the load nor the store before it is waited for with nothing to do (the empty asm pins where the wait stands).
    T next = (int)threadIdx.x < blocks ? counts[(int)threadIdx.x * stride] : (T)0;
    asm volatile("" : "+v"(next));
    for (int base = 0; base < blocks; base += THREADS) {   // (uniform: every thread reaches the scan)
        const int j = base + (int)threadIdx.x;
        const T c = next;
        next = j + THREADS < blocks ? counts[(j + THREADS) * stride] : (T)0;   // (not yet written: the stores end at j)
        T total = 0;
        const T excl = scan_workgroup<THREADS>(c, sh, &total);
        asm volatile("" : "+v"(next));
        if (j < blocks) before[j * stride] = carry + excl;
        carry += total;
    }
    return carry;
}

// Step 3: the running position of a workgroup that walks its span in tiles of THREADS elements.  `row` starts as what lies in front of
// the span (step 2's word for it).  place(v) is called once a tile by EVERY thread of the workgroup -- the tile loop's condition must
// be uniform, a thread past the span's end passes 0 -- and returns the position of this thread's element, then moves `row` past the
// tile.  T, C and sh as for scan_span_counts: a tile's sum must fit T.  (T, C) in use and tested: those of scan_span_counts and
// (uint32_t, int64_t).
template <int THREADS, typename T, typename C = T>
struct TileWalk {
    C row;
    __device__ __forceinline__ C place(T v, T *sh) {
        T total = 0;
        const T excl = scan_workgroup<THREADS>(v, sh, &total);
        const C at = row + excl;
        row += total;
        return at;
    }
};

#endif  // __HIPCC__

}  // namespace lvdgs
