// Exact order statistics of float32 arrays on the device, with no sort, no compaction and no host wait: the k-th smallest of the
// elements that pass a predicate evaluated in place (frame_stats.hip: the median of the edge magnitudes, the median rendered depth).
//
// A float goes to a 32-bit key whose unsigned order is the float order (sign bit flipped for values >= +0, every bit for negatives;
// NaN is outside the contract: torch.median propagates it, a key does not).  Four passes walk the key's bytes from the top: a pass
// counts, per value of its byte, the elements whose higher bytes equal the prefix found so far, picks the bucket that holds rank k,
// and hands prefix | bucket and k - (elements below the bucket) to the next pass.  After the fourth the prefix IS the key of the
// answer: the same 32 bits a full sort would put at position k, whatever order the elements were counted in.
//   * 8-bit digits: 256 counters are one per thread of a 256-thread workgroup (1 KB of LDS), and the bucket choice is one block scan.
//   * Counters are 32-bit: a bucket may hold every element of an image (the exact zeros of a masked magnitude image do).
//   * One LDS atomic per lane serialises when many lanes of a wave hit one counter, which is the common case here (equal values, and
//     in the later passes most survivors share the byte).  hist_add() peels the digit of the wave's first active lane: one atomic with
//     the count of the lanes that share it, single atomics for the rest.
// Two forms:
//   select_pass_kernel<Src>   many workgroups over one array; one launch per pass, all enqueued at once.  Every workgroup adds its LDS
//                             counters to the pass' 256 global counters (integer atomics: order-free), and the LAST workgroup to arrive
//                             (an agent-scope ticket, as in depth_align.hip / pnp.hip) picks the bucket.  No workgroup waits on another.
//   select_segment<Src>       one workgroup, one short segment, the four passes in a loop (the replica rule: 1024 blocks of an image).
// A source is a struct with `__device__ bool get(int64_t i, float &v) const`: element i's value, and whether it takes part.  A source
// with `__device__ bool key(int64_t i, uint32_t &k) const` instead hands out the 32-bit key itself (seeding.hip: a hash of the pixel
// index); the answer is then the key of that rank, st->prefix as it stands.
// The rank is a SelectRank: a fixed one, or a function of the number n that pass 0 finds taking part -- the lower median, or the last
// of the (int64)((double)n * fraction) smallest.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "device_utils.hpp"

namespace lvdgs {

constexpr int SEL_THREADS = 256;          // = the number of digit values
constexpr int SEL_PASSES = 4;
constexpr int SEL_MAX_BLOCKS = 512;
constexpr int SEL_ITEMS_PER_THREAD = 8;   // elements per thread a workgroup is sized for (grid-stride beyond SEL_MAX_BLOCKS)
constexpr uint32_t SEL_QUIET_NAN = 0x7fc00000u;

// Zeroed by the caller (hipMemsetAsync) in front of the first pass of every selection.
struct SelectState {
    uint32_t hist[SEL_PASSES][SEL_THREADS];
    uint32_t prefix;     // the key's bytes found so far (the key itself after the last pass)
    uint32_t k;          // the rank looked for among the elements that share the prefix
    uint32_t n;          // elements that took part (set by pass 0)
    uint32_t ticket;     // zero between launches (the last workgroup resets it)
    uint32_t pad[60];
};
static_assert(sizeof(SelectState) % 256 == 0, "the state is followed by 256-byte aligned buffers");

__host__ __device__ inline uint32_t select_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__host__ __device__ inline uint32_t select_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }
// the selected value's bits: a quiet NaN when nothing took part (torch.median of an empty tensor)
__device__ __forceinline__ uint32_t select_result_bits(uint32_t n, uint32_t prefix) { return n ? select_unkey(prefix) : SEL_QUIET_NAN; }
// torch.median's rank among n elements: the lower median
__host__ __device__ inline uint32_t lower_median_rank(uint32_t n) { return n ? (n - 1) / 2 : 0; }

// The rank looked for among the n elements that take part; n is known when pass 0's last workgroup picks its bucket.
struct SelectRank {
    int64_t fixed;      // >= 0: this rank (the caller guarantees fixed < n, or accepts the NaN of n == 0)
    double fraction;    // fixed < 0.  0: the lower median; in (0, 1]: rank keep - 1 with keep = (int64)((double)n * fraction), rank 0 when keep == 0
    __host__ __device__ uint32_t of(uint32_t n) const {
        if (fixed >= 0) return (uint32_t)fixed;
        if (fraction == 0.0) return lower_median_rank(n);
        const int64_t keep = (int64_t)((double)n * fraction);
        return keep > 0 ? (uint32_t)(keep - 1) : 0u;
    }
};
__host__ __device__ inline SelectRank select_rank(int64_t k_fixed) { return SelectRank{k_fixed, 0.0}; }   // k_fixed < 0: the lower median

template <class Src, class = void> struct yields_key : std::false_type {};
template <class Src> struct yields_key<Src, std::void_t<decltype(&Src::key)>> : std::true_type {};
// Element i's key, and whether it takes part.
template <class Src>
__device__ __forceinline__ bool source_key(const Src &src, int64_t i, uint32_t &key) {
    if constexpr (yields_key<Src>::value) {
        return src.key(i, key);
    } else {
        float v = 0.f;
        const bool in = src.get(i, v);
        key = select_key(__float_as_uint(v));
        return in;
    }
}

inline int select_blocks(int64_t n) {
    const int64_t b = (n + (int64_t)SEL_THREADS * SEL_ITEMS_PER_THREAD - 1) / ((int64_t)SEL_THREADS * SEL_ITEMS_PER_THREAD);
    return (int)(b < 1 ? 1 : (b > SEL_MAX_BLOCKS ? SEL_MAX_BLOCKS : b));
}

// One element per lane into the LDS counters.  Called by whole waves (`ok` says which lanes count).
__device__ __forceinline__ void hist_add(uint32_t *hist, bool ok, uint32_t digit) {
    const unsigned long long active = __ballot(ok);
    if (active == 0ull) return;
    const int first = __ffsll((long long)active) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)digit, first, WAVE);
    const unsigned long long same = __ballot(ok && digit == d0);
    const int lane = threadIdx.x % WAVE;
    if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
    if (ok && digit != d0) atomicAdd(&hist[digit], 1u);
}

// The bucket that holds rank k among 256 counts, one count per thread.  from_total: k is rank.of(the counts' total) (pass 0).
// -> true in the one thread whose bucket it is (none when the total is zero); k_in_bucket: the rank inside it; total: in every thread.
// sh: SCAN_WORDS words of LDS for the one workgroup scan (two barriers, none needed in front of the next call: device_utils.hpp).
__device__ __forceinline__ bool pick_bucket(uint32_t count, bool from_total, const SelectRank &rank, uint32_t k, uint32_t *sh, uint32_t *k_in_bucket,
                                            uint32_t *total) {
    const uint32_t excl = scan_workgroup<SEL_THREADS>(count, sh, total);
    if (from_total) k = rank.of(*total);
    *k_in_bucket = k - excl;
    return count > 0 && excl <= k && k - excl < count;
}

// Pass `pass` (0: the key's top byte) of a selection over src's elements 0 .. n - 1, for the rank `rank` gives.
template <class Src>
__global__ void __launch_bounds__(SEL_THREADS) select_pass_kernel(Src src, int64_t n, SelectState *st, int pass, SelectRank rank) {
    __shared__ uint32_t hist[SEL_THREADS];
    __shared__ uint32_t sh[SCAN_WORDS];
    __shared__ int s_last;
    if (pass > 0 && st->n == 0) return;   // uniform over the launch: nothing took part, the result is NaN
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t prefix = st->prefix;   // written by the pass before (kernel boundaries order it)
    const int shift = 24 - 8 * pass;
    const uint32_t high = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    const int64_t stride = (int64_t)gridDim.x * SEL_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * SEL_THREADS; base < n; base += stride) {   // (base is uniform: whole waves reach hist_add)
        const int64_t i = base + threadIdx.x;
        uint32_t key = 0;
        const bool in = i < n && source_key(src, i, key);
        hist_add(hist, in && (key & high) == prefix, (key >> shift) & 255u);
    }
    __syncthreads();
    const uint32_t mine = hist[threadIdx.x];
    if (mine) __hip_atomic_fetch_add(&st->hist[pass][threadIdx.x], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every wave's atomics have landed, then one release and the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup: the bucket of rank k ----
    const uint32_t count = __hip_atomic_load(&st->hist[pass][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t k = pass == 0 ? 0u : st->k;
    uint32_t k_in = 0, total = 0;
    const bool owner = pick_bucket(count, pass == 0, rank, k, sh, &k_in, &total);
    if (owner) {
        st->prefix = prefix | ((uint32_t)threadIdx.x << shift);
        st->k = k_in;
    }
    if (threadIdx.x == 0) {
        if (pass == 0) st->n = total;
        st->ticket = 0;   // ready for the next pass (kernel boundaries order it)
    }
}

// The four passes over one array, enqueued at once.  The caller has zeroed *st on the stream in front of them.
template <class Src>
int launch_select(const Src &src, int64_t n, SelectState *st, SelectRank rank, const char *name, hipStream_t s) {
    ProfScope ps(name, s);
    const int blocks = select_blocks(n);
    for (int pass = 0; pass < SEL_PASSES; pass++) {
        if (int e = launch_checked(name, 0, s, select_pass_kernel<Src>, dim3(blocks), dim3(SEL_THREADS), 0, src, n, st, pass, rank)) return e;
    }
    return LVDGS_OK;
}
template <class Src>
int launch_select(const Src &src, int64_t n, SelectState *st, int64_t k_fixed, const char *name, hipStream_t s) {
    return launch_select(src, n, st, select_rank(k_fixed), name, s);
}

// One workgroup, one segment of n elements: the bits of the lower median of those that take part (quiet NaN: none), in every thread.
// hist: SEL_THREADS words of LDS, sh: SCAN_WORDS + 2 words.  Called by all SEL_THREADS threads.
template <class Src>
__device__ __forceinline__ uint32_t select_segment(const Src &src, int n, uint32_t *hist, uint32_t *sh) {
    const SelectRank median = select_rank(-1);
    uint32_t prefix = 0, k = 0, taking_part = 0;
    for (int pass = 0; pass < SEL_PASSES; pass++) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        const int shift = 24 - 8 * pass;
        const uint32_t high = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        for (int base = 0; base < n; base += SEL_THREADS) {
            const int i = base + threadIdx.x;
            float v = 0.f;
            const bool in = i < n && src.get(i, v);
            const uint32_t key = select_key(__float_as_uint(v));
            hist_add(hist, in && (key & high) == prefix, (key >> shift) & 255u);
        }
        __syncthreads();
        uint32_t k_in = 0, total = 0;
        const bool owner = pick_bucket(hist[threadIdx.x], pass == 0, median, k, sh, &k_in, &total);
        if (pass == 0) taking_part = total;
        if (taking_part == 0) return SEL_QUIET_NAN;   // uniform
        if (owner) {
            sh[SCAN_WORDS] = prefix | ((uint32_t)threadIdx.x << shift);
            sh[SCAN_WORDS + 1] = k_in;
        }
        __syncthreads();
        prefix = sh[SCAN_WORDS];
        k = sh[SCAN_WORDS + 1];
        __syncthreads();
    }
    return select_unkey(prefix);
}

}  // namespace lvdgs
