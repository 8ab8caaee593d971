// Test-only kernels over the shared primitives (csrc/device_utils.hpp, spans.hpp, select.hpp): each probe calls ONE primitive the way
// the product kernels do and stores what every thread got, so that tests/test_gpu_primitives.py can compare it with a NumPy reference
// (tests/primitives_probe.py).  Built by csrc/Makefile into liblvdgs_probe.so with the product's flags; the headers are included, not
// copied.  Not part of the product library: nothing here is declared in include/lvdgs.h.
//
// Rules of this file:
//   * A host entry point validates everything before it launches (pointers, counts, the instantiated workgroup sizes, and that every
//     buffer holds what the probe will read and write) and returns LVDGS_E_INVALID otherwise: a mistake in a test launches nothing.
//   * A value probe stores at the thread's own index only.  The one probe that stores at a computed position (the TileWalk compaction)
//     brings the position into the output's capacity before it indexes.
#include "../../lvd_gs-slam_amd/csrc/select.hpp"
#include "../../lvd_gs-slam_amd/csrc/spans.hpp"

namespace lvdgs {
namespace {

using u64 = unsigned long long;

#define PROBE_REFUSE(...) do { set_error(__VA_ARGS__); return LVDGS_E_INVALID; } while (0)

bool wave_multiple(int threads) { return threads == 64 || threads == 256 || threads == 1024; }

// ---------------------------------------------------------------- wave level
// in: `in_planes` planes of n = threads * blocks elements, out: `out_planes` planes; thread g reads and writes element g of a plane.
enum WaveOp : int {
    W_SUM_I32, W_SUM_U32, W_SUM_U64, W_SUM_F32, W_SUM_F64, W_SUM_LANE63, W_MAX_I32, W_MAX_U32, W_MAX_F32, W_MIN_F32,
    W_SCAN_U32, W_SCAN_I32, W_SCAN_DPP, W_FOLD32, W_FOLD16, W_ROT1, W_ROT4, W_ROT8, W_ROT15, W_DPP_SHR1, W_DPP_SHR8,
    W_ROW_SUMS3, W_WRITE_LANE, W_OPS
};
struct WaveShape { int in_planes, in_bytes, out_planes, out_bytes; };
constexpr WaveShape WAVE_SHAPES[W_OPS] = {
    {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 8, 1, 8}, {1, 4, 1, 4}, {1, 8, 1, 8}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4},
    {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {2, 4, 1, 4}, {2, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4}, {1, 4, 1, 4},
    {3, 4, 6, 4}, {1, 4, 1, 4},
};

template <int OP>
__global__ void wave_probe_kernel(const void *in, void *out, int n, int a0, int a1) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;   // (the grid is n threads exactly)
    const float *fin = (const float *)in;
    float *fout = (float *)out;
    if constexpr (OP == W_SUM_I32) ((int *)out)[g] = wave_sum(((const int *)in)[g]);
    else if constexpr (OP == W_SUM_U32) ((uint32_t *)out)[g] = wave_sum(((const uint32_t *)in)[g]);
    else if constexpr (OP == W_SUM_U64) ((u64 *)out)[g] = wave_sum(((const u64 *)in)[g]);
    else if constexpr (OP == W_SUM_F32) fout[g] = wave_sum(fin[g]);
    else if constexpr (OP == W_SUM_F64) ((double *)out)[g] = wave_sum(((const double *)in)[g]);
    else if constexpr (OP == W_SUM_LANE63) fout[g] = wave_sum_to_lane63(fin[g]);
    else if constexpr (OP == W_MAX_I32) ((int *)out)[g] = wave_max(((const int *)in)[g]);
    else if constexpr (OP == W_MAX_U32) ((uint32_t *)out)[g] = wave_max(((const uint32_t *)in)[g]);
    else if constexpr (OP == W_MAX_F32) fout[g] = wave_max(fin[g]);
    else if constexpr (OP == W_MIN_F32) fout[g] = wave_min(fin[g]);
    else if constexpr (OP == W_SCAN_U32) ((uint32_t *)out)[g] = wave_inclusive_scan(((const uint32_t *)in)[g]);
    else if constexpr (OP == W_SCAN_I32) ((int *)out)[g] = wave_inclusive_scan(((const int *)in)[g]);
    else if constexpr (OP == W_SCAN_DPP) ((uint32_t *)out)[g] = wave_inclusive_scan_dpp(((const uint32_t *)in)[g]);
    else if constexpr (OP == W_FOLD32) fout[g] = fold32(fin[g], fin[n + g]);
    else if constexpr (OP == W_FOLD16) fout[g] = fold16(fin[g], fin[n + g]);
    else if constexpr (OP == W_ROT1) fout[g] = row_rotate<1>(fin[g]);
    else if constexpr (OP == W_ROT4) fout[g] = row_rotate<4>(fin[g]);
    else if constexpr (OP == W_ROT8) fout[g] = row_rotate<8>(fin[g]);
    else if constexpr (OP == W_ROT15) fout[g] = row_rotate<15>(fin[g]);
    else if constexpr (OP == W_DPP_SHR1) fout[g] = dpp_or_zero<0x111>(fin[g]);
    else if constexpr (OP == W_DPP_SHR8) fout[g] = dpp_or_zero<0x118>(fin[g]);
    else if constexpr (OP == W_ROW_SUMS3) {
        // twice, each time with a VALU write of the three registers right in front of the asm block: the hazard its leading s_nop guards
        const float s0 = __int_as_float(a0), s1 = __int_as_float(a1);
        float x = fin[g] * s0, y = fin[n + g] * s0, z = fin[2 * n + g] * s0;
        row_sums3(x, y, z);
        fout[g] = x; fout[n + g] = y; fout[2 * n + g] = z;
        x *= s1; y *= s1; z *= s1;
        row_sums3(x, y, z);
        fout[3 * n + g] = x; fout[4 * n + g] = y; fout[5 * n + g] = z;
    } else if constexpr (OP == W_WRITE_LANE) ((int *)out)[g] = write_lane(((const int *)in)[g], a0, a1);
}

template <int OP>
int launch_wave_probe(int op, int threads, int blocks, const void *in, void *out, int a0, int a1, hipStream_t s) {
    if constexpr (OP < W_OPS) {
        if (op != OP) return launch_wave_probe<OP + 1>(op, threads, blocks, in, out, a0, a1, s);
        if (int e = launch_checked("probe wave", 0, s, wave_probe_kernel<OP>, dim3(blocks), dim3(threads), 0, in, out, threads * blocks, a0, a1)) return e;
        return LVDGS_OK;
    } else {
        PROBE_REFUSE("probe wave: no op %d", op);
    }
}

// mask_set_bit / mask_clear_bit on a wave-uniform mask and bit (kernel arguments): one wave, every lane stores what it got
__global__ void mask_bit_kernel(int set, u64 mask, int bit, u64 *out) {
    const uint64_t m = set ? mask_set_bit((uint64_t)mask, bit) : mask_clear_bit((uint64_t)mask, bit);
    out[threadIdx.x] = (u64)m;
}

// ---------------------------------------------------------------- workgroup level
// One scan: the exclusive prefix and the total, per thread.
template <int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) scan_basic_kernel(const T *in, T *out, int n) {
    __shared__ T s_scan[SCAN_WORDS];
    const int g = blockIdx.x * THREADS + threadIdx.x;
    T total = 0;
    const T excl = scan_workgroup<THREADS>(in[g], s_scan, &total);
    out[g] = excl;
    out[n + g] = total;
}

// The barrier contracts of scan_workgroup (device_utils.hpp), with NO barrier of the probe's own anywhere:
//   in planes: 0 first values, 1 the word a thread leaves in LDS before the first call, 2 second values, 3.. one per loop trip
//   out planes: 0 1 first call (exclusive, total); 2 the word of thread (t + 64) % THREADS, read behind the first call;
//               3 4 the second call, back to back on the same s_scan; 5 + 2r, 6 + 2r trip r of a loop with a uniform trip count
template <int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) scan_contract_kernel(const T *in, T *out, int n, int trips) {
    __shared__ T s_scan[SCAN_WORDS];
    __shared__ T s_word[THREADS];
    const int t = threadIdx.x, g = blockIdx.x * THREADS + t;
    s_word[t] = in[n + g];
    T total = 0;
    T excl = scan_workgroup<THREADS>(in[g], s_scan, &total);
    out[g] = excl;
    out[n + g] = total;
    out[2 * n + g] = s_word[(t + 64) % THREADS];
    excl = scan_workgroup<THREADS>(in[2 * n + g], s_scan, &total);
    out[3 * n + g] = excl;
    out[4 * n + g] = total;
    for (int r = 0; r < trips; r++) {   // (uniform: a kernel argument)
        excl = scan_workgroup<THREADS>(in[(3 + r) * n + g], s_scan, &total);
        out[(5 + 2 * r) * n + g] = excl;
        out[(6 + 2 * r) * n + g] = total;
    }
}
constexpr int CONTRACT_MAX_TRIPS = 3;

template <int THREADS, typename T>
int launch_scan_probe(bool contract, int blocks, const void *in, void *out, int trips, hipStream_t s) {
    const int n = THREADS * blocks;
    if (contract) return launch_checked("probe scan", 0, s, scan_contract_kernel<THREADS, T>, dim3(blocks), dim3(THREADS), 0, (const T *)in, (T *)out, n, trips);
    return launch_checked("probe scan", 0, s, scan_basic_kernel<THREADS, T>, dim3(blocks), dim3(THREADS), 0, (const T *)in, (T *)out, n);
}
template <typename T>
int launch_scan_probe_t(int threads, bool contract, int blocks, const void *in, void *out, int trips, hipStream_t s) {
    if (threads == 64) return launch_scan_probe<64, T>(contract, blocks, in, out, trips, s);
    if (threads == 256) return launch_scan_probe<256, T>(contract, blocks, in, out, trips, s);
    return launch_scan_probe<1024, T>(contract, blocks, in, out, trips, s);
}

// block_sum twice, back to back on one s: planes 0 and 1 in, planes 0 and 1 out
template <int WAVES, typename T>
__global__ void __launch_bounds__(64 * WAVES) block_sum_kernel(const T *in, T *out, int n) {
    __shared__ T s[WAVES];
    const int g = blockIdx.x * 64 * WAVES + threadIdx.x;
    const T a = block_sum<WAVES>(in[g], s);
    const T b = block_sum<WAVES>(in[n + g], s);
    out[g] = a;
    out[n + g] = b;
}
template <int WAVES, typename T>
int launch_block_sum(int blocks, const void *in, void *out, hipStream_t s) {
    if (int e = launch_checked("probe block_sum", 0, s, block_sum_kernel<WAVES, T>, dim3(blocks), dim3(64 * WAVES), 0, (const T *)in, (T *)out, 64 * WAVES * blocks)) return e;
    return LVDGS_OK;
}

// ---------------------------------------------------------------- spans
__global__ void span_range_kernel(uint32_t n, uint32_t span, uint32_t *out) {
    const SpanRange<uint32_t> r = span_range<uint32_t>(n, span, blockIdx.x);
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = r.begin; out[2 * blockIdx.x + 1] = r.end; }
}

// scan_span_counts by one workgroup; totals[t]: what thread t got back
template <int THREADS, typename T, typename C>
__global__ void __launch_bounds__(THREADS) span_counts_kernel(const T *counts, C *before, int blocks, int stride, C *totals) {
    __shared__ T sh[SCAN_WORDS];
    totals[threadIdx.x] = scan_span_counts<THREADS>(counts, before, blocks, stride, sh);
}
template <int THREADS, typename T, typename C>
int launch_span_counts(const void *counts, void *before, int blocks, int stride, void *totals, hipStream_t s) {
    if (int e = launch_checked("probe scan_span_counts", 0, s, span_counts_kernel<THREADS, T, C>, dim3(1), dim3(THREADS), 0, (const T *)counts, (C *)before, blocks, stride, (C *)totals)) return e;
    return LVDGS_OK;
}

// The ordered compaction of the elements with keep[i] != 0, as seeding.hip does it: count pass, span scan, write pass.
constexpr int CP_THREADS = 256;
template <typename T>
__global__ void __launch_bounds__(CP_THREADS) compact_count_kernel(const uint8_t *keep, uint32_t n, uint32_t span, T *counts) {
    __shared__ T sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range<uint32_t>(n, span, blockIdx.x);
    T mine = 0;
    for (uint32_t i = r.begin + threadIdx.x; i < r.end; i += CP_THREADS) mine += keep[i] != 0;
    T total = 0;
    scan_workgroup<CP_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
template <typename T, typename B>
__global__ void __launch_bounds__(CP_THREADS) compact_scan_kernel(const T *counts, B *before, int blocks, u64 *total_out) {
    __shared__ T sh[SCAN_WORDS];
    const B total = scan_span_counts<CP_THREADS>(counts, before, blocks, 1, sh);
    if (threadIdx.x == 0) *total_out = (u64)total;
}
// T, C: TileWalk's; B: the type of the scanned words.  out_index[p] = the p-th kept element, out_row[p] = the row TileWalk gave it
// (row0 + p when all is well).  p is brought into [0, capacity) before it indexes.
template <typename T, typename C, typename B>
__global__ void __launch_bounds__(CP_THREADS) compact_write_kernel(const uint8_t *keep, uint32_t n, uint32_t span, const B *before, u64 row0, uint32_t *out_index,
                                                                   u64 *out_row, long long capacity) {
    __shared__ T sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range<uint32_t>(n, span, blockIdx.x);
    TileWalk<CP_THREADS, T, C> walk{(C)(row0 + (u64)before[blockIdx.x])};
    for (uint32_t base = r.begin; base < r.end; base += CP_THREADS) {   // (uniform)
        const uint32_t i = base + threadIdx.x;
        const bool sel = i < r.end && keep[i] != 0;
        const C at = walk.place(sel ? (T)1 : (T)0, sh);
        if (!sel || capacity <= 0) continue;
        u64 p = (u64)at - (u64)(C)row0;
        if (p >= (u64)capacity) p = (u64)capacity - 1;   // (never with a correct walk: the host sizes the output for every element)
        out_index[p] = i;
        out_row[p] = (u64)at;
    }
}
template <typename T, typename C, typename B>
int launch_compact(const uint8_t *keep, uint32_t n, int blocks, u64 row0, void *counts, void *before, uint32_t *out_index, u64 *out_row, long long capacity,
                   u64 *total_out, hipStream_t s) {
    const uint32_t span = span_length(n, (uint32_t)blocks, CP_THREADS);
    if (int e = launch_checked("probe compact count", 0, s, compact_count_kernel<T>, dim3(blocks), dim3(CP_THREADS), 0, keep, n, span, (T *)counts)) return e;
    if (int e = launch_checked("probe compact scan", 0, s, compact_scan_kernel<T, B>, dim3(1), dim3(CP_THREADS), 0, (const T *)counts, (B *)before, blocks, total_out)) return e;
    if (int e = launch_checked("probe compact write", 0, s, compact_write_kernel<T, C, B>, dim3(blocks), dim3(CP_THREADS), 0, keep, n, span, (const B *)before, row0,
            out_index, out_row, capacity)) return e;
    return LVDGS_OK;
}

// ---------------------------------------------------------------- select
struct ProbeSource {   // element i's value; take null: every element takes part
    const float *v;
    const uint8_t *take;
    __device__ __forceinline__ bool get(int64_t i, float &x) const { x = v[i]; return !take || take[i] != 0; }
};
struct ProbeKeySource {   // the key is a hash of the index (what seeding.hip's source does)
    const uint8_t *take;
    __device__ __forceinline__ bool key(int64_t i, uint32_t &k) const { k = fmix32((uint32_t)i); return !take || take[i] != 0; }
};
enum : int { SP_RESULT = 0, SP_N = 1, SP_TICKET = 2, SP_K = 3, SP_TICKET_AFTER_PASS = 4, SP_WORDS = 8 };
__global__ void select_record_ticket_kernel(const SelectState *st, uint32_t *out, int slot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[slot] = st->ticket;
}
__global__ void select_finish_kernel(const SelectState *st, uint32_t *out, int keys) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[SP_RESULT] = keys ? st->prefix : select_result_bits(st->n, st->prefix);
    out[SP_N] = st->n;
    out[SP_TICKET] = st->ticket;
    out[SP_K] = st->k;
}
template <class Src>
int run_select(const Src &src, int64_t n, SelectState *st, SelectRank rank, uint32_t *out, bool per_pass, bool keys, hipStream_t s) {
    if (int e = check_hip(hipMemsetAsync(st, 0, sizeof(SelectState), s), "probe select: clearing the state")) return e;
    if (int e = check_hip(hipMemsetAsync(out, 0xff, SP_WORDS * sizeof(uint32_t), s), "probe select: clearing the report")) return e;
    if (!per_pass) {
        if (int e = launch_select(src, n, st, rank, "probe_select", s)) return e;
    } else {   // launch_select's launches, with the ticket read between them
        const int blocks = select_blocks(n);
        for (int pass = 0; pass < SEL_PASSES; pass++) {
            if (int e = launch_checked("probe select pass", 0, s, select_pass_kernel<Src>, dim3(blocks), dim3(SEL_THREADS), 0, src, n, st, pass, rank)) return e;
            if (int e = launch_checked("probe select ticket", 0, s, select_record_ticket_kernel, dim3(1), dim3(WAVE), 0, st, out, SP_TICKET_AFTER_PASS + pass)) return e;
        }
    }
    if (int e = launch_checked("probe select finish", 0, s, select_finish_kernel, dim3(1), dim3(WAVE), 0, st, out, keys ? 1 : 0)) return e;
    return LVDGS_OK;
}

// select_segment: workgroup b takes elements [b * n, (b + 1) * n); every thread stores the bits it got
__global__ void __launch_bounds__(SEL_THREADS) select_segment_kernel(const float *v, const uint8_t *take, int n, uint32_t *out) {
    __shared__ uint32_t hist[SEL_THREADS];
    __shared__ uint32_t sh[SCAN_WORDS + 2];
    const int64_t first = (int64_t)blockIdx.x * n;
    const ProbeSource src{v + first, take ? take + first : nullptr};
    out[blockIdx.x * SEL_THREADS + threadIdx.x] = select_segment(src, n, hist, sh);
}

// hist_add by one wave: lane l counts digit[l] & 255 when ok[l]
__global__ void __launch_bounds__(WAVE) hist_add_kernel(const uint8_t *ok, const uint32_t *digit, uint32_t *out) {
    __shared__ uint32_t hist[SEL_THREADS];
    for (int j = threadIdx.x; j < SEL_THREADS; j += WAVE) hist[j] = 0;
    __syncthreads();
    hist_add(hist, ok[threadIdx.x] != 0, digit[threadIdx.x] & 255u);
    __syncthreads();
    for (int j = threadIdx.x; j < SEL_THREADS; j += WAVE) out[j] = hist[j];
}

constexpr int PROBE_MAX_BLOCKS = 4096;

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

// ---- host functions (no device) ----
uint32_t lvdgs_probe_span_length(uint32_t n, uint32_t blocks, uint32_t threads) { return span_length(n, blocks, threads); }
void lvdgs_probe_make_spans(int64_t n, int threads, int cap, uint32_t min_span, int *blocks, uint32_t *span) {
    const Spans s = make_spans(n, threads, cap, min_span);
    if (blocks) *blocks = s.blocks;
    if (span) *span = s.span;
}
uint32_t lvdgs_probe_select_key(uint32_t bits) { return select_key(bits); }
uint32_t lvdgs_probe_select_unkey(uint32_t key) { return select_unkey(key); }
// keys[i] = select_key(bits[i]), back[i] = select_unkey(keys[i])
int lvdgs_probe_select_keys(const uint32_t *bits, uint32_t *keys, uint32_t *back, int64_t n) {
    if (!bits || !keys || !back || n < 0) PROBE_REFUSE("probe select_keys: NULL array or negative count");
    for (int64_t i = 0; i < n; i++) { keys[i] = select_key(bits[i]); back[i] = select_unkey(keys[i]); }
    return LVDGS_OK;
}
uint32_t lvdgs_probe_lower_median_rank(uint32_t n) { return lower_median_rank(n); }
uint32_t lvdgs_probe_select_rank_of(int64_t fixed, double fraction, uint32_t n) { return SelectRank{fixed, fraction}.of(n); }
int lvdgs_probe_select_blocks(int64_t n) { return select_blocks(n); }
size_t lvdgs_probe_select_state_bytes(void) { return sizeof(SelectState); }
int lvdgs_probe_select_report_words(void) { return SP_WORDS; }

// ---- device probes ----
int lvdgs_probe_wave(int op, int threads, int blocks, const void *in, size_t in_bytes, void *out, size_t out_bytes, int a0, int a1, void *stream) {
    if (op < 0 || op >= W_OPS) PROBE_REFUSE("probe wave: no op %d", op);
    if (!wave_multiple(threads) || blocks < 1 || blocks > PROBE_MAX_BLOCKS) PROBE_REFUSE("probe wave: %d threads x %d workgroups", threads, blocks);
    if (!in || !out) PROBE_REFUSE("probe wave: in / out is NULL");
    const WaveShape sh = WAVE_SHAPES[op];
    const size_t n = (size_t)threads * blocks;
    if (in_bytes < n * sh.in_planes * sh.in_bytes || out_bytes < n * sh.out_planes * sh.out_bytes)
        PROBE_REFUSE("probe wave: op %d needs %zu bytes in and %zu out", op, n * sh.in_planes * sh.in_bytes, n * sh.out_planes * sh.out_bytes);
    if (op == W_WRITE_LANE && (a1 < 0 || a1 > 63)) PROBE_REFUSE("probe wave: lane %d", a1);
    return launch_wave_probe<0>(op, threads, blocks, in, out, a0, a1, (hipStream_t)stream);
}

int lvdgs_probe_mask_bit(int set, uint64_t mask, int bit, uint64_t *out, size_t out_bytes, void *stream) {
    if (!out || out_bytes < WAVE * sizeof(uint64_t)) PROBE_REFUSE("probe mask bit: out is NULL or holds fewer than 64 words");
    if (bit < 0 || bit > 63) PROBE_REFUSE("probe mask bit: bit %d", bit);
    hipStream_t s = (hipStream_t)stream;
    if (int e = launch_checked("probe mask bit", 0, s, mask_bit_kernel, dim3(1), dim3(WAVE), 0, set ? 1 : 0, (u64)mask, bit, (u64 *)out)) return e;
    return LVDGS_OK;
}

// dtype: 0 uint32_t, 1 int, 2 unsigned long long.  contract: 0 one scan (1 plane in, 2 out); 1 the contract probe (3 + trips planes in,
// 5 + 2 trips out)
int lvdgs_probe_scan(int contract, int dtype, int threads, int blocks, const void *in, size_t in_bytes, void *out, size_t out_bytes, int trips, void *stream) {
    if (dtype < 0 || dtype > 2) PROBE_REFUSE("probe scan: no dtype %d", dtype);
    if (!wave_multiple(threads) || blocks < 1 || blocks > PROBE_MAX_BLOCKS) PROBE_REFUSE("probe scan: %d threads x %d workgroups", threads, blocks);
    if (!in || !out) PROBE_REFUSE("probe scan: in / out is NULL");
    if (trips < 0 || trips > CONTRACT_MAX_TRIPS || (!contract && trips)) PROBE_REFUSE("probe scan: %d trips", trips);
    const size_t plane = (size_t)threads * blocks * (dtype == 2 ? 8 : 4);
    const size_t need_in = plane * (contract ? 3 + trips : 1), need_out = plane * (contract ? 5 + 2 * trips : 2);
    if (in_bytes < need_in || out_bytes < need_out) PROBE_REFUSE("probe scan: needs %zu bytes in and %zu out", need_in, need_out);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0) return launch_scan_probe_t<uint32_t>(threads, contract != 0, blocks, in, out, trips, s);
    if (dtype == 1) return launch_scan_probe_t<int>(threads, contract != 0, blocks, in, out, trips, s);
    return launch_scan_probe_t<u64>(threads, contract != 0, blocks, in, out, trips, s);
}

// is_int 0: block_sum<waves>(float), waves 4 or 8; 1: block_sum<waves>(int), waves 1, 4 or 16.  Two planes in, two out.
int lvdgs_probe_block_sum(int is_int, int waves, int blocks, const void *in, size_t in_bytes, void *out, size_t out_bytes, void *stream) {
    const bool known = is_int ? (waves == 1 || waves == 4 || waves == 16) : (waves == 4 || waves == 8);
    if (!known) PROBE_REFUSE("probe block_sum: no %s instantiation for %d waves", is_int ? "int" : "float", waves);
    if (blocks < 1 || blocks > PROBE_MAX_BLOCKS) PROBE_REFUSE("probe block_sum: %d workgroups", blocks);
    if (!in || !out) PROBE_REFUSE("probe block_sum: in / out is NULL");
    const size_t need = (size_t)64 * waves * blocks * 2 * 4;
    if (in_bytes < need || out_bytes < need) PROBE_REFUSE("probe block_sum: needs %zu bytes in and out", need);
    hipStream_t s = (hipStream_t)stream;
    if (!is_int) return waves == 4 ? launch_block_sum<4, float>(blocks, in, out, s) : launch_block_sum<8, float>(blocks, in, out, s);
    if (waves == 1) return launch_block_sum<1, int>(blocks, in, out, s);
    return waves == 4 ? launch_block_sum<4, int>(blocks, in, out, s) : launch_block_sum<16, int>(blocks, in, out, s);
}

// out: (begin, end) of each of `blocks` workgroups
int lvdgs_probe_span_range(uint32_t n, uint32_t span, int blocks, uint32_t *out, size_t out_bytes, void *stream) {
    if (blocks < 1 || blocks > PROBE_MAX_BLOCKS) PROBE_REFUSE("probe span_range: %d workgroups", blocks);
    if (!out || out_bytes < (size_t)blocks * 2 * sizeof(uint32_t)) PROBE_REFUSE("probe span_range: out is NULL or too small");
    if (n > 0x7fffffffu || span == 0 || (uint64_t)blocks * span > 0xffffffffull) PROBE_REFUSE("probe span_range: n %u, span %u outside the contract", n, span);
    hipStream_t s = (hipStream_t)stream;
    if (int e = launch_checked("probe span_range", 0, s, span_range_kernel, dim3(blocks), dim3(WAVE), 0, n, span, out)) return e;
    return LVDGS_OK;
}

// form: 0 <256, uint32_t, uint32_t>, 1 <256, uint32_t, u64>, 2 <256, u64, u64>, 3 <1024, uint32_t, u64>.  counts, before: blocks * stride
// words of T resp. C (in place, before == counts, only where T == C); totals: one C per thread.
int lvdgs_probe_span_counts(int form, const void *counts, size_t counts_bytes, void *before, size_t before_bytes, int blocks, int stride, void *totals,
                            size_t totals_bytes, void *stream) {
    if (form < 0 || form > 3) PROBE_REFUSE("probe scan_span_counts: no form %d", form);
    if (!counts || !before || !totals) PROBE_REFUSE("probe scan_span_counts: counts / before / totals is NULL");
    if (blocks < 0 || blocks > (1 << 20) || stride < 1 || stride > 64) PROBE_REFUSE("probe scan_span_counts: %d spans, stride %d", blocks, stride);
    const size_t t_bytes = form == 2 ? 8 : 4, c_bytes = form == 0 ? 4 : 8, threads = form == 3 ? 1024 : 256;
    if (counts == before && t_bytes != c_bytes) PROBE_REFUSE("probe scan_span_counts: form %d cannot run in place", form);
    const size_t words = (size_t)blocks * stride;
    if (counts_bytes < words * t_bytes || before_bytes < words * c_bytes || totals_bytes < threads * c_bytes)
        PROBE_REFUSE("probe scan_span_counts: a buffer is too small for %d spans of stride %d", blocks, stride);
    hipStream_t s = (hipStream_t)stream;
    if (form == 0) return launch_span_counts<256, uint32_t, uint32_t>(counts, before, blocks, stride, totals, s);
    if (form == 1) return launch_span_counts<256, uint32_t, u64>(counts, before, blocks, stride, totals, s);
    if (form == 2) return launch_span_counts<256, u64, u64>(counts, before, blocks, stride, totals, s);
    return launch_span_counts<1024, uint32_t, u64>(counts, before, blocks, stride, totals, s);
}

// form: TileWalk<256, uint32_t> (0), <256, uint32_t, u64> (1), <256, uint32_t, int64_t> (2), <256, u64> (3).  keep: n bytes (of keep_bytes).  scratch: two arrays of
// `blocks` 8-byte words (the span counts and what lies in front of each span).  out_index, out_row: `capacity` words each.  total_out: one u64.
int lvdgs_probe_compact(int form, const uint8_t *keep, size_t keep_bytes, int64_t n, int blocks, uint64_t row0, void *scratch, size_t scratch_bytes, uint32_t *out_index,
                        uint64_t *out_row, int64_t capacity, size_t out_index_bytes, size_t out_row_bytes, uint64_t *total_out, void *stream) {
    if (form < 0 || form > 3) PROBE_REFUSE("probe compact: no form %d", form);
    if (n < 0 || n > 0x7fffffffll || blocks < 1 || blocks > PROBE_MAX_BLOCKS) PROBE_REFUSE("probe compact: %lld elements, %d workgroups", (long long)n, blocks);
    if (!keep || !scratch || !out_index || !out_row || !total_out) PROBE_REFUSE("probe compact: a pointer is NULL");
    if (keep_bytes < (size_t)n) PROBE_REFUSE("probe compact: keep holds %zu bytes for %lld elements", keep_bytes, (long long)n);
    if (capacity < 0 || out_index_bytes < (size_t)capacity * 4 || out_row_bytes < (size_t)capacity * 8) PROBE_REFUSE("probe compact: outputs smaller than the capacity");
    if (scratch_bytes < (size_t)blocks * 16) PROBE_REFUSE("probe compact: scratch holds fewer than 2 x %d 8-byte words", blocks);
    if (form == 0 && row0 > 0xffffffffull) PROBE_REFUSE("probe compact: a 32-bit walk cannot start at row %llu", (unsigned long long)row0);
    hipStream_t s = (hipStream_t)stream;
    void *counts = scratch, *before = (char *)scratch + (size_t)blocks * 8;
    const uint32_t n32 = (uint32_t)n;
    u64 *tot = (u64 *)total_out, *rows = (u64 *)out_row;
    if (form == 0) return launch_compact<uint32_t, uint32_t, uint32_t>(keep, n32, blocks, row0, counts, before, out_index, rows, capacity, tot, s);
    if (form == 1) return launch_compact<uint32_t, u64, u64>(keep, n32, blocks, row0, counts, before, out_index, rows, capacity, tot, s);
    if (form == 2) return launch_compact<uint32_t, int64_t, u64>(keep, n32, blocks, row0, counts, before, out_index, rows, capacity, tot, s);
    return launch_compact<u64, u64, u64>(keep, n32, blocks, row0, counts, before, out_index, rows, capacity, tot, s);
}

// The radix select over v[0 .. n) (v_count, take_count: what the arrays hold; take null: all take part; use_keys: the keys fmix32(i) in place of v).  The rank: SelectRank{fixed, fraction}.
// state: lvdgs_probe_select_state_bytes() bytes, cleared here on the stream as the callers do; report: lvdgs_probe_select_report_words() words
// (result bits, n, ticket, k, and with per_pass the ticket behind each pass).
int lvdgs_probe_select(const float *v, size_t v_count, const uint8_t *take, size_t take_count, int64_t n, int use_keys, int64_t fixed, double fraction, void *state, size_t state_bytes,
                       uint32_t *report, size_t report_bytes, int per_pass, void *stream) {
    if (n < 0 || n > 0x7fffffffll) PROBE_REFUSE("probe select: %lld elements", (long long)n);
    if ((!use_keys && !v) || !state || !report) PROBE_REFUSE("probe select: v / state / report is NULL");
    if ((!use_keys && v_count < (size_t)n) || (take && take_count < (size_t)n)) PROBE_REFUSE("probe select: v or take holds fewer than %lld elements", (long long)n);
    if (state_bytes < sizeof(SelectState) || report_bytes < SP_WORDS * sizeof(uint32_t)) PROBE_REFUSE("probe select: state or report too small");
    if (fixed < 0 && !(fraction >= 0.0 && fraction <= 1.0)) PROBE_REFUSE("probe select: fraction %g", fraction);
    hipStream_t s = (hipStream_t)stream;
    const SelectRank rank{fixed, fraction};
    if (use_keys) return run_select(ProbeKeySource{take}, n, (SelectState *)state, rank, report, per_pass != 0, true, s);
    return run_select(ProbeSource{v, take}, n, (SelectState *)state, rank, report, per_pass != 0, false, s);
}

// select_segment: `segments` workgroups, workgroup b over v[b * n .. (b + 1) * n); out: 256 words per segment
int lvdgs_probe_select_segment(const float *v, const uint8_t *take, int n, int segments, size_t v_count, size_t take_count, uint32_t *out, size_t out_bytes, void *stream) {
    if (n < 0 || n > (1 << 20) || segments < 1 || segments > PROBE_MAX_BLOCKS) PROBE_REFUSE("probe select_segment: %d segments of %d", segments, n);
    if (!v || !out) PROBE_REFUSE("probe select_segment: v / out is NULL");
    if (v_count < (size_t)n * segments || (take && take_count < (size_t)n * segments) || out_bytes < (size_t)segments * SEL_THREADS * sizeof(uint32_t)) PROBE_REFUSE("probe select_segment: a buffer is too small");
    hipStream_t s = (hipStream_t)stream;
    if (int e = launch_checked("probe select_segment", 0, s, select_segment_kernel, dim3(segments), dim3(SEL_THREADS), 0, v, take, n, out)) return e;
    return LVDGS_OK;
}

// ok: 64 bytes, digit: 64 words, out: 256 counters
int lvdgs_probe_hist_add(const uint8_t *ok, const uint32_t *digit, size_t lanes, uint32_t *out, size_t out_bytes, void *stream) {
    if (!ok || !digit || !out) PROBE_REFUSE("probe hist_add: a pointer is NULL");
    if (lanes < (size_t)WAVE || out_bytes < SEL_THREADS * sizeof(uint32_t)) PROBE_REFUSE("probe hist_add: a buffer is too small");
    hipStream_t s = (hipStream_t)stream;
    if (int e = launch_checked("probe hist_add", 0, s, hist_add_kernel, dim3(1), dim3(WAVE), 0, ok, digit, out)) return e;
    return LVDGS_OK;
}

}  // extern "C"
