// Seeding a keyframe's Gaussians (GaussianModel.create_pcd_from_image_and_depth): the subsample of the valid depth pixels, their
// back-projection into the world and their colours through 8 bits, as one call with no host wait inside it (semantics and the host
// block: include/lvdgs.h, DESIGN.md section "Seeding").
//
// The selection rule.  Pixel i = v*W + u of the H x W depth map is VALID when depth[i] > 0 && depth[i] <= depth_trunc (NaN fails).
//   n_valid = the number of valid pixels;  n_keep = (int64)((double)n_valid * inv_downsample), on the device, in double.
//   Every pixel has a 32-bit key, all arithmetic uint32 with wrap-around:
//     fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16
//     key(i)   = fmix32( fmix32((uint32)i + seed_lo) ^ seed_hi )                 seed = seed_hi:seed_lo, 64 bits per call
//   fmix32, the addition and the xor are bijections of uint32: for one seed all keys of an image are DISTINCT, there are no ties.
//   Selected are the n_keep valid pixels with the smallest keys: {i valid : key(i) <= t}, t the key of rank n_keep - 1 among the
//   valid keys (n_keep == 0 selects nothing).  Output rows are in ascending pixel index.
// A pure function of (seed, pixel index, validity): every replica of a map selects the same pixels with no generator state to share.
//
// t is an order statistic of the valid keys: select.hpp's four passes with a source that yields keys and a rank that is a function of
// the count pass 0 finds.  The optional median of ALL depth values is the same four passes as they stand.
// The ordered compaction of the selected pixels is a span scan (spans.hpp).  Integer decisions and the float expressions of the header
// only: two calls give the same bytes.
//
// Launches, all enqueued at once: a clear of the state, then EIGHT -- four select passes over the keys, seed_count_kernel,
// seed_scan_kernel, seed_write_kernel, seed_publish_kernel (the host block, its sequence word last) -- and four more select passes
// in front of them when the median is asked for: TWELVE.  The number depends on nothing else.
#include "select.hpp"
#include "spans.hpp"

namespace lvdgs {
namespace {

constexpr int SEED_THREADS = 256;
constexpr int SEED_MAX_BLOCKS = SEL_MAX_BLOCKS;   // spans, = words of the count array
constexpr uint32_t SEED_MIN_SPAN = SEL_THREADS * SEL_ITEMS_PER_THREAD;   // a span is sized like a workgroup of the select passes

__host__ __device__ inline uint32_t pixel_key(uint32_t i, uint32_t seed_lo, uint32_t seed_hi) { return fmix32(fmix32(i + seed_lo) ^ seed_hi); }

struct SeedParams {
    int W, H;
    int64_t P;               // pixels
    int64_t span;            // pixels per workgroup of the count and write passes, a multiple of SEED_THREADS
    int capacity, want_median;
    float fx, fy, cx, cy, trunc;
    double inv_downsample;
    uint32_t seed_lo, seed_hi, seq;
    const float *image, *gain, *offset, *depth, *R, *T;
    float *xyz, *rgb, *f_dc;
    int32_t *pixel;
    SelectState *st_key, *st_median;
    uint32_t *counts;        // SEED_MAX_BLOCKS: per span, the selected pixels; after seed_scan_kernel the rows in front of the span
    int32_t *host;           // device address of the caller's pinned block
};

struct KeySource {   // the valid pixels' keys
    const float *depth;
    float trunc;
    uint32_t seed_lo, seed_hi;
    __device__ __forceinline__ bool key(int64_t i, uint32_t &k) const {
        const float d = depth[i];
        k = pixel_key((uint32_t)i, seed_lo, seed_hi);
        return d > 0.0f && d <= trunc;
    }
};

struct AllDepthSource {   // every depth value takes part (depth.median())
    const float *depth;
    __device__ __forceinline__ bool get(int64_t i, float &v) const { v = depth[i]; return true; }
};

__device__ __forceinline__ int64_t keep_of(uint32_t n_valid, double inv_downsample) { return (int64_t)((double)n_valid * inv_downsample); }

// Is pixel i (< P) selected?  t: the threshold key; keep: n_keep > 0.
__device__ __forceinline__ bool selected(const SeedParams &S, int64_t i, uint32_t t, bool keep) {
    const float d = S.depth[i];
    return keep && d > 0.0f && d <= S.trunc && pixel_key((uint32_t)i, S.seed_lo, S.seed_hi) <= t;
}

__global__ void __launch_bounds__(SEED_THREADS) seed_count_kernel(SeedParams S) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t t = S.st_key->prefix;
    const bool keep = keep_of(S.st_key->n, S.inv_downsample) > 0;
    const SpanRange<int64_t> r = span_range(S.P, S.span, blockIdx.x);
    uint32_t mine = 0;
    for (int64_t i = r.begin + threadIdx.x; i < r.end; i += SEED_THREADS) mine += selected(S, i, t, keep);
    uint32_t total = 0;
    scan_workgroup<SEED_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) S.counts[blockIdx.x] = total;
}

// One workgroup: the counts of the `blocks` <= SEED_MAX_BLOCKS spans become the number of rows in front of each.
__global__ void __launch_bounds__(SEED_THREADS) seed_scan_kernel(SeedParams S, int blocks) {
    __shared__ uint32_t sh[SCAN_WORDS];
    scan_span_counts<SEED_THREADS>(S.counts, S.counts, blocks, 1, sh);
}

__global__ void __launch_bounds__(SEED_THREADS) seed_write_kernel(SeedParams S) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t t = S.st_key->prefix;
    const bool keep = keep_of(S.st_key->n, S.inv_downsample) > 0;
    const SpanRange<int64_t> r = span_range(S.P, S.span, blockIdx.x);
    const float gain = S.gain ? *S.gain : 1.0f, offset = S.offset ? *S.offset : 0.0f;
    float R[9], T[3];
#pragma unroll
    for (int j = 0; j < 9; j++) R[j] = S.R[j];
#pragma unroll
    for (int j = 0; j < 3; j++) T[j] = S.T[j];
    TileWalk<SEED_THREADS, uint32_t> walk{S.counts[blockIdx.x]};
    for (int64_t base = r.begin; base < r.end; base += SEED_THREADS) {   // (uniform)
        const int64_t i = base + threadIdx.x;
        const bool sel = i < r.end && selected(S, i, t, keep);
        const int64_t row = walk.place(sel ? 1u : 0u, sh);
        if (!sel || row >= S.capacity) continue;   // (the host-side bound of n_keep keeps every row inside the capacity)
        const int v = (int)(i / S.W), u = (int)(i - (int64_t)v * S.W);
        const float z = S.depth[i];
        const float c0 = ((float)u - S.cx) * z / S.fx, c1 = ((float)v - S.cy) * z / S.fy;
        const float d0 = c0 - T[0], d1 = c1 - T[1], d2 = z - T[2];
#pragma unroll
        for (int j = 0; j < 3; j++) S.xyz[3 * row + j] = d0 * R[j] + d1 * R[3 + j] + d2 * R[6 + j];
        if (S.pixel) S.pixel[row] = (int32_t)i;
        if (S.image) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float c = fminf(fmaxf(gain * S.image[ch * S.P + i] + offset, 0.0f), 1.0f);
                const uint8_t q = (uint8_t)(c * 255.0f);
                const float rgb = (float)q * (1.0f / 255.0f);   // PyTorch's `/ 255.0` on a GPU: times the float32 reciprocal
                S.rgb[3 * row + ch] = rgb;
                S.f_dc[3 * row + ch] = (rgb - 0.5f) / 0.28209479177387814f;
            }
        }
    }
}

__global__ void seed_publish_kernel(SeedParams S) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    volatile int32_t *w = S.host;
    const uint32_t n_valid = S.st_key->n;
    w[LVDGS_SEED_N_VALID] = (int32_t)n_valid;
    w[LVDGS_SEED_N_KEEP] = (int32_t)keep_of(n_valid, S.inv_downsample);
    w[LVDGS_SEED_MEDIAN] = (int32_t)(S.want_median ? select_result_bits(S.st_median->n, S.st_median->prefix) : SEL_QUIET_NAN);
    w[LVDGS_SEED_THRESHOLD] = (int32_t)S.st_key->prefix;
    for (int j = LVDGS_SEED_THRESHOLD + 1; j < (int)(LVDGS_SEED_HOST_BYTES / sizeof(int32_t)); j++) w[j] = 0;
    seal_host_block(w, LVDGS_SEED_SEQ, (int32_t)S.seq);
}

// the scratch: the two selections' states, a count per span
size_t seed_layout(SeedParams *S, void *base) {
    Carver<SeedParams> c(S, base);
    c(c.v.st_key, 1); c(c.v.st_median, 1); c(c.v.counts, SEED_MAX_BLOCKS);
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_seed_scratch_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1 || (int64_t)width * height > INT32_MAX) return 0;
    return seed_layout(nullptr, nullptr);
}

int lvdgs_seed_points(const lvdgs_seed_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("seed points: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width < 1 || a->height < 1 || (int64_t)a->width * a->height > INT32_MAX) {
        set_error("seed points: image size %dx%d", a->width, a->height); return LVDGS_E_RANGE;
    }
    if (!(a->inv_downsample > 0.0 && a->inv_downsample <= 1.0)) {
        set_error("seed points: inv_downsample %g is outside (0, 1]", a->inv_downsample); return LVDGS_E_RANGE;
    }
    const int64_t P = (int64_t)a->width * a->height;
    const int64_t bound = (int64_t)((double)P * a->inv_downsample);
    if ((int64_t)a->capacity < bound) {
        set_error("seed points: capacity %d is below the %lld rows %dx%d pixels can give", a->capacity, (long long)bound, a->width, a->height);
        return LVDGS_E_RANGE;
    }
    if (!a->depth || !a->R || !a->T || !a->xyz || !a->host_state || !a->scratch) {
        set_error("seed points: depth / R / T / xyz / host_state / scratch is NULL"); return LVDGS_E_INVALID;
    }
    if (a->image && (!a->rgb || !a->f_dc)) { set_error("seed points: rgb / f_dc is NULL with an image"); return LVDGS_E_INVALID; }
    SeedParams S{};
    const size_t state_bytes = seed_layout(&S, a->scratch);
    if (a->scratch_bytes < state_bytes) { set_error("seed points: scratch too small"); return LVDGS_E_INVALID; }
    S.W = a->width; S.H = a->height; S.P = P;
    S.capacity = a->capacity; S.want_median = a->want_median != 0;
    S.fx = a->fx; S.fy = a->fy; S.cx = a->cx; S.cy = a->cy; S.trunc = a->depth_trunc;
    S.inv_downsample = a->inv_downsample;
    S.seed_lo = (uint32_t)a->seed; S.seed_hi = (uint32_t)(a->seed >> 32); S.seq = a->seq;
    S.image = a->image; S.gain = a->gain; S.offset = a->offset; S.depth = a->depth; S.R = a->R; S.T = a->T;
    S.xyz = a->xyz; S.rgb = a->rgb; S.f_dc = a->f_dc; S.pixel = a->pixel;
    if (int e = host_block_address(a->host_state, "seed points", &S.host)) return e;
    const Spans spans = make_spans(P, SEED_THREADS, SEED_MAX_BLOCKS, SEED_MIN_SPAN);
    const int blocks = spans.blocks;
    S.span = spans.span;
    if (int e = check_hip(hipMemsetAsync(a->scratch, 0, state_bytes, s), "seed points: clearing the state")) return e;
    if (S.want_median)
        if (int e = launch_select(AllDepthSource{S.depth}, P, S.st_median, select_rank(-1), "seed_median", s)) return e;
    if (int e = launch_select(KeySource{S.depth, S.trunc, S.seed_lo, S.seed_hi}, P, S.st_key, SelectRank{-1, S.inv_downsample}, "seed_threshold", s)) return e;
    if (int e = launch("seed_count", 0, s, seed_count_kernel, dim3(blocks), dim3(SEED_THREADS), 0, S)) return e;
    if (int e = launch("seed_scan", 0, s, seed_scan_kernel, dim3(1), dim3(SEED_THREADS), 0, S, blocks)) return e;
    if (int e = launch("seed_write", 0, s, seed_write_kernel, dim3(blocks), dim3(SEED_THREADS), 0, S)) return e;
    if (int e = launch("seed_publish", 0, s, seed_publish_kernel, dim3(1), dim3(WAVE), 0, S)) return e;
    return LVDGS_OK;
}

}  // extern "C"
