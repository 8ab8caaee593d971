// The two statements that bracket a tracked frame's loop, each as one call with no host wait inside it (semantics: include/lvdgs.h,
// DESIGN.md section "Frame statistics"):
//   lvdgs_edge_mask      Camera.compute_grad_mask (reference utils/camera_utils.py:126-155): the Scharr magnitude of the grey image under
//                        the validity mask, thresholded against its median -- of the whole image, or per block of a 32 x 32 grid (replica).
//   lvdgs_frame_summary  what the front end reads after the last tracking iteration (utils/slam_frontend.py:1579-1674, utils/slam_utils.py
//                        get_median_depth): the median rendered depth over the opaque pixels and the covisibility counts of the frame
//                        against the window's keyframes, left in one block of pinned host memory.
// Both medians are exact order statistics (select.hpp): no sort, no compaction, the bits a sort would give.
//
// Launches, all enqueued at once:
//   edge mask, whole image   a clear of the selection state; edge_magnitude_kernel; four select passes; edge_threshold_kernel
//   edge mask, replica       edge_magnitude_kernel (magnitudes straight into the result); edge_blocks_kernel, one workgroup per block:
//                            its median (select_segment), then the block thresholded in place
//   frame summary            a clear of the state; four select passes over the depth; summary_counts_kernel (covisibility rows, the
//                            visible count, the counted mask); summary_publish_kernel, one thread, the host block with its sequence
//                            word last
#include <math.h>

#include "select.hpp"

namespace lvdgs {
namespace {

constexpr int FS_THREADS = 256;
constexpr int EDGE_GRID = 32;                         // the replica rule's blocks per image edge
constexpr int EDGE_BLOCKS = EDGE_GRID * EDGE_GRID;
constexpr int FS_MAX_BLOCKS = 1024;

int stream_blocks(int64_t n) {
    const int64_t b = (n + FS_THREADS - 1) / FS_THREADS;
    return (int)(b < 1 ? 1 : (b > FS_MAX_BLOCKS ? FS_MAX_BLOCKS : b));
}

// ---------------------------------------------------------------- edge mask
struct EdgeParams {
    int W, H, mode;
    float thr;               // (float)edge_threshold
    const float *image;      // 3 * H * W
    float *mag;              // H * W: where the magnitudes go (mode 1: the result image itself)
    float *mag_copy;         // optional second copy (the caller's `magnitude`)
    uint8_t *mask;           // mode 0: the result, H * W bytes
    uint8_t *loss_mask;      // optional: result != 0 as bytes
    float *stats;            // optional: (median, cut), per block in mode 1
    SelectState *st;
};

__device__ __forceinline__ int reflect(int i, int n) {   // np.pad(mode="reflect") by one element: -1 -> 1, n -> n - 2
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

// One pixel per thread; the nine grey taps straight from the image (each is read by nine threads of the same or a neighbouring row:
// L1 / L2 serve them; 453 k pixels of a KITTI frame are 5.4 MB of image).  Every expression in the header's order.
__global__ void __launch_bounds__(FS_THREADS) edge_magnitude_kernel(EdgeParams P) {
    const int64_t n = (int64_t)P.W * P.H;
    const int64_t i = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / P.W), x = (int)(i - (int64_t)y * P.W);
    float p[3][3];
    bool full = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int yy = reflect(y + r - 1, P.H);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int xx = reflect(x + c - 1, P.W);
            const int64_t o = (int64_t)yy * P.W + xx;
            const float g = ((P.image[o] + P.image[n + o]) + P.image[2 * n + o]) / 3.0f;
            p[r][c] = g;
            full = full && fabsf(g) > 0.01f;
        }
    }
    const float scale = 1.0f / 32.0f;
    float gv = (((((p[0][0] * 3.0f + p[0][1] * 10.0f) + p[0][2] * 3.0f) + p[2][0] * -3.0f) + p[2][1] * -10.0f) + p[2][2] * -3.0f) * scale;
    float gh = (((((p[0][0] * 3.0f + p[0][2] * -3.0f) + p[1][0] * 10.0f) + p[1][2] * -10.0f) + p[2][0] * 3.0f) + p[2][2] * -3.0f) * scale;
    const float m = full ? 1.0f : 0.0f;
    gv = gv * m;
    gh = gh * m;
    const float mag = sqrtf(gv * gv + gh * gh);
    P.mag[i] = mag;
    if (P.mag_copy) P.mag_copy[i] = mag;
    if (P.mode == 1 && P.loss_mask) P.loss_mask[i] = mag != 0.0f;   // outside the block grid the result is the magnitude; inside, edge_blocks_kernel overwrites
}

struct MagSource {   // every magnitude takes part
    const float *mag;
    __device__ __forceinline__ bool get(int64_t i, float &v) const { v = mag[i]; return true; }
};

__global__ void __launch_bounds__(FS_THREADS) edge_threshold_kernel(EdgeParams P) {
    const int64_t n = (int64_t)P.W * P.H;
    const float median = __uint_as_float(select_result_bits(P.st->n, P.st->prefix));
    const float cut = median * P.thr;
    if (P.stats && blockIdx.x == 0 && threadIdx.x == 0) { P.stats[0] = median; P.stats[1] = cut; }
    for (int64_t i = (int64_t)blockIdx.x * FS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FS_THREADS) {
        const uint8_t b = P.mag[i] > cut;
        P.mask[i] = b;
        if (P.loss_mask) P.loss_mask[i] = b;
    }
}

struct BlockSource {   // block (by, bx) of the 32 x 32 grid, row-major inside the block
    const float *mag;
    int W, bw;
    int64_t origin;
    __device__ __forceinline__ int64_t at(int i) const { const int r = i / bw; return origin + (int64_t)r * W + (i - r * bw); }
    __device__ __forceinline__ bool get(int64_t i, float &v) const { v = mag[at((int)i)]; return true; }
};

__global__ void __launch_bounds__(SEL_THREADS) edge_blocks_kernel(EdgeParams P) {
    __shared__ uint32_t hist[SEL_THREADS];
    __shared__ uint32_t sh[SCAN_WORDS + 2];
    const int bh = P.H / EDGE_GRID, bw = P.W / EDGE_GRID;
    const int by = blockIdx.x / EDGE_GRID, bx = blockIdx.x - by * EDGE_GRID;
    const BlockSource src{P.mag, P.W, bw, (int64_t)by * bh * P.W + (int64_t)bx * bw};
    const int n = bh * bw;
    const float median = __uint_as_float(select_segment(src, n, hist, sh));   // (ends with a barrier: every read of the block is done)
    const float cut = median * P.thr;
    if (P.stats && threadIdx.x == 0) { P.stats[2 * blockIdx.x] = median; P.stats[2 * blockIdx.x + 1] = cut; }
    for (int i = threadIdx.x; i < n; i += SEL_THREADS) {
        const int64_t o = src.at(i);
        const float v = P.mag[o];
        float r = v > cut ? 1.0f : v;     // the reference sets 1 above the cut ...
        r = r <= cut ? 0.0f : r;          // ... and then 0 at or below it: a cut of 1 or more clears the ones again
        P.mag[o] = r;
        if (P.loss_mask) P.loss_mask[o] = r != 0.0f;
    }
}

// ---------------------------------------------------------------- frame summary
struct SummaryCounters {            // device side, behind the SelectState; zeroed with it
    uint32_t visible, mask_count, pad[2];
    uint32_t rows[LVDGS_FRAME_SUMMARY_MAX_ROWS][4];   // intersection, union, the row's own count, unused
};

struct SummaryParams {
    int64_t P;               // pixels
    int N, R;
    uint32_t seq;
    float bar;
    const float *depth, *opacity;
    const uint8_t *mask, *count_mask;
    const int32_t *n_touched;
    const uint8_t *rows[LVDGS_FRAME_SUMMARY_MAX_ROWS];
    SelectState *st;
    SummaryCounters *cnt;
    int32_t *host;           // device address of the caller's pinned block
};

struct DepthSource {   // get_median_depth's selection: depth > 0, opacity > bar, mask
    const float *depth, *opacity;
    const uint8_t *mask;
    float bar;
    __device__ __forceinline__ bool get(int64_t i, float &v) const {
        v = depth[i];
        return v > 0.0f && (!opacity || opacity[i] > bar) && (!mask || mask[i] != 0);
    }
};

__device__ __forceinline__ uint32_t wave_count(bool b) { return (uint32_t)__popcll(__ballot(b)); }

__global__ void __launch_bounds__(FS_THREADS) summary_counts_kernel(SummaryParams S) {
    __shared__ uint32_t acc[2 + 3 * LVDGS_FRAME_SUMMARY_MAX_ROWS];
    for (int j = threadIdx.x; j < 2 + 3 * LVDGS_FRAME_SUMMARY_MAX_ROWS; j += FS_THREADS) acc[j] = 0;
    __syncthreads();
    const int lane = threadIdx.x % WAVE;
    const int64_t stride = (int64_t)gridDim.x * FS_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * FS_THREADS; base < S.N; base += stride) {   // (uniform: whole waves reach the ballots)
        const int64_t i = base + threadIdx.x;
        const bool in = i < S.N;
        const bool cur = in && S.n_touched[i] > 0;
        const uint32_t c = wave_count(cur);
        if (lane == 0 && c) atomicAdd(&acc[0], c);
        for (int r = 0; r < S.R; r++) {
            const bool b = in && S.rows[r][i] != 0;
            const uint32_t ni = wave_count(cur && b), nu = wave_count(cur || b), nb = wave_count(b);
            if (lane == 0) {
                if (ni) atomicAdd(&acc[2 + 3 * r], ni);
                if (nu) atomicAdd(&acc[3 + 3 * r], nu);
                if (nb) atomicAdd(&acc[4 + 3 * r], nb);
            }
        }
    }
    if (S.count_mask) {
        for (int64_t base = (int64_t)blockIdx.x * FS_THREADS; base < S.P; base += stride) {
            const int64_t i = base + threadIdx.x;
            const uint32_t c = wave_count(i < S.P && S.count_mask[i] != 0);
            if (lane == 0 && c) atomicAdd(&acc[1], c);
        }
    }
    __syncthreads();
    // integer sums: the order of arrival does not show
    if (threadIdx.x == 0 && acc[0]) atomicAdd(&S.cnt->visible, acc[0]);
    if (threadIdx.x == 1 && acc[1]) atomicAdd(&S.cnt->mask_count, acc[1]);
    if ((int)threadIdx.x >= 2 && (int)threadIdx.x < 2 + 3 * S.R) {
        const int j = threadIdx.x - 2;
        if (acc[threadIdx.x]) atomicAdd(&S.cnt->rows[j / 3][j % 3], acc[threadIdx.x]);
    }
}

__global__ void summary_publish_kernel(SummaryParams S) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    volatile int32_t *w = S.host;
    w[LVDGS_FRAME_SUMMARY_MEDIAN] = (int32_t)select_result_bits(S.st->n, S.st->prefix);
    w[LVDGS_FRAME_SUMMARY_SELECTED] = (int32_t)S.st->n;
    w[LVDGS_FRAME_SUMMARY_VISIBLE] = (int32_t)S.cnt->visible;
    w[LVDGS_FRAME_SUMMARY_MASK_COUNT] = (int32_t)S.cnt->mask_count;
    for (int j = LVDGS_FRAME_SUMMARY_MASK_COUNT + 1; j < LVDGS_FRAME_SUMMARY_ROWS; j++) w[j] = 0;
    for (int r = 0; r < LVDGS_FRAME_SUMMARY_MAX_ROWS; r++)
        for (int j = 0; j < 3; j++) w[LVDGS_FRAME_SUMMARY_ROWS + 3 * r + j] = r < S.R ? (int32_t)S.cnt->rows[r][j] : 0;
    seal_host_block(w, LVDGS_FRAME_SUMMARY_SEQ, (int32_t)S.seq);
}

// the edge mask's scratch: the selection's state, the gradient magnitudes (LVDGS_EDGE_MASK_BLOCKS keeps them in the caller's mask plane)
size_t edge_layout(int W, int H, EdgeParams *P, void *base) {
    Carver<EdgeParams> c(P, base);
    c(c.v.st, 1); c(c.v.mag, (size_t)W * H);
    return c.off;
}

// the summary's: the selection's state, the counters
size_t summary_layout(SummaryParams *S, void *base) {
    Carver<SummaryParams> c(S, base);
    c(c.v.st, 1); c(c.v.cnt, 1);
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_edge_mask_scratch_bytes(int32_t width, int32_t height) {
    if (width < 2 || height < 2) return 0;
    return edge_layout(width, height, nullptr, nullptr);
}

int lvdgs_edge_mask(const lvdgs_edge_mask_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("edge mask: args is NULL"); return LVDGS_E_INVALID; }
    if (a->mode != LVDGS_EDGE_MASK_MEDIAN && a->mode != LVDGS_EDGE_MASK_BLOCKS) {
        set_error("edge mask: mode %d is neither LVDGS_EDGE_MASK_MEDIAN nor LVDGS_EDGE_MASK_BLOCKS", a->mode); return LVDGS_E_INVALID;
    }
    if (a->width < 2 || a->height < 2 || (int64_t)a->width * a->height > INT32_MAX) {
        set_error("edge mask: image size %dx%d (the reflected border needs two pixels per edge)", a->width, a->height); return LVDGS_E_RANGE;
    }
    if (a->mode == LVDGS_EDGE_MASK_BLOCKS && (a->width < EDGE_GRID || a->height < EDGE_GRID)) {
        set_error("edge mask: image size %dx%d has no %d x %d grid of blocks", a->width, a->height, EDGE_GRID, EDGE_GRID); return LVDGS_E_RANGE;
    }
    if (!a->image || !a->mask || !a->scratch) { set_error("edge mask: image / mask / scratch is NULL"); return LVDGS_E_INVALID; }
    EdgeParams P{};
    if (a->scratch_bytes < edge_layout(a->width, a->height, &P, a->scratch)) { set_error("edge mask: scratch too small"); return LVDGS_E_INVALID; }
    P.W = a->width; P.H = a->height; P.mode = a->mode;
    P.thr = (float)a->edge_threshold;
    P.image = a->image;
    P.loss_mask = a->loss_mask; P.stats = a->stats;
    const int64_t n = (int64_t)P.W * P.H;
    const int pixel_blocks = (int)((n + FS_THREADS - 1) / FS_THREADS);
    if (a->mode == LVDGS_EDGE_MASK_BLOCKS) {
        P.mag = reinterpret_cast<float *>(a->mask);
        P.mag_copy = a->magnitude;
        if (int e = launch("edge_magnitude", 0, s, edge_magnitude_kernel, dim3(pixel_blocks), dim3(FS_THREADS), 0, P)) return e;
        if (int e = launch("edge_blocks", 0, s, edge_blocks_kernel, dim3(EDGE_BLOCKS), dim3(SEL_THREADS), 0, P)) return e;
        return LVDGS_OK;
    }
    P.mag_copy = a->magnitude;
    P.mask = reinterpret_cast<uint8_t *>(a->mask);
    if (int e = check_hip(hipMemsetAsync(P.st, 0, sizeof(SelectState), s), "edge mask: clearing the selection state")) return e;
    if (int e = launch("edge_magnitude", 0, s, edge_magnitude_kernel, dim3(pixel_blocks), dim3(FS_THREADS), 0, P)) return e;
    if (int e = launch_select(MagSource{P.mag}, n, P.st, -1, "edge_median", s)) return e;
    if (int e = launch("edge_threshold", 0, s, edge_threshold_kernel, dim3(stream_blocks(n)), dim3(FS_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

size_t lvdgs_frame_summary_scratch_bytes(void) { return summary_layout(nullptr, nullptr); }

int lvdgs_frame_summary(const lvdgs_frame_summary_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("frame summary: args is NULL"); return LVDGS_E_INVALID; }
    if (a->num_rows < 0 || a->num_rows > LVDGS_FRAME_SUMMARY_MAX_ROWS) {
        set_error("frame summary: %d visibility rows, outside 0..%d", a->num_rows, LVDGS_FRAME_SUMMARY_MAX_ROWS); return LVDGS_E_RANGE;
    }
    if (a->num_gaussians < 0 || a->num_pixels < 0) {
        set_error("frame summary: num_gaussians %d / num_pixels %d is negative", a->num_gaussians, a->num_pixels); return LVDGS_E_RANGE;
    }
    if (!a->host_state || !a->scratch) { set_error("frame summary: host_state / scratch is NULL"); return LVDGS_E_INVALID; }
    if (a->num_pixels > 0 && !a->depth) { set_error("frame summary: depth is NULL"); return LVDGS_E_INVALID; }
    if (a->num_gaussians > 0) {
        if (!a->n_touched) { set_error("frame summary: n_touched is NULL"); return LVDGS_E_INVALID; }
        for (int r = 0; r < a->num_rows; r++)
            if (!a->rows[r]) { set_error("frame summary: visibility row %d is NULL", r); return LVDGS_E_INVALID; }
    }
    SummaryParams S{};
    const size_t state_bytes = summary_layout(&S, a->scratch);
    if (a->scratch_bytes < state_bytes) { set_error("frame summary: scratch too small"); return LVDGS_E_INVALID; }
    S.P = a->num_pixels; S.N = a->num_gaussians; S.R = a->num_rows;
    S.seq = a->seq; S.bar = a->opacity_bar;
    S.depth = a->depth; S.opacity = a->opacity; S.mask = a->mask; S.count_mask = a->count_mask;
    S.n_touched = a->n_touched;
    for (int r = 0; r < S.R; r++) S.rows[r] = a->rows[r];
    if (int e = host_block_address(a->host_state, "frame summary", &S.host)) return e;
    if (int e = check_hip(hipMemsetAsync(a->scratch, 0, state_bytes, s), "frame summary: clearing the state")) return e;
    if (int e = launch_select(DepthSource{S.depth, S.opacity, S.mask, S.bar}, S.P, S.st, -1, "summary_median", s)) return e;
    const int64_t longest = S.count_mask && S.P > S.N ? S.P : S.N;
    if (int e = launch("summary_counts", 0, s, summary_counts_kernel, dim3(stream_blocks(longest)), dim3(FS_THREADS), 0, S)) return e;
    if (int e = launch("summary_publish", 0, s, summary_publish_kernel, dim3(1), dim3(WAVE), 0, S)) return e;
    return LVDGS_OK;
}

}  // extern "C"
