// Editing the map on the device (GaussianModel.prune_points, densify_and_prune, the pruning pass's rule): lvdgs_map_edit_plan decides
// which output row comes from which source row and how, lvdgs_map_edit_apply moves the rows of every per-Gaussian array in one launch
// (semantics, the host block and the arithmetic order: include/lvdgs.h, DESIGN.md section "Map edit").
//
// The plan is an ordered compaction into four consecutive segments -- KEEP rows, CLONE rows, SPLIT0 rows, SPLIT1 rows, each ascending
// by source -- as a span scan (spans.hpp) with five counters a span: the count pass classifies every source row once into one code
// byte and counts the span's rows per segment; the write pass reads the code bytes, so the two passes cannot disagree, and runs one
// tile walk per segment.  Launches, all enqueued at once: edit_count_kernel, edit_scan_kernel, edit_write_kernel (which also fills
// the host block's src copy), edit_publish_kernel (the counts, the sequence word last).  With no rows: the scan and the publish only.
//
// Apply is a bandwidth kernel: blockIdx.y is the column, the lanes run over consecutive dwords (bytes, for rows or addresses that are
// no multiple of four) of the column's OUTPUT, so stores coalesce; the source row is looked up per element.
#include "common.hpp"
#include "device_utils.hpp"
#include "map_edit_host.hpp"
#include "spans.hpp"

namespace lvdgs {
namespace {

// code byte of a source row
constexpr uint8_t CODE_KEEP = 1;      // the original is in the output
constexpr uint8_t CODE_CLONE = 2;     // its clone is in the output
constexpr uint8_t CODE_CHILDREN = 4;  // its two split children are in the output
constexpr uint8_t CODE_SPLIT = 8;     // it is a split source (takes a rank among them, children pruned or not)
constexpr uint8_t CODE_CLONED = 16;   // the clone stage selected it (its clone pruned or not): counted only

struct PlanParams {
    int mode, N, S, capacity, blocks;
    int64_t span;
    uint32_t seq;
    const uint8_t *remove;
    int num_vis, vis_stride, prune_num, min_kf_id;
    const uint8_t *vis[LVDGS_EDIT_MAX_VIS_ROWS];
    const int32_t *kf_id;
    int32_t *n_obs;
    const float *accum, *denom, *scaling, *opacity;
    float thr, dense_extent, min_opacity, max_screen, world_extent;
    int32_t *src, *noise_row;
    uint8_t *kind;
    uint8_t *code;
    uint32_t *counts;   // [span][EDIT_COUNTERS]; after edit_scan_kernel: the rows in front of the span, per segment
    uint32_t *totals;   // [EDIT_COUNTERS]
    int32_t *host;      // device address of the caller's pinned block
    int64_t host_words;
};

// the raw scale of a split child: the one expression plan and apply share
__device__ __forceinline__ float child_scale(float s) { return logf(expf(s) / 1.6f); }

// max over the row's activated scales, a NaN propagating (torch.max)
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ bool gone(const PlanParams &P, float big, float opacity) {
    const bool faint = 1.0f / (1.0f + expf(-opacity)) < P.min_opacity;
    return faint || (P.max_screen != 0.0f && (0.0f > P.max_screen || big > P.world_extent));
}

__device__ __forceinline__ uint8_t classify(const PlanParams &P, int64_t i) {
    if (P.mode == LVDGS_EDIT_PRUNE) {
        if (P.remove) return P.remove[i] ? 0 : CODE_KEEP;
        int32_t n = 0;
        for (int k = 0; k < P.num_vis; k++) n += P.vis[k][i * P.vis_stride] != 0;
        P.n_obs[i] = n;
        return (n <= P.prune_num && P.kf_id[i] >= P.min_kf_id) ? 0 : CODE_KEEP;
    }
    float g = P.accum[i] / P.denom[i];
    if (g != g) g = 0.0f;
    float big = expf(P.scaling[i * P.S]), big_child = expf(child_scale(P.scaling[i * P.S]));
    for (int j = 1; j < P.S; j++) {
        const float s = P.scaling[i * P.S + j];
        big = nan_max(big, expf(s));
        big_child = nan_max(big_child, expf(child_scale(s)));
    }
    const bool clone = fabsf(g) >= P.thr && big <= P.dense_extent;
    const bool split = g >= P.thr && big > P.dense_extent;
    const float o = P.opacity[i];
    const bool stays = !gone(P, big, o);
    uint8_t c = clone ? CODE_CLONED : 0;
    if (!split && stays) c |= CODE_KEEP;
    if (clone && stays) c |= CODE_CLONE;
    if (split) c |= CODE_SPLIT;
    if (split && !gone(P, big_child, o)) c |= CODE_CHILDREN;
    return c;
}

__global__ void __launch_bounds__(EDIT_THREADS) edit_count_kernel(PlanParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<int64_t> r = span_range((int64_t)P.N, P.span, blockIdx.x);
    uint32_t mine[EDIT_COUNTERS] = {0, 0, 0, 0, 0};
    for (int64_t i = r.begin + threadIdx.x; i < r.end; i += EDIT_THREADS) {
        const uint8_t c = classify(P, i);
        P.code[i] = c;
#pragma unroll
        for (int q = 0; q < EDIT_COUNTERS; q++) mine[q] += (c >> q) & 1u;
    }
#pragma unroll
    for (int q = 0; q < EDIT_COUNTERS; q++) {
        uint32_t total = 0;
        scan_workgroup<EDIT_THREADS>(mine[q], sh, &total);
        if (threadIdx.x == 0) P.counts[blockIdx.x * EDIT_COUNTERS + q] = total;
    }
}

// One workgroup: per segment, the counts of the P.blocks <= EDIT_MAX_BLOCKS spans become the rows in front of each span, and the totals.
__global__ void __launch_bounds__(EDIT_THREADS) edit_scan_kernel(PlanParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    for (int q = 0; q < EDIT_COUNTERS; q++) {
        const uint32_t total = scan_span_counts<EDIT_THREADS>(P.counts + q, P.counts + q, P.blocks, EDIT_COUNTERS, sh);
        if (threadIdx.x == 0) P.totals[q] = total;
    }
}

__device__ __forceinline__ void put_row(const PlanParams &P, int64_t row, int64_t n_out, int64_t i, uint8_t kind, int32_t noise_row) {
    if (row >= P.capacity) return;   // (the host-side bound of the row count keeps every row inside the capacity)
    P.src[row] = (int32_t)i;
    P.kind[row] = kind;
    P.noise_row[row] = noise_row;
    if (LVDGS_EDIT_HOST_SRC + row < P.host_words) P.host[LVDGS_EDIT_HOST_SRC + row] = (int32_t)i;
    if (P.mode == LVDGS_EDIT_PRUNE && !P.remove && LVDGS_EDIT_HOST_SRC + n_out + row < P.host_words)
        P.host[LVDGS_EDIT_HOST_SRC + n_out + row] = P.n_obs[i];
}

__global__ void __launch_bounds__(EDIT_THREADS) edit_write_kernel(PlanParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<int64_t> r = span_range((int64_t)P.N, P.span, blockIdx.x);
    const int64_t n_keep = P.totals[0], n_clone = P.totals[1], n_child = P.totals[2], n_sel = P.totals[3];
    const int64_t n_out = n_keep + n_clone + 2 * n_child;
    // first row of this span in each segment (the children's two segments share one count), and its first split rank
    const uint32_t *front = P.counts + blockIdx.x * EDIT_COUNTERS;
    TileWalk<EDIT_THREADS, uint32_t, int64_t> walk[EDIT_SEGMENTS] = {{(int64_t)front[0]}, {n_keep + front[1]}, {n_keep + n_clone + front[2]},
                                                                     {(int64_t)front[3]}};
    for (int64_t base = r.begin; base < r.end; base += EDIT_THREADS) {   // (uniform)
        const int64_t i = base + threadIdx.x;
        const uint8_t c = i < r.end ? P.code[i] : 0;
        int64_t at[EDIT_SEGMENTS];
#pragma unroll
        for (int q = 0; q < EDIT_SEGMENTS; q++) at[q] = walk[q].place((uint32_t)((c >> q) & 1u), sh);
        if (c & CODE_KEEP) put_row(P, at[0], n_out, i, LVDGS_EDIT_KEEP, -1);
        if (c & CODE_CLONE) put_row(P, at[1], n_out, i, LVDGS_EDIT_CLONE, -1);
        if (c & CODE_CHILDREN) {
            put_row(P, at[2], n_out, i, LVDGS_EDIT_SPLIT0, (int32_t)at[3]);
            put_row(P, at[2] + n_child, n_out, i, LVDGS_EDIT_SPLIT1, (int32_t)(n_sel + at[3]));
        }
    }
}

__global__ void edit_publish_kernel(PlanParams P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    volatile int32_t *w = P.host;
    const int64_t n_keep = P.totals[0], n_clone = P.totals[1], n_child = P.totals[2], n_sel = P.totals[3];
    const int64_t n_out = n_keep + n_clone + 2 * n_child;
    // the list before the final prune: N originals less the split sources, the clone stage's rows, two children per split source
    const int64_t before = P.mode == LVDGS_EDIT_DENSIFY ? (int64_t)P.N + P.totals[4] + n_sel : (int64_t)P.N;
    w[LVDGS_EDIT_N_OUT] = (int32_t)n_out;
    w[LVDGS_EDIT_N_KEEP] = (int32_t)n_keep;
    w[LVDGS_EDIT_N_CLONE] = (int32_t)n_clone;
    w[LVDGS_EDIT_N_SPLIT_SEL] = (int32_t)n_sel;
    w[LVDGS_EDIT_N_PRUNED_FINAL] = (int32_t)(before - n_out);
    for (int j = LVDGS_EDIT_N_PRUNED_FINAL + 1; j < LVDGS_EDIT_HOST_SRC; j++) w[j] = 0;
    seal_host_block(w, LVDGS_EDIT_SEQ, (int32_t)P.seq);
}

struct ApplyParams {
    int N, n_out, S, n_sel;
    const int32_t *src, *noise_row;
    const uint8_t *kind;
    const float *noise, *scaling, *rotation;
    lvdgs_map_edit_column col[LVDGS_EDIT_MAX_COLUMNS];
};

// coordinate j of a split child's position (the header states the order)
__device__ __forceinline__ float child_xyz(const ApplyParams &A, const float *xyz, int64_t s, int32_t nr, int j) {
    float r = A.rotation[4 * s], x = A.rotation[4 * s + 1], y = A.rotation[4 * s + 2], z = A.rotation[4 * s + 3];
    const float n = sqrtf(((r * r + x * x) + y * y) + z * z);
    r /= n; x /= n; y /= n; z /= n;
    float R0, R1, R2;
    if (j == 0)      { R0 = 1.0f - 2.0f * (y * y + z * z); R1 = 2.0f * (x * y - r * z); R2 = 2.0f * (x * z + r * y); }
    else if (j == 1) { R0 = 2.0f * (x * y + r * z); R1 = 1.0f - 2.0f * (x * x + z * z); R2 = 2.0f * (y * z - r * x); }
    else             { R0 = 2.0f * (x * z - r * y); R1 = 2.0f * (y * z + r * x); R2 = 1.0f - 2.0f * (x * x + y * y); }
    const float *sc = A.scaling + s * A.S;
    const float *nz = A.noise + 3 * (int64_t)nr;
    const float v0 = nz[0] * expf(sc[0]), v1 = nz[1] * expf(sc[A.S == 3 ? 1 : 0]), v2 = nz[2] * expf(sc[A.S == 3 ? 2 : 0]);
    return ((R0 * v0 + R1 * v1) + R2 * v2) + xyz[3 * s + j];
}

__global__ void __launch_bounds__(EDIT_THREADS) edit_apply_kernel(ApplyParams A) {
    const lvdgs_map_edit_column col = A.col[blockIdx.y];
    const int64_t stride = (int64_t)gridDim.x * EDIT_THREADS;
    const int64_t first = (int64_t)blockIdx.x * EDIT_THREADS + threadIdx.x;
    const bool words = col.row_bytes % 4 == 0 && ((uintptr_t)col.in | (uintptr_t)col.out) % 4 == 0;
    if (words) {
        const int64_t wpr = col.row_bytes / 4, total = (int64_t)A.n_out * wpr;
        const uint32_t *in = reinterpret_cast<const uint32_t *>(col.in);
        uint32_t *out = reinterpret_cast<uint32_t *>(col.out);
        for (int64_t e = first; e < total; e += stride) {
            const int64_t r = wpr == 1 ? e : e / wpr;
            const int j = (int)(e - r * wpr);
            const int64_t s = A.src[r];
            const uint8_t k = A.kind[r];
            uint32_t v;
            if (k == LVDGS_EDIT_KEEP || col.new_rows == LVDGS_EDIT_COPY || (k == LVDGS_EDIT_CLONE && col.new_rows != LVDGS_EDIT_ZERO)) v = in[s * wpr + j];
            else if (col.new_rows == LVDGS_EDIT_ZERO) v = 0u;
            else if (col.new_rows == LVDGS_EDIT_SCALE) v = __float_as_uint(child_scale(__uint_as_float(in[s * wpr + j])));
            else v = __float_as_uint(child_xyz(A, reinterpret_cast<const float *>(col.in), s, A.noise_row[r], j));
            out[e] = v;
        }
    } else {   // (rows or addresses that are no multiple of four bytes: _COPY and _ZERO columns only, see the host checks)
        const int64_t bpr = col.row_bytes, total = (int64_t)A.n_out * bpr;
        const uint8_t *in = reinterpret_cast<const uint8_t *>(col.in);
        uint8_t *out = reinterpret_cast<uint8_t *>(col.out);
        for (int64_t e = first; e < total; e += stride) {
            const int64_t r = bpr == 1 ? e : e / bpr;
            const int64_t s = A.src[r];
            const bool zero = col.new_rows == LVDGS_EDIT_ZERO && A.kind[r] != LVDGS_EDIT_KEEP;
            out[e] = zero ? (uint8_t)0 : in[s * bpr + (e - r * bpr)];
        }
    }
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_map_edit_scratch_bytes(int32_t num_gaussians) {
    if (num_gaussians < 0) return 0;
    return edit_layout(num_gaussians, nullptr, nullptr);
}

int lvdgs_map_edit_plan(const lvdgs_map_edit_plan_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = edit_check_plan(a)) return e;
    PlanParams P{};
    P.mode = a->mode; P.N = a->num_gaussians; P.S = a->scale_dims; P.capacity = a->capacity; P.seq = a->seq;
    const Spans spans = edit_spans(P.N);
    P.blocks = spans.blocks; P.span = spans.span;
    P.remove = a->mode == LVDGS_EDIT_PRUNE ? a->remove : nullptr;
    P.num_vis = a->num_vis_rows; P.vis_stride = a->vis_stride ? a->vis_stride : 1; P.prune_num = a->prune_num; P.min_kf_id = a->min_kf_id;
    for (int k = 0; k < LVDGS_EDIT_MAX_VIS_ROWS; k++) P.vis[k] = a->vis_rows[k];
    P.kf_id = a->kf_id; P.n_obs = a->n_obs;
    P.accum = a->grad_accum; P.denom = a->denom; P.scaling = a->scaling; P.opacity = a->opacity;
    P.thr = a->grad_threshold; P.dense_extent = a->dense_extent; P.min_opacity = a->min_opacity;
    P.max_screen = a->max_screen_size; P.world_extent = a->world_extent;
    P.src = a->src; P.kind = a->kind; P.noise_row = a->noise_row;
    EditScratch w;
    edit_layout(P.N, &w, a->scratch);
    P.code = w.code; P.counts = w.counts; P.totals = w.totals;
    if (int e = host_block_address(a->host_state, "map edit plan", &P.host)) return e;
    P.host_words = (int64_t)(a->host_bytes / sizeof(int32_t));
    if (P.blocks) {
        if (int e = launch("edit_count", 0, s, edit_count_kernel, dim3(P.blocks), dim3(EDIT_THREADS), 0, P)) return e;
    }
    if (int e = launch("edit_scan", 0, s, edit_scan_kernel, dim3(1), dim3(EDIT_THREADS), 0, P)) return e;
    if (P.blocks) {
        if (int e = launch("edit_write", 0, s, edit_write_kernel, dim3(P.blocks), dim3(EDIT_THREADS), 0, P)) return e;
    }
    if (int e = launch("edit_publish", 0, s, edit_publish_kernel, dim3(1), dim3(WAVE), 0, P)) return e;
    return LVDGS_OK;
}

int lvdgs_map_edit_apply(const lvdgs_map_edit_apply_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = edit_check_apply(a)) return e;
    if (a->num_columns == 0 || a->n_out == 0) return LVDGS_OK;
    ApplyParams A{};
    A.N = a->num_gaussians; A.n_out = a->n_out; A.S = a->scale_dims; A.n_sel = a->n_split_sel;
    A.src = a->src; A.kind = a->kind; A.noise_row = a->noise_row;
    A.noise = a->noise; A.scaling = a->scaling; A.rotation = a->rotation;
    int64_t most = 0;   // elements of the widest column: the grid's x extent, capped (the kernel strides)
    for (int c = 0; c < a->num_columns; c++) {
        A.col[c] = a->columns[c];
        const int64_t elems = (int64_t)a->n_out * (a->columns[c].row_bytes % 4 == 0 ? a->columns[c].row_bytes / 4 : a->columns[c].row_bytes);
        if (elems > most) most = elems;
    }
    int64_t gx = (most + EDIT_THREADS - 1) / EDIT_THREADS;
    if (gx > 2048) gx = 2048;
    if (int e = launch("edit_apply", 0, s, edit_apply_kernel, dim3((unsigned)gx, (unsigned)a->num_columns), dim3(EDIT_THREADS), 0, A)) return e;
    return LVDGS_OK;
}

}  // extern "C"
