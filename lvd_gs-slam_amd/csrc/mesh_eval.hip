// Mesh scoring: area-weighted samples of a triangle mesh and exact nearest neighbours between two point clouds (rules, arithmetic and
// the rows: include/lvdgs.h, "Mesh scoring").
//
// lvdgs_mesh_sample: five launches.  Float64 areas and the maximum per span of faces; then a span scan (spans.hpp) of the integer
// weights q, in 64 bits, whose write pass leaves the inclusive prefix over the weights; one thread per sample (three keys, a binary
// search, one triangle).  Integer decisions only, no atomics: two calls give the same bytes.
//
// lvdgs_cloud_distance: the reference points' box (two launches), a grid decided by one thread, a counting sort of both clouds by
// cell (zero, count, a span scan over the cells, scatter), the search -- a workgroup of ONE wave per cell of queries, the
// cell's neighbourhood staged in LDS 512 points at a time --, and the row (two launches).  The cells are numbered
// x fastest, so the points of a run of cells along x lie side by side in the sorted array and start[] of the run's ends says how
// many there are: a row's or a plane's emptiness costs two loads.  The order of the points inside a cell depends on how the
// atomics arrive; the result does not: the minimum is exact and ties go to the lowest index.
//
// Built like every file here with -ffp-contract=off and without fast-math: the float32 and float64 expressions of the header are
// evaluated as written, divisions and square roots IEEE-rounded, and a NumPy restatement gives the same bits.
#include <cmath>

#include "common.hpp"
#include "device_utils.hpp"
#include "host_checks.hpp"
#include "spans.hpp"

namespace lvdgs {
namespace {

constexpr int ME_THREADS = 256;
constexpr int ME_MAX_BLOCKS = 2048;   // spans of the sampling passes
typedef unsigned long long u64;

// ---------------------------------------------------------------- sampling ----

__device__ __forceinline__ uint32_t sample_key(u64 i, uint32_t seed_lo, uint32_t seed_hi) {
    return fmix32(fmix32((uint32_t)i + seed_lo) ^ (seed_hi + (uint32_t)(i >> 32)));
}

struct SampleParams {
    uint32_t V, F, n, span;   // span: faces per workgroup, a multiple of ME_THREADS
    uint32_t seed_lo, seed_hi;
    const float *vertices, *vcolors;
    const int32_t *faces;
    float *points, *colors;
    int32_t *face_index;
    lvdgs_mesh_sample_info *info;
    double *area;      // F: the areas, then (the same bytes) the weights q, then the inclusive prefix
    double *bmax;      // ME_MAX_BLOCKS: per span
    u64 *bsum;         // ME_MAX_BLOCKS: per span, then the weights in front of the span
    uint32_t *bcount;  // ME_MAX_BLOCKS: weighted faces per span
    u64 *totals;       // [0] total
};

__global__ void __launch_bounds__(ME_THREADS) sample_area_kernel(SampleParams P) {
    __shared__ double s_max[ME_THREADS / 64];
    const SpanRange<uint32_t> r = span_range(P.F, P.span, blockIdx.x);
    double mine = 0.0;
    for (uint32_t f = r.begin + threadIdx.x; f < r.end; f += ME_THREADS) {
        const int32_t ia = P.faces[3 * (size_t)f], ib = P.faces[3 * (size_t)f + 1], ic = P.faces[3 * (size_t)f + 2];
        double A = 0.0;
        if ((uint32_t)ia < P.V && (uint32_t)ib < P.V && (uint32_t)ic < P.V) {
            const float *a = P.vertices + 3 * (size_t)ia, *b = P.vertices + 3 * (size_t)ib, *c = P.vertices + 3 * (size_t)ic;
            const double ax = a[0], ay = a[1], az = a[2];
            const double e1x = (double)b[0] - ax, e1y = (double)b[1] - ay, e1z = (double)b[2] - az;
            const double e2x = (double)c[0] - ax, e2y = (double)c[1] - ay, e2z = (double)c[2] - az;
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            A = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
            if (!(A > 0.0 && A < (double)__builtin_inf())) A = 0.0;
        }
        P.area[f] = A;
        mine = fmax(mine, A);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine = fmax(mine, __shfl_xor(mine, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = s_max[0];
        for (int w = 1; w < ME_THREADS / 64; w++) m = fmax(m, s_max[w]);
        P.bmax[blockIdx.x] = m;
    }
}

__global__ void __launch_bounds__(ME_THREADS) sample_weight_kernel(SampleParams P, int blocks) {
    __shared__ double s_max[ME_THREADS / 64];
    __shared__ u64 sh[SCAN_WORDS];
    __shared__ uint32_t sh32[SCAN_WORDS];
    double amax = 0.0;
    for (int b = threadIdx.x; b < blocks; b += ME_THREADS) amax = fmax(amax, P.bmax[b]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmax(amax, __shfl_xor(amax, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = s_max[0];
    for (int w = 1; w < ME_THREADS / 64; w++) amax = fmax(amax, s_max[w]);

    const SpanRange<uint32_t> r = span_range(P.F, P.span, blockIdx.x);
    u64 mine = 0;
    uint32_t weighted = 0;
    u64 *q = reinterpret_cast<u64 *>(P.area);
    for (uint32_t f = r.begin + threadIdx.x; f < r.end; f += ME_THREADS) {
        const double A = P.area[f];
        const u64 w = A > 0.0 ? (u64)floor(A / amax * 4294967296.0) : 0ull;   // (amax >= A > 0)
        q[f] = w;
        mine += w;
        weighted += A > 0.0 ? 1u : 0u;
    }
    u64 total = 0;
    uint32_t count = 0;
    scan_workgroup<ME_THREADS>(mine, sh, &total);
    scan_workgroup<ME_THREADS>(weighted, sh32, &count);
    if (threadIdx.x == 0) { P.bsum[blockIdx.x] = total; P.bcount[blockIdx.x] = count; }
}

// One workgroup: the sums of the `blocks` <= ME_MAX_BLOCKS spans become the weights in front of each; the info row.
__global__ void __launch_bounds__(ME_THREADS) sample_scan_kernel(SampleParams P, int blocks) {
    __shared__ u64 sh[SCAN_WORDS];
    __shared__ uint32_t sh32[SCAN_WORDS];
    const u64 carry = scan_span_counts<ME_THREADS>(P.bsum, P.bsum, blocks, 1, sh);
    const uint32_t weighted = scan_span_counts<ME_THREADS>(P.bcount, P.bcount, blocks, 1, sh32);   // (for its total alone)
    if (threadIdx.x == 0) {
        P.totals[0] = carry;
        P.info->flags = carry == 0ull ? LVDGS_MESH_SAMPLE_NO_AREA : 0u;
        P.info->n_weighted = weighted;
        P.info->total = carry;
    }
}

__global__ void __launch_bounds__(ME_THREADS) sample_prefix_kernel(SampleParams P) {
    __shared__ u64 sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(P.F, P.span, blockIdx.x);
    u64 *q = reinterpret_cast<u64 *>(P.area);
    TileWalk<ME_THREADS, u64> walk{P.bsum[blockIdx.x]};
    for (uint32_t tile = r.begin; tile < r.end; tile += ME_THREADS) {   // (uniform)
        const uint32_t f = tile + threadIdx.x;
        const u64 w = f < r.end ? q[f] : 0ull;
        const u64 before = walk.place(w, sh);
        if (f < r.end) q[f] = before + w;
    }
}

__global__ void __launch_bounds__(ME_THREADS) sample_points_kernel(SampleParams P) {
    const u64 total = P.totals[0];
    if (total == 0ull) return;
    const u64 *prefix = reinterpret_cast<const u64 *>(P.area);
    for (uint32_t k = blockIdx.x * ME_THREADS + threadIdx.x; k < P.n; k += gridDim.x * ME_THREADS) {
        const u64 i0 = 3ull * k;
        const uint32_t k0 = sample_key(i0, P.seed_lo, P.seed_hi), k1 = sample_key(i0 + 1, P.seed_lo, P.seed_hi),
                       k2 = sample_key(i0 + 2, P.seed_lo, P.seed_hi);
        const u64 t = __umul64hi(((u64)k0 << 32) | (u64)k1, total);   // < total
        uint32_t lo = 0, hi = P.F - 1;                               // the first f with prefix[f] > t: prefix[F-1] = total > t
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (prefix[mid] > t) hi = mid; else lo = mid + 1;
        }
        const uint32_t f = lo;   // q_f > 0, so the face's indices are inside 0 .. V-1
        const int32_t ia = P.faces[3 * (size_t)f], ib = P.faces[3 * (size_t)f + 1], ic = P.faces[3 * (size_t)f + 2];
        uint32_t u1 = k2 >> 8, u2 = k1 & 0xFFFFFFu;
        if (u1 + u2 > (1u << 24)) { u1 = (1u << 24) - u1; u2 = (1u << 24) - u2; }   // the fold, in integers
        const float r1 = (float)u1 * 5.9604644775390625e-8f, r2 = (float)u2 * 5.9604644775390625e-8f;   // (2^-24: exact)
        const float *a = P.vertices + 3 * (size_t)ia, *b = P.vertices + 3 * (size_t)ib, *c = P.vertices + 3 * (size_t)ic;
#pragma unroll
        for (int x = 0; x < 3; x++) P.points[3 * (size_t)k + x] = (a[x] + r1 * (b[x] - a[x])) + r2 * (c[x] - a[x]);
        if (P.colors) {
            const float *ca = P.vcolors + 3 * (size_t)ia, *cb = P.vcolors + 3 * (size_t)ib, *cc = P.vcolors + 3 * (size_t)ic;
#pragma unroll
            for (int x = 0; x < 3; x++) P.colors[3 * (size_t)k + x] = (ca[x] + r1 * (cb[x] - ca[x])) + r2 * (cc[x] - ca[x]);
        }
        if (P.face_index) P.face_index[k] = (int32_t)f;
    }
}

size_t sample_layout(size_t F, SampleParams *P, void *base) {
    Carver<SampleParams> c(P, base);
    c(c.v.area, F);
    c(c.v.bmax, ME_MAX_BLOCKS);
    c(c.v.bsum, ME_MAX_BLOCKS);
    c(c.v.bcount, ME_MAX_BLOCKS);
    c.bytes(c.v.totals, 256);
    return c.off;
}

// ---------------------------------------------------------------- the search ----

constexpr int CD_SEARCH_THREADS = 64;    // one wave per cell: a cell holds a few dozen queries, and a wave that has none only waits
constexpr int CD_TILE = 512;             // reference points staged at a time: 8 KiB of LDS, twenty workgroups per CU
constexpr int CD_BOX_BLOCKS = 1024;      // partial boxes
constexpr int CD_SCAN_BLOCKS = 256;      // spans of cells of the scan over the cells: one round of the single workgroup's scan
constexpr int CD_SEARCH_BLOCKS = 16384;  // workgroups of the search, each takes cells blockIdx.x, + gridDim.x, ...
constexpr int CD_SUM_BLOCKS = 512;       // partial rows
constexpr int64_t CD_MAX_CELLS = 1 << 22;
constexpr float CD_SHRINK = 0.99999f;    // L * CD_SHRINK > best: skip (include/lvdgs.h)

struct Grid {   // decided on the device, read by every later launch
    float lo[3], hi[3], h[3], inv_h[3], slop[3];
    int n[3];
    int ncells;
    uint32_t n_ref, flags;
};
struct BoxPartial { float lo[3], hi[3]; uint32_t count, pad; };
struct SumPartial { double s1, s2; uint32_t counted, skipped, below[LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS]; float maxd; uint32_t pad; };
static_assert(sizeof(BoxPartial) == 32 && sizeof(SumPartial) == 48, "scratch layout");
static_assert(sizeof(lvdgs_cloud_distance_row) == LVDGS_CLOUD_DISTANCE_ROW_BYTES, "row layout (include/lvdgs.h)");
static_assert(sizeof(lvdgs_mesh_sample_info) == LVDGS_MESH_SAMPLE_INFO_BYTES, "info layout (include/lvdgs.h)");

struct CloudParams {
    uint32_t M, N;
    const float *queries, *reference;
    int ppc, nthr;
    int64_t budget;          // cells the scratch holds
    float thr[LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS];
    float *d2;               // M: the caller's or the scratch's
    int32_t *idx;            // M: likewise
    lvdgs_cloud_distance_row *row;
    Grid *grid;
    BoxPartial *box;         // CD_BOX_BLOCKS
    uint32_t *cnt[2], *start[2];   // budget + 1 each; [0] reference, [1] queries
    uint32_t *spansum;       // 2 * CD_SCAN_BLOCKS: per span, then the points in front of the span
    float4 *sorted[2];       // N and M: x, y, z, the point's index as bits
    SumPartial *sum;         // CD_SUM_BLOCKS
};

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    const float inf = __builtin_inff();
    return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;   // (NaN fails)
}

// The fold of one partial box per thread over the workgroup, valid in thread 0: wave minima, maxima and sums, then the waves from 0
// up (all exact: any order gives the same box).  s_box: one per wave.
__device__ __forceinline__ BoxPartial empty_box() {
    const float inf = __builtin_inff();
    return BoxPartial{{inf, inf, inf}, {-inf, -inf, -inf}, 0u, 0u};
}
__device__ __forceinline__ void box_join(BoxPartial &b, const BoxPartial &q) {
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], q.lo[a]); b.hi[a] = fmaxf(b.hi[a], q.hi[a]); }
    b.count += q.count;
}
__device__ __forceinline__ BoxPartial workgroup_box(BoxPartial b, BoxPartial *s_box) {
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = wave_min(b.lo[a]); b.hi[a] = wave_max(b.hi[a]); }
    b.count = wave_sum(b.count);
    if ((threadIdx.x & 63) == 0) s_box[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x != 0) return b;
    BoxPartial out = s_box[0];
    for (int w = 1; w < ME_THREADS / 64; w++) box_join(out, s_box[w]);
    return out;
}

__global__ void __launch_bounds__(ME_THREADS) cloud_box_kernel(CloudParams P) {
    __shared__ BoxPartial s_box[ME_THREADS / 64];
    BoxPartial mine = empty_box();
    for (uint32_t j = blockIdx.x * ME_THREADS + threadIdx.x; j < P.N; j += gridDim.x * ME_THREADS) {
        const float x = P.reference[3 * (size_t)j], y = P.reference[3 * (size_t)j + 1], z = P.reference[3 * (size_t)j + 2];
        if (finite3(x, y, z)) box_join(mine, BoxPartial{{x, y, z}, {x, y, z}, 1u, 0u});
    }
    const BoxPartial out = workgroup_box(mine, s_box);
    if (threadIdx.x == 0) P.box[blockIdx.x] = out;
}

// One workgroup: the box of the `blocks` partial boxes, then thread 0 decides the grid.
__global__ void __launch_bounds__(ME_THREADS) cloud_grid_kernel(CloudParams P, int blocks) {
    __shared__ BoxPartial s_box[ME_THREADS / 64];
    const float inf = __builtin_inff();
    BoxPartial mine = empty_box();
    for (int b = threadIdx.x; b < blocks; b += ME_THREADS) box_join(mine, P.box[b]);
    const BoxPartial all = workgroup_box(mine, s_box);
    if (threadIdx.x != 0) return;
    Grid G{};
    for (int a = 0; a < 3; a++) { G.lo[a] = all.lo[a]; G.hi[a] = all.hi[a]; }
    G.n_ref = all.count;
    G.flags = G.n_ref == 0u ? LVDGS_CLOUD_DISTANCE_NO_REFERENCE : 0u;
    if (G.n_ref == 0u) { for (int a = 0; a < 3; a++) G.lo[a] = G.hi[a] = 0.f; }
    // axes with a finite positive extent share the cells; the others get one
    double ext[3], vol = 1.0;
    int axes = 0;
    for (int a = 0; a < 3; a++) {
        const float e = G.hi[a] - G.lo[a];
        ext[a] = (e > 0.f && e < inf) ? (double)e : 0.0;
        if (ext[a] > 0.0) { vol *= ext[a]; axes++; }
        G.n[a] = 1;
    }
    const double budget = (double)P.budget;
    double target = (double)G.n_ref / (double)(P.ppc > 0 ? P.ppc : LVDGS_CLOUD_DISTANCE_POINTS_PER_CELL);
    target = fmin(fmax(target, 1.0), budget);
    if (axes > 0) {
        double h = pow(vol / target, 1.0 / (double)axes);
        if (!(h > 0.0) || !(h < (double)__builtin_inf())) h = fmax(fmax(ext[0], ext[1]), ext[2]);
        for (int it = 0; it < 64; it++) {
            double cells = 1.0;
            for (int a = 0; a < 3; a++) {
                if (ext[a] > 0.0) G.n[a] = (int)fmin(floor(ext[a] / h) + 1.0, (double)LVDGS_CLOUD_DISTANCE_MAX_DIM);
                cells *= (double)G.n[a];
            }
            if (cells <= budget) break;
            h *= 1.1;
        }
        while ((double)G.n[0] * (double)G.n[1] * (double)G.n[2] > budget) {   // (ends: every halving shrinks the largest count)
            const int big = G.n[0] >= G.n[1] && G.n[0] >= G.n[2] ? 0 : G.n[1] >= G.n[2] ? 1 : 2;
            G.n[big] = (G.n[big] + 1) / 2;
        }
    }
    for (int a = 0; a < 3; a++) {
        const float e = (float)ext[a];
        G.h[a] = G.n[a] > 1 ? e / (float)G.n[a] : 0.f;
        G.inv_h[a] = G.n[a] > 1 ? (float)G.n[a] / e : 0.f;
        G.slop[a] = G.h[a] * 0.00390625f + 1e-6f * (fabsf(G.lo[a]) + fabsf(G.hi[a]));
    }
    G.ncells = G.n[0] * G.n[1] * G.n[2];
    *P.grid = G;
}

__device__ __forceinline__ int cell_axis(const Grid &G, int a, float p) {
    const float t = (p - G.lo[a]) * G.inv_h[a];
    return (int)fminf(fmaxf(t, 0.f), (float)(G.n[a] - 1));   // (a NaN -- infinity times 0 -- gives 0)
}
__device__ __forceinline__ int cell_of(const Grid &G, float x, float y, float z) {
    return cell_axis(G, 0, x) + G.n[0] * (cell_axis(G, 1, y) + G.n[1] * cell_axis(G, 2, z));
}
// the planes of cell c along axis a: the box's own faces at the ends
__device__ __forceinline__ float cell_low(const Grid &G, int a, int c) { return c == 0 ? G.lo[a] : G.lo[a] + (float)c * G.h[a]; }
__device__ __forceinline__ float cell_high(const Grid &G, int a, int c) { return c == G.n[a] - 1 ? G.hi[a] : G.lo[a] + (float)(c + 1) * G.h[a]; }
// how far q lies outside cells c0 .. c1 along axis a, at least (0 inside); the planes moved outward by the slop
__device__ __forceinline__ float axis_gap(const Grid &G, int a, int c0, int c1, float q) {
    return fmaxf(fmaxf((cell_low(G, a, c0) - G.slop[a]) - q, q - (cell_high(G, a, c1) + G.slop[a])), 0.f);
}

__global__ void __launch_bounds__(ME_THREADS) cloud_zero_kernel(CloudParams P) {
    const uint32_t n = (uint32_t)P.grid->ncells + 1u;
    for (uint32_t c = blockIdx.x * ME_THREADS + threadIdx.x; c < n; c += gridDim.x * ME_THREADS) { P.cnt[0][c] = 0u; P.cnt[1][c] = 0u; }
}

// blockIdx.y: 0 the reference points, 1 the queries.  A query with a non-finite coordinate, and every query when there is no
// reference point, gets its result here and no cell.
__global__ void __launch_bounds__(ME_THREADS) cloud_count_kernel(CloudParams P) {
    const Grid &G = *P.grid;
    const int which = blockIdx.y;
    const uint32_t n = which ? P.M : P.N;
    const float *pts = which ? P.queries : P.reference;
    const bool no_ref = G.n_ref == 0u;
    for (uint32_t i = blockIdx.x * ME_THREADS + threadIdx.x; i < n; i += gridDim.x * ME_THREADS) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (!finite3(x, y, z) || no_ref) {
            if (which) { P.d2[i] = __builtin_inff(); P.idx[i] = -1; }
            continue;
        }
        atomicAdd(&P.cnt[which][cell_of(G, x, y, z)], 1u);
    }
}

// the span scan over the cells, for both clouds (blockIdx.y).  The host does not know the cell count: always CD_SCAN_BLOCKS spans, the
// trailing ones empty, of a length decided here
__device__ __forceinline__ uint32_t cell_span(uint32_t ncells) { return span_length(ncells, CD_SCAN_BLOCKS, ME_THREADS); }
__global__ void __launch_bounds__(ME_THREADS) cloud_span_sum_kernel(CloudParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t ncells = (uint32_t)P.grid->ncells;
    const SpanRange<uint32_t> r = span_range(ncells, cell_span(ncells), blockIdx.x);
    const uint32_t *cnt = P.cnt[blockIdx.y];
    uint32_t mine = 0;
    for (uint32_t c = r.begin + threadIdx.x; c < r.end; c += ME_THREADS) mine += cnt[c];
    uint32_t total = 0;
    scan_workgroup<ME_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) P.spansum[blockIdx.y * CD_SCAN_BLOCKS + blockIdx.x] = total;
}
__global__ void __launch_bounds__(ME_THREADS) cloud_span_scan_kernel(CloudParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t ncells = (uint32_t)P.grid->ncells;
    for (int which = 0; which < 2; which++) {
        uint32_t *s = P.spansum + which * CD_SCAN_BLOCKS;
        const uint32_t total = scan_span_counts<ME_THREADS>(s, s, CD_SCAN_BLOCKS, 1, sh);
        if (threadIdx.x == 0) P.start[which][ncells] = total;
    }
}
__global__ void __launch_bounds__(ME_THREADS) cloud_span_write_kernel(CloudParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t ncells = (uint32_t)P.grid->ncells;
    const SpanRange<uint32_t> r = span_range(ncells, cell_span(ncells), blockIdx.x);
    const uint32_t *cnt = P.cnt[blockIdx.y];
    uint32_t *start = P.start[blockIdx.y];
    TileWalk<ME_THREADS, uint32_t> walk{P.spansum[blockIdx.y * CD_SCAN_BLOCKS + blockIdx.x]};
    for (uint32_t tile = r.begin; tile < r.end; tile += ME_THREADS) {   // (uniform)
        const uint32_t c = tile + threadIdx.x;
        const uint32_t at = walk.place(c < r.end ? cnt[c] : 0u, sh);
        if (c < r.end) start[c] = at;
    }
}

// a point's slot: its cell's start plus what is left of the cell's count (the counts end at zero)
__global__ void __launch_bounds__(ME_THREADS) cloud_scatter_kernel(CloudParams P) {
    const Grid &G = *P.grid;
    if (G.n_ref == 0u) return;
    const int which = blockIdx.y;
    const uint32_t n = which ? P.M : P.N;
    const float *pts = which ? P.queries : P.reference;
    for (uint32_t i = blockIdx.x * ME_THREADS + threadIdx.x; i < n; i += gridDim.x * ME_THREADS) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (!finite3(x, y, z)) continue;
        const int c = cell_of(G, x, y, z);
        const uint32_t left = atomicSub(&P.cnt[which][c], 1u);              // (1 .. the cell's count)
        const uint32_t slot = P.start[which][c] + (left - 1u);
        if (slot < n) P.sorted[which][slot] = make_float4(x, y, z, __uint_as_float(i));
    }
}

struct Best { float d2; int32_t idx; };
__device__ __forceinline__ void consider(Best &b, float qx, float qy, float qz, const float4 p) {
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int32_t j = (int32_t)__float_as_uint(p.w);
    if (d2 < b.d2 || (d2 == b.d2 && (uint32_t)j < (uint32_t)b.idx)) { b.d2 = d2; b.idx = j; }   // (idx -1: above every index)
}

// A query on its own: planes outward from cell cz, rows outward from cy inside a plane, the run of cells along x that can hold a
// point not farther than the best.  Gaps grow with the distance in cells (the planes lo + c * h are monotone in c, rounding
// included) and the best only shrinks: a direction once skipped stays skipped.
__device__ void sweep(const CloudParams &P, const Grid &G, float qx, float qy, float qz, int cy, int cz, Best &b) {
    const uint32_t *start = P.start[0];
    const float4 *pts = P.sorted[0];
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    bool zdone[2] = {false, false};
    for (int kz = 0; kz < nz && !(zdone[0] && zdone[1]); kz++) {
        for (int sz = 0; sz < 2; sz++) {
            if (zdone[sz] || (kz == 0 && sz == 1)) continue;
            const int z = sz ? cz - kz : cz + kz;
            if (z < 0 || z >= nz) { zdone[sz] = true; continue; }
            const float gz = axis_gap(G, 2, z, z, qz);
            if ((gz * gz) * CD_SHRINK > b.d2) { zdone[sz] = true; continue; }
            const uint32_t plane = (uint32_t)z * (uint32_t)ny * (uint32_t)nx;
            if (start[plane + (uint32_t)ny * (uint32_t)nx] == start[plane]) continue;   // no point in the plane
            bool ydone[2] = {false, false};
            for (int ky = 0; ky < ny && !(ydone[0] && ydone[1]); ky++) {
                for (int sy = 0; sy < 2; sy++) {
                    if (ydone[sy] || (ky == 0 && sy == 1)) continue;
                    const int y = sy ? cy - ky : cy + ky;
                    if (y < 0 || y >= ny) { ydone[sy] = true; continue; }
                    const float gy = axis_gap(G, 1, y, y, qy);
                    const float row2 = gy * gy + gz * gz;
                    if (row2 * CD_SHRINK > b.d2) { ydone[sy] = true; continue; }
                    const uint32_t row = plane + (uint32_t)y * (uint32_t)nx;
                    if (start[row + (uint32_t)nx] == start[row]) continue;               // no point in the row
                    // cells along x that may hold a point with d2 <= best: those within r of q, widened by a cell on either side
                    int xa = 0, xb = nx - 1;
                    if (nx > 1 && b.d2 < __builtin_inff()) {
                        const float r = sqrtf(fmaxf(b.d2 - row2 * CD_SHRINK, 0.f)) * 1.0001f + G.slop[0];
                        xa = max(cell_axis(G, 0, qx - r) - 1, 0);
                        xb = min(cell_axis(G, 0, qx + r) + 1, nx - 1);
                    }
                    const uint32_t first = start[row + (uint32_t)xa], last = start[row + (uint32_t)xb + 1u];
                    for (uint32_t s = first; s < last; s++) consider(b, qx, qy, qz, pts[s]);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(CD_SEARCH_THREADS) cloud_search_kernel(CloudParams P) {
    __shared__ float4 s_tile[CD_TILE];
    __shared__ uint32_t s_begin[9], s_pre[10];
    const Grid &G = *P.grid;
    if (G.n_ref == 0u) return;
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const uint32_t *start_r = P.start[0], *start_q = P.start[1];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < G.ncells; c += gridDim.x) {   // (uniform)
        const uint32_t qb = start_q[c], qe = start_q[c + 1];
        if (qb == qe) continue;
        const int cx = c % nx, cy = (c / nx) % ny, cz = c / (nx * ny);
        __syncthreads();   // the cell before is done with the lists
        if (tid < 9) {     // the neighbourhood as nine runs of up to three cells along x
            const int y = cy + tid % 3 - 1, z = cz + tid / 3 - 1;
            uint32_t first = 0, len = 0;
            if (y >= 0 && y < ny && z >= 0 && z < nz) {
                const uint32_t row = ((uint32_t)z * (uint32_t)ny + (uint32_t)y) * (uint32_t)nx;
                first = start_r[row + (uint32_t)max(cx - 1, 0)];
                len = start_r[row + (uint32_t)min(cx + 1, nx - 1) + 1u] - first;
            }
            s_begin[tid] = first;
            s_pre[tid + 1] = len;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            s_pre[0] = 0;
            for (int r = 1; r <= 9; r++) { acc += s_pre[r]; s_pre[r] = acc; }
        }
        __syncthreads();
        const uint32_t T = s_pre[9];
        // what the neighbourhood leaves out lies beyond these planes; no plane on any side: it is the whole grid
        const int cc[3] = {cx, cy, cz};
        for (uint32_t q0 = qb; q0 < qe; q0 += CD_SEARCH_THREADS) {   // (uniform)
            const bool has = q0 + (uint32_t)tid < qe;
            const float4 q = P.sorted[1][has ? q0 + (uint32_t)tid : qb];
            Best b{__builtin_inff(), -1};
            for (uint32_t t0 = 0; t0 < T; t0 += CD_TILE) {      // (uniform)
                const uint32_t cnt = T - t0 < (uint32_t)CD_TILE ? T - t0 : (uint32_t)CD_TILE;
                __syncthreads();   // the round before is done with the tile
                for (uint32_t i = tid; i < cnt; i += CD_SEARCH_THREADS) {
                    const uint32_t g = t0 + i;
                    int r = 0;
                    while (r < 8 && g >= s_pre[r + 1]) r++;
                    s_tile[i] = P.sorted[0][s_begin[r] + (g - s_pre[r])];
                }
                __syncthreads();
                if (has)
                    for (uint32_t i = 0; i < cnt; i++) consider(b, q.x, q.y, q.z, s_tile[i]);
            }
            if (!has) continue;
            float reach = __builtin_inff();
            const float qq[3] = {q.x, q.y, q.z};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (cc[a] - 2 >= 0) reach = fminf(reach, axis_gap(G, a, 0, cc[a] - 2, qq[a]));
                if (cc[a] + 2 <= G.n[a] - 1) reach = fminf(reach, axis_gap(G, a, cc[a] + 2, G.n[a] - 1, qq[a]));
            }
            if (!((reach * reach) * CD_SHRINK > b.d2)) sweep(P, G, q.x, q.y, q.z, cy, cz, b);
            const uint32_t i = __float_as_uint(q.w);
            if (i < P.M) { P.d2[i] = b.d2; P.idx[i] = b.idx; }
        }
    }
}

// The sum of one partial row per thread over the workgroup, valid in thread 0.  The order of the double additions is part of the
// row's bits: the xor-butterfly wave_sum, then thread 0 adds the waves from 0 up.  s_part: one per wave.
__device__ __forceinline__ void sum_join(SumPartial &o, const SumPartial &q) {
    o.s1 += q.s1; o.s2 += q.s2; o.counted += q.counted; o.skipped += q.skipped;
#pragma unroll
    for (int t = 0; t < LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS; t++) o.below[t] += q.below[t];
    o.maxd = fmaxf(o.maxd, q.maxd);
}
__device__ __forceinline__ SumPartial workgroup_sum(SumPartial v, SumPartial *s_part) {
    v.s1 = wave_sum(v.s1); v.s2 = wave_sum(v.s2);
    v.counted = wave_sum(v.counted); v.skipped = wave_sum(v.skipped);
#pragma unroll
    for (int t = 0; t < LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS; t++) v.below[t] = wave_sum(v.below[t]);
    v.maxd = wave_max(v.maxd);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return v;
    SumPartial o = s_part[0];
    for (int w = 1; w < ME_THREADS / 64; w++) sum_join(o, s_part[w]);
    return o;
}

__global__ void __launch_bounds__(ME_THREADS) cloud_sum_kernel(CloudParams P, uint32_t chunk) {
    __shared__ SumPartial s_part[ME_THREADS / 64];
    const SpanRange<uint32_t> r = span_range(P.M, chunk, blockIdx.x);
    SumPartial mine{};
    for (uint32_t i = r.begin + threadIdx.x; i < r.end; i += ME_THREADS) {
        if (P.idx[i] < 0) { mine.skipped++; continue; }
        const float v = P.d2[i], d = sqrtf(v);
        mine.s1 += (double)d; mine.s2 += (double)v;
        mine.counted++;
#pragma unroll
        for (int t = 0; t < LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS; t++) mine.below[t] += (t < P.nthr && d < P.thr[t]) ? 1u : 0u;
        mine.maxd = fmaxf(mine.maxd, d);
    }
    const SumPartial o = workgroup_sum(mine, s_part);
    if (threadIdx.x == 0) P.sum[blockIdx.x] = o;
}

// One workgroup: the partial rows in a fixed order (thread t takes t, t + 256, ...; then workgroup_sum's) and the row.
__global__ void __launch_bounds__(ME_THREADS) cloud_finish_kernel(CloudParams P, int blocks) {
    __shared__ SumPartial s_part[ME_THREADS / 64];
    SumPartial mine{};
    for (int b = threadIdx.x; b < blocks; b += ME_THREADS) sum_join(mine, P.sum[b]);
    const SumPartial o = workgroup_sum(mine, s_part);
    if (threadIdx.x != 0) return;
    lvdgs_cloud_distance_row *row = P.row;
    row->sum_distance = o.s1; row->sum_squared = o.s2;
    row->n_counted = o.counted; row->n_skipped = o.skipped;
    for (int t = 0; t < LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS; t++) row->n_below[t] = o.below[t];
    row->max_distance = o.maxd;
    row->flags = P.grid->flags;
    row->n_reference = P.grid->n_ref;
    row->reserved[0] = row->reserved[1] = row->reserved[2] = 0u;
}

int64_t cell_budget(int64_t N) { return N < 64 ? 64 : N > CD_MAX_CELLS ? CD_MAX_CELLS : N; }

// (d2 and idx have their place in the scratch whether or not the caller brings arrays of their own)
size_t cloud_layout(size_t M, size_t N, CloudParams *P, void *base) {
    Carver<CloudParams> c(P, base);
    const size_t cells = (size_t)cell_budget((int64_t)N) + 1;
    c(c.v.grid, 1);
    c(c.v.box, CD_BOX_BLOCKS);
    for (int w = 0; w < 2; w++) c(c.v.cnt[w], cells);
    for (int w = 0; w < 2; w++) c(c.v.start[w], cells);
    c(c.v.spansum, 2 * CD_SCAN_BLOCKS);
    c(c.v.sorted[0], N ? N : 1);
    c(c.v.sorted[1], M ? M : 1);
    c(c.v.d2, M ? M : 1);
    c(c.v.idx, M ? M : 1);
    c(c.v.sum, CD_SUM_BLOCKS);
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_mesh_sample_scratch_bytes(int64_t num_faces) {
    if (num_faces < 1 || num_faces > (int64_t)INT32_MAX) return 0;
    return sample_layout((size_t)num_faces, nullptr, nullptr);
}

int lvdgs_mesh_sample(const lvdgs_mesh_sample_args *a, void *stream) {
    const char *name = "mesh sample";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    if (a->num_vertices < 0 || a->num_faces < 0 || a->num_samples < 0) {
        set_error("%s: negative count (%lld vertices, %lld faces, %lld samples)", name, (long long)a->num_vertices, (long long)a->num_faces,
                  (long long)a->num_samples);
        return LVDGS_E_INVALID;
    }
    if (!count_ok(a->num_vertices) || !count_ok(a->num_faces) || !count_ok(a->num_samples)) {
        set_error("%s: a count above 2^31 - 1 (%lld vertices, %lld faces, %lld samples)", name, (long long)a->num_vertices,
                  (long long)a->num_faces, (long long)a->num_samples);
        return LVDGS_E_INVALID;
    }
    if (a->num_faces == 0) { set_error("%s: the mesh has no faces", name); return LVDGS_E_INVALID; }
    if (!a->vertices || !a->faces || !a->points || !a->info || !a->scratch) {
        set_error("%s: vertices / faces / points / info / scratch is NULL", name); return LVDGS_E_INVALID;
    }
    if (a->colors && !a->vertex_colors) { set_error("%s: colors asked for without vertex_colors", name); return LVDGS_E_INVALID; }
    SampleParams P{};
    if (a->scratch_bytes < sample_layout((size_t)a->num_faces, &P, a->scratch)) { set_error("%s: scratch too small", name); return LVDGS_E_INVALID; }
    if (((uintptr_t)a->scratch | (uintptr_t)a->info) & 7u) { set_error("%s: scratch and info must be 8-byte aligned", name); return LVDGS_E_INVALID; }
    if (a->num_samples == 0) return LVDGS_OK;
    P.V = (uint32_t)a->num_vertices; P.F = (uint32_t)a->num_faces; P.n = (uint32_t)a->num_samples;
    P.seed_lo = (uint32_t)a->seed; P.seed_hi = (uint32_t)(a->seed >> 32);
    P.vertices = a->vertices; P.vcolors = a->vertex_colors; P.faces = a->faces;
    P.points = a->points; P.colors = a->colors; P.face_index = a->face_index;
    P.info = reinterpret_cast<lvdgs_mesh_sample_info *>(a->info);
    const Spans spans = make_spans(a->num_faces, ME_THREADS, ME_MAX_BLOCKS, ME_THREADS);
    const int blocks = spans.blocks;
    P.span = spans.span;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks), block(ME_THREADS);
    if (int e = launch("mesh_sample_area", 0, s, sample_area_kernel, grid, block, 0, P)) return e;
    if (int e = launch("mesh_sample_weight", 0, s, sample_weight_kernel, grid, block, 0, P, blocks)) return e;
    if (int e = launch("mesh_sample_scan", 0, s, sample_scan_kernel, dim3(1), block, 0, P, blocks)) return e;
    if (int e = launch("mesh_sample_prefix", 0, s, sample_prefix_kernel, grid, block, 0, P)) return e;
    const size_t sample_blocks = ((size_t)P.n + ME_THREADS - 1) / ME_THREADS;
    if (int e = launch("mesh_sample_points", 0, s, sample_points_kernel, dim3((unsigned)(sample_blocks < 8192 ? sample_blocks : 8192)), block, 0, P)) return e;
    return LVDGS_OK;
}

size_t lvdgs_cloud_distance_scratch_bytes(int64_t num_queries, int64_t num_reference) {
    if (!count_ok(num_queries) || !count_ok(num_reference)) return 0;
    return cloud_layout((size_t)num_queries, (size_t)num_reference, nullptr, nullptr);
}

int lvdgs_cloud_distance(const lvdgs_cloud_distance_args *a, void *stream) {
    const char *name = "cloud distance";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    if (a->num_queries < 0 || a->num_reference < 0) {
        set_error("%s: negative count (%lld queries, %lld reference points)", name, (long long)a->num_queries, (long long)a->num_reference);
        return LVDGS_E_INVALID;
    }
    if (!count_ok(a->num_queries) || !count_ok(a->num_reference)) {
        set_error("%s: a count above 2^31 - 1 (%lld queries, %lld reference points)", name, (long long)a->num_queries, (long long)a->num_reference);
        return LVDGS_E_INVALID;
    }
    if (a->num_thresholds < 0 || a->num_thresholds > LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS) {
        set_error("%s: %d thresholds, at most %d", name, a->num_thresholds, LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS); return LVDGS_E_INVALID;
    }
    for (int t = 0; t < a->num_thresholds; t++)
        if (!(a->thresholds[t] >= 0.f) || !std::isfinite(a->thresholds[t])) {
            set_error("%s: threshold %d is %g, it must be finite and not negative", name, t, a->thresholds[t]); return LVDGS_E_INVALID;
        }
    if (!a->queries || !a->out_row || !a->scratch || (!a->reference && a->num_reference > 0)) {
        set_error("%s: queries / reference / out_row / scratch is NULL", name); return LVDGS_E_INVALID;
    }
    CloudParams P{};
    if (a->scratch_bytes < cloud_layout((size_t)a->num_queries, (size_t)a->num_reference, &P, a->scratch)) { set_error("%s: scratch too small", name); return LVDGS_E_INVALID; }
    if (((uintptr_t)a->scratch & 15u) || ((uintptr_t)a->out_row & 7u)) {
        set_error("%s: scratch must be 16-byte and out_row 8-byte aligned", name); return LVDGS_E_INVALID;
    }
    if (a->num_queries == 0) return LVDGS_OK;
    P.M = (uint32_t)a->num_queries; P.N = (uint32_t)a->num_reference;
    P.queries = a->queries; P.reference = a->reference;
    P.ppc = a->points_per_cell; P.nthr = a->num_thresholds;
    P.budget = cell_budget(a->num_reference);
    for (int t = 0; t < LVDGS_CLOUD_DISTANCE_MAX_THRESHOLDS; t++) P.thr[t] = t < a->num_thresholds ? a->thresholds[t] : 0.f;
    if (a->d2) P.d2 = a->d2;
    if (a->idx) P.idx = a->idx;
    P.row = reinterpret_cast<lvdgs_cloud_distance_row *>(a->out_row);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(ME_THREADS);
    auto blocks_for = [](uint32_t n, int most) { const int64_t b = ((int64_t)n + ME_THREADS - 1) / ME_THREADS; return (unsigned)(b < 1 ? 1 : b > most ? most : b); };
    const unsigned box_blocks = P.N ? blocks_for(P.N, CD_BOX_BLOCKS) : 0u;
    if (box_blocks) {
        if (int e = launch("cloud_box", 0, s, cloud_box_kernel, dim3(box_blocks), block, 0, P)) return e;
    }
    if (int e = launch("cloud_grid", 0, s, cloud_grid_kernel, dim3(1), block, 0, P, (int)box_blocks)) return e;
    const unsigned both = blocks_for(P.M > P.N ? P.M : P.N, 4096);
    if (int e = launch("cloud_zero", 0, s, cloud_zero_kernel, dim3(blocks_for((uint32_t)P.budget + 1u, 1024)), block, 0, P)) return e;
    if (int e = launch("cloud_count", 0, s, cloud_count_kernel, dim3(both, 2), block, 0, P)) return e;
    {
        ProfScope ps("cloud_cell_scan", s);
        if (int e = launch_checked("cloud_span_sum", 0, s, cloud_span_sum_kernel, dim3(CD_SCAN_BLOCKS, 2), block, 0, P)) return e;
        if (int e = launch_checked("cloud_span_scan", 0, s, cloud_span_scan_kernel, dim3(1), block, 0, P)) return e;
        if (int e = launch_checked("cloud_span_write", 0, s, cloud_span_write_kernel, dim3(CD_SCAN_BLOCKS, 2), block, 0, P)) return e;
    }
    if (int e = launch("cloud_scatter", 0, s, cloud_scatter_kernel, dim3(both, 2), block, 0, P)) return e;
    if (int e = launch("cloud_search", 0, s, cloud_search_kernel, dim3(CD_SEARCH_BLOCKS), dim3(CD_SEARCH_THREADS), 0, P)) return e;
    const unsigned sum_blocks = blocks_for(P.M, CD_SUM_BLOCKS);
    const uint32_t chunk = (uint32_t)(((uint64_t)P.M + sum_blocks - 1) / sum_blocks);
    if (int e = launch("cloud_sum", 0, s, cloud_sum_kernel, dim3(sum_blocks), block, 0, P, chunk)) return e;
    if (int e = launch("cloud_finish", 0, s, cloud_finish_kernel, dim3(1), block, 0, P, (int)sum_blocks)) return e;
    return LVDGS_OK;
}

}  // extern "C"
