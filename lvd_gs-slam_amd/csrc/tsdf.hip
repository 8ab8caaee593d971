// TSDF fusion of depth maps into a dense volume and a mesh of it by surface nets (rules, arithmetic and the host block:
// include/lvdgs.h, "TSDF fusion").
//
// The rules are tsdf_rule.hpp's, shared with tsdf_blocks.hip: the corner test of a brick, the walk of a thread's samples through the
// views, when a cell is active, which edges give faces, a cell's vertex, a quad's winding, the counts of the host block, and the host's
// checks of planes, constants and views.  This file is the dense storage around them: bricks, rows, strides and spans.
//
// lvdgs_tsdf_integrate: one launch.  A workgroup of 256 threads owns a brick of 64 x 4 x 4 voxels; a thread owns four voxels along x
// (16 lanes span a row of 64: 256 contiguous bytes of a plane), keeps them in registers across the up to 16 views and writes a row
// back only when a view changed it.  Before anything is read, lanes 0 .. count-1 of every wave test one view each against the brick's
// eight corner voxels (brick_may_touch) and a ballot makes the wave-uniform mask of the views the brick is walked for; a brick with an
// empty mask returns without touching memory.
//
// lvdgs_tsdf_mesh: six launches.  Vertices and faces are two span scans (spans.hpp) over the samples that share one scan launch:
// integer decisions only, no atomics, two calls give the same bytes.
//
// Built like every file here with -ffp-contract=off and without fast-math: the float32 expressions of the header are evaluated as
// written, the divisions IEEE-rounded, and a NumPy float32 restatement gives the same bits.
#include "common.hpp"
#include "device_utils.hpp"
#include "spans.hpp"
#include "tsdf_rule.hpp"

namespace lvdgs {
namespace {

constexpr int TSDF_THREADS = 256;
constexpr int BRICK_X = 64, BRICK_Y = 4, BRICK_Z = 4;   // 16 lanes x 4 voxels, 4 rows per wave, 4 waves
constexpr int TSDF_MAX_BLOCKS = 2048;                   // spans of the mesh passes

struct IntegrateParams {
    int nx, ny, nz, count;
    TsdfLattice lat;
    float *tsdf, *weight, *r, *g, *b;
    TsdfView v[LVDGS_TSDF_MAX_VIEWS];
};

// COLOR: the volume has colour planes.  VEC: nx % 4 == 0 and every plane 16-byte aligned -- a thread's four voxels are one float4.
template <bool COLOR, bool VEC>
__global__ void __launch_bounds__(TSDF_THREADS) tsdf_integrate_kernel(IntegrateParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bi = blockIdx.x * BRICK_X, bj = blockIdx.y * BRICK_Y, bk = blockIdx.z * BRICK_Z;
    bool touch = false;
    if (lane < p.count)
        touch = brick_may_touch(p.lat, p.v[lane], bi, min(bi + BRICK_X, p.nx) - 1, bj, min(bj + BRICK_Y, p.ny) - 1, bk, min(bk + BRICK_Z, p.nz) - 1);
    const uint32_t live = (uint32_t)__ballot(touch);   // the same in all four waves
    if (live == 0u) return;

    const int i0 = bi + (lane & 15) * 4, j = bj + (lane >> 4), k = bk + wave;
    if (i0 >= p.nx || j >= p.ny || k >= p.nz) return;
    const int nv = min(4, p.nx - i0);   // (VEC: always 4)
    const int64_t base = (int64_t)i0 + (int64_t)p.nx * ((int64_t)j + (int64_t)p.ny * (int64_t)k);
    float f[4], w[4], cr[4], cg[4], cb[4];
    auto load4 = [&](const float *plane, float (&dst)[4]) {
        if constexpr (VEC) {
            const float4 q = *reinterpret_cast<const float4 *>(plane + base);
            dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) dst[q] = q < nv ? plane[base + q] : 0.f;
        }
    };
    auto store4 = [&](float *plane, const float (&src)[4]) {
        if constexpr (VEC) {
            *reinterpret_cast<float4 *>(plane + base) = make_float4(src[0], src[1], src[2], src[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q < nv) plane[base + q] = src[q];
        }
    };
    load4(p.tsdf, f);
    load4(p.weight, w);
    if constexpr (COLOR) { load4(p.r, cr); load4(p.g, cg); load4(p.b, cb); }

    float px[4], py[4], pz[4];
    bool valid[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        px[q] = p.lat.ox + p.lat.vs * (float)(i0 + q); py[q] = p.lat.oy + p.lat.vs * (float)j; pz[q] = p.lat.oz + p.lat.vs * (float)k;
        valid[q] = q < nv;
    }
    bool changed = false, recoloured = false;
    tsdf_fuse_views<4, COLOR>(p.lat, p.v, p.count, live, px, py, pz, valid, f, w, cr, cg, cb, changed, recoloured);
    if (changed) { store4(p.tsdf, f); store4(p.weight, w); }
    if constexpr (COLOR) {
        if (recoloured) { store4(p.r, cr); store4(p.g, cg); store4(p.b, cb); }
    }
}

// ---------------------------------------------------------------- the mesh ----

struct MeshParams {
    int nx, ny, nz;
    uint32_t n, span;      // samples; samples per workgroup, a multiple of TSDF_THREADS
    float ox, oy, oz, vs;
    const float *tsdf, *weight, *r, *g, *b;
    int vcap, fcap;
    uint32_t seq;
    float *vertices, *colors;
    int32_t *faces;
    uint8_t *flags, *edges;            // n each
    int32_t *cellvert;                 // n: an active cell's vertex number, at its low corner's sample
    uint32_t *vcount, *fcount;         // TSDF_MAX_BLOCKS each: per span; vcount becomes the vertices in front of the span
    unsigned long long *fbase;         // TSDF_MAX_BLOCKS: the faces in front of the span
    unsigned long long *totals;        // [0] vertices, [1] faces
    int32_t *host;
};

struct Sample { int i, j, k; };
__device__ __forceinline__ Sample sample_of(const MeshParams &M, uint32_t s) {
    const uint32_t row = s / (uint32_t)M.nx;
    Sample c;
    c.i = (int)(s - row * (uint32_t)M.nx);
    c.k = (int)(row / (uint32_t)M.ny);
    c.j = (int)(row - (uint32_t)c.k * (uint32_t)M.ny);
    return c;
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_classify_kernel(MeshParams M) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(M.n, M.span, blockIdx.x);
    const uint32_t sx = 1u, sy = (uint32_t)M.nx, sz = (uint32_t)M.nx * (uint32_t)M.ny;
    uint32_t mine = 0;
    for (uint32_t s = r.begin + threadIdx.x; s < r.end; s += TSDF_THREADS) {
        const Sample c = sample_of(M, s);
        const bool obs = M.weight[s] > 0.f, in = M.tsdf[s] < 0.f;
        bool active = false;
        if (c.i < M.nx - 1 && c.j < M.ny - 1 && c.k < M.nz - 1) {
            active = tsdf_cell_active([&](int q) {
                const uint32_t o = s + ((q & 1) ? sx : 0u) + ((q & 2) ? sy : 0u) + ((q & 4) ? sz : 0u);
                return (uint8_t)((M.weight[o] > 0.f ? SAMPLE_OBSERVED : 0) | (M.tsdf[o] < 0.f ? SAMPLE_INSIDE : 0));
            });
        }
        M.flags[s] = (uint8_t)((active ? CELL_ACTIVE : 0) | (in ? SAMPLE_INSIDE : 0) | (obs ? SAMPLE_OBSERVED : 0));
        mine += active ? 1u : 0u;
    }
    uint32_t total = 0;
    scan_workgroup<TSDF_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) M.vcount[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_edges_kernel(MeshParams M) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(M.n, M.span, blockIdx.x);
    const uint32_t sy = (uint32_t)M.nx, sz = (uint32_t)M.nx * (uint32_t)M.ny;
    uint32_t mine = 0;
    for (uint32_t s = r.begin + threadIdx.x; s < r.end; s += TSDF_THREADS) {
        const Sample c = sample_of(M, s);
        const uint8_t fl = M.flags[s];
        const bool in0 = fl & SAMPLE_INSIDE;
        uint32_t e = 0;
        if (fl & CELL_ACTIVE) {   // c2 = the sample's own cell, for every axis; it being a cell puts i, j, k below n - 1
            // an offset of -1 along an axis needs the sample's index there to be at least 1
            auto at = [&](int dx, int dy, int dz) { return s + (uint32_t)dx + (uint32_t)dy * sy + (uint32_t)dz * sz; };
            auto differs = [&](int dx, int dy, int dz) { return ((M.flags[at(dx, dy, dz)] & SAMPLE_INSIDE) != 0) != in0; };
            auto act = [&](int dx, int dy, int dz) {
                return c.i + dx >= 0 && c.j + dy >= 0 && c.k + dz >= 0 && (M.flags[at(dx, dy, dz)] & CELL_ACTIVE) != 0;
            };
            e = tsdf_edge_axes(differs, act);
        }
        M.edges[s] = (uint8_t)(e | (in0 ? EDGE_LOW_INSIDE : 0));
        mine += 2u * (uint32_t)__popc(e);
    }
    uint32_t total = 0;
    scan_workgroup<TSDF_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) M.fcount[blockIdx.x] = total;
}

// One workgroup: the counts of the `blocks` <= TSDF_MAX_BLOCKS spans become the rows in front of each.  A round's sum fits 32 bits
// (256 spans of at most 2^20 samples, six faces each); the carry over the rounds is 64 bits for the faces.
__global__ void __launch_bounds__(TSDF_THREADS) tsdf_scan_kernel(MeshParams M, int blocks) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t nv = scan_span_counts<TSDF_THREADS>(M.vcount, M.vcount, blocks, 1, sh);
    const unsigned long long nf = scan_span_counts<TSDF_THREADS>(M.fcount, M.fbase, blocks, 1, sh);
    if (threadIdx.x == 0) { M.totals[0] = nv; M.totals[1] = nf; }
}

template <bool COLOR>
__global__ void __launch_bounds__(TSDF_THREADS) tsdf_vertices_kernel(MeshParams M) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(M.n, M.span, blockIdx.x);
    const uint32_t sy = (uint32_t)M.nx, sz = (uint32_t)M.nx * (uint32_t)M.ny;
    TileWalk<TSDF_THREADS, uint32_t> walk{M.vcount[blockIdx.x]};
    for (uint32_t tile = r.begin; tile < r.end; tile += TSDF_THREADS) {   // (uniform)
        const uint32_t s = tile + threadIdx.x;
        const bool act = s < r.end && (M.flags[s] & CELL_ACTIVE);
        const uint32_t row = walk.place(act ? 1u : 0u, sh);
        if (!act) continue;
        M.cellvert[s] = (int32_t)row;
        if (row >= (uint32_t)M.vcap) continue;
        uint32_t o[8];
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            o[q] = s + ((q & 1) ? 1u : 0u) + ((q & 2) ? sy : 0u) + ((q & 4) ? sz : 0u);
            f[q] = M.tsdf[o[q]];
        }
        float mean[3], col[3];
        tsdf_cell_vertex<COLOR>(f, [&](int q, int ch) { return (ch == 0 ? M.r : ch == 1 ? M.g : M.b)[o[q]]; }, mean, col);
        const Sample c = sample_of(M, s);
        const size_t out = (size_t)row * 3;
        M.vertices[out + 0] = M.ox + M.vs * ((float)c.i + mean[0]);
        M.vertices[out + 1] = M.oy + M.vs * ((float)c.j + mean[1]);
        M.vertices[out + 2] = M.oz + M.vs * ((float)c.k + mean[2]);
        if constexpr (COLOR) {
            if (M.colors) {
                M.colors[out + 0] = col[0];
                M.colors[out + 1] = col[1];
                M.colors[out + 2] = col[2];
            }
        }
    }
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_faces_kernel(MeshParams M) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(M.n, M.span, blockIdx.x);
    const uint32_t sy = (uint32_t)M.nx, sz = (uint32_t)M.nx * (uint32_t)M.ny;
    TileWalk<TSDF_THREADS, uint32_t, unsigned long long> walk{M.fbase[blockIdx.x]};
    const unsigned long long cap = (unsigned long long)M.fcap;
    for (uint32_t tile = r.begin; tile < r.end; tile += TSDF_THREADS) {   // (uniform)
        const uint32_t s = tile + threadIdx.x;
        const uint32_t e = s < r.end ? M.edges[s] : 0u;
        unsigned long long row = walk.place(2u * (uint32_t)__popc(e & 7u), sh);
        if (!(e & 7u) || row >= cap) continue;
        const bool low_in = e & EDGE_LOW_INSIDE;
        const int32_t own = M.cellvert[s];
#pragma unroll
        for (int axis = 0; axis < 3; axis++) {
            if (!((e >> axis) & 1u)) continue;
            const TsdfStep b = tsdf_axis_step(axis + 1), c = tsdf_axis_step(axis + 2);
            const uint32_t sb = (uint32_t)b.x + (uint32_t)b.y * sy + (uint32_t)b.z * sz, sc = (uint32_t)c.x + (uint32_t)c.y * sy + (uint32_t)c.z * sz;
            tsdf_write_quad(M.faces, row, cap, low_in, M.cellvert[s - sb - sc], M.cellvert[s - sc], own, M.cellvert[s - sb]);
            row += 2;
        }
    }
}

__global__ void tsdf_publish_kernel(MeshParams M) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    volatile int32_t *w = M.host;
    tsdf_publish_counts(w, M.totals, M.vcap, M.fcap);
    for (int j = LVDGS_TSDF_OVERFLOW + 1; j < (int)(LVDGS_TSDF_HOST_BYTES / sizeof(int32_t)); j++) w[j] = 0;
    seal_host_block(w, LVDGS_TSDF_SEQ, (int32_t)M.seq);
}

size_t mesh_layout(size_t n, MeshParams *M, void *base) {
    Carver<MeshParams> c(M, base);
    c(c.v.flags, n);
    c(c.v.edges, n);
    c(c.v.cellvert, n);
    c(c.v.vcount, TSDF_MAX_BLOCKS);
    c(c.v.fcount, TSDF_MAX_BLOCKS);
    c(c.v.fbase, TSDF_MAX_BLOCKS);
    c.bytes(c.v.totals, 256);
    return c.off;
}

// dims >= least each and at most 2^31 - 1 samples
int check_dims(const char *name, const lvdgs_tsdf_volume &v, int least) {
    if (v.nx < least || v.ny < least || v.nz < least) {
        set_error("%s: volume %dx%dx%d, every dimension must be at least %d", name, v.nx, v.ny, v.nz, least); return LVDGS_E_RANGE;
    }
    if ((int64_t)v.nx * v.ny > INT32_MAX || (int64_t)v.nx * v.ny * v.nz > INT32_MAX) {
        set_error("%s: volume %dx%dx%d has more than 2^31 - 1 cells", name, v.nx, v.ny, v.nz); return LVDGS_E_RANGE;
    }
    return LVDGS_OK;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

int lvdgs_tsdf_integrate(const lvdgs_tsdf_volume *vol, const lvdgs_tsdf_view *const *views, int32_t count, void *stream) {
    const char *name = "tsdf integrate";
    if (!vol) { set_error("%s: volume is NULL", name); return LVDGS_E_INVALID; }
    if (int e = tsdf_check_count(name, count)) return e;
    if (int e = tsdf_check_planes(name, *vol)) return e;
    if (int e = check_dims(name, *vol, 1)) return e;
    if (int e = tsdf_check_constants(name, *vol)) return e;
    const dim3 grid(cdiv(vol->nx, BRICK_X), cdiv(vol->ny, BRICK_Y), cdiv(vol->nz, BRICK_Z));
    if (grid.y > 65535u || grid.z > 65535u) { set_error("%s: ny or nz beyond 262140 (65535 bricks)", name); return LVDGS_E_RANGE; }
    IntegrateParams p{};
    if (int e = tsdf_pack_views(name, views, count, vol->r != nullptr, p.v)) return e;
    if (count == 0) return LVDGS_OK;
    p.nx = vol->nx; p.ny = vol->ny; p.nz = vol->nz; p.count = count;
    p.lat = TsdfLattice{vol->origin[0], vol->origin[1], vol->origin[2], vol->voxel_size, vol->trunc, vol->max_weight};
    p.tsdf = vol->tsdf; p.weight = vol->weight; p.r = vol->r; p.g = vol->g; p.b = vol->b;
    const bool color = vol->r != nullptr;
    const uintptr_t bits = (uintptr_t)vol->tsdf | (uintptr_t)vol->weight | (uintptr_t)vol->r | (uintptr_t)vol->g | (uintptr_t)vol->b;
    const bool vec = vol->nx % 4 == 0 && (bits & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    const auto kernel = color ? (vec ? tsdf_integrate_kernel<true, true> : tsdf_integrate_kernel<true, false>)
                              : (vec ? tsdf_integrate_kernel<false, true> : tsdf_integrate_kernel<false, false>);
    if (int e = launch("tsdf_integrate", 0, s, kernel, grid, dim3(TSDF_THREADS), 0, p)) return e;
    return LVDGS_OK;
}

size_t lvdgs_tsdf_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny > INT32_MAX || (int64_t)nx * ny * nz > INT32_MAX) return 0;
    return mesh_layout((size_t)nx * ny * nz, nullptr, nullptr);
}

int lvdgs_tsdf_mesh(const lvdgs_tsdf_mesh_args *a, void *stream) {
    const char *name = "tsdf mesh";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    const lvdgs_tsdf_volume &vol = a->vol;
    if (int e = tsdf_check_planes(name, vol)) return e;
    if (int e = check_dims(name, vol, 2)) return e;
    if (!positive_finite(vol.voxel_size)) { set_error("%s: voxel_size %g must be finite and positive", name, vol.voxel_size); return LVDGS_E_RANGE; }
    if (a->vertex_capacity < 0 || a->face_capacity < 0) {
        set_error("%s: negative capacity (%d vertices, %d faces)", name, a->vertex_capacity, a->face_capacity); return LVDGS_E_RANGE;
    }
    if (!a->vertices || !a->faces || !a->host_state || !a->scratch) {
        set_error("%s: vertices / faces / host_state / scratch is NULL", name); return LVDGS_E_INVALID;
    }
    if (a->colors && !vol.r) { set_error("%s: colors asked for, the volume has no colour planes", name); return LVDGS_E_INVALID; }
    const size_t n = (size_t)vol.nx * vol.ny * vol.nz;
    MeshParams M{};
    if (a->scratch_bytes < mesh_layout(n, &M, a->scratch)) { set_error("%s: scratch too small", name); return LVDGS_E_INVALID; }
    if ((uintptr_t)a->scratch & 7u) { set_error("%s: scratch must be 8-byte aligned", name); return LVDGS_E_INVALID; }
    M.nx = vol.nx; M.ny = vol.ny; M.nz = vol.nz; M.n = (uint32_t)n;
    M.ox = vol.origin[0]; M.oy = vol.origin[1]; M.oz = vol.origin[2]; M.vs = vol.voxel_size;
    M.tsdf = vol.tsdf; M.weight = vol.weight; M.r = vol.r; M.g = vol.g; M.b = vol.b;
    M.vcap = a->vertex_capacity; M.fcap = a->face_capacity; M.seq = a->seq;
    M.vertices = a->vertices; M.colors = a->colors; M.faces = a->faces;
    if (int e = host_block_address(a->host_state, name, &M.host)) return e;
    const Spans spans = make_spans((int64_t)n, TSDF_THREADS, TSDF_MAX_BLOCKS, TSDF_THREADS);
    const int blocks = spans.blocks;
    M.span = spans.span;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(blocks), block(TSDF_THREADS);
    if (int e = launch("tsdf_classify", 0, s, tsdf_classify_kernel, grid, block, 0, M)) return e;
    if (int e = launch("tsdf_edges", 0, s, tsdf_edges_kernel, grid, block, 0, M)) return e;
    if (int e = launch("tsdf_scan", 0, s, tsdf_scan_kernel, dim3(1), block, 0, M, blocks)) return e;
    if (int e = launch("tsdf_vertices", 0, s, vol.r ? tsdf_vertices_kernel<true> : tsdf_vertices_kernel<false>, grid, block, 0, M)) return e;
    if (int e = launch("tsdf_faces", 0, s, tsdf_faces_kernel, grid, block, 0, M)) return e;
    if (int e = launch("tsdf_publish", 0, s, tsdf_publish_kernel, dim3(1), dim3(WAVE), 0, M)) return e;
    return LVDGS_OK;
}

}  // extern "C"
