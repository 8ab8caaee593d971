// Culling a mesh to what the evaluated frames observed: which vertices some view sees, and the kept part of the mesh in the original
// order (rules, arithmetic, margins and the host block: include/lvdgs.h, "Mesh scoring").
//
// lvdgs_mesh_visibility: one launch, one thread per vertex.  Steps 1 and 2 are tsdf_rule.hpp's tsdf_pixel and the depth test its
// tsdf_seen with occlusion_eps as the truncation: the project keeps one statement of the projection.  A view's intrinsics come from the
// kernel's argument block and its pose through loads at a wave-uniform address in front of the kernel's only store, so both sit in
// scalar registers; a view that no lane of a wave projects into is skipped by the wave, and a wave whose vertices are all seen stops.
//
// lvdgs_mesh_cull: a clear and six launches.  Faces and vertices are two span scans (spans.hpp) that share one scan launch: integer
// decisions only, no atomic decides a position, two calls give the same bytes.  The used-vertex plane is written with plain stores of
// 1 -- many lanes storing the same byte is no race that matters.
//
// Built like every file here with -ffp-contract=off and without fast-math: the float32 expressions of the header are evaluated as
// written, the divisions IEEE-rounded, and a NumPy float32 restatement gives the same bits.
#include <cmath>

#include "common.hpp"
#include "device_utils.hpp"
#include "spans.hpp"
#include "tsdf_rule.hpp"

namespace lvdgs {
namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_MAX_BLOCKS = 2048;   // spans of the compaction passes

// ---------------------------------------------------------------- visibility ----

struct VisParams {
    uint32_t V;
    int count;
    float eps;
    const float *vertices;
    uint8_t *seen;
    TsdfView v[LVDGS_TSDF_MAX_VIEWS];
};

__global__ void __launch_bounds__(MC_THREADS) mesh_visibility_kernel(VisParams P) {
    const uint32_t i = blockIdx.x * MC_THREADS + threadIdx.x;
    const bool valid = i < P.V;
    const size_t at3 = 3 * (size_t)(valid ? i : 0u);
    const float px = P.vertices[at3], py = P.vertices[at3 + 1], pz = P.vertices[at3 + 2];
    bool open = valid && P.seen[valid ? i : 0u] == 0;   // still to be decided by a view
    bool seen = false;
    for (int v = 0; v < P.count; v++) {                 // (uniform)
        if (!__any(open)) break;
        const TsdfView &V = P.v[v];
        float R[9], T[3];
#pragma unroll
        for (int q = 0; q < 9; q++) R[q] = V.R[q];
#pragma unroll
        for (int q = 0; q < 3; q++) T[q] = V.T[q];
        const TsdfPixel at = tsdf_pixel(V, R, T, px, py, pz);
        const bool ok = open && at.ok;
        if (!__any(ok)) continue;                       // (a wave's vertices outside this view)
        bool sees;
        if (V.depth == nullptr) {                       // (uniform) frustum only
            sees = ok && at.z <= V.dtrunc;
        } else {
            const int pix = ok ? at.pix : 0;            // pixel 0 stands in: the gathers need no branch
            const float d = V.depth[pix];
            const uint8_t m = V.mask ? V.mask[pix] : (uint8_t)1;
            float sdf;
            sees = ok && tsdf_seen(V, P.eps, d, m, at.z, &sdf);
        }
        seen = seen || sees;
        open = open && !sees;
    }
    if (seen) P.seen[i] = 1;
}

// ---------------------------------------------------------------- compaction ----

struct CullParams {
    uint32_t V, F, vspan, fspan;   // spans: elements per workgroup, multiples of MC_THREADS
    int any;                       // the face rule
    uint32_t seq;
    const float *vertices, *vcolors;
    const int32_t *faces;
    const uint8_t *seen;
    float *out_vertices, *out_colors;
    int32_t *out_faces, *vertex_origin, *face_origin;
    uint8_t *used;                 // V: some kept face references the vertex
    uint8_t *keep;                 // F: the face is kept
    int32_t *newindex;             // V: a kept vertex's new number
    uint32_t *vcount, *fcount;     // MC_MAX_BLOCKS each: per span, then what lies in front of the span
    uint32_t *totals;              // [0] vertices, [1] faces
    int32_t *host;
};

__global__ void __launch_bounds__(MC_THREADS) cull_faces_flag_kernel(CullParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(P.F, P.fspan, blockIdx.x);
    uint32_t mine = 0;
    for (uint32_t f = r.begin + threadIdx.x; f < r.end; f += MC_THREADS) {
        const int32_t ia = P.faces[3 * (size_t)f], ib = P.faces[3 * (size_t)f + 1], ic = P.faces[3 * (size_t)f + 2];
        bool keep = false;
        if ((uint32_t)ia < P.V && (uint32_t)ib < P.V && (uint32_t)ic < P.V) {
            const bool sa = P.seen[ia] != 0, sb = P.seen[ib] != 0, sc = P.seen[ic] != 0;
            keep = P.any ? (sa || sb || sc) : (sa && sb && sc);
            if (keep) { P.used[ia] = 1; P.used[ib] = 1; P.used[ic] = 1; }
        }
        P.keep[f] = keep ? 1 : 0;
        mine += keep ? 1u : 0u;
    }
    uint32_t total = 0;
    scan_workgroup<MC_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) P.fcount[blockIdx.x] = total;
}

__global__ void __launch_bounds__(MC_THREADS) cull_vertices_count_kernel(CullParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(P.V, P.vspan, blockIdx.x);
    uint32_t mine = 0;
    for (uint32_t s = r.begin + threadIdx.x; s < r.end; s += MC_THREADS) mine += P.used[s] ? 1u : 0u;
    uint32_t total = 0;
    scan_workgroup<MC_THREADS>(mine, sh, &total);
    if (threadIdx.x == 0) P.vcount[blockIdx.x] = total;
}

// One workgroup: the counts of the vblocks and fblocks <= MC_MAX_BLOCKS spans become the rows in front of each (a count is at most
// 2^31 - 1: 32 bits hold every sum).
__global__ void __launch_bounds__(MC_THREADS) cull_scan_kernel(CullParams P, int vblocks, int fblocks) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const uint32_t nv = scan_span_counts<MC_THREADS>(P.vcount, P.vcount, vblocks, 1, sh);
    const uint32_t nf = scan_span_counts<MC_THREADS>(P.fcount, P.fcount, fblocks, 1, sh);
    if (threadIdx.x == 0) { P.totals[0] = nv; P.totals[1] = nf; }
}

__global__ void __launch_bounds__(MC_THREADS) cull_vertices_kernel(CullParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(P.V, P.vspan, blockIdx.x);
    TileWalk<MC_THREADS, uint32_t> walk{P.vcount[blockIdx.x]};
    for (uint32_t tile = r.begin; tile < r.end; tile += MC_THREADS) {   // (uniform)
        const uint32_t s = tile + threadIdx.x;
        const bool kept = s < r.end && P.used[s] != 0;
        const uint32_t row = walk.place(kept ? 1u : 0u, sh);
        if (!kept) continue;                                            // (row < V: the kept vertices in front of s are fewer than s)
        P.newindex[s] = (int32_t)row;
        const size_t in = 3 * (size_t)s, out = 3 * (size_t)row;
#pragma unroll
        for (int x = 0; x < 3; x++) P.out_vertices[out + x] = P.vertices[in + x];
        if (P.out_colors) {
#pragma unroll
            for (int x = 0; x < 3; x++) P.out_colors[out + x] = P.vcolors[in + x];
        }
        if (P.vertex_origin) P.vertex_origin[row] = (int32_t)s;
    }
}

__global__ void __launch_bounds__(MC_THREADS) cull_faces_kernel(CullParams P) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const SpanRange<uint32_t> r = span_range(P.F, P.fspan, blockIdx.x);
    TileWalk<MC_THREADS, uint32_t> walk{P.fcount[blockIdx.x]};
    for (uint32_t tile = r.begin; tile < r.end; tile += MC_THREADS) {   // (uniform)
        const uint32_t f = tile + threadIdx.x;
        const bool kept = f < r.end && P.keep[f] != 0;
        const uint32_t row = walk.place(kept ? 1u : 0u, sh);
        if (!kept) continue;                                            // (a kept face's indices are inside 0 .. V-1 and its vertices kept)
        const size_t in = 3 * (size_t)f, out = 3 * (size_t)row;
#pragma unroll
        for (int x = 0; x < 3; x++) P.out_faces[out + x] = P.newindex[P.faces[in + x]];
        if (P.face_origin) P.face_origin[row] = (int32_t)f;
    }
}

__global__ void cull_publish_kernel(CullParams P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    volatile int32_t *w = P.host;
    w[LVDGS_MESH_CULL_N_VERTICES] = (int32_t)P.totals[0];
    w[LVDGS_MESH_CULL_N_FACES] = (int32_t)P.totals[1];
    for (int j = LVDGS_MESH_CULL_N_FACES + 1; j < (int)(LVDGS_MESH_CULL_HOST_BYTES / sizeof(int32_t)); j++) w[j] = 0;
    seal_host_block(w, LVDGS_MESH_CULL_SEQ, (int32_t)P.seq);
}

size_t cull_layout(size_t V, size_t F, CullParams *P, void *base) {
    Carver<CullParams> c(P, base);
    c(c.v.used, V ? V : 1);
    c(c.v.keep, F ? F : 1);
    c(c.v.newindex, V ? V : 1);
    c(c.v.vcount, MC_MAX_BLOCKS);
    c(c.v.fcount, MC_MAX_BLOCKS);
    c.bytes(c.v.totals, 256);
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

int lvdgs_mesh_visibility(const lvdgs_mesh_visibility_args *a, void *stream) {
    const char *name = "mesh visibility";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    if (a->num_vertices < 0) { set_error("%s: negative count (%lld vertices)", name, (long long)a->num_vertices); return LVDGS_E_INVALID; }
    if (!count_ok(a->num_vertices)) { set_error("%s: a count above 2^31 - 1 (%lld vertices)", name, (long long)a->num_vertices); return LVDGS_E_INVALID; }
    if (int e = tsdf_check_count(name, a->count)) return e;
    if (!(a->occlusion_eps >= 0.f) || !std::isfinite(a->occlusion_eps)) {
        set_error("%s: occlusion_eps is %g, it must be finite and not negative", name, a->occlusion_eps); return LVDGS_E_RANGE;
    }
    if (a->num_vertices > 0 && (!a->vertices || !a->seen)) { set_error("%s: vertices / seen is NULL", name); return LVDGS_E_INVALID; }
    if (a->count > 0 && !a->views) { set_error("%s: view list is NULL", name); return LVDGS_E_INVALID; }
    VisParams P{};
    for (int v = 0; v < a->count; v++) {   // (tsdf_pack_views refuses a view without depth: not this call)
        const lvdgs_tsdf_view *w = a->views[v];
        if (int e = check_view(name, v, w, false)) return e;
        P.v[v] = TsdfView{w->width, w->height, w->fx, w->fy, w->cx, w->cy, w->depth_min, w->depth_trunc, w->R, w->T, w->depth, nullptr,
                          w->depth ? w->mask : nullptr};
    }
    if (a->num_vertices == 0 || a->count == 0) return LVDGS_OK;
    P.V = (uint32_t)a->num_vertices; P.count = a->count; P.eps = a->occlusion_eps;
    P.vertices = a->vertices; P.seen = a->seen;
    hipStream_t s = (hipStream_t)stream;
    if (int e = launch("mesh_visibility", 0, s, mesh_visibility_kernel, dim3((unsigned)(((int64_t)P.V + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

size_t lvdgs_mesh_cull_scratch_bytes(int64_t num_vertices, int64_t num_faces) {
    if (!count_ok(num_vertices) || !count_ok(num_faces)) return 0;
    return cull_layout((size_t)num_vertices, (size_t)num_faces, nullptr, nullptr);
}

int lvdgs_mesh_cull(const lvdgs_mesh_cull_args *a, void *stream) {
    const char *name = "mesh cull";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    if (a->num_vertices < 0 || a->num_faces < 0) {
        set_error("%s: negative count (%lld vertices, %lld faces)", name, (long long)a->num_vertices, (long long)a->num_faces); return LVDGS_E_INVALID;
    }
    if (!count_ok(a->num_vertices) || !count_ok(a->num_faces)) {
        set_error("%s: a count above 2^31 - 1 (%lld vertices, %lld faces)", name, (long long)a->num_vertices, (long long)a->num_faces);
        return LVDGS_E_INVALID;
    }
    if (a->face_rule != LVDGS_MESH_CULL_ALL && a->face_rule != LVDGS_MESH_CULL_ANY) {
        set_error("%s: face_rule %d is neither LVDGS_MESH_CULL_ALL nor LVDGS_MESH_CULL_ANY", name, a->face_rule); return LVDGS_E_INVALID;
    }
    const size_t V = (size_t)a->num_vertices, F = (size_t)a->num_faces;
    if (V > 0 && (!a->vertices || !a->seen || !a->out_vertices)) { set_error("%s: vertices / seen / out_vertices is NULL", name); return LVDGS_E_INVALID; }
    if (F > 0 && (!a->faces || !a->out_faces)) { set_error("%s: faces / out_faces is NULL", name); return LVDGS_E_INVALID; }
    if (!a->host_state || !a->scratch) { set_error("%s: host_state / scratch is NULL", name); return LVDGS_E_INVALID; }
    if (a->out_colors && !a->vertex_colors) { set_error("%s: out_colors asked for without vertex_colors", name); return LVDGS_E_INVALID; }
    CullParams P{};
    const size_t need = cull_layout(V, F, &P, a->scratch);
    if (a->scratch_bytes < need) { set_error("%s: scratch too small", name); return LVDGS_E_INVALID; }
    if ((uintptr_t)a->scratch & 3u) { set_error("%s: scratch must be 4-byte aligned", name); return LVDGS_E_INVALID; }
    const ByteRange in[] = {{"vertices", a->vertices, V * 12}, {"vertex_colors", a->vertex_colors, V * 12}, {"faces", a->faces, F * 12},
                            {"seen", a->seen, V}, {"scratch", a->scratch, need}};
    const ByteRange out[] = {{"out_vertices", a->out_vertices, V * 12}, {"out_colors", a->out_colors, V * 12}, {"out_faces", a->out_faces, F * 12},
                             {"vertex_origin", a->vertex_origin, V * 4}, {"face_origin", a->face_origin, F * 4}};
    if (int e = check_no_overlap(name, in, sizeof(in) / sizeof(in[0]), out, sizeof(out) / sizeof(out[0]))) return e;
    P.V = (uint32_t)V; P.F = (uint32_t)F; P.any = a->face_rule == LVDGS_MESH_CULL_ANY; P.seq = a->seq;
    P.vertices = a->vertices; P.vcolors = a->vertex_colors; P.faces = a->faces; P.seen = a->seen;
    P.out_vertices = a->out_vertices; P.out_colors = a->out_colors; P.out_faces = a->out_faces;
    P.vertex_origin = a->vertex_origin; P.face_origin = a->face_origin;
    if (int e = host_block_address(a->host_state, name, &P.host)) return e;
    const Spans vs = make_spans(a->num_vertices, MC_THREADS, MC_MAX_BLOCKS, MC_THREADS), fs = make_spans(a->num_faces, MC_THREADS, MC_MAX_BLOCKS, MC_THREADS);
    P.vspan = vs.span; P.fspan = fs.span;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(MC_THREADS);
    if (V > 0 && F > 0) {   // (without faces nothing reads the plane)
        ProfScope ps("mesh_cull_clear", s);
        if (int e = check_hip(hipMemsetAsync(P.used, 0, V, s), "mesh_cull_clear")) return e;
    }
    if (F > 0) {
        if (int e = launch("mesh_cull_flag", 0, s, cull_faces_flag_kernel, dim3(fs.blocks), block, 0, P)) return e;
    }
    const int vblocks = F > 0 ? vs.blocks : 0;   // no face: no vertex is kept
    if (vblocks > 0) {
        if (int e = launch("mesh_cull_count", 0, s, cull_vertices_count_kernel, dim3(vblocks), block, 0, P)) return e;
    }
    if (int e = launch("mesh_cull_scan", 0, s, cull_scan_kernel, dim3(1), block, 0, P, vblocks, fs.blocks)) return e;
    if (vblocks > 0) {
        if (int e = launch("mesh_cull_vertices", 0, s, cull_vertices_kernel, dim3(vblocks), block, 0, P)) return e;
    }
    if (F > 0) {
        if (int e = launch("mesh_cull_faces", 0, s, cull_faces_kernel, dim3(fs.blocks), block, 0, P)) return e;
    }
    if (int e = launch("mesh_cull_publish", 0, s, cull_publish_kernel, dim3(1), dim3(WAVE), 0, P)) return e;
    return LVDGS_OK;
}

}  // extern "C"
