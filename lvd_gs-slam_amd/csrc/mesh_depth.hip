// Depth and face indices rendered from a mesh: a triangle rasteriser with a depth buffer (rule, arithmetic, error bounds: include/lvdgs.h,
// "Mesh scoring").
//
// lvdgs_mesh_depth: a fill of the 64-bit keys, the raster launch, the resolve launch.  In the raster launch one lane owns one face and
// loads its three vertices once; steps 1 and 2 are tsdf_rule.hpp's tsdf_project, the project's one statement of the projection.  A
// view's intrinsics come from the kernel's argument block and its pose through loads at a wave-uniform address, so both sit in scalar
// registers; a view in which no face of a wave has a pixel box is skipped by the wave.  A lane walks its own box while the box holds at
// most MD_LANE_PIXELS pixels; a larger one is handed to the whole wave, one face at a time (ballot, broadcast, the 64 lanes walk the
// box in tiles of 8 x 8 pixels).  The only atomic is the unsigned 64-bit minimum on a pixel's key (zp bits << 32 | face): it decides a
// value, never a position, and a minimum does not depend on arrival order -- two calls give the same bytes, whatever the threshold.
//
// Built like every file here with -ffp-contract=off and without fast-math: the float32 expressions of the header are evaluated as
// written, the divisions IEEE-rounded, and a NumPy float32 restatement gives the same bits.
#include <cmath>

#include "common.hpp"
#include "device_utils.hpp"
#include "tsdf_rule.hpp"

namespace lvdgs {
namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_RESOLVE_BLOCKS = 2048;   // per view: the resolve launch grid-strides the rest
#ifndef LVDGS_MD_LANE_PIXELS
#define LVDGS_MD_LANE_PIXELS 16           // the largest box a lane walks alone (what was tried)
#endif
#ifndef LVDGS_MD_PRELOAD
#define LVDGS_MD_PRELOAD 0                // 1: a plain load of the key in front of the atomic skips a candidate that is not smaller;
#endif                                    // measured, it costs more than it saves
constexpr uint32_t MD_LANE_PIXELS = LVDGS_MD_LANE_PIXELS;
constexpr unsigned long long MD_EMPTY = ~0ull;

struct MdView {
    int W, H;
    float fx, fy, cx, cy, dm, dtrunc;     // dm = fmaxf(depth_min, 0)
    const float *R, *T;
    unsigned long long *keys;             // W*H, in the scratch
    float *depth;
    int32_t *fidx;                        // or null
};

struct MdParams {
    uint32_t V, F;
    int count;
    const float *vertices;
    const int32_t *faces;
    MdView v[LVDGS_TSDF_MAX_VIEWS];
};

// A face as its pixels need it: per edge k (opposite vertex k) the lower-indexed end (ul, vl), the differences to the other end and
// whether the face lists the edge from the higher index to the lower; 1 / z per vertex; the box.
struct MdFace {
    float ul[3], vl[3], du[3], dv[3], rz[3];
    uint32_t flip;                        // bit k
    int i0, j0, i1, j1;                   // the box, inclusive
    uint32_t n;                           // its pixels (0: none)
    uint32_t f;
};

__device__ __forceinline__ void md_edge(MdFace &E, int k, int32_t ia, float ua, float va, int32_t ib, float ub, float vb) {
    const bool flip = ib < ia;
    E.ul[k] = flip ? ub : ua; E.vl[k] = flip ? vb : va;
    E.du[k] = flip ? ua - ub : ub - ua; E.dv[k] = flip ? va - vb : vb - va;
    E.flip |= flip ? 1u << k : 0u;
}

// Pixel (i, j), which lies in the face's box when `inbox`: coverage, depth, and the minimum on the pixel's key.
__device__ __forceinline__ void md_pixel(const MdFace &E, const MdView &W, int i, int j, bool inbox) {
    const float fi = (float)i, fj = (float)j;
    float e[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s = E.du[k] * (fj - E.vl[k]) - E.dv[k] * (fi - E.ul[k]);
        e[k] = ((E.flip >> k) & 1u) ? -s : s;
    }
    const bool covered = inbox && ((e[0] >= 0.f && e[1] >= 0.f && e[2] >= 0.f) || (e[0] <= 0.f && e[1] <= 0.f && e[2] <= 0.f));
    if (!covered) return;                 // (in front of the four divisions: half of a box lies outside its triangle)
    const float A = (e[0] + e[1]) + e[2];
    const float w0 = e[0] / A, w1 = e[1] / A, w2 = e[2] / A;
    const float inv = (w0 * E.rz[0] + w1 * E.rz[1]) + w2 * E.rz[2];
    const float zp = 1.0f / inv;
    if (!(zp > W.dm && zp <= W.dtrunc)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zp) << 32) | (unsigned long long)E.f;
    unsigned long long *at = W.keys + ((size_t)j * (size_t)W.W + (size_t)i);   // (inside the image: the box is clamped to it)
#if LVDGS_MD_PRELOAD
    if (!(key < *at)) return;             // (a stale value is only ever larger: nothing that would have won is skipped)
#endif
    atomicMin(at, key);
}

__global__ void __launch_bounds__(MD_THREADS) mesh_depth_raster_kernel(MdParams P) {
    const uint32_t f = blockIdx.x * MD_THREADS + threadIdx.x;
    const int lane = lane_id();
    const bool exists = f < P.F;
    const size_t at3 = 3 * (size_t)(exists ? f : 0u);
    const int32_t a[3] = {P.faces[at3], P.faces[at3 + 1], P.faces[at3 + 2]};
    const bool valid = exists && (uint32_t)a[0] < P.V && (uint32_t)a[1] < P.V && (uint32_t)a[2] < P.V;
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {         // (vertex 0 stands in: the loads need no branch; the launch needs V > 0)
        const size_t v3 = 3 * (size_t)(valid ? a[k] : 0);
        p[k][0] = P.vertices[v3]; p[k][1] = P.vertices[v3 + 1]; p[k][2] = P.vertices[v3 + 2];
    }
    if (!__any(valid)) return;            // (uniform)
    const float inf = __builtin_inff();
    for (int v = 0; v < P.count; v++) {   // (uniform)
        const MdView &W = P.v[v];
        float R[9], T[3];
#pragma unroll
        for (int q = 0; q < 9; q++) R[q] = W.R[q];
#pragma unroll
        for (int q = 0; q < 3; q++) T[q] = W.T[q];
        float z[3], u[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const TsdfProjected at = tsdf_project(W.fx, W.fy, W.cx, W.cy, R, T, p[k][0], p[k][1], p[k][2]);
            z[k] = at.z; u[k] = at.u; w[k] = at.v;
        }
        bool ok = valid;
#pragma unroll
        for (int k = 0; k < 3; k++) ok = ok && z[k] > W.dm && fabsf(u[k]) < inf && fabsf(w[k]) < inf;
        const float ar = (u[1] - u[0]) * (w[2] - w[0]) - (w[1] - w[0]) * (u[2] - u[0]);
        ok = ok && (ar > 0.f || ar < 0.f);
        const float ulo = ceilf(fminf(fminf(u[0], u[1]), u[2])), uhi = floorf(fmaxf(fmaxf(u[0], u[1]), u[2]));
        const float vlo = ceilf(fminf(fminf(w[0], w[1]), w[2])), vhi = floorf(fmaxf(fmaxf(w[0], w[1]), w[2]));
        const float fW = (float)W.W, fH = (float)W.H;
        ok = ok && ulo < fW && uhi >= 0.f && ulo <= uhi && vlo < fH && vhi >= 0.f && vlo <= vhi;
        if (!__any(ok)) continue;         // (no face of the wave has a pixel in this view)
        MdFace E;
        E.flip = 0; E.f = f;
        E.i0 = ok ? (ulo > 0.f ? (int)ulo : 0) : 0;
        E.j0 = ok ? (vlo > 0.f ? (int)vlo : 0) : 0;
        E.i1 = ok ? (uhi < fW ? (int)uhi : W.W - 1) : 0;
        E.j1 = ok ? (vhi < fH ? (int)vhi : W.H - 1) : 0;
        E.n = ok ? (uint32_t)(E.i1 - E.i0 + 1) * (uint32_t)(E.j1 - E.j0 + 1) : 0u;   // (at most width * height <= 2^31 - 1)
        md_edge(E, 0, a[1], u[1], w[1], a[2], u[2], w[2]);
        md_edge(E, 1, a[2], u[2], w[2], a[0], u[0], w[0]);
        md_edge(E, 2, a[0], u[0], w[0], a[1], u[1], w[1]);
#pragma unroll
        for (int k = 0; k < 3; k++) E.rz[k] = 1.0f / z[k];
        if (E.n > 0 && E.n <= MD_LANE_PIXELS) {
            for (int j = E.j0; j <= E.j1; j++)
                for (int i = E.i0; i <= E.i1; i++) md_pixel(E, W, i, j, true);
        }
        unsigned long long big = __ballot(E.n > MD_LANE_PIXELS);
        while (big) {                     // (uniform) one large face at a time, its box walked in tiles of 8 x 8 pixels, a lane a pixel
            const int src = __builtin_ctzll(big);
            big &= big - 1;
            MdFace B;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                B.ul[k] = __shfl(E.ul[k], src, WAVE); B.vl[k] = __shfl(E.vl[k], src, WAVE);
                B.du[k] = __shfl(E.du[k], src, WAVE); B.dv[k] = __shfl(E.dv[k], src, WAVE);
                B.rz[k] = __shfl(E.rz[k], src, WAVE);
            }
            B.flip = (uint32_t)__shfl((int)E.flip, src, WAVE); B.f = (uint32_t)__shfl((int)E.f, src, WAVE);
            B.i0 = __shfl(E.i0, src, WAVE); B.j0 = __shfl(E.j0, src, WAVE); B.i1 = __shfl(E.i1, src, WAVE); B.j1 = __shfl(E.j1, src, WAVE);
            const uint32_t lx = (uint32_t)lane & 7u, ly = (uint32_t)lane >> 3;
            for (uint32_t ty = (uint32_t)B.j0; ty <= (uint32_t)B.j1; ty += 8)         // (a coordinate is below 2^31 - 1: no wrap)
                for (uint32_t tx = (uint32_t)B.i0; tx <= (uint32_t)B.i1; tx += 8) {
                    const uint32_t i = tx + lx, j = ty + ly;
                    md_pixel(B, W, (int)i, (int)j, i <= (uint32_t)B.i1 && j <= (uint32_t)B.j1);
                }
        }
    }
}

// blockIdx.y: the view.  A key becomes the depth float and the face index; an untouched key 0.0f and -1.
__global__ void __launch_bounds__(MD_THREADS) mesh_depth_resolve_kernel(MdParams P) {
    const MdView &W = P.v[blockIdx.y];
    const uint32_t n = (uint32_t)W.W * (uint32_t)W.H;
    for (uint32_t t = blockIdx.x * MD_THREADS + threadIdx.x; t < n; t += gridDim.x * MD_THREADS) {
        const unsigned long long key = W.keys[t];
        const bool hit = key != MD_EMPTY;
        W.depth[t] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (W.fidx) W.fidx[t] = hit ? (int32_t)(uint32_t)key : -1;
    }
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_mesh_depth_scratch_bytes(int64_t total_pixels) {
    if (total_pixels < 0 || total_pixels > (int64_t)LVDGS_TSDF_MAX_VIEWS * (int64_t)INT32_MAX) return 0;
    return align256((size_t)(total_pixels > 0 ? total_pixels : 1) * sizeof(unsigned long long));
}

int lvdgs_mesh_depth(const lvdgs_mesh_depth_args *a, void *stream) {
    const char *name = "mesh depth";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    if (a->num_vertices < 0 || a->num_faces < 0) {
        set_error("%s: negative count (%lld vertices, %lld faces)", name, (long long)a->num_vertices, (long long)a->num_faces); return LVDGS_E_INVALID;
    }
    if (!count_ok(a->num_vertices) || !count_ok(a->num_faces)) {
        set_error("%s: a count above 2^31 - 1 (%lld vertices, %lld faces)", name, (long long)a->num_vertices, (long long)a->num_faces);
        return LVDGS_E_INVALID;
    }
    const size_t V = (size_t)a->num_vertices, F = (size_t)a->num_faces;
    if (V > 0 && !a->vertices) { set_error("%s: vertices is NULL", name); return LVDGS_E_INVALID; }
    if (F > 0 && !a->faces) { set_error("%s: faces is NULL", name); return LVDGS_E_INVALID; }
    if (int e = tsdf_check_count(name, a->count)) return e;
    if (a->count > 0 && !a->views) { set_error("%s: view list is NULL", name); return LVDGS_E_INVALID; }
    if (a->count > 0 && !a->depth) { set_error("%s: depth list is NULL", name); return LVDGS_E_INVALID; }
    MdParams P{};
    size_t total = 0;
    for (int v = 0; v < a->count; v++) {
        const lvdgs_tsdf_view *w = a->views[v];
        if (int e = check_view(name, v, w, false)) return e;
        if (!a->depth[v]) { set_error("%s: view %d: depth output is NULL", name, v); return LVDGS_E_INVALID; }
        if (a->face_index && !a->face_index[v]) { set_error("%s: view %d: face_index output is NULL", name, v); return LVDGS_E_INVALID; }
        P.v[v] = MdView{w->width, w->height, w->fx, w->fy, w->cx, w->cy, fmaxf(w->depth_min, 0.0f), w->depth_trunc, w->R, w->T,
                        nullptr, a->depth[v], a->face_index ? a->face_index[v] : nullptr};
        total += (size_t)w->width * (size_t)w->height;
    }
    if (a->count == 0) return LVDGS_OK;
    const size_t need = total * sizeof(unsigned long long);
    if (!a->scratch) { set_error("%s: scratch is NULL", name); return LVDGS_E_INVALID; }
    if (a->scratch_bytes < need) { set_error("%s: scratch too small (%zu bytes, %zu needed)", name, a->scratch_bytes, need); return LVDGS_E_INVALID; }
    if ((uintptr_t)a->scratch & 7u) { set_error("%s: scratch must be 8-byte aligned", name); return LVDGS_E_INVALID; }
    {   // an output may overlap no input, not the scratch and no other output
        ByteRange in[3 + 2 * LVDGS_TSDF_MAX_VIEWS], out[2 * LVDGS_TSDF_MAX_VIEWS];
        int ni = 0, no = 0;
        in[ni++] = byte_range("vertices", -1, a->vertices, V * 12);
        in[ni++] = byte_range("faces", -1, a->faces, F * 12);
        in[ni++] = byte_range("scratch", -1, a->scratch, need);
        for (int v = 0; v < a->count; v++) {
            in[ni++] = byte_range("R", v, P.v[v].R, 36);
            in[ni++] = byte_range("T", v, P.v[v].T, 12);
        }
        for (int v = 0; v < a->count; v++) {
            const size_t bytes = (size_t)P.v[v].W * (size_t)P.v[v].H * 4;
            out[no++] = byte_range("depth", v, P.v[v].depth, bytes);
            if (P.v[v].fidx) out[no++] = byte_range("face_index", v, P.v[v].fidx, bytes);
        }
        if (int e = check_no_overlap(name, in, ni, out, no)) return e;
    }
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(a->scratch);
    unsigned most = 1;
    for (int v = 0; v < a->count; v++) {
        const size_t n = (size_t)P.v[v].W * (size_t)P.v[v].H;
        P.v[v].keys = keys;
        keys += n;
        most = std::max(most, (unsigned)std::min<size_t>((n + MD_THREADS - 1) / MD_THREADS, (size_t)MD_RESOLVE_BLOCKS));
    }
    P.V = (uint32_t)V; P.F = (uint32_t)F; P.count = a->count;
    P.vertices = a->vertices; P.faces = a->faces;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps("mesh_depth_fill", s);
        if (int e = check_hip(hipMemsetAsync(a->scratch, 0xFF, need, s), "mesh_depth_fill")) return e;
    }
    if (V > 0 && F > 0) {
        if (int e = launch("mesh_depth_raster", 0, s, mesh_depth_raster_kernel, dim3((unsigned)((F + MD_THREADS - 1) / MD_THREADS)), dim3(MD_THREADS), 0, P)) return e;
    }
    if (int e = launch("mesh_depth_resolve", 0, s, mesh_depth_resolve_kernel, dim3(most, (unsigned)a->count), dim3(MD_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

}  // extern "C"
