// The TSDF rules of include/lvdgs.h, stated once for the dense volume (tsdf.hip) and the block-sparse one (tsdf_blocks.hip):
//  * fusion ("TSDF fusion", steps 1-5): the corner test that lets a kernel skip a brick of voxels for a view (brick_may_touch), the
//    per-voxel arithmetic (tsdf_pixel, tsdf_seen, tsdf_blend) and the walk of one thread's samples through a call's views
//    (tsdf_fuse_views);
//  * surface nets: the bits of the classify and edge bytes, when a cell is active (tsdf_cell_active), which of a sample's edges give
//    faces (tsdf_edge_axes over the cyclic steps of tsdf_axis_step), a cell's vertex (tsdf_cell_vertex), a quad's two triangles
//    (tsdf_write_quad) and the counts of the host block (tsdf_publish_counts);
//  * the host side: what both integrate calls refuse about the planes, the constants and the views, and the packing of a view list.
// A kernel brings its storage -- how samples are found, loaded and stored -- and calls these.  Both files are built with
// -ffp-contract=off and without fast-math: the float32 expressions below are evaluated as written in either kernel.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "host_checks.hpp"

namespace lvdgs {

struct TsdfView {
    int W, H;
    float fx, fy, cx, cy, dmin, dtrunc;
    const float *R, *T, *depth, *image;
    const uint8_t *mask;
};

// the lattice p[a] = o[a] + vs * (float)index[a] and the two constants of the update
struct TsdfLattice { float ox, oy, oz, vs, trunc, maxw; };

// Can view V change a voxel of the brick whose corner voxels are (i0|i1, j0|j1, k0|k1)?  false only when the per-voxel rule skips
// every voxel of it.  The lattice positions are monotone in the index and x, y, z of step 1 are affine in them, so each quantity below
// is bounded over the brick by its values at the corners, up to the rounding of step 1: at most 4 * 2^-24 of M = |R0 px| + |R1 py| +
// |R2 pz| + |T| for a voxel and as much for a corner -- ez = 1e-6 M covers both twice over.
//  * behind:  every z <= depth_min.
//  * far:     d <= depth_trunc, so sdf <= depth_trunc - z (rounding is monotone); below -trunc for every z.
//  * frustum, for a brick with z >= M / 64 > 0 only: u + 0.5 < 0 is fx x + (cx + 0.5) z < 0, affine again, and u + 0.5 >= W likewise.
//    The computed u is off by at most fx (ex + |x / z| ez) / z + a few ulps of |u| + |cx|; times z, with 1 / z <= 64 / Mz, that is under
//    2e-5 (fx Mx + (|cx| + W + 1) Mz): the margin taken is 1e-4 of it.
__device__ __forceinline__ bool brick_may_touch(const TsdfLattice &p, const TsdfView &V, int i0, int i1, int j0, int j1, int k0, int k1) {
    float R[9], T[3];
#pragma unroll
    for (int q = 0; q < 9; q++) R[q] = V.R[q];
#pragma unroll
    for (int q = 0; q < 3; q++) T[q] = V.T[q];
    const float inf = __builtin_inff();
    const float cl = V.cx + 0.5f, cr = cl - (float)V.W, ct = V.cy + 0.5f, cb = ct - (float)V.H;
    float zmin = inf, zmax = -inf, Mx = 0.f, My = 0.f, Mz = 0.f;
    float gl = -inf, gr = inf, gt = -inf, gb = inf;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float px = p.ox + p.vs * (float)((c & 1) ? i1 : i0);
        const float py = p.oy + p.vs * (float)((c & 2) ? j1 : j0);
        const float pz = p.oz + p.vs * (float)((c & 4) ? k1 : k0);
        const float x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0];
        const float y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1];
        const float z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2];
        Mx = fmaxf(Mx, fabsf(R[0] * px) + fabsf(R[1] * py) + fabsf(R[2] * pz) + fabsf(T[0]));
        My = fmaxf(My, fabsf(R[3] * px) + fabsf(R[4] * py) + fabsf(R[5] * pz) + fabsf(T[1]));
        Mz = fmaxf(Mz, fabsf(R[6] * px) + fabsf(R[7] * py) + fabsf(R[8] * pz) + fabsf(T[2]));
        zmin = fminf(zmin, z); zmax = fmaxf(zmax, z);
        gl = fmaxf(gl, V.fx * x + cl * z); gr = fminf(gr, V.fx * x + cr * z);
        gt = fmaxf(gt, V.fy * y + ct * z); gb = fminf(gb, V.fy * y + cb * z);
    }
    if (!(Mx + My + Mz < inf)) return true;   // a NaN or an overflow somewhere: let the voxels decide
    const float ez = 1e-6f * Mz;
    if (zmax + ez <= V.dmin) return false;
    const float zlo = zmin - 2.f * ez;
    if (V.dtrunc - zlo < -p.trunc) return false;
    if (zlo > 0.f && zlo >= 0.015625f * Mz && V.fx > 0.f && V.fy > 0.f) {
        const float mx = 1e-4f * (V.fx * Mx + (fabsf(V.cx) + (float)V.W + 1.f) * Mz);
        const float my = 1e-4f * (V.fy * My + (fabsf(V.cy) + (float)V.H + 1.f) * Mz);
        if (gl + mx < 0.f || gr - mx > 0.f || gt + my < 0.f || gb - my > 0.f) return false;
    }
    return true;
}

// Steps 1 and 2 for the voxel at (px, py, pz): its camera depth z, whether it lies in front of depth_min and inside the image, and
// its pixel (pixel 0 stands in where there is none: a gather from it has a valid address and needs no branch).
// Step 1 and the two expressions of step 2 that stay continuous: the camera depth z and the image position (u, v) of (px, py, pz).
struct TsdfProjected { float z, u, v; };
__device__ __forceinline__ TsdfProjected tsdf_project(float fx, float fy, float cx, float cy, const float (&R)[9], const float (&T)[3],
                                                      float px, float py, float pz) {
    const float x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0];
    const float y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1];
    const float z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2];
    return TsdfProjected{z, fx * (x / z) + cx, fy * (y / z) + cy};
}

struct TsdfPixel { float z; int pix; bool ok; };
__device__ __forceinline__ TsdfPixel tsdf_pixel(const TsdfView &V, const float (&R)[9], const float (&T)[3], float px, float py, float pz) {
    const TsdfProjected at = tsdf_project(V.fx, V.fy, V.cx, V.cy, R, T, px, py, pz);
    const float z = at.z, u = at.u, vv = at.v;
    const float uf = floorf(u + 0.5f), vf = floorf(vv + 0.5f);
    TsdfPixel P;
    P.z = z;
    P.ok = z > V.dmin && uf >= 0.f && uf < (float)V.W && vf >= 0.f && vf < (float)V.H;
    P.pix = P.ok ? (int)vf * V.W + (int)uf : 0;
    return P;
}

// The tests of steps 3 and 4 on the pixel's depth d and mask byte m (1 where the view has no mask); *sdf = d - z.
__device__ __forceinline__ bool tsdf_seen(const TsdfView &V, float trunc, float d, uint8_t m, float z, float *sdf) {
    *sdf = d - z;
    return d > 0.f && d <= V.dtrunc && m != 0 && !(*sdf < -trunc);
}

// Steps 4 and 5: the running means and the weight of one voxel; (c0, c1, c2): the pixel's colour, read when `coloured`.
__device__ __forceinline__ void tsdf_blend(const TsdfLattice &p, float sdf, bool coloured, float c0, float c1, float c2,
                                           float &f, float &w, float &cr, float &cg, float &cb) {
    const float t = fminf(1.0f, sdf / p.trunc);
    const float w0 = w, w1 = w0 + 1.0f;
    f = (f * w0 + t) / w1;
    if (coloured) {
        cr = (cr * w0 + c0) / w1;
        cg = (cg * w0 + c1) / w1;
        cb = (cb * w0 + c2) / w1;
    }
    w = fminf(w1, p.maxw);
}

// One thread's N samples at (px, py, pz)[q] through the views of a call whose bit of `live` is set (wave-uniform: the ballot of
// brick_may_touch).  valid[q]: the sample exists; f, w and, with COLOR, cr, cg, cb: its planes in registers across the views.
// changed: some sample's tsdf and weight were updated, recoloured: some sample's colours.  Each view is walked in stages over the N
// samples, so that their gathers are in flight together: the pixels (pixel 0 stands in where there is none: every gather has a valid
// address and needs no branch), all depths, all masks, the colours, the updates.
template <int N, bool COLOR>
__device__ __forceinline__ void tsdf_fuse_views(const TsdfLattice &lat, const TsdfView *views, int count, uint32_t live,
                                                const float (&px)[N], const float (&py)[N], const float (&pz)[N], const bool (&valid)[N],
                                                float (&f)[N], float (&w)[N], float (&cr)[N], float (&cg)[N], float (&cb)[N],
                                                bool &changed, bool &recoloured) {
    for (int v = 0; v < count; v++) {
        if (!((live >> v) & 1u)) continue;   // (wave-uniform)
        const TsdfView &V = views[v];
        float R[9], T[3];
#pragma unroll
        for (int q = 0; q < 9; q++) R[q] = V.R[q];
#pragma unroll
        for (int q = 0; q < 3; q++) T[q] = V.T[q];
        const int64_t P = (int64_t)V.W * V.H;
        const bool coloured = COLOR && V.image != nullptr;
        float z[N];
        int pix[N];
        bool ok[N], any = false;
#pragma unroll
        for (int q = 0; q < N; q++) {
            const TsdfPixel at = tsdf_pixel(V, R, T, px[q], py[q], pz[q]);
            z[q] = at.z;
            ok[q] = valid[q] && at.ok;
            pix[q] = ok[q] ? at.pix : 0;
            any = any || ok[q];
        }
        if (!__any(any)) continue;   // (a wave's samples outside this view)
        float d[N], sdf[N];
        uint8_t m[N];
#pragma unroll
        for (int q = 0; q < N; q++) d[q] = V.depth[pix[q]];
#pragma unroll
        for (int q = 0; q < N; q++) m[q] = V.mask ? V.mask[pix[q]] : (uint8_t)1;
#pragma unroll
        for (int q = 0; q < N; q++) {
            const bool seen = tsdf_seen(V, lat.trunc, d[q], m[q], z[q], &sdf[q]);
            ok[q] = ok[q] && seen;
        }
        float c0[N], c1[N], c2[N];
        if (coloured) {
#pragma unroll
            for (int q = 0; q < N; q++) {
                const int from = ok[q] ? pix[q] : 0;
                c0[q] = V.image[from]; c1[q] = V.image[P + from]; c2[q] = V.image[2 * P + from];
            }
        }
#pragma unroll
        for (int q = 0; q < N; q++) {
            if (!ok[q]) continue;
            tsdf_blend(lat, sdf[q], coloured, c0[q], c1[q], c2[q], f[q], w[q], cr[q], cg[q], cb[q]);
            recoloured = recoloured || coloured;
            changed = true;
        }
    }
}

// ---------------------------------------------------------------- surface nets ----

enum : uint8_t {
    CELL_ACTIVE = 1, SAMPLE_INSIDE = 2, SAMPLE_OBSERVED = 4,   // the classify pass's byte of a sample and of the cell at it
    EDGE_LOW_INSIDE = 8                                        // the edge pass's byte: bits 0-2 the axes whose edge gives faces
};

// A cell is active when all eight corner samples are observed and some, not all, are inside.  corner(q): the classify bits of corner
// q = dx | dy << 1 | dz << 2.
template <typename Corner>
__device__ __forceinline__ bool tsdf_cell_active(Corner corner) {
    bool all = true;
    int n_in = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint8_t fl = corner(q);
        all = all && (fl & SAMPLE_OBSERVED);
        n_in += (fl & SAMPLE_INSIDE) ? 1 : 0;
    }
    return all && n_in > 0 && n_in < 8;
}

// The unit step along `axis` (taken mod 3).  With a = axis, b = axis + 1 and c = axis + 2 the three are cyclic: (x, y, z), (y, z, x),
// (z, x, y).
struct TsdfStep { int x, y, z; };
__device__ __forceinline__ constexpr TsdfStep tsdf_axis_step(int axis) { return TsdfStep{axis % 3 == 0, axis % 3 == 1, axis % 3 == 2}; }

// The axes (bit a) whose edge from a sample, the low corner of an active cell, to its +a neighbour gives faces: the two ends differ in
// sign and the other three cells around the edge, at -b - c, -c and -b, are active too.  differs(dx, dy, dz): is the sample at that
// offset on the other side of the surface; act(dx, dy, dz): is the cell at that offset active (false where there is none).
template <typename Differs, typename Act>
__device__ __forceinline__ uint32_t tsdf_edge_axes(Differs differs, Act act) {
    bool crossed[3];   // (the three ends first: their reads are in flight together, and few samples go on to the cells)
#pragma unroll
    for (int axis = 0; axis < 3; axis++) crossed[axis] = differs(tsdf_axis_step(axis).x, tsdf_axis_step(axis).y, tsdf_axis_step(axis).z);
    uint32_t e = 0;
#pragma unroll
    for (int axis = 0; axis < 3; axis++) {
        const TsdfStep b = tsdf_axis_step(axis + 1), c = tsdf_axis_step(axis + 2);
        if (crossed[axis] && act(-b.x - c.x, -b.y - c.y, -b.z - c.z) && act(-c.x, -c.y, -c.z) && act(-b.x, -b.y, -b.z)) e |= 1u << axis;
    }
    return e;
}

// The quad of the edge's four cells, v0 at -b - c, v1 at -c, v2 the sample's own, v3 at -b, as two triangles in rows `row` and
// `row + 1` of `faces`; a row at or beyond `cap` is not written.  low_in: the edge's low end is inside, which turns the winding.
__device__ __forceinline__ void tsdf_write_quad(int32_t *faces, unsigned long long row, unsigned long long cap, bool low_in,
                                                int32_t v0, int32_t v1, int32_t v2, int32_t v3) {
    const int32_t tri[2][3] = {{v0, low_in ? v1 : v2, low_in ? v2 : v1}, {v0, low_in ? v2 : v3, low_in ? v3 : v2}};
#pragma unroll
    for (int t = 0; t < 2; t++, row++) {
        if (row >= cap) continue;
        int32_t *dst = faces + (size_t)row * 3;
        dst[0] = tri[t][0]; dst[1] = tri[t][1]; dst[2] = tri[t][2];
    }
}

// The counts of a mesh call's host block from the scans' totals ([0] vertices, [1] faces); both volumes' blocks hold them in the
// same words.
static_assert(LVDGS_TSDF_BLOCKS_N_VERTICES == LVDGS_TSDF_N_VERTICES && LVDGS_TSDF_BLOCKS_N_FACES == LVDGS_TSDF_N_FACES &&
              LVDGS_TSDF_BLOCKS_OVERFLOW == LVDGS_TSDF_OVERFLOW, "the two host blocks report the counts in the same words");
__device__ __forceinline__ void tsdf_publish_counts(volatile int32_t *w, const unsigned long long *totals, int vcap, int fcap) {
    const unsigned long long nv = totals[0], nf = totals[1];
    const bool too_many = nf > (unsigned long long)INT32_MAX;
    w[LVDGS_TSDF_N_VERTICES] = (int32_t)nv;
    w[LVDGS_TSDF_N_FACES] = too_many ? INT32_MAX : (int32_t)nf;
    w[LVDGS_TSDF_OVERFLOW] = (nv > (unsigned long long)vcap ? 1 : 0) | (nf > (unsigned long long)fcap ? 2 : 0) | (too_many ? 4 : 0);
}

// The surface-nets vertex of an active cell from its eight corner samples (corner q = dx | dy << 1 | dz << 2): the mean crossing of
// its 12 edges in the header's order, as an offset from the low corner, and the mean colour.  colour(q, ch): corner q's plane ch,
// called for the ends of crossing edges only.
template <bool COLOR, typename ColourAt>
__device__ __forceinline__ void tsdf_cell_vertex(const float (&f)[8], ColourAt colour, float (&mean)[3], float (&col)[3]) {
    float sum[3] = {0.f, 0.f, 0.f};
    col[0] = col[1] = col[2] = 0.f;
    int crossings = 0;
    // the 12 edges: axis, then the two other offsets in (x before y before z) order, low bit first
#pragma unroll
    for (int e = 0; e < 12; e++) {
        const int axis = e >> 2, lo_bit = e & 1, hi_bit = (e >> 1) & 1;
        // corner number (dx | dy << 1 | dz << 2) of the edge's low end
        const int c0 = axis == 0 ? (lo_bit << 1 | hi_bit << 2) : axis == 1 ? (lo_bit | hi_bit << 2) : (lo_bit | hi_bit << 1);
        const int c1 = c0 | (1 << axis);
        const float f0 = f[c0], f1 = f[c1];
        if ((f0 < 0.f) == (f1 < 0.f)) continue;
        const float q = f0 / (f0 - f1);
#pragma unroll
        for (int a = 0; a < 3; a++) sum[a] += a == axis ? q : (float)((c0 >> a) & 1);
        if constexpr (COLOR) {
            const float r0 = colour(c0, 0), r1 = colour(c1, 0), g0 = colour(c0, 1), g1 = colour(c1, 1), b0 = colour(c0, 2), b1 = colour(c1, 2);
            col[0] += r0 + q * (r1 - r0);
            col[1] += g0 + q * (g1 - g0);
            col[2] += b0 + q * (b1 - b0);
        }
        crossings++;
    }
    const float cnt = (float)crossings;
#pragma unroll
    for (int a = 0; a < 3; a++) mean[a] = sum[a] / cnt;
    if constexpr (COLOR) {
#pragma unroll
        for (int a = 0; a < 3; a++) col[a] = col[a] / cnt;
    }
}

// ---------------------------------------------------------------- the host side ----
// What the entry points of both volumes refuse, in `name`'s words.  Vol: lvdgs_tsdf_volume or lvdgs_tsdf_blocks.

inline bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

template <typename Vol>
int tsdf_check_planes(const char *name, const Vol &v) {
    if (!v.tsdf || !v.weight) { set_error("%s: tsdf / weight plane is NULL", name); return LVDGS_E_INVALID; }
    const int colours = (v.r ? 1 : 0) + (v.g ? 1 : 0) + (v.b ? 1 : 0);
    if (colours != 0 && colours != 3) { set_error("%s: colour planes r, g, b must be all set or all NULL", name); return LVDGS_E_INVALID; }
    return LVDGS_OK;
}

template <typename Vol>
int tsdf_check_constants(const char *name, const Vol &v) {
    if (!positive_finite(v.voxel_size) || !positive_finite(v.trunc) || !positive_finite(v.max_weight)) {
        set_error("%s: voxel_size %g, trunc %g and max_weight %g must be finite and positive", name, v.voxel_size, v.trunc, v.max_weight);
        return LVDGS_E_RANGE;
    }
    return LVDGS_OK;
}

inline int tsdf_check_count(const char *name, int32_t count) {
    if (count < 0 || count > LVDGS_TSDF_MAX_VIEWS) { set_error("%s: count %d is outside 0 .. %d", name, count, LVDGS_TSDF_MAX_VIEWS); return LVDGS_E_INVALID; }
    return LVDGS_OK;
}

// The `count` <= LVDGS_TSDF_MAX_VIEWS views of an integrate call into out[]; *most_pixels, where asked for: the largest view's.
// coloured: the volume has colour planes.
inline int tsdf_pack_views(const char *name, const lvdgs_tsdf_view *const *views, int32_t count, bool coloured, TsdfView *out,
                           int64_t *most_pixels = nullptr) {
    if (count > 0 && !views) { set_error("%s: view list is NULL", name); return LVDGS_E_INVALID; }
    int64_t most = 0;
    for (int v = 0; v < count; v++) {
        const lvdgs_tsdf_view *a = views[v];
        if (int e = check_view(name, v, a, true)) return e;
        if (a->image && !coloured) { set_error("%s: view %d has an image, the volume no colour planes", name, v); return LVDGS_E_INVALID; }
        out[v] = TsdfView{a->width, a->height, a->fx, a->fy, a->cx, a->cy, a->depth_min, a->depth_trunc, a->R, a->T, a->depth, a->image, a->mask};
        most = std::max(most, (int64_t)a->width * a->height);
    }
    if (most_pixels) *most_pixels = most;
    return LVDGS_OK;
}

}  // namespace lvdgs
