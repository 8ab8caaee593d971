// The per-voxel fusion rule of include/lvdgs.h ("TSDF fusion", steps 1-5) and the corner test that lets a kernel skip a brick of
// voxels for a view, stated once for the dense volume (tsdf.hip) and the block-sparse one (tsdf_blocks.hip).  Both are built with
// -ffp-contract=off and without fast-math: the float32 expressions below are evaluated as written in either kernel.
#pragma once
#include "common.hpp"

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
struct TsdfPixel { float z; int pix; bool ok; };
__device__ __forceinline__ TsdfPixel tsdf_pixel(const TsdfView &V, const float (&R)[9], const float (&T)[3], float px, float py, float pz) {
    const float x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0];
    const float y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1];
    const float z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2];
    const float u = V.fx * (x / z) + V.cx, vv = V.fy * (y / z) + V.cy;
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

}  // namespace lvdgs
