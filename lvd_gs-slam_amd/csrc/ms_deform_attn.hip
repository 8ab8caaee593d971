// Multi-scale deformable attention: the operator of Deformable-DETR that GroundingDINO's encoder and decoder layers call as
// groundingdino._C.ms_deform_attn_forward / _backward (reference GroundingDINO-main/groundingdino/models/GroundingDINO/
// ms_deform_attn.py:53, :80; the extension's sources are CUDA and absent from the reference checkout).  The semantics are the
// published ones, which the reference states with grid_sample(bilinear, zeros, align_corners=False) (ms_deform_attn.py:93-133):
//
//   level l of size (h, w):  x = loc_x * w - 0.5,  y = loc_y * h - 0.5
//   a sample takes part only if  y > -1 && x > -1 && y < h && x < w;  each of its four corners only if it lies inside the level
//   out[b, q, h, :] = sum_{l, p} weight * sum_corners bilinear * value[b, start_l + yy * w + xx, h, :]
//
// float32 tensors and arithmetic; a gather, no MFMA.  spatial_shapes and level_start are DEVICE tensors and are read on the
// device: nothing here waits for the host.
//
// Memory safety (the three guards, all in msda_level / msda_locate below):
//   * the float -> int conversion of x, y happens only after the validity comparison has passed -- NaN, +-inf and huge
//     locations fail it and contribute nothing;
//   * a level whose size or start is negative, above 2^31 - 1 or (the start) above S counts as empty, so that the flattened
//     index below cannot overflow its 64 bits;
//   * a corner is read (forward, backward) or added to (backward) only if it lies inside its level AND its flattened index
//     start_l + yy * w + xx is below S -- shapes that do not add up to S give wrong numbers, never an access outside value.
#include "common.hpp"

namespace lvdgs {
namespace {

struct MsdaLevel { int h, w; int64_t start; float fh, fw; };

__device__ __forceinline__ MsdaLevel msda_level(const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts, int l, int S) {
    const int64_t h = shapes[2 * l], w = shapes[2 * l + 1], st = starts[l];
    const bool sane = h >= 0 && w >= 0 && h <= 0x7fffffffLL && w <= 0x7fffffffLL && st >= 0 && st <= (int64_t)S;
    MsdaLevel lv;
    lv.h = sane ? (int)h : 0; lv.w = sane ? (int)w : 0; lv.start = sane ? st : 0;
    lv.fh = (float)lv.h; lv.fw = (float)lv.w;
    return lv;
}

// One sampling location in one level: the bilinear fractions and, per corner (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1),
// its row of the value table -- or -1 when the corner takes no part (outside the level, or not below S).
struct MsdaSample { bool valid; float lx, ly; int row[4]; };

__device__ __forceinline__ MsdaSample msda_locate(const MsdaLevel &lv, int S, float loc_x, float loc_y) {
    MsdaSample s;
    const float x = loc_x * lv.fw - 0.5f, y = loc_y * lv.fh - 0.5f;
    s.valid = y > -1.f && x > -1.f && y < lv.fh && x < lv.fw;   // false for NaN; +-inf and huge values fail it too
    const float xf = floorf(s.valid ? x : 0.f), yf = floorf(s.valid ? y : 0.f);
    const int x0 = (int)xf, y0 = (int)yf;                       // -1 <= x0 < w, -1 <= y0 < h: converted only behind the comparison
    s.lx = s.valid ? x - xf : 0.f; s.ly = s.valid ? y - yf : 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
        const int64_t idx = lv.start + (int64_t)yy * lv.w + xx;   // at most 2^31 + 2^62 + 2^31
        const bool in = s.valid && yy >= 0 && xx >= 0 && yy < lv.h && xx < lv.w && idx < (int64_t)S;   // the device-side guard
        s.row[k] = in ? (int)idx : -1;
    }
    return s;
}

// Lanes: a group of 2^gp_log2 <= 64 adjacent lanes owns one (b, q, h); lane g of it owns the channel chunks g, g + 2^gp_log2, ...
// of V floats.  A power of two, so that no group straddles a wave and the backward's sums stay inside one.  At GroundingDINO's
// shape (H = 8, D = 32, V = 4) a group is 8 lanes reading one 128-byte corner row, and a wave is one query.
inline int msda_group_log2(int lanes_needed) {
    int k = 0;
    while ((1 << k) < lanes_needed && k < 6) k++;
    return k;
}

// Forward.  V floats per lane and load (4: 16 bytes); PB samples in flight per lane: their 4 PB corner loads are issued before
// the first is used.  PB = 4 needs P % 4 == 0 (the four samples share a level) and loads their locations and weights as
// three 16-byte words -- the same addresses across the group, so one request per group.
template <int V, int PB>
__global__ void __launch_bounds__(256) msda_fwd_kernel(const float *__restrict__ value, const int64_t *__restrict__ shapes,
                                                       const int64_t *__restrict__ starts, const float *__restrict__ loc,
                                                       const float *__restrict__ attw, int S, int H, int D, int Q, int L, int P,
                                                       int64_t groups, int gp_log2, float *__restrict__ out) {
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, grp = t >> gp_log2;   // grp = (b * Q + q) * H + h
    if (grp >= groups) return;
    const int g = (int)(t & ((1 << gp_log2) - 1)), G = D / V;
    const int h = (int)(grp % H), b = (int)(grp / H / Q);
    const float *lo = loc + grp * L * P * 2, *aw = attw + grp * L * P;
    const size_t row_stride = (size_t)H * D;
    const float *vb = value + ((size_t)b * S * H + h) * D;   // row r of this batch and head: vb + r * row_stride
    for (int c = g; c < G; c += 1 << gp_log2) {
        vec_t acc = (vec_t)(0.f);
        for (int l = 0; l < L; l++) {
            const MsdaLevel lv = msda_level(shapes, starts, l, S);
            for (int p0 = 0; p0 < P; p0 += PB) {
                float lx[PB], ly[PB], w[PB];
                if constexpr (PB == 4) {
                    const float4 a = *reinterpret_cast<const float4 *>(lo + (l * P + p0) * 2);
                    const float4 bb = *reinterpret_cast<const float4 *>(lo + (l * P + p0) * 2 + 4);
                    const float4 ww = *reinterpret_cast<const float4 *>(aw + l * P + p0);
                    lx[0] = a.x; ly[0] = a.y; lx[1] = a.z; ly[1] = a.w; lx[2] = bb.x; ly[2] = bb.y; lx[3] = bb.z; ly[3] = bb.w;
                    w[0] = ww.x; w[1] = ww.y; w[2] = ww.z; w[3] = ww.w;
                } else {
                    static_assert(PB == 1, "one sample or four");
                    lx[0] = lo[(l * P + p0) * 2]; ly[0] = lo[(l * P + p0) * 2 + 1]; w[0] = aw[l * P + p0];
                }
                MsdaSample s[PB];
                vec_t v[PB][4];
#pragma unroll
                for (int j = 0; j < PB; j++) {
                    s[j] = msda_locate(lv, S, lx[j], ly[j]);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        v[j][k] = s[j].row[k] >= 0 ? *reinterpret_cast<const vec_t *>(vb + (size_t)s[j].row[k] * row_stride + (size_t)c * V)
                                                   : (vec_t)(0.f);
                }
#pragma unroll
                for (int j = 0; j < PB; j++) {
                    const float hx = 1.f - s[j].lx, hy = 1.f - s[j].ly;
                    acc += w[j] * ((hy * hx) * v[j][0] + (hy * s[j].lx) * v[j][1] + (s[j].ly * hx) * v[j][2] + (s[j].ly * s[j].lx) * v[j][3]);
                }
            }
        }
        *reinterpret_cast<vec_t *>(out + grp * D + (int64_t)c * V) = acc;
    }
}

// Backward.  One channel per lane: a wave-instruction of the grad_value scatter (atomicAdd) then adds the contiguous row
// segment of its group -- at D = 32 two 128-byte segments per instruction, the shape the float atomics run at full rate in.
// The location and weight gradients of a sample belong to one group: summed over its lanes by a butterfly in a fixed order
// and stored once by lane 0, no atomics.  grad_value is zeroed by the caller (lvdgs_ms_deform_attn_backward).
__global__ void __launch_bounds__(256) msda_bwd_kernel(const float *__restrict__ value, const int64_t *__restrict__ shapes,
                                                       const int64_t *__restrict__ starts, const float *__restrict__ loc,
                                                       const float *__restrict__ attw, const float *__restrict__ grad_out, int S, int H,
                                                       int D, int Q, int L, int P, int64_t groups, int gp_log2,
                                                       float *__restrict__ grad_value, float *__restrict__ grad_loc,
                                                       float *__restrict__ grad_attw) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, grp = t >> gp_log2;   // grp = (b * Q + q) * H + h
    if (grp >= groups) return;   // a whole group leaves or stays: the butterflies below read lanes of the own group only
    const int GP = 1 << gp_log2, g = (int)(t & (GP - 1));
    const int h = (int)(grp % H), b = (int)(grp / H / Q);
    const float *lo = loc + grp * L * P * 2, *aw = attw + grp * L * P, *go = grad_out + grp * D;
    float *glo = grad_loc + grp * L * P * 2, *gaw = grad_attw + grp * L * P;
    const size_t row_stride = (size_t)H * D, base = ((size_t)b * S * H + h) * D;
    const float go0 = g < D ? go[g] : 0.f;
    for (int l = 0; l < L; l++) {
        const MsdaLevel lv = msda_level(shapes, starts, l, S);
        for (int p = 0; p < P; p++) {
            const int sp = l * P + p;
            const float weight = aw[sp];
            const MsdaSample s = msda_locate(lv, S, lo[2 * sp], lo[2 * sp + 1]);   // the same for every lane of the group
            float sum_w = 0.f, sum_x = 0.f, sum_y = 0.f;
            if (s.valid) {
                const float hx = 1.f - s.lx, hy = 1.f - s.ly;
                const float cw[4] = {hy * hx, hy * s.lx, s.ly * hx, s.ly * s.lx};
                for (int c = g; c < D; c += GP) {
                    const float d = c == g ? go0 : go[c];
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) v[k] = s.row[k] >= 0 ? value[base + (size_t)s.row[k] * row_stride + c] : 0.f;
                    sum_w += (cw[0] * v[0] + cw[1] * v[1] + cw[2] * v[2] + cw[3] * v[3]) * d;
                    sum_x += (hy * (v[1] - v[0]) + s.ly * (v[3] - v[2])) * d;
                    sum_y += (hx * (v[2] - v[0]) + s.lx * (v[3] - v[1])) * d;
                    const float wd = weight * d;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (s.row[k] >= 0) atomicAdd(grad_value + base + (size_t)s.row[k] * row_stride + c, cw[k] * wd);
                }
                for (int m = GP >> 1; m > 0; m >>= 1) {
                    sum_w += __shfl_xor(sum_w, m); sum_x += __shfl_xor(sum_x, m); sum_y += __shfl_xor(sum_y, m);
                }
            }
            if (g == 0) {
                gaw[sp] = sum_w;                        // an invalid sample: three zeros
                glo[2 * sp] = lv.fw * weight * sum_x; glo[2 * sp + 1] = lv.fh * weight * sum_y;
            }
        }
    }
}

int msda_check(const char *what, const void *value, const void *shapes, const void *starts, const void *loc, const void *attw, int B, int S,
               int H, int D, int Q, int L, int P, bool *empty) {
    *empty = true;
    if (B < 0 || S < 0 || H < 0 || D < 0 || Q < 0 || L < 0 || P < 0) { set_error("%s: negative size", what); return LVDGS_E_INVALID; }
    if (H < 1 || D < 1) { set_error("%s: H and D must be at least 1", what); return LVDGS_E_INVALID; }
    if ((int64_t)B * Q == 0) return LVDGS_OK;
    if (L == 0 || P == 0) { set_error("%s: L and P must be at least 1 when there are queries", what); return LVDGS_E_INVALID; }
    const int64_t lim = 0x7fffffffLL, hd = (int64_t)H * D, lp2 = (int64_t)L * P * 2, bq = (int64_t)B * Q;
    if (hd > lim || lp2 > lim || bq > lim / hd || bq * H > lim / lp2 || (int64_t)B * S > lim / hd) {
        set_error("%s: a tensor of more than 2^31 - 1 elements (int32 indexing)", what);
        return LVDGS_E_INVALID;
    }
    if (S > 0 && (!value || !shapes || !starts || !loc || !attw)) { set_error("%s: NULL tensor", what); return LVDGS_E_INVALID; }
    *empty = false;
    return LVDGS_OK;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

int lvdgs_ms_deform_attn_forward(const float *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *sampling_loc,
                                 const float *attn_weight, int32_t B, int32_t S, int32_t H, int32_t D, int32_t Q, int32_t L, int32_t P,
                                 float *out, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    bool empty;
    if (int e = msda_check("ms_deform_attn_forward", value, spatial_shapes, level_start, sampling_loc, attn_weight, B, S, H, D, Q, L, P, &empty)) return e;
    if (empty) return LVDGS_OK;
    if (!out) { set_error("ms_deform_attn_forward: NULL tensor"); return LVDGS_E_INVALID; }
    const int64_t groups = (int64_t)B * Q * H;
    if (S == 0) return check_hip(hipMemsetAsync(out, 0, (size_t)groups * D * sizeof(float), s), "ms_deform_attn_forward (memset)");
    const bool wide = D % 4 == 0 && aligned16(value) && aligned16(out);
    const bool four = wide && P % 4 == 0 && aligned16(sampling_loc) && aligned16(attn_weight);
    const int gp_log2 = msda_group_log2(wide ? D / 4 : D);
    const dim3 grid((unsigned)(((groups << gp_log2) + 255) / 256)), block(256);
    const auto kernel = wide ? (four ? msda_fwd_kernel<4, 4> : msda_fwd_kernel<4, 1>) : msda_fwd_kernel<1, 1>;   // (four implies wide)
    if (int e = launch("msda_fwd", 0, s, kernel, grid, block, 0, value, spatial_shapes, level_start, sampling_loc, attn_weight, S, H, D, Q, L, P, groups, gp_log2, out)) return e;
    return LVDGS_OK;
}

int lvdgs_ms_deform_attn_backward(const float *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *sampling_loc,
                                  const float *attn_weight, int32_t B, int32_t S, int32_t H, int32_t D, int32_t Q, int32_t L, int32_t P,
                                  const float *grad_out, float *grad_value, float *grad_sampling_loc, float *grad_attn_weight, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    bool empty;
    if (int e = msda_check("ms_deform_attn_backward", value, spatial_shapes, level_start, sampling_loc, attn_weight, B, S, H, D, Q, L, P, &empty)) return e;
    const size_t value_bytes = B > 0 && S > 0 ? (size_t)B * S * H * D * sizeof(float) : 0;
    if (empty) {   // no queries: grad_value is still all of the answer there is
        if ((int64_t)B * S > 0x7fffffffLL / ((int64_t)H * D)) { set_error("ms_deform_attn_backward: a tensor of more than 2^31 - 1 elements (int32 indexing)"); return LVDGS_E_INVALID; }
        if (value_bytes && grad_value) return check_hip(hipMemsetAsync(grad_value, 0, value_bytes, s), "ms_deform_attn_backward (memset)");
        return LVDGS_OK;
    }
    if (!grad_sampling_loc || !grad_attn_weight || (S > 0 && (!grad_out || !grad_value))) { set_error("ms_deform_attn_backward: NULL tensor"); return LVDGS_E_INVALID; }
    const int64_t groups = (int64_t)B * Q * H;
    if (S == 0) {
        if (int e = check_hip(hipMemsetAsync(grad_sampling_loc, 0, (size_t)groups * L * P * 2 * sizeof(float), s), "ms_deform_attn_backward (memset)")) return e;
        return check_hip(hipMemsetAsync(grad_attn_weight, 0, (size_t)groups * L * P * sizeof(float), s), "ms_deform_attn_backward (memset)");
    }
    if (int e = check_hip(hipMemsetAsync(grad_value, 0, value_bytes, s), "ms_deform_attn_backward (memset)")) return e;
    const int gp_log2 = msda_group_log2(D);
    const dim3 grid((unsigned)(((groups << gp_log2) + 255) / 256)), block(256);
    if (int e = launch("msda_bwd", 0, s, msda_bwd_kernel, grid, block, 0, value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_out, S, H, D, Q, L, P,
            groups, gp_log2, grad_value, grad_sampling_loc, grad_attn_weight)) return e;
    return LVDGS_OK;
}

}  // extern "C"
