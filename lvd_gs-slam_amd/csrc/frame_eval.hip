// Evaluation of one rendered frame (reference utils/eval_utils_0806.py:216-312, the per-frame block of eval_rendering): squared-error
// sums and counts over the non-black elements and over the static ones, SSIM of the full frame and of the frame with the non-static
// elements of both images overwritten by the background colour, the depth map's extrema, and the 8-bit images the reference writes
// to disk.  The arithmetic is stated in include/lvdgs.h ("Frame evaluation").
//
// SSIM is ssim.hip's, value only: the same taps and passes, the same expression order for m; the window is normalised by torch's sum
// (fill_eval_window says why).  Without the derivative maps a 32x32 tile
// needs m on its own pixels only, so the input window is 42x42 (ssim.hip: 52x52) and the kernel holds 27 KB of LDS (ssim.hip: 40 KB):
// three workgroups of eight waves per CU, bounded by its 80 registers.  One workgroup owns a 32x32 tile of ONE plane -- the static mask is per
// channel element (gt > 0 & static), so the planes are independent:
//   1. load the 42x42 window of clamp(render), gt and the static bytes once (zero outside the image);
//   2. this tile's own pixels: squared differences, counts, colour bytes; plane 0: depth extrema;
//   3. sweep 0: horizontal then vertical 11-tap pass over (x, y), then over (x^2 + y^2, xy); m on the tile;
//   4. with a mask: the window in LDS is overwritten by the masked pair (same loads), and sweep 1 repeats step 3;
//   5. the workgroup's partial sums (float64, fixed order) to scratch.
// A finishing workgroup adds the partials in a fixed order and writes the row; a third launch quantises the depth map with the
// row's extrema.  No atomics: two calls give the same bits.
//
// Built like every file here with -ffp-contract=off and without fast-math (csrc/Makefile): the byte images are defined as float32
// products and an IEEE-rounded float32 division evaluated as written, and must match the NumPy statements bit for bit.
#include "common.hpp"
#include "device_utils.hpp"

namespace lvdgs {
namespace {

constexpr int ET = 32;            // output tile edge
constexpr int ER = 5;             // window radius
constexpr int EW = 2 * ER + 1;    // taps
constexpr int E1 = ET + 2 * ER;   // 42: input window edge
constexpr int Q1 = E1 + 1;        // 43: odd pitch, a row-strided ds_read_b32 of 32 lanes meets 32 banks
constexpr int Q2 = ET + 1;        // 33: pitch of the horizontal pass's output
constexpr int EVAL_THREADS = 512;
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;   // ssim.hip's

struct EvalPartial {              // one per workgroup, 48 bytes
    double sq_full, sq_keep, m_full, m_static;
    uint32_t n_basic, n_keep;
    float dmin, dmax;
};
static_assert(sizeof(EvalPartial) == 48, "scratch layout");
static_assert(sizeof(lvdgs_frame_eval_row) == 64, "row layout (include/lvdgs.h)");

struct EvalParams {
    int W, H;
    const float *render, *gt;
    const uint8_t *mask;
    const float *bg, *depth;
    uint8_t *pred8, *gt8, *res8;
    EvalPartial *partial;
    float win[EW];
};

// sums of the workgroup's waves in wave order: d[4][8], u[2][8], f[2][8] were filled by lane 0 of every wave
struct EvalRed { double d[4][8]; uint32_t u[2][8]; float f[2][8]; };

// waves_per_eu(6, 8): the allocator's own choice is 81 registers, one over the 80 at which a third workgroup fits a CU (six waves per
// SIMD); asked for six it finds 80 without scratch (asked for eight it spills 56 bytes per lane: not taken)
__global__ void __launch_bounds__(EVAL_THREADS) __attribute__((amdgpu_waves_per_eu(6, 8))) frame_eval_kernel(EvalParams p) {
    __shared__ float s_in[2 * E1 * Q1];
    __shared__ float s_h[2 * E1 * Q2];
    __shared__ uint8_t s_st[E1 * Q1 + 2];
    __shared__ EvalRed s_red;

    const int tid = threadIdx.x;
    const int plane = blockIdx.z;
    const int tx0 = blockIdx.x * ET, ty0 = blockIdx.y * ET;
    const size_t plane_off = (size_t)plane * p.W * p.H;
    const float *__restrict__ X = p.render + plane_off;
    const float *__restrict__ Y = p.gt + plane_off;
    const bool masked = p.mask != nullptr;
    const float bgc = p.bg ? p.bg[plane] : 0.f;
    float w[EW];
#pragma unroll
    for (int k = 0; k < EW; k++) w[k] = p.win[k];
    float *sx = s_in, *sy = s_in + E1 * Q1;

    // ---- 1. the input window: a wave takes 64 columns of one window row (42 exist), the eight waves eight rows, six rounds ----
    constexpr int NLD = (E1 + 7) / 8;
    const int lc = tid & 63, lr = tid >> 6;
    const int lgx = tx0 - ER + lc;
    const bool col_in = lc < E1 && lgx >= 0 && lgx < p.W;
    {
        float la[NLD], lb[NLD];
        uint8_t lk[NLD];
#pragma unroll
        for (int it = 0; it < NLD; it++) {
            const int r = lr + 8 * it, gy = ty0 - ER + r;
            const bool in = col_in && r < E1 && gy >= 0 && gy < p.H;
            const size_t o = in ? (size_t)gy * p.W + lgx : 0;
            la[it] = in ? X[o] : 0.f;
            lb[it] = in ? Y[o] : 0.f;
            lk[it] = (in && masked) ? p.mask[o] : (uint8_t)1;
        }
#pragma unroll
        for (int it = 0; it < NLD; it++) {
            const int r = lr + 8 * it;
            if (lc < E1 && r < E1) {
                sx[r * Q1 + lc] = fminf(fmaxf(la[it], 0.f), 1.f);   // a = clamp(render, 0, 1); outside the image: 0
                sy[r * Q1 + lc] = lb[it];
                s_st[r * Q1 + lc] = lk[it] ? (uint8_t)1 : (uint8_t)0;
            }
        }
    }
    __syncthreads();

    // ---- 2. this tile's own pixels, two per thread ----
    double sq_full = 0.0, sq_keep = 0.0;
    uint32_t n_basic = 0u, n_keep = 0u;
    float dmin = __builtin_inff(), dmax = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + k * EVAL_THREADS, r = i >> 5, c = i & 31;
        const int gy = ty0 + r, gx = tx0 + c;
        if (gy < p.H && gx < p.W) {
            const int l = (r + ER) * Q1 + c + ER;
            const float a = sx[l], b = sy[l];
            const float d = a - b;
            const float sq = d * d;
            const bool basic = b > 0.f, keep = basic && s_st[l];
            if (basic) { sq_full += (double)sq; n_basic++; }
            if (keep) { sq_keep += (double)sq; n_keep++; }
            const size_t px = (size_t)gy * p.W + gx;
            if (p.pred8 || p.gt8 || p.res8) {
                const uint8_t pa = (uint8_t)(a * 255.0f), pb = (uint8_t)(b * 255.0f);
                const size_t o = px * 3 + plane;
                if (p.pred8) p.pred8[o] = pa;
                if (p.gt8) p.gt8[o] = pb;
                if (p.res8) p.res8[o] = pa > pb ? (uint8_t)(pa - pb) : (uint8_t)(pb - pa);
            }
            if (plane == 0 && p.depth) {
                const float z = p.depth[px];
                dmin = fminf(dmin, z);
                dmax = fmaxf(dmax, z);
            }
        }
    }

    // ---- 3. / 4. the two sweeps ----
    const int hr = tid % E1, hc0 = (tid / E1) * 4;           // horizontal item: 4 outputs of one row; 42 rows x 8 groups = 336 items
    const bool h_item = tid < E1 * (ET / 4);
    const int vc = tid & 31, vr0 = (tid >> 5) * 2;            // vertical item: 2 outputs of one column; 32 columns x 16 row pairs
    const bool v_in[2] = {ty0 + vr0 < p.H && tx0 + vc < p.W, ty0 + vr0 + 1 < p.H && tx0 + vc < p.W};
    double m_full = 0.0, m_static = 0.0;
    const int sweeps = masked ? 2 : 1;
    for (int sweep = 0; sweep < sweeps; sweep++) {
        if (sweep == 1) {
            // the masked pair from the same loads: keep ? value : bg inside the image, zero padding outside as before
#pragma unroll
            for (int it = 0; it < NLD; it++) {
                const int r = lr + 8 * it, gy = ty0 - ER + r;
                if (lc < E1 && r < E1) {
                    const bool in = col_in && gy >= 0 && gy < p.H;
                    const int l = r * Q1 + lc;
                    const bool keep = sy[l] > 0.f && s_st[l];
                    if (in && !keep) { sx[l] = bgc; sy[l] = bgc; }
                }
            }
            __syncthreads();   // (also: sweep 0's last vertical reads of s_h are behind us)
        }
        float vA[2], vB[2], vS[2], vZ[2];
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            if (h_item) {
                constexpr int NIN = 4 + EW - 1;
                float p0[NIN], p1[NIN];
#pragma unroll
                for (int i = 0; i < NIN; i++) {
                    const float xv = sx[hr * Q1 + hc0 + i], yv = sy[hr * Q1 + hc0 + i];
                    p0[i] = pass == 0 ? xv : fmaf(xv, xv, yv * yv);
                    p1[i] = pass == 0 ? yv : xv * yv;
                }
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    float a = w[0] * p0[o], b = w[0] * p1[o];
#pragma unroll
                    for (int k = 1; k < EW; k++) {
                        a = fmaf(w[k], p0[o + k], a);
                        b = fmaf(w[k], p1[o + k], b);
                    }
                    const int d = hr * Q2 + hc0 + o;
                    s_h[d] = a;
                    s_h[E1 * Q2 + d] = b;
                }
            }
            __syncthreads();
            {
                float v0[2 + EW - 1], v1[2 + EW - 1];
#pragma unroll
                for (int i = 0; i < 2 + EW - 1; i++) {
                    const int d = (vr0 + i) * Q2 + vc;
                    v0[i] = s_h[d];
                    v1[i] = s_h[E1 * Q2 + d];
                }
#pragma unroll
                for (int o = 0; o < 2; o++) {
                    float a = w[0] * v0[o], b = w[0] * v1[o];
#pragma unroll
                    for (int k = 1; k < EW; k++) {
                        a = fmaf(w[k], v0[o + k], a);
                        b = fmaf(w[k], v1[o + k], b);
                    }
                    if (pass == 0) { vA[o] = a; vB[o] = b; } else { vS[o] = a; vZ[o] = b; }
                }
            }
            __syncthreads();   // s_h is written again (pass 1, or the next sweep's pass 0)
        }
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const float A = vA[o], B = vB[o], S = vS[o], Z = vZ[o];
            const float AB = A * B, AA_BB = fmaf(A, A, B * B);
            const float num1 = fmaf(2.f, AB, SSIM_C1), num2 = fmaf(2.f, Z - AB, SSIM_C2);
            const float den1 = AA_BB + SSIM_C1, den2 = (S - AA_BB) + SSIM_C2;
            const float inv1 = __builtin_amdgcn_rcpf(den1), inv2 = __builtin_amdgcn_rcpf(den2);
            const float inv12 = inv1 * inv2;
            const float m = (num1 * num2) * inv12;
            if (v_in[o]) { if (sweep == 0) m_full += (double)m; else m_static += (double)m; }
        }
    }

    // ---- 5. the workgroup's partial: wave sums (device_utils.hpp), then the waves from 0 up ----
    {
        const double t0 = wave_sum(sq_full), t1 = wave_sum(sq_keep), t2 = wave_sum(m_full), t3 = wave_sum(m_static);
        const uint32_t u0 = wave_sum(n_basic), u1 = wave_sum(n_keep);
        const float f0 = wave_min(dmin), f1 = wave_max(dmax);
        if ((tid & 63) == 0) {
            const int wv = tid >> 6;
            s_red.d[0][wv] = t0; s_red.d[1][wv] = t1; s_red.d[2][wv] = t2; s_red.d[3][wv] = t3;
            s_red.u[0][wv] = u0; s_red.u[1][wv] = u1;
            s_red.f[0][wv] = f0; s_red.f[1][wv] = f1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        EvalPartial out{};
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        uint32_t u[2] = {0u, 0u};
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int wv = 0; wv < 8; wv++) {
            for (int q = 0; q < 4; q++) d[q] += s_red.d[q][wv];
            u[0] += s_red.u[0][wv]; u[1] += s_red.u[1][wv];
            lo = fminf(lo, s_red.f[0][wv]); hi = fmaxf(hi, s_red.f[1][wv]);
        }
        out.sq_full = d[0]; out.sq_keep = d[1]; out.m_full = d[2]; out.m_static = d[3];
        out.n_basic = u[0]; out.n_keep = u[1]; out.dmin = lo; out.dmax = hi;
        const size_t wg = ((size_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        p.partial[wg] = out;
    }
}

// One workgroup: the partials in a fixed order (thread t takes t, t + 512, ...; wave sums; the waves from 0 up) and the row.
__global__ void __launch_bounds__(EVAL_THREADS) frame_eval_finish_kernel(const EvalPartial *__restrict__ partial, int nwg, double count,
                                                                         int has_mask, int has_depth, lvdgs_frame_eval_row *row) {
    __shared__ EvalRed s_red;
    __shared__ unsigned long long s_cnt[2][8];
    const int tid = threadIdx.x;
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long n[2] = {0ull, 0ull};
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int i = tid; i < nwg; i += EVAL_THREADS) {
        const EvalPartial q = partial[i];
        d[0] += q.sq_full; d[1] += q.sq_keep; d[2] += q.m_full; d[3] += q.m_static;
        n[0] += q.n_basic; n[1] += q.n_keep;
        lo = fminf(lo, q.dmin); hi = fmaxf(hi, q.dmax);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) d[q] = wave_sum(d[q]);
    n[0] = wave_sum(n[0]); n[1] = wave_sum(n[1]);
    lo = wave_min(lo); hi = wave_max(hi);
    if ((tid & 63) == 0) {
        const int wv = tid >> 6;
#pragma unroll
        for (int q = 0; q < 4; q++) s_red.d[q][wv] = d[q];
        s_cnt[0][wv] = n[0]; s_cnt[1][wv] = n[1];
        s_red.f[0][wv] = lo; s_red.f[1][wv] = hi;
    }
    __syncthreads();
    if (tid == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        unsigned long long c[2] = {0ull, 0ull};
        float mn = __builtin_inff(), mx = -__builtin_inff();
        for (int wv = 0; wv < 8; wv++) {
            for (int q = 0; q < 4; q++) t[q] += s_red.d[q][wv];
            c[0] += s_cnt[0][wv]; c[1] += s_cnt[1][wv];
            mn = fminf(mn, s_red.f[0][wv]); mx = fmaxf(mx, s_red.f[1][wv]);
        }
        uint32_t flags = 0u;
        if (has_mask) flags |= LVDGS_FRAME_EVAL_HAS_MASK;
        if (has_depth) flags |= LVDGS_FRAME_EVAL_HAS_DEPTH;
        if (has_depth && mn == mx) flags |= LVDGS_FRAME_EVAL_DEPTH_CONSTANT;
        row->sum_sq_full = t[0];
        row->sum_sq_static = has_mask ? t[1] : t[0];
        row->n_basic = c[0];
        row->n_keep = has_mask ? c[1] : c[0];
        row->ssim_full = t[2] / count;
        row->ssim_static = has_mask ? t[3] / count : t[2] / count;
        row->depth_min = has_depth ? mn : 0.f;
        row->depth_max = has_depth ? mx : 0.f;
        row->flags = flags;
        row->reserved = 0u;
    }
}

// depth8 = (uint8)(((d - min) / (max - min)) * 255.0f), float32 as written; a constant map: 0 (include/lvdgs.h)
__global__ void __launch_bounds__(256) frame_eval_depth8_kernel(const float *__restrict__ depth, size_t n, const lvdgs_frame_eval_row *row,
                                                                uint8_t *__restrict__ out) {
    const float mn = row->depth_min, mx = row->depth_max;
    const float range = mx - mn;
    const bool constant = mn == mx;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float q = ((depth[i] - mn) / range) * 255.0f;
        out[i] = constant ? (uint8_t)0 : (uint8_t)q;
    }
}

void fill_eval_window(float (&win)[EW]) {
    // the window upstream builds in float32: g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), w = g / g.sum().  torch's g.sum() is 3.7592327594757080,
    // the float64 sum of the eleven float32 values rounded once -- what is taken here.  Adding them one by one in float32 (ssim.hip's
    // fill_window) ends an ulp lower, 3.7592325210571289: nine taps differ in their last bit, the window then sums to 1 + 4.4e-8 instead of
    // 1 - 3.1e-8, and wherever the images are smooth that shifts S - (A^2 + B^2) against C2 with one sign: 2.5e-6 on the mean SSIM of the
    // toy scene's frames, more than the 2e-6 this call is held to against the float64 statement of upstream's code.
    float g[EW];
    double sum = 0.0;
    for (int k = 0; k < EW; k++) { g[k] = expf(-(float)((k - ER) * (k - ER)) / (2.f * 1.5f * 1.5f)); sum += (double)g[k]; }
    const float total = (float)sum;
    for (int k = 0; k < EW; k++) win[k] = g[k] / total;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_frame_eval_scratch_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    const size_t nwg = (size_t)cdiv(width, ET) * cdiv(height, ET) * 3;
    return align256(nwg * sizeof(EvalPartial) + 256);
}

int lvdgs_frame_eval(const lvdgs_frame_eval_args *a, void *stream) {
    if (!a || a->width <= 0 || a->height <= 0) { set_error("frame eval: bad image size"); return LVDGS_E_INVALID; }
    if (!a->render || !a->gt_image || !a->out_row || !a->scratch) { set_error("frame eval: render / gt_image / out_row / scratch is NULL"); return LVDGS_E_INVALID; }
    if (a->depth8 && !a->depth) { set_error("frame eval: depth8 without depth"); return LVDGS_E_INVALID; }
    if (a->scratch_bytes < lvdgs_frame_eval_scratch_bytes(a->width, a->height)) { set_error("frame eval: scratch too small"); return LVDGS_E_INVALID; }
    if (((uintptr_t)a->out_row | (uintptr_t)a->scratch) & 7u) { set_error("frame eval: out_row and scratch must be 8-byte aligned"); return LVDGS_E_INVALID; }
    const dim3 grid(cdiv(a->width, ET), cdiv(a->height, ET), 3);
    if (grid.y > 65535u) { set_error("frame eval: more than 65535 tile rows"); return LVDGS_E_RANGE; }
    if ((uint64_t)grid.x * grid.y * grid.z > (uint64_t)INT32_MAX) { set_error("frame eval: more than 2^31 - 1 workgroups"); return LVDGS_E_RANGE; }
    hipStream_t s = (hipStream_t)stream;
    EvalParams p{};
    p.W = a->width; p.H = a->height;
    p.render = a->render; p.gt = a->gt_image; p.mask = a->static_mask; p.bg = a->bg; p.depth = a->depth;
    p.pred8 = a->pred8; p.gt8 = a->gt8; p.res8 = a->residual8;
    p.partial = (EvalPartial *)a->scratch;
    fill_eval_window(p.win);
    const int nwg = (int)(grid.x * grid.y * grid.z);
    lvdgs_frame_eval_row *row = (lvdgs_frame_eval_row *)a->out_row;
    if (int e = launch("frame_eval", 0, s, frame_eval_kernel, grid, dim3(EVAL_THREADS), 0, p)) return e;
    if (int e = launch("frame_eval_finish", 0, s, frame_eval_finish_kernel, dim3(1), dim3(EVAL_THREADS), 0, (const EvalPartial *)p.partial, nwg,
            (double)a->width * a->height * 3.0, a->static_mask ? 1 : 0, a->depth ? 1 : 0, row)) return e;
    if (a->depth8) {
        const size_t n = (size_t)a->width * a->height;
        const size_t blocks = (n + 255) / 256;
        if (int e = launch("frame_eval_depth8", 0, s, frame_eval_depth8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, a->depth, n,
                (const lvdgs_frame_eval_row *)row, a->depth8)) return e;
    }
    return LVDGS_OK;
}

}  // extern "C"
