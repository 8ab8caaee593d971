// Patch-based pointmap scale alignment (LVD-GS Algorithm 1; reference utils/depth_utils.py process_depth, called for every
// keyframe after the first, utils/slam_frontend.py:1380-1405): the scale of a keyframe's mono depth against the rendered depth,
// then the depth map the keyframe's Gaussians are seeded from.  Semantics: include/lvdgs.h, DESIGN.md section "Keyframe depth".
//
// One launch per iteration of the algorithm, all enqueued up front, then one fill launch:
//   depth_align_iter_kernel : one wave64 per patch (four patches per 256-thread workgroup).  Patch statistics in float64 from the
//                             float32 loads (two passes: the means, then the centred second moments), the accurate-pixel test, and
//                             the patch's partial sums (passing flag, accurate count, sum r, sum m over the accurate pixels).  The
//                             workgroup sums its four patches in order into a slab; the LAST workgroup to arrive (atomic ticket)
//                             sums the slab in a fixed order -- bit-deterministic whatever the arrival order -- and runs the
//                             algorithm's control flow on the state block.  No workgroup ever waits on another.
//   depth_align_fill_kernel : error mask and final depth from the final scale, in float32 as NumPy forms them.
// A launch whose state is not "running" stands down (every workgroup returns before it takes a ticket), as the pose step's sticky
// converged flag lets the tracking loop enqueue iterations ahead; the host reads the state once, through pinned memory.
#include <math.h>
#include <string.h>

#include "common.hpp"
#include "device_utils.hpp"

namespace lvdgs {
namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_PATCHES_PER_BLOCK = DA_THREADS / WAVE;
constexpr int DA_FILL_THREADS = 256;

// The state block at the start of scratch (the host copy: LVDGS_DEPTH_ALIGN_STATE_WORDS words of int32 in the header's order).
struct DepthAlignState {
    float s;               // current scale
    float s_prev;          // the scale at the top of the last iteration run
    int32_t status;        // LVDGS_DEPTH_ALIGN_*
    int32_t k;             // the last iteration run (-1: none)
    int32_t num_accurate;  // what the algorithm returns as num_accurate_pixels
    int32_t patch_num;     // passing patches of the last iteration run
    int32_t count;         // accurate pixels of the last iteration run
    int32_t filled;        // 1 once the fill launch has run
};
static_assert(sizeof(DepthAlignState) == LVDGS_DEPTH_ALIGN_STATE_WORDS * 4, "state block layout");

struct PatchPartial {     // one per workgroup (its four patches summed in order)
    double sum_r, sum_m;
    int32_t count, passed;
    int32_t pad[2];
};

struct DepthAlignHeader {
    DepthAlignState st;
    uint32_t ticket;      // zero between launches (the reducer resets it)
    uint32_t pad[63];
};

struct AlignParams {
    int W, H, p, npx, npatch;
    int max_iter;
    double mean_thr, std_thr, err_thr;
    float eps, final_thr;
    int64_t min_accurate;
    const float *r, *m;
    DepthAlignHeader *hdr;
    PatchPartial *slab;
    int32_t *host_state;   // device address of the caller's pinned state words
    float *final_depth;
    uint8_t *error_mask;
};

// Top of iteration k+1: stop when |s - s_prev| < eps (float32 difference, eps rounded to float32) unless s is still 1.
__host__ __device__ inline bool top_stop(float s, float s_prev, float eps) {
    const float d = fabsf(s - s_prev);
    return d < eps && s != 1.0f;
}

// The one host block that is not sealed (seal_host_block): a state without a tag, mirrored by every launch that changes it -- several
// times per call -- and read by the host only behind its wait for the stream, where the last mirror is complete.
__device__ __forceinline__ void mirror_state(const AlignParams &P, const DepthAlignState &st) {
    P.hdr->st = st;
    if (P.host_state) {
        const int32_t *w = reinterpret_cast<const int32_t *>(&st);
        for (int i = 0; i < LVDGS_DEPTH_ALIGN_STATE_WORDS; i++) P.host_state[i] = w[i];
        __threadfence_system();
    }
}

// Iteration k.  force: the scale at the top is s_in (k = 0, or the iteration after a remedy) and the status is not looked at.
__global__ void __launch_bounds__(DA_THREADS) depth_align_iter_kernel(AlignParams P, int k, int force, float s_in) {
    __shared__ double s_sum[2][DA_PATCHES_PER_BLOCK];
    __shared__ int s_cnt[2][DA_PATCHES_PER_BLOCK];
    __shared__ int s_last;
    float s;
    if (force) {
        s = s_in;
    } else {
        if (P.hdr->st.status != LVDGS_DEPTH_ALIGN_RUNNING) return;   // uniform over the launch: the state changes only in its reducer
        s = P.hdr->st.s;
    }
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int patch = blockIdx.x * DA_PATCHES_PER_BLOCK + wave;
    double acc_r = 0.0, acc_m = 0.0;
    int acc_n = 0, passed = 0;
    if (patch < P.npatch) {
        const int py = patch / P.npx, px = patch - py * P.npx;
        const int y0 = py * P.p, x0 = px * P.p;
        const int ph = min(P.p, P.H - y0), pw = min(P.p, P.W - x0), n = ph * pw;
        const float *r = P.r + (size_t)y0 * P.W + x0, *m = P.m + (size_t)y0 * P.W + x0;
        // pass 1: means (the scaled mono depth as NumPy forms it: a float32 product)
        double sr = 0.0, sm = 0.0;
        for (int i = lane; i < n; i += WAVE) {
            const int yy = i / pw, xx = i - yy * pw;
            const size_t o = (size_t)yy * P.W + xx;
            sr += (double)r[o];
            sm += (double)(m[o] * s);
        }
        const double mr = wave_sum(sr) / n, mm = wave_sum(sm) / n;
        // pass 2: population standard deviations
        double vr = 0.0, vm = 0.0;
        for (int i = lane; i < n; i += WAVE) {
            const int yy = i / pw, xx = i - yy * pw;
            const size_t o = (size_t)yy * P.W + xx;
            const double dr = (double)r[o] - mr, dm = (double)(m[o] * s) - mm;
            vr += dr * dr;
            vm += dm * dm;
        }
        const double sdr = sqrt(wave_sum(vr) / n), sdm = sqrt(wave_sum(vm) / n);
        // (NaN anywhere makes both comparisons false)
        if (fabs(mr - mm) < P.mean_thr * mm && fabs(sdr - sdm) < P.std_thr * sdm) {
            passed = 1;
            for (int i = lane; i < n; i += WAVE) {
                const int yy = i / pw, xx = i - yy * pw;
                const size_t o = (size_t)yy * P.W + xx;
                const float rv = r[o], mv = m[o];
                const double a = ((double)rv - mr) / (sdr + 1e-6), b = ((double)(mv * s) - mm) / (sdm + 1e-6);
                if (fabs(a - b) < P.err_thr) {
                    acc_n += 1;
                    acc_r += (double)rv;
                    acc_m += (double)mv;   // the scale update reads the UNSCALED mono depth
                }
            }
            acc_n = wave_sum(acc_n);
            acc_r = wave_sum(acc_r);
            acc_m = wave_sum(acc_m);
        }
    }
    if (lane == 0) {
        s_sum[0][wave] = acc_r; s_sum[1][wave] = acc_m;
        s_cnt[0][wave] = acc_n; s_cnt[1][wave] = passed;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        PatchPartial q{};
        for (int w = 0; w < DA_PATCHES_PER_BLOCK; w++) {
            q.sum_r += s_sum[0][w]; q.sum_m += s_sum[1][w];
            q.count += s_cnt[0][w]; q.passed += s_cnt[1][w];
        }
        P.slab[blockIdx.x] = q;
        // publish the slab entry (release, agent scope), then draw a ticket
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(&P.hdr->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;

    // ---- the reducer: fixed-order sums of the slab, then the control flow of iteration k ----
    double tr = 0.0, tm = 0.0;
    long long tc = 0, tp = 0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += DA_THREADS) {
        const PatchPartial q = P.slab[i];
        tr += q.sum_r; tm += q.sum_m; tc += q.count; tp += q.passed;
    }
    __shared__ double red_d[2][DA_THREADS];
    __shared__ long long red_i[2][DA_THREADS];
    red_d[0][threadIdx.x] = tr; red_d[1][threadIdx.x] = tm;
    red_i[0][threadIdx.x] = tc; red_i[1][threadIdx.x] = tp;
    __syncthreads();
    for (int h = DA_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red_d[0][threadIdx.x] += red_d[0][threadIdx.x + h]; red_d[1][threadIdx.x] += red_d[1][threadIdx.x + h];
            red_i[0][threadIdx.x] += red_i[0][threadIdx.x + h]; red_i[1][threadIdx.x] += red_i[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double sum_r = red_d[0][0], sum_m = red_d[1][0];
    const int count = (int)red_i[0][0];
    DepthAlignState st = P.hdr->st;
    st.k = k;
    st.patch_num = (int)red_i[1][0];
    st.count = count;
    st.s_prev = s;
    st.s = s;
    st.filled = 0;
    if (count < P.min_accurate && (k == 2 || k == 3)) {
        st.num_accurate = count;                    // the host applies the scale remedy
        st.status = LVDGS_DEPTH_ALIGN_REMEDY;
    } else {
        st.num_accurate = 0;
        if (count > 0 && (k < 2 || count >= P.min_accurate)) {
            st.s = (float)((sum_r / count) / (sum_m / count));
            st.num_accurate = count;
        }
        if (k + 1 >= P.max_iter) st.status = LVDGS_DEPTH_ALIGN_EXHAUSTED;
        else if (top_stop(st.s, s, P.eps)) st.status = LVDGS_DEPTH_ALIGN_CONVERGED;
        else st.status = LVDGS_DEPTH_ALIGN_RUNNING;
    }
    P.hdr->ticket = 0;   // ready for the next launch (kernel boundaries order it)
    mirror_state(P, st);
}

// force: fill with s_in whatever the status (after a remedy, or with max_iter == 0); otherwise with the state's scale unless the
// state asks for a remedy.
__global__ void __launch_bounds__(DA_FILL_THREADS) depth_align_fill_kernel(AlignParams P, int force, float s_in, int force_status) {
    float s;
    if (force) {
        s = s_in;
    } else {
        const int status = P.hdr->st.status;
        if (status == LVDGS_DEPTH_ALIGN_REMEDY || status == LVDGS_DEPTH_ALIGN_RUNNING) return;
        s = P.hdr->st.s;
    }
    const int64_t n = (int64_t)P.W * P.H;
    const float thr = P.final_thr;
    for (int64_t i = (int64_t)blockIdx.x * DA_FILL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DA_FILL_THREADS) {
        const float r = P.r[i];
        const float ms = P.m[i] * s;
        const float rel = fabsf(r - ms) / (ms + 1e-8f);
        const bool err = rel > thr || r == 0.0f;
        P.final_depth[i] = err ? ms : r;
        P.error_mask[i] = err ? 1 : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        DepthAlignState st = P.hdr->st;
        if (P.max_iter == 0) { st = DepthAlignState{}; st.k = -1; }   // no iteration: nothing of an earlier call may show
        if (force) {
            st.s = s_in;
            if (force_status >= 0) st.status = force_status;
        }
        st.filled = 1;
        mirror_state(P, st);
    }
}

int fill_blocks(int W, int H) {
    const int64_t n = (int64_t)W * H;
    const int64_t b = (n + DA_FILL_THREADS - 1) / DA_FILL_THREADS;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

namespace {

int iter_blocks(int W, int H, int p) {
    const int64_t npatch = (int64_t)cdiv(H, p) * cdiv(W, p);
    return (int)((npatch + DA_PATCHES_PER_BLOCK - 1) / DA_PATCHES_PER_BLOCK);
}

// the scratch: the header, a partial per workgroup of the iteration (a size the call refuses: the header alone)
size_t align_layout(int W, int H, int p, AlignParams *P, void *base) {
    Carver<AlignParams> c(P, base);
    c(c.v.hdr, 1); c(c.v.slab, W <= 0 || H <= 0 || p < 1 ? 0 : (size_t)iter_blocks(W, H, p));
    return c.off;
}

int align_params(const lvdgs_depth_align_args *a, AlignParams &P) {
    if (!a) { set_error("depth align: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width <= 0 || a->height <= 0 || (int64_t)a->width * a->height > INT32_MAX) {
        set_error("depth align: bad image size %dx%d", a->width, a->height); return LVDGS_E_INVALID;
    }
    if (a->patch_size < 1 || a->patch_size > LVDGS_DEPTH_ALIGN_MAX_PATCH) {
        set_error("depth align: patch_size %d outside 1..%d", a->patch_size, LVDGS_DEPTH_ALIGN_MAX_PATCH); return LVDGS_E_INVALID;
    }
    if (a->max_iter < 0) { set_error("depth align: max_iter < 0"); return LVDGS_E_INVALID; }
    if (!a->render_depth || !a->mono_depth || !a->final_depth || !a->error_mask || !a->host_state || !a->scratch) {
        set_error("depth align: render_depth / mono_depth / final_depth / error_mask / host_state / scratch is NULL"); return LVDGS_E_INVALID;
    }
    P = AlignParams{};
    if (a->scratch_bytes < align_layout(a->width, a->height, a->patch_size, &P, a->scratch)) {
        set_error("depth align: scratch too small"); return LVDGS_E_INVALID;
    }
    P.W = a->width; P.H = a->height; P.p = a->patch_size;
    P.npx = cdiv(a->width, a->patch_size);
    P.npatch = cdiv(a->height, a->patch_size) * P.npx;
    P.max_iter = a->max_iter;
    P.mean_thr = a->mean_threshold; P.std_thr = a->std_threshold; P.err_thr = a->error_threshold;
    P.eps = (float)a->epsilon; P.final_thr = (float)a->final_error_threshold;
    P.min_accurate = (int64_t)(a->min_accurate_pixels_ratio * (double)((int64_t)a->width * a->height));   // Python's int(ratio * H * W)
    P.r = a->render_depth; P.m = a->mono_depth;
    P.final_depth = a->final_depth; P.error_mask = a->error_mask;
    if (int e = host_block_address(a->host_state, "depth align", &P.host_state)) return e;
    return LVDGS_OK;
}

int launch_iter(const AlignParams &P, int k, int force, float s_in, hipStream_t s) {
    if (int e = launch("depth_align_iter", 0, s, depth_align_iter_kernel, dim3(iter_blocks(P.W, P.H, P.p)), dim3(DA_THREADS), 0, P, k, force, s_in)) return e;
    return LVDGS_OK;
}

int launch_fill(const AlignParams &P, int force, float s_in, int force_status, hipStream_t s) {
    if (int e = launch("depth_align_fill", 0, s, depth_align_fill_kernel, dim3(fill_blocks(P.W, P.H)), dim3(DA_FILL_THREADS), 0, P, force, s_in, force_status)) return e;
    return LVDGS_OK;
}

}  // namespace

extern "C" {

size_t lvdgs_depth_align_scratch_bytes(int32_t width, int32_t height, int32_t patch_size) {
    return align_layout(width, height, patch_size, nullptr, nullptr);
}

int lvdgs_depth_align(const lvdgs_depth_align_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    AlignParams P;
    if (int e = align_params(a, P)) return e;
    if (P.max_iter == 0) return launch_fill(P, 1, 1.0f, LVDGS_DEPTH_ALIGN_EXHAUSTED, s);
    if (int e = launch_iter(P, 0, 1, 1.0f, s)) return e;
    for (int k = 1; k < P.max_iter; k++)
        if (int e = launch_iter(P, k, 0, 0.0f, s)) return e;
    return launch_fill(P, 0, 0.0f, -1, s);
}

int lvdgs_depth_align_resume(const lvdgs_depth_align_args *a, float scale, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    AlignParams P;
    if (int e = align_params(a, P)) return e;
    const volatile int32_t *hs = a->host_state;
    const int status = hs[2], k = hs[3];
    if (status != LVDGS_DEPTH_ALIGN_REMEDY || (k != 2 && k != 3)) {
        set_error("depth align resume: the state asks for no remedy (status %d, k %d)", status, k); return LVDGS_E_INVALID;
    }
    float s_prev;
    memcpy(&s_prev, (const void *)&hs[1], sizeof(float));
    if (k == 2 && P.max_iter > 3 && !top_stop(scale, s_prev, P.eps)) {
        if (int e = launch_iter(P, 3, 1, scale, s)) return e;
        return launch_fill(P, 0, 0.0f, -1, s);
    }
    // k == 3 (the remedy's scale is final), or k == 2 with no iteration left / the top of iteration 3 stopping
    const int final_status = k == 2 && P.max_iter > 3 ? LVDGS_DEPTH_ALIGN_CONVERGED : LVDGS_DEPTH_ALIGN_EXHAUSTED;
    return launch_fill(P, 1, scale, final_status, s);
}

}  // extern "C"
