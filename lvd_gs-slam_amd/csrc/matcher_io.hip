// What surrounds the matcher's network in the reference's utils/init_pose.py and utils/depth_utils.py, on the device:
//   lvdgs_format_image      : torch_images_to_dust3r_format of one frame -- quantise to uint8, PIL's 8-bit resize (LANCZOS / BICUBIC),
//                             centre crop, normalise -- bit-exact with PIL.  The reference copies the frame to the host for it.
//   lvdgs_match_depth_scale : find_scale's arithmetic -- two depth maps sampled bilinearly at the raster's matches, a ratio of means.
// Semantics: include/lvdgs.h, DESIGN.md section 4e.  Parity of the bilinear rule with cv2.resize is UNPINNED (OpenCV interpolates in
// float32 with its own coefficient tables; it is not installed where this was written): the rule is the one the header states, in float64.
//
// Both are launch-bound: two launches for an image (horizontal pass over the rows the vertical pass reads, then vertical pass + crop +
// normalise), one for a scale.  The resize's coefficient tables are made on the host in float64 (lvdgs_format_table, PIL's
// precompute_coeffs + normalize_coeffs_8bpc) and live on the device; the kernels do the integer sums.  No workgroup waits on another;
// every loop is bounded.
#include <math.h>

#include "common.hpp"

namespace lvdgs {
namespace {

constexpr int FMT_THREADS = 256;
constexpr int FMT_PRECISION_BITS = 32 - 8 - 2;   // PIL's PRECISION_BITS: coefficients are fixed point with 22 fractional bits
constexpr int MS_THREADS = 1024;

// ---- PIL's filters (src/libImaging/Resample.c) ----
double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
double lanczos_filter(double x) {   // truncated sinc, support 3
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}
double bicubic_filter(double x) {   // Keys, a = -0.5, support 2
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
double filter_support(int filter) { return filter == LVDGS_FORMAT_LANCZOS ? 3.0 : 2.0; }

// the window of output sample xx of a pass from in to out samples: first input sample and their number
void pass_window(int in, int out, int filter, int xx, int *xmin, int *count, double *center_out, double *fs_out) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = filter_support(filter) * fs;
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in) hi = in;
    *xmin = lo; *count = hi - lo;
    if (center_out) *center_out = center;
    if (fs_out) *fs_out = fs;
}

int pass_taps(int in, int out, int filter) {
    if (in == out) return 1;                     // the pass is skipped: the table is the identity
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(filter_support(filter) * fs) * 2 + 1;
}

int make_plan(int W, int H, int size, lvdgs_format_plan *p, bool quiet) {
    if (W <= 0 || H <= 0) { if (!quiet) set_error("format_image: bad image size %dx%d", W, H); return LVDGS_E_INVALID; }
    if (size == 224) { if (!quiet) set_error("format_image: size 224 (the square-crop rule) is not supported"); return LVDGS_E_INVALID; }
    if (size < 16 || size > LVDGS_FORMAT_MAX_SIZE) { if (!quiet) set_error("format_image: size %d outside 16..%d", size, LVDGS_FORMAT_MAX_SIZE); return LVDGS_E_INVALID; }
    if (W > LVDGS_FORMAT_MAX_EDGE || H > LVDGS_FORMAT_MAX_EDGE) { if (!quiet) set_error("format_image: an image edge beyond %d", LVDGS_FORMAT_MAX_EDGE); return LVDGS_E_INVALID; }
    const int S = W > H ? W : H;
    const int w = (int)nearbyint((double)W * size / S), h = (int)nearbyint((double)H * size / S);   // Python's round: half to even
    const int cx = w / 2, cy = h / 2;
    int halfw = ((2 * cx) / 16) * 8, halfh = ((2 * cy) / 16) * 8;
    if (w == h) halfh = 3 * halfw / 4;
    if (halfw < 1 || halfh < 1) { if (!quiet) set_error("format_image: a %dx%d image leaves size %d an empty raster", W, H, size); return LVDGS_E_INVALID; }
    p->resized_width = w; p->resized_height = h;
    p->filter = S > size ? LVDGS_FORMAT_LANCZOS : LVDGS_FORMAT_BICUBIC;
    p->crop_x = cx - halfw; p->crop_y = cy - halfh;
    p->out_width = 2 * halfw; p->out_height = 2 * halfh;
    p->taps_x = pass_taps(W, w, p->filter); p->taps_y = pass_taps(H, h, p->filter);
    int r0 = H, r1 = 0;
    for (int y = 0; y < p->out_height; y++) {
        int lo, n;
        if (H == h) { lo = p->crop_y + y; n = 1; }
        else pass_window(H, h, p->filter, p->crop_y + y, &lo, &n, nullptr, nullptr);
        if (lo < r0) r0 = lo;
        if (lo + n > r1) r1 = lo + n;
    }
    p->row_first = r0; p->row_count = r1 - r0;
    return LVDGS_OK;
}

struct FmtParams {
    int W, H, W1, H1, taps_x, taps_y, row_first, row_count;
    const float *image;
    const int32_t *table_x, *table_y;
    uint8_t *rows;          // 3 * row_count * W1: the horizontal pass' result
    float *out;
    uint8_t *quantised;
};

__device__ __forceinline__ int quantise(float x) {   // uint8(trunc(x * 255)); outside 0..255 clamps, NaN -> 0
    const float v = x * 255.0f;
    return v != v ? 0 : (int)fminf(fmaxf(v, 0.0f), 255.0f);
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> FMT_PRECISION_BITS, 0), 255); }

// rows row_first .. row_first + row_count - 1 of the image, resized horizontally to the crop's columns.  grid: (W1 / 256, row_count, 3)
__global__ void __launch_bounds__(FMT_THREADS) format_rows_kernel(FmtParams P) {
    const int x = blockIdx.x * FMT_THREADS + threadIdx.x, r = blockIdx.y, c = blockIdx.z;
    if (x >= P.W1) return;
    const int32_t *e = P.table_x + (size_t)x * (2 + P.taps_x);
    const int xmin = e[0], n = min(e[1], P.taps_x);
    const float *src = P.image + ((size_t)c * P.H + (P.row_first + r)) * P.W;
    int acc = 1 << (FMT_PRECISION_BITS - 1);
    for (int t = 0; t < n; t++) {
        const int col = xmin + t;
        if (col >= 0 && col < P.W) acc += e[2 + t] * quantise(src[col]);
    }
    P.rows[((size_t)c * P.row_count + r) * P.W1 + x] = (uint8_t)clip8(acc);
}

// the vertical pass over those rows, the normalisation, and the uint8 copy when it is asked for.  grid: (W1 / 256, H1, 3)
__global__ void __launch_bounds__(FMT_THREADS) format_columns_kernel(FmtParams P) {
    const int x = blockIdx.x * FMT_THREADS + threadIdx.x, y = blockIdx.y, c = blockIdx.z;
    if (x >= P.W1) return;
    const int32_t *e = P.table_y + (size_t)y * (2 + P.taps_y);
    const int ymin = e[0] - P.row_first, n = min(e[1], P.taps_y);
    const uint8_t *src = P.rows + (size_t)c * P.row_count * P.W1 + x;
    int acc = 1 << (FMT_PRECISION_BITS - 1);
    for (int t = 0; t < n; t++) {
        const int r = ymin + t;
        if (r >= 0 && r < P.row_count) acc += e[2 + t] * (int)src[(size_t)r * P.W1];
    }
    const int q = clip8(acc);
    P.out[((size_t)c * P.H1 + y) * P.W1 + x] = ((float)q / 255.0f - 0.5f) / 0.5f;
    if (P.quantised) P.quantised[((size_t)y * P.W1 + x) * 3 + c] = (uint8_t)q;
}

struct ScaleParams {
    int M, W1, H1, Wa, Ha, Wb, Hb;
    const int32_t *m1;
    const float *m2;
    const float *d1, *d2;
    int32_t *host_state;    // device address of the caller's pinned block
};

// one axis of the bilinear rule: the first source sample and the weight of the next one
__device__ __forceinline__ void axis_sample(int i, int n_src, int n_dst, int *s_out, double *t_out) {
    const double f = ((double)i + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
    const double fl = floor(f);
    int s = (int)fl;
    double t = f - fl;
    if (s < 0) { s = 0; t = 0.0; }
    if (s >= n_src - 1) { s = n_src - 1; t = 0.0; }
    *s_out = s; *t_out = t;
}

__device__ __forceinline__ double bilinear(const float *d, int W, int H, int x, int y, int W1, int H1) {
    int sx, sy;
    double tx, ty;
    axis_sample(x, W, W1, &sx, &tx);
    axis_sample(y, H, H1, &sy, &ty);
    const int sx1 = min(sx + 1, W - 1), sy1 = min(sy + 1, H - 1);
    const double a = (double)d[(size_t)sy * W + sx], b = (double)d[(size_t)sy * W + sx1];
    const double c = (double)d[(size_t)sy1 * W + sx], e = (double)d[(size_t)sy1 * W + sx1];
    return (1.0 - ty) * ((1.0 - tx) * a + tx * b) + ty * ((1.0 - tx) * c + tx * e);
}

// One workgroup.  Thread t sums the matches t, t + 1024, ... in that order; the threads' sums are then added pairwise in LDS, the
// same tree in every call.
__global__ void __launch_bounds__(MS_THREADS) match_scale_kernel(ScaleParams P) {
    __shared__ double s_a[MS_THREADS], s_b[MS_THREADS];
    __shared__ int s_n[MS_THREADS];
    const int tid = threadIdx.x;
    double sum1 = 0.0, sum2 = 0.0;
    int n = 0;
    for (int i = tid; i < P.M; i += MS_THREADS) {
        const int x1 = P.m1[2 * i], y1 = P.m1[2 * i + 1];
        const float u = P.m2[2 * i], v = P.m2[2 * i + 1];
        const bool inside = x1 >= 0 && x1 < P.W1 && y1 >= 0 && y1 < P.H1 && u > -1.0f && u < (float)P.W1 && v > -1.0f && v < (float)P.H1;   // (NaN: outside)
        if (!inside) continue;
        const int x2 = (int)u, y2 = (int)v;   // toward zero
        const double a = bilinear(P.d1, P.Wa, P.Ha, x1, y1, P.W1, P.H1);
        const double b = bilinear(P.d2, P.Wb, P.Hb, x2, y2, P.W1, P.H1);
        if (a > 0.0 && a < (double)INFINITY && b > 0.0 && b < (double)INFINITY) { sum1 += a; sum2 += b; n++; }
    }
    s_a[tid] = sum1; s_b[tid] = sum2; s_n[tid] = n;
    __syncthreads();
    for (int o = MS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { s_a[tid] += s_a[tid + o]; s_b[tid] += s_b[tid + o]; s_n[tid] += s_n[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        // NOT sealed (device_utils.hpp: seal_host_block), like pnp.hip's write_state: the host's wait for the stream is what makes the block
        // complete.  Measured on the MI355X: with volatile payload stores and the seal the call sat at or above the top of its run-to-run
        // spread (3 to 6 us of 45).
        int32_t *w = P.host_state;
        const int cnt = s_n[0];
        const float scale = cnt > 0 ? (float)((s_a[0] / (double)cnt) / (s_b[0] / (double)cnt)) : 0.0f;
        w[1] = P.M; w[2] = cnt; w[3] = __float_as_int(scale); w[4] = 0; w[5] = 0; w[6] = 0; w[7] = 0;
        double *sums = reinterpret_cast<double *>(w + LVDGS_MATCH_SCALE_STATE_WORDS);
        sums[0] = s_a[0]; sums[1] = s_b[0];
        w[0] = cnt > 0 ? LVDGS_MATCH_SCALE_OK : LVDGS_MATCH_SCALE_NO_VALID;
        __threadfence_system();
    }
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

int lvdgs_format_plan_query(int32_t width, int32_t height, int32_t size, lvdgs_format_plan *plan) {
    if (!plan) { set_error("format_image: plan is NULL"); return LVDGS_E_INVALID; }
    return make_plan(width, height, size, plan, false);
}

int lvdgs_format_table(int32_t in, int32_t out, int32_t filter, int32_t first, int32_t count, int32_t *table) {
    if (in <= 0 || out <= 0 || in > LVDGS_FORMAT_MAX_EDGE || out > LVDGS_FORMAT_MAX_EDGE) { set_error("format_table: bad pass %d -> %d", in, out); return LVDGS_E_INVALID; }
    if (filter != LVDGS_FORMAT_LANCZOS && filter != LVDGS_FORMAT_BICUBIC) { set_error("format_table: unknown filter %d", filter); return LVDGS_E_INVALID; }
    if (first < 0 || count < 0 || (int64_t)first + count > out) { set_error("format_table: entries %d .. %d outside 0 .. %d", first, first + count, out); return LVDGS_E_INVALID; }
    if (!table) { set_error("format_table: table is NULL"); return LVDGS_E_INVALID; }
    const int K = pass_taps(in, out, filter);
    double *k = new double[K];
    for (int j = 0; j < count; j++) {
        int32_t *e = table + (size_t)j * (2 + K);
        const int xx = first + j;
        for (int t = 0; t < K; t++) e[2 + t] = 0;
        if (in == out) { e[0] = xx; e[1] = 1; e[2] = 1 << FMT_PRECISION_BITS; continue; }
        int xmin, n;
        double center, fs;
        pass_window(in, out, filter, xx, &xmin, &n, &center, &fs);
        const double ss = 1.0 / fs;
        double ww = 0.0;
        for (int x = 0; x < n; x++) {
            const double a = (x + xmin - center + 0.5) * ss;
            const double w = filter == LVDGS_FORMAT_LANCZOS ? lanczos_filter(a) : bicubic_filter(a);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < n; x++) {
            if (ww != 0.0) k[x] /= ww;
            e[2 + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << FMT_PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << FMT_PRECISION_BITS));
        }
        e[0] = xmin; e[1] = n;
    }
    delete[] k;
    return LVDGS_OK;
}

size_t lvdgs_format_scratch_bytes(int32_t width, int32_t height, int32_t size) {
    lvdgs_format_plan p;
    if (make_plan(width, height, size, &p, true) != LVDGS_OK) return 0;
    return align256((size_t)3 * p.row_count * p.out_width);
}

int lvdgs_format_image(const lvdgs_format_image_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("format_image: args is NULL"); return LVDGS_E_INVALID; }
    lvdgs_format_plan p;
    if (int e = make_plan(a->width, a->height, a->size, &p, false)) return e;
    if (!a->image || !a->table_x || !a->table_y || !a->out || !a->scratch) {
        set_error("format_image: image / table_x / table_y / out / scratch is NULL"); return LVDGS_E_INVALID;
    }
    if (a->scratch_bytes < lvdgs_format_scratch_bytes(a->width, a->height, a->size)) { set_error("format_image: scratch too small"); return LVDGS_E_INVALID; }
    FmtParams P{};
    P.W = a->width; P.H = a->height; P.W1 = p.out_width; P.H1 = p.out_height; P.taps_x = p.taps_x; P.taps_y = p.taps_y;
    P.row_first = p.row_first; P.row_count = p.row_count;
    P.image = a->image; P.table_x = a->table_x; P.table_y = a->table_y;
    P.rows = reinterpret_cast<uint8_t *>(a->scratch); P.out = a->out; P.quantised = a->quantised;
    if (int e = launch("format_rows", 0, s, format_rows_kernel, dim3(cdiv(P.W1, FMT_THREADS), P.row_count, 3), dim3(FMT_THREADS), 0, P)) return e;
    if (int e = launch("format_columns", 0, s, format_columns_kernel, dim3(cdiv(P.W1, FMT_THREADS), P.H1, 3), dim3(FMT_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

int lvdgs_match_depth_scale(const lvdgs_match_scale_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("match_depth_scale: args is NULL"); return LVDGS_E_INVALID; }
    if (a->num_matches < 0) { set_error("match_depth_scale: num_matches %d < 0", a->num_matches); return LVDGS_E_INVALID; }
    if (a->raster_width <= 0 || a->raster_height <= 0) { set_error("match_depth_scale: bad raster size %dx%d", a->raster_width, a->raster_height); return LVDGS_E_INVALID; }
    if (a->width1 <= 0 || a->height1 <= 0 || a->width2 <= 0 || a->height2 <= 0) {
        set_error("match_depth_scale: bad map size %dx%d / %dx%d", a->width1, a->height1, a->width2, a->height2); return LVDGS_E_INVALID;
    }
    if (a->num_matches > 0 && (!a->matches_im1 || !a->matches_im2)) { set_error("match_depth_scale: matches_im1 / matches_im2 is NULL"); return LVDGS_E_INVALID; }
    if (!a->depth1 || !a->depth2 || !a->host_state) { set_error("match_depth_scale: depth1 / depth2 / host_state is NULL"); return LVDGS_E_INVALID; }
    ScaleParams P{};
    P.M = a->num_matches; P.W1 = a->raster_width; P.H1 = a->raster_height;
    P.Wa = a->width1; P.Ha = a->height1; P.Wb = a->width2; P.Hb = a->height2;
    P.m1 = a->matches_im1; P.m2 = a->matches_im2; P.d1 = a->depth1; P.d2 = a->depth2;
    if (int e = host_block_address(a->host_state, "match_depth_scale", &P.host_state)) return e;
    if (int e = launch("match_scale", 0, s, match_scale_kernel, dim3(1), dim3(MS_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

}  // extern "C"
