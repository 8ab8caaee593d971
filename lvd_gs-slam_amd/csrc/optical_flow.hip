// Dense Farneback optical flow and the motion mask of the masker's fallback branch, as calls with no host wait inside them (semantics:
// include/lvdgs.h; reference utils/slam_frontend.py _fallback_detection :651-672).
//
// The call is bound by launches and latency, not by HBM: a KITTI frame's five-channel planes are 9 MB at the finest level, everything
// coarser lives in L2.  So the launches follow the data dependencies, and every one of them is a tile of 64 columns -- whole 256-byte
// runs of a float row -- by a few rows, worked by four waves:
//   of_grey_kernel        (motion mask) quantisation and the integer grey of the frame
// per level, coarse to fine:
//   of_level_kernel       both images (blockIdx.z): the blur along the rows of the full-resolution bytes into LDS -- only the two source
//                         columns each output column interpolates between --, the blur along the columns and the bilinear taps out of it
//   of_polyexp_kernel     both images: the three column responses of a tile and its halo in LDS, the six row sums out of them
//   of_matrices_kernel    the coarser level's flow resized (or zero), M from it
//   of_update_kernel      one per update: a tile of M and its halo of winsize / 2 through LDS -- its row sums, the column sums out of
//                         them --, the 2 x 2 solve, and the next M at the same pixel (M depends on the flow at its own pixel only: the one
//                         grid-wide dependency is between updates; M is double-buffered)
//   of_moving_kernel      (motion mask) the threshold as one __ballot per 64 pixels
//   of_dilate_kernel      (motion mask) the bit-plane dilation of bitplane.hpp, the mask's bytes, the stored frame's advance
// Sums run over their taps in ascending order, one product at a time, as the header states them: the box sum is summed directly --
// a running sum along a row drifts in float32.  No float atomics anywhere.
#include <math.h>

#include "bitplane.hpp"

namespace lvdgs {
namespace {

constexpr int OF_THREADS = 256;
constexpr int OF_TX = 64;                // a tile's columns: one wave per tile row
constexpr int OF_ROWS = OF_THREADS / OF_TX;   // tile rows worked at a time
constexpr int OF_MAX_EDGE = 16384;
constexpr int OF_MAX_POLY = 7;
constexpr int OF_MAX_WIN = 31;
constexpr int OF_MAX_LEVELS = 8;
constexpr int OF_MIN_SIZE = 32;          // a level narrower or lower than this is not built
constexpr int OF_LEVEL_CHUNK = 32;       // of_level_kernel: source rows in LDS at a time
constexpr int OF_POLY_TY = 16;           // of_polyexp_kernel: tile rows
constexpr int OF_UPDATE_LDS_ROWS = 38;   // of_update_kernel: tile rows + halo (the widest window leaves 8 rows to a tile)
constexpr int OF_UPDATE_MAX_TY = 16;
constexpr size_t MM_HEADER_BYTES = 256;
constexpr int MM_MAX_BLOCKS = 1024;

struct Level {                           // one pyramid level, on the host
    int w, h, ksize;
    double scale, sigma;
};

struct LevelParams {                     // of_level_kernel
    int W, H, w, h, ksize;
    const uint8_t *src[2];
    float *dst[2];
    float taps[LVDGS_FARNEBACK_MAX_BLUR_TAPS];
};

struct PolyParams {                      // of_polyexp_kernel
    int w, h, n;
    const float *img[2];
    float *R[2];
    float g[2 * OF_MAX_POLY + 1], xg[2 * OF_MAX_POLY + 1], xxg[2 * OF_MAX_POLY + 1];
    float ig11, ig03, ig33, ig55;
};

struct FlowParams {                      // of_matrices_kernel, of_update_kernel
    int w, h, pw, ph;                    // the level's size; the coarser level's (0: none, the flow starts from zero)
    int winsize, ty, last;               // of_update_kernel: the window, the tile's rows, no next M
    float inv_pyr_scale, inv_area;
    const float *R0, *R1;                // (h, w, 5) each
    const float *prev_flow;              // (ph, pw, 2)
    float *flow;                         // (h, w, 2)
    const float *M_in;                   // 5 planes of h * w
    float *M_out;
};

__device__ __forceinline__ int reflect101(int i, int n) {   // any i; n >= 1
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}
__device__ __forceinline__ int clampi(int i, int lo, int hi) { return min(max(i, lo), hi); }

// the bilinear taps of output index i along an axis resized from n_in to n_out: i0, i1 clamped, the weight of i1
__device__ __forceinline__ void axis_taps(int i, int n_in, int n_out, int &i0, int &i1, float &f) {
    const double s = ((double)i + 0.5) * ((double)n_in / (double)n_out) - 0.5;
    const double fl = floor(s);
    f = (float)(s - fl);
    const int k = (int)fl;
    i0 = clampi(k, 0, n_in - 1);
    i1 = clampi(k + 1, 0, n_in - 1);
}
__device__ __forceinline__ float bilinear(float a, float b, float c, float d, float fx, float fy) {
    return (a * (1.0f - fx) + b * fx) * (1.0f - fy) + (c * (1.0f - fx) + d * fx) * fy;
}

struct MmHeader {                        // the motion mask's state begins with it; all zero: no stored frame
    int32_t width, height, stored;
};

// header: null, or where to note that `grey` is the stored frame from now on (LVDGS_MOTION_OBSERVE)
__global__ void __launch_bounds__(OF_THREADS) of_grey_kernel(const float *image, int64_t n, uint8_t *grey, MmHeader *header, int W, int H) {
    if (header && blockIdx.x == 0 && threadIdx.x == 0) {
        MmHeader h;
        h.width = W; h.height = H; h.stored = 1;
        *header = h;
    }
    for (int64_t i = (int64_t)blockIdx.x * OF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OF_THREADS) {
        int q[3];
        for (int c = 0; c < 3; c++) q[c] = (int)fminf(fmaxf(image[c * n + i] * 255.0f, 0.0f), 255.0f);
        grey[i] = (uint8_t)((4899 * q[0] + 9617 * q[1] + 1868 * q[2] + 8192) >> 14);
    }
}

// A tile of 64 x 4 pixels of a level image.  A pixel interpolates between two source rows and two source columns; the blur along the
// rows is formed for the tile's 128 source columns only and for the source rows the blur along the columns reaches, OF_LEVEL_CHUNK rows
// at a time (LDS rows are UNREFLECTED row numbers a .. a + 31, each holding the row it reflects to); the taps of a pixel's two rows that
// fall into the chunk are added, in ascending order as the chunks ascend.
__global__ void __launch_bounds__(OF_THREADS) of_level_kernel(LevelParams P) {
    __shared__ float hb[OF_LEVEL_CHUNK][2 * OF_TX];
    __shared__ int colx[2 * OF_TX];
    const uint8_t *src = P.src[blockIdx.z];
    const int tx = threadIdx.x % OF_TX, ty = threadIdx.x / OF_TX;
    const int ox0 = blockIdx.x * OF_TX, oy0 = blockIdx.y * OF_ROWS;
    const int r = P.ksize >> 1;
    const int ox = min(ox0 + tx, P.w - 1), oy = min(oy0 + ty, P.h - 1);   // (threads past the edge work the edge's pixel and store nothing)
    int x0, x1, y0, y1;
    float fx, fy;
    axis_taps(ox, P.W, P.w, x0, x1, fx);
    axis_taps(oy, P.H, P.h, y0, y1, fy);
    if (ty == 0) { colx[2 * tx] = x0; colx[2 * tx + 1] = x1; }
    int first0, first1, last0, last1;   // the source rows of the tile's first and last row of pixels
    float unused;
    axis_taps(min(oy0, P.h - 1), P.H, P.h, first0, first1, unused);
    axis_taps(min(oy0 + OF_ROWS - 1, P.h - 1), P.H, P.h, last0, last1, unused);
    const int row_lo = first0 - r, row_hi = last1 + r;   // unreflected, inclusive
    float acc00 = 0.0f, acc01 = 0.0f, acc10 = 0.0f, acc11 = 0.0f;   // (row y0 | y1) x (column x0 | x1)
    __syncthreads();
    for (int a = row_lo; a <= row_hi; a += OF_LEVEL_CHUNK) {   // (block-uniform)
        const int rows = min(OF_LEVEL_CHUNK, row_hi - a + 1);
        for (int e = threadIdx.x; e < rows * 2 * OF_TX; e += OF_THREADS) {
            const int i = e / (2 * OF_TX), c = e % (2 * OF_TX);
            const uint8_t *row = src + (int64_t)reflect101(a + i, P.H) * P.W;
            const int xc = colx[c];
            float s = 0.0f;
            for (int k = 0; k < P.ksize; k++) s = s + P.taps[k] * (float)row[reflect101(xc - r + k, P.W)];
            hb[i][c] = s;
        }
        __syncthreads();
        {   // taps k of row y: unreflected row y - r + k, inside the chunk for k in [a - (y - r), a + rows - (y - r))
            const int b0 = y0 - r - a, b1 = y1 - r - a;   // LDS row of tap 0
            for (int k = max(0, -b0); k < min(P.ksize, rows - b0); k++) {
                const float t = P.taps[k];
                acc00 = acc00 + t * hb[b0 + k][2 * tx];
                acc01 = acc01 + t * hb[b0 + k][2 * tx + 1];
            }
            for (int k = max(0, -b1); k < min(P.ksize, rows - b1); k++) {
                const float t = P.taps[k];
                acc10 = acc10 + t * hb[b1 + k][2 * tx];
                acc11 = acc11 + t * hb[b1 + k][2 * tx + 1];
            }
        }
        __syncthreads();
    }
    if (ox0 + tx < P.w && oy0 + ty < P.h) P.dst[blockIdx.z][(int64_t)oy * P.w + ox] = bilinear(acc00, acc01, acc10, acc11, fx, fy);
}

// A tile of 64 x 16 pixels: v0, v1, v2 -- the column correlations with g, xg, xxg -- of the tile's rows and 64 + 2n columns in LDS, then
// the six row sums per pixel.  Both passes replicate the edge.
__global__ void __launch_bounds__(OF_THREADS) of_polyexp_kernel(PolyParams P) {
    constexpr int LW = OF_TX + 2 * OF_MAX_POLY;
    __shared__ float v[3][OF_POLY_TY][LW];
    const float *img = P.img[blockIdx.z];
    float *R = P.R[blockIdx.z];
    const int n = P.n, lw = OF_TX + 2 * n;
    const int ox0 = blockIdx.x * OF_TX, oy0 = blockIdx.y * OF_POLY_TY;
    for (int e = threadIdx.x; e < OF_POLY_TY * lw; e += OF_THREADS) {
        const int i = e / lw, c = e % lw;
        const int x = clampi(ox0 - n + c, 0, P.w - 1), y = oy0 + i;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int k = -n; k <= n; k++) {
            const float p = img[(int64_t)clampi(y + k, 0, P.h - 1) * P.w + x];
            s0 = s0 + P.g[k + n] * p;
            s1 = s1 + P.xg[k + n] * p;
            s2 = s2 + P.xxg[k + n] * p;
        }
        v[0][i][c] = s0; v[1][i][c] = s1; v[2][i][c] = s2;
    }
    __syncthreads();
    const int tx = threadIdx.x % OF_TX, x = ox0 + tx;
    for (int i = threadIdx.x / OF_TX; i < OF_POLY_TY; i += OF_ROWS) {
        const int y = oy0 + i;
        if (x >= P.w || y >= P.h) continue;
        float b1 = 0.0f, b2 = 0.0f, b3 = 0.0f, b4 = 0.0f, b5 = 0.0f, b6 = 0.0f;
        for (int k = 0; k <= 2 * n; k++) {
            const float p0 = v[0][i][tx + k], p1 = v[1][i][tx + k], p2 = v[2][i][tx + k];
            const float g = P.g[k], xg = P.xg[k], xxg = P.xxg[k];
            b1 = b1 + g * p0; b2 = b2 + xg * p0; b4 = b4 + xxg * p0;
            b3 = b3 + g * p1; b5 = b5 + xg * p1;
            b6 = b6 + g * p2;
        }
        float *out = R + ((int64_t)y * P.w + x) * 5;
        out[0] = b3 * P.ig11;
        out[1] = b2 * P.ig11;
        out[2] = b1 * P.ig03 + b6 * P.ig33;
        out[3] = b1 * P.ig03 + b4 * P.ig33;
        out[4] = b5 * P.ig55;
    }
}

__device__ __forceinline__ float border_weight(int c, int n) {
    const float B[6] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f, 1.0f};
    return B[min(c, 5)] * B[min(n - 1 - c, 5)];
}

// M at pixel (x, y) of a w x h level from the flow (dx, dy) there
__device__ __forceinline__ void matrices_at(const FlowParams &P, int x, int y, float dx, float dy, float (&M)[5]) {
    const float *r0 = P.R0 + ((int64_t)y * P.w + x) * 5;
    float fx = (float)x + dx, fy = (float)y + dy;
    const float x1f = floorf(fx), y1f = floorf(fy);
    float r2, r3, r4, r5, r6;
    if (x1f >= 0.0f && x1f < (float)(P.w - 1) && y1f >= 0.0f && y1f < (float)(P.h - 1)) {
        const int x1 = (int)x1f, y1 = (int)y1f;
        fx = fx - x1f; fy = fy - y1f;
        const float a00 = (1.0f - fx) * (1.0f - fy), a01 = fx * (1.0f - fy), a10 = (1.0f - fx) * fy, a11 = fx * fy;
        const float *p00 = P.R1 + ((int64_t)y1 * P.w + x1) * 5, *p10 = p00 + (int64_t)P.w * 5;
        float r[5];
        for (int c = 0; c < 5; c++) r[c] = a00 * p00[c] + a01 * p00[5 + c] + a10 * p10[c] + a11 * p10[5 + c];
        r4 = (r0[2] + r[2]) * 0.5f;
        r5 = (r0[3] + r[3]) * 0.5f;
        r6 = (r0[4] + r[4]) * 0.25f;
        r2 = (r0[0] - r[0]) * 0.5f + (r4 * dy + r6 * dx);
        r3 = (r0[1] - r[1]) * 0.5f + (r6 * dy + r5 * dx);
    } else {
        r2 = 0.0f; r3 = 0.0f;
        r4 = r0[2]; r5 = r0[3]; r6 = r0[4] * 0.5f;
    }
    const float s = border_weight(x, P.w) * border_weight(y, P.h);
    r2 = r2 * s; r3 = r3 * s; r4 = r4 * s; r5 = r5 * s; r6 = r6 * s;
    M[0] = r4 * r4 + r6 * r6;
    M[1] = (r4 + r5) * r6;
    M[2] = r5 * r5 + r6 * r6;
    M[3] = r4 * r2 + r6 * r3;
    M[4] = r6 * r2 + r5 * r3;
}

__global__ void __launch_bounds__(OF_THREADS) of_matrices_kernel(FlowParams P) {
    const int x = blockIdx.x * OF_TX + threadIdx.x % OF_TX, y = blockIdx.y * OF_ROWS + threadIdx.x / OF_TX;
    if (x >= P.w || y >= P.h) return;
    float dx = 0.0f, dy = 0.0f;
    if (P.pw) {
        int x0, x1, y0, y1;
        float fx, fy;
        axis_taps(x, P.pw, P.w, x0, x1, fx);
        axis_taps(y, P.ph, P.h, y0, y1, fy);
        const float *a = P.prev_flow + ((int64_t)y0 * P.pw + x0) * 2, *b = P.prev_flow + ((int64_t)y0 * P.pw + x1) * 2;
        const float *c = P.prev_flow + ((int64_t)y1 * P.pw + x0) * 2, *d = P.prev_flow + ((int64_t)y1 * P.pw + x1) * 2;
        dx = bilinear(a[0], b[0], c[0], d[0], fx, fy) * P.inv_pyr_scale;
        dy = bilinear(a[1], b[1], c[1], d[1], fx, fy) * P.inv_pyr_scale;
    }
    const int64_t o = (int64_t)y * P.w + x, plane = (int64_t)P.w * P.h;
    P.flow[2 * o] = dx; P.flow[2 * o + 1] = dy;
    float M[5];
    matrices_at(P, x, y, dx, dy, M);
    for (int c = 0; c < 5; c++) P.M_out[c * plane + o] = M[c];
}

// A tile of 64 x P.ty pixels.  Channel by channel: the tile of M_in with its halo of winsize / 2 rows and columns into LDS (an LDS row or
// column is the unclamped number, holding what it clamps to), the row sums of its rows out of that, the column sums out of those into
// registers; then the solve and the next M into M_out.
__global__ void __launch_bounds__(OF_THREADS) of_update_kernel(FlowParams P) {
    constexpr int LW = OF_TX + OF_MAX_WIN - 1, PER_THREAD = OF_UPDATE_MAX_TY / OF_ROWS;
    __shared__ float raw[OF_UPDATE_LDS_ROWS][LW];
    __shared__ float hs[OF_UPDATE_LDS_ROWS][OF_TX];
    const int tx = threadIdx.x % OF_TX, ty = threadIdx.x / OF_TX, r = P.winsize >> 1;
    const int ox0 = blockIdx.x * OF_TX, oy0 = blockIdx.y * P.ty;
    const int x = ox0 + tx;
    const int64_t plane = (int64_t)P.w * P.h;
    const int rows = P.ty + 2 * r, lw = OF_TX + 2 * r;   // rows <= OF_UPDATE_LDS_ROWS (the launcher chooses ty so), lw <= LW
    float S[PER_THREAD][5];
    for (int c = 0; c < 5; c++) {
        const float *M = P.M_in + c * plane;
        for (int e = threadIdx.x; e < rows * lw; e += OF_THREADS) {
            const int i = e / lw, j = e % lw;
            raw[i][j] = M[(int64_t)clampi(oy0 - r + i, 0, P.h - 1) * P.w + clampi(ox0 - r + j, 0, P.w - 1)];
        }
        __syncthreads();
        for (int i = ty; i < rows; i += OF_ROWS) {
            float s = 0.0f;
            for (int k = 0; k <= 2 * r; k++) s = s + raw[i][tx + k];
            hs[i][tx] = s;
        }
        __syncthreads();   // (the next channel's tile is written after this barrier, its row sums after the next one: no reader is left behind)
#pragma unroll
        for (int m = 0; m < PER_THREAD; m++) {
            const int i = ty + m * OF_ROWS;
            float s = 0.0f;
            if (i < P.ty)
                for (int k = 0; k <= 2 * r; k++) s = s + hs[i + k][tx];
            S[m][c] = s * P.inv_area;
        }
    }
#pragma unroll
    for (int m = 0; m < PER_THREAD; m++) {
        const int y = oy0 + ty + m * OF_ROWS;
        if (ty + m * OF_ROWS >= P.ty || x >= P.w || y >= P.h) continue;
        const float g11 = S[m][0], g12 = S[m][1], g22 = S[m][2], h1 = S[m][3], h2 = S[m][4];
        const float idet = 1.0f / (g11 * g22 - g12 * g12 + 1e-3f);
        const float dx = (g11 * h2 - g12 * h1) * idet, dy = (g22 * h1 - g12 * h2) * idet;
        const int64_t o = (int64_t)y * P.w + x;
        P.flow[2 * o] = dx; P.flow[2 * o + 1] = dy;
        if (!P.last) {
            float M[5];
            matrices_at(P, x, y, dx, dy, M);
            for (int c = 0; c < 5; c++) P.M_out[c * plane + o] = M[c];
        }
    }
}

// ---- the motion mask around the flow ----
struct MmParams {
    int W, H, wpr, levels, dilate_k, advance;
    int64_t words;
    float thr;
    const float *flow;
    const uint8_t *cur;                  // the grey plane of this call's image
    uint8_t *mask;
    int32_t *info;
    MmHeader *header;
    uint8_t *stored;                     // the state's grey plane
    uint64_t *plane;                     // scratch: the thresholded flow, one bit per pixel
};

__device__ __forceinline__ bool has_stored_frame(const MmParams &P) {
    const MmHeader h = *P.header;
    return h.width == P.W && h.height == P.H && h.stored == 1;
}

__global__ void __launch_bounds__(OF_THREADS) of_moving_kernel(MmParams P) {
    const int lane = threadIdx.x % WAVE;
    const bool stored = has_stored_frame(P);
    uint32_t v[1] = {0};
    for (int64_t word = (int64_t)blockIdx.x * OF_ROWS + threadIdx.x / WAVE; word < P.words; word += (int64_t)gridDim.x * OF_ROWS) {   // (wave-uniform)
        const int y = (int)(word / P.wpr), wx = (int)(word - (int64_t)y * P.wpr);
        const int x = wx * 64 + lane;
        bool moving = false;
        if (x < P.W) {
            const int64_t o = (int64_t)y * P.W + x;
            const float fx = P.flow[2 * o], fy = P.flow[2 * o + 1];
            moving = stored && sqrtf(fx * fx + fy * fy) > P.thr;
        }
        const uint64_t w = __ballot(moving);
        if (lane == 0) {
            P.plane[word] = w;
            if (word == 0) {
                P.info[LVDGS_MOTION_INFO_HAS_PREV] = stored;
                P.info[LVDGS_MOTION_INFO_LEVELS] = P.levels;
            }
        }
        v[0] += (uint32_t)__popcll(w);
    }
    const int slot[1] = {LVDGS_MOTION_INFO_MOVING_PIXELS};
    add_counts<1>(P.info, slot, v, lane == 0);
}

__global__ void __launch_bounds__(OF_THREADS) of_dilate_kernel(MmParams P) {
    const int lane = threadIdx.x % WAVE;
    uint32_t v[1] = {0};
    for (int64_t word = (int64_t)blockIdx.x * OF_ROWS + threadIdx.x / WAVE; word < P.words; word += (int64_t)gridDim.x * OF_ROWS) {
        const int y = (int)(word / P.wpr), wx = (int)(word - (int64_t)y * P.wpr);
        const uint64_t d = dilate_word(P.plane, P.W, P.H, P.wpr, y, wx, P.dilate_k, lane);
        const int x = wx * 64 + lane;
        if (x < P.W) {
            const int64_t o = (int64_t)y * P.W + x;
            P.mask[o] = (uint8_t)((d >> lane) & 1ull);
            if (P.advance) P.stored[o] = P.cur[o];   // (every reader of the stored frame ran in a launch before)
        }
        v[0] += (uint32_t)__popcll(d);
        if (P.advance && word == 0 && lane == 0) {
            MmHeader h;
            h.width = P.W; h.height = P.H; h.stored = 1;
            *P.header = h;
        }
    }
    const int slot[1] = {LVDGS_MOTION_INFO_MASK_PIXELS};
    add_counts<1>(P.info, slot, v, lane == 0);
}

// ---- the host's side ----
bool size_ok(int width, int height) { return width >= 1 && height >= 1 && width <= OF_MAX_EDGE && height <= OF_MAX_EDGE; }

int build_pyramid(int W, int H, const lvdgs_farneback_params &p, Level *out) {   // coarsest first; returns the number of levels
    int k = 0;
    double s = 1.0;
    while (k < p.levels) {
        s *= p.pyr_scale;
        if ((double)W * s < OF_MIN_SIZE || (double)H * s < OF_MIN_SIZE) break;
        k++;
    }
    for (int level = k, i = 0; level >= 0; level--, i++) {
        double scale = 1.0;
        for (int j = 0; j < level; j++) scale *= p.pyr_scale;
        Level &lv = out[i];
        lv.scale = scale;
        lv.sigma = (1.0 / scale - 1.0) / 2.0;
        lv.ksize = max((int)nearbyint(5.0 * lv.sigma) | 1, 3);   // (the default rounding mode: half to even)
        lv.w = max((int)nearbyint((double)W * scale), 1);
        lv.h = max((int)nearbyint((double)H * scale), 1);
    }
    return k + 1;
}

// the scratch of a flow call: two level images, two expansions, two M, one flow buffer for the odd levels
struct FlowScratch {
    float *img[2], *R[2], *M[2], *flow_odd;
};
size_t flow_scratch_layout(int W, int H, FlowScratch *v, void *base) {
    Carver<FlowScratch> c(v, base);
    const size_t px = (size_t)W * H;
    for (int i = 0; i < 2; i++) c(c.v.img[i], px);
    for (int i = 0; i < 2; i++) c(c.v.R[i], 5 * px);
    for (int i = 0; i < 2; i++) c(c.v.M[i], 5 * px);
    c(c.v.flow_odd, 2 * px);
    return c.off;
}

// the motion mask's state: the header, then the grey plane of the stored frame
struct MmState { MmHeader *header; uint8_t *stored; };
size_t mm_state_layout(int W, int H, MmState *v, void *base) {
    Carver<MmState> c(v, base);
    c.bytes(c.v.header, MM_HEADER_BYTES); c(c.v.stored, (size_t)W * H);
    return c.off;
}

// ... and its scratch: the flow's scratch (run_flow lays it out), then a flow buffer (used when the caller wants none), the grey plane
// of the call's image, one bit plane
struct MmScratch { void *flow_scratch; float *flow; uint8_t *cur; uint64_t *plane; };
size_t mm_scratch_layout(int W, int H, MmScratch *v, void *base) {
    Carver<MmScratch> c(v, base);
    const size_t px = (size_t)W * H;
    c.bytes(c.v.flow_scratch, flow_scratch_layout(W, H, nullptr, nullptr));
    c(c.v.flow, 2 * px); c(c.v.cur, px); c.bytes(c.v.plane, plane_bytes(W, H));
    return c.off;
}

int check_flow_params(const char *who, int width, int height, const lvdgs_farneback_params &p, Level *levels, int *num_levels) {
    if (!size_ok(width, height)) { set_error("%s: image size %dx%d (1..%d each way)", who, width, height, OF_MAX_EDGE); return LVDGS_E_RANGE; }
    if (!(p.pyr_scale > 0.0 && p.pyr_scale < 1.0)) { set_error("%s: pyr_scale %g is not inside (0, 1)", who, p.pyr_scale); return LVDGS_E_RANGE; }
    if (p.levels < 0 || p.levels > OF_MAX_LEVELS) { set_error("%s: levels %d, outside 0..%d", who, p.levels, OF_MAX_LEVELS); return LVDGS_E_RANGE; }
    if (p.iterations < 1 || p.iterations > 10) { set_error("%s: iterations %d, outside 1..10", who, p.iterations); return LVDGS_E_RANGE; }
    if (!(p.poly_sigma > 0.0) || !isfinite(p.poly_sigma)) { set_error("%s: poly_sigma %g is not above 0", who, p.poly_sigma); return LVDGS_E_RANGE; }
    if (p.winsize < 3 || p.winsize > OF_MAX_WIN || !(p.winsize & 1)) {
        set_error("%s: winsize %d (odd sizes from 3 to %d)", who, p.winsize, OF_MAX_WIN); return LVDGS_E_INVALID;
    }
    if (p.poly_n != 5 && p.poly_n != 7) { set_error("%s: poly_n %d is neither 5 nor 7", who, p.poly_n); return LVDGS_E_INVALID; }
    *num_levels = build_pyramid(width, height, p, levels);
    for (int i = 0; i < *num_levels; i++)
        if (levels[i].ksize > LVDGS_FARNEBACK_MAX_BLUR_TAPS) {
            set_error("%s: the blur of pyramid level %d has %d taps, more than %d", who, *num_levels - 1 - i, levels[i].ksize, LVDGS_FARNEBACK_MAX_BLUR_TAPS);
            return LVDGS_E_RANGE;
        }
    return LVDGS_OK;
}

void poly_setup(const lvdgs_farneback_params &p, PolyParams &P) {
    const int n = p.poly_n;
    double g[2 * OF_MAX_POLY + 1], sum = 0.0;
    for (int x = -n; x <= n; x++) {
        g[x + n] = (double)(float)exp(-(double)(x * x) / (2.0 * p.poly_sigma * p.poly_sigma));
        sum += g[x + n];
    }
    double G00 = 0.0, G11 = 0.0, G33 = 0.0, G55 = 0.0;
    for (int x = -n; x <= n; x++) {
        g[x + n] /= sum;
        P.g[x + n] = (float)g[x + n];
        P.xg[x + n] = (float)((double)x * g[x + n]);
        P.xxg[x + n] = (float)((double)(x * x) * g[x + n]);
    }
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            const double gg = g[y + n] * g[x + n];
            G00 += gg;
            G11 += gg * x * x;
            G33 += gg * x * x * x * x;
            G55 += gg * x * x * y * y;
        }
    // inv(G): rows 1, 2, 5 stand alone; rows 0, 3, 4 are the block [[a, b, b], [b, c, d], [b, d, c]] with a = G00, b = G11, c = G33,
    // d = G55, whose determinant is (c - d) (a (c + d) - 2 b^2)
    const double a = G00, b = G11, c = G33, d = G55, det = (c - d) * (a * (c + d) - 2.0 * b * b);
    P.n = n;
    P.ig11 = (float)(1.0 / G11);
    P.ig55 = (float)(1.0 / G55);
    P.ig03 = (float)(-b * (c - d) / det);
    P.ig33 = (float)((a * c - b * b) / det);
}

// every launch of a flow call (the caller has checked everything); flow: (H, W, 2)
int run_flow(int W, int H, const lvdgs_farneback_params &p, const Level *levels, int num_levels, const uint8_t *prev, const uint8_t *next,
             float *flow, void *scratch, hipStream_t s) {
    FlowScratch fs;
    flow_scratch_layout(W, H, &fs, scratch);
    PolyParams poly{};
    poly_setup(p, poly);
    const int r = p.winsize >> 1, ty = min(OF_UPDATE_MAX_TY, OF_UPDATE_LDS_ROWS - 2 * r);
    int pw = 0, ph = 0;
    for (int i = 0; i < num_levels; i++) {
        const Level &lv = levels[i];
        const int k = num_levels - 1 - i;                     // level k uses the flow buffer of its parity: level 0 ends in `flow`
        float *cur_flow = (k & 1) ? fs.flow_odd : flow, *prev_flow = (k & 1) ? flow : fs.flow_odd;
        {
            LevelParams L{};
            L.W = W; L.H = H; L.w = lv.w; L.h = lv.h; L.ksize = lv.ksize;
            L.src[0] = prev; L.src[1] = next; L.dst[0] = fs.img[0]; L.dst[1] = fs.img[1];
            if (lv.sigma == 0.0) { L.taps[0] = 0.25f; L.taps[1] = 0.5f; L.taps[2] = 0.25f; }
            else {
                double t[LVDGS_FARNEBACK_MAX_BLUR_TAPS], sum = 0.0;
                for (int j = 0; j < lv.ksize; j++) {
                    const double x = (double)(j - lv.ksize / 2);
                    t[j] = exp(-x * x / (2.0 * lv.sigma * lv.sigma));
                    sum += t[j];
                }
                for (int j = 0; j < lv.ksize; j++) L.taps[j] = (float)(t[j] / sum);
            }
            if (int e = launch("of_level", 0, s, of_level_kernel, dim3(cdiv(lv.w, OF_TX), cdiv(lv.h, OF_ROWS), 2), dim3(OF_THREADS), 0, L)) return e;
        }
        {
            poly.w = lv.w; poly.h = lv.h;
            poly.img[0] = fs.img[0]; poly.img[1] = fs.img[1]; poly.R[0] = fs.R[0]; poly.R[1] = fs.R[1];
            if (int e = launch("of_polyexp", 0, s, of_polyexp_kernel, dim3(cdiv(lv.w, OF_TX), cdiv(lv.h, OF_POLY_TY), 2), dim3(OF_THREADS), 0, poly)) return e;
        }
        FlowParams F{};
        F.w = lv.w; F.h = lv.h; F.pw = pw; F.ph = ph;
        F.winsize = p.winsize; F.ty = ty;
        F.inv_pyr_scale = (float)(1.0 / p.pyr_scale);
        F.inv_area = (float)(1.0 / ((double)p.winsize * p.winsize));
        F.R0 = fs.R[0]; F.R1 = fs.R[1]; F.prev_flow = prev_flow; F.flow = cur_flow;
        F.M_out = fs.M[0];
        if (int e = launch("of_matrices", 0, s, of_matrices_kernel, dim3(cdiv(lv.w, OF_TX), cdiv(lv.h, OF_ROWS)), dim3(OF_THREADS), 0, F)) return e;
        for (int it = 0; it < p.iterations; it++) {
            F.M_in = fs.M[it & 1]; F.M_out = fs.M[(it + 1) & 1];
            F.last = it == p.iterations - 1;
            if (int e = launch("of_update", 0, s, of_update_kernel, dim3(cdiv(lv.w, OF_TX), cdiv(lv.h, ty)), dim3(OF_THREADS), 0, F)) return e;
        }
        pw = lv.w; ph = lv.h;
    }
    return LVDGS_OK;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_farneback_scratch_bytes(int32_t width, int32_t height) {
    if (!size_ok(width, height)) return 0;
    return flow_scratch_layout(width, height, nullptr, nullptr);
}

int lvdgs_farneback_flow(const lvdgs_farneback_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("farneback flow: args is NULL"); return LVDGS_E_INVALID; }
    Level levels[OF_MAX_LEVELS + 1];
    int num_levels = 0;
    if (int e = check_flow_params("farneback flow", a->width, a->height, a->params, levels, &num_levels)) return e;
    if (!a->prev || !a->next || !a->flow || !a->scratch) { set_error("farneback flow: prev / next / flow / scratch is NULL"); return LVDGS_E_INVALID; }
    if (a->scratch_bytes < lvdgs_farneback_scratch_bytes(a->width, a->height)) { set_error("farneback flow: scratch too small"); return LVDGS_E_INVALID; }
    return run_flow(a->width, a->height, a->params, levels, num_levels, a->prev, a->next, a->flow, a->scratch, s);
}

size_t lvdgs_motion_mask_state_bytes(int32_t width, int32_t height) {
    if (!size_ok(width, height)) return 0;
    return mm_state_layout(width, height, nullptr, nullptr);
}

size_t lvdgs_motion_mask_scratch_bytes(int32_t width, int32_t height) {
    if (!size_ok(width, height)) return 0;
    return mm_scratch_layout(width, height, nullptr, nullptr);
}

int lvdgs_motion_mask(const lvdgs_motion_mask_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("motion mask: args is NULL"); return LVDGS_E_INVALID; }
    Level levels[OF_MAX_LEVELS + 1];
    int num_levels = 0;
    if (int e = check_flow_params("motion mask", a->width, a->height, a->params, levels, &num_levels)) return e;
    const bool observe = a->mode == LVDGS_MOTION_OBSERVE;
    if (!observe && a->mode != LVDGS_MOTION_MASK && a->mode != (LVDGS_MOTION_MASK | LVDGS_MOTION_ADVANCE)) {
        set_error("motion mask: mode %d is neither LVDGS_MOTION_OBSERVE, LVDGS_MOTION_MASK nor LVDGS_MOTION_MASK | LVDGS_MOTION_ADVANCE", a->mode);
        return LVDGS_E_INVALID;
    }
    if (!odd_kernel(a->dilate_kernel)) {
        set_error("motion mask: dilate_kernel %d (odd sizes from 1 to %d)", a->dilate_kernel, BITPLANE_MAX_KERNEL); return LVDGS_E_INVALID;
    }
    if (!a->image || !a->state) { set_error("motion mask: image / state is NULL"); return LVDGS_E_INVALID; }
    if (!observe && (!a->mask || !a->info || !a->scratch)) { set_error("motion mask: mask / info / scratch is NULL in a LVDGS_MOTION_MASK call"); return LVDGS_E_INVALID; }
    if (a->state_bytes < lvdgs_motion_mask_state_bytes(a->width, a->height)) { set_error("motion mask: state too small"); return LVDGS_E_INVALID; }
    if (!observe && a->scratch_bytes < lvdgs_motion_mask_scratch_bytes(a->width, a->height)) { set_error("motion mask: scratch too small"); return LVDGS_E_INVALID; }
    const int W = a->width, H = a->height;
    const int64_t px = (int64_t)W * H;
    MmState st;
    mm_state_layout(W, H, &st, a->state);
    MmHeader *header = st.header; uint8_t *stored = st.stored;
    const int grey_blocks = (int)min((int64_t)cdiv(px, OF_THREADS), (int64_t)4 * MM_MAX_BLOCKS);
    if (observe) {
        if (int e = launch("of_grey", 0, s, of_grey_kernel, dim3(grey_blocks), dim3(OF_THREADS), 0, a->image, px, stored, header, W, H)) return e;
        return LVDGS_OK;
    }
    MmScratch w;
    mm_scratch_layout(W, H, &w, a->scratch);
    float *flow = a->flow ? a->flow : w.flow;
    uint8_t *cur = w.cur;
    MmParams P{};
    P.W = W; P.H = H; P.wpr = words_per_row(W); P.words = (int64_t)H * P.wpr;
    P.levels = num_levels; P.dilate_k = a->dilate_kernel; P.advance = (a->mode & LVDGS_MOTION_ADVANCE) != 0;
    P.thr = (float)a->motion_threshold;
    P.flow = flow; P.cur = cur; P.mask = a->mask; P.info = a->info; P.header = header; P.stored = stored;
    P.plane = w.plane;
    if (int e = check_hip(hipMemsetAsync(a->info, 0, LVDGS_MOTION_INFO_WORDS * sizeof(int32_t), s), "motion mask: clearing info")) return e;
    if (int e = launch("of_grey", 0, s, of_grey_kernel, dim3(grey_blocks), dim3(OF_THREADS), 0, a->image, px, cur, (MmHeader *)nullptr, W, H)) return e;
    if (int e = run_flow(W, H, a->params, levels, num_levels, stored, cur, flow, w.flow_scratch, s)) return e;
    const int wave_blocks = (int)min((int64_t)cdiv(P.words, OF_ROWS), (int64_t)MM_MAX_BLOCKS);
    if (int e = launch("of_moving", 0, s, of_moving_kernel, dim3(wave_blocks), dim3(OF_THREADS), 0, P)) return e;
    if (int e = launch("of_dilate", 0, s, of_dilate_kernel, dim3(wave_blocks), dim3(OF_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

}  // extern "C"
