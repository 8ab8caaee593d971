// A decoded frame's way onto the device (the reference's utils/dataset.py MonocularDataset.__getitem__ :321-344, which on the host
// runs cv2.remap over the frame, divides by 255 in float64, clamps, permutes and uploads float32):
//   lvdgs_undistort_map : the fixed-point undistortion map of a calibration, once per dataset (cv2.initUndistortRectifyMap's model)
//   lvdgs_ingest_frame  : H x W x 3 bytes -> the bilinear remap through that map (optional) -> 3 x H x W float32 = byte / 255, and the
//                         remapped bytes when asked for.  One launch each, no host wait, no copy.
//   lvdgs_ingest_depth  : a depth file's 8- or 16-bit samples (a plane of their own, or the first channel of the colour bytes already
//                         on the device) -> the H x W float32 plane = (float)((double)sample / divisor).  One launch; 1..3 B read and
//                         4 B written per pixel, the same flat groups of four.
// Semantics: include/lvdgs.h, DESIGN.md section 4k.  Parity of the remap with the real cv2.remap is UNPINNED (OpenCV is not installed
// where this was written): the rule is the one the header states, in integers.
//
// The ingest kernel is memory-bound (3 B read, 12 B written per pixel, 8 B of map with a remap).  A thread owns four consecutive
// pixels of the flat H*W raster: per plane one 16-byte store, coalesced along u; the rows of a plane follow each other without a gap,
// so the flat raster needs no head or tail per row -- only the image's last group can be short, and it takes the scalar path.  The
// source is read as three aligned dwords per thread where its rows are contiguous (src_row_bytes == 3 W) and its base is dword
// aligned, byte by byte otherwise (a row pitch, an odd base).  The remap's gather reads bytes: neighbouring destinations read
// neighbouring sources, the cache serves them.  Every load and store is inside the buffers the header names whatever the map holds.
#include <math.h>

#include "common.hpp"

namespace lvdgs {
namespace {

constexpr int ING_THREADS = 256;
constexpr int ING_PIXELS = 4;                  // pixels per thread
constexpr int32_t MAP_OUTSIDE = INT32_MIN;
constexpr float MAP_LIMIT = 1048576.0f;        // 2^20: coordinates of this magnitude or beyond are stored as MAP_OUTSIDE

struct MapParams {
    int W, H;
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
    int32_t *sx, *sy;
};

__device__ __forceinline__ int32_t fixed_coordinate(float m) {
    if (!(fabsf(m) < MAP_LIMIT)) return MAP_OUTSIDE;      // (NaN and infinities too)
    return (int32_t)rintf(m * 32.0f);                      // m * 32 is exact; rintf rounds ties to even
}

// one thread per destination pixel; all arithmetic float64, evaluated as written (no contraction: the Makefile's -ffp-contract=off)
__global__ void __launch_bounds__(ING_THREADS) undistort_map_kernel(MapParams P) {
    const int64_t p = (int64_t)blockIdx.x * ING_THREADS + threadIdx.x;
    if (p >= (int64_t)P.W * P.H) return;
    const int v = (int)(p / P.W), u = (int)(p - (int64_t)v * P.W);
    const double x = ((double)u - P.cx) / P.fx, y = ((double)v - P.cy) / P.fy;
    const double r2 = x * x + y * y;
    const double kr = 1 + ((P.k3 * r2 + P.k2) * r2 + P.k1) * r2;
    const double xd = x * kr + 2 * P.p1 * x * y + P.p2 * (r2 + 2 * x * x);
    const double yd = y * kr + P.p1 * (r2 + 2 * y * y) + 2 * P.p2 * x * y;
    const float mapx = (float)(P.fx * xd + P.cx), mapy = (float)(P.fy * yd + P.cy);
    P.sx[p] = fixed_coordinate(mapx);
    P.sy[p] = fixed_coordinate(mapy);
}

struct IngestParams {
    int W, H;
    int64_t P;                 // W * H
    const uint8_t *src;
    int64_t pitch;             // src_row_bytes
    const int32_t *sx, *sy;
    float *image;
    uint8_t *u8;
    int src_dwords;            // the source is one contiguous, dword-aligned byte array: three dword loads per full group
    int map_vec, image_vec, u8_dwords;   // 16-byte map loads / plane stores, dword stores of the byte copy, for full groups
};

__device__ __forceinline__ float unit(int b) { return (float)((double)b / 255.0); }

// the bilinear sample of one destination pixel: 5 fractional bits per axis, a constant-zero border per neighbour
__device__ __forceinline__ void remap_pixel(const IngestParams &P, int32_t sx, int32_t sy, int out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (sx == MAP_OUTSIDE || sy == MAP_OUTSIDE) return;
    const int ix = sx >> 5, ax = sx & 31, iy = sy >> 5, ay = sy & 31;     // arithmetic shifts: floor for negatives too
    const bool x0 = ix >= 0 && ix < P.W, x1 = ix >= -1 && ix < P.W - 1;
    const bool y0 = iy >= 0 && iy < P.H, y1 = iy >= -1 && iy < P.H - 1;
    int acc[3] = {0, 0, 0};
    auto add = [&](bool inside, int xx, int yy, int w) {
        if (!inside) return;
        const uint8_t *s = P.src + (int64_t)yy * P.pitch + 3 * (int64_t)xx;
        acc[0] += w * (int)s[0]; acc[1] += w * (int)s[1]; acc[2] += w * (int)s[2];
    };
    add(x0 && y0, ix, iy, (32 - ax) * (32 - ay));
    add(x1 && y0, ix + 1, iy, ax * (32 - ay));
    add(x0 && y1, ix, iy + 1, (32 - ax) * ay);
    add(x1 && y1, ix + 1, iy + 1, ax * ay);
    for (int c = 0; c < 3; c++) out[c] = (acc[c] + 512) >> 10;
}

// grid: one thread per ING_PIXELS consecutive pixels of the flat raster
template <bool REMAP>
__global__ void __launch_bounds__(ING_THREADS) ingest_kernel(IngestParams P) {
    const int64_t p0 = ((int64_t)blockIdx.x * ING_THREADS + threadIdx.x) * ING_PIXELS;
    if (p0 >= P.P) return;
    const int n = P.P - p0 < ING_PIXELS ? (int)(P.P - p0) : ING_PIXELS;
    const bool full = n == ING_PIXELS;
    int px[ING_PIXELS][3];
#pragma unroll
    for (int k = 0; k < ING_PIXELS; k++) px[k][0] = px[k][1] = px[k][2] = 0;

    if constexpr (REMAP) {
        int32_t sx[ING_PIXELS], sy[ING_PIXELS];
        if (full && P.map_vec) {
            const int4 a = *reinterpret_cast<const int4 *>(P.sx + p0), b = *reinterpret_cast<const int4 *>(P.sy + p0);
            sx[0] = a.x; sx[1] = a.y; sx[2] = a.z; sx[3] = a.w;
            sy[0] = b.x; sy[1] = b.y; sy[2] = b.z; sy[3] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < ING_PIXELS; k++) {
                sx[k] = k < n ? P.sx[p0 + k] : MAP_OUTSIDE;
                sy[k] = k < n ? P.sy[p0 + k] : MAP_OUTSIDE;
            }
        }
#pragma unroll
        for (int k = 0; k < ING_PIXELS; k++) remap_pixel(P, sx[k], sy[k], px[k]);
    } else {
        if (full && P.src_dwords) {
            const uint32_t *s = reinterpret_cast<const uint32_t *>(P.src + 3 * p0);   // 12 p0 / 4 bytes: dword aligned with the base
            const uint32_t w[3] = {s[0], s[1], s[2]};
#pragma unroll
            for (int i = 0; i < 3 * ING_PIXELS; i++) px[i / 3][i % 3] = (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
        } else {
            int64_t v = p0 / P.W;
            int u = (int)(p0 - v * P.W);
#pragma unroll
            for (int k = 0; k < ING_PIXELS; k++) {
                if (k < n) {
                    const uint8_t *s = P.src + v * P.pitch + 3 * (int64_t)u;
                    px[k][0] = s[0]; px[k][1] = s[1]; px[k][2] = s[2];
                    if (++u == P.W) { u = 0; v++; }
                }
            }
        }
    }

#pragma unroll
    for (int c = 0; c < 3; c++) {
        float *dst = P.image + (int64_t)c * P.P + p0;
        if (full && P.image_vec) {
            *reinterpret_cast<float4 *>(dst) = make_float4(unit(px[0][c]), unit(px[1][c]), unit(px[2][c]), unit(px[3][c]));
        } else {
#pragma unroll
            for (int k = 0; k < ING_PIXELS; k++)
                if (k < n) dst[k] = unit(px[k][c]);
        }
    }
    if (P.u8) {
        uint8_t *dst = P.u8 + 3 * p0;
        if (full && P.u8_dwords) {
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 3 * ING_PIXELS; i++) w[i >> 2] |= (uint32_t)px[i / 3][i % 3] << (8 * (i & 3));
            uint32_t *d = reinterpret_cast<uint32_t *>(dst);
            d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
        } else {
#pragma unroll
            for (int k = 0; k < ING_PIXELS; k++)
                if (k < n) { dst[3 * k] = (uint8_t)px[k][0]; dst[3 * k + 1] = (uint8_t)px[k][1]; dst[3 * k + 2] = (uint8_t)px[k][2]; }
        }
    }
}

struct DepthParams {
    int W;
    int64_t P;                 // W * H
    const uint8_t *src;
    int64_t pitch;             // src_row_bytes
    int stride;                // bytes between the samples of neighbouring pixels
    double divisor;
    float *out;
    int src_vec;               // the samples of a full group are one aligned load: a dword (bytes) or two (16-bit words)
    int src_dwords;            // stride 3, rows without a gap, dword-aligned base: three dword loads per full group
    int out_vec;               // 16-byte stores for full groups
};

__device__ __forceinline__ float depth_value(uint32_t sample, double divisor) { return (float)((double)sample / divisor); }

// grid: one thread per ING_PIXELS consecutive pixels of the flat raster; WORD: 16-bit samples, else bytes
template <bool WORD>
__global__ void __launch_bounds__(ING_THREADS) ingest_depth_kernel(DepthParams P) {
    const int64_t p0 = ((int64_t)blockIdx.x * ING_THREADS + threadIdx.x) * ING_PIXELS;
    if (p0 >= P.P) return;
    const int n = P.P - p0 < ING_PIXELS ? (int)(P.P - p0) : ING_PIXELS;
    const bool full = n == ING_PIXELS;
    uint32_t s[ING_PIXELS] = {0u, 0u, 0u, 0u};
    if (full && P.src_vec) {                       // rows without a gap, stride == the sample's size: the group is contiguous
        if constexpr (WORD) {
            const uint2 w = *reinterpret_cast<const uint2 *>(P.src + 2 * p0);
            s[0] = w.x & 0xffffu; s[1] = w.x >> 16; s[2] = w.y & 0xffffu; s[3] = w.y >> 16;
        } else {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(P.src + p0);
            s[0] = w & 255u; s[1] = (w >> 8) & 255u; s[2] = (w >> 16) & 255u; s[3] = w >> 24;
        }
    } else if (!WORD && full && P.src_dwords) {    // the first of every three bytes: bytes 0, 3, 6, 9 of twelve
        const uint32_t *q = reinterpret_cast<const uint32_t *>(P.src + 3 * p0);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        s[0] = w0 & 255u; s[1] = w0 >> 24; s[2] = (w1 >> 16) & 255u; s[3] = (w2 >> 8) & 255u;
    } else {
        int64_t v = p0 / P.W;
        int u = (int)(p0 - v * P.W);
#pragma unroll
        for (int k = 0; k < ING_PIXELS; k++) {
            if (k < n) {
                const uint8_t *q = P.src + v * P.pitch + (int64_t)u * P.stride;
                s[k] = WORD ? (uint32_t)*reinterpret_cast<const uint16_t *>(q) : (uint32_t)*q;
                if (++u == P.W) { u = 0; v++; }
            }
        }
    }
    float *dst = P.out + p0;
    if (full && P.out_vec) {
        *reinterpret_cast<float4 *>(dst) = make_float4(depth_value(s[0], P.divisor), depth_value(s[1], P.divisor),
                                                       depth_value(s[2], P.divisor), depth_value(s[3], P.divisor));
    } else {
#pragma unroll
        for (int k = 0; k < ING_PIXELS; k++)
            if (k < n) dst[k] = depth_value(s[k], P.divisor);
    }
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

int lvdgs_undistort_map(int32_t width, int32_t height, double fx, double fy, double cx, double cy, const double dist[5],
                        int32_t *sx, int32_t *sy, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (width <= 0 || height <= 0) { set_error("undistort_map: bad image size %dx%d", width, height); return LVDGS_E_INVALID; }
    if (!dist || !sx || !sy) { set_error("undistort_map: dist / sx / sy is NULL"); return LVDGS_E_INVALID; }
    if (!(fx != 0.0) || !(fy != 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) {
        set_error("undistort_map: fx / fy must be finite and not zero, cx / cy finite"); return LVDGS_E_INVALID;
    }
    const int64_t P = (int64_t)width * height;
    if (P > (int64_t)INT32_MAX * ING_THREADS) { set_error("undistort_map: %dx%d is too large a raster", width, height); return LVDGS_E_RANGE; }
    MapParams M{};
    M.W = width; M.H = height; M.fx = fx; M.fy = fy; M.cx = cx; M.cy = cy;
    M.k1 = dist[0]; M.k2 = dist[1]; M.p1 = dist[2]; M.p2 = dist[3]; M.k3 = dist[4];   // OpenCV's order; read here, on the host
    M.sx = sx; M.sy = sy;
    if (int e = launch("undistort_map", 0, s, undistort_map_kernel, dim3(cdiv(P, ING_THREADS)), dim3(ING_THREADS), 0, M)) return e;
    return LVDGS_OK;
}

int lvdgs_ingest_frame(const lvdgs_ingest_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("ingest_frame: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width <= 0 || a->height <= 0) { set_error("ingest_frame: bad image size %dx%d", a->width, a->height); return LVDGS_E_INVALID; }
    if (!a->src || !a->image) { set_error("ingest_frame: src / image is NULL"); return LVDGS_E_INVALID; }
    if (a->src_row_bytes < 3 * (int64_t)a->width) {
        set_error("ingest_frame: src_row_bytes %lld below 3 * width = %lld", (long long)a->src_row_bytes, 3LL * a->width); return LVDGS_E_INVALID;
    }
    if ((a->map_sx == nullptr) != (a->map_sy == nullptr)) { set_error("ingest_frame: exactly one of map_sx / map_sy is NULL"); return LVDGS_E_INVALID; }
    IngestParams P{};
    P.W = a->width; P.H = a->height; P.P = (int64_t)a->width * a->height;
    const int64_t groups = (P.P + ING_PIXELS - 1) / ING_PIXELS;
    if (groups > (int64_t)INT32_MAX * ING_THREADS) { set_error("ingest_frame: %dx%d is too large a raster", a->width, a->height); return LVDGS_E_RANGE; }
    P.src = a->src; P.pitch = a->src_row_bytes; P.sx = a->map_sx; P.sy = a->map_sy; P.image = a->image; P.u8 = a->image_u8;
    P.src_dwords = a->src_row_bytes == 3 * (int64_t)a->width && aligned(a->src, 4);
    P.map_vec = a->map_sx && aligned(a->map_sx, 16) && aligned(a->map_sy, 16);
    P.image_vec = aligned(a->image, 16) && P.P % 4 == 0;      // plane c starts at float c * P
    P.u8_dwords = a->image_u8 && aligned(a->image_u8, 4);
    if (int e = launch("ingest_frame", 0, s, a->map_sx ? ingest_kernel<true> : ingest_kernel<false>, dim3(cdiv(groups, ING_THREADS)), dim3(ING_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

int lvdgs_ingest_depth(const lvdgs_ingest_depth_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("ingest_depth: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width <= 0 || a->height <= 0) { set_error("ingest_depth: bad image size %dx%d", a->width, a->height); return LVDGS_E_INVALID; }
    if (!a->src || !a->out) { set_error("ingest_depth: src / out is NULL"); return LVDGS_E_INVALID; }
    if (!(a->divisor != 0.0) || !isfinite(a->divisor)) { set_error("ingest_depth: the divisor must be finite and not zero"); return LVDGS_E_INVALID; }
    if (a->sample_type != LVDGS_DEPTH_SAMPLE_BYTE && a->sample_type != LVDGS_DEPTH_SAMPLE_WORD) {
        set_error("ingest_depth: unknown sample_type %d", a->sample_type); return LVDGS_E_INVALID;
    }
    const bool word = a->sample_type == LVDGS_DEPTH_SAMPLE_WORD;
    const int size = word ? 2 : 1;
    if (a->pixel_stride < size) { set_error("ingest_depth: pixel_stride %d below the sample's %d bytes", a->pixel_stride, size); return LVDGS_E_INVALID; }
    if (a->src_row_bytes < (int64_t)a->width * a->pixel_stride) {
        set_error("ingest_depth: src_row_bytes %lld below width * pixel_stride = %lld", (long long)a->src_row_bytes, (long long)a->width * a->pixel_stride);
        return LVDGS_E_INVALID;
    }
    if (word && (!aligned(a->src, 2) || a->src_row_bytes % 2 != 0 || a->pixel_stride % 2 != 0)) {
        set_error("ingest_depth: 16-bit samples need an even src, src_row_bytes and pixel_stride"); return LVDGS_E_INVALID;
    }
    DepthParams P{};
    P.W = a->width; P.P = (int64_t)a->width * a->height;
    const int64_t groups = (P.P + ING_PIXELS - 1) / ING_PIXELS;
    if (groups > (int64_t)INT32_MAX * ING_THREADS) { set_error("ingest_depth: %dx%d is too large a raster", a->width, a->height); return LVDGS_E_RANGE; }
    P.src = static_cast<const uint8_t *>(a->src); P.pitch = a->src_row_bytes; P.stride = a->pixel_stride; P.divisor = a->divisor; P.out = a->out;
    const bool gapless = a->src_row_bytes == (int64_t)a->width * a->pixel_stride;
    P.src_vec = gapless && a->pixel_stride == size && aligned(a->src, 4 * size);
    P.src_dwords = !word && gapless && a->pixel_stride == 3 && aligned(a->src, 4);
    P.out_vec = aligned(a->out, 16);
    if (int e = launch("ingest_depth", 0, s, word ? ingest_depth_kernel<true> : ingest_depth_kernel<false>, dim3(cdiv(groups, ING_THREADS)), dim3(ING_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

}  // extern "C"
