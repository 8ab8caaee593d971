// Does the two-step quadrant test (common.hpp: quad_prepare + reaches_rect_prepared) return THE SAME BOOLEAN as
// reaches_rect()?  The blend kernels' gradient bits depend on which (entry, quadrant) combinations survive, so one
// differing case is one too many.  One kernel evaluates the three forms on every case and counts:
//   part 1: reaches_rect_prepared<false> -- the hoisted per-Gaussian values, all four edges;
//   part 2: reaches_rect_prepared<true>  -- ... and only the edges that face the mean (what the kernels run).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize tools/quadrant_reach_check.hip -o tools/quadrant_reach_check
//   timeout 120 tools/quadrant_reach_check [seed]
//
// (the library's own flags: the expressions must compile as they do in blend.hip).  Exit status 0: both counts are 0;
// 2: part 1 is 0, part 2 is not; 1: part 1 differs, or an error.
//
// Cases: CONICS seeded random conics x the lattice of half-pixel mean offsets from 40 px left / above the 8x8 rectangle to
// 40 px right / below it (175 x 175: inside it, inside one span only, on and just beyond every corner) x 8 opacities
// (0, 1/255 -+ an ulp, 1/255, 0.004, 0.05, 0.5, 0.99).
//  * conic = inverse of R(theta) diag(l1, l2) R(theta)^T, theta uniform over the circle and, for every eighth conic, an
//    exact multiple of 45 degrees; l1 log-uniform in [0.1, 1e4]; l2 = max(l1 * ratio, floor) with ratio log-uniform in
//    [1e-5, 1]; floor = 0.1 (the eigenvalue floor) for even conics, 0.3 (the low-pass) for odd ones;
//  * one conic in 16 is not an ellipse: a <= 0, c <= 0, a c <= b b, or all zero;
//  * the rectangle's corner is a random multiple of 8 inside a 1920 x 1080 image (the rounding of mean - pixel depends on
//    the magnitudes), and every other conic's lattice is shifted by a random sub-pixel offset.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../lvd_gs-slam_amd/csrc/common.hpp"

using namespace lvdgs;

constexpr int CONICS = 8192, LATTICE = 175, OPACITIES = 8;   // 8192 * 175^2 * 8 = 2.0e9 cases (>= 2^24)
enum { N_CASES, N_TRUE, D1, D2_LOST, D2_GAINED, N_NOT_ELLIPSE, N_INSIDE, N_COUNTERS };

__device__ uint32_t hash32(uint32_t x) {   // lowbias32
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ float unit(uint32_t seed, uint32_t k, uint32_t stream) {   // [0, 1)
    return (float)(hash32(seed ^ hash32(k * 8u + stream)) >> 8) * (1.f / 16777216.f);
}

__global__ void __launch_bounds__(256) check_kernel(uint32_t seed, unsigned long long *counters) {
    const uint32_t k = blockIdx.x;
    // ---- the conic of this workgroup ----
    float a, b, c;
    {
        const float theta = (k & 7u) == 0u ? 0.78539816f * (float)(hash32(seed + k) & 7u) : 6.2831853f * unit(seed, k, 0);
        const float l1 = 0.1f * __expf(11.5129f * unit(seed, k, 1));                      // 0.1 .. 1e4
        const float l2 = fmaxf(l1 * __expf(-11.5129f * unit(seed, k, 2)), (k & 1u) ? LOWPASS : LAMBDA_FLOOR);
        const float cs = cosf(theta), sn = sinf(theta);
        const float ca = cs * cs * l1 + sn * sn * l2, cb = cs * sn * (l1 - l2), cc = sn * sn * l1 + cs * cs * l2;
        const float det_inv = 1.f / (ca * cc - cb * cb);
        a = cc * det_inv; b = -cb * det_inv; c = ca * det_inv;
        if ((k & 15u) == 5u) {
            switch ((k >> 4) & 3u) {
                case 0: a = -a; break;
                case 1: c = 0.f; break;
                case 2: b = (b < 0.f ? -1.f : 1.f) * 1.5f * sqrtf(a * c); break;
                default: a = b = c = 0.f; break;
            }
        }
    }
    const float x0 = 8.f * (float)(hash32(seed ^ (k * 2u + 1u)) % 240u), y0 = 8.f * (float)(hash32(seed ^ (k * 2u + 2u)) % 135u);
    const float x1 = x0 + 7.f, y1 = y0 + 7.f;
    const float jx = (k & 2u) ? 0.5f * unit(seed, k, 3) : 0.f, jy = (k & 2u) ? 0.5f * unit(seed, k, 4) : 0.f;
    const float ops[OPACITIES] = {0.f, __uint_as_float(__float_as_uint(ALPHA_MIN) - 1u), ALPHA_MIN, __uint_as_float(__float_as_uint(ALPHA_MIN) + 1u),
                                  0.004f, 0.05f, 0.5f, 0.99f};
    unsigned long long n[N_COUNTERS] = {};
    for (int m = threadIdx.x; m < LATTICE * LATTICE; m += 256) {
        const float mx = x0 - 40.f + 0.5f * (float)(m % LATTICE) + jx, my = y0 - 40.f + 0.5f * (float)(m / LATTICE) + jy;
        const bool in = mx >= x0 && mx <= x1 && my >= y0 && my <= y1;
#pragma unroll
        for (int o = 0; o < OPACITIES; o++) {
            const float op = ops[o];
            const bool ref = reaches_rect(mx, my, a, b, c, op, x0, y0, x1, y1);
            const QuadBound q = quad_prepare(a, b, c, op);
            const bool p1 = reaches_rect_prepared<false>(mx, my, a, b, c, q.inv_a, q.inv_c, q.bound, x0, y0, x1, y1);
            const bool p2 = reaches_rect_prepared<true>(mx, my, a, b, c, q.inv_a, q.inv_c, q.bound, x0, y0, x1, y1);
            n[N_CASES]++; n[N_TRUE] += ref; n[D1] += p1 != ref; n[D2_LOST] += ref && !p2; n[D2_GAINED] += !ref && p2;
            n[N_NOT_ELLIPSE] += !(a > 0.f && c > 0.f && a * c - b * b > 0.f); n[N_INSIDE] += in;
        }
    }
    for (int i = 0; i < N_COUNTERS; i++) atomicAdd(&counters[i], n[i]);
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 0) : 20240607u;
    unsigned long long *dev = nullptr, n[N_COUNTERS];
    CHECK(hipMalloc(&dev, sizeof(n)));
    CHECK(hipMemset(dev, 0, sizeof(n)));
    hipLaunchKernelGGL(check_kernel, dim3(CONICS), dim3(256), 0, 0, seed, dev);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(n, dev, sizeof(n), hipMemcpyDeviceToHost));
    CHECK(hipFree(dev));
    printf("{\"seed\": %u, \"conics\": %d, \"cases\": %llu, \"reaches_rect_true\": %llu, \"not_an_ellipse\": %llu, \"mean_inside\": %llu, "
           "\"part1_differs\": %llu, \"part2_differs\": %llu, \"part2_lost\": %llu, \"part2_gained\": %llu}\n",
           seed, CONICS, n[N_CASES], n[N_TRUE], n[N_NOT_ELLIPSE], n[N_INSIDE], n[D1], n[D2_LOST] + n[D2_GAINED], n[D2_LOST], n[D2_GAINED]);
    if (n[N_CASES] < (1ull << 24) || n[D1]) return 1;
    return (n[D2_LOST] + n[D2_GAINED]) ? 2 : 0;
}
