// Masks as one bit per pixel (dynamic_mask.hip, optical_flow.hip): a row is ceil(width / 64) 64-bit words, bit b of word w is column
// 64 w + b, the bits past the last column are zero.  A word is one __ballot of a wave; dilation is shifts across the neighbouring
// words and an OR over the rows; counts are __popcll.
#pragma once
#include "common.hpp"

namespace lvdgs {

constexpr int BITPLANE_MAX_KERNEL = 15;  // dilation windows: odd, up to this (one lane per row of the window, 16 lanes to OR over)

inline int words_per_row(int width) { return (width + 63) / 64; }
inline size_t plane_bytes(int width, int height) { return (size_t)height * words_per_row(width) * sizeof(uint64_t); }
inline bool odd_kernel(int k) { return k >= 1 && k <= BITPLANE_MAX_KERNEL && (k & 1); }

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }   // n in 0..64
__device__ __forceinline__ uint64_t row_valid_bits(int W, int wx) { return low_bits(min(64, W - wx * 64)); }

__device__ __forceinline__ uint64_t wave_or(uint64_t v, int lanes) {   // OR over the first `lanes` (a power of two) lanes, in all of them
    for (int off = lanes >> 1; off > 0; off >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, off);
    return v;
}

// Block-wide sums into info: every wave's lane 0 adds what the wave gathered over its words into LDS, then one atomic per counter and
// block.  Integer sums: the order of arrival does not show.  Called by every thread of the block.
template <int N>
__device__ __forceinline__ void add_counts(int32_t *info, const int (&slot)[N], const uint32_t (&v)[N], bool lane0) {
    __shared__ uint32_t acc[N];
    if ((int)threadIdx.x < N) acc[threadIdx.x] = 0;
    __syncthreads();
    if (lane0)
        for (int j = 0; j < N; j++)
            if (v[j]) atomicAdd(&acc[j], v[j]);
    __syncthreads();
    if ((int)threadIdx.x < N && acc[threadIdx.x]) atomicAdd(&info[slot[threadIdx.x]], (int32_t)acc[threadIdx.x]);
}

// Word (y, wx) of `plane` (H rows of wpr words, W columns) dilated by a k x k window of ones, the border contributing nothing.
// Wave-cooperative: lane j < k takes row y - k / 2 + j -- its word widened by shifts across its two neighbours --, the rows are OR-ed
// over 16 lanes.  All lanes return the word.
__device__ __forceinline__ uint64_t dilate_word(const uint64_t *plane, int W, int H, int wpr, int y, int wx, int k, int lane) {
    const int r = k >> 1;
    uint64_t h = 0;
    const int yy = y - r + lane;
    if (lane < k && yy >= 0 && yy < H) {
        const uint64_t *row = plane + (int64_t)yy * wpr;
        const uint64_t cur = row[wx], prev = wx > 0 ? row[wx - 1] : 0ull, next = wx + 1 < wpr ? row[wx + 1] : 0ull;
        h = cur;
        for (int s = 1; s <= r; s++) h |= (cur << s) | (prev >> (64 - s)) | (cur >> s) | (next << (64 - s));
    }
    h = wave_or(h, 16);
    return (uint64_t)__shfl((unsigned long long)h, 0) & row_valid_bits(W, wx);
}

}  // namespace lvdgs
