// Wave-level device helpers for gfx950 (wave64).
#pragma once
#include <hip/hip_runtime.h>

namespace lvdgs {

// v_mov_b32 with a DPP modifier; lanes whose source is out of range (or masked) read 0.
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ float dpp_or_zero(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, BANK_MASK, false));
}

// Rotate a register by N lanes inside every 16-lane row (row_ror:N): lane i receives the value of lane (i - N) mod 16 of
// its row.  Every lane has a source, so the "old" operand is never used; passing the input itself spares the
// zero-initialisation the compiler emits for a constant.
template <int N>
__device__ __forceinline__ float row_rotate(float x) {
    const int v = __float_as_int(x);
    return __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0x120 + N, 0xf, 0xf, false));
}

// Sum over the 64 lanes of the wave; the total is valid in lane 63 only.
// row_shr:1,2,4,8 build inclusive prefixes inside each 16-lane row, row_bcast:15 / :31 chain the rows.
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    v += dpp_or_zero<0x111>(v);
    v += dpp_or_zero<0x112>(v);
    v += dpp_or_zero<0x114>(v);
    v += dpp_or_zero<0x118>(v);
    v += dpp_or_zero<0x142, 0xa>(v);
    v += dpp_or_zero<0x143, 0xc>(v);
    return v;
}

// The integer twin: inclusive prefix over the wave in every lane (lane 63: the total).  row_shr:1,2,4,8 inside the 16-lane rows,
// row_bcast:15 / :31 chain the rows (six DPP adds instead of the six ds_bpermute round trips of wave_inclusive_scan).
__device__ __forceinline__ uint32_t wave_inclusive_scan_dpp(uint32_t inc) {
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xf, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x142, 0xa, 0xf, false);
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x143, 0xc, 0xf, false);
    return inc;
}

// Sum over the 64 lanes, valid in every lane: xor butterfly with offsets 32, 16, ... 1 (for float and double that order is part
// of the result's bits).  T: int, uint32_t, unsigned long long, float, double.  No LDS, no barrier.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Maximum over the 64 lanes, valid in every lane (same butterfly): max for integers, fmaxf for float.
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// Minimum over the 64 lanes, valid in every lane: the maximum of the negated values (exact; -inf / +inf seeds keep their meaning).
__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// Inclusive prefix sum over the wave's lanes, in every lane (lane 63: the wave's total); lane shifts by 1, 2, ... 32.
// T: uint32_t, int, unsigned long long (the 64-bit form moves both halves; tested through scan_workgroup).  Reached by all 64 lanes.
// No LDS, no barrier.
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T x = __shfl_up(v, off, 64);
        if (lane >= off) v += x;
    }
    return v;
}

// Exclusive prefix sum of one value per thread over a workgroup of THREADS threads (up to 16 whole waves, all of which reach it);
// *total = the workgroup's sum, in every thread.  T: uint32_t, int, unsigned long long (sums wrap modulo the type).  s_scan: SCAN_WORDS
// words of T in LDS; two barriers (wave scans, then the wave totals by wave 0), both passed by every thread, so they also publish what
// the caller wrote to LDS before the call.
// Words 0-15 are written before the first barrier and read between the two, words 16-31 written between them and read behind the
// second: a second call on the same s_scan needs NO barrier in front (its first barrier orders its writes of 16-31 behind this
// call's reads), and the first call needs none either when nothing else has s_scan in use.  Every instantiation in use, and these
// three promises, are pinned by tests/test_gpu_primitives.py through the probe library (tests/probe/primitives_probe.hip).
constexpr int SCAN_WORDS = 32;
template <int THREADS, typename T>
__device__ __forceinline__ T scan_workgroup(T v, T *s_scan, T *total) {
    constexpr int WAVES = THREADS / 64;
    static_assert(WAVES >= 1 && WAVES <= 16 && THREADS % 64 == 0, "up to 16 whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive_scan(v);
    if (lane == 63) s_scan[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        T w = lane < WAVES ? s_scan[lane] : (T)0;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {   // (wave_inclusive_scan, stopped at the 16 lanes that hold a total)
            const T x = __shfl_up(w, off, 64);
            if (lane >= off) w += x;
        }
        if (lane < 16) s_scan[16 + lane] = w;   // inclusive over the waves
    }
    __syncthreads();
    *total = s_scan[16 + WAVES - 1];
    return inc - v + (wave ? s_scan[16 + wave - 1] : (T)0);
}

// Sum of one value per thread over a workgroup of WAVES waves, in every thread.  s: WAVES words of LDS.  Two barriers, the first in
// FRONT of the write of s: calls may follow each other on one s with nothing in between.
// float: wave_sum_to_lane63, then the wave totals in a FIXED order that is part of the results' bits -- one per specialisation.
__device__ __forceinline__ void block_sum_publish(float v, float *s) {
    v = wave_sum_to_lane63(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 63) s[wave] = v;
    __syncthreads();
}
template <int WAVES> __device__ __forceinline__ float block_sum(float v, float *s);
// four waves: left to right, ((s0 + s1) + s2) + s3
template <> __device__ __forceinline__ float block_sum<4>(float v, float *s) {
    block_sum_publish(v, s);
    return ((s[0] + s[1]) + s[2]) + s[3];
}
// eight waves: the pairwise tree ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))
template <> __device__ __forceinline__ float block_sum<8>(float v, float *s) {
    block_sum_publish(v, s);
    return (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])));
}
// int: wave_sum, then the wave totals from wave 0 up (any order gives the same integer)
template <int WAVES> __device__ __forceinline__ int block_sum(int v, int *s) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < WAVES; w++) t += s[w];
    return t;
}

// Pairwise folds for multi-value wave reductions (gfx950 v_permlane32_swap / v_permlane16_swap).
// fold32(a, b): lanes 0-31 hold a[l] + a[l+32], lanes 32-63 hold b[l-32] + b[l].
__device__ __forceinline__ float fold32(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// fold16(a, b): 16-lane rows 0 and 2 hold a's row pairs (0+1, 2+3) summed, rows 1 and 3 hold b's.
__device__ __forceinline__ float fold16(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// In-row (16 lanes) inclusive sums of three registers at once; lane 15 of every row gets the row
// total.  Interleaving the three keeps two instructions between a register's write and its DPP read.
__device__ __forceinline__ void row_sums3(float &x, float &y, float &z) {
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %1, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %2, %2, %2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %2, %2, %2 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %2, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %1, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_f32_dpp %2, %2, %2 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1"
        : "+v"(x), "+v"(y), "+v"(z));
}

// Clear / set one bit of a wave-uniform 64-bit mask in one scalar instruction (the compiler's shift + and-not, or
// subtract-with-carry + and for m &= m - 1, are two to three on a scalar unit four SIMDs share).
__device__ __forceinline__ uint64_t mask_clear_bit(uint64_t m, int bit) {
    asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(bit));
    return m;
}
__device__ __forceinline__ uint64_t mask_set_bit(uint64_t m, int bit) {
    asm("s_bitset1_b64 %0, %1" : "+s"(m) : "s"(bit));
    return m;
}

// v with lane `lane` (wave-uniform) replaced by the wave-uniform value x (v_writelane_b32; clang has no builtin for
// it, the intrinsic is reached by name; the compiler puts the lane select into M0 itself, as gfx9's one-SGPR-per-
// instruction rule demands).
extern "C" __device__ int lvdgs_writelane_i32(int x, int lane, int v) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ int write_lane(int v, int x, int lane) { return lvdgs_writelane_i32(x, lane, v); }

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// last step of a call that reports through a pinned host block: the host sees everything stored before the tag before it sees the tag
// (the payload goes through the same volatile pointer, by the one thread that seals).  The publish kernels of the calls tagged with a
// sequence number end in it; the three tagged with a status (pnp.hip, recip_nn.hip, matcher_io.hip) say why they do not.
__device__ __forceinline__ void seal_host_block(volatile int32_t *w, int index, int32_t tag) {
    __threadfence_system();
    w[index] = tag;
    __threadfence_system();
}

}  // namespace lvdgs
