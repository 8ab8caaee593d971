// Per-Gaussian kernels of the backward: the sums of every Gaussian's per-tile gradient records, the chain from them to the
// parameter and pose gradients, the reduction of the pose partials.  (The forward: preprocess.hip; the arithmetic both share:
// projection.hpp.)  One lane per Gaussian, wave64.  HBM-streaming: 56 + 40*(tiles touched) B read, the 14-float parameter gradient
// written per Gaussian.  Compiled with -ffp-contract=off, as the forward whose expressions it re-evaluates.
#include "common.hpp"
#include "device_utils.hpp"
#include "projection.hpp"

namespace lvdgs {

namespace {

struct BwdParams {
    Cam cam;
    int N, act;
    const float *means3D, *opacities, *scales, *rotations, *cov3D_precomp, *shs, *colors_precomp;
    const int32_t *radii;
    const float *rec;
    const uint32_t *tiles_touched, *slot_base;
    const float *pair_grads;
    const uint8_t *pair_valid;   // 1 where blend_bwd wrote the pair's record (pairs behind their tile's last contributor have none)
    float *dmeans3D, *dmeans2D, *dopac, *dscales, *drot, *dcov3D, *dshs, *dcolors;
    float *tau_part;
    int accumulate;   // LVDGS_FLAG_ACCUMULATE_PARAM_GRADS: the parameter gradients are added to what their buffers hold
    // lvdgs_forward_backward_fused_loss enqueues this pass before the host knows the frame's pair count: when the count (left on the
    // device by the tile scan) exceeds the capacity the buffers were sized for, the pass does NOTHING -- its slots would lie beyond
    // the record buffer -- and the caller runs the backward again behind a forward with room.  Null: no such check.  pair_total_super
    // (two-level grouping): the super lists' count, the same verdict (the tile lists read off them were cut short beyond the capacity).
    const uint32_t *pair_total, *pair_total_super;
    uint32_t pair_capacity;
};

#ifndef LVDGS_WAVE_CHUNK
#define LVDGS_WAVE_CHUNK 192
#endif
constexpr int WAVE_CHUNK = LVDGS_WAVE_CHUNK;  // pair records a wave stages per round (a multiple of 4): 7.5 KB of LDS per wave at 192, five workgroups per CU
constexpr int BIG_RUN = 64;      // a Gaussian with more pairs than this is summed by its whole wave
#ifndef LVDGS_PBWD_BIG_UNROLL
#define LVDGS_PBWD_BIG_UNROLL 2
#endif
constexpr int BIG_UNROLL = LVDGS_PBWD_BIG_UNROLL;   // ... LVDGS_PBWD_BIG_UNROLL records per lane and trip
#ifndef LVDGS_PBWD_TAKE
#define LVDGS_PBWD_TAKE 2   // records a lane of the compacted sweep requests from LDS before it adds the first (sum_region_compacted, step 3)
#endif
#ifndef LVDGS_PBWD_SEG
#define LVDGS_PBWD_SEG 512   // slots of a large-footprint wave's region swept per round (sum_region_compacted): 512 or 1024
#endif
// a wave's LDS staging area: WAVE_CHUNK records of the streaming path, or the compacted sweep's pass of records + its lists
template <int PF>
constexpr int STAGE_BYTES = (WAVE_CHUNK * PF * 4 > 128 * PF * 4 + LVDGS_PBWD_SEG * 2 + 320 ? WAVE_CHUNK * PF * 4 : (128 * PF * 4 + LVDGS_PBWD_SEG * 2 + 320 + 15) / 16 * 16);

#ifndef LVDGS_PBWD_WGS
#define LVDGS_PBWD_WGS 5
#endif
#ifndef LVDGS_PBWD_ABLATE
#define LVDGS_PBWD_ABLATE 0   // diagnostic builds: 1 = no pair sums, 2 = no per-Gaussian chain
#endif
// The values are in their registers -- their loads waited for -- at this point of the program.
__device__ __forceinline__ void wait_for_vector_memory() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void loads_complete_here(int32_t &radius, uint32_t &slot, uint32_t &tiles, float (&pos)[3], float &opac, float (&sc)[3],
                                                    float (&q)[4], float (&c6)[6]) {
    asm volatile("" : "+v"(radius), "+v"(slot), "+v"(tiles), "+v"(pos[0]), "+v"(pos[1]), "+v"(pos[2]), "+v"(opac));
    asm volatile("" : "+v"(sc[0]), "+v"(sc[1]), "+v"(sc[2]), "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]));
    asm volatile("" : "+v"(c6[0]), "+v"(c6[1]), "+v"(c6[2]), "+v"(c6[3]), "+v"(c6[4]), "+v"(c6[5]));
}

#ifdef LVDGS_DIAG_PBWD
// diagnostic build (tools/pbwd_diag.py): clocks of the compacted sweep per wave (registers; one row of eight values per wave and launch,
// no atomics -- thousands of waves adding to the same eight words cost more than the kernel).
// [0] 1, [1] whole sweep, [2] flags -> list (wait, masks, scan, list, barrier), [3] gather (requests -> LDS, barrier), [4] sums,
// [5] segments, [6] passes, [7] records
constexpr int PBWD_DIAG_WAVES = 8192;
constexpr int PBWD_DIAG_VALUES = 12;   // [8] trips of the lanes' own loop (the longest lane's), [9] Gaussians summed by the whole wave, [10] clocks of those
__device__ unsigned long long g_pbwd_diag[PBWD_DIAG_WAVES * PBWD_DIAG_VALUES];
#define PBWD_CLK(x) const unsigned long long x = __builtin_readcyclecounter()
#define PBWD_ADD(k, v) (diag[k] += (unsigned long long)(v))
#else
#define PBWD_CLK(x)
#define PBWD_ADD(k, v)
#endif
typedef float v2f __attribute__((ext_vector_type(2)));
template <bool POSE_ONLY>
__device__ __forceinline__ void unpack_sums(const v2f (&P)[POSE_ONLY ? PAIR_FLOATS_POSE / 2 : PAIR_FLOATS / 2], float (&A)[10]) {
    A[0] = P[0].x; A[1] = P[0].y; A[2] = P[1].x; A[3] = P[1].y; A[4] = P[2].x;
    if constexpr (POSE_ONLY) { A[5] = 0.f; A[6] = 0.f; A[7] = 0.f; A[8] = 0.f; A[9] = P[2].y; }
    else { A[5] = P[2].y; A[6] = P[3].x; A[7] = P[3].y; A[8] = P[4].x; A[9] = P[4].y; }
}
#ifndef LVDGS_PBWD_INLINE_BIG
#define LVDGS_PBWD_INLINE_BIG 1   // A/B builds: 0 = a function call (same box, config 3 / opaque surfaces: 50.5 / 96 us against 44.5 / 74.3 inlined: the spills around the call cost more than the separate register allocation returns)
#endif
#if LVDGS_PBWD_INLINE_BIG
#define LVDGS_BIG_PATH_ATTR __forceinline__
#else
#define LVDGS_BIG_PATH_ATTR __attribute__((noinline))
#endif

// ---- the pair sums of a wave that holds large-footprint Gaussians: the compacted sweep ----
// (A function of its own so that it can be built as a call, LVDGS_PBWD_INLINE_BIG = 0: measured, slower.  Its three steps are blocks
// of ONE function: as functions of their own -- a struct of the staging area's layout with a method per step -- they moved the
// register allocation of the kernels with helper waves, profiles/preprocess_bwd_split/README.md.)
// s_mem: the wave's LDS staging area; [first, last): the lane's run of slots.
// A2: the ten sums as packed pairs, in the record's own layout ([0,1] [2,3] [4,5] [6,7] [8,9]; pose-only [0,1] [2,3] [4,9]): a record is
// added with PF / 2 v_pk_add_f32 -- the same IEEE additions, two per instruction.  The records of [w_first, w_hi) are added to what A2 holds.
template <bool POSE_ONLY>
__device__ LVDGS_BIG_PATH_ATTR void sum_region_compacted(const float *__restrict__ pair_grads, const uint8_t *__restrict__ pair_valid, char *s_mem,
                                                              uint32_t first, uint32_t last, uint32_t w_first, uint32_t w_hi,
                                                              v2f (&A2)[POSE_ONLY ? PAIR_FLOATS_POSE / 2 : PAIR_FLOATS / 2]) {
    constexpr int PF = POSE_ONLY ? PAIR_FLOATS_POSE : PAIR_FLOATS;
    const int lane = threadIdx.x & 63;
    // A wave that holds large-footprint Gaussians (hundreds of pairs each: the stuff opaque surfaces are made of).  Of their
    // records only those in front of their tiles' last contributors exist -- a tenth on opaque surfaces -- and a lane that
    // walks its own run (flag, record, flag, record ...: two dependent round trips per slot) while 63 wait was 1.5 ms of this
    // kernel at 100 k such Gaussians; round 3's "the whole wave sums one large Gaussian after the other" still was a chain of
    // two round trips per Gaussian and 64 slots (76 us of 88 on that workload).  Now the wave sweeps its whole region -- the
    // runs of its 64 Gaussians follow each other in memory -- 512 slots at a time:
    //   1. the segment's FLAGS, eight per lane in one load (the next segment's are requested before this one is worked on),
    //      compacted into a list of the slots that hold a record (wave scan of the per-lane counts);
    //   2. just those records, gathered densely into the wave's LDS, BIG_UNROLL per lane in flight;
    //   3. every lane adds up ITS Gaussian's records of the pass from LDS, in slot order (the order of the streaming path);
    //      a Gaussian with more than 64 records in the pass is summed by the whole wave (lane l: records l, l + 64, ...) and
    //      folded in a fixed order.
    constexpr uint32_t SEG = LVDGS_PBWD_SEG;
    constexpr uint32_t FL = SEG / 64u;   // flags (slots) per lane
    static_assert(FL == 8u || FL == 16u, "one 8- or 16-byte load of flags per lane");
    constexpr int AUX_BYTES = (int)SEG * 2 + 64 * 2 + 64 * 2 + PF * 4;                      // list, per-lane prefix, per-lane flag bits, a record of zeros
    constexpr uint32_t CAP = 128u;   // records per pass: the same number in both forms of the kernel, so that both add in the same order
    static_assert(CAP * PF * 4 + AUX_BYTES <= STAGE_BYTES<PF>, "fits the wave's staging area");
    float2 *const s_rec = reinterpret_cast<float2 *>(s_mem);
    uint16_t *const s_list = reinterpret_cast<uint16_t *>(s_mem + CAP * PF * 4);   // offsets (in the segment) of the slots with a record
    uint16_t *const s_before = s_list + SEG;                                                  // records of the segment in front of lane l's eight slots
    uint16_t *const s_bits = s_before + 64;                                                   // lane l's FL flags
    // a record of zeros behind them (8-byte aligned): what the lanes of step 3 read where their run has ended -- adding +0 to a sum
    // that started at +0 leaves its bits as they are -- so that TAKE records can be requested from LDS before the first is added
    float2 *const s_zero = reinterpret_cast<float2 *>(s_bits + 64);
    constexpr uint32_t ZERO_AT = (uint32_t)((CAP * PF * 4 + SEG * 2 + 64 * 2 + 64 * 2) / 8);   // s_zero as an index of s_rec's float2
    static_assert((CAP * PF * 4 + SEG * 2 + 64 * 2 + 64 * 2) % 8 == 0, "aligned");
    if (lane < PF / 2) s_zero[lane] = make_float2(0.f, 0.f);
    const float2 *pg = reinterpret_cast<const float2 *>(pair_grads);
    const uint32_t w_lo = w_first & ~(FL - 1u);   // w_first rounded down to the flags' 8- / 16-byte loads
    struct Flags { uint32_t w[FL / 4]; };
    auto flags_of = [&](uint32_t seg) {   // (pair_valid is padded by 16 bytes)
        const uint32_t s0 = seg + FL * (uint32_t)lane;
        Flags f{};
        if (s0 < w_hi) {
            if constexpr (FL == 8u) { const uint2 v = *reinterpret_cast<const uint2 *>(pair_valid + s0); f.w[0] = v.x; f.w[1] = v.y; }
            else { const uint4 v = *reinterpret_cast<const uint4 *>(pair_valid + s0); f.w[0] = v.x; f.w[1] = v.y; f.w[2] = v.z; f.w[3] = v.w; }
        }
        return f;
    };
    Flags fl_next = w_lo < w_hi ? flags_of(w_lo) : Flags{};
#ifdef LVDGS_DIAG_PBWD
    unsigned long long diag[PBWD_DIAG_VALUES] = {};
#endif
    PBWD_CLK(t_begin);
    PBWD_ADD(0, 1);
    for (uint32_t seg = w_lo; seg < w_hi; seg += SEG) {
        PBWD_CLK(t_seg);
        PBWD_ADD(5, 1);
        const Flags fl = fl_next;
        if (seg + SEG < w_hi) fl_next = flags_of(seg + SEG);
        // ---- 1. which of the segment's slots hold a record ----
        uint32_t mine = 0;   // bit b: slot seg + FL lane + b
#pragma unroll
        for (int w = 0; w < (int)(FL / 4); w++)
#pragma unroll
            for (int b = 0; b < 4; b++)
                if ((fl.w[w] >> (8 * b)) & 0xffu) mine |= 1u << (4 * w + b);
        {   // slots outside the wave's region are other waves' (or, behind the frame's last pair, nobody's: their flags are stale)
            constexpr uint32_t ALL = (1u << FL) - 1u;
            const uint32_t s0 = seg + FL * (uint32_t)lane;
            const uint32_t keep_hi = s0 >= w_hi ? 0u : (w_hi - s0 >= FL ? ALL : (1u << (w_hi - s0)) - 1u);
            const uint32_t keep_lo = s0 >= w_first ? ALL : (w_first - s0 >= FL ? 0u : (ALL << (w_first - s0)) & ALL);
            mine &= keep_hi & keep_lo;
        }
        const uint32_t cnt = (uint32_t)__popc(mine);
        const uint32_t inc = wave_inclusive_scan_dpp(cnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        {
            uint32_t at = inc - cnt;
            s_before[lane] = (uint16_t)at;
            s_bits[lane] = (uint16_t)mine;
            for (uint32_t m = mine; m; m &= m - 1u) s_list[at++] = (uint16_t)(FL * (uint32_t)lane + (uint32_t)__builtin_ctz(m));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // this lane's Gaussian: its records are entries [lo, hi) of the segment's list
        auto records_before = [&](uint32_t slot) {   // slot in [seg, seg + SEG]
            const uint32_t o = slot - seg;
            if (o >= SEG) return total;
            return (uint32_t)s_before[o / FL] + (uint32_t)__popc((uint32_t)s_bits[o / FL] & ((1u << (o % FL)) - 1u));
        };
        uint32_t lo = 0u, hi = 0u;
        if (first < last && first < seg + SEG && last > seg) { lo = records_before(max(first, seg)); hi = records_before(min(last, seg + SEG)); }
        PBWD_CLK(t_list);
        PBWD_ADD(2, t_list - t_seg);
        PBWD_ADD(7, total);
        for (uint32_t p0 = 0; p0 < total; p0 += CAP) {
            PBWD_CLK(t_pass);
            PBWD_ADD(6, 1);
            const uint32_t n = min(CAP, total - p0);
            // ---- 2. the pass's records, densely into LDS ----
            for (uint32_t j0 = (uint32_t)lane; j0 < n; j0 += 64u * BIG_UNROLL) {
                float2 v[BIG_UNROLL][PF / 2];
#pragma unroll
                for (int u = 0; u < BIG_UNROLL; u++) {
                    const uint32_t j = j0 + 64u * (uint32_t)u;
                    const float2 *r = pg + (size_t)(PF / 2) * (seg + (uint32_t)s_list[p0 + min(j, n - 1u)]);
#pragma unroll
                    for (int k = 0; k < PF / 2; k++) v[u][k] = r[k];
                }
#pragma unroll
                for (int u = 0; u < BIG_UNROLL; u++) {
                    const uint32_t j = j0 + 64u * (uint32_t)u;
                    if (j < n) {
#pragma unroll
                        for (int k = 0; k < PF / 2; k++) s_rec[(PF / 2) * j + k] = v[u][k];
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- 3. every Gaussian's share of the pass ----
            PBWD_CLK(t_gathered);
            PBWD_ADD(3, t_gathered - t_pass);
            const uint32_t a = max(lo, p0), b = min(hi, p0 + n);   // (empty when a >= b)
            const bool wide = b > a && b - a > 64u;
            auto take = [&](v2f (&S)[PF / 2], uint32_t t) {
                const v2f *r = reinterpret_cast<const v2f *>(s_rec) + (PF / 2) * (t - p0);
#pragma unroll
                for (int k = 0; k < PF / 2; k++) S[k] += r[k];
            };
            if (!wide) {
                // TAKE records requested before the first is added (a lane's run is a chain of LDS round trips otherwise: the
                // lane with the longest run of the pass -- tens of records where a near surface fills its tiles -- sets the
                // wave's time); the additions are the same ones in the same order
                constexpr int TAKE = LVDGS_PBWD_TAKE;
                for (uint32_t t = a; t < b; t += TAKE) {
                    v2f v[TAKE][PF / 2];
#pragma unroll
                    for (int u = 0; u < TAKE; u++) {
                        const v2f *r = reinterpret_cast<const v2f *>(s_rec) + (t + u < b ? (PF / 2) * (t + u - p0) : ZERO_AT);
#pragma unroll
                        for (int k = 0; k < PF / 2; k++) v[u][k] = r[k];
                    }
#pragma unroll
                    for (int u = 0; u < TAKE; u++) {
#pragma unroll
                        for (int k = 0; k < PF / 2; k++) A2[k] += v[u][k];
                    }
                }
            }
#ifdef LVDGS_DIAG_PBWD
            {
                int trips = (!wide && b > a) ? (int)((b - a + LVDGS_PBWD_TAKE - 1) / LVDGS_PBWD_TAKE) : 0;
                trips = wave_max(trips);
                PBWD_ADD(8, trips);
                PBWD_ADD(9, __popcll(__ballot(wide)));
            }
#endif
            PBWD_CLK(t_wide);
            for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {
                const int src = __builtin_ctzll(todo);
                const uint32_t wa = (uint32_t)__builtin_amdgcn_readlane((int)a, src), wb = (uint32_t)__builtin_amdgcn_readlane((int)b, src);   // (src is wave-uniform)
                v2f S2[PF / 2];
#pragma unroll
                for (int k = 0; k < PF / 2; k++) S2[k] = v2f{0.f, 0.f};
                for (uint32_t t = wa + (uint32_t)lane; t < wb; t += 64u) take(S2, t);
                float S[10];
                unpack_sums<POSE_ONLY>(S2, S);
                // the 64 partial sums of every value, folded in a fixed order: halves of the wave, pairs of rows, then inside the rows
                float b0 = fold16(fold32(S[0], S[1]), fold32(S[2], S[3]));   // rows: S0 S2 S1 S3
                float b1 = fold16(fold32(S[4], S[5]), fold32(S[6], S[7]));   // rows: S4 S6 S5 S7
                const float e89 = fold32(S[8], S[9]);
                float b2 = fold16(e89, e89);                                 // rows: S8 S8 S9 S9
                row_sums3(b0, b1, b2);                                       // lane 15 of a row: the row's total
                auto at_lane = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
                const float tot[10] = {at_lane(b0, 15), at_lane(b0, 47), at_lane(b0, 31), at_lane(b0, 63), at_lane(b1, 15), at_lane(b1, 47),
                                       at_lane(b1, 31), at_lane(b1, 63), at_lane(b2, 15), at_lane(b2, 47)};
                if (lane == src) {   // (tot[5..8] are zero in the pose-only form)
                    A2[0] += v2f{tot[0], tot[1]}; A2[1] += v2f{tot[2], tot[3]};
                    if constexpr (POSE_ONLY) A2[2] += v2f{tot[4], tot[9]};
                    else { A2[2] += v2f{tot[4], tot[5]}; A2[3] += v2f{tot[6], tot[7]}; A2[4] += v2f{tot[8], tot[9]}; }
                }
            }
            PBWD_CLK(t_wide_done);
            PBWD_ADD(10, t_wide_done - t_wide);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            PBWD_CLK(t_summed);
            PBWD_ADD(4, t_summed - t_gathered);
        }
    }
    PBWD_CLK(t_end);
    PBWD_ADD(1, t_end - t_begin);
#ifdef LVDGS_DIAG_PBWD
    {
        const int w = (int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);   // (helper waves have rows of their own)
        if (lane == 0 && w < PBWD_DIAG_WAVES)
            for (int k = 0; k < PBWD_DIAG_VALUES; k++) g_pbwd_diag[PBWD_DIAG_VALUES * w + k] += diag[k];
    }
#endif
}

// ---- the stages of the per-Gaussian pass (preprocess_bwd_body below), in the order it runs them ----

// What a lane reads of its Gaussian, and what that says about it.
struct BwdInputs {
    int i;             // the Gaussian (a helper thread: its owner's)
    int32_t radius;
    uint32_t slot, tiles;   // its records: slots slot ... slot + tiles - 1
    float pos[3], opac_raw, sc[3], q[4], c6[6];   // raw (not activated) values
    bool in_map;       // i < N
    bool has_run;      // visible, with at least one listed pair
    bool live;         // ... and this thread is the one that works on it (not a helper)
};
// One round of ordinary loads, all of them waited for before the records are requested: the compiler waits for
// EVERYTHING outstanding (vmcnt(0)) at the first use of an ordinary load's result while LDS-DMA loads are in flight,
// so nothing loaded the ordinary way may be used for the first time between the request and the sums.  (Parameters of
// Gaussians that turn out invisible are read for nothing: 44 bytes each.)
template <bool POSE_ONLY>
__device__ __forceinline__ BwdInputs load_inputs(const BwdParams &p, int i, bool helper) {
    BwdInputs in;
    in.i = i; in.in_map = i < p.N;
    in.radius = 0; in.slot = 0u; in.tiles = 0u;
    in.pos[0] = in.pos[1] = in.pos[2] = 0.f; in.opac_raw = 0.f;
    in.sc[0] = in.sc[1] = in.sc[2] = 0.f; in.q[0] = 1.f; in.q[1] = in.q[2] = in.q[3] = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) in.c6[k] = 0.f;
    if (in.in_map) {
        in.radius = p.radii[i]; in.slot = p.slot_base[i]; in.tiles = p.tiles_touched[i];
    }
    if (in.in_map && !helper) {
        in.pos[0] = p.means3D[3 * i]; in.pos[1] = p.means3D[3 * i + 1]; in.pos[2] = p.means3D[3 * i + 2];
        if constexpr (!POSE_ONLY) in.opac_raw = p.opacities[i];
        if (p.cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) in.c6[k] = p.cov3D_precomp[6 * (size_t)i + k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) in.sc[k] = p.scales[3 * (size_t)i + k];
#pragma unroll
            for (int k = 0; k < 4; k++) in.q[k] = p.rotations[4 * (size_t)i + k];
        }
    }
    loads_complete_here(in.radius, in.slot, in.tiles, in.pos, in.opac_raw, in.sc, in.q, in.c6);
    // (a visible Gaussian without a listed pair -- none of its tiles in the band being rendered, or every tile ruled out by the
    // reach test -- has all-zero sums, and every output is linear in them: zeros are written and the arithmetic left out)
    in.has_run = in.in_map && in.radius > 0 && in.tiles > 0u;
    in.live = in.has_run && !helper;
    return in;
}

// Where the gradients w.r.t. the parameters go.  Memory (a launch per view): written, or -- `accumulate`: a later view of a mapping
// iteration -- added to what is there.  Registers (IN_REGS, preprocess_bwd_views_kernel: the per-Gaussian passes of several views of a
// mapping window in one launch): not added to memory view after view -- 56 bytes read and 56 written per visible Gaussian and view --
// but kept in the thread's GradAcc over the views and written once by the caller.  The additions are the ones the view-after-view
// launches make, in the same order: `assign` (the launch's first view when its gradients are not added to what the buffers hold) assigns.
struct GradAcc { float opac, m3[3], sc[3], rot[4], sh[3]; bool touched; };
// a Gaussian's three / four values as ONE 12- / 16-byte access per lane: the wave's stores are whole runs of memory
// instead of three or four passes of every-third-word stores over the same sectors
struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };
template <bool IN_REGS>
struct GradSink {
    GradAcc *acc;      // IN_REGS only
    bool accumulate, assign;
    // (dst: the value's place in memory; r: its place in GradAcc)
    __device__ __forceinline__ void put(float *dst, float GradAcc::*r, float v) const {
        if constexpr (IN_REGS) acc->*r = assign ? v : acc->*r + v;
        else *dst = accumulate ? *dst + v : v;
    }
    __device__ __forceinline__ void put3(float *dst, float (GradAcc::*r)[3], float a, float b, float c) const {
        if constexpr (IN_REGS) {
            float(&x)[3] = acc->*r;
            x[0] = assign ? a : x[0] + a; x[1] = assign ? b : x[1] + b; x[2] = assign ? c : x[2] + c;
        } else {
            f3 *d = reinterpret_cast<f3 *>(dst);
            if (accumulate) { const f3 o = *d; a += o.x; b += o.y; c += o.z; }
            *d = f3{a, b, c};
        }
    }
    __device__ __forceinline__ void put4(float *dst, float (GradAcc::*r)[4], float a, float b, float c, float e) const {
        if constexpr (IN_REGS) {
            float(&x)[4] = acc->*r;
            x[0] = assign ? a : x[0] + a; x[1] = assign ? b : x[1] + b; x[2] = assign ? c : x[2] + c; x[3] = assign ? e : x[3] + e;
        } else {
            f4 *d = reinterpret_cast<f4 *>(dst);
            if (accumulate) { const f4 o = *d; a += o.x; b += o.y; c += o.z; e += o.w; }
            *d = f4{a, b, c, e};
        }
    }
    // gradients an IN_REGS pass never has (precomputed colours or covariance: launch_preprocess_bwd_views): memory only
    __device__ __forceinline__ void put(float *dst, float v) const {
        if constexpr (IN_REGS) __builtin_unreachable();
        else *dst = accumulate ? *dst + v : v;
    }
    __device__ __forceinline__ void put3(float *dst, float a, float b, float c) const {
        if constexpr (IN_REGS) __builtin_unreachable();
        else put3(dst, nullptr, a, b, c);
    }
};
// A Gaussian of the map without pairs in this view: zeros.  (Adding zero: nothing to do; IN_REGS: the caller writes what the registers hold.)
template <bool IN_REGS>
__device__ __forceinline__ void zero_outputs(const BwdParams &p, int i, const GradSink<IN_REGS> &sink) {
#pragma unroll
    for (int k = 0; k < 3; k++) p.dmeans2D[3 * (size_t)i + k] = 0.f;
    if (!IN_REGS && !sink.accumulate) {
#pragma unroll
        for (int k = 0; k < 3; k++) p.dmeans3D[3 * (size_t)i + k] = 0.f;
        p.dopac[i] = 0.f;
        if (p.dscales) { for (int k = 0; k < 3; k++) p.dscales[3 * (size_t)i + k] = 0.f; }
        if (p.drot) { for (int k = 0; k < 4; k++) p.drot[4 * (size_t)i + k] = 0.f; }
        if (p.dcov3D) { for (int k = 0; k < 6; k++) p.dcov3D[6 * (size_t)i + k] = 0.f; }
        if (p.dcolors) { for (int k = 0; k < 3; k++) p.dcolors[3 * (size_t)i + k] = 0.f; }
        if (p.dshs) { for (int k = 0; k < 3 * p.cam.M; k++) p.dshs[(size_t)i * 3 * p.cam.M + k] = 0.f; }
    }
}

// The slots of a wave's 64 Gaussians: from the first slot of its first Gaussian to the end of its last one's (slot_base is the
// running sum of tiles_touched over ALL Gaussians, visible or not; the runs follow each other in memory: slots are in id order).
struct WaveRegion {
    uint32_t first, end;
    // The two parts of a large-footprint wave's region (HELPERS, below): the split half-way, at a whole number of sweep segments from the start
    __device__ __forceinline__ uint32_t split() const {
        return min(end, first + ((end - first) / 2u + (uint32_t)LVDGS_PBWD_SEG - 1u) / (uint32_t)LVDGS_PBWD_SEG * (uint32_t)LVDGS_PBWD_SEG);
    }
};
// (N: Gaussians of the map; i, slot, tiles: the calling lane's Gaussian, its first slot and its number of slots)
__device__ __forceinline__ WaveRegion wave_region(int N, int i, uint32_t slot, uint32_t tiles, int lane) {
    WaveRegion r{0u, 0u};
    if (i - lane < N) {
        const int last_lane = min(63, N - 1 - (i - lane));
        r.first = (uint32_t)__shfl((int)slot, 0, 64);
        r.end = (uint32_t)__shfl((int)(slot + tiles), last_lane, 64);
    }
    return r;
}

// ---- sum every Gaussian's per-tile partial gradients (a contiguous run of 40-byte records, fixed order) ----
// Records exist where blend_bwd wrote them (pair_valid): pairs behind their tile's last contributor have none.
//
// The runs of a wave's 64 Gaussians follow each other in memory (slots are in id order), so the wave streams that
// region through its own piece of LDS with coalesced 16-byte loads and every lane then picks its own records out of
// it -- instead of 64 lanes walking 64 different runs with one gather each per step, which moved 2.2x the bytes
// (r01 / r02_a counters).  The loads of the first chunk (at config 3 the only one for most waves) are issued BEFORE
// the part of the per-Gaussian arithmetic that does not depend on the sums -- projection, covariance, the EWA matrices,
// the rotation matrix -- and land while it runs: with the workgroup-wide staging of before (two workgroup barriers per
// chunk) the kernel was the sum of a memory phase and an arithmetic phase, every resident workgroup in the same one
// (ablation builds: 26.7 us without the arithmetic, 28.9 without the sums, 49.5 together).
//
// Three forms behind request_first_chunk() ... finish(), which leave the lane's ten sums in A:
//   streamed    no Gaussian of the wave has more than BIG_RUN pairs: the region in chunks of WAVE_CHUNK records, request + consume;
//   two parts   a wave with large-footprint Gaussians: the compacted sweep (above) over the region's first part, then its second;
//   helpers     (HELPERS: preprocess_bwd_helpers_kernel, frames whose Gaussians have large footprints, LVDGS_FLAG_SUPER_TILES) workgroups
//               of EIGHT waves -- wave 4 + w owns nothing and sweeps the second part of wave w's region while wave w sweeps the first.
// The sums of a large-footprint wave are DEFINED in two parts, (records in front of the split) + (records behind it), the split a
// function of the region alone (WaveRegion::split): both of its forms add the same numbers in the same order.
template <bool POSE_ONLY, bool HELPERS>
struct PairSums {
    static constexpr int PF = POSE_ONLY ? PAIR_FLOATS_POSE : PAIR_FLOATS;   // floats per pair record
    static constexpr int AREAS = HELPERS ? 8 : 4;                           // LDS staging areas: one per wave
    static constexpr int QUADS_PER_LANE = (WAVE_CHUNK * PF / 4 + 63) / 64;
    typedef float4 Stage[STAGE_BYTES<PF> / 16];
    typedef uint32_t ValidStage[WAVE_CHUNK / 4];
    Stage *s_pg4;          // [AREAS] (the last load instruction of a chunk is masked to the lanes inside it)
    ValidStage *s_valid4;  // [4]
    // (copies, not references to the caller's BwdParams / BwdInputs: in the views kernel, whose BwdParams is a per-view local, the
    // references cost 10 us per ten-view window -- profiles/preprocess_bwd_split/README.md)
    const float *pair_grads;
    const uint8_t *pair_valid;
    int N, i;               // what wave_region needs of the map and of the lane's Gaussian
    uint32_t slot, tiles;
    int lane, wave, area;
    bool helper, stream;    // stream: wave-uniform
    uint32_t first, last;   // the lane's run
    float (&A)[10];         // the lane's ten sums: the caller's array, held by reference as a lambda's capture would be (handed to every
                            // piece as an argument it changed the kernels' register counts: profiles/preprocess_bwd_split/README.md)
    uint32_t r_lo, r_hi;    // the wave's region as the streamed form reads it (empty in the other forms, which look it up when they start)

    __device__ __forceinline__ PairSums(const BwdParams &p, const BwdInputs &in, bool helper_, Stage *s_pg4_, ValidStage *s_valid4_, float (&A_)[10])
        : s_pg4(s_pg4_), s_valid4(s_valid4_), pair_grads(p.pair_grads), pair_valid(p.pair_valid), N(p.N), i(in.i), slot(in.slot), tiles(in.tiles), lane(threadIdx.x & 63), wave((threadIdx.x >> 6) & 3), area(threadIdx.x >> 6),
          helper(helper_), A(A_) {
        first = in.has_run ? in.slot : 0u;
        const uint32_t npairs = in.has_run ? in.tiles : 0u;
        last = first + npairs;
        const bool big = npairs > BIG_RUN;
        stream = __ballot(big) == 0ull;
        r_lo = r_hi = 0u;
        if (stream && !helper) {
            const WaveRegion region = wave_region(N, i, slot, tiles, lane);
            r_lo = region.first & ~3u;   // a chunk starts at a multiple of 4 records: on a 16-byte boundary of the records and a word of flags
            r_hi = region.end;
        }
    }

    // global -> LDS directly (global_load_lds: the wave's lanes land side by side, 1 KiB per instruction; no registers held
    // while the chunk is on its way): one chunk of records and their flags
    __device__ __forceinline__ void request(uint32_t c0) const {
        const float4 *pg_all = reinterpret_cast<const float4 *>(pair_grads);
        const uint32_t *valid_all = reinterpret_cast<const uint32_t *>(pair_valid);
        const uint32_t n = min((uint32_t)WAVE_CHUNK, r_hi - c0);
        const uint32_t quads = (n * PF + 3) / 4, q0 = c0 / 4 * PF;   // c0 is a multiple of 4: record c0 starts at float4 c0 * PF / 4
#pragma unroll
        for (int u = 0; u < QUADS_PER_LANE; u++) {
            const uint32_t k = (uint32_t)lane + 64u * (uint32_t)u;
            if (k < quads) __builtin_amdgcn_global_load_lds(pg_all + (size_t)q0 + k, &s_pg4[wave][64 * u], 16, 0, 0);
        }
        if ((uint32_t)lane * 4u < n) __builtin_amdgcn_global_load_lds(valid_all + c0 / 4 + (uint32_t)lane, &s_valid4[wave][0], 4, 0, 0);
    }
    __device__ __forceinline__ void consume(uint32_t c0) const {   // LDS -> every lane's own records, in slot order
        const uint32_t n = min((uint32_t)WAVE_CHUNK, r_hi - c0);
        wait_for_vector_memory();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float2 *s_pg = reinterpret_cast<const float2 *>(s_pg4[wave]);
        const uint8_t *s_valid = reinterpret_cast<const uint8_t *>(s_valid4[wave]);
        const uint32_t lo = max(first, c0), hi = min(last, c0 + n);
        for (uint32_t t = lo; t < hi; t++) {
            if (!s_valid[t - c0]) continue;   // (a record blend_bwd did not write: a pair behind its tile's last contributor)
            const float2 *r = s_pg + (PF / 2) * (t - c0);
            const float2 a0 = r[0], a1 = r[1], a2 = r[2];
            A[0] += a0.x; A[1] += a0.y; A[2] += a1.x; A[3] += a1.y; A[4] += a2.x;
            if constexpr (POSE_ONLY) A[9] += a2.y;
            else {
                const float2 a3 = r[3], a4 = r[4];
                A[5] += a2.y; A[6] += a3.x; A[7] += a3.y; A[8] += a4.x; A[9] += a4.y;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // (every form sweeps with the wave's own staging area)
    __device__ __forceinline__ void sweep(uint32_t from, uint32_t to, v2f (&A2)[PF / 2]) const {
        sum_region_compacted<POSE_ONLY>(pair_grads, pair_valid, reinterpret_cast<char *>(s_pg4[area]), first, last, from, to, A2);
    }
    // One part after the other.  A run lies in one part -- the other part's sum is +0, and x + 0 is x (no sum is ever -0: they
    // start at +0) -- except the ONE run that holds the split: that lane's first-part sums wait in scalar registers while its
    // registers start the second part at zero, and are added in front afterwards.
    __device__ __forceinline__ void sum_two_parts() const {
        const WaveRegion region = wave_region(N, i, slot, tiles, lane);
        const uint32_t split = region.split();
        v2f A2[PF / 2];
#pragma unroll
        for (int k = 0; k < PF / 2; k++) A2[k] = v2f{0.f, 0.f};
        sweep(region.first, split, A2);
        const uint64_t across = __ballot(first < split && last > split);
        const int owner_lane = across ? __builtin_ctzll(across) : 0;
        float kept[PF];
#pragma unroll
        for (int k = 0; k < PF / 2; k++) {
            kept[2 * k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(A2[k].x), owner_lane));
            kept[2 * k + 1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(A2[k].y), owner_lane));
            if (across && lane == owner_lane) A2[k] = v2f{0.f, 0.f};
        }
        sweep(split, region.end, A2);
#pragma unroll
        for (int k = 0; k < PF / 2; k++)
            if (across && lane == owner_lane) A2[k] = v2f{kept[2 * k], kept[2 * k + 1]} + A2[k];
        unpack_sums<POSE_ONLY>(A2, A);
    }
    // The owner wave sweeps the first part, its helper wave the second; the helper leaves its sums for the owner: lane l's ten
    // values side by side in the helper wave's staging area.
    __device__ __forceinline__ void sum_own_part() const {
        const WaveRegion region = wave_region(N, i, slot, tiles, lane);
        const uint32_t split = region.split();
        v2f A2[PF / 2];
#pragma unroll
        for (int k = 0; k < PF / 2; k++) A2[k] = v2f{0.f, 0.f};
        sweep(helper ? split : region.first, helper ? region.end : split, A2);
        unpack_sums<POSE_ONLY>(A2, A);
        if (helper) {
            float *out = reinterpret_cast<float *>(s_pg4[area]) + 10 * lane;
#pragma unroll
            for (int k = 0; k < 10; k++) out[k] = A[k];
        }
    }
    // ... and the owner adds them behind its own (every wave of the workgroup comes here, whichever form it took)
    __device__ __forceinline__ void add_helper_part() const {
        __syncthreads();
        if (!stream && !helper) {
            const float *in = reinterpret_cast<const float *>(s_pg4[area + 4]) + 10 * lane;
#pragma unroll
            for (int k = 0; k < 10; k++) A[k] = A[k] + in[k];
        }
    }

    // The streamed form's first chunk, requested ahead of the arithmetic that needs no sums.
    __device__ __forceinline__ void request_first_chunk() const {
#if LVDGS_PBWD_ABLATE != 1
        if (r_lo < r_hi) request(r_lo);
#endif
    }
    // A: [0,1] d/d pixel mean, [2..4] d/d conic a,b,c, [5] d/d opacity, [6..8] d/d rgb, [9] d/d view depth -- of the lane's Gaussian
    __device__ __forceinline__ void finish() const {
#pragma unroll
        for (int k = 0; k < 10; k++) A[k] = 0.f;
#if LVDGS_PBWD_ABLATE != 1
        if (stream) {
            for (uint32_t c0 = r_lo; c0 < r_hi; c0 += WAVE_CHUNK) {
                if (c0 != r_lo) request(c0);
                consume(c0);
            }
        } else if constexpr (HELPERS) sum_own_part();
        else sum_two_parts();
        if constexpr (HELPERS) add_helper_part();
#endif
    }
};

// ---- the part of the per-Gaussian arithmetic that needs no sums (the first chunk is on its way while it runs) ----
struct Projected {
    float pv[3];              // the mean in the camera's frame
    Ewa e;
    float Q00, Q01, Q11;      // the inverse of the 2-D covariance
    float qnorm;
    float sc[3], q[4], c6[6]; // activated scales and rotation, the 3-D covariance
};
// V: the view matrix in registers
__device__ __forceinline__ Projected project(const BwdParams &p, const BwdInputs &in, const float (&V)[16]) {
    Projected pr{{0.f, 0.f, 1.f}, Ewa{}, 0.f, 0.f, 0.f, 1.f, {in.sc[0], in.sc[1], in.sc[2]}, {in.q[0], in.q[1], in.q[2], in.q[3]},
                 {in.c6[0], in.c6[1], in.c6[2], in.c6[3], in.c6[4], in.c6[5]}};
#if LVDGS_PBWD_ABLATE != 2
    if (in.live) {
        xform3(in.pos, V, pr.pv);
        if (!p.cov3D_precomp) {
            activate_scale_rot(p.act, pr.sc, pr.q, pr.qnorm);
            cov3d_of(pr.sc, p.cam.scale_mod, pr.q, pr.c6);
        }
        ewa_setup(pr.pv, V, p.cam, pr.e);
        float ca, cb, cc;
        cov2d_of(pr.e, pr.c6, ca, cb, cc);
        const float det = ca * cc - cb * cb, di = 1.f / det;
        pr.Q00 = cc * di; pr.Q01 = -cb * di; pr.Q11 = ca * di;
    }
#endif
    return pr;
}

// ---- the chain from the ten sums to the gradients: one function per link, in the order the body calls them ----
// What the links hand on to each other.
struct ChainGrads {
    float ndc[2];          // d/d the mean in normalised device coordinates
    float rgb[3];
    float pview[3];        // d/d the mean in the camera's frame, through the covariance and the depth
    float pview_proj[3];   // ... through the projection of the mean
    float world[3];        // d/d the mean in the world
    float S[3][3];         // d/d the 3-D covariance
    float W[3][3];         // d/d the rotation part of the view matrix, through the EWA matrices
};

template <bool POSE_ONLY, bool IN_REGS>
__device__ __forceinline__ void chain_opacity_mean2d(const BwdParams &p, const float (&A)[10], const BwdInputs &in, const GradSink<IN_REGS> &sink, ChainGrads &g) {
    const int i = in.i;
    if constexpr (!POSE_ONLY) {
        // d/d(logit) = d/d(opacity) * o (1 - o) when the sigmoid is fused (o re-evaluated with the forward's expression: the
        // record holds it too, but reading 4 bytes of a 64-byte record per Gaussian moved 20 MB for 2)
        float o = in.opac_raw;
        if (p.act & ACT_SIGMOID_OPACITY) { o = 1.f / (1.f + expf(-o)); sink.put(&p.dopac[i], &GradAcc::opac, A[5] * o * (1.f - o)); }
        else sink.put(&p.dopac[i], &GradAcc::opac, A[5]);
    }
    g.ndc[0] = A[0] * 0.5f * (float)p.cam.W; g.ndc[1] = A[1] * 0.5f * (float)p.cam.H;
    if constexpr (!POSE_ONLY) *reinterpret_cast<f3 *>(&p.dmeans2D[3 * (size_t)i]) = f3{g.ndc[0], g.ndc[1], 0.f};
    g.rgb[0] = A[6]; g.rgb[1] = A[7]; g.rgb[2] = A[8];
    g.pview[0] = 0.f; g.pview[1] = 0.f; g.pview[2] = A[9];
    g.world[0] = 0.f; g.world[1] = 0.f; g.world[2] = 0.f;
}

// colour / SH; a view-dependent colour adds to g.world and to tau.  (POSE_ONLY: colours without view dependence only -- api.hip --
// which give the pose nothing)
template <bool POSE_ONLY, bool IN_REGS>
__device__ __forceinline__ void chain_colour(const BwdParams &p, const BwdInputs &in, const GradSink<IN_REGS> &sink, ChainGrads &g, float (&tau)[6]) {
    const Cam &c = p.cam;
    const int i = in.i;
    if constexpr (POSE_ONLY) {
    } else if (p.colors_precomp) {
        sink.put3(&p.dcolors[3 * (size_t)i], g.rgb[0], g.rgb[1], g.rgb[2]);
    } else {
        float d[3] = {in.pos[0] - c.campos[0], in.pos[1] - c.campos[1], in.pos[2] - c.campos[2]};
        const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const float u[3] = {d[0] / len, d[1] / len, d[2] / len};
        float B[16], G[16][3];
        sh_basis(c.sh_degree, u, B);
        sh_basis_grad(c.sh_degree, u, G);
        const int nb = (c.sh_degree + 1) * (c.sh_degree + 1);
        const float *sh = p.shs + (size_t)i * c.M * 3;
        float *dsh = p.dshs + (size_t)i * c.M * 3;
        // recompute the clamp mask
        float val[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nb) { val[0] += B[k] * sh[3 * k]; val[1] += B[k] * sh[3 * k + 1]; val[2] += B[k] * sh[3 * k + 2]; }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) if (val[ch] + 0.5f < 0.f) g.rgb[ch] = 0.f;
        float g_u[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nb) {
                sink.put3(&dsh[3 * k], &GradAcc::sh, B[k] * g.rgb[0], B[k] * g.rgb[1], B[k] * g.rgb[2]);   // (IN_REGS: k = 0 is the only one)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const float sg = sh[3 * k + ch] * g.rgb[ch];
                    g_u[0] += G[k][0] * sg; g_u[1] += G[k][1] * sg; g_u[2] += G[k][2] * sg;
                }
            }
        if (!IN_REGS && !sink.accumulate)
            for (int k = nb; k < c.M; k++) { dsh[3 * k] = 0.f; dsh[3 * k + 1] = 0.f; dsh[3 * k + 2] = 0.f; }
        // The view direction d = mean - camera centre moves with the mean and with the camera: C = -R^T T, and under
        // T_w2c <- Exp(tau) T_w2c dC/drho = -R^T, dC/dtheta = 0 at tau = 0, so dL/drho += R g_d (oracle: same statement,
        // pinned against the dense autograd formulation in float64).  Zero at SH degree 0.
        const float dot = u[0] * g_u[0] + u[1] * g_u[1] + u[2] * g_u[2];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float g_d = (g_u[a] - u[a] * dot) / len;
            g.world[a] += g_d;
#pragma unroll
            for (int j = 0; j < 3; j++) tau[j] += c.view[4 * a + j] * g_d;
        }
    }
}

// conic -> cov2D -> (cov3D, T): g.S, g.W, and the share of g.pview that comes through the EWA matrices
template <bool POSE_ONLY, bool IN_REGS>
__device__ __forceinline__ void chain_covariance(const BwdParams &p, const float (&A)[10], const BwdInputs &in, const Projected &pr,
                                                 const GradSink<IN_REGS> &sink, ChainGrads &g) {
    const Cam &c = p.cam;
    const Ewa &e = pr.e;
    const float *Vg = c.view;   // (read where it is used, not from the registers of the early arithmetic)
    const float Q00 = pr.Q00, Q01 = pr.Q01, Q11 = pr.Q11;
    const float G00 = A[2], G01 = 0.5f * A[3], G11 = A[4];
    const float QG00 = Q00 * G00 + Q01 * G01, QG01 = Q00 * G01 + Q01 * G11;
    const float QG10 = Q01 * G00 + Q11 * G01, QG11 = Q01 * G01 + Q11 * G11;
    const float Gs[2][2] = {{-(QG00 * Q00 + QG01 * Q01), -(QG00 * Q01 + QG01 * Q11)},
                            {-(QG00 * Q01 + QG01 * Q11), -(QG10 * Q01 + QG11 * Q11)}};
    float Sg[3][3];
    sym6(pr.c6, Sg);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int s = 0; s < 2; s++) v += e.T[r][a] * Gs[r][s] * e.T[s][b];
            g.S[a][b] = v;
        }
    if (!POSE_ONLY && p.dcov3D) {
        float *o = p.dcov3D + 6 * (size_t)in.i;
        sink.put(o + 0, g.S[0][0]); sink.put(o + 1, 2.f * g.S[0][1]); sink.put(o + 2, 2.f * g.S[0][2]);
        sink.put(o + 3, g.S[1][1]); sink.put(o + 4, 2.f * g.S[1][2]); sink.put(o + 5, g.S[2][2]);
    }
    float TS[2][3], g_T[2][3];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int b = 0; b < 3; b++) TS[r][b] = e.T[r][0] * Sg[0][b] + e.T[r][1] * Sg[1][b] + e.T[r][2] * Sg[2][b];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int b = 0; b < 3; b++) g_T[r][b] = 2.f * (Gs[r][0] * TS[0][b] + Gs[r][1] * TS[1][b]);
    float g_J00 = 0.f, g_J02 = 0.f, g_J11 = 0.f, g_J12 = 0.f;
    const float tz = e.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
    const float j00 = c.fx / tz, j02 = -(c.fx * e.t[0]) / tz2, j11 = c.fy / tz, j12 = -(c.fy * e.t[1]) / tz2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float w0 = Vg[4 * k + 0], w1 = Vg[4 * k + 1], w2 = Vg[4 * k + 2];
        g_J00 += g_T[0][k] * w0; g_J02 += g_T[0][k] * w2;
        g_J11 += g_T[1][k] * w1; g_J12 += g_T[1][k] * w2;
        g.W[0][k] = j00 * g_T[0][k];
        g.W[1][k] = j11 * g_T[1][k];
        g.W[2][k] = j02 * g_T[0][k] + j12 * g_T[1][k];
    }
    g.pview[0] += e.clx ? 0.f : -(c.fx / tz2) * g_J02;
    g.pview[1] += e.cly ? 0.f : -(c.fy / tz2) * g_J12;
    g.pview[2] += -(c.fx / tz2) * g_J00 - (c.fy / tz2) * g_J11 + (2.f * c.fx * e.t[0] / tz3) * g_J02 +
                  (2.f * c.fy * e.t[1] / tz3) * g_J12;
}

// projected mean through the full projection (world) and the raw projection (pose): g.world complete, g.pview_proj
template <bool POSE_ONLY, bool IN_REGS>
__device__ __forceinline__ void chain_mean(const BwdParams &p, const BwdInputs &in, const GradSink<IN_REGS> &sink, ChainGrads &g) {
    const float *Vg = p.cam.view, *PMg = p.cam.proj, *PRg = p.cam.proj_raw;
    float ph[3];
    xform3(in.pos, PMg, ph);
    const float phw = xform_w(in.pos, PMg);
    const float pw = 1.f / (phw + HOMOG_EPS);
    const float gh0 = g.ndc[0] * pw, gh1 = g.ndc[1] * pw, gh3 = -(g.ndc[0] * ph[0] + g.ndc[1] * ph[1]) * pw * pw;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g.world[a] += PMg[4 * a + 0] * gh0 + PMg[4 * a + 1] * gh1 + PMg[4 * a + 3] * gh3;
        g.pview_proj[a] = PRg[4 * a + 0] * gh0 + PRg[4 * a + 1] * gh1 + PRg[4 * a + 3] * gh3;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g.world[a] += Vg[4 * a + 0] * g.pview[0] + Vg[4 * a + 1] * g.pview[1] + Vg[4 * a + 2] * g.pview[2];
    }
    if constexpr (!POSE_ONLY) sink.put3(&p.dmeans3D[3 * (size_t)in.i], &GradAcc::m3, g.world[0], g.world[1], g.world[2]);
}

// camera pose: T' = Exp(tau) T
__device__ __forceinline__ void chain_pose(const BwdParams &p, const Projected &pr, const ChainGrads &g, float (&tau)[6]) {
    const float *Vg = p.cam.view;
    const float(&pv)[3] = pr.pv;
    const float gv[3] = {g.pview[0] + g.pview_proj[0], g.pview[1] + g.pview_proj[1], g.pview[2] + g.pview_proj[2]};
    tau[0] += gv[0]; tau[1] += gv[1]; tau[2] += gv[2];
    tau[3] = pv[1] * gv[2] - pv[2] * gv[1];
    tau[4] = pv[2] * gv[0] - pv[0] * gv[2];
    tau[5] = pv[0] * gv[1] - pv[1] * gv[0];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float w0 = Vg[4 * k + 0], w1 = Vg[4 * k + 1], w2 = Vg[4 * k + 2];
        tau[3] += w1 * g.W[2][k] - w2 * g.W[1][k];
        tau[4] += w2 * g.W[0][k] - w0 * g.W[2][k];
        tau[5] += w0 * g.W[1][k] - w1 * g.W[0][k];
    }
}

// Sigma3 -> scale, quaternion
template <bool IN_REGS>
__device__ __forceinline__ void chain_scale_rot(const BwdParams &p, const BwdInputs &in, const Projected &pr, const GradSink<IN_REGS> &sink, const ChainGrads &g) {
    const float(&sc)[3] = pr.sc;
    const float(&q)[4] = pr.q;
    float R[3][3];
    quat_rot(q, R);
    const float sm[3] = {p.cam.scale_mod * sc[0], p.cam.scale_mod * sc[1], p.cam.scale_mod * sc[2]};
    float g_R[3][3], g_sc[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        float v = 0.f;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float gm = 2.f * (g.S[a][0] * R[0][b] * sm[b] + g.S[a][1] * R[1][b] * sm[b] + g.S[a][2] * R[2][b] * sm[b]);
            v += gm * R[a][b];
            g_R[a][b] = gm * sm[b];
        }
        // fused exp: d/d(log s) = d/ds * s
        g_sc[b] = v * p.cam.scale_mod * ((p.act & ACT_EXP_SCALES) ? sc[b] : 1.f);
    }
    sink.put3(&p.dscales[3 * (size_t)in.i], &GradAcc::sc, g_sc[0], g_sc[1], g_sc[2]);
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    float dq[4];
    dq[0] = 2.f * (-z * g_R[0][1] + y * g_R[0][2] + z * g_R[1][0] - x * g_R[1][2] - y * g_R[2][0] + x * g_R[2][1]);
    dq[1] = 2.f * (y * g_R[0][1] + z * g_R[0][2] + y * g_R[1][0] - 2.f * x * g_R[1][1] - r * g_R[1][2] + z * g_R[2][0] + r * g_R[2][1] - 2.f * x * g_R[2][2]);
    dq[2] = 2.f * (-2.f * y * g_R[0][0] + x * g_R[0][1] + r * g_R[0][2] + x * g_R[1][0] + z * g_R[1][2] - r * g_R[2][0] + z * g_R[2][1] - 2.f * y * g_R[2][2]);
    dq[3] = 2.f * (-2.f * z * g_R[0][0] - r * g_R[0][1] + x * g_R[0][2] + r * g_R[1][0] - 2.f * z * g_R[1][1] + y * g_R[1][2] + x * g_R[2][0] + y * g_R[2][1]);
    if (p.act & ACT_NORMALIZE_ROT) {
        // q = raw / |raw|: d/d raw = (g - q (q . g)) / |raw|
        const float dot = q[0] * dq[0] + q[1] * dq[1] + q[2] * dq[2] + q[3] * dq[3];
#pragma unroll
        for (int k = 0; k < 4; k++) dq[k] = (dq[k] - q[k] * dot) / pr.qnorm;
    }
    sink.put4(&p.drot[4 * (size_t)in.i], &GradAcc::rot, dq[0], dq[1], dq[2], dq[3]);
}

// Every thread's six values -> the workgroup's six sums at out[0 .. 5], no atomics: a wave fold, then a four-term sum, the order of
// the additions fixed by the code.  s: the four waves' sums; adds: false for threads whose values do not count (helper waves).
__device__ __forceinline__ void workgroup_sum6(const float (&v)[6], float (&s)[4][6], bool adds, float *out) {
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const float w = wave_sum_to_lane63(v[k]);
        if (lane == 63 && adds) s[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < 6) out[threadIdx.x] = ((s[0][threadIdx.x] + s[1][threadIdx.x]) + s[2][threadIdx.x]) + s[3][threadIdx.x];
}

// The per-Gaussian pass of one view.
// POSE_ONLY (LVDGS_FLAG_POSE_ONLY): the pose gradient alone -- six-float pair records (d/d 2-D mean, conic, view depth), no
// opacity / colour reads, no parameter-gradient stores, no scale / quaternion chain.  The statements that make dL/dtau are the
// same ones in the same order: the partial sums are bit for bit those of the full form.
// IN_REGS: GradSink above.  HELPERS: PairSums above.
template <bool POSE_ONLY, bool IN_REGS = false, bool HELPERS = false>
__device__ __forceinline__ void preprocess_bwd_body(const BwdParams &p, GradAcc *acc = nullptr, bool assign = false) {
    static_assert(!(POSE_ONLY && IN_REGS), "the pose-only pass has no parameter gradients to keep");
    typedef PairSums<POSE_ONLY, HELPERS> Sums;
    __shared__ float s_tau[4][6];
    __shared__ typename Sums::Stage s_pg4[Sums::AREAS];
    __shared__ typename Sums::ValidStage s_valid4[4];
    if ((p.pair_total && *p.pair_total > p.pair_capacity) || (p.pair_total_super && *p.pair_total_super > p.pair_capacity)) return;   // (uniform over the launch)
    const bool helper = HELPERS && threadIdx.x >= 256;
    const int i = blockIdx.x * 256 + (threadIdx.x & 255);   // (a helper thread: its owner's Gaussian)
    // The camera's view matrix, read once into scalar registers (the compiler reads it with vector loads where it is
    // used -- the pointer is not known to be invariant -- and such a load's first use would end the overlap below).
    float V[16];
#pragma unroll
    for (int k = 0; k < 16; k++) V[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(p.cam.view[k])));
    float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const BwdInputs in = load_inputs<POSE_ONLY>(p, i, helper);
    const GradSink<IN_REGS> sink{acc, p.accumulate != 0, assign};
    if constexpr (IN_REGS) { if (in.live) acc->touched = true; }
    if (!POSE_ONLY && in.in_map && !in.live && !helper) zero_outputs(p, i, sink);

    float A[10];
    const Sums sums(p, in, helper, s_pg4, s_valid4, A);
    sums.request_first_chunk();
    const Projected pr = project(p, in, V);   // (needs no sums: the first chunk lands while it runs)
    sums.finish();

#if LVDGS_PBWD_ABLATE == 2
    if (in.live) { p.dmeans2D[3 * (size_t)i] = ((A[0] + A[1]) + (A[2] + A[3])) + ((A[4] + A[5]) + (A[6] + A[7])) + (A[8] + A[9]); }
    if (false) {
#else
    if (in.live) {
#endif
        ChainGrads g;
        chain_opacity_mean2d<POSE_ONLY>(p, A, in, sink, g);
        chain_colour<POSE_ONLY>(p, in, sink, g, tau);
        chain_covariance<POSE_ONLY>(p, A, in, pr, sink, g);
        chain_mean<POSE_ONLY>(p, in, sink, g);
        chain_pose(p, pr, g, tau);
        if (!POSE_ONLY && !p.cov3D_precomp) chain_scale_rot(p, in, pr, sink, g);
    }
    // one partial of the pose gradient per workgroup
    workgroup_sum6(tau, s_tau, !helper, p.tau_part + (size_t)blockIdx.x * 6);
}

// (two plain kernels around the body: a kernel TEMPLATE with this body loses its host stub -- "substitution failure" -- on this
// toolchain)
__global__ void __launch_bounds__(256, LVDGS_PBWD_WGS) preprocess_bwd_kernel(BwdParams p) { preprocess_bwd_body<false>(p); }
#ifndef LVDGS_PBWD_WGS_POSE
#define LVDGS_PBWD_WGS_POSE 5   // (6: 80 VGPRs with 7 spilled; same box 25.1 against 24.1 us at config 3)
#endif
__global__ void __launch_bounds__(256, LVDGS_PBWD_WGS_POSE) preprocess_bwd_pose_kernel(BwdParams p) { preprocess_bwd_body<true>(p); }
// ... with helper waves (512 threads: PairSums)
__global__ void __launch_bounds__(512, 2) preprocess_bwd_helpers_kernel(BwdParams p) { preprocess_bwd_body<false, false, true>(p); }
__global__ void __launch_bounds__(512, 2) preprocess_bwd_pose_helpers_kernel(BwdParams p) { preprocess_bwd_body<true, false, true>(p); }

// The per-Gaussian passes of up to PBWD_VIEWS views of one map in ONE launch (lvdgs_gaussian_backward_batch: the views of a mapping
// window behind their batched blend pass).  A thread walks its Gaussian through the views in order with the parameter gradients in
// registers (GradAcc above) and writes them once: the view-after-view launches read and wrote 56 bytes per visible Gaussian and view.
// Every view keeps what is its own: its records, its dL/d(2-D mean) array, its pose-gradient partials.
constexpr int PBWD_VIEWS = 12;
struct BwdView {
    Cam cam; const int32_t *radii; const float *rec; const uint32_t *tiles_touched, *slot_base; const float *pair_grads; const uint8_t *pair_valid;
    float *dmeans2D, *tau_part;
};
struct BwdViews { BwdParams common; int n; BwdView v[PBWD_VIEWS]; };
static_assert(sizeof(BwdViews) <= 4000, "kernel arguments");
#ifndef LVDGS_PBWD_VIEWS_WGS
#define LVDGS_PBWD_VIEWS_WGS 4
#endif
template <bool HELPERS>
__device__ __forceinline__ void preprocess_bwd_views_body(const BwdViews &b) {
    const bool owner = !HELPERS || threadIdx.x < 256;   // (helper waves own no Gaussian and hold no gradients)
    const int i = owner ? (int)blockIdx.x * 256 + (int)threadIdx.x : b.common.N;
    const bool add_to_memory = b.common.accumulate != 0;   // (the launch's sums are added to what the buffers hold)
    GradAcc acc{};
    if (add_to_memory && i < b.common.N) {
        acc.opac = b.common.dopac[i];
#pragma unroll
        for (int k = 0; k < 3; k++) { acc.m3[k] = b.common.dmeans3D[3 * (size_t)i + k]; acc.sc[k] = b.common.dscales[3 * (size_t)i + k]; acc.sh[k] = b.common.dshs[3 * (size_t)i + k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) acc.rot[k] = b.common.drot[4 * (size_t)i + k];
    }
    for (int k = 0; k < b.n; k++) {
        BwdParams p = b.common;
        const BwdView &v = b.v[k];
        p.cam = v.cam; p.radii = v.radii; p.rec = v.rec; p.tiles_touched = v.tiles_touched; p.slot_base = v.slot_base;
        p.pair_grads = v.pair_grads; p.pair_valid = v.pair_valid; p.dmeans2D = v.dmeans2D; p.tau_part = v.tau_part;
        preprocess_bwd_body<false, true, HELPERS>(p, &acc, k == 0 && !add_to_memory);
        __syncthreads();   // (the next view's pass uses the workgroup's LDS again)
    }
    if (i < b.common.N && (acc.touched || !add_to_memory)) {   // (a Gaussian no view of the launch saw: zeros, or what was there)
        b.common.dopac[i] = acc.opac;
        *reinterpret_cast<f3 *>(&b.common.dmeans3D[3 * (size_t)i]) = f3{acc.m3[0], acc.m3[1], acc.m3[2]};
        *reinterpret_cast<f3 *>(&b.common.dscales[3 * (size_t)i]) = f3{acc.sc[0], acc.sc[1], acc.sc[2]};
        *reinterpret_cast<f3 *>(&b.common.dshs[3 * (size_t)i]) = f3{acc.sh[0], acc.sh[1], acc.sh[2]};
        *reinterpret_cast<f4 *>(&b.common.drot[4 * (size_t)i]) = f4{acc.rot[0], acc.rot[1], acc.rot[2], acc.rot[3]};
    }
}
__global__ void __launch_bounds__(256, LVDGS_PBWD_VIEWS_WGS) preprocess_bwd_views_kernel(BwdViews b) { preprocess_bwd_views_body<false>(b); }
__global__ void __launch_bounds__(512, 4) preprocess_bwd_views_helpers_kernel(BwdViews b) { preprocess_bwd_views_body<true>(b); }

// fixed-order reduction of the per-workgroup pose partials (strided per-thread sums, then workgroup_sum6:
// two barriers fewer than an LDS tree, the order of the additions fixed by the code either way)
__global__ void __launch_bounds__(256) tau_reduce_kernel(const float *part, int nblk, float *out) {
    __shared__ float s[4][6];
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
        for (int k = 0; k < 6; k++) acc[k] += part[(size_t)b * 6 + k];
    workgroup_sum6(acc, s, true, out);
}

}  // namespace

// ---- host ----
typedef void (*BwdKernel)(BwdParams);
// helper waves where the caller expects large footprints (the two-level grouping's hint): the same sums, bit for bit, sooner
static BwdKernel bwd_kernel_for(bool pose_only, bool helpers) {
    if (pose_only) return helpers ? preprocess_bwd_pose_helpers_kernel : preprocess_bwd_pose_kernel;
    return helpers ? preprocess_bwd_helpers_kernel : preprocess_bwd_kernel;
}

// what is the map's and the caller's, not a view's: the parameters, their gradient buffers, how the gradients are combined with them
static BwdParams map_bwd_params(const lvdgs_args &a) {
    BwdParams p{};
    p.N = a.num_gaussians; p.act = a.activations;
    p.means3D = a.means3D; p.opacities = a.opacities; p.scales = a.scales; p.rotations = a.rotations; p.cov3D_precomp = a.cov3D_precomp;
    p.shs = a.shs; p.colors_precomp = a.colors_precomp;
    p.dmeans3D = a.dL_dmeans3D; p.dopac = a.dL_dopacities; p.dscales = a.dL_dscales;
    p.drot = a.dL_drotations; p.dcov3D = a.cov3D_precomp ? a.dL_dcov3D : nullptr; p.dshs = a.dL_dshs;
    p.dcolors = a.dL_dcolors; p.accumulate = (a.flags & LVDGS_FLAG_ACCUMULATE_PARAM_GRADS) ? 1 : 0;
    return p;
}

int launch_preprocess_bwd(const lvdgs_args &a, const GeomView &g, const BwdScratch &b, const uint8_t *pair_valid, hipStream_t s,
                          const uint32_t *pair_total, uint32_t pair_capacity, const uint32_t *pair_total_super) {
    const int N = a.num_gaussians;
    const int nblk = cdiv(N, 256);
    if (N > 0) {
        BwdParams p = map_bwd_params(a);
        p.cam = make_cam(a); p.radii = a.radii;
        p.rec = g.rec; p.tiles_touched = g.tiles_touched; p.slot_base = g.slot_base; p.pair_grads = b.pair_grads; p.pair_valid = pair_valid;
        p.dmeans2D = a.dL_dmeans2D; p.tau_part = b.tau_part;
        p.pair_total = pair_total; p.pair_total_super = pair_total_super; p.pair_capacity = pair_capacity;
        const bool helpers = (a.flags & LVDGS_FLAG_SUPER_TILES) != 0;
        if (int e = launch("preprocess_bwd", a.debug, s, bwd_kernel_for((a.flags & LVDGS_FLAG_POSE_ONLY) != 0, helpers), dim3(nblk), dim3(helpers ? 512 : 256), 0, p)) return e;
    }
    if (a.dL_dtau) {   // NULL: the partials stay in the scratch for lvdgs_tracking_tail
        if (int e = launch("tau_reduce", a.debug, s, tau_reduce_kernel, dim3(1), dim3(256), 0, b.tau_part, nblk, a.dL_dtau)) return e;
    }
    return LVDGS_OK;
}

// The per-Gaussian passes of n views of one map in one launch (preprocess_bwd_views_kernel); the caller has checked that the views
// share the map and the gradient buffers, colour by SH of ONE coefficient, scales + rotations (no precomputed covariance).
int launch_preprocess_bwd_views(const lvdgs_args *const *a, const GeomView *g, const BwdScratch *w, const BinView *b, int n, hipStream_t s) {
    const lvdgs_args &a0 = *a[0];
    const int N = a0.num_gaussians;
    const int nblk = cdiv(N, 256);
    for (int first = 0; first < n && N > 0; first += PBWD_VIEWS) {
        const int m = n - first < PBWD_VIEWS ? n - first : PBWD_VIEWS;
        BwdViews bv{};
        bv.common = map_bwd_params(a0);   // (no pair-count verdict: pair_total stays null)
        bv.common.dcolors = nullptr;      // (no precomputed colours)
        if (first > 0) bv.common.accumulate = 1;   // (a later group of the same call adds to what the first group wrote)
        bv.n = m;
        for (int k = 0; k < m; k++) {
            const int v = first + k;
            bv.v[k] = BwdView{make_cam(*a[v]), a[v]->radii, g[v].rec, g[v].tiles_touched, g[v].slot_base, w[v].pair_grads, b[v].pair_valid, a[v]->dL_dmeans2D, w[v].tau_part};
        }
        const bool helpers = (a0.flags & LVDGS_FLAG_SUPER_TILES) != 0;   // (as in launch_preprocess_bwd)
        if (int e = launch({"preprocess_bwd", "preprocess_bwd (views)"}, a0.debug, s, helpers ? preprocess_bwd_views_helpers_kernel : preprocess_bwd_views_kernel,
                dim3(nblk), dim3(helpers ? 512 : 256), 0, bv)) return e;
    }
    for (int v = 0; v < n; v++)
        if (a[v]->dL_dtau) {
            if (N == 0) { if (int e = check_hip(hipMemsetAsync(a[v]->dL_dtau, 0, 6 * sizeof(float), s), "memset tau")) return e; continue; }
            if (int e = launch("tau_reduce", a[v]->debug, s, tau_reduce_kernel, dim3(1), dim3(256), 0, w[v].tau_part, nblk, a[v]->dL_dtau)) return e;
        }
    return LVDGS_OK;
}

}  // namespace lvdgs

#ifdef LVDGS_DIAG_PBWD
extern "C" int lvdgs_diag_pbwd(unsigned long long *out_8192x12, int reset) {
    constexpr size_t BYTES = (size_t)lvdgs::PBWD_DIAG_WAVES * lvdgs::PBWD_DIAG_VALUES * sizeof(unsigned long long);
    if (out_8192x12 && hipMemcpyFromSymbol(out_8192x12, HIP_SYMBOL(lvdgs::g_pbwd_diag), BYTES) != hipSuccess) return LVDGS_E_HIP;
    if (reset) {
        void *dptr = nullptr;
        if (hipGetSymbolAddress(&dptr, HIP_SYMBOL(lvdgs::g_pbwd_diag)) != hipSuccess || hipMemset(dptr, 0, BYTES) != hipSuccess) return LVDGS_E_HIP;
    }
    return LVDGS_OK;
}
#endif
