// Matching two descriptor maps by reciprocal nearest neighbours (the reference's get_pose starts with fast_reciprocal_NNs(desc1, desc2,
// subsample_or_initxy1=8, dist='dot'): blocks of A @ B.T + max on the device and a device-to-host copy after every half round).
// Semantics: include/lvdgs.h, DESIGN.md section 4d.
//
// 2 + 4 max_iter launches per call, all enqueued at once:
//   rnn_init_kernel   : the seed grid, every seed active, the merge keys cleared.
//   rnn_search_kernel : one half round's arg-max as a tall-skinny GEMM with an arg-max epilogue.  A workgroup holds 128 active queries
//                       (4 tiles of 32) in LDS and streams a chunk of the database map past them: each of its four waves takes
//                       RNN_WAVE_TILES tiles of 32 database rows, and a 32 x 32 tile of scores is dim / 2 v_mfma_f32_32x32x2_f32 -- exact
//                       f32, bitwise one fmaf chain over the components in ascending order, the same for every row whatever its place in
//                       a tile.  The database rows are the A operand, so a lane keeps ONE query (its column) and sixteen database rows
//                       (its registers): the running arg-max is per lane, in registers, strict > in ascending row order.  Lanes, waves
//                       and workgroups are then merged by a 64-bit max over (order-preserving score bits, complemented index): the order
//                       of the merge cannot matter, the lowest index wins a tie.  Workgroups beyond the active count return at once.
//   rnn_update_kernel : one workgroup.  Decodes the winners, retires the seeds that repeat themselves, compacts the active list (stable:
//                       ascending seed order) and leaves its length for the next search.
//   rnn_final_kernel  : one workgroup.  Bitonic sort of the retired seeds' (xy1, xy2) keys in LDS, distinct, pixel coordinates, the state
//                       words through pinned memory.
// No workgroup waits on another; every loop is bounded.
#include <math.h>

#include "common.hpp"
#include "device_utils.hpp"

namespace lvdgs {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int RNN_THREADS = 256;
constexpr int RNN_WAVES = RNN_THREADS / WAVE;
constexpr int RNN_TILE = 32;                         // the MFMA's tile edge
constexpr int RNN_QT = 4;                            // query tiles per workgroup
constexpr int RNN_QGROUP = RNN_QT * RNN_TILE;        // queries per workgroup
constexpr int RNN_QSTRIDE = RNN_QGROUP + 32;         // floats between two components in LDS: the two lane halves hit different banks
constexpr int RNN_WAVE_TILES = 4;                    // database tiles per wave
constexpr int RNN_KS_MAX = LVDGS_RNN_MAX_DIM / 2;
constexpr int RNN_ONE = 1024;                        // threads of the single-workgroup kernels
constexpr u64 RNN_DROPPED = ~0ull;                   // sort key of an unconverged seed (a map index is below 2^31)

struct RnnHeader {
    uint32_t nact[2];     // length of the active list a half round reads: [half & 1]
    uint32_t rounds;      // rounds that began with an active seed
    uint32_t pad[61];
};

struct RnnParams {
    int W1, H1, W2, H2, D, S, seeds, seeds_x, capacity;
    const float *desc1, *desc2;
    int32_t *m1;
    float *m2;
    int32_t *seed_state;
    RnnHeader *hdr;
    int32_t *xy1, *xy2, *old1, *old2, *retired;   // per seed
    uint32_t *act[2];                             // the active seeds, ascending; a half round reads [half & 1] and writes the other
    u64 *keys;                                    // per seed: the merge key of the search in flight (0 between searches)
    int32_t *host_state;                          // device address of the caller's pinned block
};

__device__ __forceinline__ uint32_t ordered_bits(float f) {   // a < b  <=>  ordered_bits(a) < ordered_bits(b), for all non-NaN floats
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ void __launch_bounds__(RNN_THREADS) rnn_init_kernel(RnnParams P) {
    const int k = blockIdx.x * RNN_THREADS + threadIdx.x;
    if (k == 0) { P.hdr->nact[0] = (uint32_t)P.seeds; P.hdr->nact[1] = 0; P.hdr->rounds = 0; }
    if (k >= P.seeds) return;
    const int gy = k / P.seeds_x, gx = k - gy * P.seeds_x;
    const int xy = (P.S / 2 + gx * P.S) + P.W1 * (P.S / 2 + gy * P.S);
    P.xy1[k] = xy; P.old1[k] = xy; P.xy2[k] = -1; P.old2[k] = -1; P.retired[k] = 0;
    P.act[0][k] = (uint32_t)k;
    P.keys[k] = 0;
}

// the running arg-max of one lane over the sixteen rows of a score tile it holds: row_base + (r & 3) + 8 (r >> 2), ascending in r
template <bool TAIL>
__device__ __forceinline__ void tile_argmax(const f32x16 &acc, int row_base, int N, float &best, int &bidx) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = row_base + (r & 3) + 8 * (r >> 2);
        const float v = acc[r];
        bool gt = v > best;
        if (TAIL) gt = gt && row < N;
        best = gt ? v : best;
        bidx = gt ? row : bidx;
    }
}

// KS_T: dim / 2 rounded up when the launcher has a build for it (the database fragment of a tile is then loaded at once), 0: any dim
template <int KS_T>
__global__ void __launch_bounds__(RNN_THREADS) rnn_search_kernel(RnnParams P, int half) {
    __shared__ float s_q[2 * RNN_KS_MAX * RNN_QSTRIDE];   // [component][query]
    __shared__ int s_row[RNN_QGROUP];
    __shared__ u64 s_keys[RNN_WAVES][RNN_QGROUP];
    const int dir = half & 1;
    const int nact = (int)P.hdr->nact[dir];
    const int q0 = blockIdx.y * RNN_QGROUP;
    if (q0 >= nact) return;                                // (uniform: before any barrier)
    const int nq = min(RNN_QGROUP, nact - q0), nqt = (nq + RNN_TILE - 1) / RNN_TILE;
    const uint32_t *act = P.act[dir];
    const float *qmap = dir ? P.desc2 : P.desc1, *db = dir ? P.desc1 : P.desc2;
    const int32_t *qrow = dir ? P.xy2 : P.xy1;
    const int N = dir ? P.W1 * P.H1 : P.W2 * P.H2, Nq = dir ? P.W2 * P.H2 : P.W1 * P.H1;
    const int D = P.D, KS = KS_T > 0 ? KS_T : (D + 1) / 2, Dpad = 2 * KS;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, j = lane % RNN_TILE, h = lane / RNN_TILE;

    if (tid < RNN_QGROUP) s_row[tid] = tid < nq ? min(max(qrow[act[q0 + tid]], 0), Nq - 1) : -1;
    __syncthreads();
    for (int e = tid; e < RNN_QGROUP * Dpad; e += RNN_THREADS) {
        const int q = e / Dpad, k = e - q * Dpad, row = s_row[q];
        s_q[k * RNN_QSTRIDE + q] = (row >= 0 && k < D) ? qmap[(size_t)row * D + k] : 0.f;
    }
    __syncthreads();

    const int ntiles = (N + RNN_TILE - 1) / RNN_TILE;
    const int t0 = (blockIdx.x * RNN_WAVES + wave) * RNN_WAVE_TILES, t1 = min(t0 + RNN_WAVE_TILES, ntiles);
    float best[RNN_QT];
    int bidx[RNN_QT];
#pragma unroll
    for (int qt = 0; qt < RNN_QT; qt++) { best[qt] = -INFINITY; bidx[qt] = min(t0 * RNN_TILE, N - 1); }
    const float *sq = s_q + j;
    for (int t = t0; t < t1; t++) {
        const int r0 = t * RNN_TILE;
        const float *p = db + (size_t)min(r0 + j, N - 1) * D;    // a row past the map reads the last one; its scores are masked below
        f32x16 acc[RNN_QT];
#pragma unroll
        for (int qt = 0; qt < RNN_QT; qt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[qt][r] = 0.f;
        if (KS_T > 0) {
            float a[KS_T > 0 ? KS_T : 1];
#pragma unroll
            for (int s = 0; s < KS_T; s++) {
                const int k = 2 * s + h;
                a[s] = p[min(k, D - 1)];
                a[s] = k < D ? a[s] : 0.f;
            }
#pragma unroll
            for (int s = 0; s < KS_T; s++) {
                const float *b = sq + (2 * s + h) * RNN_QSTRIDE;
#pragma unroll
                for (int qt = 0; qt < RNN_QT; qt++)
                    if (qt < nqt) acc[qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[qt * RNN_TILE], acc[qt], 0, 0, 0);
            }
        } else {
            float a = p[min(h, D - 1)];
            a = h < D ? a : 0.f;
            for (int s = 0; s < KS; s++) {
                const int kn = 2 * (s + 1) + h;
                float an = p[min(kn, D - 1)];                    // the next step's component, in flight under this step's products
                an = kn < D ? an : 0.f;
                const float *b = sq + (2 * s + h) * RNN_QSTRIDE;
#pragma unroll
                for (int qt = 0; qt < RNN_QT; qt++)
                    if (qt < nqt) acc[qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[qt * RNN_TILE], acc[qt], 0, 0, 0);
                a = an;
            }
        }
        if (r0 + RNN_TILE > N) {
#pragma unroll
            for (int qt = 0; qt < RNN_QT; qt++)
                if (qt < nqt) tile_argmax<true>(acc[qt], r0 + 4 * h, N, best[qt], bidx[qt]);
        } else {
#pragma unroll
            for (int qt = 0; qt < RNN_QT; qt++)
                if (qt < nqt) tile_argmax<false>(acc[qt], r0 + 4 * h, N, best[qt], bidx[qt]);
        }
    }
    // ---- the merge: lane halves, waves, workgroups ----
#pragma unroll
    for (int qt = 0; qt < RNN_QT; qt++) {
        u64 key = t0 < t1 ? ((u64)ordered_bits(best[qt]) << 32) | (u64)(~(uint32_t)bidx[qt]) : 0ull;
        const u64 other = ((u64)(uint32_t)__shfl_xor((int)(key >> 32), RNN_TILE, WAVE) << 32) | (u64)(uint32_t)__shfl_xor((int)(uint32_t)key, RNN_TILE, WAVE);
        key = other > key ? other : key;
        if (h == 0) s_keys[wave][qt * RNN_TILE + j] = key;
    }
    __syncthreads();
    if (tid < nq) {
        u64 key = s_keys[0][tid];
#pragma unroll
        for (int w = 1; w < RNN_WAVES; w++) key = s_keys[w][tid] > key ? s_keys[w][tid] : key;
        u64 *dst = P.keys + act[q0 + tid];
        // (the plain look first spares most of the atomics: a key that cannot raise the maximum changes nothing)
        if (key > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            __hip_atomic_fetch_max(dst, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(RNN_ONE) rnn_update_kernel(RnnParams P, int half) {
    __shared__ int s_scan[SCAN_WORDS];
    const int dir = half & 1, tid = threadIdx.x;
    const int nact = (int)P.hdr->nact[dir];
    const uint32_t *src = P.act[dir];
    uint32_t *dst = P.act[dir ^ 1];
    const int N = dir ? P.W1 * P.H1 : P.W2 * P.H2;
    const int per = (nact + RNN_ONE - 1) / RNN_ONE, lo = min(tid * per, nact), hi = min(lo + per, nact);
    int cnt = 0;
    for (int a = lo; a < hi; a++) {
        const uint32_t seed = src[a];
        const u64 key = P.keys[seed];
        P.keys[seed] = 0;
        const int idx = (int)min(~(uint32_t)key, (uint32_t)(N - 1));
        bool still;
        if (dir == 0) {
            P.xy2[seed] = idx;
            still = idx != P.old2[seed];
        } else {
            P.xy1[seed] = idx;
            still = idx != P.old1[seed];
            P.old1[seed] = idx; P.old2[seed] = P.xy2[seed];
        }
        if (!still) P.retired[seed] = 1;
        cnt += still ? 1 : 0;
    }
    int total;
    int out = scan_workgroup<RNN_ONE>(cnt, s_scan, &total);
    for (int a = lo; a < hi; a++) {
        const uint32_t seed = src[a];
        if (!P.retired[seed]) dst[out++] = seed;   // (this thread's own writes)
    }
    if (tid == 0) {
        P.hdr->nact[dir ^ 1] = (uint32_t)total;
        if (dir == 0 && nact > 0) P.hdr->rounds = (uint32_t)(half / 2 + 1);
    }
}

__global__ void __launch_bounds__(RNN_ONE) rnn_final_kernel(RnnParams P, int n2) {
    extern __shared__ u64 s_key[];   // n2: a power of two >= 2 RNN_ONE and >= seeds
    __shared__ int s_scan[SCAN_WORDS];
    const int tid = threadIdx.x;
    int kept = 0;
    for (int i = tid; i < n2; i += RNN_ONE) {
        u64 key = RNN_DROPPED;
        if (i < P.seeds) {
            const int a = P.xy1[i], b = P.xy2[i], r = P.retired[i];
            if (r) key = ((u64)(uint32_t)a << 32) | (u64)(uint32_t)b;
            kept += r ? 1 : 0;
            if (P.seed_state) { P.seed_state[3 * i] = a; P.seed_state[3 * i + 1] = b; P.seed_state[3 * i + 2] = r ? 1 : 0; }
        }
        s_key[i] = key;
    }
    int retired;
    scan_workgroup<RNN_ONE>(kept, s_scan, &retired);   // (its two barriers, passed by every thread, also publish s_key to the sort below)
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += RNN_ONE) {
                const int o = i ^ j;
                if (o > i) {
                    const u64 x = s_key[i], y = s_key[o];
                    if ((x > y) == ((i & k) == 0)) { s_key[i] = y; s_key[o] = x; }
                }
            }
            __syncthreads();
        }
    }
    const int per = n2 / RNN_ONE, lo = tid * per;
    int cnt = 0;
    for (int i = lo; i < lo + per; i++) cnt += (s_key[i] != RNN_DROPPED && (i == 0 || s_key[i] != s_key[i - 1])) ? 1 : 0;
    int M;
    int out = scan_workgroup<RNN_ONE>(cnt, s_scan, &M);   // (s_scan again: the sort's barriers lie between the two scans)
    for (int i = lo; i < lo + per; i++) {
        const u64 key = s_key[i];
        if (key != RNN_DROPPED && (i == 0 || key != s_key[i - 1]) && out < P.capacity) {
            const int a = (int)(key >> 32), b = (int)(uint32_t)key;
            P.m1[2 * out] = a % P.W1; P.m1[2 * out + 1] = a / P.W1;
            P.m2[2 * out] = (float)(b % P.W2); P.m2[2 * out + 1] = (float)(b / P.W2);
            out++;
        }
    }
    if (tid == 0) {
        // NOT sealed (device_utils.hpp: seal_host_block), like pnp.hip's write_state: the host's wait for the stream is what makes the block complete.
        // Measured on the MI355X: volatile payload stores and the seal cost 10-14 us per call, outside its run-to-run spread.
        int32_t *w = P.host_state;
        w[1] = P.seeds; w[2] = M; w[3] = P.seeds - retired; w[4] = (int32_t)P.hdr->rounds; w[5] = 0; w[6] = 0; w[7] = 0;
        w[0] = LVDGS_RNN_OK;
        __threadfence_system();
    }
}

int seeds_along(int n, int S) { return n > S / 2 ? (n - S / 2 + S - 1) / S : 0; }

// the scratch: the header, seven columns of a word per seed, a key per seed
size_t rnn_layout(size_t seeds, RnnParams *P, void *base) {
    Carver<RnnParams> c(P, base);
    c(c.v.hdr, 1);
    c(c.v.xy1, seeds); c(c.v.xy2, seeds); c(c.v.old1, seeds); c(c.v.old2, seeds); c(c.v.retired, seeds);
    c(c.v.act[0], seeds); c(c.v.act[1], seeds);
    c(c.v.keys, seeds);
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_recip_nn_scratch_bytes(int32_t width1, int32_t height1, int32_t subsample) {
    if (width1 <= 0 || height1 <= 0 || subsample <= 0) return 0;
    return rnn_layout((size_t)seeds_along(width1, subsample) * (size_t)seeds_along(height1, subsample), nullptr, nullptr);
}

int lvdgs_reciprocal_nn(const lvdgs_recip_nn_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    static unsigned char lds_done[16];
    if (!a) { set_error("recip_nn: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width1 <= 0 || a->height1 <= 0 || a->width2 <= 0 || a->height2 <= 0) {
        set_error("recip_nn: bad map size %dx%d / %dx%d", a->width1, a->height1, a->width2, a->height2); return LVDGS_E_INVALID;
    }
    if (a->dim < 1 || a->dim > LVDGS_RNN_MAX_DIM) { set_error("recip_nn: dim %d outside 1..%d", a->dim, LVDGS_RNN_MAX_DIM); return LVDGS_E_INVALID; }
    if ((int64_t)a->width1 * a->height1 * a->dim > INT32_MAX || (int64_t)a->width2 * a->height2 * a->dim > INT32_MAX) {
        set_error("recip_nn: a map of more than 2^31 - 1 floats"); return LVDGS_E_INVALID;
    }
    if (a->subsample < 1) { set_error("recip_nn: subsample %d < 1", a->subsample); return LVDGS_E_INVALID; }
    if (a->max_iter < 1) { set_error("recip_nn: max_iter %d < 1", a->max_iter); return LVDGS_E_INVALID; }
    const int sx = seeds_along(a->width1, a->subsample), sy = seeds_along(a->height1, a->subsample);
    const int64_t seeds = (int64_t)sx * sy;
    if (seeds < 1) { set_error("recip_nn: subsample %d leaves a %dx%d map no seed", a->subsample, a->width1, a->height1); return LVDGS_E_INVALID; }
    if (seeds > LVDGS_RNN_MAX_SEEDS) { set_error("recip_nn: %lld seeds, more than %d", (long long)seeds, LVDGS_RNN_MAX_SEEDS); return LVDGS_E_INVALID; }
    if (a->capacity < seeds) { set_error("recip_nn: capacity %d below the seed count %lld", a->capacity, (long long)seeds); return LVDGS_E_INVALID; }
    if (!a->desc1 || !a->desc2 || !a->matches_im1 || !a->matches_im2 || !a->host_state || !a->scratch) {
        set_error("recip_nn: desc1 / desc2 / matches_im1 / matches_im2 / host_state / scratch is NULL"); return LVDGS_E_INVALID;
    }
    RnnParams P{};
    if (a->scratch_bytes < rnn_layout((size_t)seeds, &P, a->scratch)) { set_error("recip_nn: scratch too small"); return LVDGS_E_INVALID; }
    P.W1 = a->width1; P.H1 = a->height1; P.W2 = a->width2; P.H2 = a->height2; P.D = a->dim; P.S = a->subsample;
    P.seeds = (int)seeds; P.seeds_x = sx; P.capacity = a->capacity;
    P.desc1 = a->desc1; P.desc2 = a->desc2; P.m1 = a->matches_im1; P.m2 = a->matches_im2; P.seed_state = a->seed_state;
    if (int e = host_block_address(a->host_state, "recip_nn", &P.host_state)) return e;
    int n2 = 2 * RNN_ONE;
    while (n2 < P.seeds) n2 *= 2;
    if (int e = allow_dynamic_lds(reinterpret_cast<const void *>(&rnn_final_kernel), LVDGS_RNN_MAX_SEEDS * (int)sizeof(u64), lds_done)) return e;
    if (int e = launch("rnn_init", 0, s, rnn_init_kernel, dim3(cdiv(P.seeds, RNN_THREADS)), dim3(RNN_THREADS), 0, P)) return e;
    const int groups = cdiv(P.seeds, RNN_QGROUP);
    const int ks = (P.D + 1) / 2;
    for (int half = 0; half < 2 * a->max_iter; half++) {
        const int N = (half & 1) ? P.W1 * P.H1 : P.W2 * P.H2;
        const dim3 grid(cdiv(cdiv(N, RNN_TILE), RNN_WAVES * RNN_WAVE_TILES), groups);
        if (int e = launch("rnn_search", 0, s, ks == 12 ? rnn_search_kernel<12> : rnn_search_kernel<0>, grid, dim3(RNN_THREADS), 0, P, half)) return e;
        if (int e = launch("rnn_update", 0, s, rnn_update_kernel, dim3(1), dim3(RNN_ONE), 0, P, half)) return e;
    }
    if (int e = launch("rnn_final", 0, s, rnn_final_kernel, dim3(1), dim3(RNN_ONE), (size_t)n2 * sizeof(u64), P, n2)) return e;
    return LVDGS_OK;
}

}  // extern "C"
