// Pose initialisation by PnP-RANSAC on the rendered depth (reference utils/init_pose.py get_pose :160-175: cv2.undistortPoints +
// depth_to_3d over every pixel + cv2.solvePnPRansac on the host, called for every tracked frame, utils/slam_frontend.py:1448).
// Semantics: include/lvdgs.h, DESIGN.md section 4c.
//
// Two launches per call, both enqueued at once:
//   pnp_gather_kernel     : one thread per match.  The depth lookup, the validity test, both ten-step undistortions, the object point;
//                           clears the inlier mask and the ticket.
//   pnp_hypotheses_kernel : one wave64 per hypothesis (four per 256-thread workgroup).  Every lane draws the same three matches and runs
//                           the same eight 6 x 6 Gauss-Newton steps (redundantly: nothing to exchange); the 64 lanes then stride over the
//                           matches for the score.  The LAST workgroup to take a ticket (agent-scope release / acquire, as
//                           depth_align.hip) picks the winner and goes straight on to the refinement: its 256 threads stride over the
//                           matches, the normal equations are summed in a fixed order (per thread, xor butterfly per wave, the four waves
//                           in order), and every thread solves the same 6 x 6 system.  No workgroup waits on another; every loop is bounded.
// All solver arithmetic is float64 from the float32 / int32 loads; the host reads the state block once, through pinned memory.
#include <math.h>

#include "common.hpp"
#include "device_utils.hpp"

namespace lvdgs {
namespace {

constexpr int PNP_THREADS = 256;
constexpr int PNP_WAVES = PNP_THREADS / WAVE;
constexpr int PNP_UNDISTORT_ITERS = 10;
constexpr int PNP_SAMPLE_DRAWS = 32;
constexpr int PNP_HYP_STEPS = 8;
constexpr int PNP_REFINE_ROUNDS = 3;
constexpr int PNP_REFINE_STEPS = 5;
constexpr int PNP_MIN_VALID = 6;
constexpr double PNP_DAMPING = 1e-3;
constexpr double PNP_SMALL_ANGLE = 1e-5;   // pose_utils' series threshold
constexpr int NA = 21, NG = 6, NS = NA + NG;   // packed upper triangle of J^T J, J^T r

struct PnpHeader {
    uint32_t ticket;      // cleared by the gather launch of every call
    uint32_t pad[63];
};

struct HypRec {           // one per hypothesis
    double pose[12];      // row-major [R | t]
    int32_t count;        // inliers; -1: void
    int32_t pad[7];
};
static_assert(sizeof(HypRec) == 128, "hypothesis record");

struct Pose {
    double R[9], t[3];
};

struct PnpParams {
    int W, H, M, hyp, min_inliers;
    uint32_t seed;
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, thr2;
    const float *depth;
    const int32_t *m1;
    const float *m2;
    uint8_t *mask;
    PnpHeader *hdr;
    double *px, *py, *pz, *qu, *qv;   // M each: the object point (pz == 0: the match is not valid), the frame point normalised
    HypRec *recs;
    int32_t *host_state;              // device address of the caller's pinned block
};

__host__ __device__ inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ void undistort(const PnpParams &P, double u, double v, double &x, double &y) {
    const double x0 = (u - P.cx) / P.fx, y0 = (v - P.cy) / P.fy;
    x = x0; y = y0;
    for (int it = 0; it < PNP_UNDISTORT_ITERS; it++) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1.0 + ((P.k3 * r2 + P.k2) * r2 + P.k1) * r2);
        const double dx = 2.0 * P.p1 * x * y + P.p2 * (r2 + 2.0 * x * x);
        const double dy = P.p1 * (r2 + 2.0 * y * y) + 2.0 * P.p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
}

__global__ void __launch_bounds__(PNP_THREADS) pnp_gather_kernel(PnpParams P) {
    if (blockIdx.x == 0 && threadIdx.x == 0) P.hdr->ticket = 0;   // (the kernel boundary orders it before the tickets)
    const int i = blockIdx.x * PNP_THREADS + threadIdx.x;
    if (i >= P.M) return;
    const int x = P.m1[2 * i], y = P.m1[2 * i + 1];
    double Z = 0.0;
    if (x >= 0 && x < P.W && y >= 0 && y < P.H) {
        const double d = (double)P.depth[(size_t)y * P.W + x];
        if (isfinite(d) && d > 0.0) Z = d;
    }
    double xn, yn, un, vn;
    undistort(P, (double)x, (double)y, xn, yn);
    undistort(P, (double)P.m2[2 * i], (double)P.m2[2 * i + 1], un, vn);
    P.px[i] = xn * Z; P.py[i] = yn * Z; P.pz[i] = Z;
    P.qu[i] = un; P.qv[i] = vn;
    P.mask[i] = 0;
}

__device__ __forceinline__ void identity(Pose &T) {
    for (int i = 0; i < 9; i++) T.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    T.t[0] = T.t[1] = T.t[2] = 0.0;
}

__device__ __forceinline__ void transform(const Pose &T, double px, double py, double pz, double &X, double &Y, double &Z) {
    X = T.R[0] * px + T.R[1] * py + T.R[2] * pz + T.t[0];
    Y = T.R[3] * px + T.R[4] * py + T.R[5] * pz + T.t[1];
    Z = T.R[6] * px + T.R[7] * py + T.R[8] * pz + T.t[2];
}

// J^T J (packed upper triangle) and J^T r of one match: r = (fx (X/Z - u), fy (Y/Z - v)), X = R P + t, under T <- Exp(tau) T
__device__ __forceinline__ void accumulate(const Pose &T, double fx, double fy, double px, double py, double pz, double qu, double qv, double *S) {
    double X, Y, Z;
    transform(T, px, py, pz, X, Y, Z);
    const double iz = 1.0 / Z;
    const double rx = fx * (X * iz - qu), ry = fy * (Y * iz - qv);
    const double a = fx * iz, c = -fx * X * iz * iz, b = fy * iz, d = -fy * Y * iz * iz;
    const double Jx[6] = {a, 0.0, c, c * Y, a * Z - c * X, -a * Y};
    const double Jy[6] = {0.0, b, d, d * Y - b * Z, -d * X, b * X};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) S[k++] += Jx[i] * Jx[j] + Jy[i] * Jy[j];
#pragma unroll
    for (int i = 0; i < 6; i++) S[NA + i] += Jx[i] * rx + Jy[i] * ry;
}

// Solves (A + damping diag A) tau = -g by Cholesky and applies T <- Exp(tau) T.  false: a pivot is not > 0 or tau is not finite.
__device__ __forceinline__ bool solve_and_apply(const double *S, Pose &T) {
    double L[6][6];
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) { L[j][i] = S[k++]; }   // lower triangle holds A
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = L[j][j] * (1.0 + PNP_DAMPING);
#pragma unroll
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
        ok = ok && (s > 0.0);
        const double dd = sqrt(s > 0.0 ? s : 1.0);
        L[j][j] = dd;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
            L[i][j] = v / dd;
        }
    }
    double y[6], tau[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = -S[NA + i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * tau[k];
        tau[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && isfinite(tau[i]);
    if (!ok) return false;
    // Exp(tau): pose_utils' SE3_exp
    const double t0 = tau[3], t1 = tau[4], t2 = tau[5];
    const double ang = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    double A = 1.0, B = 0.5, C = 1.0 / 6.0;
    if (!(ang < PNP_SMALL_ANGLE)) {
        A = sin(ang) / ang;
        B = (1.0 - cos(ang)) / (ang * ang);
        C = (ang - sin(ang)) / (ang * ang * ang);
    }
    const double K[9] = {0.0, -t2, t1, t2, 0.0, -t0, -t1, t0, 0.0};
    double K2[9], E[9], V[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double e = (i % 4 == 0) ? 1.0 : 0.0;
        E[i] = e + A * K[i] + B * K2[i];
        V[i] = e + B * K[i] + C * K2[i];
    }
    Pose N;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) N.R[3 * i + j] = E[3 * i] * T.R[j] + E[3 * i + 1] * T.R[3 + j] + E[3 * i + 2] * T.R[6 + j];
        N.t[i] = (E[3 * i] * T.t[0] + E[3 * i + 1] * T.t[1] + E[3 * i + 2] * T.t[2]) + (V[3 * i] * tau[0] + V[3 * i + 1] * tau[1] + V[3 * i + 2] * tau[2]);
    }
    T = N;
    return true;
}

__device__ __forceinline__ bool is_inlier(const Pose &T, double fx, double fy, double thr2, double px, double py, double pz, double qu, double qv) {
    if (!(pz > 0.0)) return false;
    double X, Y, Z;
    transform(T, px, py, pz, X, Y, Z);
    if (!(Z > 0.0)) return false;
    const double ex = fx * (X / Z - qu), ey = fy * (Y / Z - qv);
    return ex * ex + ey * ey < thr2;   // (NaN: never)
}

__device__ __forceinline__ void write_state(const PnpParams &P, int status, int valid, int inliers, int hyp, int winner_count, int reason, const Pose &T) {
    // NOT sealed (device_utils.hpp: seal_host_block): the status goes last but with no fence in front of it, so it is the host's wait for the stream that
    // makes the block complete, not the tag.  Measured on the MI355X: volatile payload stores and the seal cost 10-19 us per call, the
    // seal's fence alone up to 9 us (24 500 matches: it writes back what the kernel left dirty) -- outside the call's run-to-run spread.
    int32_t *w = P.host_state;
    double *pose = reinterpret_cast<double *>(w + LVDGS_PNP_STATE_WORDS);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) pose[4 * i + j] = T.R[3 * i + j];
        pose[4 * i + 3] = T.t[i];
    }
    w[1] = valid; w[2] = inliers; w[3] = hyp; w[4] = winner_count; w[5] = reason; w[6] = 0; w[7] = 0;
    w[0] = status;
    __threadfence_system();
}

__global__ void __launch_bounds__(PNP_THREADS) pnp_hypotheses_kernel(PnpParams P) {
    __shared__ int s_last;
    __shared__ int s_int[PNP_WAVES];
    __shared__ int s_best_count[PNP_THREADS], s_best_h[PNP_THREADS];
    __shared__ int s_win[2];
    __shared__ double s_sum[PNP_WAVES][NS];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int h = blockIdx.x * PNP_WAVES + wave;
    const int M = P.M;
    if (h < P.hyp) {
        // ---- the sample: three distinct valid matches, every lane the same ----
        const uint32_t b = mix32(mix32(P.seed ^ 0x9e3779b9u) + (uint32_t)h);
        int s[3] = {-1, -1, -1};
        bool live = M > 0;
        for (int slot = 0; slot < 3 && live; slot++) {
            for (int d = 0; d < PNP_SAMPLE_DRAWS; d++) {
                const int idx = (int)(mix32(b + (uint32_t)(slot * PNP_SAMPLE_DRAWS + d)) % (uint32_t)M);
                if (P.pz[idx] > 0.0 && idx != s[0] && idx != s[1]) { s[slot] = idx; break; }
            }
            live = s[slot] >= 0;
        }
        Pose T;
        identity(T);
        if (live) {
            double sp[3][5];
            for (int k = 0; k < 3; k++) {
                sp[k][0] = P.px[s[k]]; sp[k][1] = P.py[s[k]]; sp[k][2] = P.pz[s[k]]; sp[k][3] = P.qu[s[k]]; sp[k][4] = P.qv[s[k]];
            }
            for (int it = 0; it < PNP_HYP_STEPS && live; it++) {
                double S[NS];
#pragma unroll
                for (int i = 0; i < NS; i++) S[i] = 0.0;
                for (int k = 0; k < 3; k++) accumulate(T, P.fx, P.fy, sp[k][0], sp[k][1], sp[k][2], sp[k][3], sp[k][4], S);
                live = solve_and_apply(S, T);
            }
            for (int k = 0; k < 3 && live; k++) {
                double X, Y, Z;
                transform(T, sp[k][0], sp[k][1], sp[k][2], X, Y, Z);
                live = Z > 0.0;
            }
        }
        // ---- the score ----
        int count = 0;
        if (live) {
            for (int i = lane; i < M; i += WAVE)
                count += is_inlier(T, P.fx, P.fy, P.thr2, P.px[i], P.py[i], P.pz[i], P.qu[i], P.qv[i]) ? 1 : 0;
            count = wave_sum(count);
        }
        if (lane == 0) {
            HypRec &r = P.recs[h];
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) r.pose[4 * i + j] = T.R[3 * i + j];
                r.pose[4 * i + 3] = T.t[i];
            }
            r.count = live ? count : -1;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // publish the records (release, agent scope), then draw a ticket
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

    // ---- the last workgroup: valid count, winner, refinement ----
    const int tid = threadIdx.x;
    int nv = 0;
    for (int i = tid; i < M; i += PNP_THREADS) nv += P.pz[i] > 0.0 ? 1 : 0;
    const int valid = block_sum<PNP_WAVES>(nv, s_int);
    int bc = -1, bh = -1;
    for (int k = tid; k < P.hyp; k += PNP_THREADS) {
        const int c = P.recs[k].count;
        if (c > bc) { bc = c; bh = k; }
    }
    s_best_count[tid] = bc; s_best_h[tid] = bh;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < PNP_THREADS; k++)
            if (s_best_count[k] > bc || (s_best_count[k] == bc && s_best_h[k] >= 0 && s_best_h[k] < bh)) { bc = s_best_count[k]; bh = s_best_h[k]; }
        s_win[0] = bc; s_win[1] = bh;
    }
    __syncthreads();
    const int win_count = s_win[0], win = s_win[1];
    Pose T;
    identity(T);
    int reason = LVDGS_PNP_FAIL_NONE;
    if (valid < PNP_MIN_VALID) reason = LVDGS_PNP_FAIL_FEW_VALID;
    else if (win < 0) reason = LVDGS_PNP_FAIL_ALL_VOID;
    else if (win_count < P.min_inliers) reason = LVDGS_PNP_FAIL_FEW_INLIERS;
    if (reason != LVDGS_PNP_FAIL_NONE) {   // uniform over the workgroup
        if (tid == 0) write_state(P, LVDGS_PNP_FAILED, valid, 0, valid < PNP_MIN_VALID ? -1 : win, win < 0 || valid < PNP_MIN_VALID ? 0 : win_count, reason, T);
        return;
    }
    {
        const double *wp = P.recs[win].pose;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T.R[3 * i + j] = wp[4 * i + j];
            T.t[i] = wp[4 * i + 3];
        }
    }
    bool ok = true;
    for (int round = 0; round < PNP_REFINE_ROUNDS && ok; round++) {
        // a thread keeps the flags of its own matches in the mask: no other thread reads them
        for (int i = tid; i < M; i += PNP_THREADS)
            P.mask[i] = is_inlier(T, P.fx, P.fy, P.thr2, P.px[i], P.py[i], P.pz[i], P.qu[i], P.qv[i]) ? 1 : 0;
        for (int it = 0; it < PNP_REFINE_STEPS && ok; it++) {
            double S[NS];
#pragma unroll
            for (int i = 0; i < NS; i++) S[i] = 0.0;
            for (int i = tid; i < M; i += PNP_THREADS)
                if (P.mask[i]) accumulate(T, P.fx, P.fy, P.px[i], P.py[i], P.pz[i], P.qu[i], P.qv[i], S);
#pragma unroll
            for (int i = 0; i < NS; i++) S[i] = wave_sum(S[i]);
            __syncthreads();
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < NS; i++) s_sum[wave][i] = S[i];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NS; i++) {
                double v = s_sum[0][i];
                for (int w = 1; w < PNP_WAVES; w++) v += s_sum[w][i];
                S[i] = v;
            }
            ok = solve_and_apply(S, T);   // the same numbers in every thread: the same pose, the same verdict
        }
    }
    if (!ok) {
        for (int i = tid; i < M; i += PNP_THREADS) P.mask[i] = 0;
        identity(T);
        if (tid == 0) write_state(P, LVDGS_PNP_FAILED, valid, 0, win, win_count, LVDGS_PNP_FAIL_SINGULAR, T);
        return;
    }
    int ni = 0;
    for (int i = tid; i < M; i += PNP_THREADS) {
        const bool in = is_inlier(T, P.fx, P.fy, P.thr2, P.px[i], P.py[i], P.pz[i], P.qu[i], P.qv[i]);
        P.mask[i] = in ? 1 : 0;
        ni += in ? 1 : 0;
    }
    const int inliers = block_sum<PNP_WAVES>(ni, s_int);
    if (tid == 0) write_state(P, LVDGS_PNP_OK, valid, inliers, win, win_count, LVDGS_PNP_FAIL_NONE, T);
}

// the scratch: the header, five columns of a double per match, a record per hypothesis
size_t pnp_layout(int num_matches, int hypotheses, PnpParams *P, void *base) {
    Carver<PnpParams> c(P, base);
    const size_t m = num_matches > 0 ? (size_t)num_matches : 0, h = hypotheses > 0 ? (size_t)hypotheses : 0;
    c(c.v.hdr, 1);
    c(c.v.px, m); c(c.v.py, m); c(c.v.pz, m); c(c.v.qu, m); c(c.v.qv, m);
    c(c.v.recs, h);
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_pnp_scratch_bytes(int32_t num_matches, int32_t hypotheses) { return pnp_layout(num_matches, hypotheses, nullptr, nullptr); }

int lvdgs_pnp_ransac(const lvdgs_pnp_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("pnp: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width <= 0 || a->height <= 0 || (int64_t)a->width * a->height > INT32_MAX) {
        set_error("pnp: bad raster size %dx%d", a->width, a->height); return LVDGS_E_INVALID;
    }
    if (a->num_matches < 0) { set_error("pnp: num_matches < 0"); return LVDGS_E_INVALID; }
    if (a->hypotheses <= 0 || a->hypotheses > LVDGS_PNP_MAX_HYPOTHESES) {
        set_error("pnp: hypotheses %d outside 1..%d", a->hypotheses, LVDGS_PNP_MAX_HYPOTHESES); return LVDGS_E_INVALID;
    }
    if (!(a->reproj_error > 0.0) || !(a->fx > 0.0) || !(a->fy > 0.0)) { set_error("pnp: reproj_error, fx and fy must be positive"); return LVDGS_E_INVALID; }
    if (!a->depth || !a->inlier_mask || !a->host_state || !a->scratch || (a->num_matches > 0 && (!a->matches_im1 || !a->matches_im2))) {
        set_error("pnp: depth / matches_im1 / matches_im2 / inlier_mask / host_state / scratch is NULL"); return LVDGS_E_INVALID;
    }
    PnpParams P{};
    if (a->scratch_bytes < pnp_layout(a->num_matches, a->hypotheses, &P, a->scratch)) { set_error("pnp: scratch too small"); return LVDGS_E_INVALID; }
    P.W = a->width; P.H = a->height; P.M = a->num_matches; P.hyp = a->hypotheses; P.min_inliers = a->min_inliers;
    P.seed = a->seed;
    P.fx = a->fx; P.fy = a->fy; P.cx = a->cx; P.cy = a->cy;
    P.k1 = a->dist[0]; P.k2 = a->dist[1]; P.p1 = a->dist[2]; P.p2 = a->dist[3]; P.k3 = a->dist[4];
    P.thr2 = a->reproj_error * a->reproj_error;
    P.depth = a->depth; P.m1 = a->matches_im1; P.m2 = a->matches_im2; P.mask = a->inlier_mask;
    if (int e = host_block_address(a->host_state, "pnp", &P.host_state)) return e;
    if (int e = launch("pnp_gather", 0, s, pnp_gather_kernel, dim3(cdiv(P.M > 0 ? P.M : 1, PNP_THREADS)), dim3(PNP_THREADS), 0, P)) return e;
    if (int e = launch("pnp_hypotheses", 0, s, pnp_hypotheses_kernel, dim3(cdiv(P.hyp, PNP_WAVES)), dim3(PNP_THREADS), 0, P)) return e;
    return LVDGS_OK;
}

}  // extern "C"
