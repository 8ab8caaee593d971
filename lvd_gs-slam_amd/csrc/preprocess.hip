// Per-Gaussian kernels of the forward: projection, frustum test.  (The backward: preprocess_bwd.hip; the arithmetic both share:
// projection.hpp.)  One lane per Gaussian, wave64, 256-thread workgroups.  These are HBM-streaming kernels: the projection reads
// 56 B and writes 60 B per Gaussian.  Compiled with -ffp-contract=off: the float expressions that decide integers (radius, tile
// rectangle, depth sort key) are evaluated as written.
#include "common.hpp"
#include "binning.hpp"
#include "device_utils.hpp"
#include "projection.hpp"

namespace lvdgs {

namespace {

struct FwdParams {
    Cam cam;
    int N, act;
    int tile_cull;         // 0: list every tile of the rectangle (the reference's pair list)
    int row_begin, row_end; // tile rows that are rendered (lvdgs_args.tile_row_begin / _end): pairs outside are not listed
    const float *means3D, *opacities, *scales, *rotations, *cov3D_precomp, *shs, *colors_precomp;
    float *rec;
    uint32_t *tiles_touched, *depth_bits;
    uint4 *rect;
    int32_t *radii;
    uint32_t *blocksums;   // per workgroup: sum of tiles_touched (first level of the slot scan, sortscan.hip)
    // two-level grouping (LVDGS_FLAG_SUPER_TILES; preprocess_count_kernel<..., true>): the super-tile grid's rectangles, count matrix, queue counters
    uint4 *super_rect; uint32_t *super_hist, *super_queue_counts; int super_gx, super_T;
};

// What the projection reads of one Gaussian whatever becomes of it, requested in ONE round of loads (position, then --
// only if in front of the camera -- scale and rotation, then -- only if on the image -- opacity and colour were three
// dependent round trips, each of them exposed: the kernels below run as a single resident round of workgroups, every
// wave in the same phase).  Gaussians that turn out culled have 44 bytes read for nothing.
struct RawGaussian {
    float pos[3], sc[3], q[4], opac, col[3];   // raw (not activated) values; col: colors_precomp or the SH DC coefficients
};
__device__ __forceinline__ RawGaussian load_raw(const FwdParams &p, int i) {
    RawGaussian r;
#pragma unroll
    for (int k = 0; k < 3; k++) r.pos[k] = p.means3D[3 * (size_t)i + k];
    if (!p.cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 3; k++) r.sc[k] = p.scales[3 * (size_t)i + k];
#pragma unroll
        for (int k = 0; k < 4; k++) r.q[k] = p.rotations[4 * (size_t)i + k];
    } else {
        r.sc[0] = r.sc[1] = r.sc[2] = 0.f; r.q[0] = 1.f; r.q[1] = r.q[2] = r.q[3] = 0.f;
    }
    r.opac = p.opacities[i];
    const float *col = p.colors_precomp ? p.colors_precomp + 3 * (size_t)i : p.shs + (size_t)i * p.cam.M * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) r.col[k] = col[k];
    return r;
}
__device__ __forceinline__ void preprocess_one(const FwdParams &p, int i, const RawGaussian &raw, uint32_t &tiles_out, uint4 &rect_out);

__global__ void __launch_bounds__(256) preprocess_fwd_kernel(FwdParams p) {
    __shared__ uint32_t s_sum[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t tiles = 0;
    uint4 rect;
    if (i < p.N) preprocess_one(p, i, load_raw(p, i), tiles, rect);
    // the workgroup's pair count: the slot scan starts from these sums instead of re-reading tiles_touched in a launch of its own
    tiles = wave_sum(tiles);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = tiles;
    __syncthreads();
    if (threadIdx.x == 0) p.blocksums[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// The projection that also counts: a workgroup owns the chunk of GROUP_THREADS x PER consecutive Gaussians the grouping kernels
// (binning.hip) work in, keeps the per-tile pair counters of that chunk in LDS while it projects, and leaves the chunk's
// row of the [chunk][tile] count matrix and the chunk's pair total -- the grouping's first kernel and its re-read of
// every rectangle are gone from the single-call forward (lvdgs_forward).  Also clears what the later kernels of the
// frame accumulate into (n_touched, the tile-sort queue counters).
// SUPER_COUNT (two-level grouping, binning.hip): the chunk's row of the SUPER-TILE grid's count matrix and the Gaussians' super
// rectangles are made here too -- a second set of LDS counters behind the tiles', a second walk over (far fewer) cells -- instead of
// by a kernel of their own that re-reads every rectangle (17 us on the opaque-surface workload).  A template parameter: the default
// instantiation is the kernel it was.
template <int GROUP_THREADS, int OWNERS, int PER, bool SUPER_COUNT = false>
__device__ __forceinline__ void preprocess_count_body(const FwdParams &p, int T, uint32_t *__restrict__ hist,
                                                      uint32_t *__restrict__ chunk_sums, int32_t *__restrict__ n_touched,
                                                      uint32_t *__restrict__ queue_counts) {
    constexpr bool HELPERS = GROUP_THREADS > OWNERS;   // waves without a Gaussian of their own: they help with the large rectangles (binning.hpp)
    static_assert(!HELPERS || PER == 1, "helper waves: one Gaussian per owner thread");
    extern __shared__ uint32_t s_tile[];
    __shared__ uint32_t s_sum[GROUP_THREADS / 64];
    __shared__ BigRectQueue s_big;
    const bool owner = (int)threadIdx.x < OWNERS;
    // the first Gaussian's values are on their way while the counters are cleared
    const int i_first = blockIdx.x * (OWNERS * PER) + (int)threadIdx.x;
    RawGaussian raw{};
    if (owner && i_first < p.N) raw = load_raw(p, i_first);
    const int T_all = SUPER_COUNT ? T + p.super_T : T;   // (the super-tile counters lie behind the tiles')
    uint32_t *s_super = s_tile + T;
    for (int t = threadIdx.x; t < T_all; t += GROUP_THREADS) s_tile[t] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        queue_counts[threadIdx.x] = 0u;
        if constexpr (SUPER_COUNT) p.super_queue_counts[threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0) s_big.count = 0u;
    __syncthreads();
    uint32_t mine = 0;
#pragma unroll 1
    for (int k = 0; k < PER; k++) {
        const int i = blockIdx.x * (OWNERS * PER) + k * OWNERS + (int)threadIdx.x;
        uint32_t tiles = 0;
        uint4 rect = make_uint4(0u, 0u, 0u, 0u);
        if (owner && i < p.N) {
            if (k > 0) raw = load_raw(p, i);
            preprocess_one(p, i, raw, tiles, rect);
            n_touched[i] = 0;
        }
        mine += tiles;
        if constexpr (HELPERS) for_each_pair_of_rect_wg(rect, i, p.cam.gx, 0u, s_big, [&](int tile, uint32_t, uint32_t) { atomicAdd(&s_tile[tile], 1u); });
        else for_each_pair_of_rect(rect, i, p.cam.gx, 0u, [&](int tile, uint32_t, uint32_t) { atomicAdd(&s_tile[tile], 1u); });
        if constexpr (SUPER_COUNT) {
            const uint4 rs = super_rect_of(rect);
            if (owner && i < p.N) p.super_rect[i] = rs;
            if constexpr (HELPERS) {
                __syncthreads();                         // (every wave is done with the queue of the tile walk)
                if (threadIdx.x == 0) s_big.count = 0u;
                __syncthreads();
                for_each_pair_of_rect_wg(rs, i, p.super_gx, 0u, s_big, [&](int cell, uint32_t, uint32_t) { atomicAdd(&s_super[cell], 1u); });
            } else {
                for_each_pair_of_rect(rs, i, p.super_gx, 0u, [&](int cell, uint32_t, uint32_t) { atomicAdd(&s_super[cell], 1u); });
            }
        }
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < GROUP_THREADS / 64; w++) total += s_sum[w];
        chunk_sums[blockIdx.x] = total;
    }
    uint32_t *row = hist + (size_t)blockIdx.x * T;
    for (int t = threadIdx.x; t < T; t += GROUP_THREADS) row[t] = s_tile[t];
    if constexpr (SUPER_COUNT) {
        uint32_t *row_s = p.super_hist + (size_t)blockIdx.x * p.super_T;
        for (int t = threadIdx.x; t < p.super_T; t += GROUP_THREADS) row_s[t] = s_super[t];
    }
}

template <int GROUP_THREADS, int OWNERS, int PER, bool SUPER_COUNT = false>
__global__ void __launch_bounds__(GROUP_THREADS, 8) preprocess_count_kernel(FwdParams p, int T, uint32_t *__restrict__ hist,
                                                                        uint32_t *__restrict__ chunk_sums, int32_t *__restrict__ n_touched,
                                                                        uint32_t *__restrict__ queue_counts) {
    preprocess_count_body<GROUP_THREADS, OWNERS, PER, SUPER_COUNT>(p, T, hist, chunk_sums, n_touched, queue_counts);
}
// The views of a mapping window in ONE launch (lvdgs_forward_batch; blockIdx.y: the view -- same map, same image size, a camera,
// state buffers and count matrix each).  A KITTI-size frame's projection is 391 workgroups of latency-bound work on 256 CUs: ten
// of them side by side cost little more than one.
struct PrepCountView { FwdParams p; uint32_t *hist, *chunk_sums; int32_t *n_touched; uint32_t *queue_counts; };
struct PrepCountBatch { PrepCountView v[FWD_BATCH_VIEWS]; };
static_assert(sizeof(PrepCountBatch) <= 4064, "kernel arguments");
template <int GROUP_THREADS, int OWNERS, int PER, bool SUPER_COUNT = false>
__global__ void __launch_bounds__(GROUP_THREADS, 8) preprocess_count_batch_kernel(PrepCountBatch b, int T) {
    const PrepCountView &v = b.v[blockIdx.y];
    preprocess_count_body<GROUP_THREADS, OWNERS, PER, SUPER_COUNT>(v.p, T, v.hist, v.chunk_sums, v.n_touched, v.queue_counts);
}

__device__ __forceinline__ void preprocess_one(const FwdParams &p, int i, const RawGaussian &raw, uint32_t &tiles_out, uint4 &rect_out) {
    const Cam &c = p.cam;
    // culled unless proven visible
    int radius = 0;
    uint32_t tiles = 0;
    uint4 rect = make_uint4(0u, 0u, 0u, 0u);
    uint32_t depth_bits = 0u;
    const float pos[3] = {raw.pos[0], raw.pos[1], raw.pos[2]};
    float pv[3];
    xform3(pos, c.view, pv);
    if (pv[2] > NEAR_CULL) {
        float ph[3];
        xform3(pos, c.proj, ph);
        const float phw = xform_w(pos, c.proj);
        const float pw = 1.f / (phw + HOMOG_EPS);
        const float ndcx = ph[0] * pw, ndcy = ph[1] * pw;
        float c6[6];
        if (p.cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) c6[k] = p.cov3D_precomp[6 * (size_t)i + k];
        } else {
            float s[3] = {raw.sc[0], raw.sc[1], raw.sc[2]}, q[4] = {raw.q[0], raw.q[1], raw.q[2], raw.q[3]}, qn;
            activate_scale_rot(p.act, s, q, qn);
            cov3d_of(s, c.scale_mod, q, c6);
        }
        Ewa e;
        ewa_setup(pv, c.view, c, e);
        float ca, cb, cc;
        cov2d_of(e, c6, ca, cb, cc);
        const float det = ca * cc - cb * cb;
        if (det != 0.f) {
            const float det_inv = 1.f / det;
            const float k0 = cc * det_inv, k1 = -cb * det_inv, k2 = ca * det_inv;
            const float mid = 0.5f * (ca + cc);
            float disc = mid * mid - det;
            if (disc < LAMBDA_FLOOR) disc = LAMBDA_FLOOR;
            const float l1 = mid + sqrtf(disc), l2 = mid - sqrtf(disc);
            const float lmax = l1 > l2 ? l1 : l2;
            const int rad = (int)ceilf(3.f * sqrtf(lmax));
            const float px = ((ndcx + 1.f) * (float)c.W - 1.f) * 0.5f;
            const float py = ((ndcy + 1.f) * (float)c.H - 1.f) * 0.5f;
            int x0 = (int)((px - (float)rad) / (float)TILE), y0 = (int)((py - (float)rad) / (float)TILE);
            int x1 = (int)((px + (float)rad + (float)(TILE - 1)) / (float)TILE);
            int y1 = (int)((py + (float)rad + (float)(TILE - 1)) / (float)TILE);
            x0 = min(c.gx, max(0, x0)); x1 = min(c.gx, max(0, x1));
            y0 = min(c.gy, max(0, y0)); y1 = min(c.gy, max(0, y1));
            // (a Gaussian is visible -- radius > 0, record written -- when its rectangle meets the IMAGE; which of its tiles
            // are listed is then a matter of the band being rendered and of the tile culling)
            const bool on_image = (x1 - x0) * (y1 - y0) > 0;
            y0 = min(p.row_end, max(p.row_begin, y0)); y1 = min(p.row_end, max(p.row_begin, y1));
            const int area = (x1 - x0) * (y1 - y0);
            if (on_image) {
                float rgb[3];
                if (p.colors_precomp) {
                    rgb[0] = raw.col[0]; rgb[1] = raw.col[1]; rgb[2] = raw.col[2];
                } else {
                    float d[3] = {pos[0] - c.campos[0], pos[1] - c.campos[1], pos[2] - c.campos[2]};
                    const float inv = 1.f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    d[0] *= inv; d[1] *= inv; d[2] *= inv;
                    float B[16];
                    sh_basis(c.sh_degree, d, B);
                    const int nb = (c.sh_degree + 1) * (c.sh_degree + 1);
                    const float *sh = p.shs + (size_t)i * c.M * 3;
                    rgb[0] = 0.f + B[0] * raw.col[0]; rgb[1] = 0.f + B[0] * raw.col[1]; rgb[2] = 0.f + B[0] * raw.col[2];
#pragma unroll
                    for (int k = 1; k < 16; k++)
                        if (k < nb) {
                            rgb[0] += B[k] * sh[3 * k]; rgb[1] += B[k] * sh[3 * k + 1]; rgb[2] += B[k] * sh[3 * k + 2];
                        }
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) { rgb[ch] += 0.5f; rgb[ch] = rgb[ch] < 0.f ? 0.f : rgb[ch]; }
                }
                float opac = raw.opac;
                if (p.act & ACT_SIGMOID_OPACITY) opac = 1.f / (1.f + expf(-opac));
                // the tiles of the rectangle the Gaussian can reach with alpha >= 1/255 (common.hpp: rect_keeps)
                uint64_t mask = ~0ull;
                radius = rad; tiles = (uint32_t)area;
                if (area == 0) { x0 = x1 = y0 = y1 = 0; mask = 0ull; }   // not in this band
                else if (p.tile_cull) {
                    const float far_x = fmaxf(fabsf(px - (float)(x0 * TILE)), fabsf(px - (float)(x1 * TILE - 1)));
                    const float far_y = fmaxf(fabsf(py - (float)(y0 * TILE)), fabsf(py - (float)(y1 * TILE - 1)));
                    const TileReach reach(px, py, k0, k1, k2, opac, far_x, far_y);
                    mask = 0ull;
                    if (area <= RECT_MASK_TILES) {
                        uint64_t bit = 1ull;
                        for (int y = y0; y < y1; y++)
                            for (int x = x0; x < x1; x++) {
                                if (reach.tile((float)(x * TILE), (float)(y * TILE))) mask |= bit;
                                bit <<= 1;
                            }
                        tiles = (uint32_t)__popcll(mask);
                    } else {
                        // one bit per block of tiles (common.hpp: RectBlocks): the same test on the block's pixel rectangle
                        const RectBlocks g(x1 - x0, y1 - y0);
                        tiles = 0;
                        for (int b = 0; b < 64; b++) {
                            const int bwid = g.width(b), bhei = g.height(b);
                            if (bwid <= 0 || bhei <= 0) continue;
                            const int tx = x0 + (b & 7) * g.bw, ty = y0 + (b >> 3) * g.bh;
                            if (reach.rect((float)(tx * TILE), (float)(ty * TILE), (float)(bwid * TILE - 1), (float)(bhei * TILE - 1))) {
                                mask |= 1ull << b;
                                tiles += (uint32_t)(bwid * bhei);
                            }
                        }
                    }
                } else if (area > RECT_MASK_TILES) {
                    // every tile listed: all blocks that exist are kept
                    const RectBlocks g(x1 - x0, y1 - y0);
                    mask = 0ull;
                    for (int b = 0; b < 64; b++)
                        if (g.width(b) > 0 && g.height(b) > 0) mask |= 1ull << b;
                }
                rect = make_uint4((uint32_t)x0 | ((uint32_t)x1 << 16), (uint32_t)y0 | ((uint32_t)y1 << 16), (uint32_t)mask, (uint32_t)(mask >> 32));
                depth_bits = __float_as_uint(pv[2]);
                float4 *r4 = reinterpret_cast<float4 *>(p.rec + (size_t)i * REC_FLOATS);
                r4[0] = make_float4(px, py, k0, k1);
                if constexpr (REC_FLOATS >= 16) r4[3] = make_float4(__uint_as_float(rect.x), __uint_as_float(rect.y), __uint_as_float(rect.z), __uint_as_float(rect.w));
                r4[1] = make_float4(k2, opac, rgb[0], rgb[1]);
                r4[2] = make_float4(rgb[2], pv[2], 0.f, __int_as_float(rad));
            }
        }
    }
    p.radii[i] = radius;
    p.tiles_touched[i] = tiles;
    p.rect[i] = rect;
    p.depth_bits[i] = depth_bits;
    tiles_out = tiles;
    rect_out = rect;
}

__global__ void __launch_bounds__(256) mark_visible_kernel(int N, const float *means3D, const float *view, uint8_t *present) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float pos[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
    float pv[3];
    xform3(pos, view, pv);
    present[i] = pv[2] > NEAR_CULL;
}

}  // namespace

static FwdParams make_fwd_params(const lvdgs_args &a, const GeomView &g) {
    FwdParams p;
    p.blocksums = nullptr;
    p.super_rect = nullptr; p.super_hist = p.super_queue_counts = nullptr; p.super_gx = p.super_T = 0;
    p.cam = make_cam(a); p.N = a.num_gaussians; p.act = a.activations;
    p.tile_cull = !(a.flags & LVDGS_FLAG_LIST_ALL_TILES);
    tile_row_band(a, &p.row_begin, &p.row_end);
    p.means3D = a.means3D; p.opacities = a.opacities; p.scales = a.scales; p.rotations = a.rotations;
    p.cov3D_precomp = a.cov3D_precomp; p.shs = a.shs; p.colors_precomp = a.colors_precomp;
    p.rec = g.rec; p.tiles_touched = g.tiles_touched; p.depth_bits = g.depth_bits; p.rect = g.rect; p.radii = a.radii;
    return p;
}

int launch_preprocess_fwd(const lvdgs_args &a, const GeomView &g, uint32_t *blocksums, hipStream_t s) {
    if (a.num_gaussians == 0) return LVDGS_OK;
    FwdParams p = make_fwd_params(a, g);
    p.blocksums = blocksums;
    if (int e = launch("preprocess_fwd", a.debug, s, preprocess_fwd_kernel, dim3(cdiv(p.N, 256)), dim3(256), 0, p)) return e;
    return LVDGS_OK;
}

// two-level grouping: the super-tile grid is counted by the projection kernel too (launch_super_count is for the two-call API)
static void count_super_tiles_too(FwdParams &p, const lvdgs_args &a, const RenderScratch &w) {
    p.super_rect = w.super.rect; p.super_hist = w.super.hist; p.super_queue_counts = w.super.long_count;
    p.super_gx = cdiv(p.cam.gx, SUPER); p.super_T = super_tiles_of(a.image_width, a.image_height);
}

// A counting kernel's launch: its dynamic LDS (the tiles' counters, SUPER: the super tiles' behind them) allowed once per kernel (done).
template <bool SUPER_COUNT, class... Params, class... Args>
static int launch_count_kernel(const char *name, int debug, void (*kernel)(Params...), unsigned char (&done)[16], dim3 grid, int threads, size_t lds, hipStream_t s,
                               Args... args) {
    constexpr int LDS_MAX = (SUPER_COUNT ? GROUP_MAX_TILES + GROUP_MAX_TILES / (SUPER * SUPER) + 64 : GROUP_MAX_TILES) * 4;
    if (int e = allow_dynamic_lds(reinterpret_cast<const void *>(kernel), LDS_MAX, done)) return e;
    return launch_checked(name, debug, s, kernel, grid, dim3(threads), lds, args...);
}

int launch_preprocess_count(const lvdgs_args &a, const GeomView &g, const ImageView &im, const RenderScratch &w, hipStream_t s) {
    const int N = a.num_gaussians;
    if (N == 0) return LVDGS_OK;
    FwdParams p = make_fwd_params(a, g);
    const int T = p.cam.gx * p.cam.gy;
    const int nchunks = (int)group_chunks(N);
    const bool super = super_tiles_in_use(a);
    if (super) count_super_tiles_too(p, a, w);
    const size_t lds = (size_t)(T + (super ? p.super_T : 0)) * sizeof(uint32_t);
    static unsigned char done[2 * GROUP_SHAPES][16];
    ProfScope ps("preprocess_fwd", s);
    if (int e = group_dispatch(group_shape_for(N), [&](auto threads_, auto owners_, auto per_, int d) {
            constexpr int THREADS = decltype(threads_)::value, OWNERS = decltype(owners_)::value, PER = decltype(per_)::value;
            if (super) return launch_count_kernel<true>("preprocess_count", a.debug, preprocess_count_kernel<THREADS, OWNERS, PER, true>, done[GROUP_SHAPES + d], dim3(nchunks),
                                                        THREADS, lds, s, p, T, w.group_hist, w.chunk_sums, a.n_touched, im.long_count);
            return launch_count_kernel<false>("preprocess_count", a.debug, preprocess_count_kernel<THREADS, OWNERS, PER>, done[d], dim3(nchunks), THREADS, lds, s,
                                              p, T, w.group_hist, w.chunk_sums, a.n_touched, im.long_count);
        })) return e;
    return LVDGS_OK;
}

// n views of one map and one image size (lvdgs_forward_batch)
int launch_preprocess_count_batch(const lvdgs_args *const *a, const GeomView *g, const ImageView *im, const RenderScratch *w, int n, hipStream_t s) {
    const int N = a[0]->num_gaussians;
    if (N == 0 || n == 0) return LVDGS_OK;
    if (n > FWD_BATCH_VIEWS) { set_error("internal: more than %d views in one forward batch", FWD_BATCH_VIEWS); return LVDGS_E_INVALID; }
    PrepCountBatch batch{};
    const bool super = super_tiles_in_use(*a[0]);
    for (int k = 0; k < n; k++) {
        batch.v[k] = PrepCountView{make_fwd_params(*a[k], g[k]), w[k].group_hist, w[k].chunk_sums, a[k]->n_touched, im[k].long_count};
        if (super) count_super_tiles_too(batch.v[k].p, *a[k], w[k]);
    }
    const int T = batch.v[0].p.cam.gx * batch.v[0].p.cam.gy;
    const int nchunks = (int)group_chunks(N);
    const size_t lds = (size_t)(T + (super ? batch.v[0].p.super_T : 0)) * sizeof(uint32_t);
    static unsigned char done[2 * GROUP_SHAPES][16];
    ProfScope ps("preprocess_fwd", s);
    if (int e = group_dispatch(group_shape_for(N), [&](auto threads_, auto owners_, auto per_, int d) {
            constexpr int THREADS = decltype(threads_)::value, OWNERS = decltype(owners_)::value, PER = decltype(per_)::value;
            const char *name = "preprocess_count (batch)";
            if (super) return launch_count_kernel<true>(name, a[0]->debug, preprocess_count_batch_kernel<THREADS, OWNERS, PER, true>, done[GROUP_SHAPES + d], dim3(nchunks, n), THREADS, lds, s, batch, T);
            return launch_count_kernel<false>(name, a[0]->debug, preprocess_count_batch_kernel<THREADS, OWNERS, PER>, done[d], dim3(nchunks, n), THREADS, lds, s, batch, T);
        })) return e;
    return LVDGS_OK;
}

int launch_mark_visible(int N, const float *means3D, const float *view, uint8_t *present, hipStream_t s) {
    if (N == 0) return LVDGS_OK;
    if (int e = launch("mark_visible", 0, s, mark_visible_kernel, dim3(cdiv(N, 256)), dim3(256), 0, N, means3D, view, present)) return e;
    return LVDGS_OK;
}

}  // namespace lvdgs
