// The block-sparse TSDF volume: blocks of 8 x 8 x 8 samples in a pool, found through an open-addressing table of 64-bit keys
// (storage, rules and the host block: include/lvdgs.h, "Block-sparse TSDF volume").  The fusion rule with its walk over
// the views, the surface-nets decisions and the host's checks of planes, constants and views are tsdf_rule.hpp's, shared with the dense
// volume (tsdf.hip); this file is the blocks' storage around them: keys, table, pool, the 9^3 tile and the neighbours of a block.
//
// lvdgs_tsdf_blocks_integrate: three launches.  Allocation -- a thread per pixel walks its ray's band in half-voxel steps and enters
// the blocks it meets (one 64-bit atomicCAS per new key decides who enters it; the winner draws the pool index); one thread brings
// the block counter back under the pool size; then a workgroup per block in use fuses the views as the dense kernel does for a brick.
//
// lvdgs_tsdf_blocks_mesh: eight launches over the blocks in key order (`order`).  Everything a launch reads from the header, from
// `order`, from the table or from an earlier launch's scratch is brought into range before it indexes: garbage gives a wrong mesh,
// never an access outside the caller's arrays.  Integer decisions only, no atomics: two calls give the same bytes.
#include "common.hpp"
#include "device_utils.hpp"
#include "spans.hpp"
#include "tsdf_rule.hpp"

namespace lvdgs {
namespace {

constexpr int TB_THREADS = 256;          // a block's 512 samples: two per thread, l and l + 256
constexpr int TB_SCAN_THREADS = 1024;    // the one workgroup that scans the per-block counts
constexpr int BLOCK_SAMPLES = 512;
constexpr int TB_MAX_GRID = 65536;       // workgroups of the per-block launches (they stride over the blocks)
constexpr int COORD_BIAS = 1 << 20;
constexpr unsigned long long KEY_BIT = 1ull << 63;

struct BlockVolume {
    int pool, slots;
    TsdfLattice lat;
    float *tsdf, *weight, *r, *g, *b;
    unsigned long long *block_key, *keys;
    int32_t *values, *header;
};

__host__ __device__ inline unsigned long long pack_key(int bx, int by, int bz) {
    return KEY_BIT | (unsigned long long)(bz + COORD_BIAS) << 42 | (unsigned long long)(by + COORD_BIAS) << 21 | (unsigned long long)(bx + COORD_BIAS);
}
__device__ __forceinline__ void unpack_key(unsigned long long key, int &bx, int &by, int &bz) {
    bx = (int)(key & 0x1FFFFFu) - COORD_BIAS;
    by = (int)((key >> 21) & 0x1FFFFFu) - COORD_BIAS;
    bz = (int)((key >> 42) & 0x1FFFFFu) - COORD_BIAS;
}
// MurmurHash3's 64-bit finalizer, into the table
__device__ __forceinline__ uint32_t first_slot(unsigned long long k, uint32_t mask) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & mask;
}
// the blocks in use, in 0 .. pool whatever the header holds
__device__ __forceinline__ int used_blocks(const BlockVolume &v) {
    const int u = v.header[LVDGS_TSDF_BLOCKS_HEADER_USED];
    return u < 0 ? 0 : u > v.pool ? v.pool : u;
}

// Enter `key`.  won: this thread's atomicCAS put it there; *slot_out: where.  false when every slot is taken by other keys.
__device__ __forceinline__ bool enter_key(const BlockVolume &v, unsigned long long key, bool *won, uint32_t *slot_out) {
    const uint32_t mask = (uint32_t)v.slots - 1u;
    uint32_t slot = first_slot(key, mask);
    *won = false;
    for (uint32_t n = 0; n <= mask; n++, slot = (slot + 1u) & mask) {
        unsigned long long k = __hip_atomic_load(&v.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a slot's key is written once)
        if (k == 0ull) {
            k = atomicCAS(&v.keys[slot], 0ull, key);
            if (k == 0ull) { *won = true; *slot_out = slot; return true; }
        }
        if (k == key) { *slot_out = slot; return true; }
    }
    return false;
}

// The pool index of `key`, -1 when it is absent, dropped, or what the table holds is no block in use.
__device__ __forceinline__ int find_block(const BlockVolume &v, unsigned long long key, int used) {
    const uint32_t mask = (uint32_t)v.slots - 1u;
    uint32_t slot = first_slot(key, mask);
    for (uint32_t n = 0; n <= mask; n++, slot = (slot + 1u) & mask) {
        const unsigned long long k = v.keys[slot];
        if (k == key) {
            const int at = v.values[slot];
            return at >= 0 && at < used ? at : -1;
        }
        if (k == 0ull) return -1;
    }
    return -1;
}

// ---------------------------------------------------------------- allocation ----

struct AllocParams {
    BlockVolume vol;
    int n_steps;
    float step;
    TsdfView v[LVDGS_TSDF_MAX_VIEWS];
};

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_alloc_kernel(AllocParams p) {
    const TsdfView &V = p.v[blockIdx.y];
    const int64_t pixels = (int64_t)V.W * V.H, pixel = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
    if (pixel >= pixels) return;
    const float d = V.depth[pixel];
    if (!(d > 0.f && d <= V.dtrunc)) return;
    if (V.mask && V.mask[pixel] == 0) return;
    float R[9], T[3];
#pragma unroll
    for (int q = 0; q < 9; q++) R[q] = V.R[q];
#pragma unroll
    for (int q = 0; q < 3; q++) T[q] = V.T[q];
    const int vi = (int)(pixel / V.W), ui = (int)(pixel - (int64_t)vi * V.W);
    const float xn = ((float)ui - V.cx) / V.fx, yn = ((float)vi - V.cy) / V.fy;
    const float z0 = d - (float)(p.n_steps / 2) * p.step;
    const float o[3] = {p.vol.lat.ox, p.vol.lat.oy, p.vol.lat.oz};
    const float edge = 8.0f * p.vol.lat.vs;
    unsigned long long last = 0ull;
    uint32_t outside = 0;
    for (int s = 0; s < p.n_steps; s++) {
        const float zs = z0 + (float)s * p.step;
        if (!(zs > V.dmin)) continue;
        const float q0 = xn * zs - T[0], q1 = yn * zs - T[1], q2 = zs - T[2];
        float c[3];
        bool in_range = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float pw = (R[a] * q0 + R[3 + a] * q1) + R[6 + a] * q2;
            c[a] = floorf((pw - o[a]) / edge);
            in_range = in_range && c[a] >= -1048576.0f && c[a] < 1048576.0f;
        }
        if (!in_range) { outside++; continue; }
        const unsigned long long key = pack_key((int)c[0], (int)c[1], (int)c[2]);
        if (key == last) continue;   // (most samples of a ray share a block)
        last = key;
        bool won;
        uint32_t slot;
        if (!enter_key(p.vol, key, &won, &slot)) {
            atomicOr(&p.vol.header[LVDGS_TSDF_BLOCKS_HEADER_FLAGS], LVDGS_TSDF_BLOCKS_TABLE_FULL);
        } else if (won) {
            const int at = atomicAdd(&p.vol.header[LVDGS_TSDF_BLOCKS_HEADER_USED], 1);   // (runs past the pool: tsdf_blocks_settle_kernel)
            if (at >= 0 && at < p.vol.pool) {
                p.vol.values[slot] = at;
                p.vol.block_key[at] = key;
            } else {
                p.vol.values[slot] = -1;
                atomicAdd(&p.vol.header[LVDGS_TSDF_BLOCKS_HEADER_DROPPED], 1);
            }
        }
    }
    if (outside) atomicAdd(reinterpret_cast<uint32_t *>(&p.vol.header[LVDGS_TSDF_BLOCKS_HEADER_OUT_OF_RANGE]), outside);
}

// the counter of the allocation counted the dropped keys too
__global__ void tsdf_blocks_settle_kernel(BlockVolume v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) v.header[LVDGS_TSDF_BLOCKS_HEADER_USED] = used_blocks(v);
}

// ---------------------------------------------------------------- integration ----

struct BlocksIntegrateParams {
    BlockVolume vol;
    int count;
    TsdfView v[LVDGS_TSDF_MAX_VIEWS];
};

template <bool COLOR>
__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_integrate_kernel(BlocksIntegrateParams p) {
    const int lane = threadIdx.x & 63;
    const int used = used_blocks(p.vol);
    const TsdfLattice &lat = p.vol.lat;
    for (int block = blockIdx.x; block < used; block += gridDim.x) {   // (uniform)
        const unsigned long long key = p.vol.block_key[block];
        if (!(key & KEY_BIT)) continue;
        int bx, by, bz;
        unpack_key(key, bx, by, bz);
        const int gx = bx * 8, gy = by * 8, gz = bz * 8;
        bool touch = false;
        if (lane < p.count) touch = brick_may_touch(lat, p.v[lane], gx, gx + 7, gy, gy + 7, gz, gz + 7);
        const uint32_t live = (uint32_t)__ballot(touch);   // the same in all four waves
        if (live == 0u) continue;

        const int i = threadIdx.x & 7, j = (threadIdx.x >> 3) & 7, k = threadIdx.x >> 6;   // and k + 4
        const size_t base = (size_t)block * BLOCK_SAMPLES + threadIdx.x;
        float f[2], w[2], cr[2] = {0.f, 0.f}, cg[2] = {0.f, 0.f}, cb[2] = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 2; q++) {
            f[q] = p.vol.tsdf[base + 256 * q];
            w[q] = p.vol.weight[base + 256 * q];
            if constexpr (COLOR) { cr[q] = p.vol.r[base + 256 * q]; cg[q] = p.vol.g[base + 256 * q]; cb[q] = p.vol.b[base + 256 * q]; }
        }
        const float x = lat.ox + lat.vs * (float)(gx + i), y = lat.oy + lat.vs * (float)(gy + j);
        const float px[2] = {x, x}, py[2] = {y, y}, pz[2] = {lat.oz + lat.vs * (float)(gz + k), lat.oz + lat.vs * (float)(gz + k + 4)};
        const bool valid[2] = {true, true};
        bool changed = false, recoloured = false;
        tsdf_fuse_views<2, COLOR>(lat, p.v, p.count, live, px, py, pz, valid, f, w, cr, cg, cb, changed, recoloured);
        if (changed) {
#pragma unroll
            for (int q = 0; q < 2; q++) { p.vol.tsdf[base + 256 * q] = f[q]; p.vol.weight[base + 256 * q] = w[q]; }
        }
        if constexpr (COLOR) {
            if (recoloured) {
#pragma unroll
                for (int q = 0; q < 2; q++) { p.vol.r[base + 256 * q] = cr[q]; p.vol.g[base + 256 * q] = cg[q]; p.vol.b[base + 256 * q] = cb[q]; }
            }
        }
    }
}

// ---------------------------------------------------------------- the mesh ----
// Blocks are addressed by RANK, their place in `order`.  A sample or cell near a block is named by local coordinates in -1 .. 8 per
// axis; neighbour n = (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1) of the 27 holds the block that owns it.

constexpr int TILE_EDGE = 9, TILE_SAMPLES = 9 * 9 * 9;

struct BlocksMeshParams {
    BlockVolume vol;
    const int32_t *order;
    int vcap, fcap;
    int cell_lo[3], cell_hi[3];   // only cells with cell_lo <= g < cell_hi can be active
    uint32_t seq;
    float *vertices, *colors;
    int32_t *faces;
    int32_t *rank;               // pool: the rank of a pool block
    int32_t *nbr;                // pool * 27, by rank: the neighbours' ranks, -1: none
    uint32_t *mask;              // pool * 16, by rank: the block's active cells, bit l
    uint8_t *edges;              // pool * 512, by rank
    uint32_t *vcount, *fcount;   // pool each, by rank; vcount becomes the vertices in front of the block
    unsigned long long *fbase;   // pool, by rank: the faces in front of the block
    unsigned long long *totals;  // [0] vertices, [1] faces
    int32_t *host;
};

// the pool block of rank r < used, in 0 .. pool - 1 whatever `order` holds
__device__ __forceinline__ int pool_of(const BlocksMeshParams &M, int r) {
    const int at = M.order[r];
    return at < 0 ? 0 : at >= M.vol.pool ? M.vol.pool - 1 : at;
}
__device__ __forceinline__ int neighbour_of(int x, int y, int z) {   // local coordinates in -1 .. 8
    return ((x + 8) >> 3) + 3 * ((y + 8) >> 3) + 9 * ((z + 8) >> 3);
}
__device__ __forceinline__ int local_of(int x, int y, int z) { return (x & 7) + 8 * ((y & 7) + 8 * (z & 7)); }
// the rank of block r's neighbour n, in -1 .. used - 1
__device__ __forceinline__ int neighbour_rank(const BlocksMeshParams &M, int r, int n, int used) {
    const int nr = M.nbr[(size_t)r * 27 + n];
    return nr >= 0 && nr < used ? nr : -1;
}
// the active cells of rank nr with a local index below l
__device__ __forceinline__ uint32_t cells_below(const uint32_t *mask, int l) {
    uint32_t n = 0;
    for (int wd = 0; wd < (l >> 5); wd++) n += (uint32_t)__popc(mask[wd]);
    return n + (uint32_t)__popc(mask[l >> 5] & ((1u << (l & 31)) - 1u));
}

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_rank_kernel(BlocksMeshParams M) {
    const int used = used_blocks(M.vol);
    const int r = blockIdx.x * TB_THREADS + threadIdx.x;
    if (r < used) M.rank[pool_of(M, r)] = r;
}

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_neighbours_kernel(BlocksMeshParams M) {
    const int used = used_blocks(M.vol);
    const int64_t at = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x;
    const int r = (int)(at / 27), n = (int)(at - (int64_t)r * 27);
    if (r >= used) return;
    int found = -1;
    const unsigned long long key = M.vol.block_key[pool_of(M, r)];
    if (n == 13) {
        found = r;
    } else if (key & KEY_BIT) {
        int bx, by, bz;
        unpack_key(key, bx, by, bz);
        bx += n % 3 - 1; by += (n / 3) % 3 - 1; bz += n / 9 - 1;
        if (bx >= -COORD_BIAS && bx < COORD_BIAS && by >= -COORD_BIAS && by < COORD_BIAS && bz >= -COORD_BIAS && bz < COORD_BIAS) {
            const int pool = find_block(M.vol, pack_key(bx, by, bz), used);
            if (pool >= 0) {
                const int nr = M.rank[pool];
                if (nr >= 0 && nr < used && pool_of(M, nr) == pool) found = nr;
            }
        }
    }
    M.nbr[(size_t)r * 27 + n] = found;
}

// The bytes of block r and its +1 shell into LDS (9^3; a sample of a block that is not in use is unobserved).  Consecutive threads
// take consecutive x: a wave reads runs of 8 floats of a plane and writes consecutive bytes of LDS.
__device__ __forceinline__ void stage_samples(const BlocksMeshParams &M, int r, int used, uint8_t *tile) {
    for (int at = threadIdx.x; at < TILE_SAMPLES; at += TB_THREADS) {
        const int x = at % TILE_EDGE, y = (at / TILE_EDGE) % TILE_EDGE, z = at / (TILE_EDGE * TILE_EDGE);
        const int nr = neighbour_rank(M, r, neighbour_of(x, y, z), used);
        uint8_t fl = 0;
        if (nr >= 0) {
            const size_t s = (size_t)pool_of(M, nr) * BLOCK_SAMPLES + local_of(x, y, z);
            fl = (uint8_t)((M.vol.weight[s] > 0.f ? SAMPLE_OBSERVED : 0) | (M.vol.tsdf[s] < 0.f ? SAMPLE_INSIDE : 0));
        }
        tile[at] = fl;
    }
}

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_classify_kernel(BlocksMeshParams M) {
    __shared__ uint8_t tile[TILE_SAMPLES + 3];
    __shared__ uint32_t s_count[8];
    const int used = used_blocks(M.vol);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x; r < used; r += gridDim.x) {   // (uniform)
        stage_samples(M, r, used, tile);
        int bx, by, bz;
        unpack_key(M.vol.block_key[pool_of(M, r)], bx, by, bz);
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int l = threadIdx.x + 256 * half, i = l & 7, j = (l >> 3) & 7, k = l >> 6;
            const int gx = bx * 8 + i, gy = by * 8 + j, gz = bz * 8 + k;
            const bool in_range = gx >= M.cell_lo[0] && gx < M.cell_hi[0] && gy >= M.cell_lo[1] && gy < M.cell_hi[1] && gz >= M.cell_lo[2] && gz < M.cell_hi[2];
            const bool active = tsdf_cell_active([&](int q) { return tile[(i + (q & 1)) + TILE_EDGE * ((j + ((q >> 1) & 1)) + TILE_EDGE * (k + (q >> 2)))]; });
            const unsigned long long bits = __ballot(in_range && active);   // cells 64 * (wave + 4 * half) .. + 63
            if (lane == 0) {
                uint32_t *dst = M.mask + (size_t)r * 16 + 2 * (wave + 4 * half);
                dst[0] = (uint32_t)bits; dst[1] = (uint32_t)(bits >> 32);
                s_count[wave + 4 * half] = (uint32_t)__popcll(bits);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t n = 0;
            for (int q = 0; q < 8; q++) n += s_count[q];
            M.vcount[r] = n;
        }
        __syncthreads();   // (the tile and the counts are free again)
    }
}

// is the cell at local coordinates (x, y, z) in -1 .. 7 of block r's neighbourhood active?
__device__ __forceinline__ bool cell_active(const BlocksMeshParams &M, int r, int used, int x, int y, int z) {
    const int nr = neighbour_rank(M, r, neighbour_of(x, y, z), used);
    if (nr < 0) return false;
    const int l = local_of(x, y, z);
    return (M.mask[(size_t)nr * 16 + (l >> 5)] >> (l & 31)) & 1u;
}
// the vertex number of that cell, which is active
__device__ __forceinline__ int32_t cell_vertex(const BlocksMeshParams &M, int r, int used, int x, int y, int z) {
    const int nr = neighbour_rank(M, r, neighbour_of(x, y, z), used);
    if (nr < 0) return 0;
    return (int32_t)(M.vcount[nr] + cells_below(M.mask + (size_t)nr * 16, local_of(x, y, z)));
}

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_edges_kernel(BlocksMeshParams M) {
    __shared__ uint8_t tile[TILE_SAMPLES + 3];
    __shared__ uint32_t sh[SCAN_WORDS];
    const int used = used_blocks(M.vol);
    for (int r = blockIdx.x; r < used; r += gridDim.x) {   // (uniform)
        stage_samples(M, r, used, tile);
        __syncthreads();
        uint32_t mine = 0;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int l = threadIdx.x + 256 * half, i = l & 7, j = (l >> 3) & 7, k = l >> 6;
            const bool in0 = tile[i + TILE_EDGE * (j + TILE_EDGE * k)] & SAMPLE_INSIDE;
            uint32_t e = 0;
            if ((M.mask[(size_t)r * 16 + (l >> 5)] >> (l & 31)) & 1u) {   // c2 = the sample's own cell, for every axis
                auto differs = [&](int dx, int dy, int dz) { return ((tile[(i + dx) + TILE_EDGE * ((j + dy) + TILE_EDGE * (k + dz))] & SAMPLE_INSIDE) != 0) != in0; };
                auto act = [&](int dx, int dy, int dz) { return cell_active(M, r, used, i + dx, j + dy, k + dz); };
                e = tsdf_edge_axes(differs, act);
            }
            M.edges[(size_t)r * BLOCK_SAMPLES + l] = (uint8_t)(e | (in0 ? EDGE_LOW_INSIDE : 0));
            mine += 2u * (uint32_t)__popc(e);
        }
        uint32_t total = 0;
        scan_workgroup<TB_THREADS>(mine, sh, &total);   // (its barriers also free the tile)
        if (threadIdx.x == 0) M.fcount[r] = total;
    }
}

// One workgroup: the counts of the blocks become the rows in front of each.  A round's sum fits 32 bits (1024 blocks of 512 cells,
// six faces each); the carry over the rounds is 64 bits for the faces, and 2^22 blocks hold at most 2^31 vertices.
__global__ void __launch_bounds__(TB_SCAN_THREADS) tsdf_blocks_scan_kernel(BlocksMeshParams M) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const int used = used_blocks(M.vol);
    const uint32_t nv = scan_span_counts<TB_SCAN_THREADS>(M.vcount, M.vcount, used, 1, sh);
    const unsigned long long nf = scan_span_counts<TB_SCAN_THREADS>(M.fcount, M.fbase, used, 1, sh);
    if (threadIdx.x == 0) { M.totals[0] = nv; M.totals[1] = nf; }
}

template <bool COLOR>
__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_vertices_kernel(BlocksMeshParams M) {
    const int used = used_blocks(M.vol);
    const TsdfLattice &lat = M.vol.lat;
    for (int r = blockIdx.x; r < used; r += gridDim.x) {
        const uint32_t *mask = M.mask + (size_t)r * 16;
        const unsigned long long key = M.vol.block_key[pool_of(M, r)];
        int bx, by, bz;
        unpack_key(key, bx, by, bz);
        const uint32_t first = M.vcount[r];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int l = threadIdx.x + 256 * half, i = l & 7, j = (l >> 3) & 7, k = l >> 6;
            if (!((mask[l >> 5] >> (l & 31)) & 1u)) continue;
            const uint32_t row = first + cells_below(mask, l);
            if (row >= (uint32_t)M.vcap) continue;
            size_t o[8];
            float f[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {   // (an active cell: every corner's block is in use)
                const int x = i + (q & 1), y = j + ((q >> 1) & 1), z = k + (q >> 2);
                const int nr = neighbour_rank(M, r, neighbour_of(x, y, z), used);
                o[q] = (size_t)pool_of(M, nr < 0 ? r : nr) * BLOCK_SAMPLES + local_of(x, y, z);
                f[q] = M.vol.tsdf[o[q]];
            }
            float mean[3], col[3];
            tsdf_cell_vertex<COLOR>(f, [&](int q, int ch) { return (ch == 0 ? M.vol.r : ch == 1 ? M.vol.g : M.vol.b)[o[q]]; }, mean, col);
            const size_t out = (size_t)row * 3;
            M.vertices[out + 0] = lat.ox + lat.vs * ((float)(bx * 8 + i) + mean[0]);
            M.vertices[out + 1] = lat.oy + lat.vs * ((float)(by * 8 + j) + mean[1]);
            M.vertices[out + 2] = lat.oz + lat.vs * ((float)(bz * 8 + k) + mean[2]);
            if constexpr (COLOR) {
                if (M.colors) { M.colors[out + 0] = col[0]; M.colors[out + 1] = col[1]; M.colors[out + 2] = col[2]; }
            }
        }
    }
}

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_faces_kernel(BlocksMeshParams M) {
    __shared__ uint32_t sh[SCAN_WORDS];
    const int used = used_blocks(M.vol);
    const unsigned long long cap = (unsigned long long)M.fcap;
    for (int r = blockIdx.x; r < used; r += gridDim.x) {   // (uniform)
        TileWalk<TB_THREADS, uint32_t, unsigned long long> walk{M.fbase[r]};
        for (int half = 0; half < 2; half++) {   // (uniform)
            const int l = threadIdx.x + 256 * half, i = l & 7, j = (l >> 3) & 7, k = l >> 6;
            const uint32_t e = M.edges[(size_t)r * BLOCK_SAMPLES + l];
            unsigned long long row = walk.place(2u * (uint32_t)__popc(e & 7u), sh);
            if (!(e & 7u) || row >= cap) continue;
            const bool low_in = e & EDGE_LOW_INSIDE;
            const int32_t own = cell_vertex(M, r, used, i, j, k);
#pragma unroll
            for (int axis = 0; axis < 3; axis++) {
                if (!((e >> axis) & 1u)) continue;
                const TsdfStep b = tsdf_axis_step(axis + 1), c = tsdf_axis_step(axis + 2);
                tsdf_write_quad(M.faces, row, cap, low_in, cell_vertex(M, r, used, i - b.x - c.x, j - b.y - c.y, k - b.z - c.z),
                                cell_vertex(M, r, used, i - c.x, j - c.y, k - c.z), own, cell_vertex(M, r, used, i - b.x, j - b.y, k - b.z));
                row += 2;
            }
        }
    }
}

__global__ void tsdf_blocks_publish_kernel(BlocksMeshParams M) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    volatile int32_t *w = M.host;
    tsdf_publish_counts(w, M.totals, M.vcap, M.fcap);
    w[LVDGS_TSDF_BLOCKS_USED] = used_blocks(M.vol);
    w[LVDGS_TSDF_BLOCKS_DROPPED] = M.vol.header[LVDGS_TSDF_BLOCKS_HEADER_DROPPED];
    w[LVDGS_TSDF_BLOCKS_OUT_OF_RANGE] = M.vol.header[LVDGS_TSDF_BLOCKS_HEADER_OUT_OF_RANGE];
    w[LVDGS_TSDF_BLOCKS_FLAGS] = M.vol.header[LVDGS_TSDF_BLOCKS_HEADER_FLAGS];
    for (int j = LVDGS_TSDF_BLOCKS_FLAGS + 1; j < (int)(LVDGS_TSDF_BLOCKS_HOST_BYTES / sizeof(int32_t)); j++) w[j] = 0;
    seal_host_block(w, LVDGS_TSDF_BLOCKS_SEQ, (int32_t)M.seq);
}

// ---------------------------------------------------------------- growing ----

__global__ void __launch_bounds__(TB_THREADS) tsdf_blocks_rehash_kernel(BlockVolume v) {
    const int used = used_blocks(v);
    const int at = blockIdx.x * TB_THREADS + threadIdx.x;
    if (at >= used) return;
    const unsigned long long key = v.block_key[at];
    if (!(key & KEY_BIT)) return;
    bool won;
    uint32_t slot;
    if (!enter_key(v, key, &won, &slot)) atomicOr(&v.header[LVDGS_TSDF_BLOCKS_HEADER_FLAGS], LVDGS_TSDF_BLOCKS_TABLE_FULL);
    else if (won) v.values[slot] = at;
}

// ---------------------------------------------------------------- the host side ----

// the scratch of the mesh call (the arrays behind rank: by rank)
size_t blocks_mesh_layout(size_t pool, BlocksMeshParams *M, void *base) {
    Carver<BlocksMeshParams> c(M, base);
    c(c.v.rank, pool);
    c(c.v.nbr, pool * 27);
    c(c.v.mask, pool * 16);
    c(c.v.edges, pool * BLOCK_SAMPLES);
    c(c.v.vcount, pool);
    c(c.v.fcount, pool);
    c(c.v.fbase, pool);
    c.bytes(c.v.totals, 256);
    return c.off;
}

// everything the three calls refuse about the volume itself
int check_volume(const char *name, const lvdgs_tsdf_blocks *vol, BlockVolume *out) {
    if (!vol) { set_error("%s: volume is NULL", name); return LVDGS_E_INVALID; }
    if (int e = tsdf_check_planes(name, *vol)) return e;
    if (!vol->block_key || !vol->table_keys || !vol->table_values || !vol->header) {
        set_error("%s: block_key / table_keys / table_values / header is NULL", name); return LVDGS_E_INVALID;
    }
    if (vol->pool_blocks < 1 || vol->pool_blocks > LVDGS_TSDF_BLOCKS_MAX_POOL) {
        set_error("%s: pool_blocks %d is outside 1 .. %d", name, vol->pool_blocks, LVDGS_TSDF_BLOCKS_MAX_POOL); return LVDGS_E_RANGE;
    }
    const int64_t slots = vol->table_slots;
    if (slots < 2 * (int64_t)vol->pool_blocks || slots > (1 << 30) || (slots & (slots - 1)) != 0) {
        set_error("%s: table_slots %d must be a power of two, at least 2 * pool_blocks (%d) and at most 2^30", name, vol->table_slots, vol->pool_blocks);
        return LVDGS_E_RANGE;
    }
    if (int e = tsdf_check_constants(name, *vol)) return e;
    out->pool = vol->pool_blocks; out->slots = vol->table_slots;
    out->lat = TsdfLattice{vol->origin[0], vol->origin[1], vol->origin[2], vol->voxel_size, vol->trunc, vol->max_weight};
    out->tsdf = vol->tsdf; out->weight = vol->weight; out->r = vol->r; out->g = vol->g; out->b = vol->b;
    out->block_key = reinterpret_cast<unsigned long long *>(vol->block_key);
    out->keys = reinterpret_cast<unsigned long long *>(vol->table_keys);
    out->values = vol->table_values; out->header = vol->header;
    return LVDGS_OK;
}

int block_grid(int pool) { return pool < TB_MAX_GRID ? pool : TB_MAX_GRID; }

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

int lvdgs_tsdf_blocks_integrate(const lvdgs_tsdf_blocks *vol, const lvdgs_tsdf_view *const *views, int32_t count, void *stream) {
    const char *name = "tsdf blocks integrate";
    BlocksIntegrateParams p{};
    if (int e = tsdf_check_count(name, count)) return e;
    if (int e = check_volume(name, vol, &p.vol)) return e;
    const float steps = ceilf((vol->trunc + vol->voxel_size) / (0.5f * vol->voxel_size));
    if (!(steps <= (float)((LVDGS_TSDF_BLOCKS_MAX_STEPS - 1) / 2))) {
        set_error("%s: trunc %g over voxel_size %g needs more than %d steps along a ray", name, vol->trunc, vol->voxel_size, LVDGS_TSDF_BLOCKS_MAX_STEPS);
        return LVDGS_E_RANGE;
    }
    int64_t most_pixels;
    if (int e = tsdf_pack_views(name, views, count, vol->r != nullptr, p.v, &most_pixels)) return e;
    if (count == 0) return LVDGS_OK;
    p.count = count;
    AllocParams ap{};
    ap.vol = p.vol;
    ap.n_steps = 2 * (int)steps + 1;
    ap.step = 0.5f * vol->voxel_size;
    for (int v = 0; v < count; v++) ap.v[v] = p.v[v];
    hipStream_t s = (hipStream_t)stream;
    if (int e = launch("tsdf_blocks_alloc", 0, s, tsdf_blocks_alloc_kernel, dim3(cdiv(most_pixels, TB_THREADS), count), dim3(TB_THREADS), 0, ap)) return e;
    if (int e = launch("tsdf_blocks_settle", 0, s, tsdf_blocks_settle_kernel, dim3(1), dim3(WAVE), 0, p.vol)) return e;
    const dim3 grid(block_grid(p.vol.pool)), block(TB_THREADS);
    if (int e = launch("tsdf_blocks_integrate", 0, s, vol->r ? tsdf_blocks_integrate_kernel<true> : tsdf_blocks_integrate_kernel<false>, grid, block, 0, p)) return e;
    return LVDGS_OK;
}

size_t lvdgs_tsdf_blocks_mesh_scratch_bytes(int32_t pool_blocks) {
    if (pool_blocks < 1 || pool_blocks > LVDGS_TSDF_BLOCKS_MAX_POOL) return 0;
    return blocks_mesh_layout((size_t)pool_blocks, nullptr, nullptr);
}

int lvdgs_tsdf_blocks_mesh(const lvdgs_tsdf_blocks_mesh_args *a, void *stream) {
    const char *name = "tsdf blocks mesh";
    if (!a) { set_error("%s: args is NULL", name); return LVDGS_E_INVALID; }
    BlocksMeshParams M{};
    if (int e = check_volume(name, &a->vol, &M.vol)) return e;
    if (a->vertex_capacity < 0 || a->face_capacity < 0) {
        set_error("%s: negative capacity (%d vertices, %d faces)", name, a->vertex_capacity, a->face_capacity); return LVDGS_E_RANGE;
    }
    if (!a->order || !a->vertices || !a->faces || !a->host_state || !a->scratch) {
        set_error("%s: order / vertices / faces / host_state / scratch is NULL", name); return LVDGS_E_INVALID;
    }
    if (a->colors && !a->vol.r) { set_error("%s: colors asked for, the volume has no colour planes", name); return LVDGS_E_INVALID; }
    const size_t pool = (size_t)M.vol.pool;
    if (a->scratch_bytes < blocks_mesh_layout(pool, &M, a->scratch)) { set_error("%s: scratch too small", name); return LVDGS_E_INVALID; }
    if ((uintptr_t)a->scratch & 7u) { set_error("%s: scratch must be 8-byte aligned", name); return LVDGS_E_INVALID; }
    M.order = a->order;
    M.vcap = a->vertex_capacity; M.fcap = a->face_capacity; M.seq = a->seq;
    for (int q = 0; q < 3; q++) { M.cell_lo[q] = a->cell_lo[q]; M.cell_hi[q] = a->cell_hi[q]; }
    M.vertices = a->vertices; M.colors = a->colors; M.faces = a->faces;
    if (int e = host_block_address(a->host_state, name, &M.host)) return e;
    hipStream_t s = (hipStream_t)stream;
    const dim3 per_block(block_grid(M.vol.pool)), block(TB_THREADS);
    if (int e = launch("tsdf_blocks_rank", 0, s, tsdf_blocks_rank_kernel, dim3(cdiv((int64_t)pool, TB_THREADS)), block, 0, M)) return e;
    if (int e = launch("tsdf_blocks_neighbours", 0, s, tsdf_blocks_neighbours_kernel, dim3(cdiv((int64_t)pool * 27, TB_THREADS)), block, 0, M)) return e;
    if (int e = launch("tsdf_blocks_classify", 0, s, tsdf_blocks_classify_kernel, per_block, block, 0, M)) return e;
    if (int e = launch("tsdf_blocks_edges", 0, s, tsdf_blocks_edges_kernel, per_block, block, 0, M)) return e;
    if (int e = launch("tsdf_blocks_scan", 0, s, tsdf_blocks_scan_kernel, dim3(1), dim3(TB_SCAN_THREADS), 0, M)) return e;
    if (int e = launch("tsdf_blocks_vertices", 0, s, a->vol.r ? tsdf_blocks_vertices_kernel<true> : tsdf_blocks_vertices_kernel<false>, per_block, block, 0, M)) return e;
    if (int e = launch("tsdf_blocks_faces", 0, s, tsdf_blocks_faces_kernel, per_block, block, 0, M)) return e;
    if (int e = launch("tsdf_blocks_publish", 0, s, tsdf_blocks_publish_kernel, dim3(1), dim3(WAVE), 0, M)) return e;
    return LVDGS_OK;
}

int lvdgs_tsdf_blocks_rehash(const lvdgs_tsdf_blocks *vol, void *stream) {
    const char *name = "tsdf blocks rehash";
    BlockVolume v{};
    if (int e = check_volume(name, vol, &v)) return e;
    hipStream_t s = (hipStream_t)stream;
    // dropped keys are forgotten with the old table: words [_HEADER_DROPPED] and [_HEADER_FLAGS] are not adjacent to a counter in use
    if (int e = check_hip(hipMemsetAsync(v.header + LVDGS_TSDF_BLOCKS_HEADER_DROPPED, 0, sizeof(int32_t), s), name)) return e;
    if (int e = check_hip(hipMemsetAsync(v.header + LVDGS_TSDF_BLOCKS_HEADER_FLAGS, 0, sizeof(int32_t), s), name)) return e;
    if (int e = launch("tsdf_blocks_rehash", 0, s, tsdf_blocks_rehash_kernel, dim3(cdiv(v.pool, TB_THREADS)), dim3(TB_THREADS), 0, v)) return e;
    return LVDGS_OK;
}

}  // extern "C"
