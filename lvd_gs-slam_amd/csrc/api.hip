// C ABI entry points (include/lvdgs.h): argument checks, state-buffer layouts, launch sequencing.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"
#include "photometric.hpp"

namespace lvdgs {

// ---------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return LVDGS_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return LVDGS_E_HIP;
}

int host_block_address(void *host_state, const char *name, int32_t **dev) {
    void *d = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&d, host_state, 0);
    if (e != hipSuccess) { set_error("%s: host_state is not mapped pinned memory: %s", name, hipGetErrorString(e)); return LVDGS_E_HIP; }
    *dev = reinterpret_cast<int32_t *>(d);
    return LVDGS_OK;
}

// ---------------------------------------------------------------- profiling
namespace {
struct ProfSlot {
    std::string name;
    int64_t launches = 0;
    double total_ms = 0.0;
};
struct ProfPending {
    int slot;
    hipEvent_t start, stop;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfSlot> g_slots;
std::vector<ProfPending> g_pending;
std::vector<hipEvent_t> g_free_events;

hipEvent_t get_event() {
    if (!g_free_events.empty()) {
        hipEvent_t e = g_free_events.back();
        g_free_events.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
int slot_of(const char *name) {
    for (size_t i = 0; i < g_slots.size(); i++)
        if (g_slots[i].name == name) return (int)i;
    g_slots.push_back(ProfSlot{name});
    return (int)g_slots.size() - 1;
}
void drain_locked() {
    for (auto &p : g_pending) {
        (void)hipEventSynchronize(p.stop);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
            g_slots[p.slot].launches++;
            g_slots[p.slot].total_ms += ms;
        }
        g_free_events.push_back(p.start);
        g_free_events.push_back(p.stop);
    }
    g_pending.clear();
}
}  // namespace

ProfScope::ProfScope(const char *name, hipStream_t s) : slot(-1), stream(s) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    slot = slot_of(name);
    ProfPending p{slot, get_event(), get_event()};
    (void)hipEventRecord(p.start, s);
    g_pending.push_back(p);
}
ProfScope::~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    // the matching entry is the last one pushed for this scope
    for (size_t i = g_pending.size(); i-- > 0;)
        if (g_pending[i].slot == slot) {
            (void)hipEventRecord(g_pending[i].stop, stream);
            break;
        }
}

int allow_dynamic_lds(const void *kernel, int bytes, unsigned char (&done)[16]) {
    int dev = 0;
    if (int e = check_hip(hipGetDevice(&dev), "hipGetDevice")) return e;
    // Two host threads may get here together (one stream each): the flag is read and written atomically, and setting the
    // attribute twice is harmless, so the worst case is one redundant call.
    unsigned char &flag = done[dev & 15];
    if (!__atomic_load_n(&flag, __ATOMIC_ACQUIRE)) {
        if (int e = check_hip(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), "reserve dynamic LDS")) return e;
        __atomic_store_n(&flag, (unsigned char)1, __ATOMIC_RELEASE);
    }
    return LVDGS_OK;
}

// Images of up to group_max_tiles() tiles group their pairs by counting (binning.hip); larger ones, or every image
// when LVDGS_FORCE_RADIX_GROUPING is set in the environment (tests), take the radix sort on the tile id.
static bool use_counting_path(int num_tiles) {
    static const bool forced = getenv("LVDGS_FORCE_RADIX_GROUPING") != nullptr;
    return !forced && num_tiles <= group_max_tiles();
}

// Small grids (a KITTI frame: 1848 tiles for 2048 places) are resident all at once, so nothing rebalances the CUs while
// they run: the blend kernels then take their tiles longest list first, dealt round-robin (binning.hip writes the order
// into the second half of long_tiles).
#ifndef LVDGS_TILE_ORDER_MAX_TILES
#define LVDGS_TILE_ORDER_MAX_TILES 4096   // A/B builds: 0 = never
#endif
bool tile_order_in_use(int num_tiles) {
    return use_counting_path(num_tiles) && num_tiles <= LVDGS_TILE_ORDER_MAX_TILES && num_tiles > 0;
}

// ---------------------------------------------------------------- layouts
// (carve.hpp: one function per buffer gives its size and binds its arrays)
size_t geom_layout(int N, GeomView *v, void *base) {
    Carver<GeomView> c(v, base);
    const size_t n = (size_t)(N > 0 ? N : 1);
    c(c.v.rec, n * REC_FLOATS);
    c(c.v.tiles_touched, n);
    c(c.v.depth_bits, n);
    c(c.v.rect, n);
    c(c.v.slot_base, n);
    c(c.v.total, 64);
    return c.off;
}

static size_t scan_blocks(int N) { return (size_t)cdiv(N > 0 ? N : 1, 256) + 1; }  // one sum per preprocess_fwd workgroup

size_t prep_scratch_layout(int N, PrepScratch *v, void *base) {
    Carver<PrepScratch> c(v, base);
    c(c.v.blocksums, scan_blocks(N));
    return c.off;
}

size_t bin_layout(int64_t D, BinView *v, void *base) {
    Carver<BinView> c(v, base);
    const size_t d = (size_t)(D > 0 ? D : 1);
    c(c.v.point_list, d);
    c(c.v.tile_keys, d);
    c(c.v.pair_valid, d + 16);
    return c.off;
}

// Where the arrays lie is a function of the BUFFER's size, not of the pair count of the call: the forward pass lays the
// buffer out for its pair capacity, the backward pass is told the frame's actual pair count -- and both must find
// pair_valid (cleared by one, read by the other) in the same place.  The layout is the one of the largest pair count the
// buffer holds; a buffer of exactly lvdgs_binning_bytes(D) bytes has the layout bin_layout(D) describes.
int64_t bin_view(const lvdgs_args *a, BinView *v) {
    if (!a->binning_state || a->binning_bytes < bin_layout(1, nullptr, nullptr)) { *v = BinView{}; return 0; }
    int64_t p = a->binning_bytes > 2048 ? (int64_t)((a->binning_bytes - 3 * 256 - 16) / 9) : 1;   // 4 + 4 + 1 bytes per pair, three 256-byte roundings
    while (bin_layout(p + 1, nullptr, nullptr) <= a->binning_bytes) p++;
    while (p > 1 && bin_layout(p, nullptr, nullptr) > a->binning_bytes) p--;
    bin_layout(p, v, a->binning_state);
    return p;
}

size_t image_layout(int W, int H, ImageView *v, void *base) {
    Carver<ImageView> c(v, base);
    const size_t P = (size_t)W * H, T = (size_t)cdiv(W, TILE) * cdiv(H, TILE);
    c(c.v.ranges, T ? T : 1);
    c(c.v.long_count, 64);  // directly behind ranges: one memset clears both
    c(c.v.long_tiles, 2 * (T ? T : 1));  // queue of up to T tile ids (the second half is unused)
    c(c.v.final_T, P ? P : 1);
    c(c.v.n_contrib, P ? P : 1);
    return c.off;
}

size_t render_scratch_layout(int N, int64_t D, int W, int H, RenderScratch *v, void *base) {
    Carver<RenderScratch> c(v, base);
    RenderScratch &r = c.v;
    const size_t d = (size_t)(D > 0 ? D : 1);
    const TileGrid t(W, H);
    c(r.blocksums, scan_blocks(N));  // as in prep_scratch_layout: left by preprocess_fwd, read by count_pairs
    c(r.keys, d);
    c(r.vals, d);
    r.hist = r.totals = r.group_hist = r.group_totals = r.chunk_sums = nullptr;
    r.super = SuperView{};
    if (use_counting_path(t.T)) {
        c(r.group_hist, group_hist_entries(N, t.T));
        c(r.group_totals, (size_t)(t.T > 0 ? t.T : 1) + 4);   // (+4: the tile-range scan reads them 16 bytes at a time)
        c(r.chunk_sums, group_chunks(N));
        // two-level grouping (LVDGS_FLAG_SUPER_TILES): the super-tile grid's own counting state
        const size_t Ts = (size_t)(t.Ts ? t.Ts : 1);
        c(r.super.rect, (size_t)(N > 0 ? N : 1));
        c(r.super.hist, group_chunks(N) * Ts);
        c(r.super.totals, Ts + 4);
        c(r.super.ranges, Ts);
        c(r.super.long_count, 64);
        c(r.super.long_tiles, 2 * Ts);
        c(r.super.total, 64);
    } else {
        c(r.hist, radix_hist_entries(D));
        c(r.totals, (size_t)1 << SORT_MAX_BITS);
    }
    return c.off;
}

size_t bwd_scratch_layout(int N, int64_t D, BwdScratch *v, void *base) {
    Carver<BwdScratch> c(v, base);
    // (the pose-gradient partials first: their place must not depend on the pair count -- lvdgs_forward_backward_fused_loss
    // enqueues the backward before the host knows it, and lvdgs_tracking_tail looks for them with the count the caller then has)
    c(c.v.tau_part, (size_t)(cdiv(N > 0 ? N : 1, 256)) * 6);
    c(c.v.pair_grads, (size_t)(D > 0 ? D : 1) * PAIR_FLOATS + 8);   // (+8: the staging loads of preprocess_bwd are 16 bytes wide)
    return c.off;
}

int tile_sort_bits(int W, int H) {
    const int T = TileGrid(W, H).T;
    int bits = 0;
    while ((1 << bits) < T) bits++;
    return bits < 1 ? 1 : bits;
}

// ---------------------------------------------------------------- argument checks
static int check_common(const lvdgs_args *a) {
    if (!a) { set_error("args is NULL"); return LVDGS_E_INVALID; }
    if (a->image_width <= 0 || a->image_height <= 0) { set_error("bad image size %dx%d", a->image_width, a->image_height); return LVDGS_E_INVALID; }
    if (a->num_gaussians < 0) { set_error("negative Gaussian count"); return LVDGS_E_INVALID; }
    if (!(a->tanfovx > 0.f) || !(a->tanfovy > 0.f)) { set_error("tanfov must be positive"); return LVDGS_E_INVALID; }
    if (a->sh_degree < 0 || a->sh_degree > 3) { set_error("sh_degree %d outside 0..3", a->sh_degree); return LVDGS_E_INVALID; }
    if (!a->bg || !a->viewmatrix || !a->projmatrix) { set_error("bg / viewmatrix / projmatrix is NULL"); return LVDGS_E_INVALID; }
    // (in 64 bits: this is the check that makes a TileGrid's products fit an int)
    if ((int64_t)cdiv(a->image_width, TILE) * cdiv(a->image_height, TILE) > (1 << 22)) { set_error("image too large"); return LVDGS_E_RANGE; }
    return LVDGS_OK;
}

static int check_gaussians(const lvdgs_args *a) {
    if (a->num_gaussians == 0) return LVDGS_OK;
    if (!a->means3D || !a->opacities) { set_error("means3D / opacities is NULL"); return LVDGS_E_INVALID; }
    if ((a->shs == nullptr) == (a->colors_precomp == nullptr)) { set_error("provide exactly one of shs / colors_precomp"); return LVDGS_E_INVALID; }
    const bool sr = a->scales && a->rotations;
    if (sr == (a->cov3D_precomp != nullptr) || (!!a->scales != !!a->rotations)) { set_error("provide exactly one of scales+rotations / cov3D_precomp"); return LVDGS_E_INVALID; }
    if (a->shs) {
        if (!a->campos) { set_error("campos is NULL"); return LVDGS_E_INVALID; }
        if (a->sh_coeffs < (a->sh_degree + 1) * (a->sh_degree + 1)) { set_error("sh_coeffs %d too small for degree %d", a->sh_coeffs, a->sh_degree); return LVDGS_E_INVALID; }
    }
    return LVDGS_OK;
}

}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

const char *lvdgs_last_error(void) { return g_err; }
const char *lvdgs_version(void) { return "lvdgs 0.1.0 (gfx950)"; }

size_t lvdgs_geom_bytes(int32_t N) { return geom_layout(N, nullptr, nullptr); }
size_t lvdgs_prepare_scratch_bytes(int32_t N) { return prep_scratch_layout(N, nullptr, nullptr); }
size_t lvdgs_binning_bytes(int64_t D) { return bin_layout(D, nullptr, nullptr); }
size_t lvdgs_image_bytes(int32_t W, int32_t H) { return image_layout(W, H, nullptr, nullptr); }
size_t lvdgs_render_scratch_bytes(int32_t N, int64_t D, int32_t W, int32_t H) { return render_scratch_layout(N, D, W, H, nullptr, nullptr); }
size_t lvdgs_backward_scratch_bytes(int32_t N, int64_t D) { return bwd_scratch_layout(N, D, nullptr, nullptr); }

int lvdgs_state_layout_query(int32_t N, int64_t D, int32_t W, int32_t H, lvdgs_state_layout *out) {
    if (!out) { set_error("out is NULL"); return LVDGS_E_INVALID; }
    char *base = (char *)4096;  // offsets are computed by carving from a fake base
    GeomView g; BinView b; ImageView im;
    geom_layout(N, &g, base); bin_layout(D, &b, base); image_layout(W, H, &im, base);
    out->geom_rec = (char *)g.rec - base; out->geom_tiles_touched = (char *)g.tiles_touched - base;
    out->geom_slot_base = (char *)g.slot_base - base;
    out->bin_point_list = (char *)b.point_list - base; out->bin_tile_keys = (char *)b.tile_keys - base;
    out->img_ranges = (char *)im.ranges - base; out->img_final_T = (char *)im.final_T - base;
    out->img_n_contrib = (char *)im.n_contrib - base;
    out->geom_rec_floats = REC_FLOATS;
    return LVDGS_OK;
}

namespace {
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield");
#endif
}

// Per-thread, per-device host resources of the forward calls that wait for their pair counts: the pinned words the tile scans report in
// (common.hpp: PROBE_*) with their protocol -- sequence numbers, the wait, what becomes of the hints.  Nothing else in the library is stateful.
struct PairProbe {
    int device = -1;
    uint32_t *pinned = nullptr;       // PROBE_WORDS words
    uint32_t *pinned_dev = nullptr;   // the same words as the device addresses them
    uint32_t seq = 0;                 // of the last call on this thread and device whose tile scans reported
    hipEvent_t ready = nullptr;
    int longest_super = -1, queued_super = 0;   // the same hints for the super-tile lists of the two-level grouping (LVDGS_FLAG_SUPER_TILES)
    int longest = 0, queued = 0;  // of the previous frame on this device: which kernels for long segments the next frame
    int keep = 0;                 // launches behind its tile sort (a hint, never a result); kept for a few frames
    // (a call whose scans report, or the next group of a batch's views: under a number no block holds -- 0 is what the words are allocated with)
    void next_sequence() { if (++seq == 0u) seq = 1u; }
    PairReport report() const { return PairReport{pinned_dev, seq}; }
    uint32_t count(int block) const { return pinned[block + PROBE_COUNT]; }
    // The tile scan of this call has written a block when its sequence word holds the call's number.  (Two-level grouping: the later of
    // the view's two scans writes it, so the wait for the tile lists' block covers the super lists'.)
    int wait(int block) const {
        const uint32_t *flag = pinned + block + PROBE_SEQ;
        const auto t0 = std::chrono::steady_clock::now();
        // The count arrives some tens of microseconds after the call got here (the projection and the two scans); the wait is a
        // spin on a pinned word, polite to the core's sibling thread (pause) and, past ~20 us, to the scheduler (yield) -- the
        // reference's front end and back end are two processes that each sit in this wait once per render.
        for (uint64_t spins = 0;; spins++) {
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return LVDGS_OK;
            if (spins < 2000) cpu_relax();
            else std::this_thread::yield();
            if ((spins & 0xffffu) == 0xffffu) {
                if (int e = check_hip(hipGetLastError(), "while waiting for the pair count")) return e;
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                    set_error("timed out waiting for the pair count (the kernels before it never finished)");
                    return LVDGS_E_HIP;
                }
            }
        }
    }
    // What the next frames expect: this call's long segments -- the longest over its `views` tile-list blocks from `block` on -- or a recent call's
    // for a while (views alternate).  super_block (< 0: none): the super lists' block of its first view, whose hints are taken as they are.
    void fold_hints(int block, int views, int super_block) {
        int l = 0, q = 0;
        for (const uint32_t *w = pinned + block; views-- > 0; w += PROBE_BLOCK) { l = std::max(l, (int)w[PROBE_LONGEST]); q = std::max(q, (int)w[PROBE_QUEUED]); }
        if (l >= longest || keep == 0) { longest = l; queued = q; keep = l ? 32 : 0; }
        else keep--;
        if (super_block >= 0) { longest_super = (int)pinned[super_block + PROBE_LONGEST]; queued_super = (int)pinned[super_block + PROBE_QUEUED]; }
    }
};
thread_local PairProbe g_probe[16];

int get_probe(PairProbe **out) {
    int dev = 0;
    if (int e = check_hip(hipGetDevice(&dev), "hipGetDevice")) return e;
    PairProbe &p = g_probe[dev & 15];
    if (p.device != dev || !p.pinned) {
        p.device = dev;
        if (int e = check_hip(hipHostMalloc((void **)&p.pinned, PROBE_WORDS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent), "pinned pair count")) return e;
        for (int k = 0; k < PROBE_WORDS; k++) p.pinned[k] = 0u;
        if (int e = check_hip(hipHostGetDevicePointer((void **)&p.pinned_dev, p.pinned, 0), "device address of the pinned pair count")) return e;
        if (int e = check_hip(hipEventCreateWithFlags(&p.ready, hipEventDisableTiming), "pair count event")) return e;
    }
    *out = &p;
    return LVDGS_OK;
}

// The host's verdict on a view's pair counts (total_super: its super lists', 0 without two-level grouping): *num_rendered and the status, in whose
// message `view` (< 0: none) names the view of a batch and `remedy` is the entry point's advice; *redo: see enqueue_render_one_level.
int pair_verdict(uint32_t total, uint32_t total_super, int64_t cap, int view, const char *remedy, int64_t *num_rendered, bool *redo) {
    *redo = false;
    if (total > 0x7FFFFFFFu) { set_error("%u (Gaussian, tile) pairs exceed the 2^31 limit", total); return LVDGS_E_RANGE; }
    *num_rendered = (int64_t)total;
    if ((int64_t)total > cap) {
        char who[24] = "";
        if (view >= 0) snprintf(who, sizeof(who), "view %d: ", view);
        set_error("%s%u pairs exceed pair_capacity %lld: grow binning_state / scratch%s", who, total, (long long)cap, remedy);
        return LVDGS_E_CAPACITY;
    }
    *redo = (int64_t)total_super > cap;
    return LVDGS_OK;
}

// preprocess -> prefix sum of tiles touched; the pair count ends up in g.total (device)
int enqueue_prepare(const lvdgs_args *a, const GeomView &g, hipStream_t s) {
    const int N = a->num_gaussians;
    PrepScratch w;
    prep_scratch_layout(N, &w, a->scratch);
    if (int e = launch_preprocess_fwd(*a, g, w.blocksums, s)) return e;
    return launch_slot_scan(g.tiles_touched, g.slot_base, w.blocksums, g.total, N, a->debug, s);
}

// Where the pair count of a render comes from
enum class PairCount {
    known,     // the caller has it: `cap` IS the count (lvdgs_forward_render; an empty map)
    scanned,   // the slot scan behind the projection has left it in g.total (enqueue_prepare: lvdgs_forward on the radix path); clamped to cap
    counted,   // the projection kernel has left the per-chunk tile counts (enqueue_counted_forward): the tile-range scan makes the count in g.total,
               // reports it to the call's probe -- if it has one -- as soon as it exists, and the scatter makes slot_base
};
// (pair emission ->) grouping by tile -> ranges -> depth order inside each tile -> blend.  `cap` sizes grids and buffers.
// probe (may be null): the hints of the recent frames on this device, and where a counted render reports.
int enqueue_render(const lvdgs_args *a, int64_t cap, PairCount from, const PairProbe *probe, hipStream_t s) {
    const int N = a->num_gaussians, W = a->image_width, H = a->image_height;
    GeomView g{}; BinView b{}; ImageView im; RenderScratch w{};
    image_layout(W, H, &im, a->image_state);
    const TileGrid t(W, H);
    const bool counted = from == PairCount::counted;
    int row0, row1;
    tile_row_band(*a, &row0, &row1);
    const uint32_t *count = nullptr;
    if (N > 0) {
        geom_layout(N, &g, a->geom_state);
        // blend_fwd accumulates into n_touched: the counting path clears it in its first kernel, the radix path here
        if (!(cap > 0 && use_counting_path(t.T)))
            if (int e = check_hip(hipMemsetAsync(a->n_touched, 0, sizeof(int32_t) * (size_t)N, s), "memset n_touched")) return e;
        if (from != PairCount::known) count = g.total;
    }
    bool grouped = false, super = false;
    if (cap > 0) {
        if (bin_view(a, &b) < cap) { set_error("internal: binning_state smaller than the pair capacity"); return LVDGS_E_INVALID; }
        render_scratch_layout(N, cap, W, H, &w, a->scratch);
        if (use_counting_path(t.T)) {
            // counting path: no pair list is materialised, the tile ranges fall out of the counts
            if (!counted)
                if (int e = launch_group_count(*a, g, im, w, s)) return e;
            super = super_tiles_in_use(*a);
            if (super && !counted)   // two-level grouping: the super-tile grid's counts first (single-call forward: the projection kernel has made them), the scan below then takes both grids in its two launches
                if (int e = launch_super_count(*a, g, w.super, s)) return e;
            // (single-call forward: the tile scan writes the pair count and the hints into the caller thread's pinned words itself)
            uint32_t *total_out = counted ? g.total : nullptr;
            const PairReport report = counted && probe ? probe->report() : PairReport{};
            if (int e = launch_group_scan(*a, im, w, cap, total_out, report, s)) return e;
            if (int e = launch_group_scatter(*a, g, im, w, (unsigned long long *)w.keys, cap, counted, b.pair_valid, total_out, report, s)) return e;
            if (super) {
                // two-level grouping: keys scattered and sorted per 64 x 64-pixel super-tile, the tiles' lists read off the sorted super lists
                // (binning.hip); b.tile_keys -- the radix path's -- takes the sorted super lists
                ImageView ims{};
                ims.ranges = w.super.ranges; ims.long_count = w.super.long_count; ims.long_tiles = w.super.long_tiles;
                if (int e = launch_tile_depth_sort(ims, t.Ts, 0, t.Ts, g.rec, b.tile_keys, w.keys, true, probe ? probe->longest_super : -1,
                                                   probe ? probe->queued_super : 0, a->debug, s)) return e;
                if (int e = launch_super_expand(*a, g, w.super, im, b.tile_keys, b.point_list, s)) return e;
            }
            grouped = true;
        } else {
            if (!w.hist) { set_error("internal: scratch was not laid out for the radix grouping"); return LVDGS_E_INVALID; }
            const int bits = tile_sort_bits(W, H);
            // start in the buffer that makes the sorted result land in binning_state
            const bool start_in_state = (radix_num_passes(bits) % 2) == 0;
            uint32_t *k0 = start_in_state ? b.tile_keys : w.keys, *v0 = start_in_state ? b.point_list : w.vals;
            uint32_t *k1 = start_in_state ? w.keys : b.tile_keys, *v1 = start_in_state ? w.vals : b.point_list;
            if (int e = check_hip(hipMemsetAsync(b.pair_valid, 0, (size_t)cap, s), "memset pair_valid")) return e;
            if (int e = launch_emit_pairs(*a, g, k0, v0, cap, s)) return e;
            bool in_first = true;
            if (int e = radix_sort_pairs(k0, v0, k1, v1, cap, bits, w.hist, w.totals, &in_first, a->debug, s, count)) return e;
            if ((in_first ? k0 : k1) != b.tile_keys) { set_error("internal: sorted list not in binning_state"); return LVDGS_E_INVALID; }
        }
    }
    if (!grouped)
        if (int e = launch_tile_ranges(b.tile_keys, cap, count, im, t.T, a->debug, s)) return e;
    // w.keys + w.vals: the (depth, id) keys the counting path scattered, or scratch for over-long segments after the radix path
    if (cap > 0 && !super) {
        // long segments: expected as the recent frames on this device had them (single-call forward), unknown otherwise
        if (int e = launch_tile_depth_sort(im, t.T, row0 * t.gx, row1 * t.gx, g.rec, b.point_list, w.keys, grouped, probe ? probe->longest : -1,
                                           probe ? probe->queued : 0, a->debug, s)) return e;
    }
    // (tile lists beyond what one wave sorts on recent frames: the blend kernel built for deep lists)
    if (a->flags & LVDGS_FLAG_NO_BLEND) return LVDGS_OK;   // the caller blends several views in one launch: lvdgs_blend_forward_batch
    return launch_blend_fwd(*a, g, b, im, probe && probe->longest > 0, s);
}

int check_render_buffers(const lvdgs_args *a, int64_t cap) {
    const int N = a->num_gaussians, W = a->image_width, H = a->image_height;
    if (!a->out_color || !a->out_depth || !a->out_opacity || !a->image_state) { set_error("output image or image_state is NULL"); return LVDGS_E_INVALID; }
    if (a->image_bytes < lvdgs_image_bytes(W, H)) { set_error("image_state too small"); return LVDGS_E_INVALID; }
    if (N > 0 && (!a->n_touched || !a->geom_state)) { set_error("n_touched / geom_state is NULL"); return LVDGS_E_INVALID; }
    if (cap > 0) {
        if (!a->binning_state || !a->scratch) { set_error("binning_state / scratch is NULL"); return LVDGS_E_INVALID; }
        if (a->binning_bytes < lvdgs_binning_bytes(cap) || a->scratch_bytes < lvdgs_render_scratch_bytes(N, cap, W, H)) {
            set_error("binning_state or scratch too small for %lld pairs", (long long)cap); return LVDGS_E_INVALID;
        }
    }
    return LVDGS_OK;
}

// What the projection of a map (N > 0) writes: the geometry half of a forward call's buffers
int check_projection_buffers(const lvdgs_args *a) {
    if (!a->radii || !a->geom_state || !a->scratch) { set_error("radii / geom_state / scratch is NULL"); return LVDGS_E_INVALID; }
    if (a->geom_bytes < lvdgs_geom_bytes(a->num_gaussians) || a->scratch_bytes < lvdgs_prepare_scratch_bytes(a->num_gaussians)) {
        set_error("geom_state or scratch too small"); return LVDGS_E_INVALID;
    }
    return LVDGS_OK;
}

// A forward of a map (N > 0) with a pair capacity: the capacity and every buffer it sizes
int check_forward(const lvdgs_args *a) {
    const int64_t cap = a->pair_capacity;
    if (cap <= 0 || cap > 0x7FFFFFFFll) { set_error("pair_capacity must be in 1..2^31-1"); return LVDGS_E_INVALID; }
    if (int e = check_projection_buffers(a)) return e;
    return check_render_buffers(a, cap);
}

// Are a and a0 views of one frame: the image size, the band, and those of `flags` that must agree
bool one_frame(const lvdgs_args *a, const lvdgs_args *a0, int flags) {
    return a->image_width == a0->image_width && a->image_height == a0->image_height && a->tile_row_begin == a0->tile_row_begin &&
           a->tile_row_end == a0->tile_row_end && !((a->flags ^ a0->flags) & flags);
}

// lvdgs_loss_args as the backward blend pass of this rasterizer call reads it
int fused_loss_params(const lvdgs_args *a, const lvdgs_loss_args *loss, LossParams *out) {
    if (int e = loss_fused_params(loss, out)) return e;
    if (loss->width != a->image_width || loss->height != a->image_height) { set_error("fused loss: image size differs from the rasterizer's"); return LVDGS_E_INVALID; }
    return LVDGS_OK;
}

// Two-level grouping whose super lists outgrew the pair capacity while the tile lists fit (Ds > cap >= D: a Gaussian whose rectangle spans
// more than 64 super-tiles is listed on all of them, however few of its tiles are kept): the tile lists read off the super lists were cut
// short.  The view is redone one-level behind what is enqueued -- the projection's counts, geom_state and slot_base stand -- with no
// further host wait; the flag's contract makes the bits those the hint would have given.
int enqueue_render_one_level(const lvdgs_args *a, int64_t cap, hipStream_t s) {
    lvdgs_args one = *a;
    one.flags &= ~LVDGS_FLAG_SUPER_TILES;
    // (the blend of the cut lists counted into n_touched; the counting path's projection cleared it)
    if (int e = check_hip(hipMemsetAsync(a->n_touched, 0, sizeof(int32_t) * (size_t)a->num_gaussians, s), "memset n_touched")) return e;
    return enqueue_render(&one, cap, PairCount::counted, nullptr, s);
}

// A forward on the counting path: the projection kernel counts the pairs per (chunk, tile) as it goes, the tile-range scan makes the pair count
// and the scatter the slot prefix sum: three launches fewer than project / scan / count in turn.  (render: a, or its copy with LVDGS_FLAG_NO_BLEND)
int enqueue_counted_forward(const lvdgs_args *a, const lvdgs_args *render, PairProbe *probe, GeomView *g, hipStream_t s) {
    const int N = a->num_gaussians, W = a->image_width, H = a->image_height;
    ImageView im; RenderScratch w{};
    geom_layout(N, g, a->geom_state);
    image_layout(W, H, &im, a->image_state);
    render_scratch_layout(N, a->pair_capacity, W, H, &w, a->scratch);
    if (int e = launch_preprocess_count(*a, *g, im, w, s)) return e;
    probe->next_sequence();
    return enqueue_render(render, a->pair_capacity, PairCount::counted, probe, s);
}
// ... and the host's half behind everything the call enqueues: the wait for the counts, the hints for the next frames, the verdict
int finish_counted_forward(const lvdgs_args *a, PairProbe *probe, const char *remedy, int64_t *num_rendered, bool *redo) {
    if (int e = probe->wait(PROBE_CALL)) return e;
    const bool super = super_tiles_in_use(*a);
    probe->fold_hints(PROBE_CALL, 1, super ? PROBE_CALL_SUPER : -1);
    return pair_verdict(probe->count(PROBE_CALL), super ? probe->count(PROBE_CALL_SUPER) : 0u, a->pair_capacity, -1, remedy, num_rendered, redo);
}
}  // namespace

int lvdgs_forward_prepare(const lvdgs_args *a, int64_t *num_rendered, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = check_common(a)) return e;
    if (int e = check_gaussians(a)) return e;
    if (!num_rendered) { set_error("num_rendered is NULL"); return LVDGS_E_INVALID; }
    const int N = a->num_gaussians;
    *num_rendered = 0;
    if (N == 0) return LVDGS_OK;
    if (int e = check_projection_buffers(a)) return e;
    GeomView g;
    geom_layout(N, &g, a->geom_state);
    if (int e = enqueue_prepare(a, g, s)) return e;
    uint32_t total = 0;
    if (int e = check_hip(hipMemcpyAsync(&total, g.total, sizeof(uint32_t), hipMemcpyDeviceToHost, s), "read pair count")) return e;
    if (int e = check_hip(hipStreamSynchronize(s), "synchronize after prepare")) return e;
    if (total > 0x7FFFFFFFu) { set_error("%u (Gaussian, tile) pairs exceed the 2^31 limit", total); return LVDGS_E_RANGE; }
    *num_rendered = (int64_t)total;
    return LVDGS_OK;
}

int lvdgs_forward_render(const lvdgs_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = check_common(a)) return e;
    const int64_t D = a->num_gaussians == 0 ? 0 : a->num_rendered;
    if (D < 0) { set_error("negative num_rendered"); return LVDGS_E_INVALID; }
    if (int e = check_render_buffers(a, D)) return e;
    // (two-level grouping is left out: the super lists' count is not known here, and this call is the rare re-render behind a count
    // that outgrew the capacity -- the contract makes the bits the same)
    lvdgs_args one = *a;
    one.flags &= ~LVDGS_FLAG_SUPER_TILES;
    return enqueue_render(&one, D, PairCount::known, nullptr, s);
}

int lvdgs_forward(const lvdgs_args *a, int64_t *num_rendered, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = check_common(a)) return e;
    if (int e = check_gaussians(a)) return e;
    if (!num_rendered) { set_error("num_rendered is NULL"); return LVDGS_E_INVALID; }
    const int N = a->num_gaussians;
    *num_rendered = 0;
    if (N == 0) {
        if (int e = check_render_buffers(a, 0)) return e;
        return enqueue_render(a, 0, PairCount::known, nullptr, s);
    }
    if (int e = check_forward(a)) return e;
    const int64_t cap = a->pair_capacity;
    PairProbe *probe = nullptr;
    if (int e = get_probe(&probe)) return e;
    GeomView g;
    const char *remedy = " and call lvdgs_forward_render";
    bool redo;
    // Everything after the count is enqueued BEFORE the host waits for it: the GPU keeps working on
    // the tile sort and the blend while the host learns whether the capacity was enough.
    if (use_counting_path(TileGrid(*a).T)) {
        if (int e = enqueue_counted_forward(a, a, probe, &g, s)) return e;
        if (int e = finish_counted_forward(a, probe, remedy, num_rendered, &redo)) return e;
    } else {
        geom_layout(N, &g, a->geom_state);
        if (int e = enqueue_prepare(a, g, s)) return e;
        // (the slot scan leaves the pair count alone -- ONE word is copied; the words behind it are the counting path's hints and
        // the sequence number its wait spins on, which a copy of uninitialised device words must not touch)
        if (int e = check_hip(hipMemcpyAsync(probe->pinned + PROBE_CALL + PROBE_COUNT, g.total, sizeof(uint32_t), hipMemcpyDeviceToHost, s), "read pair count")) return e;
        if (int e = check_hip(hipEventRecord(probe->ready, s), "record pair count event")) return e;
        if (int e = enqueue_render(a, cap, PairCount::scanned, probe, s)) return e;
        if (int e = check_hip(hipEventSynchronize(probe->ready), "wait for pair count")) return e;
        if (int e = pair_verdict(probe->count(PROBE_CALL), 0u, cap, -1, remedy, num_rendered, &redo)) return e;
    }
    return redo ? enqueue_render_one_level(a, cap, s) : LVDGS_OK;
}

// What a backward call is given for the pixels' gradients: which pointers it needs, which flags it may carry
enum class BackwardKind {
    pixel_gradients,   // dL_dout_*: the call's own blend pass reads them (lvdgs_backward)
    fused_loss,        // a lvdgs_loss_args: the blend pass evaluates the photometric loss itself
    masked_loss,       // a lvdgs_masked_loss_args: ... the static-mask mapping loss
    blended,           // nothing: the blend pass has run (lvdgs_gaussian_backward_batch behind a batched one)
};
struct BackwardViews { int64_t D; GeomView g; BinView b; ImageView im; BwdScratch w; };

// The arguments of a backward call of a kind, and its buffers laid out (D: its pair count)
static int check_backward(const lvdgs_args *a, BackwardKind kind, BackwardViews *v) {
    if (int e = check_common(a)) return e;
    if (int e = check_gaussians(a)) return e;
    const int N = a->num_gaussians, W = a->image_width, H = a->image_height;
    const int64_t D = N == 0 ? 0 : a->num_rendered;
    if (D < 0) { set_error("negative num_rendered"); return LVDGS_E_INVALID; }
    if (!a->image_state || a->image_bytes < lvdgs_image_bytes(W, H)) { set_error("image_state is NULL or too small"); return LVDGS_E_INVALID; }
    *v = BackwardViews{};
    v->D = D;
    image_layout(W, H, &v->im, a->image_state);
    const bool pose_only = (a->flags & LVDGS_FLAG_POSE_ONLY) != 0;
    if (N == 0) return LVDGS_OK;
    if ((kind == BackwardKind::pixel_gradients && !a->dL_dout_color) || !a->projmatrix_raw || !a->radii) { set_error("a required backward pointer is NULL"); return LVDGS_E_INVALID; }
    if (kind == BackwardKind::masked_loss && pose_only) { set_error("LVDGS_FLAG_POSE_ONLY: the static-mask mapping loss is a mapping loss, its backward makes every gradient"); return LVDGS_E_INVALID; }
    if (pose_only) {
        // a view-dependent colour moves with the camera centre: its gradient feeds dL/dtau (preprocess_bwd.hip: chain_colour), and the
        // pose-only passes do not make it
        if (a->shs && a->sh_degree > 0) { set_error("LVDGS_FLAG_POSE_ONLY needs sh_degree 0 or colors_precomp"); return LVDGS_E_INVALID; }
        if (a->flags & LVDGS_FLAG_ACCUMULATE_PARAM_GRADS) { set_error("LVDGS_FLAG_POSE_ONLY writes no parameter gradients: nothing to accumulate"); return LVDGS_E_INVALID; }
    } else {
        if (!a->dL_dmeans3D || !a->dL_dmeans2D || !a->dL_dopacities) { set_error("a required backward pointer is NULL"); return LVDGS_E_INVALID; }
        if (a->cov3D_precomp ? !a->dL_dcov3D : (!a->dL_dscales || !a->dL_drotations)) { set_error("covariance gradient output is NULL"); return LVDGS_E_INVALID; }
        if (a->shs ? !a->dL_dshs : !a->dL_dcolors) { set_error("colour gradient output is NULL"); return LVDGS_E_INVALID; }
    }
    if (!a->geom_state || !a->scratch || (D > 0 && !a->binning_state)) { set_error("a state / scratch buffer is NULL"); return LVDGS_E_INVALID; }
    if (a->geom_bytes < lvdgs_geom_bytes(N) || (D > 0 && a->binning_bytes < lvdgs_binning_bytes(D)) ||
        a->scratch_bytes < lvdgs_backward_scratch_bytes(N, D)) {
        set_error("a state / scratch buffer is too small"); return LVDGS_E_INVALID;
    }
    geom_layout(N, &v->g, a->geom_state);
    bwd_scratch_layout(N, D, &v->w, a->scratch);
    if (D > 0) bin_view(a, &v->b);
    return LVDGS_OK;
}

// The per-Gaussian pass behind a view's backward blend pass (an empty map: the pose gradient is zero)
static int enqueue_gaussian_backward(const lvdgs_args *a, const BackwardViews &v, hipStream_t s) {
    if (a->num_gaussians == 0) return a->dL_dtau ? check_hip(hipMemsetAsync(a->dL_dtau, 0, 6 * sizeof(float), s), "memset tau") : LVDGS_OK;
    return launch_preprocess_bwd(*a, v.g, v.w, v.b.pair_valid, s);
}

int lvdgs_backward(const lvdgs_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (a && (a->flags & LVDGS_FLAG_NO_BLEND)) { set_error("LVDGS_FLAG_NO_BLEND: lvdgs_backward runs its own blend pass; the calls that leave it to a batched one (lvdgs_blend_backward_fused_loss_batch / lvdgs_blend_backward_window_batch) are lvdgs_backward_fused_loss, lvdgs_backward_masked_loss and lvdgs_gaussian_backward_batch"); return LVDGS_E_INVALID; }
    BackwardViews v;
    if (int e = check_backward(a, BackwardKind::pixel_gradients, &v)) return e;
    if (v.D > 0)
        if (int e = launch_blend_bwd(*a, v.g, v.b, v.im, v.w, s)) return e;
    return enqueue_gaussian_backward(a, v, s);
}

int lvdgs_backward_fused_loss(const lvdgs_args *a, const lvdgs_loss_args *loss, int32_t propagate_opacity_grad, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("backward: args is NULL"); return LVDGS_E_INVALID; }
    LossParams lp;
    if (int e = fused_loss_params(a, loss, &lp)) return e;
    BackwardViews v;
    if (int e = check_backward(a, BackwardKind::fused_loss, &v)) return e;
    // With the loss inside, the blend pass runs even over empty lists (a view that sees nothing, an empty map): it is what
    // evaluates the loss of the background image -- value and exposure gradients -- and no pair record is written.
    if (!(a->flags & LVDGS_FLAG_NO_BLEND))
        if (int e = launch_blend_bwd_fused_loss(*a, v.g, v.b, v.im, v.w, lp, propagate_opacity_grad != 0, s)) return e;
    return enqueue_gaussian_backward(a, v, s);
}

// The forward passes of `count` views of one map and one image size, every stage ONE launch (include/lvdgs.h).
int lvdgs_forward_batch(const lvdgs_args *const *views, int32_t count, int64_t *num_rendered, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (count < 0 || (count > 0 && (!views || !num_rendered))) { set_error("forward batch: bad view list"); return LVDGS_E_INVALID; }
    if (count == 0) return LVDGS_OK;
    for (int k = 0; k < count; k++) num_rendered[k] = 0;
    const lvdgs_args *a0 = views[0];
    if (!a0) { set_error("forward batch: view 0 is NULL"); return LVDGS_E_INVALID; }
    const int N = a0->num_gaussians, W = a0->image_width, H = a0->image_height;
    if (int e = check_common(a0)) return e;
    if (N <= 0 || !use_counting_path(TileGrid(W, H).T)) { set_error("forward batch: needs a map (N > 0) and an image of at most %d tiles (the views go through lvdgs_forward one by one otherwise)", group_max_tiles()); return LVDGS_E_INVALID; }
    std::vector<GeomView> g(count); std::vector<BinView> b(count); std::vector<ImageView> im(count); std::vector<RenderScratch> w(count);
    std::vector<int64_t> caps(count);
    for (int k = 0; k < count; k++) {
        const lvdgs_args *a = views[k];
        if (!a) { set_error("forward batch: view %d is NULL", k); return LVDGS_E_INVALID; }
        if (int e = check_common(a)) return e;
        if (int e = check_gaussians(a)) return e;
        if (a->num_gaussians != N || !one_frame(a, a0, LVDGS_FLAG_LIST_ALL_TILES | LVDGS_FLAG_NO_BLEND | LVDGS_FLAG_SUPER_TILES) ||
            a->means3D != a0->means3D || a->opacities != a0->opacities || a->scales != a0->scales || a->rotations != a0->rotations ||
            a->cov3D_precomp != a0->cov3D_precomp || a->shs != a0->shs || a->colors_precomp != a0->colors_precomp || a->sh_coeffs != a0->sh_coeffs ||
            a->activations != a0->activations) {
            set_error("forward batch: the views differ in map (means3D / opacities / scales / rotations / cov3D_precomp / shs / colors_precomp / activations), image size, band or flags"); return LVDGS_E_INVALID;
        }
        if (int e = check_forward(a)) return e;
        caps[k] = a->pair_capacity;
        geom_layout(N, &g[k], a->geom_state);
        image_layout(W, H, &im[k], a->image_state);
        render_scratch_layout(N, caps[k], W, H, &w[k], a->scratch);
        if (bin_view(a, &b[k]) < caps[k]) { set_error("internal: binning_state smaller than the pair capacity"); return LVDGS_E_INVALID; }
    }
    PairProbe *probe = nullptr;
    if (int e = get_probe(&probe)) return e;
    const bool super = super_tiles_in_use(*a0);   // two-level grouping: the scan and the scatter work on the super-tile grid; the tiles' lists are read off the sorted super lists
    int status = LVDGS_OK;
    for (int first = 0; first < count; first += FWD_BATCH_VIEWS) {
        const int m = count - first < FWD_BATCH_VIEWS ? count - first : FWD_BATCH_VIEWS;
        const lvdgs_args *const *av = views + first;
        probe->next_sequence();
        if (int e = launch_preprocess_count_batch(av, &g[first], &im[first], &w[first], m, s)) return e;
        if (int e = launch_group_scan_batch(av, &g[first], &im[first], &w[first], &caps[first], m, probe->report(), s)) return e;
        if (int e = launch_group_scatter_batch(av, &g[first], &im[first], &w[first], &b[first], &caps[first], m, s)) return e;
        if (int e = launch_tile_depth_sort_batch(av, &g[first], &im[first], &w[first], &b[first], m, super ? probe->longest_super : probe->longest,
                                                 super ? probe->queued_super : probe->queued, s)) return e;
        if (super)
            if (int e = launch_super_expand_batch(av, &g[first], &im[first], &w[first], &b[first], m, s)) return e;
        if (!(a0->flags & LVDGS_FLAG_NO_BLEND))
            if (int e = launch_blend_fwd_batch(av, &g[first], &b[first], &im[first], m, probe->longest > 0, s)) return e;
        // everything is enqueued: now the counts (the GPU is busy with the scatter, the sorts and the blend meanwhile)
        for (int k = 0; k < m; k++) {
            const int block = PROBE_BATCH + PROBE_BLOCK * k, block_super = PROBE_BATCH_SUPER + PROBE_BLOCK * k;
            if (int e = probe->wait(block)) return e;
            bool redo;
            const int e = pair_verdict(probe->count(block), super ? probe->count(block_super) : 0u, caps[first + k], first + k, " and call lvdgs_forward_render for it",
                                       &num_rendered[first + k], &redo);
            if (e == LVDGS_E_RANGE) return e;
            if (e) status = e;
            if (redo)
                if (int e2 = enqueue_render_one_level(av[k], caps[first + k], s)) return e2;
        }
        probe->fold_hints(PROBE_BATCH, m, super ? PROBE_BATCH_SUPER : -1);
    }
    return status;
}

// lvdgs_forward + lvdgs_backward_fused_loss as one call; on small grids the two blend passes are ONE launch (blend.hip:
// blend_fwd_bwd_kernel).  Frames beyond this many tiles fill the chip in either blend kernel by themselves: the calls in turn.
#ifndef LVDGS_FUSED_BLEND_MAX_TILES
#define LVDGS_FUSED_BLEND_MAX_TILES 4096   // A/B builds: 0 = never
#endif
int lvdgs_forward_backward_fused_loss(const lvdgs_args *a, const lvdgs_loss_args *loss, int32_t propagate_opacity_grad, int64_t *num_rendered,
                                      void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a || !num_rendered) { set_error("forward + backward: args / num_rendered is NULL"); return LVDGS_E_INVALID; }
    if (int e = check_common(a)) return e;
    const int N = a->num_gaussians, num_tiles = TileGrid(*a).T;
    const int64_t cap = a->pair_capacity;
    static const bool off = getenv("LVDGS_NO_FUSED_BLEND") != nullptr;   // (test / A-B hook: the two calls in turn whatever the grid)
    const bool fuse = !off && N > 0 && use_counting_path(num_tiles) && num_tiles <= LVDGS_FUSED_BLEND_MAX_TILES && !(a->flags & LVDGS_FLAG_NO_BLEND) &&
                      cap > 0 && cap <= 0x7FFFFFFFll;
    if (!fuse) {
        if (int e = lvdgs_forward(a, num_rendered, stream)) return e;
        lvdgs_args b = *a;
        b.num_rendered = *num_rendered;
        return lvdgs_backward_fused_loss(&b, loss, propagate_opacity_grad, stream);
    }
    *num_rendered = 0;
    if (int e = check_gaussians(a)) return e;
    LossParams lp;
    if (int e = fused_loss_params(a, loss, &lp)) return e;
    if (int e = check_forward(a)) return e;
    // the backward's arguments, checked with the pair CAPACITY standing in for the count (the scratch must hold that many records)
    lvdgs_args bw = *a;
    bw.num_rendered = cap;
    BackwardViews v;
    if (int e = check_backward(&bw, BackwardKind::fused_loss, &v)) return e;
    PairProbe *probe = nullptr;
    if (int e = get_probe(&probe)) return e;
    GeomView g;
    lvdgs_args fw = *a;
    fw.flags |= LVDGS_FLAG_NO_BLEND;   // (grouping and tile sort; the blend follows below, together with the backward's)
    if (int e = enqueue_counted_forward(a, &fw, probe, &g, s)) return e;
    // (both halves of the backward look at the frame's pair count on the device and stand down when it exceeds the capacity)
    // (two-level grouping: and when the super lists' count does -- the tile lists read off them were cut short)
    const bool super = super_tiles_in_use(*a);
    const uint32_t *total_super_dev = super ? g.total + SUPER_TOTAL_WORD : nullptr;
    if (int e = launch_blend_fwd_bwd_fused_loss(*a, v.g, v.b, v.im, v.w, lp, propagate_opacity_grad != 0, probe->longest > 0, g.total, (uint32_t)cap, total_super_dev, s)) return e;
    if (int e = launch_preprocess_bwd(*a, v.g, v.w, v.b.pair_valid, s, g.total, (uint32_t)cap, total_super_dev)) return e;
    bool redo;
    if (int e = finish_counted_forward(a, probe, ", then lvdgs_forward_render and lvdgs_backward_fused_loss", num_rendered, &redo)) return e;
    if (redo) {
        // both passes stood down: the view one-level (enqueue_render_one_level), then the two blend passes and the per-Gaussian pass again
        if (int e = enqueue_render_one_level(&fw, cap, s)) return e;
        if (int e = launch_blend_fwd_bwd_fused_loss(*a, v.g, v.b, v.im, v.w, lp, propagate_opacity_grad != 0, probe->longest > 0, nullptr, 0u, nullptr, s)) return e;
        if (int e = launch_preprocess_bwd(*a, v.g, v.w, v.b.pair_valid, s)) return e;
    }
    return LVDGS_OK;
}

int lvdgs_blend_forward_batch(const lvdgs_args *const *views, int32_t count, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (count < 0 || (count > 0 && !views)) { set_error("blend batch: bad view list"); return LVDGS_E_INVALID; }
    if (count == 0) return LVDGS_OK;
    std::vector<GeomView> g(count); std::vector<BinView> b(count); std::vector<ImageView> im(count);
    for (int k = 0; k < count; k++) {
        const lvdgs_args *a = views[k];
        if (!a) { set_error("blend batch: view %d is NULL", k); return LVDGS_E_INVALID; }
        if (int e = check_common(a)) return e;
        const int64_t D = a->num_gaussians == 0 ? 0 : a->num_rendered;
        if (D < 0) { set_error("negative num_rendered"); return LVDGS_E_INVALID; }
        if (int e = check_render_buffers(a, D)) return e;
        if (!one_frame(a, views[0], 0)) { set_error("blend batch: the views differ in image size or band"); return LVDGS_E_INVALID; }
        g[k] = GeomView{}; b[k] = BinView{};
        if (a->num_gaussians > 0) geom_layout(a->num_gaussians, &g[k], a->geom_state);
        bin_view(a, &b[k]);
        image_layout(a->image_width, a->image_height, &im[k], a->image_state);
    }
    PairProbe *probe = nullptr;
    if (int e = get_probe(&probe)) return e;
    return launch_blend_fwd_batch(views, g.data(), b.data(), im.data(), count, probe->longest > 0, s);
}

// lvdgs_masked_loss_args as the backward reads it
static int masked_loss_view(const lvdgs_args *a, const lvdgs_masked_loss_args *m, MaskedLossView *out) {
    if (!m || !m->d_image || !m->out) { set_error("masked loss backward: loss / d_image / out is NULL"); return LVDGS_E_INVALID; }
    if (m->width != a->image_width || m->height != a->image_height) { set_error("masked loss backward: image size differs from the rasterizer's"); return LVDGS_E_INVALID; }
    if (m->gt_depth && !m->depth) { set_error("masked loss backward: gt_depth without the rendered depth"); return LVDGS_E_INVALID; }
    if (a->tile_row_begin != 0 || a->tile_row_end != 0) { set_error("masked loss backward: the loss is not a sum over pixels, a view scored by it cannot be rendered in bands"); return LVDGS_E_INVALID; }
    *out = MaskedLossView{m->d_image, m->depth, m->gt_depth, m->static_mask, m->depth_lambda, m->out};
    return LVDGS_OK;
}

int lvdgs_backward_masked_loss(const lvdgs_args *a, const lvdgs_masked_loss_args *loss, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("backward: args is NULL"); return LVDGS_E_INVALID; }
    MaskedLossView mv;
    if (int e = masked_loss_view(a, loss, &mv)) return e;
    BackwardViews v;
    if (int e = check_backward(a, BackwardKind::masked_loss, &v)) return e;
    if (v.D > 0 && !(a->flags & LVDGS_FLAG_NO_BLEND))
        if (int e = launch_blend_bwd_masked_loss(*a, v.g, v.b, v.im, v.w, mv, s)) return e;
    return enqueue_gaussian_backward(a, v, s);
}

int lvdgs_blend_backward_window_batch(const lvdgs_args *const *views, const lvdgs_loss_args *const *losses,
                                      const lvdgs_masked_loss_args *const *masked, int32_t count, int32_t propagate_opacity_grad, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (count < 0 || (count > 0 && (!views || (!losses && !masked)))) { set_error("blend batch: bad view list"); return LVDGS_E_INVALID; }
    if (count == 0) return LVDGS_OK;
    std::vector<GeomView> g(count); std::vector<BinView> b(count); std::vector<ImageView> im(count); std::vector<BwdScratch> w(count);
    std::vector<LossParams> lp(count);
    std::vector<MaskedLossView> mv(count); std::vector<const MaskedLossView *> mp(count, nullptr);
    for (int k = 0; k < count; k++) {
        const lvdgs_args *a = views[k];
        const lvdgs_masked_loss_args *m = masked ? masked[k] : nullptr;
        if (!a || (!m && !(losses && losses[k]))) { set_error("blend batch: view %d is NULL or has no loss", k); return LVDGS_E_INVALID; }
        if (!one_frame(a, views[0], LVDGS_FLAG_POSE_ONLY)) { set_error("blend batch: the views differ in image size, band or LVDGS_FLAG_POSE_ONLY"); return LVDGS_E_INVALID; }
        if (m) {
            if (int e = masked_loss_view(a, m, &mv[k])) return e;
            mp[k] = &mv[k];
        } else if (int e = fused_loss_params(a, losses[k], &lp[k])) return e;
        BackwardViews v;
        if (int e = check_backward(a, m ? BackwardKind::masked_loss : BackwardKind::fused_loss, &v)) return e;
        g[k] = v.g; b[k] = v.b; im[k] = v.im; w[k] = v.w;
    }
    return launch_blend_bwd_fused_loss_batch(views, g.data(), b.data(), im.data(), w.data(), lp.data(), masked ? mp.data() : nullptr, count,
                                             propagate_opacity_grad != 0, s);
}

int lvdgs_blend_backward_fused_loss_batch(const lvdgs_args *const *views, const lvdgs_loss_args *const *losses, int32_t count,
                                          int32_t propagate_opacity_grad, void *stream) {
    if (count > 0 && !losses) { set_error("blend batch: bad view list"); return LVDGS_E_INVALID; }
    return lvdgs_blend_backward_window_batch(views, losses, nullptr, count, propagate_opacity_grad, stream);
}

// The per-Gaussian passes of `count` views behind their (batched) backward blend pass, in one launch (include/lvdgs.h).
int lvdgs_gaussian_backward_batch(const lvdgs_args *const *views, int32_t count, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (count < 0 || (count > 0 && !views)) { set_error("gaussian backward batch: bad view list"); return LVDGS_E_INVALID; }
    if (count == 0) return LVDGS_OK;
    std::vector<GeomView> g(count); std::vector<BinView> b(count); std::vector<BwdScratch> w(count);
    const lvdgs_args *a0 = views[0];
    if (!a0) { set_error("gaussian backward batch: view 0 is NULL"); return LVDGS_E_INVALID; }
    for (int k = 0; k < count; k++) {
        const lvdgs_args *a = views[k];
        if (!a) { set_error("gaussian backward batch: view %d is NULL", k); return LVDGS_E_INVALID; }
        if (a->flags & LVDGS_FLAG_POSE_ONLY) { set_error("gaussian backward batch: LVDGS_FLAG_POSE_ONLY makes no parameter gradients"); return LVDGS_E_INVALID; }
        if (a->num_gaussians != a0->num_gaussians || a->means3D != a0->means3D || a->opacities != a0->opacities || a->scales != a0->scales ||
            a->rotations != a0->rotations || a->shs != a0->shs || a->activations != a0->activations || a->dL_dmeans3D != a0->dL_dmeans3D ||
            a->dL_dopacities != a0->dL_dopacities || a->dL_dscales != a0->dL_dscales || a->dL_drotations != a0->dL_drotations || a->dL_dshs != a0->dL_dshs) {
            set_error("gaussian backward batch: the views differ in map or gradient buffers"); return LVDGS_E_INVALID;
        }
        if (!a->shs || a->colors_precomp || a->cov3D_precomp || a->sh_coeffs != 1 || a->sh_degree != 0) {
            set_error("gaussian backward batch: needs SH colours of one coefficient (degree 0) and scales + rotations (the views go through lvdgs_backward_fused_loss / _masked_loss one by one otherwise)");
            return LVDGS_E_INVALID;
        }
        if (k > 0 && !(a->flags & LVDGS_FLAG_ACCUMULATE_PARAM_GRADS)) { set_error("gaussian backward batch: view %d does not carry LVDGS_FLAG_ACCUMULATE_PARAM_GRADS (the views' gradients are summed)", k); return LVDGS_E_INVALID; }
    }
    for (int k = 0; k < count; k++) {
        BackwardViews v;
        if (int e = check_backward(views[k], BackwardKind::blended, &v)) return e;
        g[k] = v.g; b[k] = v.b; w[k] = v.w;
    }
    return launch_preprocess_bwd_views(views, g.data(), w.data(), b.data(), count, s);
}

int lvdgs_mark_visible(int32_t N, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present,
                       void *stream) {
    (void)projmatrix;
    if (N < 0 || (N > 0 && (!means3D || !viewmatrix || !present))) { set_error("bad mark_visible arguments"); return LVDGS_E_INVALID; }
    return launch_mark_visible(N, means3D, viewmatrix, present, (hipStream_t)stream);
}

void lvdgs_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
}
void lvdgs_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    drain_locked();
    g_slots.clear();
}
int lvdgs_profile_read(lvdgs_kernel_time *out, int cap) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    drain_locked();
    int n = 0;
    for (auto &sl : g_slots) {
        if (n >= cap) break;
        memset(&out[n], 0, sizeof(out[n]));
        strncpy(out[n].name, sl.name.c_str(), sizeof(out[n].name) - 1);
        out[n].launches = sl.launches;
        out[n].total_ms = sl.total_ms;
        n++;
    }
    return n;
}

}  // extern "C"
