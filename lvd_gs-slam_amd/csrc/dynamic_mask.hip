// From the detector's boxes and the segmenter's masks to the masks the loops consume, as one call with no host wait inside it
// (semantics: include/lvdgs.h): EnhancedDynamicObjectMasker.detect_and_segment after its two networks
// (reference utils/slam_frontend.py:906-1056), _temporal_consistency (:1168-1182), FrontEnd._expand_dynamic_mask (:1260-1266) and
// add_new_keyframe's valid_rgb / masked depth (:1290-1323, :1367-1369).
//
// Every mask is held as one bit per pixel: a row is ceil(width / 64) 64-bit words, bit b of word w is column 64 w + b, the bits past
// the last column are zero.  A word is one __ballot of a wave that reads 64 bytes; boxes are filled per word, dilation is shifts
// across the neighbouring words and an OR over the rows, the history's majority is a bit-sliced count, counts are __popcll.  Bytes
// appear only in the final stores.
//
// Launches, all enqueued at once (their number depends on expand_kernel alone: never on the boxes, on use_sam_result, or on the history):
//   a clear of the 16 info words
// ("a wave per word": up to 1024 workgroups of four waves walk the words with the grid's stride; a wave's counts leave it once)
//   dm_build_kernel    a wave per word: the box mask (the boxes shared out among the lanes, OR-ed over the wave) and the union of the
//                      segmenter's masks; their pixel counts, the surviving boxes, vehicle_detected
//   dm_select_kernel   a thread per word: use_sam_result from the union's count, final := union or boxes; the temporal filter -- the
//                      word goes into the ring, the majority over the ring's planes comes out -- when the frame is not first and no
//                      segmenter result is used
//   dm_vehicle_kernel  a wave per word: the vehicle dilation when vehicle_detected; dynamic_mask / static_mask bytes and counts; one
//                      thread moves the history's header on (every reader of it ran in the launch before)
//   dm_expand_kernel   (expand_kernel != 0) a wave per word: the keyframe's dilation; expanded_* / valid_rgb bytes, the masked depth, counts
#include "bitplane.hpp"

namespace lvdgs {
namespace {

constexpr int DM_THREADS = 256;
constexpr int DM_WAVES = DM_THREADS / WAVE;
constexpr int DM_MAX_BLOCKS = 1024;      // of the wave-per-word kernels: a wave walks the words with the grid's stride, its counts leave once
constexpr int DM_MAX_KERNEL = BITPLANE_MAX_KERNEL;   // dilation windows: odd, up to this (bitplane.hpp)
constexpr int DM_MAX_HISTORY = 8;        // a 4-bit count per pixel
constexpr size_t DM_HEADER_BYTES = 256;

struct DmHeader {                        // the persistent history's first words; all zero: empty
    int32_t width, height, history_length, length, head;
};

struct DmParams {
    int W, H, wpr;                       // wpr: words per row
    int64_t words;                       // H * wpr
    int first, box_format, num_boxes, num_sam, history_length, vehicle_k, expand_k;
    float thr;                           // (float)rgb_boundary_threshold
    const float *boxes;
    const uint8_t *vehicle, *sam;
    const float *image, *depth_in;
    float *depth_out;
    uint8_t *static_mask, *dynamic_mask, *expanded_dynamic, *expanded_static, *valid_rgb;
    int32_t *info;
    DmHeader *header;
    uint64_t *ring;                      // history_length planes of `words` words
    uint64_t *plane0, *plane1;           // scratch: boxes, then final (in place) | the union, then dynamic
};

__device__ __forceinline__ uint64_t valid_bits(const DmParams &P, int wx) { return row_valid_bits(P.W, wx); }

// A box as the reference's statements leave it: x1, y1 inclusive, x2, y2 exclusive; false when it is dropped.
__device__ __forceinline__ bool box_rect(const DmParams &P, int b, int &x1, int &y1, int &x2, int &y2, bool &veh) {
    float f0 = P.boxes[4 * (int64_t)b], f1 = P.boxes[4 * (int64_t)b + 1], f2 = P.boxes[4 * (int64_t)b + 2], f3 = P.boxes[4 * (int64_t)b + 3];
    if (P.box_format == LVDGS_DYNAMIC_MASK_BOXES_CXCYWH) {   // GroundingDINODetector.detect (:364-382), float32 in its order
        const float w = (float)P.W, h = (float)P.H;
        const float cx = f0 * w, cy = f1 * h, bw = f2 * w, bh = f3 * h;
        const float hw = bw / 2.0f, hh = bh / 2.0f;
        f0 = fminf(fmaxf(cx - hw, 0.0f), w);
        f1 = fminf(fmaxf(cy - hh, 0.0f), h);
        f2 = fminf(fmaxf(cx + hw, 0.0f), w);
        f3 = fminf(fmaxf(cy + hh, 0.0f), h);
    }
    // astype(int): toward zero (the conversion saturates; the clamps below bring anything into the frame)
    const long long i0 = (long long)f0, i1 = (long long)f1, i2 = (long long)f2, i3 = (long long)f3;
    const long long xm = P.W - 1, ym = P.H - 1;
    x1 = (int)max(0ll, min(i0, xm)); y1 = (int)max(0ll, min(i1, ym));
    x2 = (int)max(0ll, min(i2, xm)); y2 = (int)max(0ll, min(i3, ym));
    veh = false;
    if (x2 <= x1 || y2 <= y1) return false;
    veh = P.vehicle && P.vehicle[b] != 0;
    if (veh) {
        const double r = P.first ? 0.15 : 0.1;
        const int ew = (int)((double)(x2 - x1) * r), eh = (int)((double)(y2 - y1) * r);
        x1 = max(0, x1 - ew); y1 = max(0, y1 - eh);
        x2 = min(P.W, x2 + ew); y2 = min(P.H, y2 + eh);
    }
    return true;
}

// (the block-wide sums into info: add_counts of bitplane.hpp; at most DM_MAX_BLOCKS blocks meet on a word of info)
__global__ void __launch_bounds__(DM_THREADS) dm_build_kernel(DmParams P) {
    const int lane = threadIdx.x % WAVE;
    const int64_t n = (int64_t)P.W * P.H;
    uint32_t v[2] = {0, 0};
    for (int64_t word = (int64_t)blockIdx.x * DM_WAVES + threadIdx.x / WAVE; word < P.words; word += (int64_t)gridDim.x * DM_WAVES) {   // (wave-uniform)
        const int y = (int)(word / P.wpr), wx = (int)(word - (int64_t)y * P.wpr);
        const int x = wx * 64 + lane;
        const bool in = x < P.W;
        const int64_t o = (int64_t)y * P.W + x;
        uint8_t any = 0;
        for (int m = 0; m < P.num_sam; m++) any |= in ? P.sam[(int64_t)m * n + o] : (uint8_t)0;
        const uint64_t sam_word = __ballot(any != 0);
        uint64_t mine = 0;
        uint32_t kept = 0, vehicles = 0;
        for (int base = 0; base < P.num_boxes; base += WAVE) {   // (uniform: whole waves reach the ballots)
            const int b = base + lane;
            int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
            bool veh = false;
            const bool ok = b < P.num_boxes && box_rect(P, b, x1, y1, x2, y2, veh);
            if (word == 0) {
                kept += (uint32_t)__popcll(__ballot(ok));
                vehicles += (uint32_t)__popcll(__ballot(ok && veh));
            }
            if (ok && y >= y1 && y < y2) {
                const int lo = max(x1 - wx * 64, 0), hi = min(x2 - wx * 64, 64);
                if (hi > lo) mine |= low_bits(hi) & ~low_bits(lo);
            }
        }
        const uint64_t box_word = wave_or(mine, WAVE);
        if (lane == 0) {
            P.plane0[word] = box_word;
            P.plane1[word] = sam_word;
            if (word == 0) {
                P.info[LVDGS_DYNAMIC_MASK_INFO_BOXES] = (int32_t)kept;
                P.info[LVDGS_DYNAMIC_MASK_INFO_VEHICLE] = vehicles != 0;
            }
        }
        v[0] += (uint32_t)__popcll(box_word);
        v[1] += (uint32_t)__popcll(sam_word);
    }
    const int slot[2] = {LVDGS_DYNAMIC_MASK_INFO_BOX_PIXELS, LVDGS_DYNAMIC_MASK_INFO_SAM_PIXELS};
    add_counts<2>(P.info, slot, v, lane == 0);
}

// The history as the header describes it, brought into range whatever the bytes are: a block of another frame size or ring
// length -- a zeroed block among them -- is an empty history.
struct DmHistory { int length, head; };
__device__ __forceinline__ DmHistory read_history(const DmParams &P) {
    const DmHeader h = *P.header;
    const bool same = h.width == P.W && h.height == P.H && h.history_length == P.history_length;
    DmHistory s;
    s.length = same ? min(max(h.length, 0), P.history_length) : 0;
    s.head = same ? min(max(h.head, 0), P.history_length - 1) : 0;
    return s;
}
// ... and after _temporal_consistency's append: the slot the new entry takes is returned
__device__ __forceinline__ int append_history(const DmParams &P, DmHistory &s) {
    if (s.length < P.history_length) return (s.head + s.length++) % P.history_length;
    const int slot = s.head;             // the oldest entry goes
    s.head = (s.head + 1) % P.history_length;
    return slot;
}

__global__ void __launch_bounds__(DM_THREADS) dm_select_kernel(DmParams P) {
    const int64_t word = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    const bool use_sam = P.info[LVDGS_DYNAMIC_MASK_INFO_SAM_PIXELS] > 0;
    const bool filter = !P.first && !use_sam;
    DmHistory s = read_history(P);
    const int slot = filter ? append_history(P, s) : 0;
    if (word == 0) {
        P.info[LVDGS_DYNAMIC_MASK_INFO_USE_SAM] = use_sam;
        P.info[LVDGS_DYNAMIC_MASK_INFO_FILTERED] = filter;
        P.info[LVDGS_DYNAMIC_MASK_INFO_HISTORY] = s.length;
    }
    if (word >= P.words) return;
    uint64_t final_word = use_sam ? P.plane1[word] : P.plane0[word];
    if (filter) {
        P.ring[(int64_t)slot * P.words + word] = final_word;
        if (s.length >= 3) {
            // set in more than length / 2 of the entries: a 4-bit count per bit position, compared with length / 2 + 1 from the top bit down
            uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
            for (int j = 0; j < s.length; j++) {
                const int e = (s.head + j) % P.history_length;
                uint64_t carry = e == slot ? final_word : P.ring[(int64_t)e * P.words + word];
                uint64_t t = c0 & carry; c0 ^= carry; carry = t;
                t = c1 & carry; c1 ^= carry; carry = t;
                t = c2 & carry; c2 ^= carry; carry = t;
                c3 ^= carry;
            }
            const int need = s.length / 2 + 1;
            const uint64_t c[4] = {c0, c1, c2, c3};
            uint64_t greater = 0, equal = ~0ull;
            for (int b = 3; b >= 0; b--) {
                const uint64_t tb = ((need >> b) & 1) ? ~0ull : 0ull;
                greater |= equal & c[b] & ~tb;
                equal &= ~(c[b] ^ tb);
            }
            final_word = greater | equal;
        }
    }
    P.plane0[word] = final_word;
}

// Word (y, wx) of `plane` dilated by a k x k window of ones (bitplane.hpp).  All lanes return the word.
__device__ __forceinline__ uint64_t dilate_word(const DmParams &P, const uint64_t *plane, int y, int wx, int k, int lane) {
    return lvdgs::dilate_word(plane, P.W, P.H, P.wpr, y, wx, k, lane);
}

__global__ void __launch_bounds__(DM_THREADS) dm_vehicle_kernel(DmParams P) {
    const int lane = threadIdx.x % WAVE;
    const bool veh = P.info[LVDGS_DYNAMIC_MASK_INFO_VEHICLE] != 0;
    uint32_t v[2] = {0, 0};
    for (int64_t word = (int64_t)blockIdx.x * DM_WAVES + threadIdx.x / WAVE; word < P.words; word += (int64_t)gridDim.x * DM_WAVES) {
        const int y = (int)(word / P.wpr), wx = (int)(word - (int64_t)y * P.wpr);
        const uint64_t d = veh ? dilate_word(P, P.plane0, y, wx, P.vehicle_k, lane) : P.plane0[word];
        const int x = wx * 64 + lane;
        if (x < P.W) {
            const int64_t o = (int64_t)y * P.W + x;
            const uint8_t bit = (uint8_t)((d >> lane) & 1ull);
            if (P.dynamic_mask) P.dynamic_mask[o] = bit;
            if (P.static_mask) P.static_mask[o] = (uint8_t)(1 - bit);
        }
        if (lane == 0) P.plane1[word] = d;
        const uint32_t set = (uint32_t)__popcll(d);
        v[0] += set;
        v[1] += (uint32_t)__popcll(valid_bits(P, wx)) - set;
        if (word == 0 && lane == 0) {      // the history's header: dm_select_kernel's statements again, for the next call
            DmHistory s = read_history(P);
            if (!P.first && P.info[LVDGS_DYNAMIC_MASK_INFO_USE_SAM] == 0) append_history(P, s);
            DmHeader h;
            h.width = P.W; h.height = P.H; h.history_length = P.history_length; h.length = s.length; h.head = s.head;
            *P.header = h;
        }
    }
    const int slot[2] = {LVDGS_DYNAMIC_MASK_INFO_DYNAMIC_PIXELS, LVDGS_DYNAMIC_MASK_INFO_STATIC_PIXELS};
    add_counts<2>(P.info, slot, v, lane == 0);
}

__global__ void __launch_bounds__(DM_THREADS) dm_expand_kernel(DmParams P) {
    const int lane = threadIdx.x % WAVE;
    const int64_t n = (int64_t)P.W * P.H;
    uint32_t v[3] = {0, 0, 0};
    for (int64_t word = (int64_t)blockIdx.x * DM_WAVES + threadIdx.x / WAVE; word < P.words; word += (int64_t)gridDim.x * DM_WAVES) {
        const int y = (int)(word / P.wpr), wx = (int)(word - (int64_t)y * P.wpr);
        const uint64_t e = dilate_word(P, P.plane1, y, wx, P.expand_k, lane);
        const int x = wx * 64 + lane;
        bool valid = false, deep = false;
        if (x < P.W) {
            const int64_t o = (int64_t)y * P.W + x;
            const uint8_t bit = (uint8_t)((e >> lane) & 1ull);
            if (P.expanded_dynamic) P.expanded_dynamic[o] = bit;
            if (P.expanded_static) P.expanded_static[o] = (uint8_t)(1 - bit);
            valid = ((P.image[o] + P.image[n + o]) + P.image[2 * n + o]) > P.thr && !bit;
            if (P.valid_rgb) P.valid_rgb[o] = valid;
            if (P.depth_in) {
                const float d = valid ? P.depth_in[o] : 0.0f;
                if (P.depth_out) P.depth_out[o] = d;
                deep = d > 0.0f;
            }
        }
        v[0] += (uint32_t)__popcll(e);
        v[1] += (uint32_t)__popcll(__ballot(valid));
        v[2] += (uint32_t)__popcll(__ballot(deep));
    }
    const int slot[3] = {LVDGS_DYNAMIC_MASK_INFO_EXPANDED_PIXELS, LVDGS_DYNAMIC_MASK_INFO_VALID_PIXELS, LVDGS_DYNAMIC_MASK_INFO_DEPTH_PIXELS};
    add_counts<3>(P.info, slot, v, lane == 0);
}

// the state: the header, the ring of the last history_length dynamic masks
size_t dm_state_layout(int W, int H, int history_length, DmParams *P, void *base) {
    Carver<DmParams> c(P, base);
    c.bytes(c.v.header, DM_HEADER_BYTES); c.bytes(c.v.ring, (size_t)history_length * plane_bytes(W, H));
    return c.off;
}

// the scratch: two bit planes
size_t dm_scratch_layout(int W, int H, DmParams *P, void *base) {
    Carver<DmParams> c(P, base);
    c.bytes(c.v.plane0, plane_bytes(W, H)); c.bytes(c.v.plane1, plane_bytes(W, H));
    return c.off;
}

}  // namespace
}  // namespace lvdgs

using namespace lvdgs;

extern "C" {

size_t lvdgs_dynamic_mask_state_bytes(int32_t width, int32_t height, int32_t history_length) {
    if (width < 1 || height < 1 || (int64_t)width * height > INT32_MAX || history_length < 1 || history_length > DM_MAX_HISTORY) return 0;
    return dm_state_layout(width, height, history_length, nullptr, nullptr);
}

size_t lvdgs_dynamic_mask_scratch_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1 || (int64_t)width * height > INT32_MAX) return 0;
    return dm_scratch_layout(width, height, nullptr, nullptr);
}

int lvdgs_dynamic_mask(const lvdgs_dynamic_mask_args *a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!a) { set_error("dynamic mask: args is NULL"); return LVDGS_E_INVALID; }
    if (a->width < 1 || a->height < 1 || (int64_t)a->width * a->height > INT32_MAX) {
        set_error("dynamic mask: image size %dx%d (at least 1x1, at most 2^31 - 1 pixels)", a->width, a->height); return LVDGS_E_RANGE;
    }
    if (a->num_boxes < 0 || a->num_sam_masks < 0) {
        set_error("dynamic mask: num_boxes %d / num_sam_masks %d is negative", a->num_boxes, a->num_sam_masks); return LVDGS_E_RANGE;
    }
    if (a->history_length < 1 || a->history_length > DM_MAX_HISTORY) {
        set_error("dynamic mask: history_length %d, outside 1..%d", a->history_length, DM_MAX_HISTORY); return LVDGS_E_RANGE;
    }
    if (a->box_format != LVDGS_DYNAMIC_MASK_BOXES_XYXY && a->box_format != LVDGS_DYNAMIC_MASK_BOXES_CXCYWH) {
        set_error("dynamic mask: box_format %d is neither LVDGS_DYNAMIC_MASK_BOXES_XYXY nor LVDGS_DYNAMIC_MASK_BOXES_CXCYWH", a->box_format);
        return LVDGS_E_INVALID;
    }
    if (!odd_kernel(a->vehicle_kernel_first) || !odd_kernel(a->vehicle_kernel)) {
        set_error("dynamic mask: vehicle kernels %d / %d (odd sizes from 1 to %d)", a->vehicle_kernel_first, a->vehicle_kernel, DM_MAX_KERNEL);
        return LVDGS_E_INVALID;
    }
    if (a->expand_kernel != 0 && !odd_kernel(a->expand_kernel)) {
        set_error("dynamic mask: expand_kernel %d (0, or an odd size from 1 to %d)", a->expand_kernel, DM_MAX_KERNEL); return LVDGS_E_INVALID;
    }
    if (!a->state || !a->scratch || !a->info) { set_error("dynamic mask: state / scratch / info is NULL"); return LVDGS_E_INVALID; }
    if (a->num_boxes > 0 && !a->boxes) { set_error("dynamic mask: boxes is NULL"); return LVDGS_E_INVALID; }
    if (a->num_sam_masks > 0 && !a->sam_masks) { set_error("dynamic mask: sam_masks is NULL"); return LVDGS_E_INVALID; }
    if (a->expand_kernel != 0 && !a->image) { set_error("dynamic mask: image is NULL (expand_kernel %d)", a->expand_kernel); return LVDGS_E_INVALID; }
    if (a->depth_out && !a->depth_in) { set_error("dynamic mask: depth_out without depth_in"); return LVDGS_E_INVALID; }
    DmParams P{};
    if (a->state_bytes < dm_state_layout(a->width, a->height, a->history_length, &P, a->state)) {
        set_error("dynamic mask: state too small"); return LVDGS_E_INVALID;
    }
    if (a->scratch_bytes < dm_scratch_layout(a->width, a->height, &P, a->scratch)) { set_error("dynamic mask: scratch too small"); return LVDGS_E_INVALID; }
    P.W = a->width; P.H = a->height; P.wpr = words_per_row(P.W);
    P.words = (int64_t)P.H * P.wpr;
    P.first = a->first_frame != 0; P.box_format = a->box_format;
    P.num_boxes = a->num_boxes; P.num_sam = a->num_sam_masks; P.history_length = a->history_length;
    P.vehicle_k = P.first ? a->vehicle_kernel_first : a->vehicle_kernel;
    P.expand_k = a->expand_kernel;
    P.thr = (float)a->rgb_boundary_threshold;
    P.boxes = a->boxes; P.vehicle = a->vehicle; P.sam = a->sam_masks;
    P.image = a->image; P.depth_in = a->depth_in; P.depth_out = a->depth_out;
    P.static_mask = a->static_mask; P.dynamic_mask = a->dynamic_mask;
    P.expanded_dynamic = a->expanded_dynamic; P.expanded_static = a->expanded_static; P.valid_rgb = a->valid_rgb;
    P.info = a->info;
    const int wave_blocks = (int)min((int64_t)cdiv(P.words, DM_WAVES), (int64_t)DM_MAX_BLOCKS), thread_blocks = cdiv(P.words, DM_THREADS);
    if (int e = check_hip(hipMemsetAsync(a->info, 0, LVDGS_DYNAMIC_MASK_INFO_WORDS * sizeof(int32_t), s), "dynamic mask: clearing info")) return e;
    if (int e = launch("dm_build", 0, s, dm_build_kernel, dim3(wave_blocks), dim3(DM_THREADS), 0, P)) return e;
    if (int e = launch("dm_select", 0, s, dm_select_kernel, dim3(thread_blocks), dim3(DM_THREADS), 0, P)) return e;
    if (int e = launch("dm_vehicle", 0, s, dm_vehicle_kernel, dim3(wave_blocks), dim3(DM_THREADS), 0, P)) return e;
    if (P.expand_k != 0) {
        if (int e = launch("dm_expand", 0, s, dm_expand_kernel, dim3(wave_blocks), dim3(DM_THREADS), 0, P)) return e;
    }
    return LVDGS_OK;
}

}  // extern "C"
