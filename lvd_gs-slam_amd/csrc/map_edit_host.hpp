// The pure-host half of the map edit (map_edit.hip): argument validation, the column-table checks and the scratch layout.
// No HIP call and no device code in here, so a stand-alone host program can compile and run it (with a set_error of its own).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lvdgs.h"
#include "carve.hpp"
#include "spans.hpp"

namespace lvdgs {

void set_error(const char *fmt, ...);

constexpr int EDIT_THREADS = 256;
constexpr int EDIT_MAX_BLOCKS = 1024;   // spans of the plan's count and write passes
constexpr int EDIT_COUNTERS = 5;        // per span: KEEP rows, CLONE rows, surviving split sources, split sources, clone-stage selections
constexpr int EDIT_SEGMENTS = 4;        // the first four place rows (the write pass scans them); the fifth is only counted

// scratch: [code: one byte per source row][counts: EDIT_MAX_BLOCKS x EDIT_COUNTERS words][totals: 8 words]
struct EditScratch { uint8_t *code; uint32_t *counts, *totals; };
inline size_t edit_layout(int32_t N, EditScratch *v, void *base) {
    Carver<EditScratch> c(v, base);
    c(c.v.code, (size_t)(N > 0 ? N : 0));
    c(c.v.counts, (size_t)EDIT_MAX_BLOCKS * EDIT_COUNTERS);
    c.bytes(c.v.totals, 256);
    return c.off;
}

// the spans of a plan over N rows (spans.hpp)
inline Spans edit_spans(int32_t N) { return make_spans(N, EDIT_THREADS, EDIT_MAX_BLOCKS, EDIT_THREADS); }

inline int edit_check_plan(const lvdgs_map_edit_plan_args *a) {
    if (!a) { set_error("map edit plan: args is NULL"); return LVDGS_E_INVALID; }
    const int32_t N = a->num_gaussians;
    if (N < 0) { set_error("map edit plan: num_gaussians %d", N); return LVDGS_E_RANGE; }
    if (a->mode != LVDGS_EDIT_PRUNE && a->mode != LVDGS_EDIT_DENSIFY) { set_error("map edit plan: mode %d", a->mode); return LVDGS_E_RANGE; }
    if (!a->src || !a->kind || !a->noise_row || !a->host_state || !a->scratch) {
        set_error("map edit plan: src / kind / noise_row / host_state / scratch is NULL"); return LVDGS_E_INVALID;
    }
    const int64_t rows = a->mode == LVDGS_EDIT_DENSIFY ? 2 * (int64_t)N : (int64_t)N;
    if ((int64_t)a->capacity < rows) {
        set_error("map edit plan: capacity %d is below the %lld rows %d Gaussians can give", a->capacity, (long long)rows, N); return LVDGS_E_RANGE;
    }
    if (a->host_bytes < sizeof(int32_t) * ((size_t)LVDGS_EDIT_HOST_SRC + 2 * (size_t)N)) {
        set_error("map edit plan: host_state of %zu bytes is too small for %d Gaussians", a->host_bytes, N); return LVDGS_E_RANGE;
    }
    if (a->mode == LVDGS_EDIT_PRUNE && !a->remove) {
        if (a->num_vis_rows < 0 || a->num_vis_rows > LVDGS_EDIT_MAX_VIS_ROWS) {
            set_error("map edit plan: %d visibility rows (at most %d)", a->num_vis_rows, LVDGS_EDIT_MAX_VIS_ROWS); return LVDGS_E_RANGE;
        }
        if (a->vis_stride != 0 && a->vis_stride != 1 && a->vis_stride != 4 && a->vis_stride != 8) {
            set_error("map edit plan: vis_stride %d (1, 4 or 8)", a->vis_stride); return LVDGS_E_RANGE;
        }
        if (!a->kf_id || !a->n_obs) { set_error("map edit plan: kf_id / n_obs is NULL"); return LVDGS_E_INVALID; }
        for (int k = 0; k < a->num_vis_rows; k++)
            if (!a->vis_rows[k]) { set_error("map edit plan: visibility row %d is NULL", k); return LVDGS_E_INVALID; }
    }
    if (a->mode == LVDGS_EDIT_DENSIFY) {
        if (a->scale_dims != 1 && a->scale_dims != 3) { set_error("map edit plan: scale_dims %d (1 or 3)", a->scale_dims); return LVDGS_E_RANGE; }
        if (!a->grad_accum || !a->denom || !a->scaling || !a->opacity) {
            set_error("map edit plan: grad_accum / denom / scaling / opacity is NULL"); return LVDGS_E_INVALID;
        }
    }
    if (a->scratch_bytes < edit_layout(N, nullptr, nullptr)) { set_error("map edit plan: scratch too small"); return LVDGS_E_INVALID; }
    return LVDGS_OK;
}

inline int edit_check_apply(const lvdgs_map_edit_apply_args *a) {
    if (!a) { set_error("map edit apply: args is NULL"); return LVDGS_E_INVALID; }
    if (a->num_columns < 0 || a->num_columns > LVDGS_EDIT_MAX_COLUMNS) {
        set_error("map edit apply: %d columns (at most %d)", a->num_columns, LVDGS_EDIT_MAX_COLUMNS); return LVDGS_E_RANGE;
    }
    if (a->num_gaussians < 0 || a->n_out < 0 || a->n_split_sel < 0) {
        set_error("map edit apply: num_gaussians %d, n_out %d, n_split_sel %d", a->num_gaussians, a->n_out, a->n_split_sel); return LVDGS_E_RANGE;
    }
    if (!a->src || !a->kind) { set_error("map edit apply: src / kind is NULL"); return LVDGS_E_INVALID; }
    for (int c = 0; c < a->num_columns; c++) {
        const lvdgs_map_edit_column &col = a->columns[c];
        if (!col.in || !col.out) { set_error("map edit apply: column %d: in / out is NULL", c); return LVDGS_E_INVALID; }
        if (col.row_bytes < 1) { set_error("map edit apply: column %d: row_bytes %d", c, col.row_bytes); return LVDGS_E_INVALID; }
        if (col.new_rows < LVDGS_EDIT_COPY || col.new_rows > LVDGS_EDIT_SCALE) {
            set_error("map edit apply: column %d: new_rows %d", c, col.new_rows); return LVDGS_E_INVALID;
        }
        if (col.new_rows == LVDGS_EDIT_XYZ || col.new_rows == LVDGS_EDIT_SCALE) {
            if (a->scale_dims != 1 && a->scale_dims != 3) { set_error("map edit apply: scale_dims %d (1 or 3)", a->scale_dims); return LVDGS_E_RANGE; }
            if (((uintptr_t)col.in | (uintptr_t)col.out) % 4) { set_error("map edit apply: column %d: float rows must be 4-byte aligned", c); return LVDGS_E_INVALID; }
        }
        if (col.new_rows == LVDGS_EDIT_XYZ) {
            if (col.row_bytes != 12) { set_error("map edit apply: column %d: an xyz row has 12 bytes, not %d", c, col.row_bytes); return LVDGS_E_INVALID; }
            if (!a->noise_row || !a->scaling || !a->rotation || (a->n_split_sel > 0 && !a->noise)) {
                set_error("map edit apply: column %d: noise_row / noise / scaling / rotation is NULL", c); return LVDGS_E_INVALID;
            }
        }
        if (col.new_rows == LVDGS_EDIT_SCALE && col.row_bytes != 4 * a->scale_dims) {
            set_error("map edit apply: column %d: a scale row has %d bytes, not %d", c, 4 * a->scale_dims, col.row_bytes); return LVDGS_E_INVALID;
        }
    }
    return LVDGS_OK;
}

}  // namespace lvdgs
