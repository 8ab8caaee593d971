// What the mesh and TSDF entry points refuse alike, in `name`'s words: counts, views, outputs that alias.  Pure host code, no HIP
// include (as carve.hpp), so a stand-alone host program can compile and run it (with a set_error of its own).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lvdgs.h"

namespace lvdgs {

void set_error(const char *fmt, ...);

// a count the kernels index in 32 bits
inline bool count_ok(int64_t n) { return n >= 0 && n <= (int64_t)INT32_MAX; }

// View v of a call's list: there, of 1 .. 2^31 - 1 pixels, with its pose -- and its depth plane where the caller needs one.
inline int check_view(const char *name, int v, const lvdgs_tsdf_view *w, bool needs_depth) {
    if (!w) { set_error("%s: view %d is NULL", name, v); return LVDGS_E_INVALID; }
    if (w->width < 1 || w->height < 1 || (int64_t)w->width * w->height > INT32_MAX) {
        set_error("%s: view %d: image size %dx%d", name, v, w->width, w->height); return LVDGS_E_RANGE;
    }
    if (!w->R || !w->T || (needs_depth && !w->depth)) { set_error("%s: view %d: R / T%s is NULL", name, v, needs_depth ? " / depth" : ""); return LVDGS_E_INVALID; }
    return LVDGS_OK;
}

// A named run of a caller's bytes; v >= 0: the one of view v, "what[v]".  NULL or empty: overlaps nothing.
struct ByteRange { char name[24]; const void *p; size_t bytes; };
inline ByteRange byte_range(const char *what, int v, const void *p, size_t bytes) {
    ByteRange r{};
    if (v < 0) snprintf(r.name, sizeof(r.name), "%s", what);
    else snprintf(r.name, sizeof(r.name), "%s[%d]", what, v);
    r.p = p; r.bytes = bytes;
    return r;
}
inline bool overlap(const ByteRange &a, const ByteRange &b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// No output overlaps an input (the scratch is one of them) or an earlier output.
inline int check_no_overlap(const char *name, const ByteRange *in, int ni, const ByteRange *out, int no) {
    for (int o = 0; o < no; o++) {
        for (int i = 0; i < ni; i++)
            if (overlap(out[o], in[i])) { set_error("%s: %s overlaps %s", name, out[o].name, in[i].name); return LVDGS_E_INVALID; }
        for (int q = 0; q < o; q++)
            if (overlap(out[o], out[q])) { set_error("%s: %s overlaps %s", name, out[o].name, out[q].name); return LVDGS_E_INVALID; }
    }
    return LVDGS_OK;
}

}  // namespace lvdgs
