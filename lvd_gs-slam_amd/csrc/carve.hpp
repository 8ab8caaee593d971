// The layout of a caller-provided scratch or state buffer, stated once: a `*_layout(dims, View *, base)` function carves the arrays
// of a view out of the buffer in their order, and returns the bytes the buffer needs.  The public lvdgs_*_bytes function calls it
// with no view and no buffer, the entry point with its view (often the kernels' parameter struct) and the caller's buffer -- the
// size asked for and the pointers bound cannot disagree.  Pure host code, no HIP include (as map_edit_host.hpp).
#pragma once
#include <stddef.h>

namespace lvdgs {

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// Carves the arrays of a view out of a buffer, every one aligned to 256 bytes (no view: into one of its own; no buffer: null
// pointers, sizes only).  No allocation: a layout function runs on every call of its entry point.
template <typename V>
struct Carver {
    V own, &v;
    char *base;
    size_t off = 0;
    Carver(V *view, void *buffer) : v(view ? *view : own), base((char *)buffer) {}
    // `count` elements
    template <typename T>
    void operator()(T *&ptr, size_t count) { bytes(ptr, count * sizeof(T)); }
    // a run of `n` bytes: a header struct, an array with a tail behind it
    template <typename T>
    void bytes(T *&ptr, size_t n) {
        ptr = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += align256(n);
    }
};

}  // namespace lvdgs
