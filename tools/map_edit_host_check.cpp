// Stand-alone host program: the pure-host half of the map edit (csrc/map_edit_host.hpp: argument validation, the column-table checks,
// the scratch layout) for a run under AddressSanitizer and UBSan on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ilvd_gs-slam_amd/csrc tools/map_edit_host_check.cpp -o tools/map_edit_host_check && tools/map_edit_host_check
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
#include "map_edit_host.hpp"
namespace lvdgs { static char last[512]; void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(last, sizeof last, fmt, ap); va_end(ap); } }
using namespace lvdgs;
int main() {
    int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAIL line %d: %s (%s)\n", __LINE__, #cond, last); fails++; } } while (0)
    for (int32_t N : {0, 1, 255, 256, 257, 70001, 262144, 262145, 262400, 262401, 2000000, INT32_MAX}) {
        char *const base = (char *)4096;   // offsets: carved from a fake base, never dereferenced
        EditScratch w;
        const size_t bytes = edit_layout(N, &w, base), counts = (char *)w.counts - base, totals = (char *)w.totals - base;
        EXPECT((char *)w.code == base && bytes == edit_layout(N, nullptr, nullptr));
        EXPECT(counts >= (size_t)N && counts % 256 == 0 && totals % 256 == 0 && bytes > totals);
        EXPECT(totals - counts >= (size_t)EDIT_MAX_BLOCKS * EDIT_COUNTERS * 4);
        const Spans s = edit_spans(N);
        const int blocks = s.blocks; const int64_t span = s.span;
        EXPECT(blocks >= 0 && blocks <= EDIT_MAX_BLOCKS && span >= EDIT_THREADS && span % EDIT_THREADS == 0 && (int64_t)blocks * span >= N);
        if (N > 0) EXPECT((int64_t)(blocks - 1) * span < N);   // no span is empty
        else EXPECT(blocks == 0);
    }
    // the shared geometry with a smallest span above the workgroup (seeding's): 1100 x 960 pixels in 459 spans of 2304, not 512
    { const Spans s = make_spans(1100 * 960, 256, 512, 2048); EXPECT(s.blocks == 459 && s.span == 2304); }
    { const Spans s = make_spans(3000, 256, 512, 2048); EXPECT(s.blocks == 2 && s.span == 2048); }
    EXPECT(span_length(0, 256, 256) == 256 && span_length(65536, 256, 256) == 256 && span_length(65537, 256, 256) == 512);
    std::vector<char> mem(4096);
    lvdgs_map_edit_plan_args a; memset(&a, 0, sizeof a);
    EXPECT(edit_check_plan(nullptr) == LVDGS_E_INVALID);
    a.mode = LVDGS_EDIT_PRUNE; a.num_gaussians = 100; a.capacity = 100;
    a.src = (int32_t *)mem.data(); a.kind = (uint8_t *)mem.data(); a.noise_row = (int32_t *)mem.data(); a.host_state = (int32_t *)mem.data();
    a.scratch = mem.data(); a.remove = (uint8_t *)mem.data(); a.host_bytes = 4 * (LVDGS_EDIT_HOST_SRC + 200); a.scratch_bytes = edit_layout(100, nullptr, nullptr);
    EXPECT(edit_check_plan(&a) == LVDGS_OK);
    a.scratch_bytes--; EXPECT(edit_check_plan(&a) == LVDGS_E_INVALID); a.scratch_bytes++;
    a.host_bytes -= 4; EXPECT(edit_check_plan(&a) == LVDGS_E_RANGE); a.host_bytes += 4;
    a.num_gaussians = INT32_MAX; EXPECT(edit_check_plan(&a) == LVDGS_E_RANGE); a.num_gaussians = 100;
    a.remove = nullptr; a.num_vis_rows = 17; EXPECT(edit_check_plan(&a) == LVDGS_E_RANGE);
    a.num_vis_rows = 16; a.kf_id = (int32_t *)mem.data(); a.n_obs = (int32_t *)mem.data();
    for (int k = 0; k < 15; k++) a.vis_rows[k] = (uint8_t *)mem.data();
    EXPECT(edit_check_plan(&a) == LVDGS_E_INVALID); a.vis_rows[15] = (uint8_t *)mem.data(); EXPECT(edit_check_plan(&a) == LVDGS_OK);
    a.vis_stride = 3; EXPECT(edit_check_plan(&a) == LVDGS_E_RANGE); a.vis_stride = 8; EXPECT(edit_check_plan(&a) == LVDGS_OK);
    a.mode = LVDGS_EDIT_DENSIFY; a.scale_dims = 3; EXPECT(edit_check_plan(&a) == LVDGS_E_RANGE); a.capacity = 200;
    EXPECT(edit_check_plan(&a) == LVDGS_E_INVALID);
    a.grad_accum = a.denom = a.scaling = a.opacity = (float *)mem.data(); EXPECT(edit_check_plan(&a) == LVDGS_OK);
    a.scale_dims = 0; EXPECT(edit_check_plan(&a) == LVDGS_E_RANGE);
    lvdgs_map_edit_apply_args *b = new lvdgs_map_edit_apply_args; memset(b, 0, sizeof *b);
    EXPECT(edit_check_apply(nullptr) == LVDGS_E_INVALID);
    b->num_gaussians = 10; b->n_out = 10; b->scale_dims = 3; b->src = (int32_t *)mem.data(); b->kind = (uint8_t *)mem.data();
    b->num_columns = LVDGS_EDIT_MAX_COLUMNS + 1; EXPECT(edit_check_apply(b) == LVDGS_E_RANGE);
    b->num_columns = LVDGS_EDIT_MAX_COLUMNS;
    for (int c = 0; c < LVDGS_EDIT_MAX_COLUMNS; c++) { b->columns[c].in = mem.data(); b->columns[c].out = mem.data() + 2048; b->columns[c].row_bytes = 1 + c; b->columns[c].new_rows = c & 1; }
    EXPECT(edit_check_apply(b) == LVDGS_OK);
    b->columns[47].row_bytes = 0; EXPECT(edit_check_apply(b) == LVDGS_E_INVALID); b->columns[47].row_bytes = 12;
    b->columns[47].new_rows = LVDGS_EDIT_XYZ; EXPECT(edit_check_apply(b) == LVDGS_E_INVALID);
    b->noise_row = (int32_t *)mem.data(); b->scaling = b->rotation = (float *)mem.data(); EXPECT(edit_check_apply(b) == LVDGS_OK);
    b->n_split_sel = 1; EXPECT(edit_check_apply(b) == LVDGS_E_INVALID); b->noise = (float *)mem.data(); EXPECT(edit_check_apply(b) == LVDGS_OK);
    b->columns[47].in = mem.data() + 1; EXPECT(edit_check_apply(b) == LVDGS_E_INVALID); b->columns[47].in = mem.data();
    b->columns[46].new_rows = LVDGS_EDIT_SCALE; b->columns[46].row_bytes = 4; EXPECT(edit_check_apply(b) == LVDGS_E_INVALID);
    b->columns[46].row_bytes = 12; EXPECT(edit_check_apply(b) == LVDGS_OK);
    delete b;
    printf(fails ? "%d FAILED\n" : "host checks ok (%d failures)\n", fails);
    return fails != 0;
}
