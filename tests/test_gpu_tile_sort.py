"""The tile depth sort (csrc/tilesort.hip) at every size class, boundary and hint state.

Which code sorts a tile's segment depends on its length, on the grid and on a per-thread hint (what the previous frames on the thread
queued: csrc/api.hip, PairProbe).  The scenes of tests/tile_sort_cases.py put a segment on both sides of every boundary -- 256/257,
512/513, 1024/1025, 2048/2049, 16384/16385 -- and the tests script the hint: every sequence of frames runs in a thread of its own,
which starts with no expectation whatever ran before.  The four states and who sorts what in each:

    state  expectation                       (1024, 2048] sorted by                      > 2048 sorted by
    a      0 (nothing queued lately)         last workgroups, LDS                        last workgroups, global memory
    b      1025..2048                        head workgroups, four waves in registers    last workgroups, global memory
    c      > 2048                            head workgroups                             tile_depth_sort_long_kernel
    d      -1 (unknown)                      last workgroups, LDS                        tile_depth_sort_long_kernel

(d: lvdgs_forward_render, which is given no hint, and a thread's first frame with LVDGS_FLAG_SUPER_TILES.)

On the counting path a segment's ids reach point_list only through its sort, so a length that falls between two launches' ranges is
never written: every buffer is allocated zero-filled, and such a segment shows up as a list of zeros.

After every call num_rendered, tiles_touched, ranges and point_list must equal the float32 oracle's, bit for bit; colour, depth,
opacity and n_touched of a scene must be the same bits in every hint state, through every entry point and with and without
LVDGS_FLAG_LIST_ALL_TILES.  There is no tolerance in this file.

The library's launch profile (lvdgs_profile_*) is global to the process and guarded by a mutex, so it counts the launches of a call
made on another thread: each call's count of "tile_sort_long" launches is asserted against the table, through a host-side restatement
of the hint rule (``Hints``), and the scripted sequences assert the states they mean to reach -- a change of the rule fails these tests
instead of emptying them.  In every state every length has exactly one owner, so a list that is right was sorted by that owner.

What reaches which branch (FULL = 0, 1, 2, 3, 63, 64, 65, 255..257, 511..513, 1023..1025, 2047..2049, 4095..4097, 16383..16385, 20000;
"small" = 160 x 160, "large" = 1040 x 1040, "radix" = 2064 x 2064):

  tile_depth_sort_wave_body
    head workgroups, four waves with 8 keys per lane   1025, 2047, 2048 in states b and c: every_hint_state frames 2-5, batch (c),
                                                       super4 (c); more_segments_than_head_workgroups: 80 segments of 1025..2048 on
                                                       64 workgroups (a workgroup sorts two in turn); longer segments are passed over
    solo workgroups, 2 / 4 keys per lane               257, 511, 512 / 513, 1023, 1024: every test on small, the super lists, the batch;
                                                       every other length leaves at once
    one wave: 0 or 1 entry                             0, 1 (1: "the id must land") on every grid
    one wave: 4 keys per lane                          2, 3, 63, 64, 65, 255, 256 on every grid
    one wave: 8 / 16 keys per lane                     257, 511, 512 / 513, 1023, 1024 on large and radix (small: the solo workgroups')
    one wave queues the segment (radix path)           1025..20000 on radix
    last workgroups                                    -> sort_queued_segments
  sort_queued_segments (the launch's 256 last workgroups)
    LDS                                                1025, 2047, 2048 in states a and d: every_hint_state frames 1 and 6,
                                                       nothing_expected, super4 frame 1; more_segments_than_last_workgroups: 260 on 256
    global memory, keys in place                       2049..20000 in states a and b: nothing_expected frame 2, every_hint_state frame 3,
                                                       batch (a), band (a); super1 frame 4 (b: lists of 6658..55714)
    global memory, keys gathered                       unreachable: the last workgroups exist on the counting path only, whose keys are ready
    not theirs (take_from / take_upto)                 b: 1025..2048; c: everything; d: beyond 2048
  tile_depth_sort_long_kernel
    LDS, keys ready                                    2049..16384 in states c and d: every_hint_state frames 4-6, batch (c), band (c),
                                                       super4 frames 1-2; more_segments_than_long_kernel_workgroups: 260 on 256
    global memory, keys ready                          16385, 20000 in states c and d (the same frames); super1 frames 1-2: 22590, 55714
    LDS / global memory, keys gathered                 1025..16384 / 16385, 20000 on radix (done_below = 0)
    done before (done_below)                           1025..2048 in states c and d
  launch_tile_depth_sort                               counting path in states a-d, small (tile order, solo workgroups) and large;
                                                       radix path; the super lists' call; a band of rows; the 32-frame memory of the hint
  launch_tile_depth_sort_batch                         tile lists in states a and c; super lists in states d and c"""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import tile_sort_cases as tc

pytestmark = pytest.mark.gpu

LONG_LAUNCHES = {"a": 0, "b": 0, "c": 1, "d": 1}      # tile_depth_sort_long_kernel launches behind a tile sort
COUNTING_MAX_TILES = 16384
SLACK = 4096                                          # pair capacity beyond the count (single-call forward)


def _state(expectation):
    if expectation < 0:
        return "d"
    return "a" if expectation <= tc.WAVE_LIMIT else "b" if expectation <= tc.GROUP_LIMIT else "c"


def _longest_queued(lengths):
    m = int(np.max(lengths)) if len(lengths) else 0
    return m if m > tc.WAVE_LIMIT else 0


class Hints:
    """What a fresh thread's calls expect, restated from csrc/api.hip (PairProbe::fold_hints): the longest queued segment of a frame
    raises the expectation at once and lowers it only after 32 frames without one as long; the super-tile lists' expectation is the
    previous super-tile frame's, unknown (-1) before the first."""

    def __init__(self):
        self.longest, self.keep, self.longest_super = 0, 0, -1

    def fold(self, tile_lengths, super_lengths=None):
        l = _longest_queued(tile_lengths)
        if l >= self.longest or self.keep == 0:
            self.longest, self.keep = l, (32 if l else 0)
        else:
            self.keep -= 1
        if super_lengths is not None:
            self.longest_super = _longest_queued(super_lengths)


def in_fresh_thread(fn):
    """fn() on a thread of its own -- the library's hints are per thread -- with its exception re-raised here."""
    box = {}

    def run():
        try:
            box["result"] = fn()
        except BaseException as e:   # noqa: BLE001  (re-raised in the caller)
            box["error"] = e

    th = threading.Thread(target=run)
    th.start()
    th.join()
    if "error" in box:
        raise box["error"]
    return box.get("result")


_MAPS = {}      # case -> its Gaussians on the device
_IMAGES = {}    # (case, shift, band) -> the first call's colour, depth, opacity, n_touched (host copies): every later call must give the same bits


def _device_map(name):
    if name not in _MAPS:
        g, _ = tc.scene(name)
        _MAPS[name] = {k: v.cuda().contiguous() for k, v in g.items()}
    return _MAPS[name]


def _camera(name, shift):
    _, W, H, _, _ = tc.CASES[name]
    _, cam = tc.scene(name)
    return tc.shifted_camera(cam, W, H, shift) if shift else cam


def _describe_wrong_tiles(ranges, got, want):
    wrong = []
    for t in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        b, e = int(ranges[t, 0]), int(ranges[t, 1])
        if not np.array_equal(got[b:e], want[b:e]):
            seg = got[b:e]
            wrong.append(f"tile {int(t)}: {e - b} entries, {int((seg == 0).sum())} zeros, {int((seg != want[b:e]).sum())} differ")
    return "; ".join(wrong[:12])


class Session:
    """The calls of one thread: every frame through the raw C ABI with zero-filled buffers of its own, compared with the oracle, its
    long-segment launches counted and compared with the table."""

    def __init__(self):
        from lvdgs import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.dev = torch.device("cuda")
        self.bg = torch.zeros(3, device=self.dev)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.hints = Hints()
        self.states = []     # of the tile sort of every call so far
        self.keep = []

    # ---- one view's buffers and what they must hold ----
    def _view(self, name, cap, flags=0, shift=0, band=None):
        import c_abi_views
        _, W, H, _, _ = tc.CASES[name]
        a, st = c_abi_views.forward_view(self.L, _device_map(name), _camera(name, shift), W, H, self.bg, cap)
        a.flags = flags
        if band:
            a.tile_row_begin, a.tile_row_end = band
            for k in ("color", "depth", "opacity"):
                st[k].fill_(7.0)
        self.keep = self.keep[-6:] + [st]
        return a, st

    def _super_in_use(self, name, flags, band):
        _, W, H, _, _ = tc.CASES[name]
        T = (W // tc.TILE) * (H // tc.TILE)
        return bool(flags & self.lib.FLAG_SUPER_TILES) and not (flags & self.lib.FLAG_LIST_ALL_TILES) and not band and 64 <= T <= COUNTING_MAX_TILES

    def _check(self, name, st, cap, D, shift=0, band=None):
        import c_abi_views
        _, W, H, _, _ = tc.CASES[name]
        ref = tc.reference(name, shift)
        N = ref["radii"].shape[0]
        gx = W // tc.TILE
        if band is None:
            assert D == ref["num_rendered"]
            touched, ranges, plist = c_abi_views.read_lists(self.L, st, N, cap, W, H, D)
            np.testing.assert_array_equal(st["radii"].cpu().numpy(), ref["radii"])
            np.testing.assert_array_equal(touched, ref["tiles_touched"])
            np.testing.assert_array_equal(ranges, ref["ranges"])
            assert np.array_equal(plist, ref["ids_sorted"]), _describe_wrong_tiles(ranges.astype(np.int64), plist, ref["ids_sorted"])
        else:
            # a band of tile rows: only its pairs are listed -- the band's tiles hold the oracle's lists, whatever their offsets
            r0, r1 = band
            n = tc.list_lengths(ref)
            in_band = np.zeros(len(n), bool)
            in_band[r0 * gx:r1 * gx] = True
            assert D == int(n[in_band].sum())
            touched, ranges, plist = c_abi_views.read_lists(self.L, st, N, cap, W, H, D)
            ranges = ranges.astype(np.int64)
            tile_of = ref["rect"][:, 1].astype(np.int64) * gx + ref["rect"][:, 0]
            np.testing.assert_array_equal(touched, in_band[tile_of].astype(np.uint32))
            covered = np.zeros(D, bool)
            for t in np.nonzero(in_band)[0]:
                b, e = ranges[t]
                assert e - b == n[t] and 0 <= b <= e <= D, int(t)
                want = ref["ids_sorted"][ref["ranges"][t, 0]:ref["ranges"][t, 1]]
                got = plist[b:e]
                assert np.array_equal(got, want), f"tile {int(t)}: {int(n[t])} entries, {int((got == 0).sum())} zeros"
                assert not covered[b:e].any()
                covered[b:e] = True
            assert covered.all()
            # pixels outside the band are not written
            for k in ("color", "depth", "opacity"):
                img = st[k]
                assert bool((img[:, :r0 * tc.TILE] == 7.0).all()) and bool((img[:, r1 * tc.TILE:] == 7.0).all()), k
        # the same lists: the same blend, whatever sorted them
        key = (name, shift, band)
        out = {k: st[k].cpu() for k in ("color", "depth", "opacity", "n_touched")}
        first = _IMAGES.setdefault(key, out)
        for k, v in out.items():
            assert torch.equal(v, first[k]), f"{k} differs from the first call's on this scene"
        assert bool(out["opacity"].max() > 0)

    def _profiled(self, call, tile_sorts=1):
        """call() with the launch profile on -> the number of tile_sort_long launches it made."""
        self.lib.profile_enable(True)
        try:
            self.lib.profile_reset()
            call()
            torch.cuda.synchronize()
            prof = self.lib.profile_read()
        finally:
            self.lib.profile_enable(False)
        assert prof.get("tile_sort", (0, 0.0))[0] == tile_sorts, prof     # (the profile does see this thread's launches)
        return prof.get("tile_sort_long", (0, 0.0))[0]

    def _counting(self, name):
        _, W, H, _, _ = tc.CASES[name]
        return (W // tc.TILE) * (H // tc.TILE) <= COUNTING_MAX_TILES

    # ---- the entry points ----
    def forward(self, name, flags=0, band=None, expect=None):
        """lvdgs_forward of a case; ``expect``: the state the script means this call's tile sort to meet."""
        _, W, H, _, _ = tc.CASES[name]
        ref = tc.reference(name)
        n = tc.list_lengths(ref)
        if band:
            gx = W // tc.TILE
            n = n[band[0] * gx:band[1] * gx]
        cap = int(n.sum()) + SLACK
        a, st = self._view(name, cap, flags, band=band)
        D = C.c_int64()
        launches = self._profiled(lambda: self.lib.check(self.L.lvdgs_forward(C.byref(a), C.byref(D), self.stream), "lvdgs_forward"))
        super_ = self._super_in_use(name, flags, band)
        if self._counting(name):
            state = _state(self.hints.longest_super if super_ else self.hints.longest)
            self.hints.fold(n, tc.super_list_lengths(tc.list_lengths(ref), W, H) if super_ else None)
        else:
            state = "c"     # the radix path queues long segments itself: always the long-segment kernel, no hint folded
        self.states.append(state)
        if expect is not None:
            assert state == expect, (state, expect)
        self._check(name, st, cap, D.value, band=band)
        assert launches == LONG_LAUNCHES[state], (state, launches)
        return st

    def prepare_render(self, name, flags=0):
        """lvdgs_forward_prepare + lvdgs_forward_render: no hint reaches the tile sort (state d), none is left."""
        D_ref = tc.reference(name)["num_rendered"]
        a, st = self._view(name, D_ref, flags)
        D = C.c_int64()
        self.lib.check(self.L.lvdgs_forward_prepare(C.byref(a), C.byref(D), self.stream), "lvdgs_forward_prepare")
        assert D.value == D_ref
        a.num_rendered = D.value
        launches = self._profiled(lambda: self.lib.check(self.L.lvdgs_forward_render(C.byref(a), self.stream), "lvdgs_forward_render"))
        self.states.append("d")
        self._check(name, st, D_ref, D.value)
        assert launches == LONG_LAUNCHES["d"]
        return st

    def batch(self, name, shifts, flags=0, expect=None):
        """lvdgs_forward_batch of the case's map under the cameras shifted by ``shifts`` tile columns -> the views' buffers."""
        _, W, H, _, _ = tc.CASES[name]
        refs = [tc.reference(name, s) for s in shifts]
        cap = max(r["num_rendered"] for r in refs) + SLACK
        views = [self._view(name, cap, flags, shift=s) for s in shifts]
        V = len(views)
        arr = (C.POINTER(self.lib.Args) * V)(*[C.pointer(a) for a, _ in views])
        nums = (C.c_int64 * V)()
        launches = self._profiled(lambda: self.lib.check(self.L.lvdgs_forward_batch(arr, V, nums, self.stream), "lvdgs_forward_batch"))
        super_ = self._super_in_use(name, flags, None)
        state = _state(self.hints.longest_super if super_ else self.hints.longest)
        # (the tile lists' expectation: the longest over the views; the super lists': the first view's)
        self.hints.fold(np.concatenate([tc.list_lengths(r) for r in refs]), tc.super_list_lengths(tc.list_lengths(refs[0]), W, H) if super_ else None)
        self.states.append(state)
        if expect is not None:
            assert state == expect, (state, expect)
        for k, s in enumerate(shifts):
            self._check(name, views[k][1], cap, nums[k], shift=s)
        assert launches == V * LONG_LAUNCHES[state], (state, launches)     # (a long-segment kernel per view)
        return [st for _, st in views]

    def forward_shifted(self, name, shift, cap):
        """lvdgs_forward of one view of a batch, with the batch's capacity (the state buffers are then laid out alike)."""
        a, st = self._view(name, cap, 0, shift=shift)
        D = C.c_int64()
        self.lib.check(self.L.lvdgs_forward(C.byref(a), C.byref(D), self.stream), "lvdgs_forward")
        torch.cuda.synchronize()
        self.hints.fold(tc.list_lengths(tc.reference(name, shift)))
        self._check(name, st, cap, D.value, shift=shift)
        return st


def _flags(all_tiles):
    from lvdgs import _lib
    return _lib.FLAG_LIST_ALL_TILES if all_tiles else 0


GRIDS = ["small", "large"]     # <= 4096 tiles: tile order and solo workgroups; 4097..16384 tiles: the plain wave path


@pytest.mark.parametrize("all_tiles", [False, True], ids=["culled", "all_tiles"])
@pytest.mark.parametrize("grid", GRIDS)
def test_every_hint_state_on_the_counting_path(grid, all_tiles):
    """MID (a), MID (b), FULL (b, longer than expected), FULL (c), MID (c, shorter than expected), prepare + render of FULL (d)."""
    def script():
        s = Session()
        f = _flags(all_tiles)
        s.forward("mid_" + grid, f, expect="a")
        s.forward("mid_" + grid, f, expect="b")
        s.forward("full_" + grid, f, expect="b")
        s.forward("full_" + grid, f, expect="c")
        s.forward("mid_" + grid, f, expect="c")
        s.prepare_render("full_" + grid, f)
        assert s.states == ["a", "b", "b", "c", "c", "d"]
    in_fresh_thread(script)


@pytest.mark.parametrize("all_tiles", [False, True], ids=["culled", "all_tiles"])
@pytest.mark.parametrize("grid", GRIDS)
def test_nothing_expected_and_everything_arrives(grid, all_tiles):
    """SHORT, then FULL: the launch's last workgroups alone sort everything from 1025 to 20000 entries (state a)."""
    def script():
        s = Session()
        f = _flags(all_tiles)
        s.forward("short_" + grid, f, expect="a")
        s.forward("full_" + grid, f, expect="a")
    in_fresh_thread(script)


@pytest.mark.parametrize("all_tiles", [False, True], ids=["culled", "all_tiles"])
def test_radix_path_queues_and_gathers(all_tiles):
    """More than 16384 tiles (2064 x 2064): the wave kernel queues the long segments itself, every sort gathers its keys from ids and
    records, the long-segment kernel takes everything beyond 1024 entries.  Twice: the second call finds the first one's buffers' like."""
    def script():
        s = Session()
        f = _flags(all_tiles)
        s.forward("full_radix", f)
        s.forward("full_radix", f)
        assert s.states == ["c", "c"]
    in_fresh_thread(script)


def test_expectation_outlives_32_short_frames_and_no_more():
    """The hint is kept for 32 frames: behind a FULL frame, 33 SHORT frames in a row still get the long-segment kernel (state c, the
    33rd lowers the expectation), and the FULL frame after them meets state a again -- every frame's lists checked, every frame's
    launches counted."""
    def script():
        s = Session()
        s.forward("full_small", expect="a")
        for _ in range(33):
            s.forward("short_small", expect="c")
        s.forward("full_small", expect="a")
    in_fresh_thread(script)


def test_more_segments_than_head_workgroups():
    """MID, MID, then 80 segments of 1025..2048 entries for the 64 workgroups at the head of the launch: some sort two in turn, through
    the same LDS exchange buffer."""
    def script():
        s = Session()
        s.forward("mid_small", expect="a")
        s.forward("mid_small", expect="b")
        s.forward("many_mid", expect="b")
    in_fresh_thread(script)


def test_more_segments_than_last_workgroups():
    """SHORT, then 260 segments of 1025..1084 entries for the launch's 256 last workgroups."""
    def script():
        s = Session()
        s.forward("short_small", expect="a")
        s.forward("many_tail", expect="a")
    in_fresh_thread(script)


def test_more_segments_than_long_kernel_workgroups():
    """FULL, then 260 segments of 2049..2108 entries for the long-segment kernel's 256 workgroups."""
    def script():
        s = Session()
        s.forward("full_small", expect="a")
        s.forward("many_long", expect="c")
    in_fresh_thread(script)


@pytest.mark.parametrize("placement", ["super4", "super1"])
def test_super_tile_lists(placement):
    """LVDGS_FLAG_SUPER_TILES: the same sort on the 64 x 64-pixel super-tiles' lists, the tiles' lists read off them.  super4: one
    populated tile per super-tile, the super lists have the ladder's lengths; super1 (128 x 128): four super lists of thousands to tens
    of thousands of entries, each the union of several tiles.  First frame (d), the same again (c), SHORT, FULL."""
    from lvdgs import _lib
    def script():
        s = Session()
        f = _lib.FLAG_SUPER_TILES
        s.forward("full_" + placement, f, expect="d")
        s.forward("full_" + placement, f, expect="c")
        s.forward("short_" + placement, f, expect="c")
        # (super1: the SHORT ladder's 4549 entries on four super-tiles may queue a list; super4: nothing is queued)
        s.forward("full_" + placement, f, expect="a" if placement == "super4" else None)
        # and without the hint flag, for the images' sake: the same bits
        s.forward("full_" + placement, 0)
    in_fresh_thread(script)


def test_batch_of_three_views_in_states_a_and_c():
    """lvdgs_forward_batch with three views of one map whose ladders differ (cameras a whole number of tile columns apart): in a fresh
    thread (a), and behind a single-call FULL frame on the same thread (c) -- against the oracle and against lvdgs_forward view by view."""
    def script():
        s = Session()
        name, shifts = "full_small", tc.BATCH_SHIFTS
        first = s.batch(name, shifts, expect="a")
        cap = max(tc.reference(name, sh)["num_rendered"] for sh in shifts) + SLACK
        single = [s.forward_shifted(name, shifts[0], cap)]
        second = s.batch(name, shifts, expect="c")
        single += [s.forward_shifted(name, sh, cap) for sh in shifts[1:]]
        for views in (first, second):
            for st, ref in zip(views, single):
                for k in ("radii", "geom", "color", "depth", "opacity", "n_touched"):
                    assert torch.equal(st[k], ref[k]), k
    in_fresh_thread(script)


def test_batch_with_super_tile_lists():
    """lvdgs_forward_batch with LVDGS_FLAG_SUPER_TILES: the batched launcher on the views' super lists (nine per view on this frame,
    unions of up to 16 tiles), first unknown (d), then expected long (c)."""
    from lvdgs import _lib
    def script():
        s = Session()
        s.batch("full_small", tc.BATCH_SHIFTS, _lib.FLAG_SUPER_TILES, expect="d")
        s.batch("full_small", tc.BATCH_SHIFTS, _lib.FLAG_SUPER_TILES, expect="c")
    in_fresh_thread(script)


def test_band_of_tile_rows():
    """tile_row_begin / tile_row_end: a strict sub-range of rows that holds segments of every class, in states a and c.  Outside the band
    include/lvdgs.h promises only that no pair is listed and no pixel written."""
    def script():
        s = Session()
        s.forward("full_small", band=tc.BAND_ROWS, expect="a")
        s.forward("full_small", band=tc.BAND_ROWS, expect="c")
    in_fresh_thread(script)
