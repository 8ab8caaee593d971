"""The ladder scenes of tests/tile_sort_cases.py and their reference, checked on the CPU: every case that tests/test_gpu_tile_sort.py
runs has exactly the prescribed list lengths in the float32 oracle, every Gaussian on one tile, depth ties and depth differences in
every long segment -- and the oracle's sorted lists equal a NumPy restatement of the order, so the reference does not rest on its C
sort alone.  These are conditions on the scenes: a scene that misses one is fixed, not excused."""
import numpy as np
import pytest

import tile_sort_cases as tc


def _grid(name):
    _, W, H, _, _ = tc.CASES[name]
    return W // tc.TILE, H // tc.TILE


@pytest.mark.parametrize("name", list(tc.CASES))
def test_ladder_has_exactly_the_prescribed_lists(name):
    lengths, W, H, seed, stride = tc.CASES[name]
    assert W % tc.TILE == 0 and H % tc.TILE == 0
    f = tc.reference(name)
    gx, gy = _grid(name)
    N = int(sum(lengths))
    assert f["radii"].shape[0] == N and f["num_rendered"] == N
    n = tc.list_lengths(f)
    assert n.shape[0] == gx * gy
    # the prescribed multiset of lengths, on that many tiles, and nothing anywhere else
    assert sorted(n[n > 0].tolist()) == sorted(x for x in lengths if x > 0)
    assert (f["ranges"][n == 0] == 0).all()
    assert (f["tiles_touched"] == 1).all()
    assert (f["radii"] > 0).all() and f["radii"].max() <= 5
    if stride > 1:
        t = np.nonzero(n > 0)[0]
        assert ((t % gx) % stride == 0).all() and ((t // gx) % stride == 0).all()
        # one populated tile per super-tile: the super lists have the tile lists' lengths
        s = tc.super_list_lengths(n, W, H)
        assert sorted(s[s > 0].tolist()) == sorted(n[n > 0].tolist())


@pytest.mark.parametrize("name", list(tc.CASES))
def test_long_segments_hold_equal_and_different_depths(name):
    """Otherwise the tie rule (equal depth bits: the smaller id first) or the depth rule goes untested in that segment."""
    f = tc.reference(name)
    bits = np.ascontiguousarray(f["depths"], dtype=np.float32).view(np.uint32)
    n = tc.list_lengths(f)
    for t in np.nonzero(n >= 64)[0]:
        seg = bits[f["ids_sorted"][f["ranges"][t, 0]:f["ranges"][t, 1]]]
        distinct = len(np.unique(seg))
        assert 1 < distinct < len(seg), (name, int(t), int(n[t]), distinct)
    # id order says nothing about depth: a long segment's sorted ids are not ascending
    t = int(np.argmax(n))
    assert (np.diff(f["ids_sorted"][f["ranges"][t, 0]:f["ranges"][t, 1]].astype(np.int64)) < 0).any()


@pytest.mark.parametrize("name,shift", [(name, 0) for name in tc.CASES] + [("full_small", s) for s in tc.BATCH_SHIFTS if s])
def test_oracle_lists_equal_the_numpy_restatement(name, shift):
    f = tc.reference(name, shift)
    gx, _ = _grid(name)
    ids, tiles = tc.numpy_sorted_ids(f, gx)
    np.testing.assert_array_equal(f["ids_sorted"], ids)
    np.testing.assert_array_equal((f["keys_sorted"] >> np.uint64(32)).astype(np.int64), tiles)
    # the ranges are those tiles' runs
    n = np.bincount(tiles, minlength=f["ranges"].shape[0])
    np.testing.assert_array_equal(tc.list_lengths(f), n)
    start = np.concatenate([[0], np.cumsum(n)[:-1]])
    np.testing.assert_array_equal(f["ranges"][n > 0, 0], start[n > 0])


def _classes_of(lengths):
    return [any(lo <= x <= hi for x in lengths) for lo, hi in tc.CLASSES]


def test_the_batch_views_are_the_ladder_moved_by_whole_tile_columns():
    """lvdgs_forward_batch takes several views of ONE map: the three cameras differ by whole tile columns of the principal point, which
    keeps every centre where it was inside its tile -- the segments move with their tiles, those that leave the frame are culled."""
    name = "full_small"
    gx, gy = _grid(name)
    base = tc.list_lengths(tc.reference(name)).reshape(gy, gx)
    seen = set()
    for shift in tc.BATCH_SHIFTS:
        f = tc.reference(name, shift)
        moved = np.zeros_like(base)
        if shift >= 0:
            moved[:, shift:] = base[:, :gx - shift]
        else:
            moved[:, :gx + shift] = base[:, -shift:]
        np.testing.assert_array_equal(tc.list_lengths(f).reshape(gy, gx), moved)
        assert (f["tiles_touched"] <= 1).all() and int(f["tiles_touched"].sum()) == int(moved.sum()) == f["num_rendered"]
        assert ((f["radii"] > 0) == (f["tiles_touched"] == 1)).all()
        assert all(_classes_of(moved[moved > 0].tolist())), shift
        seen.add(tuple(moved.ravel().tolist()))
    assert len(seen) == len(tc.BATCH_SHIFTS)     # three different ladders
    assert tc.BATCH_SHIFTS[0] == 0


def test_the_band_holds_every_size_class_and_leaves_segments_outside():
    name = "full_small"
    gx, gy = _grid(name)
    n = tc.list_lengths(tc.reference(name)).reshape(gy, gx)
    r0, r1 = tc.BAND_ROWS
    assert 0 < r0 < r1 < gy
    inside = n[r0:r1]
    assert all(_classes_of(inside[inside > 0].tolist()))
    outside = np.concatenate([n[:r0].ravel(), n[r1:].ravel()])
    assert (outside > tc.WAVE_LIMIT).any() and ((outside > 0) & (outside <= tc.WAVE_LIMIT)).any()


def test_the_grids_are_of_the_classes_the_gpu_file_means():
    tiles = lambda wh: (wh[0] // tc.TILE) * (wh[1] // tc.TILE)
    assert 64 <= tiles(tc.SMALL) <= 4096 < tiles(tc.LARGE) <= 16384 < tiles(tc.RADIX)
    assert 64 <= tiles(tc.QUEUE) <= 16384
    assert len(tc.MANY_MID) == 80 and min(tc.MANY_MID) == 1025 and max(tc.MANY_MID) == 2048
    assert len(tc.MANY_TAIL) == 260 and min(tc.MANY_TAIL) == 1025 and max(tc.MANY_TAIL) == 1084
    assert len(tc.MANY_LONG) == 260 and min(tc.MANY_LONG) == 2049 and max(tc.MANY_LONG) == 2108
    assert max(tc.MID) == 2048 and max(tc.SHORT) == 1024
    # 128 x 128, stride 1: four super lists, each the union of several tiles and all for the long-segment kernel -- some for its LDS
    # sort, some for the one in place on global memory
    _, W, H, _, _ = tc.CASES["full_super1"]
    n = tc.list_lengths(tc.reference("full_super1"))
    s = tc.super_list_lengths(n, W, H)
    assert len(s) == 4 and s.min() > tc.GROUP_LIMIT and s.min() <= tc.LDS_LIMIT < s.max() and s.max() > n.max()
