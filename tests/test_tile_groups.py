"""CPU: the line-group tile mapping of the scan pipeline (csrc/lrc_device.h, tile_ray with a grouping word), through the
library's host compilation of the function the trace kernel calls (lrc_internal_tile_map_groups), against a restatement of
the rule in numpy: lines [0, split) and [split, H) are cut from their own start into groups of four (L = 4), then a group of
two if two or three lines remain (L = 2: groups of two all the way), then 64 consecutive rays for an odd last line; a group
of g lines deals 64 / g columns of each of its lines to a tile.  For every (W, H, split, L) -- nonsense included -- the map
covers every ray of the pose once, no tile holds lines from both sides of the split, and each quarter of a wave is an
aligned quarter of a 1-D tile in lane order, so the 16-bit words the waves store assemble the keep masks of the 1-D tiles."""
import ctypes

import numpy as np
import pytest


def _tile_map(line_width, n_rays, split, lines):
    import lidarcast
    lib = lidarcast.load()
    fn = lib.lrc_internal_tile_map_groups
    fn.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    fn.restype = ctypes.c_uint32
    assert n_rays % 64 == 0
    tpp = n_rays // 64
    out = np.full(tpp * 64, 0xFFFFFFFF, dtype=np.uint32)
    widest = fn(line_width, tpp, split, lines, out.ctypes.data)
    return widest, out.reshape(tpp, 64).astype(np.int64)


def _restated(W, H, split, L):
    """The rule, group by group: (tiles, 64) rays and the widest group."""
    if W % 64 or H < 2 or L not in (2, 4):
        return np.arange(W * H).reshape(-1, 64), 1
    s = split if 0 < split < H else 0
    tiles, widest = [], 1
    for a, b in (((0, s), (s, H)) if s else ((0, H),)):
        line = a
        while line < b:
            left = b - line
            g = 4 if (L == 4 and left >= 4) else (2 if left >= 2 else 1)
            widest = max(widest, g)
            cols = 64 // g
            grp = np.arange(g * W).reshape(g, W // cols, cols).transpose(1, 0, 2) + line * W
            tiles.append(grp.reshape(-1, 64))
            line += g
    return np.concatenate(tiles), widest


def _check_cover_quarters_and_masks(rays, n_rays, seed):
    flat = rays.reshape(-1)
    assert np.array_equal(np.sort(flat), np.arange(n_rays)), "not every ray exactly once"
    q = rays.reshape(-1, 4, 16)
    assert np.all(q[:, :, 0] % 16 == 0)
    assert np.array_equal(q - q[:, :, :1], np.broadcast_to(np.arange(16), q.shape))
    # the masks as the kernel stores them: quarter j of a wave's ballot to 16-bit word (first ray of the quarter) / 16
    keep = np.random.RandomState(seed).rand(n_rays) < 0.6
    want = np.packbits(keep.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)
    ballots = np.packbits(keep[rays], axis=1, bitorder="little").view(np.uint16).reshape(-1, 4)
    word = q[:, :, 0] // 16
    assert np.array_equal(np.sort(word.reshape(-1)), np.arange(n_rays // 16)), "a mask word is written twice or never"
    words = np.zeros(n_rays // 16, dtype=np.uint16)
    words[word.reshape(-1)] = ballots.reshape(-1)
    assert np.array_equal(words.view(np.uint64), want)


@pytest.mark.parametrize("W", [64, 128, 192, 2048])
@pytest.mark.parametrize("H", [1, 2, 3, 5, 8, 9, 32])
def test_every_split_and_group_size_matches_the_rule(W, H):
    n = W * H
    for L in (1, 2, 4):
        for split in range(H + 1):
            widest, rays = _tile_map(W, n, split, L)
            want, want_widest = _restated(W, H, split, L)
            assert np.array_equal(rays, want), (W, H, split, L)
            assert widest == want_widest, (W, H, split, L, widest)
            _check_cover_quarters_and_masks(rays, n, seed=W + H + split)
            line = rays // W
            assert np.all(line.reshape(-1, 4, 16) == line.reshape(-1, 4, 16)[:, :, :1]), "a quarter wave spans two lines"
            if 0 < split < H:
                below = line < split
                assert np.all(below.all(axis=1) | (~below).all(axis=1)), ("a tile holds lines of both sides", W, H, split, L)
            assert np.all(line.max(axis=1) - line.min(axis=1) < max(widest, 1))


def test_benchmark_sensor_shape_groups_of_four_on_both_sides():
    """32 lines x 2048 with the crossing at line 14 (not a multiple of four): 3 groups of four and a pair above, 4 groups
    of four and a pair below; tile r of a group of four takes columns 16 r ... 16 r + 15 of its four lines."""
    W, H, split = 2048, 32, 14
    widest, rays = _tile_map(W, W * H, split, 4)
    assert widest == 4
    wt = W // 64
    for first_line, g, u0 in ((0, 4, 0), (8, 4, 8 * wt), (12, 2, 12 * wt), (14, 4, 14 * wt), (26, 4, 26 * wt), (30, 2, 30 * wt)):
        cols = 64 // g
        for r in (0, 1, g * wt - 1):
            want = np.concatenate([(first_line + j) * W + r * cols + np.arange(cols) for j in range(g)])
            assert np.array_equal(rays[u0 + r], want), (first_line, g, r)


@pytest.mark.parametrize("hint,W,H,split,L", [(128, 2048, 32, 14, 4), (1024, 2048, 32, 70, 4), (4096, 2048, 32, 3, 4),
                                              (192, 64, 9, 0xFFFFFFFF, 4), (64, 1024, 5, 0x7FFFFFFF, 4), (320, 64, 35, 6, 3),
                                              (64, 64, 9, 4, 0), (128, 64, 10, 2, 7)])
def test_nonsense_widths_splits_and_line_counts_are_still_bijections(hint, W, H, split, L):
    n = W * H
    _, rays = _tile_map(hint, n, split, L)
    _check_cover_quarters_and_masks(rays, n, seed=hint)


@pytest.mark.parametrize("hint,n", [(0, 2048 * 32), (100, 6400), (2048, 2048), (1920, 2048 * 32), (96, 96 * 8)])
def test_unusable_widths_fall_back_to_one_line_tiles(hint, n):
    widest, rays = _tile_map(hint, n, 2, 4)
    assert widest == 1
    assert np.array_equal(rays.reshape(-1), np.arange(n))


def test_the_two_line_hook_is_the_grouping_word_zero():
    """lrc_internal_tile_map (tests/test_tile_mapping.py) and the group form with L = 2 and no split give one map."""
    import lidarcast
    fn = lidarcast.load().lrc_internal_tile_map
    fn.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    fn.restype = ctypes.c_uint32
    for W, H in ((128, 9), (2048, 32), (64, 3)):
        tpp = W * H // 64
        out = np.zeros(tpp * 64, dtype=np.uint32)
        fn(W, tpp, out.ctypes.data)
        _, rays = _tile_map(W, W * H, 0, 2)
        assert np.array_equal(out.reshape(tpp, 64), rays)
