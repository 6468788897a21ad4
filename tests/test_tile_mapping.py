"""CPU: the two-line tile mapping of the scan pipeline (csrc/lrc_device.h, tile_ray / line_tiles_for), through the library's
host compilation of the functions the trace kernel calls (lrc_internal_tile_map).  For every line width -- the table's own
or not -- the (tile, lane) -> ray map must cover every ray of a pose exactly once, and each half of a wave must be one
aligned half of a 1-D tile in lane order, so that the 32-bit words the waves store assemble exactly the keep masks of the
1-D tiles."""
import ctypes

import numpy as np
import pytest


def _tile_map(line_width, n_rays):
    import lidarcast
    lib = lidarcast.load()
    fn = lib.lrc_internal_tile_map
    fn.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    fn.restype = ctypes.c_uint32
    assert n_rays % 64 == 0
    tpp = n_rays // 64
    out = np.full(tpp * 64, 0xFFFFFFFF, dtype=np.uint32)
    wt = fn(line_width, tpp, out.ctypes.data)
    return wt, out.reshape(tpp, 64)


def _check_bijection_and_masks(rays, n_rays, seed):
    flat = rays.reshape(-1).astype(np.int64)
    assert np.array_equal(np.sort(flat), np.arange(n_rays)), "not every ray exactly once"
    # each half wave = rays 32 k ... 32 k + 31 in lane order: one 32-bit word of the 64-bit mask of 1-D tile k // 2
    halves = rays.reshape(-1, 2, 32).astype(np.int64)
    assert np.all(halves[:, :, 0] % 32 == 0)
    assert np.array_equal(halves - halves[:, :, :1], np.broadcast_to(np.arange(32), halves.shape))
    # assemble the masks as the kernel stores them and compare with the masks of the 1-D tiles
    keep = np.random.RandomState(seed).rand(n_rays) < 0.6
    want = np.packbits(keep.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)
    words = np.zeros(n_rays // 32, dtype=np.uint32)
    written = np.zeros(n_rays // 32, dtype=np.int32)
    for u in range(rays.shape[0]):
        ballot = np.packbits(keep[rays[u].astype(np.int64)], bitorder="little").view(np.uint32)     # low half, high half
        for h in (0, 1):
            w = int(rays[u, 32 * h]) >> 5
            words[w] = ballot[h]
            written[w] += 1
    assert np.all(written == 1), "a mask word is written twice or never"
    assert np.array_equal(words.view(np.uint64), want)


@pytest.mark.parametrize("W,H", [(2048, 32), (64, 2), (64, 3), (1024, 5), (4096, 64)])
def test_true_width_covers_every_ray_once_and_assembles_the_masks(W, H):
    n = W * H
    wt, rays = _tile_map(W, n)
    assert wt == W // 64
    _check_bijection_and_masks(rays, n, seed=W + H)
    # the shape itself: a tile of a whole line pair holds 32 consecutive columns of lines 2g and 2g + 1
    per_pair = 2 * wt
    for u in (0, per_pair - 1, (H // 2) * per_pair - 1):
        g, r = divmod(u, per_pair)
        assert np.array_equal(rays[u, :32], (2 * g) * W + r * 32 + np.arange(32))
        assert np.array_equal(rays[u, 32:], (2 * g + 1) * W + r * 32 + np.arange(32))
    if H % 2:      # an odd last line keeps the 1-D mapping
        u0 = (H // 2) * per_pair
        assert np.array_equal(rays[u0:].reshape(-1), np.arange(u0 * 64, n))


@pytest.mark.parametrize("hint,W,H", [(128, 2048, 32), (1024, 2048, 32), (4096, 2048, 32), (192, 64, 9), (64, 1024, 5), (320, 64, 35)])
def test_a_hint_that_is_not_the_tables_width_is_still_a_bijection(hint, W, H):
    n = W * H
    wt, rays = _tile_map(hint, n)
    assert wt == hint // 64          # accepted: a multiple of 64 that divides the pose into >= 2 lines
    _check_bijection_and_masks(rays, n, seed=hint)


@pytest.mark.parametrize("hint,n", [(0, 2048 * 32), (1, 4096), (100, 6400), (2048, 2048), (1920, 2048 * 32), (128, 64 * 3), (65536, 4096)])
def test_unusable_widths_fall_back_to_one_line_tiles(hint, n):
    wt, rays = _tile_map(hint, n)
    assert wt == 0
    assert np.array_equal(rays.reshape(-1), np.arange(n))
