"""Chosen inputs for the seeded noise generator (numpy only): the Philox4x32-10 known answers and the words that sit on the
edges of normal_of (csrc/lrc_noise.h) -- the clamp below r = 128, the first and the last word and one inside every one of the
24 x 64 cells, L = 7 (a one-bit place in the cell) to L = 30 (24 bits), every r below 2^17, each with both signs.  The host
tests put them behind lrc_internal_noise_words (through the inverse of the generator, tests/noise_restate.py), the device
tests behind lrc_internal_noise_words_dev."""
import numpy as np

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

SIGN = np.uint32(0x80000000)


def cell_words():
    """(24, 64, 3) uint32, sign bit clear: the first word, one inside and the last word of cell c of octave e = 30 - L, indexed
    [L - 7, c]."""
    out = np.zeros((24, 64, 3), np.uint32)
    for L in range(7, 31):
        sh = L - 6
        first = (1 << L) + (np.arange(64, dtype=np.int64) << sh)
        out[L - 7, :, 0] = first
        out[L - 7, :, 1] = first + ((1 << sh) * 2) // 3
        out[L - 7, :, 2] = first + (1 << sh) - 1
    assert out[0, 0, 0] == 128 and out[23, 63, 2] == 0x7FFFFFFF
    assert (out[0, :, 1] == out[0, :, 2]).all() and (out[1:, :, 1] > out[1:, :, 0]).all() and (out[1:, :, 1] < out[1:, :, 2]).all()
    return out


def crafted_words():
    """(n, 4) uint32 blocks: the cell words, r in {0, 1, 127, 128, 2^31 - 1} and every r < 2^17, then all of them again with
    the sign bit set (padded with zero words to whole blocks)."""
    r = np.concatenate([cell_words().reshape(-1), np.array([0, 1, 127, 128, 0x7FFFFFFF], np.uint32),
                        np.arange(1 << 17, dtype=np.uint32)])
    w = np.concatenate([r, r | SIGN])
    w = np.concatenate([w, np.zeros(-len(w) % 4, np.uint32)])
    return w.reshape(-1, 4)


def host_blocks(ctr, key):
    """(words (n, 4) uint32, z (n, 4) float32) of lrc_internal_noise_words, one call per block."""
    import lidarcast
    fn = lidarcast.load().lrc_internal_noise_words
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
    key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
    assert len(ctr) == len(key)
    words = np.zeros((len(ctr), 4), np.uint32)
    z = np.full((len(ctr), 4), np.nan, np.float32)
    c0, k0, w0, z0 = (a.ctypes.data for a in (ctr, key, words, z))
    for j in range(len(ctr)):
        rc = fn(c0 + 16 * j, k0 + 8 * j, w0 + 16 * j, z0 + 16 * j)
        assert rc == 0, (j, rc)
    return words, z


def random_pairs(n, seed):
    """(n, 4) counters and (n, 2) keys, seeded; the first rows are the known answers' and all-zero / all-one words."""
    rng = np.random.default_rng(seed)
    ctr = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    for j, (c, k, _) in enumerate(KNOWN):
        ctr[j], key[j] = c, k
    return ctr, key
