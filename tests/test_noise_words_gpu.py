"""-m gpu: philox4x32_10 and normal_of (csrc/lrc_noise.h) as the DEVICE compiles them, on chosen inputs, through the test hook
lrc_internal_noise_words_dev (lidarcast.noise.words_dev).  In a scan the words are a pure function of (seed, frame, ray), so no
scan puts a chosen word in front of the device's normal_of; the hook does: the Philox known answers, 100 000 seeded (counter,
key) pairs against the numpy restatement, and the edge words of tests/noise_words.py -- the clamp below r = 128, the first
word, the last word and one inside every cell of every octave (L = 7: a one-bit place in the cell, to L = 30: 24 bits), every
r < 2^17, each with both signs -- against tests/noise_restate.py bit for bit and against the host hook.  At a cell's first word
the variate is the entry of lrc_noise_table itself: that pins the context's resident copy of the table."""
import ctypes as C

import numpy as np
import pytest

import noise_restate as nr
import noise_words as nw
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tab():
    from lidarcast import noise
    return noise.table()


def test_philox_known_answers_on_the_device(ctx, tab):
    from lidarcast import noise
    base, slope = tab
    ctr = np.array([k[0] for k in nw.KNOWN], np.uint32)
    key = np.array([k[1] for k in nw.KNOWN], np.uint32)
    words, z = noise.words_dev(ctx, ctr=ctr, key=key)
    assert [tuple(int(x) for x in w) for w in words] == [k[2] for k in nw.KNOWN]
    assert_bit_equal(z, nr.normal_of(words, base, slope), "variates of the known answers")


def test_random_blocks_against_the_restatement_and_the_host(ctx, tab):
    from lidarcast import noise
    base, slope = tab
    ctr, key = nw.random_pairs(100000, seed=20261021)
    words, z = noise.words_dev(ctx, ctr=ctr, key=key)
    want = nr.philox4x32_10(ctr, key)
    assert words.dtype == np.uint32 and np.array_equal(words, want), \
        f"first differing block {np.argwhere((words != want).any(axis=1))[:1].tolist()}"
    assert_bit_equal(z, nr.normal_of(want, base, slope), "variates of the random blocks")
    host_w, host_z = nw.host_blocks(ctr, key)
    assert np.array_equal(words, host_w)
    assert_bit_equal(z, host_z, "device against host hook")


def test_crafted_words(ctx, tab):
    from lidarcast import noise
    base, slope = tab
    words = nw.crafted_words()
    assert len(words) == (24 * 64 * 3 + 5 + (1 << 17)) * 2 // 4 + 1
    r = words & np.uint32(0x7FFFFFFF)
    assert (r < 128).sum() >= 2 * 128 and (r == 128).sum() >= 2
    back, z = noise.words_dev(ctx, words=words)
    assert np.array_equal(back, words)                                           # words given are not written over
    assert_bit_equal(z, nr.normal_of(words, base, slope), "variates of the crafted words")
    # ... and the host hook, which takes a counter: the generator's inverse of the words under seeded keys
    rng = np.random.default_rng(17)
    key = rng.integers(0, 1 << 32, size=(len(words), 2), dtype=np.uint64).astype(np.uint32)
    ctr = nr.philox4x32_10_inverse(words, key)
    host_w, host_z = nw.host_blocks(ctr, key)
    assert np.array_equal(host_w, words)
    assert_bit_equal(z, host_z, "device against host hook")
    dev_w, dev_z = noise.words_dev(ctx, ctr=ctr, key=key)                        # the same blocks generated on the device
    assert np.array_equal(dev_w, words)
    assert_bit_equal(dev_z, z, "generated against given words")


def test_cell_starts_are_the_table(ctx, tab):
    """The first word of cell c of octave e = 30 - L has f = 0: the variate is base[e][c] of lrc_noise_table, exactly, with the
    word's sign; below r = 128 it is the clamp base[23][0]; the last word of a cell stays inside the cell."""
    from lidarcast import noise
    base, slope = tab
    cells = nw.cell_words()
    first = np.ascontiguousarray(cells[:, :, 0]).reshape(-1, 4)
    _, z = noise.words_dev(ctx, words=first)
    assert_bit_equal(z.reshape(24, 64), np.ascontiguousarray(base[::-1]), "cell starts")
    _, zn = noise.words_dev(ctx, words=first | nw.SIGN)
    assert_bit_equal(zn.reshape(24, 64), np.ascontiguousarray(-base[::-1]), "cell starts, sign bit set")
    small = np.array([[0, 1, 127, 128], [0x80000000, 0x80000001, 0x8000007F, 0x80000080]], np.uint32)
    _, zs = noise.words_dev(ctx, words=small)
    assert (zs[0] == base[23, 0]).all() and (zs[1] == -base[23, 0]).all()
    last = np.ascontiguousarray(cells[:, :, 2]).reshape(-1, 4)
    _, zl = noise.words_dev(ctx, words=last)
    zl = zl.reshape(24, 64)[::-1]                                                # [e, c]
    nxt = base + slope                                                           # the next cell's start, as the table holds it
    assert (zl < base).all() and (zl >= nxt).all()


def test_refusals_and_the_empty_call(ctx):
    import torch
    from lidarcast import _capi, noise
    lib = _capi.load()
    fn = lib.lrc_internal_noise_words_dev
    c = torch.zeros(4, dtype=torch.int32, device="cuda")
    k = torch.zeros(2, dtype=torch.int32, device="cuda")
    w = torch.zeros(4, dtype=torch.int32, device="cuda")
    z = torch.zeros(4, dtype=torch.float32, device="cuda")
    assert fn(None, c.data_ptr(), k.data_ptr(), 1, w.data_ptr(), z.data_ptr(), None) == _capi.LRC_ERR_INVALID_ARG
    assert fn(ctx._h, c.data_ptr(), k.data_ptr(), 1, None, z.data_ptr(), None) == _capi.LRC_ERR_INVALID_ARG
    assert b"lrc_internal_noise_words_dev" in lib.lrc_last_error()
    assert fn(ctx._h, c.data_ptr(), None, 1, w.data_ptr(), z.data_ptr(), None) == _capi.LRC_ERR_INVALID_ARG
    assert fn(ctx._h, None, None, 0, None, None, None) == 0
    assert fn(ctx._h, c.data_ptr(), k.data_ptr(), 1, w.data_ptr(), None, None) == 0          # the variates are optional, as on the host
    torch.cuda.synchronize()
    assert tuple(int(x) & 0xFFFFFFFF for x in w.tolist()) == nw.KNOWN[0][2]
    # the host hook's own refusals, for comparison
    out = (C.c_uint32 * 4)()
    assert lib.lrc_internal_noise_words(None, (C.c_uint32 * 2)(), out, None) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_internal_noise_words((C.c_uint32 * 4)(), None, out, None) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_internal_noise_words((C.c_uint32 * 4)(), (C.c_uint32 * 2)(), None, None) == _capi.LRC_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        noise.words_dev(ctx)
    with pytest.raises(ValueError):
        noise.words_dev(ctx, ctr=np.zeros((1, 4), np.uint32))
    got_w, got_z = noise.words_dev(ctx, words=np.zeros((0, 4), np.uint32))
    assert got_w.shape == (0, 4) and got_z.shape == (0, 4)
