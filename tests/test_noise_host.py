"""CPU: the seeded sensor noise generator (csrc/lrc_noise.h) through its host entry points -- Philox known answers, the
quantile table against the exact quantile, lrc_noise_draws against the numpy restatement bit for bit (tests/noise_restate.py),
independence of chunking, moments, and the argument checks."""
import ctypes as C
import math
import statistics

import numpy as np
import pytest

import noise_restate as nr
import noise_words as nw
from helpers import assert_bit_equal
from noise_words import KNOWN          # shared with the device tests (tests/test_noise_words_gpu.py)


@pytest.fixture(scope="module")
def tab():
    from lidarcast import noise
    return noise.table()


def _lib_words(ctr, key, want_z=False):
    import lidarcast
    lib = lidarcast.load()
    out, z = (C.c_uint32 * 4)(), (C.c_float * 4)()
    rc = lib.lrc_internal_noise_words((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out, z if want_z else None)
    assert rc == 0
    return (tuple(out), np.array(z, dtype=np.float32)) if want_z else tuple(out)


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(x) for x in nr.philox4x32_10(np.array(ctr), np.array(key))) == want
    assert _lib_words(ctr, key) == want


def test_draws_use_the_known_block(tab):
    """seed 0, frame 0, ray 0 is counter 0 under key 0: lrc_noise_draws returns the variates of the first known answer."""
    from lidarcast import noise
    base, slope = tab
    d = noise.draws(noise.NoiseModel(seed=0, dropout=0.5), 1, 1)
    w = np.array(KNOWN[0][2], dtype=np.uint32)
    z = nr.normal_of(w, base, slope)
    assert_bit_equal(np.array([d["z_range"][0, 0], d["z_az"][0, 0], d["z_el"][0, 0]]), z[:3])
    assert bool(d["keep"][0, 0]) == bool(w[3] >= nr.drop_threshold(0.5))
    words, zl = _lib_words(KNOWN[0][0], KNOWN[0][1], want_z=True)
    assert_bit_equal(zl, nr.normal_of(np.array(words, dtype=np.uint32), base, slope))


def test_philox_inverse_round_trip():
    ctr, key = nw.random_pairs(20000, seed=5)
    words = nr.philox4x32_10(ctr, key)
    assert [tuple(int(x) for x in w) for w in words[:3]] == [k[2] for k in KNOWN]
    assert np.array_equal(nr.philox4x32_10_inverse(words, key), ctr)
    assert np.array_equal(nr.philox4x32_10(nr.philox4x32_10_inverse(ctr, key), key), ctr)       # any four words are a block


def test_crafted_words_through_the_host_hook(tab):
    """The edge words of normal_of (tests/noise_words.py) behind lrc_internal_noise_words, which takes a counter and a key:
    the counter is the generator's inverse of the words.  The hook returns the words, and their variates are the restatement's
    bit for bit; at a cell's first word the variate is the table's entry itself, below r = 128 the clamp."""
    base, slope = tab
    words = nw.crafted_words()
    rng = np.random.default_rng(17)
    key = rng.integers(0, 1 << 32, size=(len(words), 2), dtype=np.uint64).astype(np.uint32)
    got_w, got_z = nw.host_blocks(nr.philox4x32_10_inverse(words, key), key)
    assert np.array_equal(got_w, words)
    assert_bit_equal(got_z, nr.normal_of(words, base, slope), "variates of the crafted words")
    cells = nw.cell_words()
    z = {int(w): v for w, v in zip(words.reshape(-1), got_z.reshape(-1))}
    first = np.array([[z[int(w)] for w in row] for row in cells[:, :, 0]], np.float32)
    assert_bit_equal(first, base[::-1], "first word of a cell: octave e = 30 - L")
    neg = np.array([[z[int(w) | 0x80000000] for w in row] for row in cells[:, :, 0]], np.float32)
    assert_bit_equal(neg, -base[::-1], "first word of a cell, sign bit set")
    for r in (0, 1, 127):
        assert z[r] == base[23, 0] and z[r | 0x80000000] == -base[23, 0]
    assert z[128] == base[23, 0] and z[0x7FFFFFFF] < base[0, 63] and z[0x7FFFFFFF] > 0.0


def test_table_is_the_exact_quantile_at_every_cell_start(tab):
    base, slope = tab
    nd = statistics.NormalDist()
    ref = np.array([[nd.inv_cdf(1.0 - (2.0 ** -(e + 1) * (1.0 + c / 64.0)) / 2.0) for c in range(64)] for e in range(24)],
                   dtype=np.float64).astype(np.float32)
    ulps = np.abs(base.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, (int(ulps.max()), np.argwhere(ulps > 1)[:4])
    # the slopes are the float32 differences to the next cell start; behind the last cell comes the octave above (0 at the top)
    flat = base.reshape(-1)
    nxt = np.empty_like(base)
    nxt[:, :63] = base[:, 1:]
    nxt[1:, 63] = base[:-1, 0]
    nxt[0, 63] = 0.0
    assert_bit_equal(slope, (nxt - base).astype(np.float32))
    assert flat.shape == (1536,) and 5.41 < base[23, 0] < 5.43


def test_interpolated_quantile_error(tab):
    """|z| against the exact quantile of q = r / 2^31 on 2e5 random words with r >= 128: at most 1e-4 (the interpolation
    bound (1/64)^2 / 8 * 1.5 = 4.6e-5 plus float32 rounding of values up to 5.4)."""
    base, slope = tab
    rng = np.random.default_rng(11)
    w = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    w = w[(w & np.uint32(0x7FFFFFFF)) >= 128]
    # every octave is met: the random words reach e ~ 17; the deeper ones are added by hand
    deep = np.array([(1 << L) + k * ((1 << L) // 7) for L in range(7, 31) for k in range(7)], dtype=np.uint32)
    w = np.concatenate([w, deep])
    a = nr.abs_normal_of(w, base, slope).astype(np.float64)
    nd = statistics.NormalDist()
    r = (w & np.uint32(0x7FFFFFFF)).astype(np.float64)
    exact = np.array([nd.inv_cdf(1.0 - (x / 2147483648.0) / 2.0) for x in r])
    err = np.abs(a - exact)
    print(f"\n[noise table] {len(w)} words: max |z - exact| {err.max():.3e}, mean {err.mean():.3e}")
    assert err.max() <= 1e-4


@pytest.mark.parametrize("first_frame", [0, 5, 2 ** 32 - 1, 2 ** 64 - 2])
def test_draws_equal_the_restatement(tab, first_frame):
    from lidarcast import noise
    base, slope = tab
    P, N = 3, 400
    m = noise.NoiseModel(seed=0x9E3779B97F4A7C15, dropout=0.05, first_frame=first_frame)
    got = noise.draws(m, P, N)
    ref = nr.draws(m.seed, first_frame, P, N, 0.05, base, slope)
    for k in ("z_range", "z_az", "z_el"):
        assert_bit_equal(got[k], ref[k], k)
    assert np.array_equal(got["keep"], ref["keep"])
    if first_frame == 2 ** 32 - 1:      # pose 1 carries into the high counter word: not the draws of frame 0
        low = noise.draws(noise.NoiseModel(seed=m.seed, dropout=0.05, first_frame=0), 1, N)
        assert not np.array_equal(got["z_range"][1], low["z_range"][0])


def test_draws_do_not_depend_on_chunking():
    from lidarcast import noise
    m = noise.NoiseModel(seed=42, dropout=0.1, first_frame=7)
    whole = noise.draws(m, 6, 130)
    a, b = noise.draws(m, 2, 130), noise.draws(m.at_frame(7 + 2), 4, 130)
    for k in ("z_range", "z_az", "z_el", "keep"):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]])), k


def test_seeds_differ():
    from lidarcast import noise
    a, b = noise.draws(noise.NoiseModel(seed=1), 2, 256), noise.draws(noise.NoiseModel(seed=2), 2, 256)
    for k in ("z_range", "z_az", "z_el"):
        assert (a[k] != b[k]).mean() > 0.99
    hi = noise.draws(noise.NoiseModel(seed=1 + 2 ** 32), 2, 256)       # the high key word counts too
    assert (a["z_range"] != hi["z_range"]).mean() > 0.99


def test_moments_and_dropout_fraction():
    from lidarcast import noise
    P, N = 64, 65536
    n = P * N
    assert n == 2 ** 22
    d = noise.draws(noise.NoiseModel(seed=20261018, dropout=0.05), P, N)
    for k in ("z_range", "z_az", "z_el"):
        z = d[k].astype(np.float64).reshape(-1)
        mean, std = z.mean(), z.std()
        print(f"\n[noise moments] {k}: mean {mean:+.3e}, std {std:.6f}, m4 {(z ** 4).mean():.4f}, max |z| {np.abs(z).max():.3f}")
        assert abs(mean) <= 5.0 / math.sqrt(n)
        assert abs(std - 1.0) <= 5.0 / math.sqrt(2 * n) + 1e-4
    frac = 1.0 - d["keep"].mean()
    assert abs(frac - 0.05) <= 5.0 * math.sqrt(0.05 * 0.95 / n)
    assert noise.draws(noise.NoiseModel(seed=20261018, dropout=0.0), 4, 65536)["keep"].all()


def test_from_intrinsics_converts_degrees():
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast import noise
    k = Indoor8LineLidarIntrinsics.create_standard_8line()
    m = noise.NoiseModel.from_intrinsics(k, seed=3)
    assert m.range_std == k.range_noise_std and m.dropout == k.dropout_probability
    assert m.angle_std == float(np.deg2rad(k.angle_noise_std)) and m.seed == 3 and m.first_frame == 0


@pytest.mark.parametrize("bad", [dict(range_std=-0.01), dict(range_std=float("nan")), dict(range_std=float("inf")),
                                 dict(angle_std=-1e-9), dict(angle_std=float("nan")), dict(angle_std=float("inf")),
                                 dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=float("nan"))])
def test_rejected_models(bad):
    import lidarcast
    from lidarcast import _capi, noise
    lib = lidarcast.load()
    nz = noise.NoiseModel(seed=1, **bad).struct()
    assert lib.lrc_noise_draws(C.byref(nz), 1, 1, None, None, None, None) == _capi.LRC_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="lrc_noise_draws"):
        noise.draws(noise.NoiseModel(seed=1, **bad), 1, 4)


def test_symbols_load():
    from lidarcast import _capi
    lib = _capi.load()
    for name in ("lrc_scan_noisy_dev", "lrc_scan_noisy_compact", "lrc_noise_draws", "lrc_noise_table"):
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
    for name in ("lrc_internal_noise_words", "lrc_internal_noise_words_dev"):
        assert name in _capi.INTERNAL_SYMBOLS and hasattr(lib, name), name
    out = (C.c_uint32 * 4)()
    assert lib.lrc_internal_noise_words(None, (C.c_uint32 * 2)(), out, None) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_internal_noise_words_dev(None, None, None, 0, None, None, None) == _capi.LRC_ERR_INVALID_ARG       # no context
    assert b"lrc_internal_noise_words_dev: ctx is NULL" in lib.lrc_last_error()


def test_rejected_ray_count():
    import lidarcast
    from lidarcast import _capi, noise
    lib = lidarcast.load()
    nz = noise.NoiseModel(seed=1).struct()
    assert lib.lrc_noise_draws(C.byref(nz), 0, 2 ** 32, None, None, None, None) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_noise_draws(C.byref(nz), 0, 2 ** 32 - 1, None, None, None, None) == 0
    assert lib.lrc_noise_draws(None, 1, 1, None, None, None, None) == _capi.LRC_ERR_INVALID_ARG
