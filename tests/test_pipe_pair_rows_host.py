"""CPU: the output row of a ray of a prepared pipeline submit (csrc/lrc_device.h, pair_row: x, y, z = o + h * t and the label),
made by the library's host compilation of the very function the trace's write-back and every consumer of a lean record set
call (lrc_internal_pair_rows), against numpy float32 -- multiply, then add, one rounding per operation -- bit for bit."""
import ctypes

import numpy as np

from helpers import bits


def _rows(o, h, t, label):
    import lidarcast
    fn = lidarcast.load().lrc_internal_pair_rows
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    fn.restype = None
    o = np.ascontiguousarray(o, dtype=np.float32)
    h = np.ascontiguousarray(h, dtype=np.float32)
    t = np.ascontiguousarray(t, dtype=np.float32)
    label = np.ascontiguousarray(label, dtype=np.uint32)
    assert o.shape == h.shape == (len(t), 3) and label.shape == t.shape
    out = np.empty((len(t), 4), dtype=np.uint32)
    fn(o.ctypes.data, h.ctypes.data, t.ctypes.data, label.ctypes.data, len(t), out.ctypes.data)
    return out


def _want(o, h, t, label):
    o, h, t = np.asarray(o, np.float32), np.asarray(h, np.float32), np.asarray(t, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        prod = h * t[:, None]
        assert prod.dtype == np.float32
        p = o + prod
        assert p.dtype == np.float32
    return np.concatenate([bits(p), np.asarray(label, np.uint32)[:, None]], axis=1)


def _check(o, h, t, label, what):
    got, want = _rows(o, h, t, label), _want(o, h, t, label)
    nan = np.zeros(got.shape, bool)
    nan[:, :3] = np.isnan(got[:, :3].view(np.float32)) & np.isnan(want[:, :3].view(np.float32))
    ne = (got != want) & ~nan
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} words differ; first at {np.argwhere(ne)[0]}"


def test_random_rays():
    """Origins of a few metres, unit vectors, ranges up to 100 m: where a fused multiply-add would round differently in about
    a quarter of the components."""
    rng = np.random.default_rng(5)
    n = 200_000
    o = rng.uniform(-30, 30, size=(n, 3)).astype(np.float32)
    h = rng.normal(size=(n, 3))
    h = (h / np.linalg.norm(h, axis=1, keepdims=True)).astype(np.float32)
    t = rng.uniform(0.01, 100.0, size=n).astype(np.float32)
    label = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    _check(o, h, t, label, "random rays")
    # the separate roundings are visible in this sample: a single-rounding o + h * t differs somewhere
    fused = (o.astype(np.float64) + h.astype(np.float64) * t.astype(np.float64)[:, None]).astype(np.float32)
    assert (bits(fused) != _want(o, h, t, label)[:, :3]).any()


def test_wide_exponents():
    rng = np.random.default_rng(6)
    n = 50_000
    o = (rng.normal(size=(n, 3)) * np.ldexp(1.0, rng.integers(-40, 40, size=(n, 3)))).astype(np.float32)
    h = (rng.normal(size=(n, 3)) * np.ldexp(1.0, rng.integers(-40, 2, size=(n, 3)))).astype(np.float32)
    t = (rng.uniform(0.5, 1.0, size=n) * np.ldexp(1.0, rng.integers(-40, 40, size=n))).astype(np.float32)
    _check(o, h, t, np.arange(n, dtype=np.uint32), "wide exponents")


def test_signed_zeros_and_specials():
    """Every combination of signed zeros, ones, a denormal, a huge value and infinities in (o, h, t): -0.0 + (+0.0 * t) is +0.0,
    -0.0 + (-0.0 * t) is -0.0, and so on, as numpy gives them."""
    den = float(np.float32(1e-41))
    vals = [0.0, -0.0, 1.0, -1.0, den, -den, 3e38, -3e38, np.inf, -np.inf, 0.5]
    grid = np.array([(a, b, c) for a in vals for b in vals for c in vals], dtype=np.float32)
    o = np.stack([grid[:, 0], grid[:, 0], -grid[:, 0]], axis=1)
    h = np.stack([grid[:, 1], -grid[:, 1], grid[:, 1]], axis=1)
    t = grid[:, 2]
    label = np.full(len(t), 0xFFFF0001, dtype=np.uint32)
    _check(o, h, t, label, "specials")
    got = _rows(o, h, t, label)
    # spot checks of the zero signs, independent of numpy
    k = np.flatnonzero((bits(grid[:, 0]) == 0x80000000) & (bits(grid[:, 1]) == 0) & (grid[:, 2] == 1.0))[0]
    assert got[k, 0] == 0x00000000          # -0.0 + (+0.0 * 1) = +0.0
    assert got[k, 1] == 0x80000000          # -0.0 + (-0.0 * 1) = -0.0
    assert got[k, 2] == 0x00000000          # +0.0 + (+0.0 * 1) = +0.0
    assert (got[:, 3] == 0xFFFF0001).all()
