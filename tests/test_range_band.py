"""CPU: the trace kernel's range filter decides `sqrt(s) < max_range` on the squared float64 distance s wherever s lies
outside a narrow band around max_range^2, and by the square root itself inside it (csrc/lrc_device.h, range_band).  The
library's host compilation of those very functions (lrc_internal_range_decide) must agree with numpy's correctly rounded
square root on every value -- every float64 within 64 ulp of max_range^2 included -- and the band must be narrow enough
that the square root is the exception."""
import ctypes

import numpy as np
import pytest


def _decide(R, s):
    import lidarcast
    lib = lidarcast.load()
    fn = lib.lrc_internal_range_decide
    fn.argtypes = [ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = None
    s = np.ascontiguousarray(s, dtype=np.float64)
    keep = np.empty(len(s), dtype=np.uint8)
    band = np.empty(len(s), dtype=np.uint8)
    bounds = np.zeros(3, dtype=np.float64)
    fn(R, s.ctypes.data, len(s), keep.ctypes.data, band.ctypes.data, bounds.ctypes.data)
    return keep.astype(bool), band.astype(bool), bounds


def _values(R, n_random=1_000_000):
    r2 = np.float64(R) * np.float64(R)
    bits = np.array([r2]).view(np.int64)[0]
    near = (bits + np.arange(-4096, 4097, dtype=np.int64)).view(np.float64)        # every float64 within 4096 ulp of R^2
    rng = np.random.RandomState(1234)
    # squares of distances around R at every scale from 2^-40 relative to 4x, both sides, plus the far field
    rel = np.ldexp(rng.uniform(0.5, 1.0, n_random // 2), rng.randint(-40, 2, n_random // 2))
    sign = rng.choice([-1.0, 1.0], n_random // 2)
    d = R * (1.0 + sign * rel)
    around = (d * d)[d > 0]
    far = r2 * np.ldexp(rng.uniform(0.5, 1.0, n_random // 2), rng.randint(-60, 60, n_random // 2))
    special = np.array([0.0, np.inf, r2, np.nextafter(r2, 0), np.nextafter(r2, np.inf), 5e-324, 1.7e308])
    return np.concatenate([near, around, far, special])


@pytest.mark.parametrize("R", [25.0, 20.0, 0.5, 1e-3, 1e6])
def test_decision_equals_sqrt_less_than_range(R):
    s = _values(R)
    assert len(s) >= 10 ** 6
    keep, band, bounds = _decide(R, s)
    lo, hi, fast = bounds
    assert fast == 1.0
    want = np.sqrt(s) < R
    bad = np.flatnonzero(keep != want)
    assert bad.size == 0, (R, s[bad[:5]], keep[bad[:5]], want[bad[:5]])
    # the 64-ulp neighbourhood is covered value by value, and both outcomes occur in it
    r2 = np.float64(R) * np.float64(R)
    near = np.abs(np.array(s).view(np.int64) - np.array([r2]).view(np.int64)[0]) <= 64
    assert near.sum() >= 129 and want[near].any() and (~want[near]).any()
    # the bounds bracket R^2 and the band is a few tens of ulp wide: outside it no square root is formed
    assert lo < r2 < hi and (hi - lo) / r2 < 2.0 ** -46
    assert not band[(s < lo) | (s > hi)].any() and band[(s >= lo) & (s <= hi)].all()


@pytest.mark.parametrize("R", [0.0, -1.0, np.inf, np.nan, 1e-200, 1e200])
def test_degenerate_ranges_always_take_the_square_root(R):
    s = np.array([0.0, 1e-300, 1.0, 625.0, 1e300, np.inf])
    keep, band, bounds = _decide(R, s)
    assert bounds[2] == 0.0 and band.all()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(keep, np.sqrt(s) < R)
