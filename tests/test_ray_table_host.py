"""CPU: the rows of the ray table of a prepared pipeline submit (csrc/lrc_device.h, ray_row: per table row the float32 world
direction d for a rotation block, its guarded reciprocal and its unit vector), made by the library's host compilation of the
very function the preparation kernel calls (lrc_internal_ray_table_rows), against a numpy restatement, bit for bit:
  d   = np.dot(dirs, R.T).astype(float32)       -- also against the rays captured from the reference at yaw 0.7 (tests/golden)
  inv = float32 1 / x, with |x| < 1e-30 replaced by copysign(1e-30, x) first
  h   = d / sqrt((dx*dx + dy*dy) + dz*dz), float32, one rounding per operation"""
import ctypes

import numpy as np
import pytest

from helpers import bits, pose, sensor_32x2048, sensor_8x512


def assert_bit_equal(a, b, what=""):
    """Bit for bit; a NaN must be a NaN in the same place (its payload is the instruction set's business: rows with a NaN
    component are never cast)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN in different places"
    ne = (bits(a) != bits(b)) & ~na
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} entries differ; first at {np.argwhere(ne)[0]}"


def _rows(R, dirs):
    import lidarcast
    fn = lidarcast.load().lrc_internal_ray_table_rows
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    fn.restype = None
    R = np.ascontiguousarray(R, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    out = np.empty((len(dirs), 9), dtype=np.float32)
    fn(R.ctypes.data, dirs.ctypes.data, len(dirs), out.ctypes.data)
    return out[:, 0:3], out[:, 3:6], out[:, 6:9]


def _inv_np(d):
    tiny = np.float32(1e-30)
    s = np.where(np.abs(d) < tiny, np.copysign(tiny, d), d).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.float32(1.0) / s).astype(np.float32)


def _unit_np(d):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        nrm = np.sqrt((x * x + y * y) + z * z)
        assert nrm.dtype == np.float32
        return (d / nrm[:, None]).astype(np.float32)


def _check(R, dirs, what, dot=True):
    d, inv, h = _rows(R, dirs)
    if dot:
        with np.errstate(over="ignore"):
            assert_bit_equal(d, np.dot(dirs, np.asarray(R).T).astype(np.float32), what + ": d")
    assert_bit_equal(inv, _inv_np(d), what + ": inv")
    assert_bit_equal(h, _unit_np(d), what + ": h")
    return d


def _table(sensor):
    from lidar import IndoorLidar
    return IndoorLidar(sensor, np.eye(4)).sensor_directions()


@pytest.mark.parametrize("yaw", [0.0, 0.7, -2.9])
def test_benchmark_table_rows(yaw):
    """All 65 536 rows of the C3 table (32 lines x 2048) under a yaw."""
    _check(pose(0, 0, 0, yaw)[:3, :3], _table(sensor_32x2048()), f"C3 table, yaw {yaw}")


def test_directions_equal_the_reference_vectors_at_yaw_0_7(golden):
    arrays, _ = golden
    R = arrays["pose_yawed"][:3, :3]
    d = _check(R, _table(sensor_8x512()), "8 x 512 at the golden yawed pose")
    assert_bit_equal(d, arrays["g1_8x512_yawed"][:, 3:6], "8 x 512: d against the reference's rays")
    d = _check(R, _table(sensor_32x2048()), "32 x 2048 at the golden yawed pose")
    assert_bit_equal(d[::97], arrays["g1_32x2048_yawed_stride97"][:, 3:6], "32 x 2048: d against the reference's rays")


def test_random_rows_under_random_rotations():
    rng = np.random.default_rng(11)
    for k in range(4):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        dirs = rng.normal(size=(10_000, 3)) * np.ldexp(1.0, rng.integers(-8, 8, size=(10_000, 1)))
        _check(R, dirs, f"random rows {k}")


def test_zeros_of_both_signs_denormals_and_non_finite_components():
    """Under the identity d = float32(row) except that the dgemm chain starts from +0.0: a -0.0 component comes out as +0.0
    (as np.dot gives it).  Rows with zero, denormal (float32 and float64), tiny, huge, infinite and NaN components."""
    f32_den = float(np.float32(1e-41))
    specials = [0.0, -0.0, 1.0, -1.0, f32_den, -f32_den, 5e-324, -5e-324, 1e-30, -1e-30, 0.99e-30, -0.99e-30, 1.1754944e-38,
                3e38, -3e38, 1e39, np.inf, -np.inf, np.nan, 0.5]
    dirs = np.array([(a, b, c) for a in specials for b in specials for c in (0.0, -0.0, 1.0, f32_den, -0.3)])
    R = np.eye(3)
    with np.errstate(over="ignore", invalid="ignore"):
        d = _check(R, dirs, "special rows, identity", dot=False)
        # np.dot's BLAS route is not promised for tables with NaN / Inf rows; the chain itself is restated term by term
        # (every product with an entry of the identity is exact, and x + 0.0 is x except for -0.0)
        want = (dirs + 0.0).astype(np.float32)
        fin = np.isfinite(dirs).all(axis=1)
        assert_bit_equal(d[fin], want[fin], "special rows: d")
        assert fin.sum() > 1000 and (~fin).sum() > 100
    # the sign of a zero survives a rotation that negates it: 0.0 * -1 accumulates from +0.0 to +0.0, as dgemm does
    flip = np.diag([-1.0, 1.0, -1.0])
    d = _check(flip, dirs[fin], "special rows, flipped axes")
    z = dirs[fin][:, 0] == 0.0
    assert z.any() and not np.signbit(d[z, 0]).any()
    # axis-aligned rows: two exact zeros, reciprocals +-1e30, unit vector on the axis
    axes = np.array([(1.0, 0, 0), (-1.0, 0, 0), (0, 2.0, 0), (0, 0, -0.5), (0, -0.0, 3.0)])
    _check(R, axes, "axis rows")
    d, inv, h = _rows(R, axes)
    assert inv[0, 0] == 1.0 and inv[0, 1] > 9e29 and inv[0, 2] > 9e29 and inv[1, 0] == -1.0
    assert_bit_equal(h[3], np.array([0.0, 0.0, -1.0], np.float32), "axis row: h")
    assert_bit_equal(h[4], np.array([0.0, 0.0, 1.0], np.float32), "axis row with a -0.0: h")
