"""Shared builders for the tests: sensors, poses, random rays, bit-pattern comparison."""
import dataclasses

import numpy as np


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def assert_bit_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.size == 0:
        return
    ne = bits(a) != bits(b)
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} entries differ; first at {np.argwhere(ne)[0]}"


def pose(x, y, z, yaw=0.0):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    c, s = np.cos(yaw), np.sin(yaw)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    return m


def sensor_8x512():
    from lidar import Indoor8LineLidarIntrinsics
    return dataclasses.replace(Indoor8LineLidarIntrinsics.create_standard_8line(), horizontal_res=512)


def sensor_32x2048():
    from lidar import Indoor8LineLidarIntrinsics
    return dataclasses.replace(Indoor8LineLidarIntrinsics.create_dense_32line(), horizontal_res=2048)


def sensor_small(lines=4, width=96, max_range=20.0):
    from lidar import Indoor8LineLidarIntrinsics
    degs = list(np.linspace(25.0, -35.0, lines))
    return Indoor8LineLidarIntrinsics(vertical_res=lines, horizontal_res=width, max_range=max_range,
                                      vertical_degrees=degs)


def beam_table(elev_deg, width, half_az_deg):
    """(H * width, 3) float64 direction table of a narrow beam about the sensor's -x axis (where column width / 2 of
    IndoorLidar's tables looks): one line of constant elevation per entry of ``elev_deg``, ``width`` columns over
    +-half_az_deg of azimuth, line-major and azimuth-minor like IndoorLidar.sensor_directions().  A sensor far outside a
    room sees it under a few degrees; a full-circle table would miss it with nearly every ray."""
    beta = np.pi - (np.arange(width) - width / 2) / width * 2 * np.deg2rad(half_az_deg)
    alpha = np.deg2rad(np.asarray(elev_deg, dtype=np.float64))
    out = np.empty((len(alpha), width, 3))
    out[..., 0] = np.cos(alpha)[:, None] * np.cos(beta)[None, :]
    out[..., 1] = np.cos(alpha)[:, None] * np.sin(beta)[None, :]
    out[..., 2] = np.sin(alpha)[:, None]
    return out.reshape(-1, 3)


def aimed_pose(target, dist, yaw=0.0, pitch=0.0, roll=0.0):
    """4x4 pose rotated by Rz(yaw) Ry(pitch) Rx(roll) and placed ``dist`` away from ``target`` so that the sensor's -x axis
    (the axis of ``beam_table``) points at it."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    m = np.eye(4)
    m[:3, :3] = rz @ ry @ rx
    m[:3, 3] = np.asarray(target, dtype=np.float64) + dist * m[:3, 0]
    return m


def table_rays(dirs, poses):
    """(P * N, 6) float32 world rays of the float64 direction table ``dirs`` at ``poses`` (P, 4, 4), pose after pose, and
    the (P, 3) float64 centres: the arithmetic of IndoorLidar.get_rays() for a table that no sensor record describes."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    out = np.empty((len(poses), len(dirs), 6), np.float32)
    for p, m in enumerate(poses):
        out[p, :, :3] = m[:3, 3].astype(np.float32)
        out[p, :, 3:] = np.dot(dirs, m[:3, :3].T).astype(np.float32)
    return out.reshape(-1, 6), poses[:, :3, 3].copy()


def random_rays(n, lo, hi, seed=0, unit=True):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, size=(n, 3))
    d = rng.normal(size=(n, 3))
    if unit:
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def random_soup(n_tris, seed=0, extent=4.0, size=0.5):
    """Unstructured triangle soup (non-watertight, overlapping): stresses ties and traversal order."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, size=(n_tris, 1, 3))
    v = c + rng.normal(scale=size, size=(n_tris, 3, 3))
    return v.reshape(-1, 3), np.arange(3 * n_tris, dtype=np.int32).reshape(-1, 3)
