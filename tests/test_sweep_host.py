"""CPU: the host side of moving-sensor sweeps -- the per-ray arithmetic restated in numpy (tests/sweep_restate.py) against
the static generator, motion_records, the path rule of sweep_end_poses, the firing tables and the nlerp angle bound the
header states."""
import re

import numpy as np
import pytest

from conftest import REPO
from helpers import assert_bit_equal, sensor_32x2048, sensor_8x512, sensor_small
from sweep_restate import quat_matrix, slerp_rotation, sweep_rays


def _rot(yaw, pitch, roll):
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


def _random_poses(n, seed):
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        out[k, :3, :3] = _rot(*rng.uniform(-np.pi, np.pi, 3))
        out[k, :3, 3] = rng.uniform(-3, 3, 3)
    out[0, :3, 3] = (-0.0, 1.5, 0.0)                # signed zeros of the start centre survive
    return out


def _random_quat(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0.0, max_angle)
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * axis])


SENSORS = {"small": sensor_small, "8x512": sensor_8x512, "32x2048": sensor_32x2048}


@pytest.mark.parametrize("name", list(SENSORS))
def test_static_sweep_is_the_static_scan_for_every_fraction(name):
    """end == start: the restated sweep rays equal IndoorLidar.get_rays() of the start pose bit for bit, whatever s."""
    from lidar import IndoorLidar
    from lidarcast import motion_records
    k = SENSORS[name]()
    starts = _random_poses(3, seed=1)
    rec = motion_records(starts, starts)
    assert (rec[:, 12:16] == (1.0, 0.0, 0.0, 0.0)).all() and (rec[:, 16:] == 0.0).all()
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
    rng = np.random.default_rng(2)
    for fire in (IndoorLidar(k, np.eye(4)).firing_fractions(), rng.uniform(0.0, 1.0, len(dirs))):
        rays, cen = sweep_rays(rec, dirs, fire)
        for p, m in enumerate(starts):
            assert_bit_equal(rays[p * len(dirs):(p + 1) * len(dirs)], IndoorLidar(k, m).get_rays(), f"{name} pose {p}")
            assert_bit_equal(cen[p * len(dirs):(p + 1) * len(dirs)], np.broadcast_to(m[:3, 3], (len(dirs), 3)).copy())


def test_fraction_zero_is_the_static_ray_for_any_end_pose():
    from lidar import IndoorLidar
    from lidarcast import motion_records
    k = sensor_8x512()
    starts = _random_poses(4, seed=3)
    rng = np.random.default_rng(4)
    ends = starts.copy()
    for p in range(4):
        ends[p, :3, :3] = quat_matrix(_random_quat(rng, 1.5)) @ starts[p, :3, :3]
        ends[p, :3, 3] += rng.normal(scale=0.3, size=3)
    rec = motion_records(starts, ends)
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
    rays, _ = sweep_rays(rec, dirs, np.zeros(len(dirs)))
    for p, m in enumerate(starts):
        assert_bit_equal(rays[p * len(dirs):(p + 1) * len(dirs)], IndoorLidar(k, m).get_rays(), f"pose {p}")


def test_motion_records_round_trip_against_slerp():
    from lidarcast import motion_records
    rng = np.random.default_rng(5)
    starts = _random_poses(64, seed=6)
    qs = np.array([_random_quat(rng, np.pi / 2 * 0.999) for _ in range(64)])
    qs[:4] = [(1, 0, 0, 0), (np.cos(0.7), 0, 0, np.sin(0.7)), (np.cos(0.7), np.sin(0.7), 0, 0), (np.cos(0.7), 0, np.sin(0.7), 0)]
    ends = starts.copy()
    for p in range(64):
        ends[p, :3, :3] = quat_matrix(qs[p]) @ starts[p, :3, :3]
        ends[p, :3, 3] = starts[p, :3, 3] + rng.normal(size=3)
    rec = motion_records(starts, ends)
    assert rec.shape == (64, 24) and rec.dtype == np.float64
    assert_bit_equal(rec[:, :12], starts.reshape(64, 16)[:, :12])
    assert (rec[:, 19:] == 0).all()
    assert np.abs(rec[:, 12:16] - qs).max() <= 1e-12
    assert (rec[:, 12] >= 0).all()
    assert_bit_equal(rec[:, 16:19], ends[:, :3, 3] - starts[:, :3, 3])
    for p in range(0, 64, 7):          # the slerp of the record reaches the end rotation and halves it on the way
        assert np.abs(slerp_rotation(rec[p, 12:16], 1.0) @ starts[p, :3, :3] - ends[p, :3, :3]).max() <= 1e-12
        half = slerp_rotation(rec[p, 12:16], 0.5)
        assert np.abs(half @ half @ starts[p, :3, :3] - ends[p, :3, :3]).max() <= 1e-12


def test_motion_records_identity_and_limits():
    from lidarcast import motion_records
    starts = _random_poses(5, seed=7)
    rec = motion_records(starts, starts.copy())
    assert_bit_equal(rec[:, 12:19], np.tile([1.0, 0, 0, 0, 0, 0, 0], (5, 1)))
    ends = starts.copy()
    ends[2, :3, :3] = quat_matrix((np.cos(0.85), 0, 0, np.sin(0.85))) @ starts[2, :3, :3]     # 1.7 rad > pi/2
    with pytest.raises(ValueError, match="pi/2"):
        motion_records(starts, ends)
    ends[2, :3, :3] = quat_matrix((np.cos(0.78), 0, 0, np.sin(0.78))) @ starts[2, :3, :3]     # 1.56 rad: accepted
    motion_records(starts, ends)
    bad = starts.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(ValueError):
        motion_records(starts, bad)
    with pytest.raises(ValueError):
        motion_records(starts, starts[:4])


def test_nlerp_angle_stays_within_the_header_table():
    """The rotation the kernel applies at fraction s (the nlerp of dq, restated) against constant-rate slerp, on vectors
    perpendicular to the axis (where the angle error is largest): at most the table of include/lidarcast.h."""
    hdr = open(f"{REPO}/include/lidarcast.h").read()
    m = re.search(r"rotation per sweep\s+([^\n]*)\n\s*\*\s*max angle error\s+([^\n]*)", hdr)
    rots = [float(eval(x.replace("rad", "").replace("pi", "np.pi"))) for x in m.group(1).split("rad") if x.strip()]
    bounds = [float(x) for x in m.group(2).replace("rad", "").split()]
    assert len(rots) == len(bounds) == 5
    rng = np.random.default_rng(8)
    s = np.linspace(0.0, 1.0, 2049)[:-1]
    for a, bound in zip(rots, bounds):
        worst = 0.0
        for _ in range(8):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            v = np.cross(axis, rng.normal(size=3))
            v /= np.linalg.norm(v)
            dq = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * axis])
            rec = np.zeros((1, 24))
            rec[0, [0, 5, 10]] = 1.0
            rec[0, 12:16] = dq
            rays, _ = sweep_rays(rec, v[None].repeat(len(s), 0), s)
            # float64 directions: restate once more without the float32 narrowing
            qw = (1 - s) + s * dq[0]
            u = s[:, None] * dq[1:][None]
            n = ((qw * qw + u[:, 0] * u[:, 0]) + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
            t = np.cross(u, v[None])
            got = v[None] + (2.0 / n)[:, None] * (qw[:, None] * t + np.cross(u, t))
            want = np.array([slerp_rotation(dq, x) @ v for x in s])
            err = np.arccos(np.clip((got * want).sum(1) / np.linalg.norm(got, axis=1), -1, 1))
            worst = max(worst, float(err.max()))
            assert np.abs(rays[:, 3:] - got).max() < 1e-6
        assert worst <= bound, (a, worst, bound)
        assert worst >= bound / 2 or a < 0.06, (a, worst, bound)    # the table is tight, not just an upper bound


def test_firing_fractions_of_both_tables():
    import dataclasses
    from lidar import Indoor8LineLidarIntrinsics, IndoorLidar
    for k in (sensor_small(), sensor_8x512(), dataclasses.replace(Indoor8LineLidarIntrinsics(), vertical_degrees=None,
                                                                   vertical_res=6, horizontal_res=100)):
        lid = IndoorLidar(k, np.eye(4))
        f = lid.firing_fractions()
        W = k.horizontal_res
        assert f.shape == (lid.get_total_rays(),) == (len(lid.sensor_directions()),) and f.dtype == np.float64
        assert_bit_equal(f, (np.arange(len(f)) % W) / W)
        assert (f >= 0).all() and (f < 1).all()


def _wp(x, y, yaw=0.0, **kw):
    from trajectory import Waypoint
    return Waypoint(x, y, 1.0, yaw, **kw)


def test_sweep_end_poses_path_rule():
    from trajectory import Waypoint, poses_from_waypoints, sweep_end_poses
    T = 0.1
    wps = [_wp(0.0, 0.0, 0.0), _wp(1.0, 0.0, 0.4), _wp(1.0, 0.02, 3.0), _wp(1.0, 2.0, -3.0)]
    end = sweep_end_poses(wps, 10.0, 0.5)            # 5 cm per sweep
    assert end.shape == (4, 4, 4)
    # inside one segment: 5 cm along +x, yaw a twentieth of the way from 0 to 0.4
    assert np.allclose(end[0], Waypoint(0.05, 0.0, 1.0, 0.05 * 0.4).to_pose_matrix(), atol=1e-15)
    # crossing a waypoint: the 2 cm segment 1 -> 2, then 3 cm into segment 2 -> 3 whose yaw turns the short way
    # from 3.0 to -3.0 (+0.283 rad, through pi)
    dy = (-3.0 - 3.0 + np.pi) % (2 * np.pi) - np.pi
    f = 0.03 / 1.98
    want = Waypoint(1.0, 0.02 + f * 1.98, 1.0, 3.0 + f * dy).to_pose_matrix()
    assert np.allclose(end[1], want, atol=1e-12)
    # the last waypoint: static, and bitwise the start pose
    start = poses_from_waypoints(wps)
    assert_bit_equal(end[3], start[3])
    # speed 0: every sweep is static
    assert_bit_equal(sweep_end_poses(wps, 10.0, 0.0), start)
    # past the end of the path: clamped at the last waypoint
    far = sweep_end_poses(wps[:2], 10.0, 50.0)
    assert np.allclose(far[0], Waypoint(1.0, 0.0, 1.0, 0.4).to_pose_matrix(), atol=1e-15)


def test_sweep_end_poses_waypoint_velocity_and_turn_rate():
    from trajectory import Waypoint, sweep_end_poses
    wps = [_wp(0.0, 0.0, 0.0, velocity=2.0, angular_velocity=1.0), _wp(1.0, 0.0, 0.0, angular_velocity=-0.5),
           _wp(2.0, 0.0, 0.0)]
    end = sweep_end_poses(wps, 20.0, 0.5)            # T = 0.05 s
    # waypoint 0: its own velocity (10 cm) and turn rate (+0.05 rad)
    assert np.allclose(end[0], Waypoint(0.1, 0.0, 1.0, 0.05).to_pose_matrix(), atol=1e-15)
    # waypoint 1: the default speed (2.5 cm), its turn rate (-0.025 rad)
    assert np.allclose(end[1], Waypoint(1.025, 0.0, 1.0, -0.025).to_pose_matrix(), atol=1e-15)
    with pytest.raises(ValueError):
        sweep_end_poses(wps, 0.0, 0.5)
