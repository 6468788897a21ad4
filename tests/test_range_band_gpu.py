"""-m gpu: the trace kernel's range filter (csrc/lidarcast.hip range_filter: the squared distance against two bounds, the
float64 square root only for a wave with a ray between them) against numpy's `sqrt(s) < max_range`, with max_range set to
the exact distance of rays of the scan itself -- so squared distances equal to max_range^2 and within a few ulp of it occur,
waves take the square-root path beside waves that do not, and a wrong decision on either path drops or keeps a ray numpy
does not."""
import dataclasses

import numpy as np
import pytest

from helpers import pose, sensor_small

pytestmark = pytest.mark.gpu


def _scan(eng, k, poses, mesh):
    rec, n = eng.scan_poses(k, poses, mesh, want=("t", "point3"))
    return np.stack([rec["t"][p] for p in range(len(poses))]), np.stack([rec["point3"][p] for p in range(len(poses))])


def test_range_filter_equals_numpy_at_ranges_taken_from_the_scan():
    from lidarcast import synth
    from raycast_engine import RaycastEngineGPU
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=7, cell=0.04)
    rng = np.random.default_rng(11)
    P = 4
    poses = np.stack([pose(0.8 + 2.4 * rng.random(), 0.8 + 1.4 * rng.random(), 0.6 + 1.2 * rng.random(), yaw=rng.uniform(-3, 3))
                      for _ in range(P)])
    eng = RaycastEngineGPU()
    far = sensor_small(lines=8, width=512, max_range=1e6)
    t_all, pts = _scan(eng, far, poses, mesh)
    hit = t_all != np.inf
    assert hit.mean() > 0.9
    # the kernel's float64 expression, op for op: s = (ex*ex + ey*ey) + ez*ez with e = double(point) - centre
    e = pts.astype(np.float64) - poses[:, None, :3, 3]
    s = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    dist = np.sqrt(s)
    in_band = 0
    for q in (0.2, 0.5, 0.8):
        R = float(np.quantile(dist[hit], q, method="nearest"))        # the distance of a ray of this scan: sqrt(s) == R for it
        r2 = R * R
        in_band += int((hit & (np.abs(s - r2) <= r2 * 2.0 ** -48)).sum())
        t_r, _ = _scan(eng, dataclasses.replace(far, max_range=R), poses, mesh)
        want = hit & (dist < R)
        got = t_r != np.inf
        bad = np.argwhere(got != want)
        assert bad.size == 0, (R, len(bad), bad[:4], s[tuple(bad[0])], r2)
        assert 0 < want.sum() < hit.sum()
    assert in_band >= 3          # each chosen range has at least its own ray between the bounds
