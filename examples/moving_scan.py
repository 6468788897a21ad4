#!/usr/bin/env python3
"""Motion-distorted sweeps: a spinning 32-line sensor on a robot that drives at 0.5 m/s and turns at 0.5 rad/s fires its
columns one after the other during each 0.1 s sweep, so every column is cast from its own pose and every point carries its
time.  Once through the engine (RaycastEngineGPU.scan_sweep_frames) and once through the simulator (config key
``motion``); the static scan of the same waypoints is shown beside it.

    python examples/moving_scan.py
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import synth  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints, sweep_end_poses  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
for w in waypoints:
    w.angular_velocity = 0.5                 # rad/s, adds 0.05 rad of yaw per 10 Hz sweep

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}, "motion": {"speed": 0.5}}, use_dense_lidar=True)
sim.load_scene(mesh, "moving_room")
engine, sensor = sim.raycast_engine, sim.lidar_config

start = poses_from_waypoints(waypoints)
end = sweep_end_poses(waypoints, sensor.scan_frequency, 0.5)
moving = engine.scan_sweep_frames(sensor, start, end, mesh, want=("point3", "index"))
static = engine.scan_frames(sensor, start, mesh, want=("point3", "index"))
print(f"scan_sweep_frames: {len(start)} sweeps, {moving['total']} points (static scan: {static['total']}), "
      f"point times {moving['point_times'].min():.4f} .. {moving['point_times'].max():.4f} s")
a, b = engine.split_frames(moving, "point3"), engine.split_frames(static, "point3")
ia, ib = engine.split_frames(moving, "index"), engine.split_frames(static, "index")
_, x, y = np.intersect1d(ia[0], ib[0], return_indices=True)
d = np.linalg.norm(a[0][x] - b[0][y], axis=1)
print(f"sweep 0: a ray that hits in both scans moves its point by {np.median(d) * 100:.2f} cm (median), "
      f"{d.max() * 100:.2f} cm (max)")

scene = sim.run_simulation(waypoints)
f = scene.frames[0]
print(f"run_simulation: {scene.get_total_frames()} frames, frame 0 has {len(f.points)} points, "
      f"times in [{f.point_times.min():.4f}, {f.point_times.max():.4f}] s")
