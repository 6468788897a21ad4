#!/usr/bin/env python3
"""Animated movers under sweeps: a walking person, legs and arms swinging, seen from a sensor that drives through a synthetic room
and fires its columns one after the other.  Every ray meets the walker at the pose AND the shape it has at the moment the ray
fires: within one 0.1 s sweep a swinging foot travels some 15 cm, an order of magnitude above the range noise, so a shape frozen
per sweep is wrong by that much.  Once through lidarcast.deform.scan_deforming_sweep_frames and once through the simulator
(nested config key ``motion: {speed, movers: {per_ray_shape: true, ...}}``), which also writes the ground-truth tracks with the
shape at both ends of every sweep.

    python examples/walking_pedestrian_sweep.py
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import deform, synth  # noqa: E402
from lidarcast.movers import MoverSet, MoverTrack, sweep_records  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints, sweep_end_poses  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
period, speed = 0.1, 0.5
path = [[0.0, 0.8, 3.0, 0.0, 0.0], [1.6, 3.0, 2.9, 0.0, 0.0]]              # 1.4 m/s beside the sensor's line
animation = {"cycle": 0.8, "phase": 0.1}                                   # two steps in 0.8 s
objects = [{"mesh": "walker", "semantic": 13, "instance": 1001, "path": path, "animation": animation}]

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True},
                      "motion": {"speed": speed, "movers": {"period": period, "per_ray_shape": True, "objects": objects}}},
                     use_dense_lidar=True)
sim.load_scene(mesh, "walking_room")
engine, sensor = sim.raycast_engine, sim.lidar_config

start = poses_from_waypoints(waypoints)
end = sweep_end_poses(waypoints, sensor.scan_frequency, speed)
T = 1.0 / sensor.scan_frequency
times = np.arange(len(waypoints)) * period
records = sweep_records([MoverTrack(path)], times, times + T)
walker = synth.make_walker(semantic=13, instance=1001)
clip = deform.Clip(len(walker.keyframes), animation["cycle"], phase=animation["phase"])
shapes_a = clip.shapes3(times)[:, None, :]                 # (P, 1, 3): [k0, k1, w] at the start of every sweep
shapes_b = clip.shapes3(times + T)[:, None, :]             # ... and at its end
d = deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
movers = MoverSet(engine.ctx, [d])
want = ("point3", "sem", "ins", "index")
fr = deform.scan_deforming_sweep_frames(engine, sensor, start, end, mesh, movers, records, shapes_a, shapes_b, want=want)
frozen = deform.scan_deforming_sweep_frames(engine, sensor, start, end, mesh, movers, records, shapes_a, shapes_a, want=want)
movers.close()
d.close()
who = np.bincount(fr["mover"], minlength=2)
print(f"scan_deforming_sweep_frames: {fr['total']} points, {who[1]} of them on the walker")
ends, ends_f = np.cumsum(fr["counts"]), np.cumsum(frozen["counts"])
for f in (2, len(start) // 2, len(start) - 3):
    rows, rows_f = slice(ends[f] - fr["counts"][f], ends[f]), slice(ends_f[f] - frozen["counts"][f], ends_f[f])
    on, on_f = fr["mover"][rows] == 1, frozen["mover"][rows_f] == 1
    # the rays that end on the walker in both scans, matched by their index in the sweep
    _, i, j = np.intersect1d(fr["index"][rows][on], frozen["index"][rows_f][on_f], return_indices=True)
    if len(i):
        gap = np.linalg.norm(fr["point3"][rows][on][i] - frozen["point3"][rows_f][on_f][j], axis=1)
        t = fr["point_times"][rows][on]
        print(f"  sweep {f:2d}: the walker is hit by {int(on.sum())} rays between {t.min() * 1e3:.1f} and {t.max() * 1e3:.1f} ms of the "
              f"sweep ({int(on_f.sum())} with its shape frozen at the sweep's start); a ray that hits it in both scans ends up to "
              f"{gap.max() * 100:.1f} cm elsewhere")

scene = sim.run_simulation(waypoints)
out = tempfile.mkdtemp(prefix="walking_pedestrian_sweep_")
tracks = scene.export_mover_tracks(out)
f8 = tracks["frames"][8]["movers"][0]
print(f"run_simulation with per_ray_shape: {scene.get_total_frames()} frames; frame 8 has {len(scene.frames[8].points)} points with "
      f"point_times and mover_ids, {f8['num_points']} on the walker, whose shape goes from {f8['shape']} to {f8['end_shape']}")
print("tracks written to", os.path.join(out, "walking_room_mover_tracks.json"))
