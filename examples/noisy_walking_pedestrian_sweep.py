#!/usr/bin/env python3
"""Seeded sensor noise under movers in sweeps: a walking person, legs and arms swinging, seen from a sensor that drives through a
synthetic room and fires its columns one after the other -- with range noise, angle jitter and dropped returns drawn in the
kernels.  The noise cannot be added afterwards: the jitter decides whether a ray meets the room or the walker, a dropped ray is
never cast, and the range filter acts on the noisy range.  Once through lidarcast.deform.scan_deforming_sweep_frames(...,
noise=...) and once through the simulator (``motion: {speed, movers: {sensor_noise: {seed}, per_ray_shape: true, ...}}``), which
also writes the ground-truth tracks with the noise model.  Sweep p has frame id p, so any run of sweeps can be scanned again with
its exact noise.

    python examples/noisy_walking_pedestrian_sweep.py
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
from lidarcast.noise import NoiseModel  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints, sweep_end_poses  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
period, speed, seed = 0.1, 0.5, 7
path = [[0.0, 0.8, 3.0, 0.0, 0.0], [1.6, 3.0, 2.9, 0.0, 0.0]]              # 1.4 m/s beside the sensor's line
animation = {"cycle": 0.8, "phase": 0.1}                                   # two steps in 0.8 s
objects = [{"mesh": "walker", "semantic": 13, "instance": 1001, "path": path, "animation": animation}]

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True},
                      "motion": {"speed": speed, "movers": {"period": period, "per_ray_shape": True, "sensor_noise": {"seed": seed},
                                                            "objects": objects}}},
                     use_dense_lidar=True)
sim.load_scene(mesh, "noisy_walking_room")
engine, sensor = sim.raycast_engine, sim.lidar_config
model = NoiseModel.from_intrinsics(sensor, seed)           # the sensor record's own range noise, angle jitter and dropout
print(f"noise model: range_std {model.range_std} m, angle_std {np.degrees(model.angle_std):.4f} degrees, dropout {model.dropout}")

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
args = (engine, sensor, start, end, mesh, movers, records, shapes_a, shapes_b)
clean = deform.scan_deforming_sweep_frames(*args, want=want)
noisy = deform.scan_deforming_sweep_frames(*args, want=want, noise=model)
# sweeps 8.. alone, with their own first frame: the same bytes
tail = deform.scan_deforming_sweep_frames(engine, sensor, start[8:], end[8:], mesh, movers, records[8:], shapes_a[8:], shapes_b[8:],
                                          want=want, noise=model.at_frame(8))
movers.close()
d.close()
off = int(noisy["counts"][:8].sum())
assert np.array_equal(tail["point3"], noisy["point3"][off:]) and np.array_equal(tail["mover"], noisy["mover"][off:])
print(f"clean: {clean['total']} points, {int((clean['mover'] == 1).sum())} on the walker; "
      f"noisy: {noisy['total']} points, {int((noisy['mover'] == 1).sum())} on the walker; sweeps 8.. scanned again alone: the same bytes")
ends_c, ends_n = np.cumsum(clean["counts"]), np.cumsum(noisy["counts"])
for f in (2, len(start) // 2, len(start) - 3):
    rc, rn = slice(ends_c[f] - clean["counts"][f], ends_c[f]), slice(ends_n[f] - noisy["counts"][f], ends_n[f])
    on_c, on_n = clean["mover"][rc] == 1, noisy["mover"][rn] == 1
    # the rays that end on the walker in both scans, matched by their index in the sweep
    _, i, j = np.intersect1d(clean["index"][rc][on_c], noisy["index"][rn][on_n], return_indices=True)
    moved = np.linalg.norm(clean["point3"][rc][on_c][i] - noisy["point3"][rn][on_n][j], axis=1) if len(i) else np.zeros(1)
    print(f"  sweep {f:2d}: the walker returns {int(on_c.sum())} points clean and {int(on_n.sum())} noisy; a ray that ends on it in "
          f"both scans lands up to {moved.max() * 100:.1f} cm elsewhere")

scene = sim.run_simulation(waypoints)
out = tempfile.mkdtemp(prefix="noisy_walking_pedestrian_sweep_")
tracks = scene.export_mover_tracks(out)
f8 = tracks["frames"][8]
print(f"run_simulation with sensor_noise: {scene.get_total_frames()} frames; frame 8 has {f8['returns']} returns with point_times and "
      f"mover_ids, {f8['movers'][0]['num_points']} on the walker; the tracks file holds the model {tracks['noise']}")
assert np.array_equal(np.asarray(scene.frames[8].points, np.float32),
                      noisy["point3"][ends_n[8] - noisy["counts"][8]:ends_n[8]])          # the simulator's frames are this scan
print("tracks written to", os.path.join(out, "noisy_walking_room_mover_tracks.json"))
