#!/usr/bin/env python3
"""Moving objects: two pedestrians walk through a synthetic room while the sensor drives along its middle.  The room is built
once; every frame traces each pedestrian in its own frame and keeps the nearest return, so a pedestrian hides the room behind
it, the room hides a pedestrian, and every point says which mover it came from.  Once through the engine
(RaycastEngineGPU.scan_mover_frames) and once through the simulator (config key ``movers``), which also writes the movers'
ground-truth tracks.

    python examples/moving_objects.py
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import synth  # noqa: E402
from lidarcast.movers import MoverSet, MoverTrack  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
period = 0.1
paths = [[[0.0, 1.2, 3.1, 0.0, -5.0], [1.5, 4.0, 2.9, 0.0, -5.0]],                         # beside the sensor's line, overtaken
         [[0.0, 4.4, 1.1, 0.0, 170.0], [0.8, 3.4, 1.0, 0.0, -170.0], [1.5, 2.4, 1.2, 0.0, -160.0]]]   # towards it, turning through 180
objects = [{"mesh": "pedestrian", "semantic": 13, "instance": 1001 + m, "path": p} for m, p in enumerate(paths)]

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}, "movers": {"period": period, "objects": objects}}, use_dense_lidar=True)
sim.load_scene(mesh, "moving_room")
engine, sensor = sim.raycast_engine, sim.lidar_config

poses = poses_from_waypoints(waypoints)
times = np.arange(len(waypoints)) * period
mover_poses = np.stack([MoverTrack(p).poses12(times) for p in paths], axis=1)        # (P, M, 12) float32
movers = MoverSet(engine.ctx, [synth.make_pedestrian(instance=1001 + m) for m in range(len(paths))])
clean = engine.scan_frames(sensor, poses, mesh, want=("point3", "sem"))
fr = engine.scan_mover_frames(sensor, poses, mesh, movers, mover_poses, want=("point3", "sem", "ins"))
who = np.bincount(fr["mover"], minlength=3)
print(f"scan_mover_frames: {fr['total']} points ({clean['total']} in the clean scan): {who[0]} from the room, "
      f"{who[1]} and {who[2]} from the two pedestrians")
ends = np.cumsum(fr["counts"])
for f in (0, len(poses) // 2, len(poses) - 1):
    ids = fr["mover"][ends[f] - fr["counts"][f]:ends[f]]
    print(f"  frame {f:2d} (t = {times[f]:.1f} s): {np.bincount(ids, minlength=3)[1:].tolist()} points on the pedestrians")

# no movers: the clean scan, byte for byte
same = engine.scan_mover_frames(sensor, poses, mesh, None, None, want=("point3",))
print("a scan without movers equals the clean scan:", bool(np.array_equal(same["point3"], clean["point3"])))
movers.close()

scene = sim.run_simulation(waypoints)
out = tempfile.mkdtemp(prefix="moving_objects_")
tracks = scene.export_mover_tracks(out)
f8 = tracks["frames"][8]
print(f"run_simulation with the movers key: {scene.get_total_frames()} frames; frame 8 has {len(scene.frames[8].points)} points, "
      f"{[m['num_points'] for m in f8['movers']]} on the movers, whose boxes are "
      f"{[[round(v, 2) for v in m['box7']] for m in f8['movers']]}")
print("tracks written to", os.path.join(out, "moving_room_mover_tracks.json"))
