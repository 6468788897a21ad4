#!/usr/bin/env python3
"""A walking pedestrian: the walker of synth.make_walker swings its legs and arms while it crosses a synthetic room next to a
rigid pedestrian.  The walker's scene is built once from keyframe 0; every frame blends two keyframes and refits the tree on
the GPU (lidarcast.deform), then the frame is scanned like any frame with movers.  Once through the engine
(deform.scan_deforming_frames) and once through the simulator (an ``animation`` entry under the ``movers`` key), which also
writes the movers' tracks with each frame's shape.

    python examples/walking_pedestrian.py
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import deform, synth  # noqa: E402
from lidarcast.movers import MoverSet, MoverTrack  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
period = 0.1
paths = [[[0.0, 1.2, 3.1, 0.0, -5.0], [1.5, 4.0, 2.9, 0.0, -5.0]],        # the walker, beside the sensor's line
         [[0.0, 4.4, 1.1, 0.0, 170.0], [1.5, 2.4, 1.2, 0.0, 170.0]]]      # a rigid pedestrian coming the other way
animation = {"cycle": 1.0, "phase": 0.0, "loop": True}                    # one stride per second
objects = [{"mesh": "walker", "semantic": 13, "instance": 1001, "path": paths[0], "animation": animation},
           {"mesh": "pedestrian", "semantic": 13, "instance": 1002, "path": paths[1]}]

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}, "movers": {"period": period, "objects": objects}}, use_dense_lidar=True)
sim.load_scene(mesh, "walking_room")
engine, sensor = sim.raycast_engine, sim.lidar_config

poses = poses_from_waypoints(waypoints)
times = np.arange(len(waypoints)) * period
mover_poses = np.stack([MoverTrack(p).poses12(times) for p in paths], axis=1)        # (P, M, 12) float32
walker = synth.make_walker(instance=1001)
body = deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
movers = MoverSet(engine.ctx, [body, synth.make_pedestrian(instance=1002)])
clip = deform.Clip(len(walker.keyframes), **animation)
shapes = clip.shapes3(times)[:, None, :]                                              # (P, D = 1, 3): [k0, k1, w] per frame
fr = deform.scan_deforming_frames(engine, sensor, poses, mesh, movers, mover_poses, shapes, want=("point3", "sem", "ins"))
who = np.bincount(fr["mover"], minlength=3)
print(f"scan_deforming_frames: {fr['total']} points: {who[0]} from the room, {who[1]} from the walker, {who[2]} from the pedestrian; "
      f"one shape change is {body.launches()[0]} kernel launches, no rebuild")
ends = np.cumsum(fr["counts"])
for f in (0, 3, 8):
    ids = fr["mover"][ends[f] - fr["counts"][f]:ends[f]]
    pts = fr["point3"][ends[f] - fr["counts"][f]:ends[f]][ids == 1]
    span = np.ptp(pts @ mover_poses[f, 0].reshape(3, 4)[:, 0]) if len(pts) else 0.0      # along the walker's own x axis
    print(f"  frame {f:2d} (t = {times[f]:.1f} s, shape {shapes[f, 0].tolist()}): {len(pts)} points on the walker, "
          f"{span:.2f} m from heel to toe")
movers.close()
body.close()

scene = sim.run_simulation(waypoints)
out = tempfile.mkdtemp(prefix="walking_pedestrian_")
tracks = scene.export_mover_tracks(out)
f3 = tracks["frames"][3]
print(f"run_simulation with an animation entry: {scene.get_total_frames()} frames; frame 3 has {len(scene.frames[3].points)} points, "
      f"{[m['num_points'] for m in f3['movers']]} on the movers; the walker's shape is {f3['movers'][0]['shape']} and its box "
      f"{[round(v, 2) for v in f3['movers'][0]['box7']]}")
print("tracks written to", os.path.join(out, "walking_room_mover_tracks.json"))
