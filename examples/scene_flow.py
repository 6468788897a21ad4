#!/usr/bin/env python3
"""Scene flow: two pedestrians walk through a synthetic room while the sensor drives along its middle.  For every point of
frame k the scan also says where the surface under it will be at frame k + 1 (zero for the room, the pedestrian's rigid step for
a pedestrian) and whether that place can be seen from the sensor's next pose: visible, occluded or out of range -- the occlusion
mask scene-flow benchmarks ship.  Once through the engine (RaycastEngineGPU.scan_flow_frames) and once through the simulator
(config key ``movers`` with ``flow: true``), which writes the ground truth as one .npz.

    python examples/scene_flow.py
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import flow, synth  # noqa: E402
from lidarcast.movers import MoverSet, MoverTrack  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
period = 0.1
paths = [[[0.0, 1.2, 3.1, 0.0, -5.0], [1.5, 4.0, 2.9, 0.0, -5.0]],                         # beside the sensor's line, overtaken
         [[0.0, 4.4, 1.1, 0.0, 170.0], [0.8, 3.4, 1.0, 0.0, -170.0], [1.5, 2.4, 1.2, 0.0, -160.0]]]   # towards it, turning through 180
objects = [{"mesh": "pedestrian", "semantic": 13, "instance": 1001 + m, "path": p} for m, p in enumerate(paths)]

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}, "movers": {"period": period, "objects": objects, "flow": True}},
                     use_dense_lidar=True)
sim.load_scene(mesh, "flow_room")
engine, sensor = sim.raycast_engine, sim.lidar_config

poses = poses_from_waypoints(waypoints)
times = np.arange(len(waypoints)) * period
mover_poses = np.stack([MoverTrack(p).poses12(times) for p in paths], axis=1)        # (P, M, 12) float32
movers = MoverSet(engine.ctx, [synth.make_pedestrian(instance=1001 + m) for m in range(len(paths))])
fr = engine.scan_flow_frames(sensor, poses, mesh, movers, mover_poses, want=("point3", "sem", "ins"))
movers.close()
names = dict(enumerate(flow.STATUS_NAMES))
ends = np.cumsum(fr["counts"])
print(f"scan_flow_frames: {fr['total']} points in {len(poses)} frames")
for f in (0, len(poses) // 2, len(poses) - 1):
    sl = slice(ends[f] - fr["counts"][f], ends[f])
    st, who, fl = fr["flow_status"][sl], fr["mover"][sl], fr["flow"][sl]
    speed = np.linalg.norm(fl[who > 0], axis=1) / period if (who > 0).any() else np.zeros(1)
    print(f"  frame {f:2d}: " + ", ".join(f"{names[s]} {int((st == s).sum())}" for s in range(4)) +
          f"; {int((who > 0).sum())} points on the pedestrians move at up to {speed.max():.2f} m/s, "
          f"{int(((who > 0) & (st == flow.OCCLUDED)).sum())} of them out of sight next")
f = 3
sl = slice(ends[f] - fr["counts"][f], ends[f])
sensor_frame = flow.sensor_flow(fr["point3"][sl], fr["flow"][sl], poses[f], poses[f + 1])
print(f"  frame {f} in the sensor's own coordinates: static points flow by {np.linalg.norm(sensor_frame[fr['mover'][sl] == 0], axis=1).mean():.3f} m "
      f"(the sensor's own step), pedestrians by {np.linalg.norm(sensor_frame[fr['mover'][sl] > 0], axis=1).mean():.3f} m")

scene = sim.run_simulation(waypoints)
out = tempfile.mkdtemp(prefix="scene_flow_")
arrays = scene.export_scene_flow(out)
print(f"run_simulation with movers: {{..., flow: true}}: {scene.get_total_frames()} frames, {len(arrays['points'])} points, status counts "
      f"{np.bincount(arrays['status'], minlength=4).tolist()} (none, visible, occluded, out of range)")
print("scene flow written to", os.path.join(out, "flow_room_scene_flow.npz"))
