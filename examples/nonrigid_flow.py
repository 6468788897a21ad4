#!/usr/bin/env python3
"""Non-rigid scene flow: a walking person (synth.make_walker, a deforming mover) crosses a synthetic room while the sensor drives
along its middle.  For every point of frame k the scan says where ITS point of the surface will be at frame k + 1 -- the rigid
step of the walk plus the swing of the limb the point lies on -- and whether that place can be seen from the sensor's next pose.
Once through the engine (lidarcast.deform.scan_deforming_flow_frames) and once through the simulator (config key ``movers`` with
``nonrigid_flow: true``), which writes the ground truth with the shapes as one .npz.

    python examples/nonrigid_flow.py
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import deform, flow, synth  # noqa: E402
from lidarcast.movers import MoverSet, MoverTrack  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
period, cycle = 0.1, 0.8
path = [[0.0, 1.2, 3.1, 0.0, -5.0], [1.5, 4.0, 2.9, 0.0, -5.0]]           # beside the sensor's line, overtaken
objects = [{"mesh": "walker", "semantic": 13, "instance": 1001, "path": path, "animation": {"cycle": cycle}}]

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}, "movers": {"period": period, "objects": objects, "nonrigid_flow": True}},
                     use_dense_lidar=True)
sim.load_scene(mesh, "walker_room")
engine, sensor = sim.raycast_engine, sim.lidar_config

poses = poses_from_waypoints(waypoints)
times = np.arange(len(waypoints)) * period
mover_poses = MoverTrack(path).poses12(times)[:, None, :]                  # (P, 1, 12) float32
walker = synth.make_walker(instance=1001)
shapes = deform.Clip(len(walker.keyframes), cycle).shapes3(times)[:, None, :]          # (P, 1, 3): [k0, k1, w] per frame
body = deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
movers = MoverSet(engine.ctx, [body])
fr = deform.scan_deforming_flow_frames(engine, sensor, poses, mesh, movers, mover_poses, shapes, want=("point3", "sem", "ins"))
rigid_step = np.linalg.norm(np.diff(mover_poses[:, 0, [3, 7, 11]], axis=0), axis=1)     # the walk alone, per frame
movers.close()
body.close()
names = dict(enumerate(flow.STATUS_NAMES))
ends = np.cumsum(fr["counts"])
print(f"scan_deforming_flow_frames: {fr['total']} points in {len(poses)} frames")
for f in range(len(poses)):
    sl = slice(ends[f] - fr["counts"][f], ends[f])
    st, who, fl = fr["flow_status"][sl], fr["mover"][sl], fr["flow"][sl]
    on = who == 1
    limb = np.linalg.norm(fl[on], axis=1).max() if on.any() else 0.0
    step = rigid_step[f] if f < len(rigid_step) else 0.0
    print(f"  frame {f:2d}: " + ", ".join(f"{names[s]} {int((st == s).sum())}" for s in range(4)) +
          f"; {int(on.sum())} points on the walker, largest flow {limb:.3f} m (the walk alone: {step:.3f} m)")

scene = sim.run_simulation(waypoints)
out = tempfile.mkdtemp(prefix="nonrigid_flow_")
arrays = scene.export_scene_flow(out)
print(f"run_simulation with movers: {{..., nonrigid_flow: true}}: {scene.get_total_frames()} frames, {len(arrays['points'])} points, "
      f"status counts {np.bincount(arrays['status'], minlength=4).tolist()} (none, visible, occluded, out of range); shapes of frame 3: "
      f"{arrays['mover_shapes'][3, 0].tolist()}")
print("scene flow written to", os.path.join(out, "walker_room_scene_flow.npz"))
