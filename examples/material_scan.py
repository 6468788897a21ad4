#!/usr/bin/env python3
"""Surface materials: the bookcases of a synthetic room are glass and its tables mirrors.  A ray that meets one of them is
continued inside the trace kernel: glass is seen only near normal incidence and looked through otherwise, a mirror puts ghost
points behind the wall, and every point carries an intensity that depends on the surface.  Once through the engine
(RaycastEngineGPU.scan_material_frames) and once through the simulator (config key ``materials``).

    python examples/material_scan.py
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
from lidarcast import synth  # noqa: E402
from lidarcast.material import MaterialTable  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints  # noqa: E402

mesh = synth.make_room(size=(5.0, 4.0, 2.8), num_boxes=6, seed=2, cell=0.04)
waypoints = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 16, yaw=0.2)
classes = {"bookcase": {"kind": "glass", "pass": 0.9, "albedo": 0.1, "retro_deg": 3},
           "table": {"kind": "mirror", "pass": 0.95, "albedo": 0.05, "retro_deg": 3}}

sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}, "materials": {"max_bounces": 4, "min_intensity": 0.0, "classes": classes}},
                     use_dense_lidar=True)
sim.load_scene(mesh, "material_room")
engine, sensor = sim.raycast_engine, sim.lidar_config
table = MaterialTable.from_classes(classes, max_bounces=4)
print(table)

poses = poses_from_waypoints(waypoints)
clean = engine.scan_frames(sensor, poses, mesh, want=("point3", "sem"))
fr = engine.scan_material_frames(sensor, poses, mesh, table, want=("point3", "sem"))
b = fr["bounces"]
print(f"scan_material_frames: {fr['total']} points ({clean['total']} in the clean scan); returns after 0..4 panes or mirrors: "
      f"{np.bincount(b, minlength=5).tolist()}")
ghost = b > 0
off = np.linalg.norm(fr["point3"][ghost] - fr["surface_point3"][ghost], axis=1)
print(f"points that came over a mirror or through glass lie {off.mean():.2f} m (mean) from the surface that returned them; "
      f"their mean intensity is {fr['intensity'][ghost].mean():.3f} against {fr['intensity'][~ghost].mean():.3f} for direct returns")
own = (~ghost) & np.isin(fr["sem"], (7, 10))
print(f"{int(own.sum())} returns come from the glass and the mirrors themselves (incidence within 3 degrees of the normal)")

# the all-diffuse table is the clean scan
same = engine.scan_material_frames(sensor, poses, mesh, MaterialTable.diffuse(13), want=("point3",))
print("all-diffuse table equals the clean scan:", bool(np.array_equal(same["point3"], clean["point3"])))

scene = sim.run_simulation(waypoints)
f0 = scene.frames[0]
print(f"run_simulation with the materials key: {scene.get_total_frames()} frames, frame 0 has {len(f0.points)} points, "
      f"{int((f0.bounces > 0).sum())} of them over a mirror or through glass, intensities {f0.intensities.min():.3f}.."
      f"{f0.intensities.max():.3f}")
