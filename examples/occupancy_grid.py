#!/usr/bin/env python3
"""Semantic occupancy grid on synth_A6_office2: scan the simulator's planned trajectory, carve free space along every
returned ray and write <scene>_occupancy.npz, <scene>_occupancy.json and <scene>_occupied_voxels.ply to
./occupancy_grid_out/.  Needs an MI355X."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402

from lidarcast import synth  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "occupancy_grid_out"
    mesh = synth.make_scene("synth_A6_office2")
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    sim.load_scene(mesh, "synth_A6_office2")
    np.random.seed(0)
    wps, _ = sim.generate_auto_trajectory(num_waypoints=20)
    rep = sim.export_occupancy_grid(wps, out, voxel_size=0.05)
    c = rep["counts"]
    total = c["free"] + c["occupied"] + c["unknown"]
    print(f"{rep['num_poses']} poses, grid {rep['dims']} at {rep['voxel_size']} m from {rep['origin']}")
    print(f"  occupied {c['occupied']:9d}  ({100 * c['occupied'] / total:5.2f} %), {c['returns']} returns")
    print(f"  free     {c['free']:9d}  ({100 * c['free'] / total:5.2f} %)")
    print(f"  unknown  {c['unknown']:9d}  ({100 * c['unknown'] / total:5.2f} %)")
    for name, n in sorted(rep["per_class_occupied_voxels"].items(), key=lambda kv: -kv[1]):
        print(f"    {name:10s} {n:8d} occupied voxels")
    z = np.load(os.path.join(out, "synth_A6_office2_occupancy.npz"))
    print(f"wrote {out}/: state {z['state'].shape} {z['state'].dtype}, sem / ins / returns, json, occupied-voxel ply")


if __name__ == "__main__":
    main()
