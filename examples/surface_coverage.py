#!/usr/bin/env python3
"""Surface coverage on synth_A6_office2: what the simulator's planned trajectory saw of the room, per semantic class,
and the greedy next-best-view list over all planner candidates' poses that reaches 90 % of what they see together.
Needs an MI355X."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402

from lidarcast import synth  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import poses_from_waypoints  # noqa: E402


def main():
    mesh = synth.make_scene("synth_A6_office2")
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    sim.load_scene(mesh, "synth_A6_office2")
    np.random.seed(0)
    wps, _ = sim.generate_auto_trajectory(num_waypoints=20)
    rep = sim.evaluate_surface_coverage(wps)
    print(f"trajectory: {rep['num_poses']} poses saw {rep['covered_area_m2']:.2f} of {rep['total_area_m2']:.2f} m^2 "
          f"({100 * rep['ratio']:.1f} %), {rep['redundancy_returns_per_m2']:.0f} returns per m^2")
    for name, c in rep["per_class"].items():
        print(f"  {name:10s} {c['covered_m2']:8.2f} / {c['total_m2']:8.2f} m^2  {100 * c['ratio']:5.1f} %")

    # every pose of every planner candidate is a candidate view
    gen = sim.auto_trajectory_generator
    np.random.seed(0)
    gen.room_analysis = gen._analyze_room_layout(mesh, sim._bounds_dict())
    cands = gen._generate_trajectory_candidates(max(int(20 * gen.interpolation_density), gen.min_waypoints))
    poses = np.concatenate([poses_from_waypoints(c.waypoints) for c in cands])
    eng = sim.raycast_engine
    union = eng.surface_coverage(sim.lidar_config, poses, mesh)
    target = 0.9 * union.ratio
    picks, gains, cum = eng.select_views(sim.lidar_config, poses, mesh, budget=len(poses), target_ratio=target)
    print(f"{len(poses)} candidate views see {100 * union.ratio:.1f} % together; {len(picks)} of them reach 90 % of that "
          f"({100 * cum[-1]:.1f} %):")
    for k, (p, g, c) in enumerate(zip(picks, gains, cum)):
        if k == 10 and len(picks) > 11:
            print(f"  ... {len(picks) - 11} more ...")
        if 10 <= k < len(picks) - 1:
            continue
        x, y, z = poses[p][:3, 3]
        print(f"  {k + 1:3d}. pose {p:4d} at ({x:.2f}, {y:.2f}, {z:.2f})  +{g:6.2f} m^2  -> {100 * c:5.1f} %")


if __name__ == "__main__":
    main()
