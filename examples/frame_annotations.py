#!/usr/bin/env python3
"""Per-frame detection annotations on synth_A6_office2: scan the benchmark's trajectory (64 poses on the line x = 1..4 m,
y = 2, z = 1) with the dense 32-line sensor, reduce every frame's returns per object on the GPU and write
<scene>_frame_annotations.json to ./frame_annotations_out/.  Needs an MI355X."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

from lidarcast import synth  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "frame_annotations_out"
    mesh = synth.make_scene("synth_A6_office2")
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}}, use_dense_lidar=True)
    sim.load_scene(mesh, "synth_A6_office2")
    wps = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 64)
    rep = sim.export_frame_annotations(wps, out, min_points=10)
    listed = [len(f["objects"]) for f in rep["frames"]]
    print(f"{rep['num_frames']} frames, {len(rep['objects'])} objects in the room, "
          f"{min(listed)}..{max(listed)} listed per frame (min_points {rep['min_points']})")
    for o in rep["frames"][0]["objects"]:
        c = o["box7"]
        print(f"  frame 0: {o['class']:9s} ins {o['ins']:3d}  {o['num_points']:6d} points  seen {100 * o['seen_ratio']:5.1f} %  "
              f"box centre ({c[0]:+.2f}, {c[1]:+.2f}, {c[2]:+.2f}) size ({c[3]:.2f}, {c[4]:.2f}, {c[5]:.2f})")
    print(f"wrote {os.path.join(out, 'synth_A6_office2_frame_annotations.json')}")


if __name__ == "__main__":
    main()
