#!/usr/bin/env python3
"""Dynamic occupancy on synth_A6_office2: a pedestrian crosses the room while the sensor drives along it.  One occupancy grid
PER FRAME (occupied / free / unknown, sem, ins and the mover id per voxel) and the static map (the room with the pedestrian's
returns left out) go to ./dynamic_occupancy_out/ as <scene>_dynamic_occupancy.npz, <scene>_static_map.npz and
<scene>_dynamic_occupancy.json.  Needs an MI355X."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402

from lidarcast import synth  # noqa: E402
from s3dis_simulator import S3DISSimulator  # noqa: E402
from trajectory import line_trajectory  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "dynamic_occupancy_out"
    name = "synth_A6_office2"
    mesh = synth.make_scene(name)
    sx, sy, _ = synth.scene_size(name)
    frames, period = 12, 0.1
    # the pedestrian walks across the room, the sensor along it
    walk = [[0.0, 0.5 * sx, 0.2 * sy, 0.0, 90.0], [period * (frames - 1), 0.5 * sx, 0.8 * sy, 0.0, 90.0]]
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True},
                          "movers": {"period": period, "objects": [{"mesh": "pedestrian", "semantic": "clutter", "instance": 1001,
                                                                    "path": walk}]}})
    sim.load_scene(mesh, name)
    wps = line_trajectory((0.2 * sx, 0.5 * sy, 1.0), (0.35 * sx, 0.5 * sy, 1.0), frames)
    rep = sim.export_dynamic_occupancy(wps, out, voxel_size=0.05)
    print(f"{rep['num_frames']} frames, grid {rep['dims']} at {rep['voxel_size']} m from {rep['origin']}")
    for fr in rep["frames"]:
        c = fr["counts"]
        print(f"  frame {fr['frame']:2d}: occupied {c['occupied']:7d}  free {c['free']:8d}  unknown {c['unknown']:8d}  "
              f"dynamic voxels per mover {fr['dynamic_voxels_per_mover']}")
    s = rep["static_map"]
    print(f"static map: occupied {s['counts']['occupied']}  free {s['counts']['free']}  unknown {s['counts']['unknown']}  "
          f"dynamic voxels {s['dynamic_voxels_per_mover']}")
    z = np.load(os.path.join(out, f"{name}_dynamic_occupancy.npz"))
    # where the pedestrian stood in frame 0 is free once they have walked on -- a single grid over all frames could not say so
    f0 = z["idx"][int(z["frame_offsets"][0]):int(z["frame_offsets"][1])][z["mover"][int(z["frame_offsets"][0]):int(z["frame_offsets"][1])] != 0]
    later = z["state"][-1].reshape(-1)[f0]
    print(f"of the {len(f0)} voxels the pedestrian occupied in frame 0, {int((later == 1).sum())} are free and "
          f"{int((later == 0).sum())} unknown in frame {rep['num_frames'] - 1}")
    print(f"wrote {out}/: state {z['state'].shape} {z['state'].dtype}, the sparse list with mover / mover_returns, static map, json")


if __name__ == "__main__":
    main()
