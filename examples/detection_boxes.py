#!/usr/bin/env python3
"""Detection boxes without the cloud leaving the GPU: scan synth_A6_office2 through the scan pipeline (C3 sensor,
32 lines x 2048 azimuths, 64 poses), hand the pipeline's (K,4) rows to lidarcast.instance_boxes_dev (per-instance
k-NN outlier filter and AABB, one call), and write the Group-Free-3D annotation file the reference's
lidar_net_bbox_visualizer.py would write for the same labelled cloud.

    python examples/detection_boxes.py [out_dir]      # default: detection_boxes_out/
"""
import dataclasses
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lidarcast  # noqa: E402
from lidar import IndoorLidar, Indoor8LineLidarIntrinsics  # noqa: E402
from lidar_net_bbox_visualizer import S3DIS_SEMANTIC_MAPPING, LiDARNetBBoxVisualizer  # noqa: E402
from lidarcast import synth  # noqa: E402
from trajectory import line_trajectory, poses_from_waypoints  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else "detection_boxes_out"
mesh = synth.make_scene("synth_A6_office2")
sensor = dataclasses.replace(Indoor8LineLidarIntrinsics.create_dense_32line(), horizontal_res=2048)
poses = poses_from_waypoints(line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 64))
dirs = IndoorLidar(intrinsics=sensor, pose=np.eye(4)).sensor_directions()
P, N = poses.shape[0], dirs.shape[0]

ctx = lidarcast.Context(0)
scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
pipe = lidarcast.ScanPipe(scene, P, N)
rows = torch.empty((P * N, 4), dtype=torch.float32, device="cuda")     # x, y, z, sem | ins << 16
counts = torch.zeros(P, dtype=torch.int64, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
pipe.submit(torch.from_numpy(poses.reshape(P, 16)).cuda(), torch.from_numpy(dirs).cuda(), sensor.max_range,
            out_rows_t=rows, counts_t=counts, stream=stream)
pipe.wait(stream)
K = int(counts.sum())

boxes = lidarcast.instance_boxes_dev(ctx, rows[:K], list(S3DIS_SEMANTIC_MAPPING.values()), stream=stream)
vis = LiDARNetBBoxVisualizer(S3DIS_SEMANTIC_MAPPING, ctx=ctx)
bboxes = vis.bboxes_from_boxes(boxes)
os.makedirs(out_dir, exist_ok=True)
path = os.path.join(out_dir, "synth_A6_office2_detection_annotations.json")
vis.generate_detection_annotations(bboxes, path)
print(f"{K} rows, {len(boxes)} instances, {len(bboxes)} boxes accepted -> {path}")
for b in bboxes:
    print(f"  {b['object_name']:9s} ins {int(b['instance_id']):3d}: {b['point_count']:6d} points, "
          f"size {np.round(b['size'], 3).tolist()}")
pipe.close()
scene.close()
