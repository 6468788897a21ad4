#!/usr/bin/env python3
"""Room preprocessing timing on synthetic S3DIS-like rooms (lidarcast.synth.sample_s3dis_room, 3-decimal coordinates,
300 outliers) of about 0.25 M / 1 M / 4 M rows, the reference's parameters (k = 20, std_ratio = 2, radius = 0.1,
max_nn = 30):

  device : lidarcast.preprocess_cloud_dev on a resident float64 tensor, HIP events around each call, warmed up; median
           and min of --calls calls (the call returns once its stream has finished: the figure is end to end);
  host   : S3DISPreprocessor.preprocess_pointcloud from host arrays (upload, device call, download, label handling);
  scipy  : the cKDTree restatement of tests/test_preprocess_gpu.py (outlier avg over all rows, hybrid neighbours,
           cumulant covariance, numpy eigh), workers = 16.  It is NOT Open3D, which is not installed: a CPU yardstick
           only.

    python tools/preprocess_time.py                  # all three
    python tools/preprocess_time.py --device-only    # the device calls alone (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

ROOMS = {"0.25M": ((5.0, 4.0, 3.0), 6, 250_000), "1M": ((6.0, 5.0, 3.0), 8, 1_000_000),
         "4M": ((8.0, 6.0, 3.0), 10, 4_000_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    import lidarcast
    from lidarcast import synth
    ctx = lidarcast.Context(0)
    for name, (size, boxes, n) in ROOMS.items():
        pts, cols, labels = synth.sample_s3dis_room(synth.make_room(size=size, num_boxes=boxes, seed=3), num_points=n,
                                                    num_outliers=300, seed=1)
        t = torch.from_numpy(pts).cuda()
        for _ in range(args.warmup):
            r = lidarcast.preprocess_cloud_dev(ctx, t)
        ms = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = lidarcast.preprocess_cloud_dev(ctx, t)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(f"{name}: rows {len(pts)} kept {len(r.kept)}  device median {np.median(ms):.2f} ms  min {min(ms):.2f} ms",
              flush=True)
        if args.device_only:
            continue
        from s3dis_data_loader import S3DISPreprocessor
        cfg = {"preprocessing": {"remove_outliers": True, "outlier_nb_neighbors": 20, "outlier_std_ratio": 2.0,
                                 "estimate_normals": True, "normal_search_radius": 0.1, "normal_max_nn": 30}}
        pre = S3DISPreprocessor(cfg, ctx=ctx)
        pre.preprocess_pointcloud(pts, cols / 255.0, labels)
        t0 = time.perf_counter()
        pre.preprocess_pointcloud(pts, cols / 255.0, labels)
        host = (time.perf_counter() - t0) * 1e3
        import test_preprocess_gpu as ref
        t0 = time.perf_counter()
        avg = ref.restate_avg(pts, 20)
        mean, thr = ref.restate_filter(avg, 2.0)
        pk = pts[(avg > 0) & (avg < thr)]
        cnt, _, cov = ref.restate_neighbours(pk, 0.1, 30, np.arange(len(pk)))
        np.linalg.eigh(cov[cnt >= 3])
        cpu = (time.perf_counter() - t0) * 1e3
        print(f"{name}:   preprocess_pointcloud {host:.1f} ms   scipy restatement (16 workers, not Open3D) {cpu:.0f} ms",
              flush=True)


if __name__ == "__main__":
    main()
