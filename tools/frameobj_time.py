#!/usr/bin/env python3
"""Per-frame object annotation timings: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x 64
poses, bench.c3_poses) on synth_A6_office2, on the records of ONE scan.

HIP events around each call, --warmup rounds first, then --steps rounds, median and minimum:
    scan                 lrc_scan_poses_dev writing t, prim and point3 (the scan step itself)
    coverage_accumulate  lrc_coverage_accumulate_dev on the scan's t and prim (8 B per ray: the yardstick)
    frameobj_accumulate  lrc_frameobj_accumulate_dev on the scan's t, prim and point3 (20 B per ray + the reductions)
Both accumulates run on an object that already holds the trajectory (the steady state: every triangle bit is set after the
first round), and once more right after a reset (the first call of a trajectory, every bit newly set).

    python tools/frameobj_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/frameobj_c3.txt holds this report as a table, with the rows of a rocprofv3 --kernel-trace --stats run of this tool.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def _stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="synth_A6_office2")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, FrameObjects, SurfaceCoverage, synth
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "prim", "point3"))
    cov = SurfaceCoverage(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, num_sets=P)
    fo = FrameObjects(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins, num_frames=P)
    stream = torch.cuda.current_stream().cuda_stream

    run = {"scan": lambda: scene.scan_poses_dev(poses_t, dirs_t, hits, sensor.max_range, stream=stream),
           "coverage_accumulate": lambda: cov.accumulate_dev(hits["t"], hits["prim"], P, N, stream=stream),
           "frameobj_accumulate": lambda: fo.accumulate_dev(hits["t"], hits["prim"], hits["point3"], poses_t, N,
                                                            stream=stream)}
    reset = {"coverage_accumulate": lambda: cov.reset(stream), "frameobj_accumulate": lambda: fo.reset(stream)}

    def timed(n, fresh=False):
        if fresh:
            reset[n]()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run[n]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    names = list(run)
    for _ in range(a.warmup):
        for n in names:
            timed(n)
    ms = {n: [] for n in names}
    fresh = {n: [] for n in reset}
    for _ in range(a.steps):
        for n in names:
            ms[n].append(timed(n))
    for _ in range(a.steps):
        for n in reset:
            fresh[n].append(timed(n, fresh=True))
    r = fo.export()
    res = {"workload": f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses", "rays": P * N,
           "triangles": int(len(mesh.triangles)), "objects": r.num_objects,
           "returns_per_frame": int(r.returns[0].sum()), "rows_with_returns": int((r.returns > 0).sum()),
           "rejected_rays": r.rejected_rays}
    res.update({n: _stats(v) for n, v in ms.items()})
    res.update({n + "_after_reset": _stats(v) for n, v in fresh.items()})
    res["frameobj_over_coverage"] = round(res["frameobj_accumulate"]["median_ms"] / res["coverage_accumulate"]["median_ms"], 3)
    res["frameobj_over_scan"] = round(res["frameobj_accumulate"]["median_ms"] / res["scan"]["median_ms"], 3)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/frameobj_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    fo.close()
    cov.close()
    scene.close()


if __name__ == "__main__":
    main()
