#!/usr/bin/env python3
"""Seeded sensor noise on C3 (bench.SCENE, 32 x 2048 rays x 64 poses): the scan + compaction step, three ways.

  clean       lrc_scan_poses_dev + lrc_compact_dev                                  (what exists without noise)
  noisy       lrc_scan_noisy_dev + lrc_compact_dev: range noise, angle jitter and dropout drawn in the kernel
  host noise  the route the noisy scan replaces: np.random normal draw of one float32 per ray on the host, its upload,
              set_options(range_noise=...), lrc_scan_poses_dev + lrc_compact_dev   (range noise only: the option has no
              angle jitter or dropout)

Same poses, same output columns (t, point3, sem, ins, tile_count -> packed rows and counts).  --warmup rounds first, then
--steps rounds that alternate the order.  The device steps are timed with HIP events; the host route is wall clock around
draw + upload + launches + synchronisation, and so are the device steps a second time, to compare like with like.

    python tools/noise_time.py --steps 40 --warmup 5
    python tools/noise_time.py --noisy-only --steps 5     # the noisy launches alone (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noisy-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, synth
    from lidarcast._capi import LrcCompactIO
    from lidarcast.noise import NoiseModel
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    model = NoiseModel.from_intrinsics(sensor, seed=20261018)
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    n = P * N
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    hits = DeviceHits(n, "cuda", want=("t", "point3", "sem", "ins", "tile_count"))
    rows = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros((P,), dtype=torch.int64, device="cuda")
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[k].data_ptr() for k in ("t", "point3", "sem", "ins"))
    io.tile_count = hits["tile_count"].data_ptr()
    io.out_xyzl, io.counts = rows.data_ptr(), counts.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)
    pinned = torch.empty((n,), dtype=torch.float32).pin_memory()
    noise_t = torch.empty((n,), dtype=torch.float32, device="cuda")

    def clean():
        scene.scan_poses_dev(poses_t, dirs_t, hits, sensor.max_range, stream=stream)
        ctx.compact_dev(P, N, io, stream)

    def noisy():
        scene.scan_noisy_dev(poses_t, dirs_t, hits, sensor.max_range, model, stream=stream)
        ctx.compact_dev(P, N, io, stream)

    def host_noise():
        pinned.numpy()[:] = rng.normal(scale=model.range_std, size=n)       # float64 draw, narrowed on assignment
        noise_t.copy_(pinned, non_blocking=True)
        scene.set_options(range_noise=(noise_t.data_ptr(), n))
        try:
            clean()
        finally:
            scene.reset_options()

    run = {"clean": clean, "noisy": noisy, "host_noise": host_noise}
    names = ["noisy"] if a.noisy_only else ["clean", "noisy", "host_noise"]

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        run[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, int(counts.sum().item())
    for _ in range(a.warmup):
        for k in names:
            timed(k)
    ev, wall, kept = {k: [] for k in names}, {k: [] for k in names}, {}
    for step in range(a.steps):
        for k in (names if step % 2 == 0 else names[::-1]):     # alternate which one goes first
            e, w, c = timed(k)
            ev[k].append(e)
            wall[k].append(w)
            kept[k] = c
    out = {"workload": f"C3 {bench.SCENE} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses", "rays": n,
           "steps": a.steps, "warmup": a.warmup,
           "model": {"range_std_m": model.range_std, "angle_std_rad": model.angle_std, "dropout": model.dropout}}
    for k in names:
        e, w = np.array(ev[k]), np.array(wall[k])
        out[k] = {"events_median_ms": round(float(np.median(e)), 4), "events_min_ms": round(float(e.min()), 4),
                  "wall_median_ms": round(float(np.median(w)), 4), "wall_min_ms": round(float(w.min()), 4),
                  "kept_points": kept[k]}
    if not a.noisy_only:
        out["noisy_over_clean_events_median"] = round(out["noisy"]["events_median_ms"] / out["clean"]["events_median_ms"], 4)
        out["noisy_over_clean_events_min"] = round(out["noisy"]["events_min_ms"] / out["clean"]["events_min_ms"], 4)
        out["noisy_over_host_noise_wall_median"] = round(out["noisy"]["wall_median_ms"] / out["host_noise"]["wall_median_ms"], 5)
        out["host_noise_over_noisy_wall_median"] = round(out["host_noise"]["wall_median_ms"] / out["noisy"]["wall_median_ms"], 2)
    print(json.dumps(out, indent=1))
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
