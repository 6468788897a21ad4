#!/usr/bin/env python3
"""Moving-sensor sweeps against the static scan on C3 (bench.SCENE, 32 x 2048 rays x 64 poses):

  lrc_scan_sweeps_dev (GEN = 4: motion records, 10 Hz sweeps at 0.5 m/s and 1 rad/s) and lrc_scan_poses_dev (GEN = 1) on the
  SAME start poses, same output columns (t, point3, sem, ins), HIP events around each launch, --warmup launches of each
  first, then --steps rounds that alternate the two in one process.  Prints per-launch medians / minima and their ratio.

    python tools/sweep_time.py --steps 40 --warmup 5
    python tools/sweep_time.py --sweeps-only --steps 5     # the sweep launches alone (for rocprofv3 --kernel-trace --stats)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--speed", type=float, default=0.5)
    ap.add_argument("--turn", type=float, default=1.0)
    ap.add_argument("--sweeps-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, motion_records, synth
    from trajectory import line_trajectory, sweep_end_poses
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    wps = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), bench.POSES_PER_GPU)
    for w in wps:
        w.angular_velocity = a.turn
    starts = bench.c3_poses(0, 1)
    ends = sweep_end_poses(wps, sensor.scan_frequency, a.speed)
    rec = motion_records(starts, ends)
    lid = IndoorLidar(sensor, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(starts), len(dirs)
    poses_t = torch.from_numpy(starts.reshape(P, 16).copy()).cuda()
    motion_t = torch.from_numpy(rec).cuda()
    dirs_t, fire_t = torch.from_numpy(dirs).cuda(), torch.from_numpy(fire).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    stream = torch.cuda.current_stream().cuda_stream
    run = {"static": lambda: scene.scan_poses_dev(poses_t, dirs_t, hits, sensor.max_range, stream=stream),
           "sweeps": lambda: scene.scan_sweeps_dev(motion_t, dirs_t, fire_t, hits, sensor.max_range, stream=stream)}
    names = ["sweeps"] if a.sweeps_only else ["static", "sweeps"]

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(a.warmup):
        for n in names:
            timed(n)
    ms = {n: [] for n in names}
    for step in range(a.steps):
        for n in (names if step % 2 == 0 else names[::-1]):     # alternate which one goes first
            ms[n].append(timed(n))
    out = {"workload": f"C3 {bench.SCENE} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses",
           "rays": P * N, "steps": a.steps, "warmup": a.warmup, "speed_m_s": a.speed, "turn_rad_s": a.turn,
           "rotation_per_sweep_rad": float(2 * np.arccos(min(rec[0, 12], 1.0)))}
    for n in names:
        v = np.array(ms[n])
        out[n] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
                  "grays_per_s_median": round(P * N / np.median(v) / 1e6, 2)}
    if not a.sweeps_only:
        out["sweeps_over_static_median"] = round(out["sweeps"]["median_ms"] / out["static"]["median_ms"], 4)
        out["sweeps_over_static_min"] = round(out["sweeps"]["min_ms"] / out["static"]["min_ms"], 4)
    print(json.dumps(out, indent=1))
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
