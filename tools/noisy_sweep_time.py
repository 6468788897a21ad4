#!/usr/bin/env python3
"""Noisy moving-sensor sweeps on C3 (bench.SCENE, 32 x 2048 rays x 64 poses): the scan + compaction step, four ways.

  clean         lrc_scan_poses_dev + lrc_compact_dev           GEN = 1   (what exists without either effect)
  sweeps        lrc_scan_sweeps_dev + lrc_compact_dev          GEN = 4   10 Hz sweeps at --speed m/s and --turn rad/s
  noisy         lrc_scan_noisy_dev + lrc_compact_dev           GEN = 5   the sensor record's noise model
  noisy_sweeps  lrc_scan_noisy_sweeps_dev + lrc_compact_dev    GEN = 8   both: the same records, the same model

Same start poses, same output columns (t, point3, sem, ins, tile_count -> packed rows and counts).  --warmup rounds first, then
--steps rounds in one process, the order flipped every round; HIP events around each step.  Prints medians and minima, every
step against the clean one, and the new step against the sum of the two increments it joins.  --out appends the result to a
text file (profiles/noisy_sweep_c3.txt).

    python tools/noisy_sweep_time.py --steps 40 --warmup 5 --out profiles/noisy_sweep_c3.txt
    python tools/noisy_sweep_time.py --only noisy_sweeps --steps 5     # those launches alone
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

NAMES = ["clean", "sweeps", "noisy", "noisy_sweeps"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--speed", type=float, default=0.5)
    ap.add_argument("--turn", type=float, default=1.0)
    ap.add_argument("--only", choices=NAMES)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, motion_records, noise, synth
    from lidarcast._capi import LrcCompactIO
    from trajectory import line_trajectory, sweep_end_poses
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    wps = line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), bench.POSES_PER_GPU)      # the C3 poses, as tools/sweep_time.py
    for w in wps:
        w.angular_velocity = a.turn
    starts = bench.c3_poses(0, 1)
    rec = motion_records(starts, sweep_end_poses(wps, sensor.scan_frequency, a.speed))
    lid = IndoorLidar(sensor, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    model = noise.NoiseModel.from_intrinsics(sensor, seed=20261019)
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(starts), len(dirs)
    n = P * N
    poses_t = torch.from_numpy(starts.reshape(P, 16).copy()).cuda()
    motion_t = torch.from_numpy(rec).cuda()
    dirs_t, fire_t = torch.from_numpy(dirs).cuda(), torch.from_numpy(fire).cuda()
    hits = DeviceHits(n, "cuda", want=("t", "point3", "sem", "ins", "tile_count"))
    rows = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros((P,), dtype=torch.int64, device="cuda")
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[k].data_ptr() for k in ("t", "point3", "sem", "ins"))
    io.tile_count = hits["tile_count"].data_ptr()
    io.out_xyzl, io.counts = rows.data_ptr(), counts.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    R = sensor.max_range
    scan = {"clean": lambda: scene.scan_poses_dev(poses_t, dirs_t, hits, R, stream=stream),
            "sweeps": lambda: scene.scan_sweeps_dev(motion_t, dirs_t, fire_t, hits, R, stream=stream),
            "noisy": lambda: scene.scan_noisy_dev(poses_t, dirs_t, hits, R, model, stream=stream),
            "noisy_sweeps": lambda: noise.scan_noisy_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, R, model, stream=stream)}
    names = [a.only] if a.only else NAMES

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scan[name]()
        ctx.compact_dev(P, N, io, stream)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), int(counts.sum().item())
    for _ in range(a.warmup):
        for k in names:
            timed(k)
    ms, kept = {k: [] for k in names}, {}
    for step in range(a.steps):
        for k in (names if step % 2 == 0 else names[::-1]):     # alternate which one goes first
            e, kept[k] = timed(k)
            ms[k].append(e)
    out = {"workload": f"C3 {bench.SCENE} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses", "rays": n,
           "steps": a.steps, "warmup": a.warmup, "speed_m_s": a.speed, "turn_rad_s": a.turn,
           "rotation_per_sweep_rad": float(2 * np.arccos(min(rec[0, 12], 1.0))),
           "model": {"range_std_m": model.range_std, "angle_std_rad": model.angle_std, "dropout": model.dropout}}
    for k in names:
        v = np.array(ms[k])
        out[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "kept_points": kept[k]}
    if not a.only:
        for stat in ("median_ms", "min_ms"):
            over = {k: out[k][stat] / out["clean"][stat] - 1.0 for k in NAMES[1:]}
            out[f"over_clean_{stat[:-3]}"] = {k: round(v, 4) for k, v in over.items()}
            out[f"sum_of_sweeps_and_noisy_over_clean_{stat[:-3]}"] = round(over["sweeps"] + over["noisy"], 4)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
