#!/usr/bin/env python3
"""Beam footprint and multi-echo returns on C3 (bench.SCENE, 32 x 2048 beams x 64 poses), hex7, E = 2: three steps.

  echo      lrc_scan_echoes_dev + lrc_compact_dev over P poses of N * E echo records (no per-tile keep counts: the compaction
            counts itself)
  clean8    lrc_scan_poses_dev + lrc_compact_dev on a table of 8 N directions: the SAME rays in the same lanes -- row 8 i + k
            is sub-ray k of beam i as the echo kernel forms it, lane 7 the axis again -- but every lane writes a record.  Same
            lane count: the difference is what the in-kernel float64 offset and the reduction cost against what not writing
            (and not compacting) 8 N records per pose saves.
  replaced  the route the echo scan replaces: 7 scans with 7 offset tables (t only), the download of 7 P N distances and a
            vectorised numpy reduction to (representative, weight) per echo; wall clock, few rounds (it takes seconds)

--warmup rounds first, then --steps rounds that alternate the order of the two device steps, timed with HIP events (and wall
clock, to set beside the replaced route).

    python tools/echo_time.py --steps 20 --warmup 3
    python tools/echo_time.py --echo-only --steps 5      # the echo launches alone (for rocprofv3 --kernel-trace --stats)
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


def subray_rows(dirs, offsets):
    """(K, N, 3) float64 rows of the sub-rays (include/lidarcast.h, "beam footprint"): the arithmetic of the kernel in numpy."""
    a, b, c = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    h = np.sqrt(a * a + b * b)
    flat = h == 0.0
    hs = np.where(flat, 1.0, h)
    out = np.empty((len(offsets), len(dirs), 3))
    for k, (du, dv) in enumerate(offsets):
        if du == 0.0 and dv == 0.0:
            out[k] = dirs
            continue
        dp = du / hs
        ca, cb = (c * a) / hs, (c * b) / hs
        a1, b1, c1 = (a - dp * b) - dv * ca, (b + dp * a) - dv * cb, c + dv * h
        n = np.sqrt((a1 * a1 + b1 * b1) + c1 * c1)
        out[k] = np.stack([a1 / n, b1 / n, c1 / n], axis=1)
        out[k][flat] = dirs[flat]
    return out


def reduce_numpy(t, E, separation):
    """Vectorised numpy reduction of (B, K) float32 distances (min_count 1): rep (B, E) int8, weight (B, E) uint8."""
    B, K = t.shape
    order = np.argsort(t, axis=1, kind="stable")                    # by (t, k)
    s = np.take_along_axis(t, order, axis=1)
    hit = s < np.inf
    start = hit.copy()
    with np.errstate(invalid="ignore"):
        start[:, 1:] &= (s[:, 1:] - s[:, :-1]) > np.float32(separation)
    cid = np.cumsum(start, axis=1) - 1
    rep = np.full((B, E), -1, np.int8)
    weight = np.zeros((B, E), np.uint8)
    for e in range(E):
        m = hit & (cid == e)
        weight[:, e] = m.sum(axis=1)
        rep[:, e] = np.where(m, order, K).min(axis=1)
    rep[weight == 0] = -1
    return rep, weight


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--divergence-mrad", type=float, default=3.0)
    ap.add_argument("--echo-only", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, synth
    from lidarcast._capi import LrcCompactIO
    from lidarcast.echo import BeamModel
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    beam = BeamModel(a.divergence_mrad * 1e-3, pattern="hex7", max_echoes=2)
    K, E = beam.subrays, beam.max_echoes
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def io_for(hits, n, tile):
        rows = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        counts = torch.zeros((P,), dtype=torch.int64, device="cuda")
        io = LrcCompactIO()
        io.t, io.point3, io.sem, io.ins = (hits[k].data_ptr() for k in ("t", "point3", "sem", "ins"))
        if tile:
            io.tile_count = hits["tile_count"].data_ptr()
        io.out_xyzl, io.counts = rows.data_ptr(), counts.data_ptr()
        return io, rows, counts

    cols = ("t", "point3", "sem", "ins")
    hits_e = DeviceHits(P * N * E, "cuda", want=cols)
    weight_t = torch.zeros((P * N * E,), dtype=torch.uint8, device="cuda")
    io_e, rows_e, counts_e = io_for(hits_e, P * N * E, False)
    off_t = torch.from_numpy(np.array(beam.offsets)).cuda()

    def echo():
        scene.scan_echoes_dev(poses_t, dirs_t, hits_e, sensor.max_range, beam, weight_t=weight_t, offsets_t=off_t, stream=stream)
        ctx.compact_dev(P, N * E, io_e, stream)
        return counts_e

    run = {"echo": echo}
    names = ["echo"]
    if not a.echo_only:
        rows = subray_rows(dirs, beam.offsets)                                          # (7, N, 3)
        lanes = np.concatenate([rows, rows[:1]]).transpose(1, 0, 2).reshape(8 * N, 3)   # row 8 i + k; lane 7 the axis again
        dirs8_t = torch.from_numpy(np.ascontiguousarray(lanes)).cuda()
        hits_8 = DeviceHits(P * N * 8, "cuda", want=cols + ("tile_count",))
        io_8, rows_8, counts_8 = io_for(hits_8, P * N * 8, True)
        sub_t = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rows]
        hits_k = [DeviceHits(P * N, "cuda", want=("t",)) for _ in range(K)]
        t_host = torch.empty((K, P * N), dtype=torch.float32).pin_memory()

        def clean8():
            scene.scan_poses_dev(poses_t, dirs8_t, hits_8, sensor.max_range, stream=stream)
            ctx.compact_dev(P, N * 8, io_8, stream)
            return counts_8

        def replaced():
            for k in range(K):
                scene.scan_poses_dev(poses_t, sub_t[k], hits_k[k], 1e30, stream=stream)     # raw distances: nothing filtered
                t_host[k].copy_(hits_k[k]["t"], non_blocking=True)
            torch.cuda.synchronize()
            return reduce_numpy(np.ascontiguousarray(t_host.numpy().T), E, beam.separation)
        run["clean8"] = clean8
        names = ["echo", "clean8"]

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        c = run[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, int(c.sum().item())
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
    out = {"workload": f"C3 {bench.SCENE} {sensor.vertical_res}x{sensor.horizontal_res} beams x {P} poses",
           "beams": P * N, "subrays": K, "max_echoes": E, "divergence_mrad": a.divergence_mrad, "separation_m": beam.separation,
           "steps": a.steps, "warmup": a.warmup}
    for k in names:
        e, w = np.array(ev[k]), np.array(wall[k])
        out[k] = {"events_median_ms": round(float(np.median(e)), 4), "events_min_ms": round(float(e.min()), 4),
                  "events_max_ms": round(float(e.max()), 4), "wall_median_ms": round(float(np.median(w)), 4),
                  "kept_rows": kept[k]}
    w = weight_t.cpu().numpy().reshape(-1, E)
    out["echo"]["beams_with_two_echoes"] = int((w[:, 1] > 0).sum())
    out["echo"]["beams_without_echo"] = int((w[:, 0] == 0).sum())
    if not a.echo_only:
        out["echo_over_clean8_events_median"] = round(out["echo"]["events_median_ms"] / out["clean8"]["events_median_ms"], 4)
        rw = []
        for _ in range(max(1, a.host_steps)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep, wt = replaced()
            rw.append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(wt, w))
        out["replaced"] = {"wall_median_ms": round(float(np.median(rw)), 2), "wall_min_ms": round(float(min(rw)), 2),
                           "rounds": len(rw), "weights_equal_the_kernels": same}
        out["replaced_over_echo_wall_median"] = round(out["replaced"]["wall_median_ms"] / out["echo"]["wall_median_ms"], 1)
    print(json.dumps(out, indent=1))
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
