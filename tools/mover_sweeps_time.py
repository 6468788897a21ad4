#!/usr/bin/env python3
"""Timings of the movers under moving-sensor sweeps: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x
64 poses, bench.c3_poses) on synth_A6_office2, swept at --speed m/s, with M pedestrians that walk on while a sweep is scanned.

HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and minimum:
    scan_sweeps          lrc_scan_sweeps_dev: the sweep scan without movers, a yardstick of the same session
    mover_sweeps_null    lrc_scan_mover_sweeps_dev with a NULL set (the same launch plus the zeroed mover column)
    scan_movers_M        lrc_scan_movers_dev with M = 1, 4 pedestrians (--movers) frozen at their pose of the sweep's start, the
                         sensor frozen at its own: the other yardstick
    mover_sweeps_M       lrc_scan_mover_sweeps_dev with the same M pedestrians, each moving through the sweep
    mover_sweeps_M_still the same call with still records: the branch that takes the frozen arithmetic
Derived, from the medians: mover_sweeps_M over scan_movers_M and over scan_sweeps.  Each mover configuration also reports the
share of the returns that movers win.

    python tools/mover_sweeps_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/mover_sweeps_c3.txt holds this report.
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


def walk_tracks(M, size, P, seed=11):
    """M seeded walks through a room of ``size`` at about 1.2 m/s, turning 30 degrees per second: tools/movers_time.py's walks
    as tracks, so that they can be evaluated at both ends of a sweep"""
    from lidarcast.movers import MoverTrack
    rng = np.random.default_rng(seed)
    end = (P - 1) * 0.1 + 0.1
    out = []
    for _ in range(M):
        a = rng.uniform((0.5, 0.5), (size[0] - 0.5, size[1] - 0.5))
        heading = rng.uniform(0.0, 2.0 * np.pi)
        b = np.clip(a + 1.2 * end * np.array([np.cos(heading), np.sin(heading)]), 0.4, (size[0] - 0.4, size[1] - 0.4))
        yaw = np.degrees(heading)
        out.append(MoverTrack([[0.0, a[0], a[1], 0.0, yaw], [end, b[0], b[1], 0.0, yaw + 30.0 * end]]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="synth_A6_office2")
    ap.add_argument("--movers", default="1,4")
    ap.add_argument("--speed", type=float, default=0.5, help="sensor speed along the trajectory, m/s")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, motion_records, synth
    from lidarcast.movers import MoverSet, scan_mover_sweeps_dev, sweep_records
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    size = synth.scene_size(a.scene)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    lid = IndoorLidar(sensor, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    T = 1.0 / float(sensor.scan_frequency)
    ends = poses.copy()                       # every sweep moves speed * T along the step to the next pose
    step = np.diff(poses[:, :3, 3], axis=0, append=poses[-1:, :3, 3] + (poses[-1:, :3, 3] - poses[-2:-1, :3, 3]))
    norm = np.linalg.norm(step, axis=1, keepdims=True)
    ends[:, :3, 3] += a.speed * T * step / np.where(norm > 0, norm, 1.0)
    motion_t = torch.from_numpy(motion_records(poses, ends)).cuda()
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    fire_t = torch.from_numpy(np.ascontiguousarray(fire, dtype=np.float64)).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    reach = sensor.max_range
    counts = [int(m) for m in a.movers.split(",") if m]
    times = np.arange(P) * 0.1
    sets, frozen, moving, still = {}, {}, {}, {}
    for M in counts:
        tracks = walk_tracks(M, size, P)
        sets[M] = MoverSet(ctx, [synth.make_pedestrian(instance=1000 + m) for m in range(M)])
        rec = sweep_records(tracks, times, times + T)
        stood = np.zeros_like(rec)
        stood[:, :, :12], stood[:, :, 12] = rec[:, :, :12], 1.0
        frozen[M] = torch.from_numpy(np.ascontiguousarray(rec[:, :, :12])).cuda()
        moving[M] = torch.from_numpy(rec).cuda()
        still[M] = torch.from_numpy(stood).cuda()

    run = {"scan_sweeps": lambda: scene.scan_sweeps_dev(motion_t, dirs_t, fire_t, hits, reach, stream=stream),
           "mover_sweeps_null": lambda: scan_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach, None, None, mover_t=who,
                                                              stream=stream)}
    for M in counts:
        run[f"scan_movers_{M}"] = (lambda m: lambda: scene.scan_movers_dev(poses_t, dirs_t, hits, reach, sets[m], frozen[m], mover_t=who,
                                                                           stream=stream))(M)
        run[f"mover_sweeps_{M}"] = (lambda m: lambda: scan_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach, sets[m],
                                                                            moving[m], mover_t=who, stream=stream))(M)
        run[f"mover_sweeps_{M}_still"] = (lambda m: lambda: scan_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach, sets[m],
                                                                                  still[m], mover_t=who, stream=stream))(M)

    def timed(n):
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
    for _ in range(a.steps):            # interleaved: every configuration sees the same clocks
        for n in names:
            ms[n].append(timed(n))
    res = {"workload": f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} sweeps at {a.speed} m/s", "rays": P * N,
           "triangles": int(len(mesh.triangles)), "mover_triangles": 288}
    res.update({n: _stats(v) for n, v in ms.items()})
    for n in names:                     # who wins what
        if "null" in n or n == "scan_sweeps":
            continue
        run[n]()
        torch.cuda.synchronize()
        t = hits["t"].cpu().numpy()
        w = who.cpu().numpy()
        res[n]["returns"] = int((t < np.inf).sum())
        res[n]["mover_returns_share"] = round(float((w > 0).sum()) / max(1, int((t < np.inf).sum())), 5)
    for M in counts:
        mine = res[f"mover_sweeps_{M}"]["median_ms"]
        res[f"mover_sweeps_{M}_over_scan_movers_{M}"] = round(mine / res[f"scan_movers_{M}"]["median_ms"], 3)
        res[f"mover_sweeps_{M}_over_scan_sweeps"] = round(mine / res["scan_sweeps"]["median_ms"], 3)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/mover_sweeps_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    for s in sets.values():
        s.close()
    scene.close()


if __name__ == "__main__":
    main()
