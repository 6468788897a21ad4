#!/usr/bin/env python3
"""Timings of the seeded sensor noise under movers in sweeps: the C3 trajectory (bench.c3_sensor, 32 x 2048
rays x 64 sweeps, bench.c3_poses) on synth_A6_office2, swept at --speed m/s, with M pedestrians that walk on while a sweep is
scanned (the walks of tools/movers_time.py as tracks: tools/mover_sweeps_time.py walk_tracks), under the sensor record's own noise
model (range_noise_std, angle_noise_std, dropout_probability of bench.c3_sensor).

HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and minimum:
    scan_sweeps              lrc_scan_sweeps_dev: the clean sweep scan
    scan_noisy_sweeps        lrc_scan_noisy_sweeps_dev: the noise increment of the plain sweep scan in the same session, the yardstick
    mover_sweeps_M           lrc_scan_mover_sweeps_dev with M = 1, 4 pedestrians (--movers)
    noisy_mover_sweeps_M     lrc_scan_noisy_mover_sweeps_dev with the same sets, records and the model
    mover_sweeps_walker      lrc_scan_mover_sweeps_dev with one spanned walker (a per-ray shape) that walks 0.8 m
                             beside every pose, in view
    noisy_mover_sweeps_walker  lrc_scan_noisy_mover_sweeps_dev with the same walker, span and the model
Derived, from the medians: per configuration the increment of the noise in milliseconds and as a ratio, and that increment over
the plain sweep scan's.  Each noisy configuration also reports its returns and the share of them that movers win.

    python tools/mover_sweep_noise_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/mover_sweep_noise_c3.txt holds this report.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "indoor-point-cloud-datasets-controllable-generation-method-for-mobile-"
                                      "robots-3d-scene-perception_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402


def _stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="synth_A6_office2")
    ap.add_argument("--movers", default="1,4")
    ap.add_argument("--speed", type=float, default=0.5, help="sensor speed along the trajectory, m/s")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, deform, motion_records, synth
    from lidarcast.movers import MoverSet, scan_mover_sweeps_dev, scan_noisy_mover_sweeps_dev, sweep_records
    from lidarcast.noise import NoiseModel, scan_noisy_sweeps_dev
    from mover_sweeps_time import walk_tracks
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    size = synth.scene_size(a.scene)
    sensor = bench.c3_sensor()
    model = NoiseModel.from_intrinsics(sensor, a.seed)
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
    dirs_t = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    fire_t = torch.from_numpy(np.ascontiguousarray(fire, dtype=np.float64)).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    reach = sensor.max_range
    times = np.arange(P) * 0.1
    sets, records = {}, {}
    for M in [int(m) for m in a.movers.split(",") if m]:
        sets[str(M)] = MoverSet(ctx, [synth.make_pedestrian(instance=1000 + m) for m in range(M)])
        records[str(M)] = torch.from_numpy(sweep_records(walk_tracks(M, size, P), times, times + T)).cuda()
    # one spanned walker 0.8 m beside every pose, feet on the floor, walking 0.12 m per sweep (tools/span_time.py's in_view_1); a
    # sweep of 0.1 s in a clip of 0.8 s: one keyframe further
    walker = synth.make_walker()
    d = deform.Deformable(ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
    near = np.zeros((P, 1, 24), np.float32)
    for p in range(P):
        c = poses[p][:3, 3]
        near[p, 0, :12] = [1, 0, 0, c[0], 0, 1, 0, c[1] + 0.8, 0, 0, 1, 0.0]
        near[p, 0, 12], near[p, 0, 16] = 1.0, 0.12
    sets["walker"] = MoverSet(ctx, [d])
    records["walker"] = torch.from_numpy(near).cuda()
    d.span((1, 2, 0.25), (2, 3, 0.25), stream=stream)
    torch.cuda.synchronize()

    run = {"scan_sweeps": lambda: scene.scan_sweeps_dev(motion_t, dirs_t, fire_t, hits, reach, stream=stream),
           "scan_noisy_sweeps": lambda: scan_noisy_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach, model, stream=stream)}
    for key in sets:
        run[f"mover_sweeps_{key}"] = (lambda m: lambda: scan_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach, sets[m],
                                                                              records[m], mover_t=who, stream=stream))(key)
        run[f"noisy_mover_sweeps_{key}"] = (lambda m: lambda: scan_noisy_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach,
                                                                                          sets[m], records[m], model, mover_t=who,
                                                                                          stream=stream))(key)

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
           "triangles": int(len(mesh.triangles)), "pedestrian_triangles": 288, "walker_triangles": int(len(walker.triangles)),
           "model": {"seed": a.seed, "range_std": model.range_std, "angle_std_deg": float(np.degrees(model.angle_std)),
                     "dropout": model.dropout}}
    res.update({n: _stats(v) for n, v in ms.items()})
    for key in sets:                    # who wins what, clean and under the noise
        for n in (f"mover_sweeps_{key}", f"noisy_mover_sweeps_{key}"):
            run[n]()
            torch.cuda.synchronize()
            t = hits["t"].cpu().numpy()
            w = who.cpu().numpy()
            res[n]["returns"] = int((t < np.inf).sum())
            res[n]["mover_returns_share"] = round(float((w > 0).sum()) / max(1, int((t < np.inf).sum())), 5)
    plain = res["scan_noisy_sweeps"]["median_ms"] - res["scan_sweeps"]["median_ms"]
    res["noise_increment_plain_ms"] = round(plain, 4)
    res["noise_increment_plain_ratio"] = round(res["scan_noisy_sweeps"]["median_ms"] / res["scan_sweeps"]["median_ms"], 4)
    for key in sets:
        clean, noisy = res[f"mover_sweeps_{key}"]["median_ms"], res[f"noisy_mover_sweeps_{key}"]["median_ms"]
        res[f"noise_increment_{key}_ms"] = round(noisy - clean, 4)
        res[f"noise_increment_{key}_ratio"] = round(noisy / clean, 4)
        res[f"noise_increment_{key}_over_plain"] = round((noisy - clean) / plain, 3) if plain else None
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/mover_sweep_noise_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    for s in sets.values():
        s.close()
    d.close()
    scene.close()


if __name__ == "__main__":
    main()
