#!/usr/bin/env python3
"""Timings of the seeded sensor noise under movers: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x
64 poses, bench.c3_poses) on synth_A6_office2 with M pedestrians walking the room (the walks of tools/movers_time.py), under
the sensor record's own noise model (range_noise_std, angle_noise_std, dropout_probability of bench.c3_sensor).

HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and minimum:
    scan_poses        lrc_scan_poses_dev: the clean scan
    scan_noisy        lrc_scan_noisy_dev: the noise increment of the plain scan in the same session, the yardstick
    movers_M          lrc_scan_movers_dev with M = 1, 4 pedestrians (--movers)
    noisy_movers_M    lrc_scan_noisy_movers_dev with the same sets, poses and the model
Derived, from the medians: per M the increment of the noise under movers in milliseconds and as a ratio, and that increment
over the plain scan's (the yardstick: where it is more than twice the plain scan's, DESIGN.md section 5r says where it goes).
Each noisy configuration also reports its returns and the share of them that movers win.

    python tools/mover_noise_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/mover_noise_c3.txt holds this report.
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
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, synth
    from lidarcast.movers import MoverSet
    from lidarcast.noise import NoiseModel
    from movers_time import walks
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    size = synth.scene_size(a.scene)
    sensor = bench.c3_sensor()
    model = NoiseModel.from_intrinsics(sensor, a.seed)
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    counts = [int(m) for m in a.movers.split(",") if m]
    sets, mposes = {}, {}
    for M in counts:
        sets[M] = MoverSet(ctx, [synth.make_pedestrian(instance=1000 + m) for m in range(M)])
        mposes[M] = torch.from_numpy(walks(M, size, P)).cuda()

    reach = sensor.max_range
    run = {"scan_poses": lambda: scene.scan_poses_dev(poses_t, dirs_t, hits, reach, stream=stream),
           "scan_noisy": lambda: scene.scan_noisy_dev(poses_t, dirs_t, hits, reach, model, stream=stream)}
    for M in counts:
        run[f"movers_{M}"] = (lambda m: lambda: scene.scan_movers_dev(poses_t, dirs_t, hits, reach, sets[m], mposes[m], mover_t=who,
                                                                      stream=stream))(M)
        run[f"noisy_movers_{M}"] = (lambda m: lambda: scene.scan_noisy_movers_dev(poses_t, dirs_t, hits, reach, sets[m], mposes[m], model,
                                                                                  mover_t=who, stream=stream))(M)

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
    res = {"workload": f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses", "rays": P * N,
           "triangles": int(len(mesh.triangles)), "mover_triangles": 288,
           "model": {"seed": a.seed, "range_std": model.range_std, "angle_std_deg": float(np.degrees(model.angle_std)),
                     "dropout": model.dropout}}
    res.update({n: _stats(v) for n, v in ms.items()})
    for M in counts:                    # who wins what under the noise
        n = f"noisy_movers_{M}"
        run[n]()
        torch.cuda.synchronize()
        t = hits["t"].cpu().numpy()
        w = who.cpu().numpy()
        res[n]["returns"] = int((t < np.inf).sum())
        res[n]["mover_returns_share"] = round(float((w > 0).sum()) / max(1, int((t < np.inf).sum())), 5)
    plain = res["scan_noisy"]["median_ms"] - res["scan_poses"]["median_ms"]
    res["noise_increment_plain_ms"] = round(plain, 4)
    res["noise_increment_plain_ratio"] = round(res["scan_noisy"]["median_ms"] / res["scan_poses"]["median_ms"], 4)
    for M in counts:
        inc = res[f"noisy_movers_{M}"]["median_ms"] - res[f"movers_{M}"]["median_ms"]
        res[f"noise_increment_movers_{M}_ms"] = round(inc, 4)
        res[f"noise_increment_movers_{M}_ratio"] = round(res[f"noisy_movers_{M}"]["median_ms"] / res[f"movers_{M}"]["median_ms"], 4)
        res[f"noise_increment_movers_{M}_over_plain"] = round(inc / plain, 3) if plain else None
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/mover_noise_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    for s in sets.values():
        s.close()
    scene.close()


if __name__ == "__main__":
    main()
