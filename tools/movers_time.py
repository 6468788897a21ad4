#!/usr/bin/env python3
"""Moving-object scan timings: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x 64 poses,
bench.c3_poses) on synth_A6_office2 with M pedestrians walking the room.

HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and minimum:
    scan_poses        lrc_scan_poses_dev: the clean scan, the yardstick of the same session
    movers_null       lrc_scan_movers_dev with a NULL set (the same launch plus the zeroed mover column)
    movers_M          lrc_scan_movers_dev with M = 1, 4, 16 pedestrians (--movers) on seeded walks through the room
    movers_1_unseen   one pedestrian 1000 m away: every ray is culled, nothing is traversed -- what a mover costs before any
                      traversal: the ray kernel, the keep bytes, the explicit-ray launch whose waves find nothing to do, the
                      merge kernel
Derived, from the medians: the cost per mover as the slope between the smallest and the largest M; the fixed cost of
going through explicit rays and a merge at all (the smallest M's time minus its movers' slope minus scan_poses); the cost of a
mover no ray can meet (movers_1_unseen minus that fixed cost minus scan_poses) and its share of the slope: what part of a
mover's cost is ray set-up, mask traffic, empty waves and the merge rather than traversal.  Each configuration also reports the
share of the returns that movers win.

    python tools/movers_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/movers_c3.txt holds this report.
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


def walks(M, size, P, seed=11):
    """(P, M, 12) float32: M seeded walks through a room of ``size``, one pose per frame, 0.1 s apart at about 1.2 m/s"""
    from lidarcast.movers import MoverTrack
    rng = np.random.default_rng(seed)
    times = np.arange(P) * 0.1
    out = np.empty((P, M, 12), np.float32)
    for m in range(M):
        a = rng.uniform((0.5, 0.5), (size[0] - 0.5, size[1] - 0.5))
        heading = rng.uniform(0.0, 2.0 * np.pi)
        b = np.clip(a + 1.2 * times[-1] * np.array([np.cos(heading), np.sin(heading)]), 0.4, (size[0] - 0.4, size[1] - 0.4))
        yaw = np.degrees(heading)
        out[:, m] = MoverTrack([[0.0, a[0], a[1], 0.0, yaw], [times[-1], b[0], b[1], 0.0, yaw]]).poses12(times)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="synth_A6_office2")
    ap.add_argument("--movers", default="1,4,16")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, synth
    from lidarcast.movers import MoverSet
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    size = synth.scene_size(a.scene)
    sensor = bench.c3_sensor()
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
        sets[f"movers_{M}"] = MoverSet(ctx, [synth.make_pedestrian(instance=1000 + m) for m in range(M)])
        mposes[f"movers_{M}"] = torch.from_numpy(walks(M, size, P)).cuda()
    sets["movers_1_unseen"] = MoverSet(ctx, [synth.make_pedestrian()])
    far = walks(1, size, P)
    far[:, :, 3] += 1000.0
    mposes["movers_1_unseen"] = torch.from_numpy(far).cuda()

    run = {"scan_poses": lambda: scene.scan_poses_dev(poses_t, dirs_t, hits, sensor.max_range, stream=stream),
           "movers_null": lambda: scene.scan_movers_dev(poses_t, dirs_t, hits, sensor.max_range, None, None, mover_t=who, stream=stream)}
    for name in sets:
        run[name] = (lambda n: lambda: scene.scan_movers_dev(poses_t, dirs_t, hits, sensor.max_range, sets[n], mposes[n], mover_t=who,
                                                             stream=stream))(name)

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
           "triangles": int(len(mesh.triangles)), "mover_triangles": 288}
    res.update({n: _stats(v) for n, v in ms.items()})
    for n in sets:                      # who wins what
        run[n]()
        torch.cuda.synchronize()
        t = hits["t"].cpu().numpy()
        w = who.cpu().numpy()
        res[n]["returns"] = int((t < np.inf).sum())
        res[n]["mover_returns_share"] = round(float((w > 0).sum()) / max(1, int((t < np.inf).sum())), 5)
    base = res["scan_poses"]["median_ms"]
    lo, hi = min(counts), max(counts)
    if hi > lo:
        slope = (res[f"movers_{hi}"]["median_ms"] - res[f"movers_{lo}"]["median_ms"]) / (hi - lo)
        fixed = res[f"movers_{lo}"]["median_ms"] - lo * slope - base
        unseen = res["movers_1_unseen"]["median_ms"] - fixed - base
        res["per_mover_ms"] = round(slope, 4)
        res["per_mover_over_scan"] = round(slope / base, 3)
        res["explicit_static_pass_extra_ms"] = round(fixed, 4)
        res["unseen_mover_ms"] = round(unseen, 4)
        res["overhead_share_of_a_mover"] = round(unseen / slope, 3)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/movers_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    for s in sets.values():
        s.close()
    scene.close()


if __name__ == "__main__":
    main()
