#!/usr/bin/env python3
"""Scene-flow timings: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x 64 poses, bench.c3_poses) on
synth_A6_office2 with M pedestrians walking the room (the walks of tools/movers_time.py); frame k flows to frame k + 1.

HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and minimum, per M = 1, 4, 16:
    movers_M         lrc_scan_movers_dev: the mover scan, the yardstick of the same session
    flow_only_M      lrc_scan_flow_dev without a status column on that scan's records: one elementwise pass, nothing cast
    flow_status_M    lrc_scan_flow_dev with the status: the ray kernel, the cast on the room, per mover a ray kernel, a cast and a merge
    movers_compact_M lrc_scan_movers_compact: the mover scan to frames on the host (host clock: the call synchronises)
    flow_compact_M   lrc_scan_flow_compact: the same with the flow and status columns
Derived, from the medians: flow_only / movers, flow_status / movers, and (flow_compact - movers_compact) / movers -- what the two
extra columns cost on the way to frames, in mover scans.  Each M also reports the status counts of the kept rows.

    python tools/flow_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/flow_c3.txt holds this report.
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
    ap.add_argument("--movers", default="1,4,16")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, DirectionTable, flow, synth
    from lidarcast.movers import MoverSet
    from movers_time import walks
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    size = synth.scene_size(a.scene)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    table = DirectionTable(ctx, dirs)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    flow_t = torch.zeros((P * N, 3), dtype=torch.float32, device="cuda")
    status_t = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    counts = [int(m) for m in a.movers.split(",") if m]
    run, host, sets = {}, {}, {}
    for M in counts:
        mset = sets[M] = MoverSet(ctx, [synth.make_pedestrian(instance=1000 + m) for m in range(M)])
        mp = walks(M, size, P)
        nxt, nmp, has = flow.pair_next(poses, mp)
        mt, nmt = torch.from_numpy(mp).cuda(), torch.from_numpy(nmp).cuda()
        nt, ht = torch.from_numpy(nxt.reshape(P, 16).copy()).cuda(), torch.from_numpy(has).cuda()

        def scan(mset=mset, mt=mt):
            scene.scan_movers_dev(poses_t, dirs_t, hits, sensor.max_range, mset, mt, mover_t=who, stream=stream)

        def flow_dev(status, mset=mset, mt=mt, nmt=nmt, nt=nt, ht=ht):
            scene.scan_flow_dev(hits, who, P, N, sensor.max_range, mset, mt, nmt, nt, flow_t, status_t=status, has_next_t=ht,
                                stream=stream)
        run[f"movers_{M}"] = scan                       # leaves the records the two flow calls behind it read
        run[f"flow_only_{M}"] = lambda f=flow_dev: f(None)
        run[f"flow_status_{M}"] = lambda f=flow_dev: f(status_t)
        host[f"movers_compact_{M}"] = lambda mset=mset, mp=mp: scene.scan_movers_compact(poses, table, sensor.max_range, mset, mp)
        host[f"flow_compact_{M}"] = lambda mset=mset, mp=mp, nxt=nxt, nmp=nmp, has=has: scene.scan_flow_compact(
            poses, table, sensor.max_range, mset, mp, nxt, nmp, has)

    def timed(n):
        if n in host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host[n]()
            return (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run[n]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    names = list(run) + list(host)
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
    for M in counts:
        run[f"movers_{M}"]()
        run[f"flow_status_{M}"]()
        torch.cuda.synchronize()
        kept = hits["t"].cpu().numpy() < np.inf
        base = res[f"movers_{M}"]["median_ms"]
        res[f"M_{M}"] = {"status_counts_none_visible_occluded_out_of_range": np.bincount(status_t.cpu().numpy()[kept], minlength=4).tolist(),
                         "moved_rows": int((flow_t.cpu().numpy()[kept] != 0).any(axis=1).sum()),
                         "flow_only_over_movers": round(res[f"flow_only_{M}"]["median_ms"] / base, 4),
                         "flow_status_over_movers": round(res[f"flow_status_{M}"]["median_ms"] / base, 4),
                         "compact_extra_over_movers": round((res[f"flow_compact_{M}"]["median_ms"] -
                                                             res[f"movers_compact_{M}"]["median_ms"]) / base, 4)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/flow_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms; *_compact: host clock)\n{text}\n")
    for s in sets.values():
        s.close()
    scene.close()


if __name__ == "__main__":
    main()
