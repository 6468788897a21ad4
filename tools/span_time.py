#!/usr/bin/env python3
"""Timings of the animated movers under sweeps, one box, one session: the C3 trajectory (bench.c3_sensor,
32 x 2048 rays x 64 poses, bench.c3_poses) on synth_A6_office2, swept at --speed m/s, with M walkers (synth.make_walker, 384
triangles, --movers) that walk on AND swing their limbs while a sweep is scanned.

1. The span against two sets.  HIP events around --calls calls of lrc_deform_span_dev (two blends, the slot refit of A, the span
   slots, the node refit from the span boxes; the shapes change with every call), against the same number of PAIRS of
   lrc_deform_set_dev calls (two blends and two whole refits): what the two end shapes of a sweep cost either way.  The launch
   counts are reported with each.
2. The scan step.  lrc_scan_mover_sweeps_dev with the M walkers spanned (the per-ray-shape cast, span_trace_kernel) against the
   same call with each walker frozen at the sweep's start shape (lrc_deform_set_dev: the explicit-ray launch of the trace
   kernel on the refitted tree), HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and
   minimum.  Also with one walker 0.8 m beside every pose (the mover fills a large part of the view: few rays are culled).  Each
   configuration reports the share of the returns that movers win.

    python tools/span_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/span_c3.txt holds this report.
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
    ap.add_argument("--calls", type=int, default=200)
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
    from lidarcast import DeviceHits, deform, motion_records, synth
    from lidarcast.movers import MoverSet, scan_mover_sweeps_dev, sweep_records
    from mover_sweeps_time import walk_tracks
    ctx = lidarcast.Context(0)
    walker = synth.make_walker()
    K = len(walker.keyframes)
    stream = torch.cuda.current_stream().cuda_stream
    res = {}

    # ---- 1: one span against two sets -----------------------------------------------------------------------------------------
    d = deform.Deformable(ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)

    def span(i):
        d.span((i % K, (i + 1) % K, 0.25), ((i + 1) % K, (i + 2) % K, 0.25 + 0.5 * (i % 2)), stream=stream)

    def two_sets(i):
        d.set(i % K, (i + 1) % K, 0.25, stream=stream)
        d.set((i + 1) % K, (i + 2) % K, 0.25 + 0.5 * (i % 2), stream=stream)
    shape = {}
    for label, call in (("span", span), ("two_sets", two_sets)):
        for i in range(20):
            call(i)
        torch.cuda.synchronize()
        per_call = []
        for _ in range(5):                              # five blocks of --calls calls each
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.calls):
                call(i)
            e1.record()
            e1.synchronize()
            per_call.append(e0.elapsed_time(e1) / a.calls)
        shape[label] = _stats(per_call)
    shape["span"]["launches"] = d.span_launches()[0]
    shape["two_sets"]["launches"] = 2 * d.launches()[0]
    shape["span_over_two_sets"] = round(shape["span"]["median_ms"] / shape["two_sets"]["median_ms"], 3)
    shape["vertices"], shape["triangles"], shape["nodes"] = int(walker.keyframes.shape[1]), int(len(walker.triangles)), int(d.scene.info["num_nodes"])
    shape["device_bytes"] = int(d.scene.info["device_bytes"])
    d.close()
    res["shapes_of_a_sweep"] = shape

    # ---- 2: the scan step, spanned against frozen -------------------------------------------------------------------------------
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
    dirs_t = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    fire_t = torch.from_numpy(np.ascontiguousarray(fire, dtype=np.float64)).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    reach = sensor.max_range
    times = np.arange(P) * 0.1
    configs = {}
    for M in [int(m) for m in a.movers.split(",") if m]:
        configs[f"walking_{M}"] = (M, sweep_records(walk_tracks(M, size, P), times, times + T))
    near = np.zeros((P, 1, 24), np.float32)                 # 0.8 m beside every pose, feet on the floor, walking 0.12 m per sweep
    for p in range(P):
        c = poses[p][:3, 3]
        near[p, 0, :12] = [1, 0, 0, c[0], 0, 1, 0, c[1] + 0.8, 0, 0, 1, 0.0]
        near[p, 0, 12], near[p, 0, 16] = 1.0, 0.12
    configs["in_view_1"] = (1, near)
    A, B = (1, 2, 0.25), (2, 3, 0.25)           # a sweep of 0.1 s in a clip of 0.8 s: one keyframe further
    scan = {}
    for name, (M, rec) in configs.items():
        ds = [deform.Deformable(ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins) for _ in range(M)]
        mset = MoverSet(ctx, ds)
        rec_t = torch.from_numpy(np.ascontiguousarray(rec)).cuda()

        def state(spanned):
            for x in ds:
                x.span(A, B, stream=stream) if spanned else x.set(*A, stream=stream)

        def timed():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            scan_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, reach, mset, rec_t, mover_t=who, stream=stream)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        ms = {"spanned": [], "frozen": []}
        for rnd in range(a.warmup + a.steps):               # interleaved: both states see the same clocks
            for label in ms:
                state(label == "spanned")
                t = timed()
                if rnd >= a.warmup:
                    ms[label].append(t)
        r = {n: _stats(v) for n, v in ms.items()}
        for label in ms:
            state(label == "spanned")
            timed()
            t, w = hits["t"].cpu().numpy(), who.cpu().numpy()
            r[label]["returns"] = int((t < np.inf).sum())
            r[label]["mover_returns_share"] = round(float((w > 0).sum()) / max(1, int((t < np.inf).sum())), 5)
        r["spanned_over_frozen"] = round(r["spanned"]["median_ms"] / r["frozen"]["median_ms"], 4)
        scan[name] = r
        mset.close()
        for x in ds:
            x.close()
    res["scan_step"] = dict(workload=f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} sweeps at {a.speed} m/s",
                            rays=P * N, triangles=int(len(mesh.triangles)), mover_triangles=int(len(walker.triangles)), **scan)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/span_time.py --calls {a.calls} --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    scene.close()


if __name__ == "__main__":
    main()
