#!/usr/bin/env python3
"""Deforming-mover timings, one box, one session.  Two meshes: the walker of synth.make_walker (384
triangles) and the same walker subdivided three times (24 576 triangles, every keyframe subdivided alike).

1. Refit against rebuild.  HIP events around --calls calls of lrc_deform_set_dev (a blend and the refit; the shape changes
   with every call), once with the single-workgroup tail and once on a deformable created under LRC_DEFORM_TAIL=0 (one launch
   per height to the top), against lrc_scene_create_dev of the same vertices and triangles resident in HBM (wall clock around
   the synchronous call, --builds builds, median): what a mover that changes shape costs without this feature.  The launch
   count per refit is reported with each.
2. Refitted tree against fresh tree.  The C3 mover scan step (bench.c3_sensor, 32 x 2048 rays x 64 poses on synth_A6_office2,
   one walker walking the room, lrc_scan_movers_dev) with the walker at its extreme keyframe on the refitted tree, against the
   same scan with a fresh scene of those vertices: the refit keeps keyframe 0's splits, so this ratio is what the feature costs
   while it runs.  The fresh scene twice: as lrc_scene_create makes it (quantised node images where the grid allows), and under
   LRC_QNODES=0 (float32 nodes, the refitted tree's own route), which isolates the splits.  Also with the walker 0.8 m beside every pose (the mover fills a large part of the view).

    python tools/deform_time.py [--calls 200] [--builds 20] [--steps 20] [--out report.txt]
profiles/deform_c3.txt holds this report.
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


def subdivide(keys, tris, times):
    """Every triangle into four by its edge midpoints, ``times`` times, in every keyframe alike (float64 midpoints of the
    float32 keyframes, narrowed)."""
    keys = keys.astype(np.float64)
    for _ in range(times):
        V = keys.shape[1]
        e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], 0), 1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.reshape(3, len(tris)).T + V                      # midpoint vertex of edge 01, 12, 20 per triangle
        keys = np.concatenate([keys, 0.5 * (keys[:, uniq[:, 0]] + keys[:, uniq[:, 1]])], 1)
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = inv[:, 0], inv[:, 1], inv[:, 2]
        tris = np.concatenate([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1),
                               np.stack([ab, bc, ca], 1)], 0).astype(np.int32)
    return keys.astype(np.float32), tris


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--builds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="synth_A6_office2")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, deform, synth
    from lidarcast.movers import MoverSet
    from movers_time import walks
    ctx = lidarcast.Context(0)
    walker = synth.make_walker()
    big_keys, big_tris = subdivide(walker.keyframes, np.asarray(walker.triangles, np.int32), 3)
    meshes = {"walker": (walker.keyframes, np.asarray(walker.triangles, np.int32)), "walker_x64": (big_keys, big_tris)}
    stream = torch.cuda.current_stream().cuda_stream
    res = {}

    # ---- 1: refit against rebuild ------------------------------------------------------------------------------------------
    for name, (keys, tris) in meshes.items():
        K = len(keys)
        sem = np.full(len(tris), 13, np.uint16)
        out = {"vertices": int(keys.shape[1]), "triangles": int(len(tris))}
        for label, env in (("refit_tail", "1"), ("refit_levels", "0")):
            os.environ["LRC_DEFORM_TAIL"] = env            # read at creation
            d = deform.Deformable(ctx, keys, tris, sem, sem)
            os.environ.pop("LRC_DEFORM_TAIL")
            for i in range(20):
                d.set(i % K, (i + 1) % K, 0.3, stream=stream)
            torch.cuda.synchronize()
            per_call = []
            for _ in range(5):                              # five blocks of --calls calls each
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.calls):
                    d.set(i % K, (i + 1) % K, 0.25 + 0.5 * (i % 2), stream=stream)
                e1.record()
                e1.synchronize()
                per_call.append(e0.elapsed_time(e1) / a.calls)
            out[label] = dict(_stats(per_call), launches_per_set=d.launches()[0], nodes=int(d.scene.info["num_nodes"]))
            if label == "refit_tail":
                d.set(2, 2, 0.0, stream=stream)
                verts_t = torch.from_numpy(d.vertices()).cuda()
            d.close()
        tris_t = torch.from_numpy(tris).cuda()
        sem_t = torch.from_numpy(sem.view(np.int16)).cuda()
        builds = []
        for i in range(a.builds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc = lidarcast.Scene.from_device(ctx, verts_t, tris_t, sem_t, sem_t)
            t1 = time.perf_counter()
            if i >= 2:
                builds.append((t1 - t0) * 1e3)
            info = sc.info
            sc.close()
        out["rebuild_create_dev"] = dict(_stats(builds), device_build=int(info["device_build"]), nodes=int(info["num_nodes"]))
        out["rebuild_over_refit"] = round(out["rebuild_create_dev"]["median_ms"] / out["refit_tail"]["median_ms"], 1)
        out["tail_over_levels"] = round(out["refit_tail"]["median_ms"] / out["refit_levels"]["median_ms"], 3)
        res[name] = out

    # ---- 2: the scan on the refitted tree against a fresh tree -----------------------------------------------------------------
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
    near = np.zeros((P, 1, 12), np.float32)                 # 0.8 m beside every pose, feet on the floor
    for p in range(P):
        c = poses[p][:3, 3]
        near[p, 0] = [1, 0, 0, c[0], 0, 1, 0, c[1] + 0.8, 0, 0, 1, 0.0]
    placements = {"walking": torch.from_numpy(walks(1, size, P)).cuda(), "in_view": torch.from_numpy(near).cuda()}
    scan = {}
    for name, (keys, tris) in meshes.items():
        sem = np.full(len(tris), 13, np.uint16)
        d = deform.Deformable(ctx, keys, tris, sem, sem)
        d.set(2, 2, 0.0)                                    # the extreme keyframe, on the tree of keyframe 0
        verts = d.vertices()
        rigid = synth.TriangleMesh(vertices=verts.astype(np.float64), triangles=tris, triangle_sem=sem, triangle_ins=sem)
        sets = {"refitted": MoverSet(ctx, [d]), "fresh": MoverSet(ctx, [rigid])}        # fresh: the node route LRC_QNODES picks
        os.environ["LRC_QNODES"] = "0"                      # read at creation: a fresh tree on the refitted tree's own node route
        sets["fresh_float32"] = MoverSet(ctx, [rigid])
        os.environ.pop("LRC_QNODES")
        fresh_q = int(sets["fresh"].scenes[0].info["quantised_nodes"])
        for place, mp_t in placements.items():
            run = {k: (lambda s: lambda: scene.scan_movers_dev(poses_t, dirs_t, hits, sensor.max_range, s, mp_t, mover_t=who,
                                                                stream=stream))(s) for k, s in sets.items()}

            def timed(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run[n]()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            for _ in range(a.warmup):
                for n in run:
                    timed(n)
            ms = {n: [] for n in run}
            for _ in range(a.steps):                        # interleaved: both trees see the same clocks
                for n in run:
                    ms[n].append(timed(n))
            r = {n: _stats(v) for n, v in ms.items()}
            run["refitted"]()
            torch.cuda.synchronize()
            r["mover_share_of_returns"] = round(float((who > 0).sum().item()) / max(1, int((hits["t"] < float("inf")).sum().item())), 5)
            r["refitted_over_fresh"] = round(r["refitted"]["median_ms"] / r["fresh"]["median_ms"], 4)
            r["refitted_over_fresh_float32"] = round(r["refitted"]["median_ms"] / r["fresh_float32"]["median_ms"], 4)
            r["fresh_has_quantised_nodes"] = fresh_q
            scan[f"{name}/{place}"] = r
        for ms_ in sets.values():
            ms_.close()
        d.close()
    res["scan_step"] = dict(workload=f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses, one mover at its extreme keyframe",
                            rays=P * N, **scan)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
