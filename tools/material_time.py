#!/usr/bin/env python3
"""Surface materials on C3 (bench.SCENE, 32 x 2048 rays x 64 poses): what the continuation loop costs.  Four steps over the
SAME rays, each a scan plus lrc_compact_dev over the same record columns (t, point3, sem, ins, tile_count):

  clean      lrc_scan_poses_dev                                              trace_kernel<1, ...>
  diffuse    lrc_scan_materials_dev with an all-diffuse table (albedo 1): the clean scan's bytes, no lane ever goes on -- what
             differs from `clean` is the kernel's larger register footprint (fewer waves per SIMD), the class record fetched per
             ray and the original ray formed a second time                   trace_kernel<7, ...>
  diffuse+   the same with intensity, bounces and surface points written too: every lane forms the normal, the unit direction
             and the hit point that those columns read (a lane on a diffuse surface skips them when no output asks)
  materials  lrc_scan_materials_dev with a window / board table (--classes), intensity, bounces and surface points written too

--warmup rounds first, then --steps rounds that rotate the order of the steps, timed with HIP events.  The share of rays per
bounce count is reported for `materials`.

    python tools/material_time.py --steps 20 --warmup 3
    python tools/material_time.py --only materials --steps 5      # one step alone (for rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-bounces", type=int, default=4)
    ap.add_argument("--retro-deg", type=float, default=3.0)
    ap.add_argument("--glass", default="window", help="comma-separated classes that are glass")
    ap.add_argument("--mirror", default="board", help="comma-separated classes that are mirrors")
    ap.add_argument("--only", choices=("clean", "diffuse", "diffuse+", "materials"))
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, synth
    from lidarcast._capi import LrcCompactIO
    from lidarcast.material import MaterialTable
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    classes = {c: {"kind": "glass", "pass": 0.9, "albedo": 0.1, "retro_deg": a.retro_deg} for c in a.glass.split(",") if c}
    classes.update({c: {"kind": "mirror", "pass": 0.95, "albedo": 0.05, "retro_deg": a.retro_deg} for c in a.mirror.split(",") if c})
    table = MaterialTable.from_classes(classes, max_bounces=a.max_bounces)
    diffuse_table = MaterialTable.diffuse(table.num_classes, max_bounces=a.max_bounces)
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    cols = ("t", "point3", "sem", "ins", "tile_count")

    def io_for(hits):
        rows = torch.empty((P * N, 4), dtype=torch.float32, device="cuda")
        counts = torch.zeros((P,), dtype=torch.int64, device="cuda")
        io = LrcCompactIO()
        io.t, io.point3, io.sem, io.ins, io.tile_count = (hits[k].data_ptr() for k in cols)
        io.out_xyzl, io.counts = rows.data_ptr(), counts.data_ptr()
        return io, rows, counts

    hits = {k: DeviceHits(P * N, "cuda", want=cols + (("intensity",) if k in ("materials", "diffuse+") else ())) for k in ("clean", "diffuse", "diffuse+", "materials")}
    ios = {k: io_for(h) for k, h in hits.items()}
    bounces_t = torch.zeros((P * N,), dtype=torch.uint8, device="cuda")
    surface_t = torch.zeros((P * N, 3), dtype=torch.float32, device="cuda")
    bounces_d, surface_d = torch.zeros_like(bounces_t), torch.zeros_like(surface_t)      # diffuse+ writes its own

    def clean():
        scene.scan_poses_dev(poses_t, dirs_t, hits["clean"], sensor.max_range, stream=stream)

    def diffuse():
        scene.scan_materials_dev(poses_t, dirs_t, hits["diffuse"], sensor.max_range, diffuse_table, stream=stream)

    def diffuse_all():
        scene.scan_materials_dev(poses_t, dirs_t, hits["diffuse+"], sensor.max_range, diffuse_table, bounces_t=bounces_d,
                                 surface_t=surface_d, stream=stream)

    def materials():
        scene.scan_materials_dev(poses_t, dirs_t, hits["materials"], sensor.max_range, table, bounces_t=bounces_t,
                                 surface_t=surface_t, stream=stream)
    run = {"clean": clean, "diffuse": diffuse, "diffuse+": diffuse_all, "materials": materials}
    names = [a.only] if a.only else ["clean", "diffuse", "diffuse+", "materials"]

    def timed(name):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        e0.record()
        run[name]()
        e1.record()
        ctx.compact_dev(P, N, ios[name][0], stream)
        e2.record()
        e2.synchronize()
        return e0.elapsed_time(e1), e0.elapsed_time(e2), int(ios[name][2].sum().item())
    for _ in range(a.warmup):
        for k in names:
            timed(k)
    scan, both, kept = {k: [] for k in names}, {k: [] for k in names}, {}
    for step in range(a.steps):
        r = step % len(names)
        for k in names[r:] + names[:r]:     # rotate which one goes first
            s, b, c = timed(k)
            scan[k].append(s)
            both[k].append(b)
            kept[k] = c
    out = {"workload": f"C3 {bench.SCENE} {sensor.vertical_res}x{sensor.horizontal_res} rays x {P} poses", "rays": P * N,
           "steps": a.steps, "warmup": a.warmup, "glass": a.glass, "mirror": a.mirror, "retro_deg": a.retro_deg,
           "max_bounces": a.max_bounces, "quantised_nodes": int(scene.info["quantised_nodes"])}
    for k in names:
        s, b = np.array(scan[k]), np.array(both[k])
        out[k] = {"scan_median_ms": round(float(np.median(s)), 4), "scan_min_ms": round(float(s.min()), 4),
                  "scan_max_ms": round(float(s.max()), 4), "scan_and_compact_median_ms": round(float(np.median(b)), 4),
                  "kept_rows": kept[k]}
    if "materials" in names:
        t = hits["materials"]["t"].cpu().numpy()
        bn = bounces_t.cpu().numpy()
        ret = t != np.inf
        out["materials"]["returns_per_bounce_count"] = np.bincount(bn[ret], minlength=a.max_bounces + 1).tolist()
        out["materials"]["rays_without_return"] = int((~ret).sum())
        if "clean" in names:
            out["materials"]["clean_rays_without_return"] = int((hits["clean"]["t"].cpu().numpy() == np.inf).sum())
    if "clean" in names and "diffuse" in names:
        same = all(bool(torch.equal(hits["clean"][c], hits["diffuse"][c])) for c in cols)
        out["diffuse"]["records_equal_the_clean_scan"] = same
        out["diffuse_over_clean_scan_median"] = round(out["diffuse"]["scan_median_ms"] / out["clean"]["scan_median_ms"], 4)
    if "clean" in names and "diffuse+" in names:
        out["diffuse+_over_clean_scan_median"] = round(out["diffuse+"]["scan_median_ms"] / out["clean"]["scan_median_ms"], 4)
    if "clean" in names and "materials" in names:
        out["materials_over_clean_scan_median"] = round(out["materials"]["scan_median_ms"] / out["clean"]["scan_median_ms"], 4)
    print(json.dumps(out, indent=1))
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
