#!/usr/bin/env python3
"""Non-rigid scene-flow timings: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x 64 poses,
bench.c3_poses) on synth_A6_office2 with the walker (synth.make_walker, 384 triangles, a deformable) on the walk of
tools/movers_time.py.

HIP events around each call, --warmup rounds first, then --steps rounds interleaved, median and minimum:
    movers             lrc_scan_movers_dev with the walker in shape A: the records both flow calls read
    rigid_only         lrc_scan_flow_dev on those records without a status column (flow_rays_kernel alone)
    nonrigid_only      lrc_scan_nonrigid_flow_dev with the pair (shape A -> shape B), no status (nonrigid_target_kernel alone)
    rigid_status       lrc_scan_flow_dev with the status: the ray kernel and every pass behind it
    nonrigid_status    lrc_scan_nonrigid_flow_dev with the status: the same passes behind the non-rigid ray kernel
    snapshot           lrc_deform_snapshot_dev
    loop_rigid         per frame: scan_deforming_dev's steps (set, scan), then after all frames one lrc_scan_flow_dev
    loop_nonrigid      scan_deforming_flow_dev: per frame set / scan / snapshot / set / flow, the shape changing in every frame
Derived from the medians: nonrigid_only / rigid_only, nonrigid_status / rigid_status, loop_nonrigid / loop_rigid.

    python tools/nonrigid_flow_time.py --steps 20 --warmup 3 [--out report.txt]
profiles/nonrigid_flow_c3.txt holds this report.
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
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, deform, flow, synth
    from lidarcast.movers import MoverSet
    from movers_time import walks
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    size = synth.scene_size(a.scene)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    walker = synth.make_walker(instance=1000)
    d = deform.Deformable(ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
    mset = MoverSet(ctx, [d])
    P, N = len(poses), len(dirs)
    mp = walks(1, size, P)
    nxt, nmp, has = flow.pair_next(poses, mp)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    poses_t, dirs_t = dev(poses.reshape(P, 16)), dev(dirs)
    mt, nmt, nt, ht = dev(mp), dev(nmp), dev(nxt.reshape(P, 16)), dev(has)
    hits = DeviceHits(P * N, "cuda", want=("t", "point3", "prim"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    flow_t = torch.zeros((P * N, 3), dtype=torch.float32, device="cuda")
    status_t = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    shape_a, shape_b = (0, 1, 0.37), (2, 3, 0.8)
    shapes = deform.Clip(walker.keyframes.shape[0], cycle=1.1).shapes3(np.arange(P) * 0.1)[:, None, :]      # a new shape per frame
    d.set(*shape_a, stream=stream)
    snap = d.snapshot(stream=stream)                    # shape A, kept: the pair of every non-rigid call below
    spare = torch.empty_like(snap)                      # what the timed snapshot writes

    def movers():
        d.set(*shape_a, stream=stream)
        scene.scan_movers_dev(poses_t, dirs_t, hits, sensor.max_range, mset, mt, mover_t=who, stream=stream)
        d.set(*shape_b, stream=stream)                  # the flow calls cast against the next shape

    def rigid(status):
        scene.scan_flow_dev(hits, who, P, N, sensor.max_range, mset, mt, nmt, nt, flow_t, status_t=status, has_next_t=ht, stream=stream)

    def nonrigid(status):
        scene.scan_nonrigid_flow_dev(hits, who, P, N, sensor.max_range, mset, mt, nmt, nt, flow_t, pairs=[(0, snap, None)],
                                     status_t=status, has_next_t=ht, stream=stream)

    def loop_rigid():
        deform.scan_deforming_dev(scene, poses_t, dirs_t, hits, sensor.max_range, mset, mt, shapes, mover_t=who, stream=stream)
        rigid(status_t)

    def loop_nonrigid():
        deform.scan_deforming_flow_dev(scene, poses_t, dirs_t, hits, sensor.max_range, mset, mt, shapes, flow_t, status_t,
                                       mover_t=who, stream=stream)
    run = {"movers": movers, "rigid_only": lambda: rigid(None), "nonrigid_only": lambda: nonrigid(None),
           "rigid_status": lambda: rigid(status_t), "nonrigid_status": lambda: nonrigid(status_t),
           "snapshot": lambda: d.snapshot(spare, stream=stream), "loop_rigid": loop_rigid, "loop_nonrigid": loop_nonrigid}

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run[n]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    # the two loops leave other records and another shape behind: they go last in every round, and `movers` restores both
    names = list(run)
    for _ in range(a.warmup):
        for n in names:
            timed(n)
    ms = {n: [] for n in names}
    for _ in range(a.steps):            # interleaved: every configuration sees the same clocks
        for n in names:
            ms[n].append(timed(n))
    res = {"workload": f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses", "rays": P * N,
           "triangles": int(len(mesh.triangles)), "walker_triangles": int(len(walker.triangles))}
    res.update({n: _stats(v) for n, v in ms.items()})
    run["movers"]()
    run["nonrigid_status"]()
    torch.cuda.synchronize()
    kept = hits["t"].cpu().numpy() < np.inf
    walker_rows = (who.cpu().numpy() == 1) & kept
    f_non = flow_t.cpu().numpy().copy()
    s_non = status_t.cpu().numpy().copy()
    run["rigid_status"]()
    torch.cuda.synchronize()
    f_rig = flow_t.cpu().numpy()
    med = lambda n: res[n]["median_ms"]
    res["derived"] = {"walker_rows": int(walker_rows.sum()),
                      "status_counts_none_visible_occluded_out_of_range": np.bincount(s_non[kept], minlength=4).tolist(),
                      "rows_whose_flow_differs_from_the_rigid_step": int((f_non.view(np.uint32) != f_rig.view(np.uint32)).any(axis=1).sum()),
                      "largest_difference_m": round(float(np.abs(f_non[walker_rows] - f_rig[walker_rows]).max()), 4) if walker_rows.any() else 0.0,
                      "nonrigid_only_over_rigid_only": round(med("nonrigid_only") / med("rigid_only"), 4),
                      "nonrigid_status_over_rigid_status": round(med("nonrigid_status") / med("rigid_status"), 4),
                      "loop_nonrigid_over_loop_rigid": round(med("loop_nonrigid") / med("loop_rigid"), 4)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"tools/nonrigid_flow_time.py --steps {a.steps} --warmup {a.warmup} (MI355X, HIP events, ms)\n{text}\n")
    mset.close()
    d.close()
    scene.close()


if __name__ == "__main__":
    main()
