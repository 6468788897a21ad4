#!/usr/bin/env python3
"""Dynamic occupancy timings: the C3 trajectory (bench.c3_sensor, 32 x 2048 rays x 64 poses,
bench.c3_poses) on synth_A6_office2, default extent, voxel 0.05, in three shapes:

  one_slot      all 64 poses into ONE slot of a sequence, beside lrc_voxgrid_accumulate_dev on the same scan's records in
                the same session (the existing walk kernel: the yardstick), alternating the two
  per_frame     F = 64, one slot per pose, no mover
  pedestrian    F = 64, one slot per pose, one pedestrian crossing the room (lrc_scan_movers_dev's records and mover column)

Per shape, HIP events around reset + accumulate of the whole trajectory and around finalize_dev with the dense state.
--warmup rounds first, then --steps rounds.  The scans themselves are not timed (their records are the input).

    python tools/voxseq_time.py --steps 20 --warmup 3
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="synth_A6_office2")
    ap.add_argument("--voxel", type=float, default=0.05)
    a = ap.parse_args()
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, OccupancyGrid, OccupancySequence, synth
    from lidarcast.movers import MoverSet, MoverTrack
    from lidarcast.voxgrid import default_extent
    from lidarcast.voxseq import pose_origins
    ctx = lidarcast.Context(0)
    mesh = synth.make_scene(a.scene)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    origins_t = torch.from_numpy(pose_origins(poses)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    # the records: the clean scan (with the t_label pairs the existing grid reads) and the scan with one pedestrian
    clean = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins", "t_label"))
    scene.scan_poses_dev(poses_t, dirs_t, clean, sensor.max_range, stream=stream)
    size = synth.scene_size(a.scene)
    track = MoverTrack([[0.0, 0.2 * size[0], 0.3 * size[1], 0.0, 30.0], [6.3, 0.8 * size[0], 0.7 * size[1], 0.0, 30.0]])
    mset = MoverSet(ctx, [synth.make_pedestrian(semantic=13, instance=1001)])
    mp_t = torch.from_numpy(track.poses12(np.arange(P) * 0.1)[:, None, :].copy()).cuda()
    walked = DeviceHits(P * N, "cuda", want=("t", "point3", "sem", "ins"))
    mover_t = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    scene.scan_movers_dev(poses_t, dirs_t, walked, sensor.max_range, mset, mp_t, mover_t, stream=stream)
    torch.cuda.synchronize()
    origin, dims = default_extent(mesh.vertices, a.voxel)
    V = int(np.prod(dims))
    grid = OccupancyGrid(ctx, origin, a.voxel, dims)
    one = OccupancySequence(ctx, origin, a.voxel, dims, 1)
    seq = OccupancySequence(ctx, origin, a.voxel, dims, P)
    zeros_t = torch.zeros(P, dtype=torch.int32, device="cuda")

    def grid_acc():
        grid.reset(stream)
        grid.accumulate_dev(poses_t, dirs_t, clean["t_label"], stream=stream)

    def one_acc():
        one.reset(stream)
        one.accumulate_dev(origins_t, clean, P, N, frame_of_pose_t=zeros_t, stream=stream)

    def frames_acc():
        seq.reset(stream)
        seq.accumulate_dev(origins_t, clean, P, N, stream=stream)

    def walker_acc():
        seq.reset(stream)
        seq.accumulate_dev(origins_t, walked, P, N, mover_t=mover_t, stream=stream)

    results = {}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    # each accumulate is followed by its own finalize: finalize reads what the accumulate before it left
    stages = [("voxgrid", grid_acc, lambda: grid.finalize()), ("one_slot", one_acc, lambda: one.finalize()),
              ("per_frame", frames_acc, lambda: seq.finalize()), ("pedestrian", walker_acc, lambda: seq.finalize())]
    ms = {f"{n}_{k}": [] for n, _, _ in stages for k in ("accumulate", "finalize")}
    for step in range(a.warmup + a.steps):
        order = stages if step % 2 == 0 else stages[::-1]            # alternate the order: drift hits every shape alike
        for n, acc, fin in order:
            ta, _ = timed(acc)
            tf, res = timed(fin)                                      # includes the copy of the result to the host
            if step >= a.warmup:
                ms[f"{n}_accumulate"].append(ta)
                ms[f"{n}_finalize"].append(tf)
            results[n] = res
    g, o1, fr, wk = (results[n] for n, _, _ in stages)
    assert np.array_equal(g.idx, o1.idx) and np.array_equal(g.state, o1.state[0]) and np.array_equal(g.returns, o1.returns)
    info = seq.info()
    returns = int(fr.counts[:, 5].sum())
    out = {"workload": f"C3 {a.scene} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses", "voxel_m": a.voxel,
           "dims": list(dims), "voxels": V, "rays": P * N, "returns": returns,
           "one_slot_equals_voxgrid": True,
           "pedestrian_dynamic_voxels": int(sum(sum(wk.dynamic_per_mover(f).values()) for f in range(P))),
           "per_frame_occupied_mean": float(fr.counts[:, 2].mean()), "per_frame_free_mean": float(fr.counts[:, 1].mean()),
           "bitset_bytes_per_frame": int(info.words_per_frame) * 4, "key_bytes_per_ray": 16,
           "finalize_scratch_bytes_per_ray": 8 + 8 + 4 + 4 + 4,
           "finalize_note": "finalize_* = lrc_voxseq_finalize_dev (or lrc_voxgrid_finalize_dev) plus the result's copy to the host"}
    out.update({n: _stats(v) for n, v in ms.items()})
    out["one_slot_over_voxgrid_accumulate"] = round(out["one_slot_accumulate"]["median_ms"] / out["voxgrid_accumulate"]["median_ms"], 3)
    print(json.dumps(out, indent=1))
    for x in (grid, one, seq, mset, scene):
        x.close()


if __name__ == "__main__":
    main()
