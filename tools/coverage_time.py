#!/usr/bin/env python3
"""Surface coverage timings, three workloads in one process:

  accumulate  C3 (bench.SCENE, 32 x 2048 rays x 64 poses): lrc_scan_poses_dev (t, prim) and lrc_coverage_accumulate_dev
              on its records, one set for the trajectory and one set per pose; HIP events around each launch, --warmup
              launches first, then --steps rounds alternating the three.
  select      the greedy selection over the poses of ALL planner candidates on synth_A6_office2 (standard 8-line sensor,
              one set per pose): host clock around lrc_coverage_select, which ends in its one synchronisation.
  planner     generate_optimal_trajectory with selection="reference" and "surface_coverage" on the same seed, host clock,
              alternating.

    python tools/coverage_time.py --steps 20 --warmup 3
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

import numpy as np  # noqa: E402


def _stats(v):
    v = np.array(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "n": len(v)}


def accumulate(a):
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, SurfaceCoverage, synth
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    ctx = lidarcast.Context(0)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dirs_t = torch.from_numpy(dirs).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "prim"))
    t0 = time.perf_counter()
    one = SurfaceCoverage(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, num_sets=1)
    create_ms = (time.perf_counter() - t0) * 1e3
    per = SurfaceCoverage(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, num_sets=P)
    zeros = torch.zeros(P, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    run = {"trace_t_prim": lambda: scene.scan_poses_dev(poses_t, dirs_t, hits, sensor.max_range, stream=stream),
           "accumulate_one_set": lambda: one.accumulate_dev(hits["t"], hits["prim"], P, N, zeros, stream=stream),
           "accumulate_set_per_pose": lambda: per.accumulate_dev(hits["t"], hits["prim"], P, N, stream=stream)}
    names = list(run)

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    run["trace_t_prim"]()
    for _ in range(a.warmup):
        for n in names:
            timed(n)
    ms = {n: [] for n in names}
    for step in range(a.steps):
        for n in (names if step % 2 == 0 else names[::-1]):
            ms[n].append(timed(n))
    t0 = time.perf_counter()
    s = one.summary(0)
    summary_ms = (time.perf_counter() - t0) * 1e3
    out = {"workload": f"C3 {bench.SCENE} {sensor.vertical_res}x{sensor.horizontal_res} x {P} poses",
           "rays": P * N, "triangles": len(mesh.triangles), "create_ms_host_clock": round(create_ms, 3),
           "summary_ms_host_clock": round(summary_ms, 3), "ratio": s.ratio}
    out.update({n: _stats(v) for n, v in ms.items()})
    out["accumulate_one_set_over_trace_median"] = round(out["accumulate_one_set"]["median_ms"] /
                                                        out["trace_t_prim"]["median_ms"], 4)
    for c in (one, per, scene):
        c.close()
    ctx.close()
    return out


def _planner_setup():
    from lidarcast import synth
    from s3dis_simulator import S3DISSimulator
    mesh = synth.make_scene("synth_A6_office2")
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    sim.load_scene(mesh, "synth_A6_office2")
    return sim, mesh


def select(a, sim, mesh):
    from trajectory import poses_from_waypoints
    gen = sim.auto_trajectory_generator
    np.random.seed(0)
    gen.room_analysis = gen._analyze_room_layout(mesh, sim._bounds_dict())
    cands = gen._generate_trajectory_candidates(max(int(20 * gen.interpolation_density), gen.min_waypoints))
    poses = np.concatenate([poses_from_waypoints(c.waypoints) for c in cands])
    eng = sim.raycast_engine
    t0 = time.perf_counter()
    cov = eng.coverage_sets(sim.lidar_config, poses, mesh)
    build_ms = (time.perf_counter() - t0) * 1e3
    P = len(poses)
    cov.select(P)
    ms, picks = [], None
    for _ in range(a.steps):
        t0 = time.perf_counter()
        picks, _, cum = cov.select(P)
        ms.append((time.perf_counter() - t0) * 1e3)
    union = cov.summary(None)
    p90, _, _ = cov.select(P, target_ratio=0.9 * union.ratio)
    out = {"candidates": len(cands), "poses": P, "rays_per_pose": len(eng._direction_table(sim.lidar_config)),
           "bitset_mb": round(P * cov.words_per_set * 4 / 1e6, 2),
           "scan_and_accumulate_ms_host_clock": round(build_ms, 2), "select_all": _stats(ms),
           "picks_to_gain_0": len(picks), "picks_to_90pct_of_union": len(p90), "union_ratio": union.ratio}
    cov.close()
    return out


def planner(a, sim, mesh):
    gen = sim.auto_trajectory_generator
    b = sim._bounds_dict()
    ms = {"reference": [], "surface_coverage": []}
    for step in range(a.warmup + a.steps):
        for sel in (("reference", "surface_coverage") if step % 2 == 0 else ("surface_coverage", "reference")):
            np.random.seed(1)
            t0 = time.perf_counter()
            gen.generate_optimal_trajectory(mesh, b, num_waypoints=20, selection=sel)
            if step >= a.warmup:
                ms[sel].append((time.perf_counter() - t0) * 1e3)
    return {k: _stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"accumulate": accumulate(a)}
    sim, mesh = _planner_setup()
    out["select"] = select(a, sim, mesh)
    out["planner"] = planner(argparse.Namespace(steps=max(3, a.steps // 4), warmup=1), sim, mesh)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
