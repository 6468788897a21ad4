"""-m gpu: the HIP path (through the C ABI) against the CPU oracle, bit for bit.

Bars: hit mask, surviving ray indices and triangle ids bit-exact; range t
bit-exact (the allowed tolerance is 1e-5 m; the implementation meets 0 ulp and the tests assert it);
float64 incident angles within 1e-9 degree (device acos vs numpy's libm).
"""
import os

import numpy as np
import pytest

from helpers import (assert_bit_equal, pose, random_rays, random_soup, sensor_32x2048, sensor_8x512,
                     sensor_small)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def _scene_pair(ctx, mesh):
    import lidarcast
    from oracle.c_oracle import OracleMesh
    sem = getattr(mesh, "triangle_sem", None)
    ins = getattr(mesh, "triangle_ins", None)
    return lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, sem, ins), OracleMesh(mesh.vertices, mesh.triangles)


def _check_cast(scene, om, rays, brute):
    out = scene.cast(rays)
    t, prim = om.brute(rays) if brute else om.cast(rays, threads=8)
    assert_bit_equal(out["t"], t, "t")
    assert_bit_equal(out["prim"], prim, "prim")
    assert_bit_equal(out["normal3"], om.normals(prim), "normal")
    return out, t, prim


@pytest.mark.parametrize("seed,n_tris", [(0, 1), (1, 7), (2, 300), (3, 5000)])
def test_soup_vs_brute_force(ctx, seed, n_tris):
    from lidarcast.synth import TriangleMesh
    v, f = random_soup(n_tris, seed)
    scene, om = _scene_pair(ctx, TriangleMesh(v, f))
    rays = random_rays(3000, -5, 5, seed + 10)
    out, t, prim = _check_cast(scene, om, rays, brute=True)
    if n_tris >= 300:
        assert 0.05 < np.isfinite(t).mean() < 1.0


def test_room_vs_brute_force_and_bvh(ctx):
    from lidarcast import synth
    mesh = synth.make_room(size=(3, 2.5, 2), num_boxes=3, seed=11, cell=0.05)
    scene, om = _scene_pair(ctx, mesh)
    rays = random_rays(4000, 0.2, 1.8, 5)
    out, t, prim = _check_cast(scene, om, rays, brute=True)
    t2, prim2 = om.cast(rays)
    assert_bit_equal(t2, t, "oracle bvh vs brute")
    assert_bit_equal(prim2, prim)
    assert np.isfinite(t).mean() > 0.99
    # labels are those of the hit triangle
    hit = prim != 0xFFFFFFFF
    assert np.array_equal(out["sem"][hit], mesh.triangle_sem[prim[hit]])
    assert np.array_equal(out["ins"][hit], mesh.triangle_ins[prim[hit]])
    assert not out["sem"][~hit].any() and not out["ins"][~hit].any()


def test_known_answers(ctx):
    from lidarcast import synth
    # quad at z = 2: straight up hits at t = 2 exactly, point (0.25, 0.25, 2)
    scene, om = _scene_pair(ctx, synth.quad(z=2.0))
    rays = np.array([[0.25, 0.25, 0, 0, 0, 1], [0.25, 0.25, 0, 0, 0, -1], [5, 5, 0, 0, 0, 1],
                     [0.25, 0.25, 0, 0, 0, 2], [0.25, 0.25, 2.0, 0, 0, 1]], dtype=np.float32)
    out = scene.cast(rays)
    assert out["t"][0] == 2.0 and np.isinf(out["t"][1]) and np.isinf(out["t"][2])
    assert out["t"][3] == 1.0                      # t is parametric along the given direction
    assert np.isinf(out["t"][4])                   # tnear = 0 is exclusive: origin on the surface
    assert np.allclose(out["point3"][0], [0.25, 0.25, 2.0])
    # the reference multiplies the NORMALISED direction by the parametric t (raycast_engine_cpu.py:57-62),
    # which is only the hit point for unit directions; reproduced as is
    assert np.allclose(out["point3"][3], [0.25, 0.25, 1.0])
    assert np.array_equal(out["normal3"][0], [0, 0, 1]) and out["prim"][1] == 0xFFFFFFFF
    assert not out["point3"][1].any() and not out["normal3"][1].any()
    # unit cube from the centre: every ray hits, t = 1 / max|d_k|
    scene, om = _scene_pair(ctx, synth.unit_cube())
    rays = random_rays(5000, 0, 0, 3)
    out, t, prim = _check_cast(scene, om, rays, brute=True)
    expect = 1.0 / np.abs(rays[:, 3:].astype(np.float64)).max(axis=1)
    assert np.isfinite(t).all() and np.abs(t - expect).max() < 1e-5


def test_ties_edges_and_degenerates(ctx):
    from lidarcast.synth import TriangleMesh
    # two coincident quads (exact t ties -> smaller triangle row wins), a zero-area triangle, and rays
    # aimed exactly at shared edges / vertices / along the surface
    v = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2],
                  [-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2],
                  [0, 0, 1], [0, 0, 1], [0, 0, 1]], dtype=np.float64)
    f = np.array([[4, 5, 6], [4, 6, 7], [0, 1, 2], [0, 2, 3], [8, 9, 10]], dtype=np.int32)
    scene, om = _scene_pair(ctx, TriangleMesh(v, f))
    g = np.linspace(-1, 1, 21)
    X, Y = np.meshgrid(g, g)
    tgt = np.stack([X.ravel(), Y.ravel(), np.full(X.size, 2.0)], 1)
    o = np.array([0.1, -0.2, 0.0])
    d = tgt - o
    rays = np.concatenate([np.tile(o, (len(d), 1)), d], 1).astype(np.float32)
    graze = np.array([[-2, 0, 2, 1, 0, 0], [0, 0, 2, 1, 1, 0], [-2, -2, 2, 1, 1, 0]], dtype=np.float32)
    rays = np.concatenate([rays, graze])
    out, t, prim = _check_cast(scene, om, rays, brute=True)
    inside = np.isfinite(t[:len(d)])
    assert inside.mean() > 0.9
    assert set(np.unique(prim[:len(d)][inside])) <= {0, 1}      # rows 0/1 beat the coincident rows 2/3


def test_empty_and_tiny_inputs(ctx):
    import lidarcast
    from lidarcast.synth import TriangleMesh, quad
    scene = lidarcast.Scene(ctx, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    out = scene.cast(random_rays(100, -1, 1, 0))
    assert np.isinf(out["t"]).all() and (out["prim"] == 0xFFFFFFFF).all()
    scene = lidarcast.Scene(ctx, quad().vertices, quad().triangles)
    out = scene.cast(np.zeros((0, 6), np.float32))
    assert out["t"].shape == (0,) and out["point3"].shape == (0, 3)
    with pytest.raises(ValueError):
        scene.cast(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError):
        lidarcast.Scene(ctx, np.zeros((3, 3)), np.array([[0, 1, 3]]))        # index out of range
    for dt in (np.int32, np.int64):                                          # a negative index: int32 goes in uncopied and is
        with pytest.raises(ValueError):                                      # caught by the build's range check on the device
            lidarcast.Scene(ctx, np.eye(3), np.array([[0, 1, -1]], dtype=dt))
    with pytest.raises(ValueError):
        lidarcast.Scene(ctx, np.full((3, 3), np.nan), np.array([[0, 1, 2]]))


def test_bvh_invariants(ctx):
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_room(size=(3, 2, 2), num_boxes=3, seed=2, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles)
    nodes, slot_prim = scene.export_bvh()
    info = scene.info
    T = len(mesh.triangles)
    assert sorted(slot_prim.tolist()) == list(range(T))
    assert info["max_depth"] <= 31 and info["max_leaf_size"] <= 4
    refs = nodes[:, 12:14].view(np.int32)
    v32 = mesh.vertices.astype(np.float32)
    tri_lo = v32[mesh.triangles].min(axis=1)
    tri_hi = v32[mesh.triangles].max(axis=1)
    seen = np.zeros(T, bool)
    inner_seen = np.zeros(len(nodes), bool)
    inner_seen[0] = True

    def walk(ref, lo, hi, depth):
        """returns exact bounds below ref; checks they equal the stored child box"""
        if ref < 0:
            enc = ~ref
            first, cnt = enc >> 3, enc & 7
            assert 1 <= cnt <= 4 and depth <= 31
            ids = slot_prim[first:first + cnt]
            assert not seen[ids].any()
            seen[ids] = True
            blo, bhi = tri_lo[ids].min(0), tri_hi[ids].max(0)
        else:
            assert not inner_seen[ref] or ref == 0
            inner_seen[ref] = True
            n = nodes[ref]
            a = walk(int(refs[ref, 0]), n[0:3], n[3:6], depth + 1)
            b = walk(int(refs[ref, 1]), n[6:9], n[9:12], depth + 1)
            blo, bhi = np.minimum(a[0], b[0]), np.maximum(a[1], b[1])
        if lo is not None:
            assert np.array_equal(blo, lo) and np.array_equal(bhi, hi)     # exact, unpadded boxes
        return blo, bhi

    import sys
    sys.setrecursionlimit(10000)
    walk(0, None, None, 0)
    assert seen.all() and inner_seen.all()


# ---- configs C1/C2: 8 x 512 single pose in synth_A1_office ---------------------------------------
@pytest.fixture(scope="module")
def a1():
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_scene("synth_A1_office")
    return mesh, OracleMesh(mesh.vertices, mesh.triangles).build()


def test_c2_8x512_single_pose_bit_exact(engine, a1):
    from lidar import create_lidar
    from oracle import np_oracle
    mesh, om = a1
    lidar = create_lidar(sensor_8x512(), pose(4.0, 3.0, 1.0))
    pts, ang = engine.lidar_intersect_mesh(lidar, mesh)
    ref_pts, ref_ang, ref_idx = np_oracle.lidar_intersect_mesh(om, lidar, threads=8, return_index=True)
    assert pts.dtype == np.float32 and ang.dtype == np.float64
    assert_bit_equal(pts, ref_pts, "points")
    assert ang.shape == ref_ang.shape and np.abs(ang - ref_ang).max() < 1e-9
    # per-ray view: hit mask, surviving indices, triangle ids, t
    res = engine.cast_rays(lidar.get_rays(), mesh, center=lidar.pose[:3, 3], max_range=lidar.intrinsics.max_range)
    assert np.array_equal(np.flatnonzero(res["t_hit"] != np.inf), ref_idx)
    t, prim = om.cast(lidar.get_rays(), threads=8)
    assert_bit_equal(res["t_hit"][ref_idx], t[ref_idx])
    assert_bit_equal(res["primitive_ids"][ref_idx], prim[ref_idx])
    assert len(pts) > 4000
    # rays_intersect_mesh: same compaction without the range filter
    p2 = engine.rays_intersect_mesh(rays=lidar.get_rays(), mesh=mesh)
    assert_bit_equal(p2, np_oracle.rays_intersect_mesh(om, lidar.get_rays(), threads=8))


def test_range_filter_strict_and_rotated_pose(engine, a1):
    import dataclasses
    from lidar import create_lidar
    from oracle import np_oracle
    mesh, om = a1
    k = dataclasses.replace(sensor_8x512(), max_range=2.5)       # cuts through the hits
    lidar = create_lidar(k, pose(1.7, 2.2, 1.3, yaw=0.7))
    pts, ang = engine.lidar_intersect_mesh(lidar, mesh)
    ref_pts, ref_ang = np_oracle.lidar_intersect_mesh(om, lidar, threads=8)
    assert 0 < len(ref_pts) < 4096 * 0.9
    assert_bit_equal(pts, ref_pts)
    assert np.abs(ang - ref_ang).max() < 1e-9
    k0 = dataclasses.replace(sensor_8x512(), max_range=0.05)     # removes everything
    pts, ang = engine.lidar_intersect_mesh(create_lidar(k0, pose(4, 3, 1)), mesh)
    assert pts.shape == (0, 3) and ang.shape == (0,) and ang.dtype == np.float64


def test_dual_axis_seeded_noise(engine, a1):
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from oracle import np_oracle
    mesh, om = a1
    k = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
    np.random.seed(0)
    lidar = create_lidar(k, pose(4.0, 3.0, 1.0))
    rays = lidar.get_rays()

    class Frozen:                       # same rays for both engines
        intrinsics, pose = k, lidar.pose
        def get_rays(self):
            return rays
    pts, ang = engine.lidar_intersect_mesh(Frozen(), mesh)
    ref_pts, ref_ang = np_oracle.lidar_intersect_mesh(om, Frozen(), threads=8)
    assert rays.shape == (62739, 6)
    assert_bit_equal(pts, ref_pts)
    assert np.abs(ang - ref_ang).max() < 1e-9


def test_scan_poses_matches_per_pose_calls(engine):
    from lidar import create_lidar
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    from oracle import np_oracle
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    k = sensor_small(lines=6, width=200, max_range=2.2)
    poses = np.stack([pose(1.0 + 0.4 * i, 1.5, 1.0, yaw=0.0) for i in range(5)] + [pose(2.0, 1.4, 1.1, yaw=1.1)])
    rec, N = engine.scan_poses(k, poses, mesh, want=("t", "prim", "point3", "incident_deg", "sem", "ins"))
    assert N == 1200 and rec["t"].shape == (6, 1200)
    for p in range(len(poses)):
        lidar = create_lidar(k, poses[p])
        ref_pts, ref_ang, ref_idx = np_oracle.lidar_intersect_mesh(om, lidar, threads=4, return_index=True)
        keep = rec["t"][p] != np.inf
        # in-kernel ray generation is bit-identical to the host generator (numpy + BLAS), rotated pose included
        assert np.array_equal(np.flatnonzero(keep), ref_idx)
        assert_bit_equal(rec["point3"][p][keep], ref_pts)
        assert np.abs(rec["incident_deg"][p][keep] - ref_ang).max() < 1e-9


def test_uniform_fov_branch_and_drop_in_fast_path(engine):
    """lidar_intersect_mesh on this package's IndoorLidar (rays generated in the kernel) == the same call through a
    duck-typed lidar that forces host get_rays(), for both ray-generator branches and a rotated pose."""
    import dataclasses
    from lidar import create_lidar
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    for k in (sensor_small(lines=5, width=160, max_range=2.4),
              dataclasses.replace(sensor_small(lines=6, width=128, max_range=20.0), vertical_degrees=None,
                                  fov_up=20.0, fov_down=30.0)):
        for m in (pose(1.2, 1.4, 1.0), pose(2.2, 1.6, 1.1, yaw=-2.3)):
            lidar = create_lidar(k, m)

            class Duck:
                intrinsics, pose = lidar.intrinsics, lidar.pose
                def get_rays(self):
                    return lidar.get_rays()
            fast_pts, fast_ang = engine.lidar_intersect_mesh(lidar, mesh)
            host_pts, host_ang = engine.lidar_intersect_mesh(Duck(), mesh)
            assert len(host_pts) > 100
            assert_bit_equal(fast_pts, host_pts)
            assert_bit_equal(fast_ang, host_ang)


def test_compaction_matches_numpy(ctx):
    rng = np.random.default_rng(0)
    for nseg, seg_len in ((1, 1), (3, 1000), (5, 256), (2, 4097), (7, 63), (3, 64), (40, 1920), (2, 70001)):
        n = nseg * seg_len
        t = rng.uniform(0, 10, n).astype(np.float32)
        t[rng.random(n) < 0.37] = np.inf
        pts = rng.normal(size=(n, 3)).astype(np.float32)
        sem = rng.integers(0, 13, n).astype(np.uint16)
        ins = rng.integers(0, 60000, n).astype(np.uint16)
        ang = rng.uniform(0, 90, n)
        r = ctx.compact(t, seg_len, point3=pts, sem=sem, ins=ins, incident_deg=ang, want_index=True,
                        want_xyzl=True)
        keep = np.isfinite(t)
        assert r["total"] == keep.sum()
        assert np.array_equal(r["counts"], keep.reshape(nseg, seg_len).sum(1))
        assert_bit_equal(r["point3"], pts[keep])
        assert np.array_equal(r["sem"], sem[keep]) and np.array_equal(r["ins"], ins[keep])
        assert_bit_equal(r["incident_deg"], ang[keep])
        assert np.array_equal(r["index"], np.tile(np.arange(seg_len), nseg)[keep].astype(np.uint32))
        assert_bit_equal(r["xyzl"][:, :3], pts[keep])
        assert np.array_equal(r["xyzl"][:, 3].copy().view(np.uint32),
                              sem[keep].astype(np.uint32) | (ins[keep].astype(np.uint32) << 16))
    r = ctx.compact(np.full(300, np.inf, np.float32), 100, point3=np.zeros((300, 3), np.float32))
    assert r["total"] == 0 and r["point3"].shape == (0, 3)


def test_simulator_scan_stage(tmp_path):
    """S3DISSimulator.run_simulation (batched HIP scan) against the reference loop restated with the oracle."""
    import s3dis_simulator
    from containers import read_labeled_ply
    from lidar import create_lidar
    from lidarcast import synth
    from oracle import np_oracle
    from oracle.c_oracle import OracleMesh
    from trajectory import line_trajectory
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    sim.load_scene(mesh, "room")
    wps = line_trajectory((1.0, 1.5, 1.0), (3.0, 1.5, 1.0), 4)
    scene = sim.run_simulation(wps)
    assert scene.get_total_frames() == 4
    total = sim.lidar_config.get_total_points_per_scan()
    vol = sim.scene.room_bounds.get_volume()
    sems = []
    for i, wp in enumerate(wps):
        lidar = create_lidar(sim.lidar_config, wp.to_pose_matrix())
        ref_pts, _, idx = np_oracle.lidar_intersect_mesh(om, lidar, threads=8, return_index=True)
        f = scene.frames[i]
        assert_bit_equal(f.points, ref_pts)
        assert not f.incident_angles.any()                       # reference quirk, s3dis_simulator.py:266-269
        q = f.scan_quality
        assert q.num_points == len(ref_pts) and q.coverage_ratio == len(ref_pts) / total
        assert q.scan_density == len(ref_pts) / vol
        assert q.range_mean == np.mean(np.linalg.norm(ref_pts, axis=1))      # from the world origin
        _, prim = om.cast(lidar.get_rays(), threads=8)
        assert np.array_equal(f.semantic_labels, mesh.triangle_sem[prim[idx]])
        sems.append(f.semantic_labels)
    scene.save_results(tmp_path)
    rec = read_labeled_ply(tmp_path / "combined_pointcloud_with_label.ply")
    assert len(rec) == scene.get_total_points() and np.array_equal(rec["sem"], np.concatenate(sems))
    # the dual-axis sensor goes pose by pose through cast_rays
    sim2 = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}}, use_blk2go=True)
    sim2.load_scene(mesh, "room")
    np.random.seed(3)
    sc2 = sim2.run_simulation(wps[:2])
    np.random.seed(3)
    for i in range(2):
        lidar = create_lidar(sim2.lidar_config, wps[i].to_pose_matrix())
        rays = lidar.get_rays()
        class Frozen:
            intrinsics, pose = sim2.lidar_config, lidar.pose
            def get_rays(self):
                return rays
        ref_pts, _ = np_oracle.lidar_intersect_mesh(om, Frozen(), threads=8)
        assert_bit_equal(sc2.frames[i].points, ref_pts)


def test_device_path_fused_tile_counts_and_packed_rows(ctx):
    """The bench's device-resident step: scan_poses_dev (with per-wave keep counts) -> compact_dev into
    16-byte rows, against the host-array API of the same library and the oracle's hit count."""
    import torch
    import lidarcast
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    from lidar import IndoorLidar
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    for lines, width, max_range in ((4, 256, 2.0), (3, 100, 20.0)):       # 1024 (tiles line up) and 300 rays per pose
        k = sensor_small(lines=lines, width=width, max_range=max_range)
        poses = np.stack([pose(1.0 + 0.5 * i, 1.5, 1.0) for i in range(5)])
        dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
        P, N = len(poses), len(dirs)
        ref = scene.scan_poses(poses, dirs, k.max_range, want=("t", "point3", "sem", "ins"))
        dev = torch.device("cuda", 0)
        hits = lidarcast.DeviceHits(P * N, dev, want=("t", "point3", "sem", "ins", "tile_count", "t_label"))
        d_poses = torch.from_numpy(poses.reshape(P, 16)).to(dev)
        d_dirs = torch.from_numpy(dirs).to(dev)
        rows = torch.zeros((P * N, 4), dtype=torch.float32, device=dev)
        counts = torch.zeros(P, dtype=torch.int64, device=dev)
        io = LrcCompactIO()
        io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
        io.tile_count, io.counts, io.out_xyzl = hits["tile_count"].data_ptr(), counts.data_ptr(), rows.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        scene.scan_poses_dev(d_poses, d_dirs, hits, k.max_range, st)
        ctx.compact_dev(P, N, io, st)
        torch.cuda.synchronize()
        keep = np.isfinite(ref["t"])
        assert 0 < keep.sum() < P * N or max_range > 10
        assert np.array_equal(counts.cpu().numpy(), keep.reshape(P, N).sum(1))
        got = rows.cpu().numpy()[:keep.sum()]
        assert_bit_equal(got[:, :3], ref["point3"][keep])
        lab = ref["sem"][keep].astype(np.uint32) | (ref["ins"][keep].astype(np.uint32) << 16)
        assert np.array_equal(got[:, 3].copy().view(np.uint32), lab)
        # the same rows rebuilt from the 8-byte (t, label) pairs alone (what the multi-GPU all-gather moves)
        rows2 = torch.zeros_like(rows)
        counts2 = torch.zeros_like(counts)
        ctx.cloud_from_ranges_dev(d_poses, d_dirs, hits["t_label"], rows2, counts2, st)
        torch.cuda.synchronize()
        assert torch.equal(counts2, counts)
        assert torch.equal(rows2[:keep.sum()].view(torch.int32), rows[:keep.sum()].view(torch.int32))
        tl = hits["t_label"].cpu().numpy()
        assert np.array_equal(tl[:, 0].copy().view(np.float32), ref["t"])
        tc = hits["tile_count"].cpu().numpy()
        pad = np.zeros(len(tc) * 64, bool)
        pad[:P * N] = keep
        assert np.array_equal(tc, pad.reshape(-1, 64).sum(1))


def test_simulator_workflows_write_the_reference_file_set(tmp_path):
    """run_complete_simulation / run_auto_simulation under the reference's signatures: scene from a PLY path, straight
    or planned trajectory, scan, result files (reference s3dis_simulator.py:373-455)."""
    import json
    import s3dis_simulator
    from containers import read_labeled_ply
    from lidarcast import ply, synth
    from trajectory import PathType
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=3, seed=2, cell=0.08)
    path = tmp_path / "office_9.ply"
    ply.write_triangle_mesh(path, mesh)
    sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}, "trajectory": {"robot_height": 1.1}})
    with pytest.raises(ValueError):
        sim.generate_trajectory((1, 1, 1), (2, 1, 1))                 # no scene yet
    with pytest.raises(ValueError):
        sim.generate_auto_trajectory(5)
    sc = sim.run_complete_simulation(str(path), (1.0, 1.5, 1.0), (3.0, 1.5, 1.0), PathType.STRAIGHT, 5,
                                     output_dir=tmp_path / "a")
    assert sim.scene.scene_name == "office_9" and sim.trajectory_generator.robot_height == 1.1
    assert sc.get_total_frames() == 5 and sc.get_total_points() > 1000
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == [
        "combined_pointcloud.ply", "combined_pointcloud_with_label.ply", "simulation_statistics.txt",
        "simulation_summary.txt"]
    assert len(read_labeled_ply(tmp_path / "a" / "combined_pointcloud_with_label.ply")) == sc.get_total_points()
    wps, q = sim.generate_trajectory((1.0, 1.5, 1.0), (3.0, 1.5, 1.0), num_waypoints=9)
    assert len(wps) == 9 and isinstance(q, dict) and abs(q["path_length"] - 2.0) < 1e-12
    np.random.seed(4)
    sc2 = sim.run_auto_simulation(str(path), num_waypoints=6, output_dir=tmp_path / "b", scene_name="auto_room")
    assert sim.scene.scene_name == "auto_room" and sc2.get_total_frames() == len(sim.last_waypoints) > 0
    with open(tmp_path / "b" / "trajectory_analysis.json") as f:
        assert json.load(f) == json.loads(json.dumps(sim.last_analysis))
    assert (tmp_path / "b" / "combined_pointcloud_with_label.ply").exists()
    with pytest.raises(NotImplementedError):
        sim.add_furniture(mesh, "desk")
    with pytest.raises(FileNotFoundError):
        s3dis_simulator.load_default_config()
    cfg = tmp_path / "c.yaml"
    cfg.write_text("raycast_engine:\n  use_gpu: true\ntrajectory:\n  robot_height: 0.8\n")
    sim3 = s3dis_simulator.create_simulator_from_config(str(cfg))
    assert sim3.config["trajectory"]["robot_height"] == 0.8


def test_opt_in_intensity(engine, a1):
    """Row N4: lrc_hits.intensity = |h.n| in float32 (Lambertian return), 0 on a miss, and requesting it changes no
    other output.  Restated with numpy from the engine's own normals and the rays' unit directions."""
    mesh, _ = a1
    k = sensor_small(lines=6, width=128, max_range=4.0)
    lidar = __import__("lidar").create_lidar(k, pose(2.0, 3.0, 1.0, yaw=0.4))
    rays = lidar.get_rays()
    scene = engine.scene_for(mesh)
    base = scene.cast(rays, center=lidar.pose[:3, 3], max_range=k.max_range, want=("t", "prim", "normal3", "point3"))
    got = scene.cast(rays, center=lidar.pose[:3, 3], max_range=k.max_range,
                     want=("t", "prim", "normal3", "point3", "intensity"))
    for a in ("t", "prim", "normal3", "point3"):
        assert_bit_equal(got[a], base[a], a)
    only = scene.cast(rays, center=lidar.pose[:3, 3], max_range=k.max_range, want=("intensity",))
    assert_bit_equal(only["intensity"], got["intensity"])
    hit = np.isfinite(got["t"])
    assert 0 < hit.sum() < len(rays)
    d = rays[:, 3:]
    h = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    n = got["normal3"]
    want = np.abs(np.float32(h[:, 2] * n[:, 2]) + (np.float32(h[:, 1] * n[:, 1]) + np.float32(h[:, 0] * n[:, 0])))
    assert got["intensity"].dtype == np.float32 and (got["intensity"][~hit] == 0).all()
    assert np.abs(got["intensity"][hit] - want[hit]).max() <= 2e-7          # fused vs unfused products
    assert (got["intensity"] >= 0).all() and (got["intensity"] <= 1.0 + 1e-6).all()
    poses = np.stack([lidar.pose, pose(2.5, 3.0, 1.0)])
    rec, n_per = engine.scan_poses(k, poses, mesh, want=("t", "intensity"))
    assert_bit_equal(rec["intensity"][0], got["intensity"])


def test_in_kernel_rays_keep_the_sign_of_zero_components(ctx):
    """np.dot(directions, R.T) runs through dgemm, which accumulates from +0.0: a zero component of a rotated
    direction is +0.0 even when its only non-zero product is -0.0.  The in-kernel generator must give the same sign,
    because for a ray that lies exactly in a box plane the sign of the zero decides hit or miss.  Direction tables with
    exact (signed) zeros, origins on the planes of a unit cube and of a snapped triangle soup: pose-batched scan ==
    cast of the host-generated rays, bit for bit."""
    import lidarcast
    from lidarcast import synth
    cube = synth.unit_cube()
    rng = np.random.default_rng(3)
    soup_v = rng.choice([-1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0], size=(90, 3))
    soup_f = np.arange(90).reshape(-1, 3)
    comps = [0.0, -0.0, 1.0, -1.0, 0.5]
    dirs = np.array([[a, b, c] for a in comps for b in comps for c in comps if (a, b, c) != (0.0, 0.0, 0.0)
                     and any(x != 0 for x in (a, b, c))], dtype=np.float64)
    poses = np.stack([pose(x, y, z, yaw=yaw) for (x, y, z) in ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (-1.0, 2.0, 1.0),
                                                                (1.0, 0.25, 0.0))
                      for yaw in (0.0, 0.5, np.pi / 2, np.pi, -2.0)])
    for v, f in ((np.asarray(cube.vertices), np.asarray(cube.triangles)), (soup_v, soup_f)):
        scene = lidarcast.Scene(ctx, v, f)
        got = {k: a.reshape(len(poses), len(dirs)) for k, a in
               scene.scan_poses(poses, dirs, 100.0, want=("t", "prim")).items()}
        for p, m in enumerate(poses):
            d = np.dot(dirs, m[:3, :3].T).astype(np.float32)
            o = np.repeat(m[:3, 3][None, :], len(dirs), 0).astype(np.float32)
            ref = scene.cast(np.concatenate([o, d], 1), center=m[:3, 3], max_range=100.0, want=("t", "prim"))
            assert_bit_equal(got["t"][p], ref["t"], f"pose {p}")
            assert_bit_equal(got["prim"][p], ref["prim"], f"pose {p}")
        scene.close()


def test_cloud_rebuilt_from_triangle_ids(ctx):
    """What the multi-GPU all-gather moves is 4 bytes per ray, the hit triangle's row: the rows rebuilt from ids
    alone (t recomputed by the same ray/triangle test) equal the local compaction bit for bit -- over one
    contiguous array, and in place over per-rank send slabs (ids, then per-wave keep counts, then padding; a
    short rank padded with invalid ids), with and without the senders' counts, for yawed poses too."""
    import torch
    import lidarcast
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    from lidar import IndoorLidar
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    for lines, width, max_range in ((4, 256, 2.0), (3, 100, 20.0)):       # 1024 (tiles line up) and 300 rays per pose
        k = sensor_small(lines=lines, width=width, max_range=max_range)
        poses = np.stack([pose(1.0 + 0.5 * i, 1.5, 1.0, yaw=0.37 * i) for i in range(5)])
        dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
        P, N = len(poses), len(dirs)
        hits = lidarcast.DeviceHits(P * N, dev, want=("t", "prim", "point3", "sem", "ins", "tile_count"))
        d_poses = torch.from_numpy(poses.reshape(P, 16)).to(dev)
        d_dirs = torch.from_numpy(dirs).to(dev)
        rows = torch.zeros((P * N, 4), dtype=torch.float32, device=dev)
        counts = torch.zeros(P, dtype=torch.int64, device=dev)
        io = LrcCompactIO()
        io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
        io.tile_count, io.counts, io.out_xyzl = hits["tile_count"].data_ptr(), counts.data_ptr(), rows.data_ptr()
        scene.scan_poses_dev(d_poses, d_dirs, hits, k.max_range, st)
        ctx.compact_dev(P, N, io, st)
        torch.cuda.synchronize()
        K = int(counts.sum().item())
        assert 0 < K and (K < P * N or max_range > 10)
        # (1) one contiguous id array, counting pass in the rebuild
        rows2, counts2 = torch.full_like(rows, 7.0), torch.zeros_like(counts)
        scene.cloud_from_prims_dev(d_poses, d_dirs, hits["prim"], rows2, counts2, stream=st)
        torch.cuda.synchronize()
        assert torch.equal(counts2, counts)
        assert torch.equal(rows2[:K].view(torch.int32), rows[:K].view(torch.int32))
        # (2) three "ranks" of 2 poses each (the last one owns a single pose): slabs = ids | counts | padding
        pps, nslab = 2, 3
        tps = N // 64 if N % 64 == 0 else 0
        words = (pps * N + pps * tps + 3) // 4 * 4 + 8               # + 8: a stride larger than the payload
        slabs = torch.full((nslab * words,), -1, dtype=torch.int32, device=dev)
        prim = hits["prim"].view(P, N)
        tc = hits["tile_count"][:P * tps].view(P, tps) if tps else None
        for r in range(nslab):
            own = range(r * pps, min((r + 1) * pps, P))
            for j, pi in enumerate(own):
                slabs[r * words + j * N:r * words + (j + 1) * N] = prim[pi]
                if tps:
                    slabs[r * words + pps * N + j * tps:r * words + pps * N + (j + 1) * tps] = tc[pi]
            if tps:
                for j in range(len(own), pps):
                    slabs[r * words + pps * N + j * tps:r * words + pps * N + (j + 1) * tps] = 0
        padded = np.concatenate([poses, poses[:1]]).reshape(nslab * pps, 16)   # the padding pose is arbitrary
        d_padded = torch.from_numpy(padded).to(dev)
        for with_counts in ((True, False) if tps else (False,)):
            rows3 = torch.full_like(rows, 7.0)
            counts3 = torch.zeros(nslab * pps, dtype=torch.int64, device=dev)
            scene.cloud_from_prims_dev(d_padded, d_dirs, slabs, rows3, counts3,
                                       tile_count_t=slabs[pps * N:] if with_counts else None,
                                       poses_per_slab=pps, slab_stride_bytes=words * 4, stream=st)
            torch.cuda.synchronize()
            assert torch.equal(counts3[:P], counts) and int(counts3[P:].sum().item()) == 0
            assert torch.equal(rows3[:K].view(torch.int32), rows[:K].view(torch.int32))
            assert bool((rows3[K:] == 7.0).all())
    # argument checks: counts need aligned tiles; a range-noise scan cannot be rebuilt from ids
    with pytest.raises(ValueError):
        scene.cloud_from_prims_dev(d_poses, d_dirs, hits["prim"], rows2, counts2, tile_count_t=hits["tile_count"],
                                   stream=st)
    noise = torch.zeros(P * N, dtype=torch.float32, device=dev)
    scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
    with pytest.raises(ValueError):
        scene.cloud_from_prims_dev(d_poses, d_dirs, hits["prim"], rows2, counts2, stream=st)
    scene.reset_options()


def test_cloud_assembly_with_own_records_and_device_range_stats(ctx):
    """N-rank assembly where a rank's OWN rows are not rebuilt from ids but scattered from the records its trace wrote
    (lrc_cloud_from_prims_own_dev): three slabs of two poses, every slab in turn playing "own" -- the assembled cloud
    equals the single-process compaction bit for bit each time.  Then the ScanQuality range statistics of the assembled
    rows on the device (lrc_cloud_range_stats_dev) against np.mean / np.std of np.linalg.norm(points) per pose."""
    import torch
    import lidarcast
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    from lidar import IndoorLidar
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    k = sensor_small(lines=4, width=256, max_range=2.0)
    poses = np.stack([pose(1.0 + 0.4 * i, 1.5, 1.0, yaw=0.37 * i) for i in range(6)])
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
    P, N = len(poses), len(dirs)
    want = ("t", "prim", "point3", "sem", "ins", "tile_count")
    hits = lidarcast.DeviceHits(P * N, dev, want=want)
    d_poses, d_dirs = torch.from_numpy(poses.reshape(P, 16)).to(dev), torch.from_numpy(dirs).to(dev)
    rows = torch.zeros((P * N, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(P, dtype=torch.int64, device=dev)
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
    io.tile_count, io.counts, io.out_xyzl = hits["tile_count"].data_ptr(), counts.data_ptr(), rows.data_ptr()
    scene.scan_poses_dev(d_poses, d_dirs, hits, k.max_range, st)
    ctx.compact_dev(P, N, io, st)
    torch.cuda.synchronize()
    K = int(counts.sum().item())
    assert 0 < K < P * N
    pps, nslab, tps = 2, 3, N // 64
    words = (pps * N + pps * tps + 3) // 4 * 4 + 8
    slabs = torch.full((nslab * words,), -1, dtype=torch.int32, device=dev)
    for r in range(nslab):
        slabs[r * words:r * words + pps * N] = hits["prim"][r * pps * N:(r + 1) * pps * N]
        slabs[r * words + pps * N:r * words + pps * N + pps * tps] = hits["tile_count"][r * pps * tps:(r + 1) * pps * tps]
    for own in range(nslab):
        # the own rank's records: a separate scan of just its poses (what a rank holds), local indexing
        mine = lidarcast.DeviceHits(pps * N, dev, want=want)
        scene.scan_poses_dev(d_poses[own * pps:(own + 1) * pps], d_dirs, mine, k.max_range, st)
        oio = LrcCompactIO()
        oio.t, oio.point3, oio.sem, oio.ins = (mine[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
        # poison the own slab's ids: they must not be read
        poisoned = slabs.clone()
        poisoned[own * words:own * words + pps * N] = 123456789
        rows2 = torch.full_like(rows, 7.0)
        counts2 = torch.zeros(P, dtype=torch.int64, device=dev)
        scene.cloud_from_prims_dev(d_poses, d_dirs, poisoned, rows2, counts2, tile_count_t=poisoned[pps * N:],
                                   poses_per_slab=pps, slab_stride_bytes=words * 4, stream=st, own_slab=own, own_io=oio)
        torch.cuda.synchronize()
        assert torch.equal(counts2, counts), own
        assert torch.equal(rows2[:K].view(torch.int32), rows[:K].view(torch.int32)), own
        assert bool((rows2[K:] == 7.0).all())
    rng = torch.empty(P * N, dtype=torch.float32, device=dev)
    mean = torch.empty(P, dtype=torch.float32, device=dev)
    std = torch.empty(P, dtype=torch.float32, device=dev)
    ctx.cloud_range_stats_dev(rows, counts, rng, mean, std, stream=st)
    torch.cuda.synchronize()
    pts = rows[:K, :3].cpu().numpy()
    ends = np.cumsum(counts.cpu().numpy())
    for p in range(P):
        seg = pts[ends[p] - int(counts[p]):ends[p]]
        r = np.linalg.norm(seg, axis=1)
        assert r.dtype == np.float32
        assert np.mean(r) == mean[p].item() and np.std(r) == std[p].item(), p


def test_examples_run(tmp_path):
    """examples/ are part of the documentation: they must run as written."""
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "drop_in_engine.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "lidar_intersect_mesh:" in r.stdout and "bad input -> ValueError" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "simulate_room.py"), "--out",
                        str(tmp_path / "out"), "--waypoints", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "combined_pointcloud_with_label.ply" in r.stdout and "planned" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "scan_trajectory.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "scan_frames   : 16 frames" in r.stdout and "run_simulation: 16 frames" in r.stdout


def test_many_short_poses(ctx):
    """A long trajectory of small scans (3 000 poses x 96 rays: more poses than threads in a workgroup, rays per pose
    not a multiple of the wave size): per-pose counts, compaction and the rebuild from ids agree with numpy on the
    host records; a sample of poses agrees with the host-ray path."""
    import torch
    import lidarcast
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    from lidar import IndoorLidar
    mesh = synth.make_room(size=(6, 4, 2.5), num_boxes=5, seed=8, cell=0.05)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    k = sensor_small(lines=3, width=32, max_range=2.5)
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
    rng = np.random.default_rng(5)
    P, N = 3000, len(dirs)
    poses = np.stack([pose(*rng.uniform([0.5, 0.5, 0.5], [5.5, 3.5, 2.0]), yaw=float(rng.uniform(-3, 3))) for _ in range(P)])
    host = scene.scan_poses(poses, dirs, k.max_range, want=("t", "prim", "point3", "sem", "ins"))
    keep = np.isfinite(host["t"]).reshape(P, N)
    assert 0.05 < keep.mean() < 0.95
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    hits = lidarcast.DeviceHits(P * N, dev, want=("t", "prim", "point3", "sem", "ins"))
    d_poses, d_dirs = torch.from_numpy(poses.reshape(P, 16)).to(dev), torch.from_numpy(dirs).to(dev)
    scene.scan_poses_dev(d_poses, d_dirs, hits, k.max_range, st)
    rows = torch.full((P * N, 4), 7.0, dtype=torch.float32, device=dev)
    counts = torch.zeros(P, dtype=torch.int64, device=dev)
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
    io.counts, io.out_xyzl = counts.data_ptr(), rows.data_ptr()
    ctx.compact_dev(P, N, io, st)
    rows2, counts2 = torch.full_like(rows, 7.0), torch.zeros_like(counts)
    scene.cloud_from_prims_dev(d_poses, d_dirs, hits["prim"], rows2, counts2, stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), keep.sum(1)) and torch.equal(counts2, counts)
    K = int(keep.sum())
    got = rows.cpu().numpy()
    assert_bit_equal(got[:K, :3], host["point3"][keep.reshape(-1)])
    lab = host["sem"][keep.reshape(-1)].astype(np.uint32) | (host["ins"][keep.reshape(-1)].astype(np.uint32) << 16)
    assert np.array_equal(got[:K, 3].copy().view(np.uint32), lab) and (got[K:] == 7.0).all()
    assert torch.equal(rows2.view(torch.int32), rows.view(torch.int32))
    for p in (0, 1, 255, 256, 257, 1023, 2999):
        ref = scene.cast(IndoorLidar(k, poses[p]).get_rays(), center=poses[p][:3, 3], max_range=k.max_range,
                         want=("t", "prim"))
        assert_bit_equal(host["t"].reshape(P, N)[p], ref["t"], f"pose {p}")
        assert_bit_equal(host["prim"].reshape(P, N)[p], ref["prim"], f"pose {p}")


def test_full_size_c3_properties(ctx):
    """BASELINE config C3 at full size (64 poses x 65 536 rays, T = 605 328), device-resident path.
    Size-independent properties + every ray of all 64 poses against the oracle."""
    import hashlib
    import torch
    import bench
    import full_parity as fp
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    mesh = synth.make_scene(bench.SCENE)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    P, N = len(poses), len(dirs)
    dev = torch.device("cuda", 0)
    hits = lidarcast.DeviceHits(P * N, dev, want=("t", "prim", "normal3", "point3", "sem", "ins", "tile_count"))
    d_poses, d_dirs = torch.from_numpy(poses.reshape(P, 16)).to(dev), torch.from_numpy(dirs).to(dev)
    rows = torch.zeros((P * N, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(P, dtype=torch.int64, device=dev)
    io = LrcCompactIO()
    io.t, io.point3, io.sem, io.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
    io.tile_count, io.counts, io.out_xyzl = hits["tile_count"].data_ptr(), counts.data_ptr(), rows.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    digests = []
    for _ in range(2):                                   # idempotence: two scans, identical bytes
        scene.scan_poses_dev(d_poses, d_dirs, hits, sensor.max_range, st)
        ctx.compact_dev(P, N, io, st)
        torch.cuda.synchronize()
        k = int(counts.sum().item())
        h = hashlib.sha256()
        for a in ("t", "prim", "normal3", "point3", "sem", "ins"):
            h.update(hits[a].cpu().numpy().tobytes())
        h.update(rows[:k].cpu().numpy().tobytes())
        digests.append(h.hexdigest())
    assert digests[0] == digests[1]
    t = hits["t"].cpu().numpy().reshape(P, N)
    prim = hits["prim"].cpu().numpy().view(np.uint32).reshape(P, N)
    pts = hits["point3"].cpu().numpy().reshape(P, N, 3)
    nrm = hits["normal3"].cpu().numpy().reshape(P, N, 3)
    hit = np.isfinite(t)
    assert hit.mean() > 0.999 and (prim[~hit] == 0xFFFFFFFF).all() and (prim[hit] < len(mesh.triangles)).all()
    assert np.array_equal(counts.cpu().numpy(), hit.sum(1)) and k == hit.sum()
    lo, hi = mesh.vertices.min(0) - 1e-3, mesh.vertices.max(0) + 1e-3
    assert (pts[hit] >= lo).all() and (pts[hit] <= hi).all()             # every hit lies inside the room
    assert np.abs(np.linalg.norm(nrm[hit], axis=1) - 1).max() < 1e-5
    assert np.array_equal(hits["sem"].cpu().numpy().view(np.uint16).reshape(P, N)[hit], mesh.triangle_sem[prim[hit]])
    rng = np.linalg.norm(pts - poses[:, None, :3, 3], axis=2)
    assert (rng[hit] < sensor.max_range).all() and np.abs(rng[hit] - t[hit]).max() < 1e-4   # unit directions
    assert np.array_equal(rows[:k, :3].cpu().numpy(), pts[hit])         # cloud = np.vstack of the frames
    # all 64 poses ray by ray against the oracle (tests/full_parity.py): surviving indices (the positions of the finite t),
    # points, t and triangle ids as the four-pose loop compared them, plus normals, labels, counts and the compacted rows;
    # a difference is reported with its pose, tile and lane
    want = fp.c3_expected()
    assert np.array_equal(hit.reshape(-1), want["keep"])
    got = {"t": t, "prim": prim, "point3": pts, "normal3": nrm,
           "sem": hits["sem"].cpu().numpy().view(np.uint16), "ins": hits["ins"].cpu().numpy().view(np.uint16),
           "counts": counts.cpu().numpy(), "rows": rows.cpu().numpy(), "fill": 0.0}
    assert fp.assert_scan_equal(got, want, "C3 full size") == P * N == 64 * 65536
    fp.report("C3 properties test, all 64 poses", want)


def test_bench_contract(tmp_path):
    """bench.py prints one JSON line with the driver's keys plus roofline and cpu_baseline objects; --steps is the number of
    timed steps, --dump-outputs writes what the last of them computed."""
    import json
    import subprocess
    import sys
    from conftest import REPO
    steps = 2000                     # ~0.8 s of timed steps: a stable figure for the pipelined / serial comparison below
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", str(steps), "--warmup", "3",
                          "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, check=True).stdout
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r = json.loads(line[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in r, k
    assert r["n_gpus"] == 1 and r["steps"] == steps and r["unit"] == "rays/s" and r["vs_baseline"] is None
    # throughput guards that guard: the round-3 step did 11.3 G rays/s on the slowest box seen (a regression to the round-2
    # kernel or to a host-built scene lands below), and the pipelined step must not be slower than the two calls it replaces
    assert "workload" in r["config"] and r["value"] > 8e9
    assert r["config"]["step_arrangement"].startswith("scan pipeline")
    assert r["ms_per_step"] <= r["config"]["serial_ms_per_step"] * 1.01, (r["ms_per_step"], r["config"]["serial_ms_per_step"])
    assert r["config"]["scene_create_ms"] < 20.0                     # the device builder (a host build takes 130+ ms)
    rf = r["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(rf) and rf["bound"] == "valu"
    if rf["frac"] is not None:       # counters of THIS binary are committed (profiles/pmc_latest.json matches the sources)
        assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0.0 < rf["frac"] <= 1.0
        assert abs(rf["frac"] - rf["valu_issue_frac"] * rf["lane_utilisation"]) < 1e-6
        assert rf["traffic"] > 0 and rf["hbm_side"]["frac_of_hbm_peak"] < 1.0
    assert r["timed"]["blocks"] == 1 and r["timed"]["steps"] == steps and r["config"]["caller_path_rays_per_s"] > 1.5e9
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(r["cpu_baseline"])
    assert r["cpu_baseline"]["kind"] == ("port" if "not installed" in r["cpu_baseline"].get("open3d", "") else "reference")
    # the dumped outputs: float32 / float64 .npy files, at most 64 MB, the counts of every pose and the hits they add up to
    files = {f.name: np.load(f) for f in dump.iterdir()}
    assert set(files) == {"counts.npy", "row_index.npy", "points.npy", "sem.npy", "ins.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(f.stat().st_size for f in dump.iterdir()) <= 64 << 20
    c = files["counts.npy"]
    assert c.shape == (64,) and c.sum() == round(r["config"]["hit_fraction"] * r["config"]["rays_per_step_per_gpu"])
    m = len(files["row_index.npy"])
    assert files["points.npy"].shape == (m, 3) and len(files["sem.npy"]) == len(files["ins.npy"]) == m
    assert m == min(int(c.sum()), 1 << 20) and np.isfinite(files["points.npy"]).all()


def test_two_rank_launch_of_the_bench_path():
    """The N > 1 path launched the way the driver launches it (torch.distributed.run, one process per rank), two
    ranks sharing this one GPU with the collective staged through gloo (RCCL refuses two ranks on one device): pose
    sharding by rank, the gather of triangle ids -- as separate kernels (`prim`) and through the scan pipeline
    (`prim_pipe`: lrc_pipe_submit_sharded) --, and on EVERY rank a rebuilt scene cloud equal to the local
    compaction of all ranks' poses, bit for bit.  (With world size 1 the same code runs through RCCL: the
    --dist-selftest runs in DESIGN.md section 6.)"""
    import json
    import socket
    import subprocess
    import sys
    from conftest import REPO
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    seen = set()
    for forced in (None, "prim_pipe", "prim"):                 # the calibrated choice, then each id payload by name
        if forced in seen:
            continue
        env = dict(os.environ, LRC_DIST_BACKEND="gloo")
        if forced:
            env["LRC_DIST_PAYLOAD"] = forced
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(REPO, "bench.py"),
                            "--gpus", "2", "--steps", "3", "--warmup", "1", "--dist-selftest"],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr.count("dist selftest ok") == 2 and "world 2" in r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(line) == 1                                  # rank 0 alone prints
        res = json.loads(line[0])
        assert res["n_gpus"] == 2 and res["scaling"] == "weak" and "cpu_baseline" not in res
        assert res["config"]["rays_per_step_per_gpu"] == 64 * 65536 and 0.99 < res["config"]["hit_fraction"] <= 1.0
        assert forced is None or res["config"]["gather_payload"] == forced
        seen.add(res["config"]["gather_payload"])


def test_cast_segments_ragged_poses(engine, a1):
    """BLK2GO poses (ragged ray sets on one seeded stream) in one launch == pose-by-pose calls == oracle."""
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from oracle import np_oracle
    mesh, om = a1
    k = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
    poses = [pose(2.0 + 0.5 * i, 3.0, 1.0, yaw=0.2 * i) for i in range(3)]
    np.random.seed(11)
    lidars = [create_lidar(k, m) for m in poses]
    rec, off = engine.scan_lidars(lidars, mesh, want=("t", "prim", "point3", "incident_deg"))
    assert len(off) == 4 and off[0] == 0 and off[-1] == len(rec["t"]) and len(set(np.diff(off))) > 1
    np.random.seed(11)
    for i, m in enumerate(poses):
        rays = create_lidar(k, m).get_rays()
        assert len(rays) == off[i + 1] - off[i]

        class Frozen:
            intrinsics, pose = k, m
            def get_rays(self):
                return rays
        ref_pts, ref_ang, ref_idx = np_oracle.lidar_intersect_mesh(om, Frozen(), threads=8, return_index=True)
        sl = slice(off[i], off[i + 1])
        keep = rec["t"][sl] != np.inf
        assert np.array_equal(np.flatnonzero(keep), ref_idx)
        assert_bit_equal(rec["point3"][sl][keep], ref_pts)
        assert np.abs(rec["incident_deg"][sl][keep] - ref_ang).max() < 1e-9
    scene = engine.scene_for(mesh)
    with pytest.raises(ValueError):
        scene.cast_segments(np.zeros((4, 6), np.float32), [0, 5], np.zeros((1, 3)), 1.0)     # offsets do not end at N
    with pytest.raises(ValueError):
        scene.cast_segments(np.zeros((4, 6), np.float32), [0, 3, 2, 4], np.zeros((3, 3)), 1.0)   # decreasing


def test_opt_in_sensor_options(ctx):
    """Row N4: min_range, host-drawn range noise and the ray/normal incident angle.  Off by default (the
    reference never applies them); when on, checked against a numpy restatement."""
    import lidarcast
    from lidarcast import synth
    from lidar import IndoorLidar, create_lidar
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles)
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    k = sensor_small(lines=6, width=300, max_range=2.6)
    lidar = create_lidar(k, pose(1.4, 1.5, 1.0, 0.4))
    rays = lidar.get_rays()
    c = lidar.pose[:3, 3]
    base = scene.cast(rays, center=c, max_range=k.max_range)
    t0, prim0 = om.cast(rays)
    rs = np.random.RandomState(5)
    noise = rs.normal(0, 0.02, len(rays)).astype(np.float32)
    noise[::50] = -100.0                                        # forces t' <= 0 on some rays
    scene.set_options(min_range=0.9, range_noise=noise, incident_mode=1)
    out = scene.cast(rays, center=c, max_range=k.max_range)
    # numpy restatement
    t1 = (t0 + noise).astype(np.float32)
    ok = np.isfinite(t0) & (t1 > 0)
    d = rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    pts = np.where(ok[:, None], rays[:, :3] + d * np.where(ok, t1, 0)[:, None], 0).astype(np.float32)
    dist = np.linalg.norm(pts.astype(np.float64) - c, axis=1)
    keep = ok & (dist < k.max_range) & (dist >= 0.9)
    assert 0 < keep.sum() < ok.sum() < len(rays)
    assert np.array_equal(np.isfinite(out["t"]), keep)
    assert_bit_equal(out["t"][keep], t1[keep])
    assert_bit_equal(out["point3"][keep], pts[keep])
    assert np.array_equal(out["prim"][keep], prim0[keep]) and (out["prim"][~keep] == 0xFFFFFFFF).all()
    nrm = om.normals(prim0)[keep].astype(np.float64)
    dd = d[keep].astype(np.float64)
    cs = np.abs((dd[:, 0] * nrm[:, 0] + dd[:, 1] * nrm[:, 1]) + dd[:, 2] * nrm[:, 2])
    want = np.degrees(np.arccos(np.minimum(cs, 1.0)))
    assert np.abs(out["incident_deg"][keep] - want).max() < 1e-6 and out["incident_deg"][keep].max() <= 90.0
    with pytest.raises(ValueError):
        scene.cast(rays[:10], center=c, max_range=k.max_range)          # noise length mismatch
    with pytest.raises(ValueError):
        scene.set_options(min_range=-1.0)
    scene.reset_options()
    again = scene.cast(rays, center=c, max_range=k.max_range)
    for key in ("t", "point3", "prim", "incident_deg"):
        assert_bit_equal(again[key], base[key])


def _surface_cloud(m, seed):
    """annotated points on the faces of a 5 x 4 x 3 box with mm-level scatter (S3DIS-like density)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform([0, 0, 0], [5, 4, 3], size=(m, 3))
    face = rng.integers(0, 6, m)
    for a in range(3):
        p[face == 2 * a, a] = 0.0
        p[face == 2 * a + 1, a] = [5, 4, 3][a]
    return p + rng.normal(0, 0.002, p.shape)


def test_nearest_annotated_point_vs_sklearn_ball_tree(ctx):
    """Row N1: the GPU 1-NN against the reference's own query (sklearn ball_tree, s3dis_sim_scene.py:416-418)."""
    import lidarcast
    from sklearn.neighbors import NearestNeighbors
    cloud = _surface_cloud(150_000, 1)
    q = (_surface_cloud(40_000, 2) + np.random.default_rng(3).normal(0, 0.01, (40_000, 3))).astype(np.float32)
    q[:50] += 3.0                                             # queries well outside the cloud's bounding box
    nn = lidarcast.NearestIndex(ctx, cloud)
    idx, dist = nn.query(q, return_distance=True)
    ref_d, ref_i = NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(cloud).kneighbors(q)
    assert np.array_equal(idx, ref_i[:, 0].astype(np.uint32))
    assert np.abs(dist - ref_d[:, 0]).max() < 1e-12
    # brute force on a slice (float64, same expression)
    sl = slice(0, 300)
    d2 = ((q[sl].astype(np.float64)[:, None, :] - cloud[None, :, :]) ** 2)
    d2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
    assert np.array_equal(idx[sl], d2.argmin(1).astype(np.uint32))
    # other grid spacings give the same answer
    for h in (0.01, 0.5, 50.0):
        assert np.array_equal(lidarcast.NearestIndex(ctx, cloud, cell_size=h).query(q[:5000]), idx[:5000])
    # duplicates: ties go to the smaller row; a single point; empty query
    dup = np.concatenate([cloud[:1000], cloud[:1000]])
    assert (lidarcast.NearestIndex(ctx, dup).query(cloud[:1000].astype(np.float32)) < 1000).all()
    one = lidarcast.NearestIndex(ctx, np.array([[1.0, 2.0, 3.0]]))
    assert (one.query(q[:100]) == 0).all() and one.query(np.zeros((0, 3), np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        lidarcast.NearestIndex(ctx, np.zeros((0, 3)))


def test_export_labels_from_annotated_cloud(tmp_path, engine):
    """S3DISSimScene._get_colors_and_labels_from_s3dis with an annotated cloud == the reference's sklearn path;
    baked per-triangle labels arrive per ray through the trace kernel."""
    import lidarcast
    from sklearn.neighbors import NearestNeighbors
    from containers import S3DISSimFrame, S3DISSimScene, ScanQuality, read_labeled_ply
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=3, seed=8, cell=0.05)
    rng = np.random.default_rng(0)
    v = mesh.vertices
    tri = mesh.triangles[rng.integers(0, len(mesh.triangles), 60_000)]
    w = rng.dirichlet([1, 1, 1], len(tri))
    ann = (v[tri] * w[:, :, None]).sum(1) + rng.normal(0, 0.003, (len(tri), 3))     # annotated cloud near the surfaces
    ann_sem = rng.integers(0, 13, len(ann)).astype(np.uint16)
    ann_ins = rng.integers(0, 300, len(ann)).astype(np.uint16)
    ann_col = rng.random((len(ann), 3))
    k = sensor_small(lines=8, width=256, max_range=20.0)
    rec, n = engine.scan_poses(k, np.stack([pose(1.5, 1.5, 1.0), pose(2.5, 1.5, 1.0)]), mesh, want=("t", "point3"))
    sc = S3DISSimScene("room")
    sc.set_annotated_cloud(ann, ann_col, ann_sem, ann_ins)
    q = ScanQuality(0, 0, 0, 0, 0, 0, 0)
    for i in range(2):
        pts = rec["point3"][i][np.isfinite(rec["t"][i])]
        sc.append_frame(S3DISSimFrame(i, pts, np.zeros(len(pts)), q))
    sc.save_results(tmp_path)
    out = read_labeled_ply(tmp_path / "combined_pointcloud_with_label.ply")
    allp = sc.combined_points()
    ref_i = NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(ann).kneighbors(allp)[1][:, 0]
    assert np.array_equal(out["sem"], ann_sem[ref_i]) and np.array_equal(out["ins"], ann_ins[ref_i])
    assert np.array_equal(np.stack([out["red"], out["green"], out["blue"]], 1), (ann_col[ref_i] * 255).astype(np.uint8))
    # baking: labels per triangle once, then per ray from the kernel
    nn = lidarcast.NearestIndex(engine.ctx, ann)
    sem_t, ins_t = lidarcast.bake_triangle_labels(nn, mesh.vertices, mesh.triangles, ann_sem, ann_ins)
    cen = mesh.vertices[mesh.triangles].mean(1)
    ref_t = NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(ann).kneighbors(cen.astype(np.float32))[1][:, 0]
    assert np.array_equal(sem_t, ann_sem[ref_t]) and np.array_equal(ins_t, ann_ins[ref_t])
    baked = synth.TriangleMesh(mesh.vertices, mesh.triangles, sem_t, ins_t)
    rec2, _ = engine.scan_poses(k, np.stack([pose(1.5, 1.5, 1.0)]), baked, want=("t", "prim", "sem", "ins"))
    hit = np.isfinite(rec2["t"][0])
    assert np.array_equal(rec2["sem"][0][hit], sem_t[rec2["prim"][0][hit]])
    assert np.array_equal(rec2["ins"][0][hit], ins_t[rec2["prim"][0][hit]])


def test_kernel_variants_are_bit_identical():
    """Traversal order / fetch strategy / leaf size / builder must not change a single output byte.
    The product library with the scene built on the device (default) and on the host, with smaller leaves, with every
    split forced through the median fallback, on float32 nodes and on forced quantised images; then the laboratory build
    (-DLRC_VARIANTS, liblidarcast_lab.so through LRC_LIB): the packet kernel behind the grid entry point (on by default
    there) and with it off, the workgroup -> tile order (XCD striping, the default for this scan, against contiguous ranges
    and another chunk size), scalar fetch off, one triangle per leaf round trip, speculative postponement, private refill,
    four-wide nodes, and every third / every ray sent through the redo route (the route a ray takes when its closest
    candidate fails the box clause, which no input so far has made happen), on quantised and on float32 nodes."""
    import subprocess
    import sys
    import __graft_entry__ as entry
    from conftest import REPO
    tool = os.path.join(REPO, "tools", "variant_digest.py")
    assert os.path.exists(entry.LAB_LIB)
    lab = {"LRC_LIB": entry.LAB_LIB}
    variants = {"default": {}, "host_builder": {"LRC_DEVICE_BUILD": "0"},
                "leaves_of_2": {"LRC_MAX_LEAF": "2"}, "leaves_of_1": {"LRC_MAX_LEAF": "1"},
                "leaves_of_1_host_builder": {"LRC_MAX_LEAF": "1", "LRC_DEVICE_BUILD": "0"},
                "median_splits_only": {"LRC_BUILD_MEDIAN_ONLY": "1"}, "no_depth_slack": {"LRC_DEPTH_SLACK": "0"},
                "float32_nodes": {"LRC_QNODES": "0"}, "quantised_nodes_forced": {"LRC_QNODES": "2"},
                "lab_default": lab, "lab_no_packet_kernel": dict(lab, LRC_SECTOR="0"),
                "contiguous_tile_ranges": dict(lab, LRC_SECTOR="0", LRC_TILE_CHUNK="-1"),
                "tile_chunks_of_32": dict(lab, LRC_SECTOR="0", LRC_TILE_CHUNK="32"),
                "no_scalar_fetch": dict(lab, LRC_UNIFORM="0"), "leaf_singles": dict(lab, LRC_LEAFW="1"),
                "speculative": dict(lab, LRC_SPEC="1"), "speculative_leaf_singles": dict(lab, LRC_SPEC="1", LRC_LEAFW="1"),
                "refill_2": dict(lab, LRC_REFILL="2"),
                "refill_4": dict(lab, LRC_REFILL="4"), "refill_2_w7": dict(lab, LRC_REFILL="2", LRC_REFILL_W="7"),
                "quantised_leaf_singles": dict(lab, LRC_QNODES="2", LRC_LEAFW="1"),
                "four_wide_nodes": dict(lab, LRC_QNODES="2", LRC_WIDE="1"),
                "every_third_ray_redone": dict(lab, LRC_QNODES="2", LRC_DEBUG_FORCE_REDO="3"),
                "every_ray_redone": dict(lab, LRC_QNODES="2", LRC_DEBUG_FORCE_REDO="1"),
                "every_ray_redone_float32_nodes": dict(lab, LRC_QNODES="0", LRC_DEBUG_FORCE_REDO="1")}
    digests = {}
    for name, env in variants.items():
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=300, env=e, check=True)
        digests[name] = r.stdout.strip().splitlines()[-1]
    assert len(set(digests.values())) == 1, digests
    assert int(digests["default"].split()[1]) > 30000 and int(digests["default"].split()[2]) > 1000


def _build_both(ctx, mesh, **env):
    """The same mesh through the host builder and the device builder (LRC_* build knobs from env)."""
    import lidarcast
    scenes = []
    keys = list(env) + ["LRC_DEVICE_BUILD"]
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        for dev in ("0", "1"):
            os.environ["LRC_DEVICE_BUILD"] = dev
            scenes.append(lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, getattr(mesh, "triangle_sem", None),
                                          getattr(mesh, "triangle_ins", None)))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return scenes


def _assert_same_scene(host, dev, what):
    ih, idv = host.info, dev.info
    assert ih["device_build"] == 0 and idv["device_build"] == 1, what
    for k in ("num_nodes", "num_leaves", "num_slots", "max_depth", "max_leaf_size", "bounds_lo", "bounds_hi",
              "quantised_nodes"):
        assert ih[k] == idv[k], (what, k, ih[k], idv[k])
    assert abs(ih["leaf_inflation"] - idv["leaf_inflation"]) < 1e-6, what
    for a in ("nodes", "tris", "slot_prim", "slot_label", "prim_plane", "nodes_q", "nodes_n"):
        x, y = host.export_array(a), dev.export_array(a)
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: array {a} differs"


def test_device_build_equals_host_build(ctx):
    """The scene build on the GPU (csrc/lrc_bvh_device.hip) against the host builder (csrc/bvh_build.cpp): the same tree
    and the same bytes in every array the trace kernels read -- nodes, triangle records, ids, labels, plane table and both
    quantised images -- for rooms and soups around every size-class boundary of the device builder (one wave <= 64, one
    workgroup <= 1024, chunked above), all leaf sizes, layout heads that cut a level in the middle, depth caps that
    force median splits near the root, the median-only hook (the radix-sort path of big nodes), snapped coordinates with
    signed zeros, and a mesh no SAH plane can split."""
    from lidarcast import synth
    from lidarcast.synth import TriangleMesh
    room = synth.make_room(size=(3.0, 2.5, 2.0), num_boxes=3, seed=9, cell=0.05)
    _assert_same_scene(*_build_both(ctx, room), "room")
    for ml in (1, 2, 3):
        _assert_same_scene(*_build_both(ctx, room, LRC_MAX_LEAF=ml), f"room max_leaf={ml}")
    for bfs in (1, 2, 7, 100, 10 ** 6):
        _assert_same_scene(*_build_both(ctx, room, LRC_BFS_NODES=bfs), f"room bfs_nodes={bfs}")
    for sl in (0, 1, 5, -1):
        _assert_same_scene(*_build_both(ctx, room, LRC_DEPTH_SLACK=sl), f"room depth_slack={sl}")
    _assert_same_scene(*_build_both(ctx, room, LRC_BUILD_MEDIAN_ONLY=1), "room, median splits only")
    rng = np.random.default_rng(3)
    for nt in (5, 6, 9, 64, 65, 66, 200, 1024, 1025, 1030, 3000, 20000):
        v, f = random_soup(nt, seed=nt)
        m = TriangleMesh(v, f)
        _assert_same_scene(*_build_both(ctx, m), f"soup {nt}")
        _assert_same_scene(*_build_both(ctx, m, LRC_BUILD_MEDIAN_ONLY=1), f"soup {nt}, median splits only")
    nt = 5000
    v = np.round(rng.uniform(-2, 2, (nt, 3, 3)) * 2) / 2
    v[v == 0] = rng.choice([0.0, -0.0], size=int((v == 0).sum()))
    snapped = TriangleMesh(v.reshape(-1, 3), np.arange(3 * nt).reshape(-1, 3))
    _assert_same_scene(*_build_both(ctx, snapped), "snapped soup")
    same = TriangleMesh(np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float64), (3000, 1)),
                        np.arange(9000).reshape(-1, 3))
    _assert_same_scene(*_build_both(ctx, same), "3000 coincident triangles")
    # errors come back as the host builder reports them
    import lidarcast
    with pytest.raises(ValueError, match="out of range"):
        lidarcast.Scene(ctx, room.vertices, np.concatenate([room.triangles, [[0, 1, len(room.vertices)]]]))
    bad = np.array(room.vertices, dtype=np.float64)
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        lidarcast.Scene(ctx, bad, room.triangles)


def test_device_build_equals_host_build_on_random_meshes(ctx):
    """The same comparison on 32 seeded random meshes whose shapes stress the builder differently: uniform soups, one
    dense cluster with a few far outliers (bins nearly empty, median fallbacks), grid-aligned quads (many equal centroids,
    equal costs: the first-minimum rule decides), long slivers (boxes that overlap along one axis), each with a random
    size, leaf size and depth slack."""
    from lidarcast.synth import TriangleMesh
    for seed in range(32):
        rng = np.random.default_rng(1000 + seed)
        nt = int(rng.choice([rng.integers(5, 70), rng.integers(60, 1100), rng.integers(1000, 6000)]))
        style = seed % 4
        if style == 0:
            c = rng.uniform(-3, 3, (nt, 1, 3))
            tri = c + rng.normal(scale=0.3, size=(nt, 3, 3))
        elif style == 1:
            c = rng.normal(scale=0.01, size=(nt, 1, 3))
            far = rng.random(nt) < 0.02
            c[far] += rng.uniform(-50, 50, (int(far.sum()), 1, 3))
            tri = c + rng.normal(scale=0.002, size=(nt, 3, 3))
        elif style == 2:
            g = int(np.ceil(np.sqrt(nt / 2)))
            ij = np.stack(np.meshgrid(np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 2)[: (nt + 1) // 2]
            a = np.concatenate([ij * 0.25, np.zeros((len(ij), 1))], 1)
            q = np.stack([a, a + [0.25, 0, 0], a + [0.25, 0.25, 0], a, a + [0.25, 0.25, 0], a + [0, 0.25, 0]], 1).reshape(-1, 3, 3)
            tri = q[:nt]
        else:
            c = rng.uniform(-2, 2, (nt, 1, 3))
            d = rng.normal(size=(nt, 1, 3)) * rng.uniform(0.5, 4.0, (nt, 1, 1))
            tri = c + np.concatenate([np.zeros((nt, 1, 3)), d, d + rng.normal(scale=0.01, size=(nt, 1, 3))], 1)
        mesh = TriangleMesh(np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 3), np.arange(3 * len(tri)).reshape(-1, 3))
        env = {"LRC_MAX_LEAF": int(rng.integers(1, 5)), "LRC_DEPTH_SLACK": int(rng.integers(0, 3))}
        _assert_same_scene(*_build_both(ctx, mesh, **env), f"random mesh {seed}: style {style}, T={len(tri)}, {env}")


def test_device_build_full_size_and_device_resident_mesh(ctx):
    """BASELINE-size scenes: device build == host build byte for byte; a mesh handed over in HBM (lrc_scene_create_dev)
    gives the same scene again; the build stays inside its time budget (T = 605 k resident in <= 10 ms)."""
    import time
    import torch
    import lidarcast
    from lidarcast import synth
    for name in ("synth_A6_office2", "synth_rough_A6"):
        mesh = synth.make_scene(name)
        host, dev = _build_both(ctx, mesh)
        _assert_same_scene(host, dev, name)
        d = torch.device("cuda", 0)
        v = torch.from_numpy(np.ascontiguousarray(mesh.vertices, dtype=np.float32)).to(d)
        f = torch.from_numpy(np.ascontiguousarray(mesh.triangles, dtype=np.int32)).to(d)
        sem = torch.from_numpy(mesh.triangle_sem.astype(np.int16)).to(d)
        ins = torch.from_numpy(mesh.triangle_ins.astype(np.int16)).to(d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident = lidarcast.Scene.from_device(ctx, v, f, sem, ins)
        ms_resident = (time.perf_counter() - t0) * 1e3
        for a in ("nodes", "tris", "slot_prim", "slot_label", "prim_plane", "nodes_q", "nodes_n"):
            assert np.array_equal(resident.export_array(a), host.export_array(a)), (name, a)
        t0 = time.perf_counter()
        again = lidarcast.Scene(ctx, mesh.vertices.astype(np.float32), mesh.triangles.astype(np.uint32),
                                mesh.triangle_sem, mesh.triangle_ins)
        ms_host_mesh = (time.perf_counter() - t0) * 1e3
        info = again.info
        print(f"{name}: T={info['num_triangles']} host builder {host.info['build_ms']:.1f} ms | device builder: mesh in "
              f"host memory {ms_host_mesh:.2f} ms (transfer {info['upload_ms']:.2f} + build {info['build_ms']:.2f}), "
              f"mesh in HBM {ms_resident:.2f} ms")
        assert ms_host_mesh < 10.0 and ms_resident < 10.0, (ms_host_mesh, ms_resident)


def test_export_labels_from_annotation_files(tmp_path, engine):
    """The whole label path from files on disk, as the reference wires it: S3DISSimScene(s3dis_data_root, area, room)
    -> s3dis_annotation_loader (Annotations/<class>_<k>.txt) -> raw coloured cloud <room>.txt -> nearest annotated point
    per hit point -> labelled PLY.  Checked against the same steps done with numpy + sklearn."""
    from sklearn.neighbors import NearestNeighbors
    from containers import S3DISSimFrame, S3DISSimScene, ScanQuality, read_labeled_ply
    from lidarcast import synth
    from s3dis_annotation_loader import S3DISAnnotationLoader
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=2, seed=3, cell=0.08)
    rng = np.random.default_rng(1)
    room = tmp_path / "data" / "Area_7" / "office_3"
    (room / "Annotations").mkdir(parents=True)
    raw = []
    for name, n in (("wall_1", 4000), ("floor_1", 2500), ("chair_1", 800), ("table_1", 900), ("ceiling_1", 2000)):
        tri = mesh.triangles[rng.integers(0, len(mesh.triangles), n)]
        w = rng.dirichlet([1, 1, 1], n)
        pts = (mesh.vertices[tri] * w[:, :, None]).sum(1)
        rgb = rng.integers(0, 256, (n, 3))
        np.savetxt(room / "Annotations" / f"{name}.txt", np.hstack([pts, rgb]), fmt="%.6f %.6f %.6f %d %d %d")
        raw.append(np.hstack([pts, rgb]))
    np.savetxt(room / "office_3.txt", np.vstack(raw), fmt="%.6f %.6f %.6f %d %d %d")
    k = sensor_small(lines=6, width=128, max_range=20.0)
    rec, _ = engine.scan_poses(k, np.stack([pose(1.5, 1.5, 1.0), pose(2.5, 1.5, 1.2)]), mesh, want=("t", "point3"))
    sc = S3DISSimScene("office_3", s3dis_data_root=str(tmp_path / "data"), area="Area_7", room="office_3")
    q = ScanQuality(0, 0, 0, 0, 0, 0, 0)
    for i in range(2):
        pts = rec["point3"][i][np.isfinite(rec["t"][i])]
        sc.append_frame(S3DISSimFrame(i, pts, np.zeros(len(pts)), q))
    sc._export_combined_pointcloud_with_labels(tmp_path)
    out = read_labeled_ply(tmp_path / "combined_pointcloud_with_label.ply")
    # the same with the loader + sklearn
    loader = S3DISAnnotationLoader(str(tmp_path / "data"))
    ap, al, ai = loader.create_labeled_pointcloud_with_instances(loader.load_room_annotations("Area_7", "office_3"))
    assert len(ap) == 10200 and set(np.unique(al)) == {0, 1, 2, 7, 8}
    rawd = np.loadtxt(room / "office_3.txt")
    col = rawd[NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(rawd[:, :3]).kneighbors(ap)[1][:, 0], 3:6] / 255.0
    allp = sc.combined_points()
    j = NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(ap).kneighbors(allp)[1][:, 0]
    assert len(out) == len(allp) > 500
    assert np.array_equal(out["sem"], al[j].astype(np.uint16)) and np.array_equal(out["ins"], ai[j].astype(np.uint16))
    assert np.array_equal(np.stack([out["red"], out["green"], out["blue"]], 1), (col[j] * 255).astype(np.uint8))



def test_scan_pipeline_equals_scan_plus_compaction(ctx):
    """lrc_pipe_*: batches submitted back to back (trace launches alternating between two internal streams, the rows of
    submit k scattered by the leading workgroups of the trace launch of submit k+2, four rotating record sets) against the
    same batches through lrc_scan_poses_dev + lrc_compact_dev on one stream: rows, per-pose counts and the fixed-stride
    records, bit for bit -- ragged batch sizes, every output kind, a flush in the middle, and the fallback for tables whose
    tiles do not line up.  Poses are independent (reference: s3dis_simulator.py:254-288), so the order of execution is free."""
    import ctypes as C
    import torch
    import lidarcast
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    from lidar import IndoorLidar
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    for lines, width, max_range, pmax in ((8, 512, 2.5, 9), (4, 256, 20.0, 33), (3, 100, 20.0, 6)):
        k = sensor_small(lines=lines, width=width, max_range=max_range)
        dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
        N = len(dirs)
        d_dirs = torch.from_numpy(dirs).to(dev)
        pipe = lidarcast.ScanPipe(scene, pmax, N)
        hits = lidarcast.DeviceHits(pmax * N, dev, want=("t", "prim", "normal3", "point3", "sem", "ins", "tile_count"))
        batches, outs = [], []
        sizes = [pmax, 1, pmax - 2, 3, pmax, 2, pmax - 1, pmax]
        for b, P in enumerate(sizes):
            poses = np.stack([pose(0.6 + 2.8 * rng.random(), 0.6 + 1.8 * rng.random(), 0.5 + 1.5 * rng.random(),
                                   yaw=rng.uniform(-3, 3)) for _ in range(P)])
            d_poses = torch.from_numpy(poses.reshape(P, 16)).to(dev)
            rows = torch.full((P * N, 4), -7.0, dtype=torch.float32, device=dev)
            counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
            io = LrcCompactIO()
            io.counts = counts.data_ptr()
            extra = {}
            if b % 3 == 1:            # every output kind: the per-tile form of the leading workgroups
                extra = {"p3": torch.zeros((P * N, 3), dtype=torch.float32, device=dev),
                         "sem": torch.zeros(P * N, dtype=torch.int16, device=dev),
                         "ins": torch.zeros(P * N, dtype=torch.int16, device=dev),
                         "idx": torch.zeros(P * N, dtype=torch.int32, device=dev),
                         "rng": torch.zeros(P * N, dtype=torch.float32, device=dev)}
                io.out_point3, io.out_sem, io.out_ins = extra["p3"].data_ptr(), extra["sem"].data_ptr(), extra["ins"].data_ptr()
                io.out_index, io.out_range_origin = extra["idx"].data_ptr(), extra["rng"].data_ptr()
                if b % 2:
                    io.out_xyzl = rows.data_ptr()
            else:
                io.out_xyzl = rows.data_ptr()
            ticket = pipe.submit(d_poses, d_dirs, k.max_range, io=io, stream=st)
            batches.append((d_poses, P, ticket))
            outs.append((rows, counts, extra, io))
            if b == 4:                # a flush in the middle: everything so far is complete, the pipeline starts afresh
                pipe.wait(st)
                torch.cuda.synchronize()
                assert all(int(o[1].min().item()) >= 0 for o in outs)
        pipe.wait(st)
        torch.cuda.synchronize()
        # the records of the last submits are still there (four sets rotate)
        for (d_poses, P, ticket), (rows, counts, extra, io) in zip(batches, outs):
            rows2 = torch.full_like(rows, -7.0)
            counts2 = torch.full_like(counts, -1)
            io2 = LrcCompactIO()
            io2.t, io2.point3, io2.sem, io2.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
            io2.tile_count, io2.counts, io2.out_xyzl = hits["tile_count"].data_ptr(), counts2.data_ptr(), rows2.data_ptr()
            extra2 = {n_: torch.zeros_like(t_) for n_, t_ in extra.items()}
            if extra:
                io2.out_point3, io2.out_sem, io2.out_ins = extra2["p3"].data_ptr(), extra2["sem"].data_ptr(), extra2["ins"].data_ptr()
                io2.out_index, io2.out_range_origin = extra2["idx"].data_ptr(), extra2["rng"].data_ptr()
            scene.scan_poses_dev(d_poses, d_dirs, hits, k.max_range, st)
            ctx.compact_dev(P, N, io2, st)
            torch.cuda.synchronize()
            assert torch.equal(counts, counts2), f"per-pose counts differ, batch of {P} poses"
            kk = int(counts2.sum().item())
            if io.out_xyzl:
                assert torch.equal(rows[:kk].view(torch.int32), rows2[:kk].view(torch.int32)), "rows differ"
                assert bool((rows[kk:] == -7.0).all()), "rows beyond the kept ones were touched"
            for n_ in extra:
                a, b2 = extra[n_][:kk], extra2[n_][:kk]
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b2.view(torch.int32) if b2.dtype == torch.float32 else b2), n_
            if pipe_ticket_alive(pipe, ticket):
                rec = pipe.records(ticket)
                for name, width_ in (("t", 4), ("prim", 4), ("normal3", 12), ("point3", 12), ("sem", 2), ("ins", 2)):
                    nbytes = P * N * width_
                    got = (C.c_char * nbytes).from_buffer_copy(_dev_bytes(getattr(rec, name), nbytes))
                    ref = hits[name].view(torch.uint8).flatten()[:nbytes].cpu().numpy().tobytes()
                    assert bytes(got) == ref, f"records differ: {name}"
        pipe.close()


def pipe_ticket_alive(pipe, ticket):
    try:
        pipe.records(ticket)
        return True
    except ValueError:
        return False


def _dev_bytes(ptr, nbytes):
    """nbytes at device address ptr as host bytes (through a torch byte tensor filled by hipMemcpy)."""
    import ctypes as C
    import torch
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(int(ptr)), nbytes, 3) == 0      # device to device
    return buf.cpu().numpy().tobytes()


def test_sharded_scan_pipeline_assembles_the_scene_cloud(ctx):
    """The N-rank form of the pipeline (lrc_pipe_submit_sharded / trace_done / scan_gathered / assemble), three ranks
    emulated on one GPU: this rank (the MIDDLE slab, so that rows land before and after its own) traces its pose block with
    ids and keep counts written into its send slab; the "collective" -- here a copy of that slab plus scans of the other
    ranks' poses into their slabs, on a communication stream behind lrc_pipe_trace_done -- is followed by the scan over the
    gathered counts; the assembly of step s rides in the leading workgroups of the trace launch of step s+2, the last two
    steps go through lrc_pipe_assemble.  Every step has its own poses; every step's cloud and per-pose counts must equal
    the local scan + compaction of all ranks' poses of that step, bit for bit (np.vstack order, reference:
    containers/s3dis_sim_scene.py:326)."""
    import torch
    import lidarcast
    from lidarcast import synth
    from lidarcast._capi import LrcCompactIO
    from lidarcast.distributed import PrimGather
    from lidar import IndoorLidar

    class OneRank:                     # PrimGather only asks the process group for its size when sizing the receive view
        @staticmethod
        def get_world_size(group=None):
            return 1

    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04)
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    dev = torch.device("cuda", 0)
    main = torch.cuda.current_stream()
    comm = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(11)
    W, own = 3, 1
    for lines, width, max_range, P, steps in ((8, 512, 2.5, 5, 7), (4, 256, 20.0, 19, 5), (16, 1024, 3.0, 3, 4)):
        k = sensor_small(lines=lines, width=width, max_range=max_range)
        dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
        N = len(dirs)
        d_dirs = torch.from_numpy(dirs).to(dev)
        pipe = lidarcast.ScanPipe(scene, P, N)
        gathers = [PrimGather(P, N, OneRank, dev, world=W) for _ in range(2)]
        tl = lidarcast.DeviceHits(0, dev, want=())
        all_poses, clouds, cnts, tickets, scanned = [], [], [], [0, 0], [None, None]

        def job_of(kk, s):
            g = gathers[kk]
            return lidarcast.ScanPipe.gathered(all_poses[s], g.all_prims, g.all_tile_counts, P, g.stride_bytes, own,
                                               tickets[kk], clouds[s], cnts[s], scan_slot=kk)

        for s in range(steps):
            poses = np.stack([pose(0.6 + 2.8 * rng.random(), 0.6 + 1.8 * rng.random(), 0.5 + 1.5 * rng.random(),
                                   yaw=rng.uniform(-3, 3)) for _ in range(W * P)])
            all_poses.append(torch.from_numpy(poses.reshape(W * P, 16)).to(dev))
            clouds.append(torch.full((W * P * N, 4), -7.0, dtype=torch.float32, device=dev))
            cnts.append(torch.full((W * P,), -1, dtype=torch.int64, device=dev))
            kk = s % 2
            g = gathers[kk]
            asm = None
            if scanned[kk] is not None:
                main.wait_event(scanned[kk])
                asm = job_of(kk, s - 2)
            tickets[kk] = pipe.submit_sharded(all_poses[s][own * P:(own + 1) * P], d_dirs, k.max_range, g.prim, g.tile_count,
                                              assemble=asm, stream=main.cuda_stream)
            pipe.trace_done(tickets[kk], comm.cuda_stream)
            with torch.cuda.stream(comm):
                g.all_slabs[own * g.words:(own + 1) * g.words].copy_(g.slab)
                for v in range(W):
                    if v != own:
                        tl.struct.prim = g.all_slabs[v * g.words:].data_ptr()
                        tl.struct.tile_count = g.all_slabs[v * g.words + g.n:].data_ptr()
                        scene.scan_poses_dev(all_poses[s][v * P:(v + 1) * P], d_dirs, tl, k.max_range, comm.cuda_stream)
                pipe.scan_gathered(d_dirs, job_of(kk, s), comm.cuda_stream)
                ev = torch.cuda.Event()
                ev.record(comm)
            scanned[kk] = ev
        for s in (steps - 2, steps - 1):
            kk = s % 2
            main.wait_event(scanned[kk])
            pipe.assemble(d_dirs, job_of(kk, s), main.cuda_stream)
        pipe.wait(main.cuda_stream)
        torch.cuda.synchronize()
        hits = lidarcast.DeviceHits(W * P * N, dev, want=("t", "point3", "sem", "ins", "tile_count"))
        for s in range(steps):
            rows2 = torch.full_like(clouds[s], -7.0)
            counts2 = torch.full_like(cnts[s], -1)
            io2 = LrcCompactIO()
            io2.t, io2.point3, io2.sem, io2.ins = (hits[a].data_ptr() for a in ("t", "point3", "sem", "ins"))
            io2.tile_count, io2.counts, io2.out_xyzl = hits["tile_count"].data_ptr(), counts2.data_ptr(), rows2.data_ptr()
            scene.scan_poses_dev(all_poses[s], d_dirs, hits, k.max_range, main.cuda_stream)
            ctx.compact_dev(W * P, N, io2, main.cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(cnts[s], counts2), f"per-pose counts differ, step {s}"
            kept = int(counts2.sum().item())
            assert 0 < kept and (kept < W * P * N or max_range > 10)
            assert torch.equal(clouds[s][:kept].view(torch.int32), rows2[:kept].view(torch.int32)), f"rows differ, step {s}"
            assert bool((clouds[s][kept:] == -7.0).all()), "rows beyond the kept ones were touched"
        # argument checks: an assembly whose own records have rotated away, a slab outside the gathered ones
        stale = job_of(0, 0)
        stale.own_ticket = 1
        if steps > 4:
            with pytest.raises(ValueError):
                pipe.assemble(d_dirs, stale, main.cuda_stream)
        outside = job_of(0, steps - 2 if (steps - 2) % 2 == 0 else steps - 1)
        outside.own_slab = W
        with pytest.raises(ValueError):
            pipe.assemble(d_dirs, outside, main.cuda_stream)
        pipe.close()
