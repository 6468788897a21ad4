"""-m gpu: the BASELINE configurations at their stated sizes (C3 witness, C4, C5), the frame-producing entry points
of the plugin surface (lrc_scan_poses_compact, lrc_scan_angles_compact), the diagnostics (box-clause counter,
float64 witness) and the rank-aware simulator, all through the C ABI.

Oracle legs compare bit for bit with oracle/ (CPU restatement); the float64 witness (oracle/lrc_oracle.c,
orc_witness_f64) is an independent double-precision statement of the closest hit that bounds what the float32
definition can differ from exact geometry -- the honest parity statement against
/root/reference/raycast_engine/raycast_engine_cpu.py:51, whose Embree arithmetic cannot run here."""
import hashlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from helpers import assert_bit_equal, pose, sensor_32x2048, sensor_8x512, sensor_small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def _line_poses(name, n):
    from lidarcast import synth
    from trajectory import line_trajectory, poses_from_waypoints
    Lx, Ly, _ = synth.scene_size(name)
    return poses_from_waypoints(line_trajectory((1.0, Ly / 2, 1.0), (Lx - 1.0, Ly / 2, 1.0), n))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- plugin surface: scan straight to frames -------------------------------------------------------------------
def test_scan_frames_equals_fixed_stride_records(engine):
    """lrc_scan_poses_compact (scan + compaction in HBM, kept rows into page-locked buffers) == the fixed-stride
    records of lrc_scan_poses masked on the host, attribute by attribute, incl. ragged widths and the world-origin
    range column; the pinned pages are recycled once the caller drops the frames."""
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    for k in (sensor_small(lines=5, width=200, max_range=2.2), sensor_small(lines=4, width=128, max_range=30.0)):
        poses = np.stack([pose(0.8 + 0.5 * i, 1.4, 1.0, 0.3 * i) for i in range(5)])
        rec, n = engine.scan_poses(k, poses, mesh, want=("t", "point3", "incident_deg", "sem", "ins"))
        fr = engine.scan_frames(k, poses, mesh, want=("point3", "sem", "ins", "incident_deg", "index", "xyzl",
                                                      "range_origin"))
        keep = np.isfinite(rec["t"])
        assert np.array_equal(fr["counts"], keep.sum(1)) and fr["total"] == keep.sum() > 100
        assert 0 < keep.mean() < 1 or k.max_range > 10
        assert_bit_equal(fr["point3"], rec["point3"][keep])
        assert_bit_equal(fr["incident_deg"], rec["incident_deg"][keep])
        assert np.array_equal(fr["sem"], rec["sem"][keep]) and np.array_equal(fr["ins"], rec["ins"][keep])
        assert np.array_equal(fr["index"], np.concatenate([np.flatnonzero(m) for m in keep]))
        assert_bit_equal(fr["xyzl"][:, :3].copy(), rec["point3"][keep])
        lab = fr["xyzl"][:, 3].copy().view(np.uint32)
        assert np.array_equal(lab, rec["sem"][keep].astype(np.uint32) | (rec["ins"][keep].astype(np.uint32) << 16))
        assert_bit_equal(fr["range_origin"], np.linalg.norm(rec["point3"][keep], axis=1))
        views = engine.split_frames(fr, "point3")
        assert len(views) == 5 and all(np.shares_memory(v, fr["point3"]) or len(v) == 0 for v in views)
        assert_bit_equal(views[3], rec["point3"][3][keep[3]])
    # page-locked buffers (arrays of >= 4 MB): a second scan after the first result was dropped allocates nothing new
    scene = engine.scene_for(mesh)
    big = sensor_32x2048()
    dirs = engine._direction_table(big)
    poses = np.stack([pose(0.8 + 0.4 * i, 1.4, 1.0, 0.3 * i) for i in range(6)])
    k = big
    a = scene.scan_poses_compact(poses, dirs, k.max_range)
    before = engine.ctx.pinned.allocations
    assert before >= 1 and a["point3"].nbytes >= 4 << 20
    del a, fr, views
    b = scene.scan_poses_compact(poses, dirs, k.max_range)
    assert engine.ctx.pinned.allocations == before
    # a result the caller still holds is never overwritten by the next scan
    snap = b["point3"].copy()
    c = scene.scan_poses_compact(poses[::-1].copy(), dirs, k.max_range)
    assert_bit_equal(b["point3"], snap) and c["total"] == b["total"]
    # too small a buffer: an error that names the size needed, nothing written past the buffer
    with pytest.raises(ValueError, match="capacity"):
        scene.scan_poses_compact(poses, dirs, k.max_range, capacity=10)
    # no poses / no rays
    assert scene.scan_poses_compact(np.zeros((0, 4, 4)), dirs, 5.0)["total"] == 0


def test_nonfinite_rays_are_misses(engine):
    """Finite-ray contract of the C ABI: a NaN / infinite component makes the ray a miss, like the oracle."""
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    cube = synth.unit_cube()
    rays = np.random.default_rng(3).normal(size=(256, 6)).astype(np.float32)
    rays[:, :3] *= 0.2
    rays[::4, 0] = np.nan
    rays[1::4, 4] = np.inf
    rays[2::4, 5] = -np.inf
    out = engine.cast_rays(rays, cube)
    t, prim = OracleMesh(cube.vertices, cube.triangles).cast(rays)
    sick = ~np.isfinite(rays).all(1)
    assert sick.sum() == 192 and np.isinf(out["t_hit"][sick]).all() and (out["primitive_ids"][sick] == 0xFFFFFFFF).all()
    assert not out["points"][sick].any() and np.isfinite(out["t_hit"][~sick]).all()
    assert_bit_equal(out["t_hit"], t)
    assert_bit_equal(out["primitive_ids"], prim)


# ---- the hit definition against an independent witness -------------------------------------------------------
def test_c3_rays_against_the_float64_witness(engine):
    """>= 10^5 rays of the C3 workload: the HIP float32 result against double-precision Moeller-Trumbore over the
    whole mesh.  Asserts the north-star tolerance |t32 - t64| <= 1e-5 m on every ray, the same triangle except on a
    shared edge, and counts the rays on which float32 and exact geometry disagree about hit / miss (edge leaks)."""
    import bench
    from lidar import create_lidar
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_scene(bench.SCENE)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)[[0, 31, 63]]
    rec, n = engine.scan_poses(sensor, poses, mesh, want=("t", "prim"))
    t32, p32 = rec["t"].reshape(-1), rec["prim"].reshape(-1)
    rays = np.concatenate([create_lidar(sensor, m).get_rays() for m in poses])
    assert len(rays) == 196608
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    t64, p64, m64 = om.witness(rays, threads=16)
    h32, h64 = np.isfinite(t32), np.isfinite(t64)       # max_range 25 m never cuts in this 5 m room
    leaks_in, leaks_out = int((h64 & ~h32).sum()), int((h32 & ~h64).sum())
    both = h32 & h64
    dt = np.abs(t32[both].astype(np.float64) - t64[both])
    other = both & (p32 != p64)
    print(f"\n[witness] rays {len(rays)}: both hit {int(both.sum())}, both miss {int((~h32 & ~h64).sum())} (seams of the "
          f"synthetic room), f64-hit/f32-miss {leaks_in}, f32-hit/f64-miss {leaks_out}, other triangle {int(other.sum())}, "
          f"max |dt| {dt.max():.3e} m, p99.9 {np.percentile(dt, 99.9):.3e} m, mean {dt.mean():.3e} m")
    assert dt.max() <= 1e-5
    assert leaks_in + leaks_out <= 4                    # measured: 0
    assert (m64[other] < 1e-4).all() and other.sum() <= 20
    # the misses of this closed room are gaps of the mesh, not of the arithmetic: exact geometry misses too
    assert ((~h32) == (~h64)).all() or leaks_in + leaks_out > 0


def test_other_configs_against_the_float64_witness(engine):
    """The same witness comparison on the other kinds of input the BASELINE configs feed the cast: C1/C2 (8 x 512 in
    synth_A1_office), C4 (BLK2GO rays with angle noise, explicit-ray kernel), the rough welded scene, and a yawed,
    pitched sensor close to a wall.  Same bars: |t32 - t64| <= 1e-5 m, hit/miss and triangle agree (edge cases counted)."""
    import bench
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    a1 = synth.make_scene("synth_A1_office")
    rough = synth.make_scene("synth_rough_A6")
    tilt = np.eye(4)
    tilt[:3, :3] = _rot(0.9, 0.35, -0.2)
    tilt[:3, 3] = (0.12, 2.0, 1.4)
    np.random.seed(0)
    cases = {
        "C1/C2 8x512, A1": (a1, create_lidar(sensor_8x512(), pose(4.0, 3.0, 1.0)).get_rays()),
        "C4 BLK2GO, A1": (a1, create_lidar(DualAxisLidarIntrinsics.create_blk2go_dual_axis(), pose(2.0, 3.0, 1.0, 0.4)).get_rays()),
        "C3 sensor, rough A6": (rough, np.concatenate([create_lidar(bench.c3_sensor(), m).get_rays()
                                                       for m in bench.c3_poses(0, 1)[[7, 50]]])),
        "C3 sensor tilted 12 cm from a wall, A6": (None, create_lidar(bench.c3_sensor(), tilt).get_rays()),
    }
    a6 = synth.make_scene(bench.SCENE)
    total = worst = 0
    for name, (mesh, rays) in cases.items():
        mesh = a6 if mesh is None else mesh
        out = engine.cast_rays(rays, mesh, want=("t", "prim"))
        t32, p32 = out["t_hit"], out["primitive_ids"]
        t64, p64, m64 = OracleMesh(mesh.vertices, mesh.triangles).witness(rays, threads=16)
        h32, h64 = np.isfinite(t32), np.isfinite(t64)
        both = h32 & h64
        dt = np.abs(t32[both].astype(np.float64) - t64[both])
        other = both & (p32 != p64)
        print(f"\n[witness] {name}: rays {len(rays)}, both hit {int(both.sum())}, hit/miss disagreements "
              f"{int((h32 != h64).sum())}, other triangle {int(other.sum())}, max |dt| {dt.max():.3e} m")
        assert dt.max() <= 1e-5 and (h32 != h64).sum() <= 2 and (m64[other] < 1e-4).all() and other.sum() <= 10
        total += len(rays)
        worst = max(worst, dt.max())
    assert total > 250000


def test_box_clause_never_acts_on_the_baseline_configs(engine):
    """The hit definition's one clause Embree does not have (t inside the padded slab interval of the triangle's own
    box) rejects nothing on C1/C2, C3 and the C5 scenes: instrumented trace kernel, counter [4] of
    lrc_debug_scan_stats; C4's explicit rays through the oracle's counter."""
    import bench
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    total = {}
    a1 = synth.make_scene("synth_A1_office")
    sc = engine.scene_for(a1)
    k8 = sensor_8x512()
    st = sc.scan_stats(pose(4.0, 3.0, 1.0)[None], engine._direction_table(k8), k8.max_range)
    total["C1/C2"] = int(st[:, 4].sum())
    assert st[:, 0].mean() > 10 and st[:, 1].mean() > 1          # the counters count
    np.random.seed(0)
    rays = create_lidar(DualAxisLidarIntrinsics.create_blk2go_dual_axis(), pose(2.0, 3.0, 1.0)).get_rays()
    total["C4"] = int(OracleMesh(a1.vertices, a1.triangles).cast_diag(rays, threads=16)[2].sum())
    sensor = bench.c3_sensor()
    dirs = engine._direction_table(sensor)
    for name in synth.SCENES:
        mesh = a1 if name == "synth_A1_office" else synth.make_scene(name)
        sc = engine.scene_for(mesh)
        st = sc.scan_stats(_line_poses(name, 64)[::21], dirs, sensor.max_range)
        total[name] = int(st[:, 4].sum())
        if name == bench.SCENE:
            uni = st[:, 2].sum() / st[:, 0].sum()
            assert 0.3 < uni < 0.6                               # share of node steps on the scalar path
    print("\n[box clause] rejections:", total)
    assert all(v == 0 for v in total.values()), total


# ---- C5: six scenes ------------------------------------------------------------------------------------------
def test_c5_six_scenes_full_size(engine):
    """BASELINE config C5: the C3 sensor x 64 poses over synth_A1..A6 through the plugin surface
    (S3DISSimulator.run_simulation -> lrc_scan_poses_compact).  Every ray of every scene through size-independent
    properties; all 64 frames of every scene ray by ray against the oracle; per-scene Chamfer distance (definition of
    evaluate_single_scene.py:81-96, evaluated on the full clouds of poses 5 and 58 with lrc_min_distances) between the
    HIP cloud and the oracle cloud == 0.0."""
    import bench
    import full_parity as fp
    from lidarcast import synth
    from lidarcast.metrics import min_distances
    from oracle.c_oracle import OracleMesh
    from s3dis_simulator import run_scene_batch
    sensor = bench.c3_sensor()
    names = list(synth.SCENES)
    meshes = {n: synth.make_scene(n) for n in names}
    checked = []

    def check_scene(name, sim):
        # called per scene, which is then released (as the reference's batch loop keeps no scene): the next scene's frames
        # reuse its page-locked buffers
        mesh = meshes[name]
        poses = _line_poses(name, 64)
        assert len(sim.frames) == 64
        counts = np.array([len(f.points) for f in sim.frames])
        assert counts.min() > 0.99 * 65536 and counts.max() <= 65536
        cloud = sim.combined_points()
        lo, hi = mesh.vertices.min(0) - 1e-3, mesh.vertices.max(0) + 1e-3
        assert cloud.dtype == np.float32 and len(cloud) == counts.sum()
        assert (cloud >= lo).all() and (cloud <= hi).all()                      # every return lies in the room
        sem = np.concatenate([f.semantic_labels for f in sim.frames])
        assert set(np.unique(sem)) <= {0, 1, 2, 7, 8, 10} and (sem == 2).mean() > 0.2
        om = OracleMesh(mesh.vertices, mesh.triangles).build()
        # all 64 frames against the oracle (tests/full_parity.py): per-frame sizes, points, semantic and instance labels
        want = fp.expected_sensor_scan(om, mesh, sensor, poses, threads=16)
        rows = np.empty((len(cloud), 4), np.float32)
        rows[:, :3] = cloud
        rows[:, 3] = fp.pack_labels(sem, np.concatenate([f.instance_labels for f in sim.frames]))
        n = fp.assert_scan_equal({"rows": rows, "counts": counts.astype(np.int64)}, want, f"C5 {name}", fields=fp.CLOUD)
        assert n == 64 * 65536 and want["keep"].mean() > 0.99
        fp.report(f"C5 {name}, all 64 frames", want, rays=n)
        expected = list(fp.frames(want))
        ref, mine = [], []
        for p in (5, 58):
            ridx, rp, rsem, _ = expected[p]
            assert_bit_equal(sim.frames[p].points, rp, f"{name} pose {p}")
            assert np.array_equal(sim.frames[p].semantic_labels, rsem) and len(ridx) == len(rp)
            ref.append(rp)
            mine.append(sim.frames[p].points)
        ref, mine = np.concatenate(ref), np.concatenate(mine)
        cd = float(np.mean(min_distances(mine, ref, engine.ctx)) + np.mean(min_distances(ref, mine, engine.ctx)))
        assert cd == 0.0, (name, cd)
        om.free()
        checked.append(name)

    report = run_scene_batch([(n, meshes[n]) for n in names], {n: _line_poses(n, 64) for n in names},
                             sensor=sensor, config={"raycast_engine": {"use_gpu": True}}, on_scene=check_scene)
    assert set(report["scenes"]) == set(names) and report["total_rays"] == 6 * 64 * 65536 and checked == names
    assert all(report["scenes"][n]["sim_scene"] is None and report["scenes"][n]["frames"] == 64 for n in names)
    print("\n[C5]", {k: v for k, v in report.items() if k != "scenes"})
    print("[C5] per scene, scan + build ms (the first scene's scan page-locks the frame buffers the others reuse):",
          " ".join(f"{n}:{v['seconds'] * 1e3:.1f}+{v['build_seconds'] * 1e3:.1f}" for n, v in report["scenes"].items()))
    # a guard that guards: round 3 measured 0.29-0.38 G rays/s including the builds (0.02 G with the round-2 host builder,
    # which this bound rejects); the check_scene callback's oracle work is outside both clocks
    assert report["rays_per_s_including_build"] > 2e8 and report["rays_per_s"] > 3e8, report


# ---- C4: BLK2GO, 256 poses -----------------------------------------------------------------------------------
def _c4_hash(points, sem, ins, counts):
    h = hashlib.sha256()
    for a in (points, sem, ins, counts):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_c4_blk2go_256_poses_and_two_rank_gather(engine, tmp_path):
    """BASELINE config C4 as stated: create_blk2go_dual_axis, np.random.seed(0) once, 256 poses on a line through
    synth_A1_office, ONE lrc_cast_segments launch per rank; all 256 poses ray by ray against the oracle; then the
    same job as a 2-rank launch (torch.distributed.run, gloo, both ranks on this one GPU) through
    S3DISSimulator.run_simulation: SHA-256 of the assembled scene equal to the 1-rank run's."""
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from lidarcast import synth
    from oracle import np_oracle
    from oracle.c_oracle import OracleMesh
    from s3dis_simulator import S3DISSimulator
    from trajectory import line_trajectory
    mesh = synth.make_scene("synth_A1_office")
    wps = line_trajectory((1.0, 3.0, 1.0), (7.0, 3.0, 1.0), 256)
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}}, use_blk2go=True)
    sim.raycast_engine = engine
    sim.load_scene(mesh, "synth_A1_office")
    np.random.seed(0)
    scene = sim.run_simulation(wps)
    launches, rays_cast = engine.scene_for(mesh).counters()
    counts = np.array([len(f.points) for f in scene.frames])
    assert len(scene.frames) == 256 and 0.97 * 64000 * 0.98 < counts.mean() < 64000
    one_rank = _c4_hash(scene.combined_points(), *scene.combined_labels(), counts)
    # the oracle on the same seeded stream, all 256 poses in stream order
    kd = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    np.random.seed(0)
    rays_compared = kept = 0
    for i, wp in enumerate(wps):
        lidar = create_lidar(kd, wp.to_pose_matrix())
        rays = lidar.get_rays()                                                  # draws this pose's rays

        class Frozen:
            intrinsics, pose = kd, lidar.pose
            def get_rays(self):
                return rays
        rp, _ = np_oracle.lidar_intersect_mesh(om, Frozen(), threads=16)
        assert_bit_equal(scene.frames[i].points, rp, f"pose {i}")
        rays_compared += len(rays)
        kept += len(rp)
    assert rays_compared > 256 * 64000 * 0.97 and kept == counts.sum()
    print(f"\n[full parity] C4 all 256 poses: rays compared {rays_compared}, kept share {kept / rays_compared:.5f}, "
          "rays that differ 0")
    # two ranks on the one GPU, launched the way the driver launches bench.py
    out = tmp_path / "c4.json"
    env = dict(os.environ, LRC_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(REPO, "tests", "configs", "run_simulation_ranks.py"), "c4", str(out)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(out.read_text())
    assert got["world"] == 2 and got["frames"] == 256
    assert got["sha256"] == [one_rank, one_rank], "the 2-rank scene differs from the 1-rank scene"


def test_run_simulation_two_ranks_multiline(engine, tmp_path):
    """The rank-aware plugin surface for the multi-line sensor: S3DISSimulator.run_simulation inside a 2-rank
    torch.distributed job (PrimGather: one all-gather of triangle ids, cloud rebuilt on every rank) returns on EVERY
    rank the scene a single process returns: points, labels and frame sizes hash-identical (13 poses: ragged blocks)."""
    from lidarcast import synth
    from s3dis_simulator import S3DISSimulator
    from trajectory import line_trajectory
    mesh = synth.make_room(size=(5, 4, 3), num_boxes=6, seed=6, cell=0.04)
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}}, use_dense_lidar=True)
    sim.raycast_engine = engine
    sim.load_scene(mesh, "room")
    scene = sim.run_simulation(line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 13, yaw=0.4))
    counts = np.array([len(f.points) for f in scene.frames])
    want = _c4_hash(scene.combined_points(), *scene.combined_labels(), counts)
    out = tmp_path / "ml.json"
    env = dict(os.environ, LRC_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(REPO, "tests", "configs", "run_simulation_ranks.py"), "multiline", str(out)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(out.read_text())
    assert got["world"] == 2 and got["frames"] == 13 and got["sha256"] == [want, want]
    assert got["quality"] == [[f.scan_quality.num_points, float(f.scan_quality.range_mean)] for f in scene.frames][:3]


# ---- dual-axis rays generated on the device (opt-in) ------------------------------------------------------------
def test_dual_axis_device_generation(engine):
    """lrc_scan_angles_compact: scan angles drawn on the host from the seeded stream, trigonometry + rotation in the
    kernel.  Reports how many float32 directions differ from the host generator's and the largest range difference
    on rays both paths return; the frames must agree to 1e-5 m and the stream must end where get_rays() leaves it."""
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from lidarcast import synth
    mesh = synth.make_room(size=(6, 5, 3), num_boxes=8, seed=2, cell=0.04)
    kd = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
    poses = [pose(1.0 + 0.5 * i, 2.5, 1.0, 0.25 * i) for i in range(6)]
    np.random.seed(5)
    lid = [create_lidar(kd, m) for m in poses]
    rec, off = engine.scan_lidars(lid, mesh, want=("t", "point3", "sem", "ins", "incident_deg"))
    end_host = np.random.random()
    np.random.seed(5)
    fr = engine.scan_frames_dual_axis([create_lidar(kd, m) for m in poses], mesh,
                                      want=("point3", "sem", "ins", "incident_deg", "index"))
    assert np.random.random() == end_host                        # same number of draws consumed
    keep = np.isfinite(rec["t"])
    host_counts = np.array([int(keep[off[i]:off[i + 1]].sum()) for i in range(6)])
    n_diff_sets, worst = 0, 0.0
    ends = np.cumsum(fr["counts"])
    for i in range(6):
        a = rec["point3"][off[i]:off[i + 1]][keep[off[i]:off[i + 1]]]
        b = fr["point3"][ends[i] - fr["counts"][i]:ends[i]]
        if len(a) == len(b):
            d = np.abs(a.astype(np.float64) - b).max()
            same = np.array_equal(a.view(np.uint32), b.view(np.uint32))
        else:                     # a ray flipped between hit and miss: compare through the nearest points
            d, same = 0.0, False
        n_diff_sets += not same
        worst = max(worst, d)
    frac = np.abs(fr["counts"] - host_counts).sum() / host_counts.sum()
    print(f"\n[dual-axis device generation] poses whose frames differ in any bit: {n_diff_sets}/6, "
          f"largest coordinate difference {worst:.3e} m, hit-count difference {frac:.2e}")
    assert frac <= 1e-4 and worst <= 1e-5
    assert fr["total"] > 6 * 60000
    # through the simulator: opt-in switch, same frames as the direct call
    from s3dis_simulator import S3DISSimulator
    from trajectory import Waypoint
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True, "device_ray_generation": True}}, use_blk2go=True)
    sim.raycast_engine = engine
    sim.load_scene(mesh, "room")
    np.random.seed(5)
    sc = sim.run_simulation([Waypoint(m[0, 3], m[1, 3], m[2, 3], yaw=0.25 * i) for i, m in enumerate(poses)])
    assert [len(f.points) for f in sc.frames] == fr["counts"].tolist()
    assert_bit_equal(sc.combined_points(), fr["point3"])


# ---- labels from annotation files through the simulator (advisor finding) ---------------------------------------
def test_simulator_export_reads_the_annotation_files(tmp_path, engine):
    """S3DISSimulator configured with s3dis_data_root / area / room, as the reference wires it
    (containers/s3dis_sim_scene.py:379-427): run_simulation attaches the hit triangles' labels to every frame, and
    save_results must STILL take colours and labels from the annotation files on disk (nearest annotated point)."""
    from sklearn.neighbors import NearestNeighbors
    from containers import read_labeled_ply
    from lidarcast import synth
    from s3dis_annotation_loader import S3DISAnnotationLoader
    from s3dis_simulator import S3DISSimulator
    from trajectory import line_trajectory
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
    cfg = {"raycast_engine": {"use_gpu": True}, "s3dis_data_root": str(tmp_path / "data"), "area": "Area_7",
           "room": "office_3"}
    sim = S3DISSimulator(cfg)
    sim.raycast_engine = engine
    sim.load_scene(mesh, "office_3")
    scene = sim.run_simulation(line_trajectory((1.2, 1.5, 1.0), (2.8, 1.5, 1.0), 3))
    assert all(f.semantic_labels is not None for f in scene.frames)        # the kernel's labels are attached ...
    sim.save_results(scene, tmp_path / "out")
    out = read_labeled_ply(tmp_path / "out" / "combined_pointcloud_with_label.ply")
    loader = S3DISAnnotationLoader(str(tmp_path / "data"))
    ap, al, ai = loader.create_labeled_pointcloud_with_instances(loader.load_room_annotations("Area_7", "office_3"))
    rawd = np.loadtxt(room / "office_3.txt")
    col = rawd[NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(rawd[:, :3]).kneighbors(ap)[1][:, 0], 3:6] / 255.0
    allp = scene.combined_points()
    j = NearestNeighbors(n_neighbors=1, algorithm="ball_tree").fit(ap).kneighbors(allp)[1][:, 0]
    assert len(out) == len(allp) > 500
    assert np.array_equal(out["sem"], al[j].astype(np.uint16)) and np.array_equal(out["ins"], ai[j].astype(np.uint16))   # ... the files decide
    assert np.array_equal(np.stack([out["red"], out["green"], out["blue"]], 1), (col[j] * 255).astype(np.uint8))
    assert len(np.unique(out["red"])) > 50                                  # not the default grey


# ---- the grid entry points / the packet kernel: same bytes as the per-ray kernel ------------------------------------
# In the product library lrc_scan_grid_* run the per-ray kernel; the packet kernel lives in the laboratory build.  The two
# tests below run in-process against the product library (the entry points, their argument checks, the routing) and once
# more in a child process against liblidarcast_lab.so (test_packet_kernel_in_the_laboratory_build), where they compare
# the packet kernel itself with the per-ray kernel.
def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def test_packet_kernel_is_bit_identical(engine):
    """lrc_scan_grid_dev (one wavefront per packet of rays: frustum traversal + per-triangle candidate rays, LDS
    atomic min) against lrc_scan_poses_dev (one lane per ray) on the same tables: every output attribute must agree
    bit for bit -- tessellated and rough rooms, giant triangles (a cube), a triangle soup, a single quad; yawed, pitched
    and rolled sensors; steep scan lines; origins millimetres from a wall; line counts that do not fill a packet."""
    import torch
    import lidarcast
    from lidar import Indoor8LineLidarIntrinsics, IndoorLidar
    from lidarcast import synth
    from lidarcast.synth import TriangleMesh
    from raycast_engine.raycast_engine_hip import RaycastEngineHIP
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    v, f = __import__("helpers").random_soup(3000, 5, extent=3.0, size=0.4)
    cube = synth.unit_cube(-2.0, 2.5)
    scenes = {
        "room": synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.04),
        "rough": synth.make_room(size=(4, 3, 2.5), num_boxes=3, seed=8, rough=True),
        "cube": TriangleMesh(cube.vertices + 0.25, cube.triangles),
        "soup": TriangleMesh(v + 1.0, f),
        "quad": synth.quad(z=1.7, half=3.0),
    }
    sensors = {
        "8x512": Indoor8LineLidarIntrinsics(vertical_res=8, horizontal_res=512, max_range=20.0,
                                            vertical_degrees=[15.0, 10.0, 5.0, 0.0, -5.0, -10.0, -15.0, -20.0]),
        "32x2048": sensor_32x2048(),
        "steep5x256": Indoor8LineLidarIntrinsics(vertical_res=5, horizontal_res=256, max_range=3.0,
                                                 vertical_degrees=[75.0, 40.0, 1.0, -33.0, -80.0]),
        "11x320": Indoor8LineLidarIntrinsics(vertical_res=11, horizontal_res=320, max_range=50.0,
                                             vertical_degrees=list(np.linspace(25, -35, 11))),
    }
    poses = []
    for (x, y, z, yaw, pitch, roll) in [(1.0, 1.2, 1.0, 0.0, 0.0, 0.0), (2.2, 1.6, 1.1, 0.7, 0.0, 0.0),
                                        (3.0, 1.0, 0.6, -2.5, 0.3, -0.2), (0.03, 1.5, 1.2, 3.1, 0.0, 0.0),
                                        (2.0, 0.004, 2.4, 1.3, -0.5, 1.0), (1.5, 1.5, 1.7, 0.2, 0.0, 0.0)]:
        m = np.eye(4)
        m[:3, :3] = _rot(yaw, pitch, roll)
        m[:3, 3] = (x, y, z)
        poses.append(m)
    poses = np.stack(poses)
    want = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg", "tile_count")
    checked = 0
    for sname, mesh in scenes.items():
        scene = lidarcast.Scene(engine.ctx, mesh.vertices, mesh.triangles, getattr(mesh, "triangle_sem", None),
                                getattr(mesh, "triangle_ins", None))
        for kname, k in sensors.items():
            dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
            grid = RaycastEngineHIP._derive_grid(dirs, k.horizontal_res)
            assert grid is not None, kname
            ps = poses[:2] if kname == "32x2048" else poses
            P, N = len(ps), len(dirs)
            d_poses, d_dirs = torch.from_numpy(ps.reshape(P, 16)).to(dev), torch.from_numpy(dirs).to(dev)
            a = lidarcast.DeviceHits(P * N, dev, want=want)
            b = lidarcast.DeviceHits(P * N, dev, want=want)
            scene.scan_poses_dev(d_poses, d_dirs, a, k.max_range, st)
            scene.scan_poses_dev(d_poses, d_dirs, b, k.max_range, st, grid=grid)
            torch.cuda.synchronize()
            for att in want:
                x, y = a[att].cpu().numpy(), b[att].cpu().numpy()
                ne = x.view(np.uint8) != y.view(np.uint8)
                assert not ne.any(), (f"{sname} / {kname}: {att} differs in {int(ne.reshape(len(x), -1).any(1).sum())} of "
                                      f"{len(x)} entries, first at {np.argwhere(ne.reshape(len(x), -1).any(1))[0]}")
            hit = np.isfinite(a["t"].cpu().numpy())
            if sname in ("room", "rough", "cube"):
                assert hit.mean() > 0.3
            checked += int(hit.sum())
        scene.close()
    assert checked > 500000


def test_packet_kernel_in_the_laboratory_build():
    """The two packet-kernel tests again, in a child process that loads the laboratory build (LRC_LIB)."""
    import subprocess
    import sys
    import __graft_entry__ as entry
    from conftest import REPO
    env = dict(os.environ, LRC_LIB=entry.LAB_LIB, LRC_SECTOR="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_configs_gpu.py"), "-q", "-x", "-m", "gpu",
                        "-k", "test_packet_kernel_is_bit_identical or test_packet_kernel_full_size_c3"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=REPO)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_packet_kernel_full_size_c3(engine):
    """C3 at full size through the packet kernel: all 4.19 M rays' records equal the per-ray kernel's, byte for byte
    (SHA-256 of every attribute), through both the device and the frame-producing entry points."""
    import torch
    import bench
    import lidarcast
    from lidarcast import synth
    mesh = synth.make_scene(bench.SCENE)
    scene = engine.scene_for(mesh)
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    dirs = engine._direction_table(sensor)
    assert engine._grid_of(sensor, len(poses)) is None              # off by default: a measured alternative
    engine.packet_kernel = True
    grid = engine._grid_of(sensor, len(poses))
    engine.packet_kernel = False
    assert grid == (32, 2048, np.pi, -2 * np.pi / 2048)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    P, N = len(poses), len(dirs)
    want = ("t", "prim", "normal3", "point3", "sem", "ins", "tile_count")
    d_poses, d_dirs = torch.from_numpy(poses.reshape(P, 16)).to(dev), torch.from_numpy(dirs).to(dev)
    dig = []
    for g in (None, grid):
        h = lidarcast.DeviceHits(P * N, dev, want=want)
        scene.scan_poses_dev(d_poses, d_dirs, h, sensor.max_range, st, grid=g)
        torch.cuda.synchronize()
        dig.append({a: hashlib.sha256(h[a].cpu().numpy().tobytes()).hexdigest() for a in want})
    assert dig[0] == dig[1]
    fa = scene.scan_poses_compact(poses, dirs, sensor.max_range, want=("point3", "sem", "ins", "index"))
    fb = scene.scan_poses_compact(poses, dirs, sensor.max_range, want=("point3", "sem", "ins", "index"), grid=grid)
    assert fa["total"] == fb["total"] > 4e6 and np.array_equal(fa["counts"], fb["counts"])
    for a in ("point3", "sem", "ins", "index"):
        assert_bit_equal(fa[a], fb[a], a)


def test_device_frame_statistics_carry_numpys_bits(engine):
    """lrc_frames.range_origin_mean/std, incident_mean/std (csrc/lrc_stats.h) against np.mean / np.std of the same
    frames: equal BITS, for frame sizes on every branch of numpy's summation (a handful of returns, <= 128, several
    full 8192-element chunks, a ragged tail), float32 and float64; and through S3DISSimulator.run_simulation the
    ScanQuality records equal what the reference's formulas give on the frames (s3dis_simulator.py:276-286)."""
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast import synth
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    sensors = [sensor_small(lines=4, width=64, max_range=1.05),                 # a few returns per pose
               sensor_small(lines=5, width=200, max_range=1.9),                 # hundreds, ragged
               Indoor8LineLidarIntrinsics(vertical_res=16, horizontal_res=1024, max_range=30.0,
                                          vertical_degrees=list(np.linspace(20, -25, 16))),   # 2 full chunks
               sensor_32x2048()]                                              # 8 full chunks, minus the room's seams
    seen = set()
    for k in sensors:
        poses = np.stack([pose(0.6 + 0.45 * i, 1.2 + 0.1 * i, 1.0, 0.37 * i) for i in range(7)])
        fr = engine.scan_frames(k, poses, mesh, want=("point3", "incident_deg", "range_origin", "range_origin_stats",
                                                      "incident_stats"))
        rng_f, ang_f = engine.split_frames(fr, "range_origin"), engine.split_frames(fr, "incident_deg")
        for i in range(len(poses)):
            n = int(fr["counts"][i])
            seen.add(0 if n == 0 else 1 if n < 8 else 2 if n <= 128 else 3 if n < 8192 else 4)
            if n == 0:
                assert fr["range_origin_mean"][i] == 0 and fr["incident_std"][i] == 0
                continue
            assert_bit_equal(fr["range_origin_mean"][i:i + 1], np.array([np.mean(rng_f[i])]), f"range mean, n={n}")
            assert_bit_equal(fr["range_origin_std"][i:i + 1], np.array([np.std(rng_f[i])]), f"range std, n={n}")
            assert_bit_equal(fr["incident_mean"][i:i + 1], np.array([np.mean(ang_f[i])]), f"incident mean, n={n}")
            assert_bit_equal(fr["incident_std"][i:i + 1], np.array([np.std(ang_f[i])]), f"incident std, n={n}")
    assert {2, 3, 4} <= seen or {1, 3, 4} <= seen, seen
    # through the simulator, not bug-compatible so the incident statistics are live too
    from s3dis_simulator import S3DISSimulator
    from trajectory import line_trajectory
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}}, use_dense_lidar=True, bug_compatible=False)
    sim.raycast_engine = engine
    sim.load_scene(mesh, "room")
    sc = sim.run_simulation(line_trajectory((0.8, 1.5, 1.0), (3.2, 1.5, 1.0), 9, yaw=0.3))
    for f in sc.frames:
        q, r = f.scan_quality, np.linalg.norm(f.points, axis=1)
        assert q.num_points == len(f.points) > 1000
        assert q.range_mean == np.mean(r) and q.range_std == np.std(r) and type(q.range_mean) is np.float32
        assert q.incident_angle_mean == np.mean(f.incident_angles) and q.incident_angle_std == np.std(f.incident_angles)


def test_frames_entry_point_edge_cases(engine):
    """lrc_scan_poses_compact off the beaten path: an empty mesh, one pose, a ray count that is not a multiple of 64
    (no fused keep counts, no chunking), and 70 poses x 16 384 rays (the chunked pipeline with uneven chunks 17/18/17/18)
    against the fixed-stride records; statistics against numpy every time."""
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast import synth
    from lidarcast.synth import TriangleMesh
    room = synth.make_room(size=(4, 3, 2.5), num_boxes=3, seed=9, cell=0.05)
    empty = TriangleMesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    big = Indoor8LineLidarIntrinsics(vertical_res=16, horizontal_res=1024, max_range=2.4,
                                     vertical_degrees=list(np.linspace(20, -25, 16)))
    odd = Indoor8LineLidarIntrinsics(vertical_res=5, horizontal_res=20, max_range=30.0,
                                     vertical_degrees=[10.0, 5.0, 0.0, -5.0, -10.0])
    cases = [(empty, sensor_small(lines=4, width=64), 3), (room, sensor_small(lines=4, width=64), 1), (room, odd, 6),
             (room, big, 70)]
    for mesh, k, n_poses in cases:
        poses = np.stack([pose(0.7 + 2.6 * i / max(n_poses - 1, 1), 1.5, 1.1, 0.05 * i) for i in range(n_poses)])
        rec, n = engine.scan_poses(k, poses, mesh, want=("t", "point3", "incident_deg"))
        fr = engine.scan_frames(k, poses, mesh, want=("point3", "incident_deg", "range_origin", "range_origin_stats",
                                                      "incident_stats"))
        keep = np.isfinite(rec["t"])
        assert np.array_equal(fr["counts"], keep.sum(1)) and fr["total"] == keep.sum()
        assert_bit_equal(fr["point3"], rec["point3"][keep])
        assert_bit_equal(fr["incident_deg"], rec["incident_deg"][keep])
        ends = np.cumsum(fr["counts"])
        for i in range(n_poses):
            r = fr["range_origin"][ends[i] - fr["counts"][i]:ends[i]]
            a = fr["incident_deg"][ends[i] - fr["counts"][i]:ends[i]]
            if len(r) == 0:
                assert fr["range_origin_mean"][i] == 0 and fr["range_origin_std"][i] == 0
                continue
            assert fr["range_origin_mean"][i] == np.mean(r) and fr["range_origin_std"][i] == np.std(r)
            assert fr["incident_mean"][i] == np.mean(a) and fr["incident_std"][i] == np.std(a)
        if mesh is empty:
            assert fr["total"] == 0
        if n_poses == 70:
            assert fr["total"] > 3e5 and 0.1 < keep.mean() < 0.9        # the range filter cuts through: ragged frames


def test_dual_axis_default_path_to_frames(engine):
    """lrc_scan_rays_compact (all host-generated rays at a fixed stride + dropout mask, compaction in HBM) against
    lrc_cast_segments on the ragged kept rays + host masking: the same frames bit for bit on the same seeded stream,
    the same number of RNG draws, statistics equal to numpy's."""
    from lidar import DualAxisLidarIntrinsics, create_lidar
    from lidarcast import synth
    mesh = synth.make_room(size=(6, 5, 3), num_boxes=8, seed=2, cell=0.04)
    kd = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
    poses = [pose(1.0 + 0.5 * i, 2.5, 1.0, 0.25 * i) for i in range(5)]
    np.random.seed(11)
    rec, off = engine.scan_lidars([create_lidar(kd, m) for m in poses], mesh, want=("t", "point3", "sem", "ins", "incident_deg"))
    end_a = np.random.random()
    np.random.seed(11)
    fr = engine.scan_frames_lidars([create_lidar(kd, m) for m in poses], mesh,
                                   want=("point3", "sem", "ins", "incident_deg", "range_origin_stats", "incident_stats"))
    assert np.random.random() == end_a
    keep = np.isfinite(rec["t"])
    assert fr["total"] == keep.sum() > 5 * 60000
    assert np.array_equal(fr["counts"], [int(keep[off[i]:off[i + 1]].sum()) for i in range(5)])
    assert_bit_equal(fr["point3"], rec["point3"][keep])
    assert_bit_equal(fr["incident_deg"], rec["incident_deg"][keep])
    assert np.array_equal(fr["sem"], rec["sem"][keep]) and np.array_equal(fr["ins"], rec["ins"][keep])
    ends = np.cumsum(fr["counts"])
    for i in range(5):
        pts = fr["point3"][ends[i] - fr["counts"][i]:ends[i]]
        r = np.linalg.norm(pts, axis=1)
        assert fr["range_origin_mean"][i] == np.mean(r) and fr["range_origin_std"][i] == np.std(r)
        a = fr["incident_deg"][ends[i] - fr["counts"][i]:ends[i]]
        assert fr["incident_mean"][i] == np.mean(a) and fr["incident_std"][i] == np.std(a)


def test_resident_direction_table_handle(engine):
    """lrc_table_create + lrc_scan_table_compact (the sensor's table uploaded once) against lrc_scan_poses_compact (table
    from host memory every call): the same frames bit for bit, statistics included; the handle survives many calls,
    a closed handle is refused loudly, and the engine keeps one per sensor."""
    import lidarcast
    from lidar import IndoorLidar
    from lidarcast import synth
    mesh = synth.make_room(size=(5, 4, 2.6), num_boxes=5, seed=4, cell=0.05)
    k = sensor_small(lines=8, width=256)
    dirs = IndoorLidar(intrinsics=k, pose=np.eye(4)).sensor_directions()
    poses = np.stack([pose(0.8 + 0.5 * i, 2.0, 1.2, 0.3 * i) for i in range(7)])
    scene = engine.scene_for(mesh)
    want = ("point3", "sem", "incident_deg", "index", "range_origin", "range_origin_stats", "incident_stats")
    a = scene.scan_poses_compact(poses, dirs, k.max_range, want=want)
    table = lidarcast.DirectionTable(scene.ctx, dirs)
    assert len(table) == len(dirs)
    for _ in range(3):
        b = scene.scan_poses_compact(poses, table, k.max_range, want=want)
        assert b["total"] == a["total"] > 0 and np.array_equal(a["counts"], b["counts"])
        for key in ("point3", "incident_deg", "range_origin", "range_origin_mean", "range_origin_std", "incident_mean",
                    "incident_std"):
            assert_bit_equal(a[key], b[key])
        assert np.array_equal(a["sem"], b["sem"]) and np.array_equal(a["index"], b["index"])
    one = scene.scan_poses_compact(poses[2:3], table, k.max_range, want=("point3",))
    lo = int(a["counts"][:2].sum())
    assert_bit_equal(one["point3"], a["point3"][lo:lo + int(a["counts"][2])])
    table.close()
    table.close()                                                   # idempotent
    with pytest.raises((ValueError, RuntimeError)):
        scene.scan_poses_compact(poses, table, k.max_range, want=want)
    t1 = engine._resident_table(k)
    assert engine._resident_table(k) is t1 and len(t1) == len(dirs)  # one upload per sensor


def test_quantised_node_images_and_their_fallbacks(engine, monkeypatch):
    """The 32-byte quantised node images against the definition (oracle, brute force): a room the
    grid fits (images in use), rays the margin is proven for, rays it is not (origins many scene widths away, waves
    that mix both, huge direction vectors), waves that straddle an axis direction (mixed octants), and a scene too
    far from the world origin for the grid (float32 nodes only).  Same bytes every time; float32-only scene equal too."""
    import lidarcast
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_room(size=(5, 4, 2.6), num_boxes=6, seed=12, cell=0.04)
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    rng = np.random.default_rng(3)
    n = 64 * 300
    o = rng.uniform([0.3, 0.3, 0.3], [4.7, 3.7, 2.3], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aim = rng.uniform([0.5, 0.5, 0.2], [4.5, 3.5, 2.4], (n, 3))
    # waves 0..99 in the room; 100..149 from 20..5000 m away aimed at the room; 150..199 alternate lane by lane;
    # 200..249 axis-parallel directions and directions of length 1e25; 250..299 one octant per wave (sorted signs)
    far_o = aim + d * rng.uniform(20.0, 5000.0, (n, 1))
    sl = slice(64 * 100, 64 * 150)
    o[sl] = far_o[sl]; d[sl] = -d[sl]
    sl = slice(64 * 150, 64 * 200)
    alt = (np.arange(64 * 50) % 2).astype(bool)
    o[sl][alt] = far_o[sl][alt]; d[sl][alt] = -d[sl][alt]
    sl = slice(64 * 200, 64 * 225)
    ax = np.eye(3)[rng.integers(0, 3, 64 * 25)] * rng.choice([-1.0, 1.0], (64 * 25, 1))
    d[sl] = ax
    d[64 * 225:64 * 250] *= 1e25
    sl = slice(64 * 250, 64 * 300)
    d[sl] = np.abs(d[sl]) * np.repeat(rng.choice([-1.0, 1.0], (50, 3)), 64, axis=0)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    t_ref, prim_ref = om.cast(rays)
    assert 0.5 < np.isfinite(t_ref).mean() <= 1.0 and np.isfinite(t_ref[64 * 100:64 * 150]).mean() > 0.5
    pick = rng.choice(n, 2500, replace=False)            # and the definition itself, no tree at all
    t_bf, prim_bf = om.brute(rays[pick])
    assert_bit_equal(t_bf, t_ref[pick])
    assert np.array_equal(prim_bf, prim_ref[pick])
    scene = lidarcast.Scene(engine.ctx, mesh.vertices, mesh.triangles)
    assert scene.info["quantised_nodes"] == 1 and 1.0 < scene.info["leaf_inflation"] < 1.05
    out = scene.cast(rays, want=("t", "prim"))
    assert_bit_equal(out["t"], t_ref)
    assert np.array_equal(out["prim"], prim_ref)
    monkeypatch.setenv("LRC_QNODES", "0")
    plain = lidarcast.Scene(engine.ctx, mesh.vertices, mesh.triangles)
    assert plain.info["quantised_nodes"] == 0
    out0 = plain.cast(rays, want=("t", "prim"))
    assert_bit_equal(out0["t"], t_ref)
    assert np.array_equal(out0["prim"], prim_ref)
    monkeypatch.delenv("LRC_QNODES")
    # the same room 3 km from the world origin: float32 coordinates there are 0.25 mm apart; the grid is not used
    shift = np.array([3000.0, -2000.0, 100.0])
    v_far = (mesh.vertices + shift).astype(np.float32)
    distant = lidarcast.Scene(engine.ctx, v_far, mesh.triangles)
    assert distant.info["quantised_nodes"] == 0
    rays_far = rays[:64 * 100].copy()
    rays_far[:, :3] = (rays_far[:, :3].astype(np.float64) + shift).astype(np.float32)
    om_far = OracleMesh(v_far, mesh.triangles).build()
    t2, p2 = om_far.cast(rays_far)
    out2 = distant.cast(rays_far, want=("t", "prim"))
    assert_bit_equal(out2["t"], t2)
    assert np.array_equal(out2["prim"], p2)


def test_quantised_images_on_random_scenes(engine, monkeypatch):
    """Quantised node images against the float32 nodes of the same tree, bit for bit, over scenes of very different
    shape -- triangle soups from millimetres to hundreds of metres, offset from the world origin by up to three scene
    widths, flat in one axis, a single triangle -- with origins inside, on the faces of and around the scene's box and
    directions that graze box planes (axis-parallel, one component 0 or -0, denormal-small components)."""
    import lidarcast
    from oracle.c_oracle import OracleMesh
    rng = np.random.default_rng(2024)
    used = 0
    for case in range(12):
        scale = 10.0 ** rng.uniform(-2.0, 2.5)
        T = int(rng.integers(1, 4000)) if case else 1
        centre = rng.uniform(-1.0, 1.0, 3) * scale * rng.choice([0.0, 0.5, 3.0])
        ext = np.array([1.0, rng.uniform(0.05, 1.0), rng.uniform(0.0 if case == 3 else 0.01, 1.0)]) * scale
        c = rng.uniform(-0.5, 0.5, (T, 1, 3)) * ext
        tri = (centre + c + rng.normal(scale=0.03 * scale, size=(T, 3, 3)) * (ext > 0)).astype(np.float32)
        v, f = tri.reshape(-1, 3), np.arange(3 * T, dtype=np.int32).reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        n = 64 * 400
        o = rng.uniform(lo - 0.3 * (hi - lo) - 1e-3 * scale, hi + 0.3 * (hi - lo) + 1e-3 * scale, (n, 3))
        onface = rng.random(n) < 0.2                       # origins exactly on a face of the scene's box
        ax = rng.integers(0, 3, n)
        o[onface, ax[onface]] = np.where(rng.random(onface.sum()) < 0.5, lo[ax[onface]], hi[ax[onface]])
        target = v[rng.integers(0, len(v), n)].astype(np.float64) + rng.normal(scale=0.01 * scale, size=(n, 3))
        d = target - o
        kind = rng.integers(0, 8, n)
        d[kind == 0] = np.eye(3)[rng.integers(0, 3, (kind == 0).sum())] * rng.choice([-1.0, 1.0], ((kind == 0).sum(), 1))
        z = kind == 1
        d[z, rng.integers(0, 3, z.sum())] = rng.choice([0.0, -0.0], z.sum())
        t = kind == 2
        d[t, rng.integers(0, 3, t.sum())] = rng.choice([1e-38, -1e-38, 1e-42, -1e-30], t.sum())
        rays = np.concatenate([o, d], 1).astype(np.float32)
        monkeypatch.setenv("LRC_QNODES", "2")
        q = lidarcast.Scene(engine.ctx, v, f)
        monkeypatch.setenv("LRC_QNODES", "0")
        w = lidarcast.Scene(engine.ctx, v, f)
        monkeypatch.delenv("LRC_QNODES")
        used += q.info["quantised_nodes"]
        assert w.info["quantised_nodes"] == 0
        a = q.cast(rays, want=("t", "prim", "point3"))
        b = w.cast(rays, want=("t", "prim", "point3"))
        assert_bit_equal(a["t"], b["t"])
        assert np.array_equal(a["prim"], b["prim"])
        assert_bit_equal(a["point3"], b["point3"])
        if T <= 1500:                                      # and the definition itself on the smaller scenes
            om = OracleMesh(v, f)
            pick = rng.choice(n, 4000, replace=False)
            t_bf, p_bf = om.brute(rays[pick])
            assert_bit_equal(a["t"][pick], t_bf)
            assert np.array_equal(a["prim"][pick], p_bf)
        q.close(); w.close()
    assert used >= 6          # most of these scenes take the grid (those offset by three widths do not)


# ---- the reference's own arithmetic, where the measuring host has it ----------------------------------------------------
def test_hip_against_open3d_cast_rays(engine):
    """The ONE thing that can pin parity at the Embree boundary: Open3D's
    RaycastingScene.cast_rays -- the call the reference makes at raycast_engine_cpu.py:46-51 -- on the same float32 rays as the
    HIP engine: C2 (8 x 512 in synth_A1_office) and three poses of C3.  Hit mask equal except on rays whose float64 witness
    puts the hit within 1e-6 of a triangle edge (or that graze a seam), |t_hip - t_open3d| <= 1e-5 m (north star), the same
    triangle row.  Skipped where Open3D is not installed (it is absent on this pool's boxes: DESIGN.md section 7)."""
    o3d = pytest.importorskip("open3d")
    import bench
    from lidar import create_lidar
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    cases = [("C2", "synth_A1_office", sensor_8x512(), [pose(4.0, 3.0, 1.0)]),
             ("C3", bench.SCENE, bench.c3_sensor(), list(bench.c3_poses(0, 1)[[0, 31, 63]]))]
    for name, scene_name, sensor, poses in cases:
        mesh = synth.make_scene(scene_name)
        rays = np.concatenate([create_lidar(sensor, m).get_rays() for m in poses]).astype(np.float32)
        out = engine.cast_rays(rays, mesh)
        legacy = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(np.asarray(mesh.vertices, dtype=np.float64)),
                                           o3d.utility.Vector3iVector(np.asarray(mesh.triangles, dtype=np.int32)))
        sc = o3d.t.geometry.RaycastingScene()
        sc.add_triangles(o3d.t.geometry.TriangleMesh.from_legacy(legacy))
        ans = sc.cast_rays(o3d.core.Tensor(rays))
        t_ref, p_ref = ans["t_hit"].numpy(), ans["primitive_ids"].numpy()
        t_hip, p_hip = out["t_hit"], out["primitive_ids"]
        h_ref, h_hip = np.isfinite(t_ref), np.isfinite(t_hip)
        _, _, margin = OracleMesh(mesh.vertices, mesh.triangles).witness(rays, threads=16)
        differ = h_ref != h_hip
        both = h_ref & h_hip
        dt = np.abs(t_ref[both].astype(np.float64) - t_hip[both].astype(np.float64))
        other = both & (p_ref != p_hip)
        print(f"\n[open3d {o3d.__version__}] {name}: rays {len(rays)}, both hit {int(both.sum())}, hit/miss disagreements "
              f"{int(differ.sum())} (of them with witness margin >= 1e-6: {int((differ & (margin >= 1e-6)).sum())}), other "
              f"triangle {int(other.sum())}, max |dt| {dt.max():.3e} m, bit-equal t {int((t_ref[both] == t_hip[both]).sum())}")
        assert not (differ & (margin >= 1e-6)).any(), "hit mask differs from Open3D away from triangle edges"
        assert dt.max() <= 1e-5
        assert (margin[other] < 1e-4).all(), "another triangle than Open3D's away from a shared edge"
