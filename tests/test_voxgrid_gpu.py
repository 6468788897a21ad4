"""-m gpu: semantic occupancy grids (csrc/lrc_voxgrid.hip) against the numpy restatement (tests/voxgrid_restate.py):
synthetic rays bit for bit, analytic scenes, a real trajectory, the returns invariant on C3, order and chunking, and
the engine / simulator layers."""
import json

import numpy as np
import pytest

import voxgrid_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    return RaycastEngineGPU()


@pytest.fixture(scope="module")
def office():
    from lidarcast import synth
    return synth.make_scene("synth_A6_office2")


def _pose(x, y, z, R3=None):
    m = np.eye(4)
    if R3 is not None:
        m[:3, :3] = R3
    m[:3, 3] = (x, y, z)
    return m


def _dirs_sphere(n):
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    r = np.sqrt(1 - z * z)
    phi = i * np.pi * (3 - np.sqrt(5))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def _rows_of(ctx, poses, dirs, t_label):
    """(o, e, labels) of the returned rays of a pose-batched (t, label) array, e rebuilt on the device by the scene
    cloud's own rebuild (lrc_cloud_from_ranges_dev: the rows the scan's compaction writes)."""
    import torch
    P, N = len(poses), len(dirs)
    poses_t = torch.from_numpy(np.ascontiguousarray(poses, np.float64).reshape(P, 16)).cuda()
    dirs_t = torch.from_numpy(np.ascontiguousarray(dirs, np.float64)).cuda()
    tl_t = torch.from_numpy(np.ascontiguousarray(t_label).view(np.int32).reshape(P * N, 2)).cuda()
    rows = torch.empty((P * N, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros(P, dtype=torch.int64, device="cuda")
    ctx.cloud_from_ranges_dev(poses_t, dirs_t, tl_t, rows, counts)
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    r = rows[:int(c.sum())].cpu().numpy()
    o = np.repeat(np.asarray(poses, np.float64).reshape(P, 4, 4)[:, :3, 3].astype(np.float32), c, axis=0)
    return o, r[:, :3].copy(), r[:, 3].view(np.uint32).copy(), (poses_t, dirs_t, tl_t)


def _t_label(t, sem, ins):
    tl = np.zeros((len(t), 2), np.uint32)
    tl[:, 0] = np.asarray(t, np.float32).view(np.uint32)
    tl[:, 1] = np.asarray(sem, np.uint32) | (np.asarray(ins, np.uint32) << 16)
    return tl


def _assert_equal(res, sp, st, c):
    assert np.array_equal(res.idx, sp["idx"]) and res.idx.dtype == np.uint32
    assert np.array_equal(res.sem, sp["sem"]) and np.array_equal(res.ins, sp["ins"])
    assert np.array_equal(res.returns, sp["returns"])
    if res.state is not None:
        assert np.array_equal(res.state.reshape(-1), st), int((res.state.reshape(-1) != st).sum())
    assert (res.num_free, res.num_occupied, res.num_unknown) == (c["free"], c["occupied"], c["unknown"])
    assert res.rejected_rays == c.get("rejected_rays", 0)


def _same(a, b):
    assert np.array_equal(a.idx, b.idx) and np.array_equal(a.sem, b.sem) and np.array_equal(a.ins, b.ins)
    assert np.array_equal(a.returns, b.returns) and np.array_equal(a.state, b.state)
    assert (a.num_free, a.num_occupied, a.num_unknown, a.rejected_rays) == \
        (b.num_free, b.num_occupied, b.num_unknown, b.rejected_rays)


# ---- synthetic rays -------------------------------------------------------------------------------------------------
def _synthetic(seed):
    """Random rotated poses, an arbitrary (unnormalised) direction table with rays aimed through voxel corners and
    edges, crafted t: misses, a few labels so that votes tie."""
    rng = np.random.default_rng(seed)
    P, N = 6, 700
    poses = []
    for p in range(P):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        poses.append(_pose(*rng.uniform(0.2, 1.0, 3), q if p % 2 else None))
    poses[0][:3, 3] = (0.5, 0.5, 0.5)                         # on a voxel corner of the dyadic grid
    dirs = rng.normal(size=(N, 3)) * rng.uniform(0.5, 2.0, (N, 1))
    dirs[:8] = [[1, 1, 1], [1, 1, 0], [1, 0, 0], [0, 0, 1], [-1, -1, 1], [-1, 0, -1], [0, -1, 0], [1, -1, -1]]
    t = rng.uniform(0.0, 1.6, P * N).astype(np.float32)
    t[rng.random(P * N) < 0.15] = np.inf
    t[:8] = np.float32(0.5) * np.sqrt(np.float32([3, 2, 1, 1, 3, 2, 1, 3]))   # ends on corners and edges too
    sem = rng.integers(0, 3, P * N)
    ins = rng.integers(0, 3, P * N)
    return np.stack(poses), dirs, _t_label(t, sem, ins)


GRIDS = [((0.0, 0.0, 0.0), 0.0625, (24, 24, 24)),            # dyadic: exact corner and edge ties
         ((-0.35, -0.2, -0.1), 0.05, (50, 44, 40)),            # covers everything
         ((0.3, 0.25, 0.2), 0.05, (13, 9, 17))]                # sensors outside, segments entering and leaving


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("grid", GRIDS)
def test_synthetic_rays_bit_equal_to_restatement(ctx, seed, grid):
    from lidarcast import OccupancyGrid
    poses, dirs, tl = _synthetic(seed)
    o, e, lab, (poses_t, dirs_t, tl_t) = _rows_of(ctx, poses, dirs, tl)
    g, s, dims = grid
    vg = OccupancyGrid(ctx, g, s, dims)
    vg.accumulate_dev(poses_t, dirs_t, tl_t)
    for mr in (1, 2, 3):
        res = vg.finalize(min_returns=mr)
        sp, st, c = R.grid_from_rays(o, e, lab, g, s, dims, min_returns=mr)
        _assert_equal(res, sp, st, c)
    free, _, _, _ = R.walk(o, e, g, s, dims)
    bits = vg.free_bits()
    assert np.array_equal(np.unpackbits(bits.view(np.uint8), bitorder="little")[:len(free)].astype(bool), free)
    # accumulation is additive: the same rays again double every count and keep the bits
    vg.accumulate_dev(poses_t, dirs_t, tl_t)
    twice = vg.finalize()
    sp, st, c = R.grid_from_rays(np.concatenate([o, o]), np.concatenate([e, e]), np.concatenate([lab, lab]), g, s, dims)
    _assert_equal(twice, sp, st, c)
    vg.reset()
    empty = vg.finalize()
    assert len(empty.idx) == 0 and empty.num_free == 0 and empty.num_unknown == int(np.prod(dims))
    assert not empty.state.any()
    vg.close()


def test_without_dense_state_and_bad_min_returns(ctx):
    from lidarcast import OccupancyGrid
    poses, dirs, tl = _synthetic(2)
    _, _, _, (poses_t, dirs_t, tl_t) = _rows_of(ctx, poses, dirs, tl)
    vg = OccupancyGrid(ctx, *GRIDS[1])
    vg.accumulate_dev(poses_t, dirs_t, tl_t)
    a, b = vg.finalize(dense=True), vg.finalize(dense=False)
    assert b.state is None and np.array_equal(a.idx, b.idx) and a.num_free == b.num_free
    with pytest.raises(ValueError):
        vg.finalize(min_returns=0)
    with pytest.raises(ValueError):
        vg.accumulate_dev(poses_t.float(), dirs_t, tl_t)


# ---- analytic scenes --------------------------------------------------------------------------------------------------
def _scan_grid(ctx, mesh, poses, dirs, g, s, dims, max_range=10.0):
    from lidarcast import OccupancyGrid, Scene, scan_occupancy
    scene = Scene(ctx, mesh.vertices, mesh.triangles)
    vg = OccupancyGrid(ctx, g, s, dims)
    scan_occupancy(scene, vg, poses, dirs, max_range)
    res = vg.finalize()
    rec = scene.scan_poses(poses, dirs, max_range, want=("t", "point3"))
    vg.close()
    return res, rec


def test_unit_cube_from_its_centre(ctx):
    """Grid offset by half a voxel: the faces x = +-1 lie mid-voxel (index 2 and 22 of 25).  Occupied voxels are exactly
    the shell, everything outside is unknown, the interior is all free (200 000 directions reach every shell voxel,
    the cube's corner voxels included, and cross every interior one)."""
    from lidarcast import synth
    m = synth.unit_cube()
    g, s, dims = (-1.25, -1.25, -1.25), 0.1, (25, 25, 25)
    dirs = _dirs_sphere(200000)
    res, rec = _scan_grid(ctx, m, _pose(0, 0, 0)[None], dirs, g, s, dims)
    ijk = np.stack(np.meshgrid(*[np.arange(25)] * 3, indexing="ij"), -1)
    inner = np.all((ijk >= 3) & (ijk <= 21), -1)
    box = np.all((ijk >= 2) & (ijk <= 22), -1)
    shell = box & ~inner
    assert np.array_equal(res.state == R.OCCUPIED, shell)
    assert (res.state[~box] == R.UNKNOWN).all()
    assert (res.state[inner] == R.FREE).all()
    assert res.returns.sum() == 200000 and res.num_occupied == int(shell.sum())
    # the restatement agrees on the rays themselves
    o = np.zeros((200000, 3), np.float32)
    sp, st, c = R.grid_from_rays(o, rec["point3"], np.zeros(200000, np.uint32), g, s, dims)
    _assert_equal(res, sp, st, c)


def test_box_occluder_leaves_the_space_behind_it_unknown(ctx):
    from lidarcast import synth
    c = synth.unit_cube(-2.0, 2.0)
    v = np.concatenate([c.vertices, [[1, -2.5, -2.5], [1, 2.5, -2.5], [1, 2.5, 2.5], [1, -2.5, 2.5]]])
    f = np.concatenate([c.triangles, np.array([[8, 9, 10], [8, 10, 11]], np.int32)])
    m = synth.TriangleMesh(vertices=v, triangles=f.astype(np.int32))
    g, s, dims = (-2.25, -2.25, -2.25), 0.1, (45, 45, 45)
    res, rec = _scan_grid(ctx, m, _pose(0, 0, 0)[None], _dirs_sphere(300000), g, s, dims)
    # x = 1 lies mid-voxel 32; x = 2 mid-voxel 42
    assert (res.state[33:] == R.UNKNOWN).all()                      # behind the occluder: no ray got there
    assert (res.state[32, 3:42, 3:42] == R.OCCUPIED).all()          # the occluder itself, inside the cube
    assert (res.state[2, 3:42, 3:42] == R.OCCUPIED).all()           # the -x face in front of the sensor
    assert (res.state[3:32, 3:42, 3:42] != R.UNKNOWN).all()         # the space in front of it is all seen
    sp, st, cnt = R.grid_from_rays(np.zeros((len(rec["t"]), 3), np.float32)[np.isfinite(rec["t"])],
                                   rec["point3"][np.isfinite(rec["t"])], np.zeros(int(np.isfinite(rec["t"]).sum())),
                                   g, s, dims)
    _assert_equal(res, sp, st, cnt)


# ---- a real trajectory ------------------------------------------------------------------------------------------------
def _small_sensor():
    import dataclasses
    from lidar import Indoor8LineLidarIntrinsics
    return dataclasses.replace(Indoor8LineLidarIntrinsics.create_standard_8line(), horizontal_res=256)


def _line_poses(n, z=1.0):
    from trajectory import line_trajectory, poses_from_waypoints
    return poses_from_waypoints(line_trajectory((0.8, 1.1, z), (4.2, 2.9, z), n))


def _cloud(engine, sensor, poses, mesh):
    fr = engine.scan_frames(sensor, poses, mesh, want=("point3", "sem", "ins"))
    o = np.repeat(poses[:, :3, 3].astype(np.float32), fr["counts"], axis=0)
    lab = fr["sem"].astype(np.uint32) | (fr["ins"].astype(np.uint32) << 16)
    return o, fr["point3"], lab, fr


def test_real_trajectory_bit_equal_to_restatement(engine, office):
    sensor = _small_sensor()
    poses = _line_poses(8)
    res = engine.occupancy_grid(sensor, poses, office, voxel_size=0.05)
    o, e, lab, fr = _cloud(engine, sensor, poses, office)
    assert len(e) > 0.5 * len(poses) * 8 * 256
    sp, st, c = R.grid_from_rays(o, e, lab, res.origin, res.voxel_size, res.dims)
    _assert_equal(res, sp, st, c)
    assert res.num_free > 0 and res.num_occupied > 0 and len(res.per_class) >= 2
    res2 = engine.occupancy_grid(sensor, poses, office, voxel_size=0.05, min_returns=2)
    sp, st, c = R.grid_from_rays(o, e, lab, res.origin, res.voxel_size, res.dims, min_returns=2)
    _assert_equal(res2, sp, st, c)


def test_returns_invariant_on_c3(engine, office):
    """Sum of returns = returned rays of scan_frames; the sparse (idx, returns) = np.unique of the scene cloud rows'
    voxel indices (the default extent holds every row)."""
    import bench
    sensor = bench.c3_sensor()
    poses = bench.c3_poses(0, 1)
    res = engine.occupancy_grid(sensor, poses, office)
    fr = engine.scan_frames(sensor, poses, office, want=("point3",))
    assert int(res.returns.sum(dtype=np.uint64)) == fr["total"] and res.rejected_rays == 0
    c = R.voxel_of(fr["point3"].astype(np.float64), res.origin, res.voxel_size).astype(np.int64)
    assert R.inside(c, res.dims).all()
    u, n = np.unique(R.linear(c, res.dims), return_counts=True)
    assert np.array_equal(res.idx, u.astype(np.uint32)) and np.array_equal(res.returns, n.astype(np.uint32))
    assert res.num_free + res.num_occupied + res.num_unknown == int(np.prod(res.dims))
    assert res.num_occupied == len(u) and res.num_free > res.num_occupied


def test_pose_order_and_chunking_do_not_matter(ctx, engine, office):
    from lidarcast import OccupancyGrid, scan_occupancy
    from lidarcast.voxgrid import default_extent
    sensor = _small_sensor()
    poses = _line_poses(23)
    dirs = engine._direction_table(sensor)
    scene = engine.scene_for(office)
    g, dims = default_extent(office.vertices, 0.05)
    outs = []
    for ps, chunk in ((poses, None), (poses, 7), (poses[::-1].copy(), None), (poses[::-1].copy(), 5)):
        vg = OccupancyGrid(ctx, g, 0.05, dims)
        scan_occupancy(scene, vg, ps, dirs, sensor.max_range, chunk_poses=chunk)
        outs.append(vg.finalize())
        vg.close()
    for b in outs[1:]:
        _same(outs[0], b)
    # the engine's one-call form is the same computation
    _same(outs[0], engine.occupancy_grid(sensor, poses, office, voxel_size=0.05))


# ---- upper layers ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(office):
    from s3dis_simulator import S3DISSimulator
    s = S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    s.load_scene(office, "synth_A6_office2")
    return s


def test_simulator_export_round_trips(sim, office, tmp_path):
    from containers.s3dis_sim_scene import read_labeled_ply
    from lidarcast.synth import S3DIS_CLASSES
    from trajectory import line_trajectory, poses_from_waypoints
    wps = line_trajectory((1.0, 1.5, 1.0), (4.0, 2.5, 1.0), 6)
    d = sim.export_occupancy_grid(wps, tmp_path, voxel_size=0.1, min_returns=1)
    ref = sim.raycast_engine.occupancy_grid(sim.lidar_config, poses_from_waypoints(wps), office, voxel_size=0.1)
    z = np.load(tmp_path / "synth_A6_office2_occupancy.npz")
    assert np.array_equal(z["state"], ref.state) and np.array_equal(z["sem"], ref.dense_sem)
    assert np.array_equal(z["ins"], ref.dense_ins) and np.array_equal(z["returns"], ref.dense_returns)
    assert np.array_equal(z["origin"], ref.origin) and float(z["voxel_size"]) == 0.1
    assert tuple(z["dims"]) == ref.dims and z["state"].shape == ref.dims
    # the dense arrays and the sparse list describe the same voxels
    flat = z["returns"].reshape(-1)
    assert np.array_equal(np.flatnonzero(flat), ref.idx.astype(np.int64))
    with open(tmp_path / "synth_A6_office2_occupancy.json") as f:
        j = json.load(f)
    assert j == json.loads(json.dumps(d))
    assert j["counts"]["occupied"] == ref.num_occupied and j["counts"]["free"] == ref.num_free
    assert j["num_poses"] == 6 and j["dims"] == list(ref.dims)
    assert j["per_class_occupied_voxels"] == {S3DIS_CLASSES[k]: v for k, v in ref.per_class.items()}
    assert sum(j["per_class_occupied_voxels"].values()) == ref.num_occupied
    ply = read_labeled_ply(tmp_path / "synth_A6_office2_occupied_voxels.ply")
    centres, sem, ins = ref.occupied_centres()
    assert len(ply) == ref.num_occupied
    assert np.array_equal(np.stack([ply["x"], ply["y"], ply["z"]], 1), centres.astype(np.float32))
    assert np.array_equal(ply["sem"], sem) and np.array_equal(ply["ins"], ins)
    # every occupied centre lies in the voxel it names
    c = R.voxel_of(centres, ref.origin, ref.voxel_size).astype(np.int64)
    assert np.array_equal(R.linear(c, ref.dims), ref.idx[ref.occupied].astype(np.int64))


def test_dual_axis_and_sweeps_are_out_of_scope(sim, office, tmp_path):
    from lidar import DualAxisLidarIntrinsics
    from trajectory import line_trajectory
    with pytest.raises(NotImplementedError):
        sim.raycast_engine.occupancy_grid(DualAxisLidarIntrinsics.create_blk2go_dual_axis(), np.eye(4)[None], office)
    sim.config["motion"] = {"speed": 0.5}
    try:
        with pytest.raises(NotImplementedError):
            sim.export_occupancy_grid(line_trajectory((1, 1, 1), (2, 2, 1), 3), tmp_path)
    finally:
        del sim.config["motion"]
    assert not list(tmp_path.iterdir())
