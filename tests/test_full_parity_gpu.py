"""-m gpu: every ray of every full-size scan path against the oracle, bit for bit (tests/full_parity.py).

The sampled full-size tests compared a few poses of 64 with the oracle and the scan pipeline only with the plain device
path.  Here nothing is sampled and nothing is compared through a chain: the plain device path, the scan pipeline as bench.py
drives it, the sharded pipeline, rotated / close / range-cut poses, moving-sensor sweeps and the host-facing compact entry
each meet ``full_parity.expected_scan`` on 100 % of their rays.  Every test asserts the kept share of its input (an empty
comparison cannot pass) and prints one line: rays compared, kept share, rays that differ."""
import dataclasses

import numpy as np
import pytest

import full_parity as fp
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

FILL = -7.0                      # what test_pipe_edges_gpu.outputs() fills the caller's rows with
C3_RAYS = 64 * 65536
_HOST_TYPES = {"t": np.float32, "prim": np.uint32, "normal3": np.float32, "point3": np.float32, "sem": np.uint16,
               "ins": np.uint16}
_WIDTH = {"t": 4, "prim": 4, "normal3": 12, "point3": 12, "sem": 2, "ins": 2}


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


@pytest.fixture(scope="module")
def c3(ctx):
    """bench.SCENE with its oracle tree, the C3 sensor and its direction table on the device."""
    import torch
    import bench
    import lidarcast
    from lidar import IndoorLidar
    mesh, om = fp.scene_and_oracle(bench.SCENE)
    sensor = bench.c3_sensor()
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    yield {"mesh": mesh, "om": om, "sensor": sensor, "scene": scene, "N": len(dirs),
           "d_dirs": torch.from_numpy(dirs).to("cuda")}
    scene.close()


def _device(poses):
    import torch
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    return torch.from_numpy(poses.reshape(len(poses), 16)).to("cuda")


def _records_of_hits(hits):
    """One device-to-host copy per record field of a DeviceHits."""
    return {a: hits[a].cpu().numpy().view(dt) for a, dt in _HOST_TYPES.items()}


def _records_of_pointers(rec, n):
    """The same for an LrcHits of bare device pointers (lrc_pipe_records)."""
    from test_pipe_edges_gpu import _dev_bytes
    out = {}
    for a, dt in _HOST_TYPES.items():
        out[a] = _dev_bytes(getattr(rec, a), n * _WIDTH[a]).cpu().numpy().view(dt)
    return out


def _cloud_of(o):
    return {"rows": o["rows"].cpu().numpy(), "counts": o["counts"].cpu().numpy(), "fill": FILL}


def _assert_every_kind(o, want, what):
    """The other output kinds of a compaction (gathered points, labels, in-pose indices, |point| from the world origin)."""
    K, N = len(want["rows"]), want["N"]
    keep = want["keep"]
    assert_bit_equal(o["p3"][:K].cpu().numpy(), want["point3"][keep], f"{what}: gathered points")
    assert np.array_equal(o["sem"][:K].cpu().numpy().view(np.uint16), want["sem"][keep]), f"{what}: gathered sem"
    assert np.array_equal(o["ins"][:K].cpu().numpy().view(np.uint16), want["ins"][keep]), f"{what}: gathered ins"
    assert np.array_equal(o["idx"][:K].cpu().numpy().view(np.uint32), (np.flatnonzero(keep) % N).astype(np.uint32)), \
        f"{what}: in-pose indices"
    assert_bit_equal(o["rng"][:K].cpu().numpy(), np.linalg.norm(want["point3"][keep], axis=1), f"{what}: range from the origin")


def _plain(c3, poses, max_range, want, what):
    """lrc_scan_poses_dev + lrc_compact_dev of these poses: all records, counts, rows, rows beyond the kept ones."""
    from test_pipe_edges_gpu import Reference
    ref = Reference(c3["scene"], len(poses) * c3["N"])
    o = ref.run(_device(poses), c3["d_dirs"], max_range, every_kind=True)
    got = _records_of_hits(ref.hits)
    got.update(_cloud_of(o))
    n = fp.assert_scan_equal(got, want, what)
    _assert_every_kind(o, want, what)
    tc = ref.hits["tile_count"].cpu().numpy()
    assert np.array_equal(tc, want["keep"].reshape(-1, 64).sum(1)), f"{what}: per-tile keep counts"
    return n


# ---- a. C3, plain device path -------------------------------------------------------------------------------------------
def test_c3_plain_device_path_every_ray(c3):
    import bench
    want = fp.c3_expected()
    assert want["keep"].mean() > 0.999
    n = _plain(c3, bench.c3_poses(0, 1), c3["sensor"].max_range, want, "C3 plain device path")
    assert n == C3_RAYS
    fp.report("2a C3 plain device path (lrc_scan_poses_dev + lrc_compact_dev)", want, rays=n)


# ---- b. C3, the scan pipeline as bench.py drives it -----------------------------------------------------------------------
def _shifted_c3(c3, s):
    """The C3 line moved by 3 cm per submit in y, and what the oracle says of it."""
    import bench
    poses = bench.c3_poses(0, 1).copy()
    if s == 0:
        return poses, fp.c3_expected()
    poses[:, 1, 3] += 0.03 * s
    return poses, fp.expected_sensor_scan(c3["om"], c3["mesh"], c3["sensor"], poses)


def test_c3_scan_pipeline_every_ray_of_every_submit(c3):
    """Six lrc_pipe_submit calls back to back over three rotating row buffers, rows-only and every-output-kind submits
    alternating (the multi-tile and the per-tile scatter), lrc_pipe_wait after the third and after the last.  A caller's
    rows are complete only once its stream has passed a wait, so three submits lie between two waits: each of the three
    buffers is then read, compared and handed to the next three submits.  Every submit scans its own poses, so rows left
    over from an earlier scan cannot pass.  The lean record sets still in the four-set window (the last four submits),
    expanded by lrc_pipe_records, meet the oracle's records."""
    import torch
    import lidarcast
    from test_pipe_edges_gpu import outputs
    P, N, scene, sensor = 64, c3["N"], c3["scene"], c3["sensor"]
    st = torch.cuda.current_stream().cuda_stream
    pipe = lidarcast.ScanPipe(scene, P, N)
    bufs = [outputs(P, N, every_kind=j % 2 == 1) for j in range(3)]     # submit s uses buffer s % 3: kinds alternate too
    wants, tickets, keepalive = [], [], []
    compared = 0

    def check(group):
        nonlocal compared
        for s in group:
            o, _ = bufs[s % 3]
            n = fp.assert_scan_equal(_cloud_of(o), wants[s], f"pipeline submit {s}", fields=fp.CLOUD)
            if "p3" in o:
                _assert_every_kind(o, wants[s], f"pipeline submit {s}")
            assert wants[s]["keep"].mean() > 0.999
            fp.report(f"2b pipeline submit {s} ({'every output kind' if 'p3' in o else 'rows only'})", wants[s], rays=n)
            compared += n
            o["rows"].fill_(FILL)
            o["counts"].fill_(-1)

    for s in range(6):
        poses, want = _shifted_c3(c3, s)
        wants.append(want)
        d_poses = _device(poses)
        keepalive.append(d_poses)
        tickets.append(pipe.submit(d_poses, c3["d_dirs"], sensor.max_range, io=bufs[s % 3][1], stream=st))
        if s in (2, 5):
            pipe.wait(st)
            torch.cuda.synchronize()
            check(range(s - 2, s + 1))
    for a, b in zip(wants, wants[1:]):
        assert not np.array_equal(a["rows"][:1000], b["rows"][:1000])         # the submits do scan different poses
    for s in range(2, 6):
        got = _records_of_pointers(pipe.records(tickets[s]), P * N)
        fp.assert_scan_equal(got, wants[s], f"records of pipeline submit {s}", fields=fp.RECORDS)
    pipe.close()
    assert compared == 6 * C3_RAYS
    print(f"[full parity] 2b pipeline: {compared} rays in 6 submits, records of the last 4 submits, rays that differ 0")


# ---- c. C3, sharded pipeline --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3_two_ranks(c3):
    """All 2 x 64 poses of the two-rank C3 job, slab after slab, and the oracle's scene cloud."""
    import bench
    poses = np.concatenate([bench.c3_poses(r, 2) for r in range(2)])
    return poses, fp.expected_sensor_scan(c3["om"], c3["mesh"], c3["sensor"], poses)


@pytest.mark.parametrize("own", [0, 1], ids=["own-first", "own-last"])
def test_c3_sharded_pipeline_every_ray_of_every_step(c3, c3_two_ranks, own):
    from test_pipe_edges_gpu import Sharded
    poses, want = c3_two_ranks
    d_poses = _device(poses)

    class C3Ranks(Sharded):
        def poses_of_step(self, j):
            return d_poses

    r = C3Ranks(c3["scene"], c3["sensor"], 64, W=2, own=own, lag=2)
    assert r.N == c3["N"]
    r.run(steps=4)
    assert want["keep"].mean() > 0.999 and len(r.steps) == 4
    for j, s in enumerate(r.steps):
        n = fp.assert_scan_equal({"rows": s["cloud"].cpu().numpy(), "counts": s["counts"].cpu().numpy(), "fill": FILL},
                                 want, f"sharded step {j}, own slab {own}", fields=fp.CLOUD)
        assert n == 2 * C3_RAYS
        fp.report(f"2c sharded pipeline W 2 own slab {own} step {j}", want, rays=n)
    r.pipe.close()


# ---- d. rotated, close and range-cut poses ------------------------------------------------------------------------------
def _random_poses():
    """16 poses: any orientation, anywhere in the room down to 5 cm from its walls, floor and ceiling."""
    rng = np.random.default_rng(11)
    try:
        from scipy.spatial.transform import Rotation
        R = Rotation.random(16, random_state=rng).as_matrix()
    except ImportError:
        from test_configs_gpu import _rot
        R = np.stack([_rot(*rng.uniform(-np.pi, np.pi, 3)) for _ in range(16)])
    poses = np.tile(np.eye(4), (16, 1, 1))
    poses[:, :3, :3] = R
    poses[:, :3, 3] = rng.uniform([0.05, 0.05, 0.05], [4.95, 3.95, 2.95], size=(16, 3))
    return poses


def test_rotated_close_and_range_cut_poses_every_ray(c3, engine):
    import torch
    import lidarcast
    from test_pipe_edges_gpu import outputs
    poses = _random_poses()
    P, N = 16, c3["N"]
    short = dataclasses.replace(c3["sensor"], max_range=1.5)
    want = fp.expected_sensor_scan(c3["om"], c3["mesh"], short, poses)
    share = want["keep"].reshape(P, N).mean(1)
    assert 0.3 < share.mean() < 0.8, share                    # the strict filter decides a large share of the rays
    n = _plain(c3, poses, 1.5, want, "random poses, plain device path")
    assert n == P * N == 1048576
    fp.report("2d random poses max_range 1.5, plain device path", want, rays=n)
    # one pipeline submit of the same poses: rows, counts, the expanded lean records
    st = torch.cuda.current_stream().cuda_stream
    pipe = lidarcast.ScanPipe(c3["scene"], P, N)
    o, io = outputs(P, N, every_kind=False)
    d_poses = _device(poses)
    ticket = pipe.submit(d_poses, c3["d_dirs"], 1.5, io=io, stream=st)
    pipe.wait(st)
    torch.cuda.synchronize()
    got = _records_of_pointers(pipe.records(ticket), P * N)
    got.update(_cloud_of(o))
    n = fp.assert_scan_equal(got, want, "random poses, pipeline submit")
    pipe.close()
    fp.report("2d random poses max_range 1.5, one pipeline submit", want, rays=n)
    # the same poses at 25 m through the host-facing engine.scan_poses
    far = dataclasses.replace(c3["sensor"], max_range=25.0)
    want = fp.expected_sensor_scan(c3["om"], c3["mesh"], far, poses)
    assert want["keep"].mean() > 0.999
    rec, n_rays = engine.scan_poses(far, poses, c3["mesh"], want=fp.RECORDS)
    assert n_rays == N
    n = fp.assert_scan_equal(rec, want, "random poses, engine.scan_poses", fields=fp.RECORDS)
    fp.report("2d random poses max_range 25, engine.scan_poses", want, rays=n)


# ---- e. moving-sensor sweeps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["realistic", "extreme"])
def test_sweeps_every_ray_against_the_oracle(ctx, motion):
    """8 sweeps of the 32 x 2048 sensor on synth_A1_office: the restated rays (tests/sweep_restate.py) cast by the oracle,
    with one range-filter centre per column, against lrc_scan_sweeps_dev."""
    import lidarcast
    from helpers import sensor_32x2048
    from lidar import IndoorLidar
    from lidarcast import motion_records
    from sweep_restate import sweep_rays
    from test_sweep_gpu import MOTIONS, _dev, _sweeps
    name = "synth_A1_office"
    mesh, om = fp.scene_and_oracle(name)
    k = sensor_32x2048()
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    starts, ends = _sweeps(name, 8, *MOTIONS[motion])
    rec = motion_records(starts, ends)
    rays, centres = sweep_rays(rec, dirs, fire)
    want = fp.expected_scan(om, rays, centres, k.max_range, 8, mesh.triangle_sem, mesh.triangle_ins)
    assert want["keep"].mean() > 0.5
    static = np.concatenate([IndoorLidar(k, m).get_rays() for m in starts])
    assert (rays[:, 3:] != static[:, 3:]).mean() > 0.5          # the motion is real
    scene = lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    got = _dev(scene, rec, dirs, fire, k.max_range, want=fp.RECORDS)
    n = fp.assert_scan_equal(got, want, f"sweeps, {motion}", fields=fp.RECORDS)
    scene.close()
    assert n == 524288
    fp.report(f"2e sweeps {motion} (lrc_scan_sweeps_dev)", want, rays=n)


# ---- f. the host-facing compact entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["on demand", "eager"])
def test_run_simulation_every_frame_of_c3(c3, engine, labels):
    """S3DISSimulator.run_simulation (lrc_scan_poses_compact) on C3: points, semantic and instance labels of all 64 frames,
    with the labels fetched on demand (the default: a second, labels-only scan) and brought with the points."""
    from s3dis_simulator import S3DISSimulator
    from trajectory import line_trajectory
    want = fp.c3_expected()
    config = {"raycast_engine": {"use_gpu": True, "eager_labels": labels == "eager"}}
    sim = S3DISSimulator(config)
    sim.raycast_engine = engine
    sim.lidar_config = c3["sensor"]
    sim.load_scene(c3["mesh"], "c3")
    scene = sim.run_simulation(line_trajectory((1.0, 2.0, 1.0), (4.0, 2.0, 1.0), 64))
    assert scene.get_total_frames() == 64 and want["keep"].mean() > 0.999
    counts = np.array([len(f.points) for f in scene.frames], dtype=np.int64)
    rows = np.empty((int(counts.sum()), 4), np.float32)
    rows[:, :3] = np.concatenate([f.points for f in scene.frames])
    rows[:, 3] = fp.pack_labels(np.concatenate([f.semantic_labels for f in scene.frames]),
                                np.concatenate([f.instance_labels for f in scene.frames]))
    n = fp.assert_scan_equal({"rows": rows, "counts": counts}, want, f"run_simulation, labels {labels}", fields=fp.CLOUD)
    assert n == C3_RAYS
    fp.report(f"2f S3DISSimulator.run_simulation, labels {labels}", want, rays=n)
