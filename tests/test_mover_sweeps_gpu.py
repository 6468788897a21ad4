"""-m gpu: movers under moving-sensor sweeps (lrc_scan_mover_sweeps_dev / lrc_scan_mover_sweeps_compact: the sweep ray kernel,
the explicit-ray launch per mover, the sweep merge kernel).

The comparator is the composition the feature is defined by (tests/mover_sweep_restate.py, compose_host): gen_ray_sweep's rays
from the sweep restatement (tests/sweep_restate.py), the library's host step lidarcast.movers.sweep_rays, the EXISTING
explicit-ray cast per mover on the GPU (Scene.cast, no centre, no filter, which never culls), sweep_normals and merge on the
host, and the write-back restatement with the sweep's per-ray centres.  Every column must agree bit for bit -- t, prim, normal3,
point3, sem, ins, intensity and the mover column -- except incident_deg, where the device's acos meets libm's on identical
inputs: rtol 1e-13, as in tests/test_movers_gpu.py.

Shapes: N in {40, 64, 200} rays per sweep (64: a wave lies in one sweep and the records come through the scalar cache; 40 and
200: they do not), P in {1, 3} sweeps, M in {1, 3} movers; no P * N is a multiple of the block of 256.

The physical check of tests/test_mover_sweeps_host.py runs again on the GPU's output, with the bound measured there."""
import json

import numpy as np
import pytest

import mover_restate as mv
import mover_sweep_restate as ms
import sweep_restate
from helpers import aimed_pose, beam_table
from test_mover_sweeps_host import BOUND_ON_BOX
from test_movers_gpu import HITS, _views, assert_bit_equal, assert_records, cast_of, labelled, scene_of

pytestmark = pytest.mark.gpu

TARGET = (2.5, 2.0, 0.9)
WIDTH = {40: 10, 64: 16, 200: 50}          # four lines each


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


class World:
    """The room, the three mover meshes (a 12-triangle box, a pedestrian, a small cube), a set of all three and one of the box."""


@pytest.fixture(scope="module")
def world(engine):
    from lidarcast import synth
    from lidarcast.movers import MoverSet
    w = World()
    w.ctx = engine.ctx
    w.room = mv.room_mesh()
    w.meshes = [ms.box_mover(13, 77), synth.make_pedestrian(semantic=13, instance=1001), labelled(synth.unit_cube(-0.3, 0.3), 12, 1002)]
    w.scene = scene_of(w.ctx, w.room)
    w.sets = {3: MoverSet(w.ctx, w.meshes), 1: MoverSet(w.ctx, w.meshes[:1])}
    w.casts = [cast_of(s) for s in w.sets[3].scenes]
    w.static = cast_of(w.scene)
    yield w
    for s in w.sets.values():
        s.close()
    w.scene.close()


def inputs(N, P, moving=True):
    """A narrow table of four lines x N / 4 columns about the sensor's -x axis, the firing fractions (column / width), P sweeps
    that look at TARGET from 1.5 m while the sensor moves 0.12 m and turns 0.05 rad (or stands still), and the world rays and
    centres of the sweep restatement."""
    from lidarcast import motion_records
    W = WIDTH[N]
    dirs = beam_table([18.0, 4.0, -10.0, -24.0], W, 40.0)
    fire = (np.arange(N) % W) / W
    yaws = (0.3, -1.0, 2.2)[:P]
    start = np.stack([aimed_pose(TARGET, 1.5, yaw=y) for y in yaws])
    end = start.copy()
    if moving:
        for p, y in enumerate(yaws):
            end[p] = aimed_pose(TARGET, 1.5, yaw=y + 0.05)
            end[p, :3, 3] = start[p, :3, 3] + (0.08, -0.09, 0.02)
    motion = motion_records(start, end)
    rays, cen = sweep_restate.sweep_rays(motion, dirs, fire)
    return dirs, fire, start, motion, rays, cen


def mover_records(P, M, moving=True):
    """the box crossing in front of TARGET, the pedestrian walking and turning behind it, the cube turning a quarter at chest height"""
    out = np.zeros((P, 3, 24), np.float32)
    for p in range(P):
        if moving:
            out[p, 0] = ms.record24(2.1 + 0.2 * p, 1.8, 0.0, 0.2 + p, 0.5, 0.3, 0.0, 0.3)
            out[p, 1] = ms.record24(2.9, 2.4 - 0.2 * p, 0.0, -0.7, -0.1, 0.1, 0.0, -0.4)
            out[p, 2] = ms.record24(2.5, 2.0, 1.0, 0.3 + p, 0.0, 0.0, 0.2, np.pi / 2)
        else:
            out[p, 0] = ms.still_record(mv.pose12(2.1 + 0.2 * p, 1.8, 0.0, 0.2 + p))
            out[p, 1] = ms.still_record(mv.pose12(2.9, 2.4 - 0.2 * p, 0.0, -0.7))
            out[p, 2] = ms.still_record(mv.pose12(2.5, 2.0, 1.0, 0.3 + p))
    return np.ascontiguousarray(out[:, :M])


def sweeps_dev(scene, mset, motion, dirs, fire, records, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    from lidarcast.movers import scan_mover_sweeps_dev
    P, N = len(motion), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    rt = None if records is None else torch.from_numpy(np.ascontiguousarray(records, np.float32)).cuda()
    scan_mover_sweeps_dev(scene, torch.from_numpy(np.ascontiguousarray(motion)).cuda(), torch.from_numpy(np.ascontiguousarray(dirs)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(fire)).cuda(), hits, max_range, mset, rt, mover_t=who)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["mover"] = who.cpu().numpy()
    return out


def plain_sweeps_dev(scene, motion, dirs, fire, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(motion), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    scene.scan_sweeps_dev(torch.from_numpy(np.ascontiguousarray(motion)).cuda(), torch.from_numpy(np.ascontiguousarray(dirs)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(fire)).cuda(), hits, max_range)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


# ---- 1: parity with the composition -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N", [40, 64, 200])
def test_parity_with_the_composition(world, N, P, M):
    dirs, fire, _, motion, rays, cen = inputs(N, P)
    rec = mover_records(P, M)
    assert (P * N) % 256 != 0 and (N % 64 == 0) == (N == 64)
    want, win = ms.compose_host(world.static, world.casts[:M], rays, cen, fire, rec, N, 2.2)
    wins = np.bincount(want["mover"], minlength=M + 1)
    filtered = int(((win["t"] < np.inf) & ~want["keep"]).sum())
    print(f"\n[mover sweeps] N {N}, P {P}, M {M}: room / movers win {wins.tolist()} rays, the filter removes {filtered}")
    assert wins[0] > 0 and wins[1:].sum() > 0 and filtered > 0
    if N == 200:
        assert (wins > 0).all()
    got = sweeps_dev(world.scene, world.sets[M], motion, dirs, fire, rec, 2.2)
    assert_records(got, want, f"N {N}, P {P}, M {M}")


def test_incident_mode_1_uses_the_turned_normal(world):
    dirs, fire, _, motion, rays, cen = inputs(200, 3)
    rec = mover_records(3, 3)
    want, _ = ms.compose_host(world.static, world.casts, rays, cen, fire, rec, 200, 20.0, incident_mode=1)
    try:
        world.scene.set_options(incident_mode=1)
        got = sweeps_dev(world.scene, world.sets[3], motion, dirs, fire, rec, 20.0)
    finally:
        world.scene.reset_options()
    assert (want["mover"] > 0).sum() > 100
    assert_records(got, want, "incident_mode 1")


# ---- 2: identities ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 200])
def test_a_null_set_is_the_sweep_scan(world, N):
    dirs, fire, _, motion, _, _ = inputs(N, 3)
    clean = plain_sweeps_dev(world.scene, motion, dirs, fire, 2.2)
    got = sweeps_dev(world.scene, None, motion, dirs, fire, None, 2.2)
    assert not got["mover"].any() and (clean["t"] < np.inf).sum() > 40
    for a in HITS:
        assert_bit_equal(got[a], clean[a], f"NULL set, N {N}: {a}")


@pytest.mark.parametrize("N", [64, 200])
def test_all_standing_still_is_the_mover_scan(world, N):
    """a sensor that does not move and movers with still records: the bytes of lrc_scan_movers_dev, for every firing fraction"""
    from test_movers_gpu import movers_dev
    dirs, fire, start, motion, _, _ = inputs(N, 3, moving=False)
    rec = mover_records(3, 3, moving=False)
    assert all(ms.still(r) for r in rec.reshape(-1, 24))
    frozen = movers_dev(world.scene, world.sets[3], start, dirs, np.ascontiguousarray(rec[:, :, :12]), 2.2)
    got = sweeps_dev(world.scene, world.sets[3], motion, dirs, fire, rec, 2.2)
    assert (np.bincount(frozen["mover"], minlength=4) > 0).all()
    for a in HITS + ("mover",):
        assert_bit_equal(got[a], frozen[a], f"all still, N {N}: {a}")


def test_a_copy_of_the_room_never_wins(world):
    """the room's copy at the identity with a still record meets every ray at the room's own float32 range: the room keeps the tie"""
    from lidarcast.movers import MoverSet
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    rec = np.tile(ms.still_record(mv.pose12(0.0, 0.0, 0.0, 0.0)), (3, 1, 1))
    copy = MoverSet(world.ctx, [labelled(world.room, 99, 9999)])
    try:
        clean = plain_sweeps_dev(world.scene, motion, dirs, fire, 20.0)
        got = sweeps_dev(world.scene, copy, motion, dirs, fire, rec, 20.0)
        assert not got["mover"].any() and 99 not in got["sem"] and (clean["t"] < np.inf).sum() > 500
        for a in HITS:
            assert_bit_equal(got[a], clean[a], f"copy of the room: {a}")
    finally:
        copy.close()


# ---- 3: min_range -------------------------------------------------------------------------------------------------------------------

def test_min_range_does_not_uncover_the_room(world):
    """min_range 1.4 m removes the near returns of the box that crosses 1 m in front of the sensor; the room behind them stays
    hidden (no return at all), and the room is returned where the box is not in the way."""
    dirs, fire, _, motion, rays, cen = inputs(200, 3)
    rec = mover_records(3, 1)
    want, win = ms.compose_host(world.static, world.casts[:1], rays, cen, fire, rec, 200, 20.0, min_range=1.4)
    removed = (win["mover"] == 1) & ~want["keep"]
    room_behind = np.concatenate([world.static(rays[p * 200:(p + 1) * 200])["t"] for p in range(3)])
    print(f"\n[mover sweeps] min_range: {int(removed.sum())} near returns of the box are removed, "
          f"{int((removed & (room_behind < np.inf)).sum())} of them with the room behind")
    assert (removed & (room_behind < np.inf)).sum() >= 20 and np.isinf(want["t"][removed]).all() and not want["mover"][removed].any()
    assert (want["keep"] & (want["mover"] == 0)).sum() > 100
    try:
        world.scene.set_options(min_range=1.4)
        got = sweeps_dev(world.scene, world.sets[1], motion, dirs, fire, rec, 20.0)
    finally:
        world.scene.reset_options()
    assert_records(got, want, "min_range")


# ---- 4: the compact call and the frames ----------------------------------------------------------------------------------------------

def test_compact_call_and_frames_are_the_dev_call(engine, world):
    from lidarcast.movers import scan_mover_sweeps_compact
    from test_movers_gpu import FRAMES, assert_frames_equal, host_frames
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    rec = mover_records(3, 3)
    dev = sweeps_dev(world.scene, world.sets[3], motion, dirs, fire, rec, 2.2)
    want = host_frames(dev, 3, 200)
    assert (np.bincount(want["mover"], minlength=4) > 0).all() and 0 < want["counts"].sum() < 600
    fr = scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, world.sets[3], rec, want=FRAMES)
    assert_frames_equal(fr, want, "compact")
    none = scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, None, None, want=FRAMES)
    clean = world.scene.scan_sweeps_compact(motion, dirs, fire, 2.2, want=FRAMES)
    assert none["counts"].tolist() == clean["counts"].tolist() and not none["mover"].any() and len(none["mover"]) == clean["total"]
    for a in FRAMES:
        assert_bit_equal(none[a], clean[a], f"NULL set, compact: {a}")
    # what the compact call checks on the host
    bad = rec.copy()
    bad[1, 0, 17] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, world.sets[3], bad)
    bad = rec.copy()
    bad[2, 1, 0] += np.float32(2.0 ** -12)
    with pytest.raises(ValueError, match="no rotation"):
        scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, world.sets[3], bad)
    bad = rec.copy()
    bad[0, 2, 12:16] = [np.cos(0.8), 0.0, 0.0, np.sin(0.8)]
    with pytest.raises(ValueError, match="more than pi/2 per sweep"):
        scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, world.sets[3], bad)
    with pytest.raises(ValueError, match=r"\(P, M, 24\)"):
        scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, world.sets[3], rec[:2])
    import torch
    noise = torch.zeros(600, dtype=torch.float32, device="cuda")
    try:
        world.scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match="range_noise"):
            scan_mover_sweeps_compact(world.scene, motion, dirs, fire, 2.2, world.sets[3], rec)
    finally:
        world.scene.reset_options()


def test_engine_frames_carry_times_movers_and_labels(engine, world):
    """the engine's sensor: point_times, mover and the labels have one entry per kept row and belong together"""
    from helpers import sensor_small
    from lidarcast.movers import MoverSet, scan_mover_sweep_frames
    k = sensor_small(lines=4, width=64, max_range=6.0)
    start = np.stack([aimed_pose(TARGET, 1.5, yaw=y) for y in (0.3, -1.0)])
    end = start.copy()
    end[:, :3, 3] += (0.08, -0.09, 0.02)
    rec = mover_records(2, 3)
    mset = MoverSet(engine.ctx, world.meshes)
    try:
        fr = scan_mover_sweep_frames(engine, k, start, end, world.room, mset, rec, want=("point3", "sem", "ins", "index"))
        motion, fire, T = engine.sweep_inputs(k, start, end)
        from lidar import IndoorLidar
        dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
        dev = sweeps_dev(engine.scene_for(world.room), mset, motion, dirs, fire, rec, k.max_range)
    finally:
        mset.close()
    keep = dev["t"] != np.inf
    K = int(keep.sum())
    assert fr["total"] == K == len(fr["point_times"]) == len(fr["mover"]) == len(fr["sem"]) == len(fr["ins"]) == len(fr["point3"])
    assert_bit_equal(fr["point3"], dev["point3"][keep], "frames: point3")
    assert_bit_equal(fr["mover"], dev["mover"][keep], "frames: mover")
    assert_bit_equal(fr["ins"], dev["ins"][keep], "frames: ins")
    assert np.array_equal(fr["point_times"], fire[fr["index"]] * T) and T == 1.0 / k.scan_frequency
    assert (fr["ins"][fr["mover"] == 1] == 77).all() and (fr["ins"][fr["mover"] == 2] == 1001).all()
    assert (fr["ins"][fr["mover"] == 3] == 1002).all() and (np.bincount(fr["mover"], minlength=4) > 0).all()
    with pytest.raises(NotImplementedError, match="direction table"):
        scan_mover_sweep_frames(engine, object(), start, end, world.room, None, None)


# ---- 5: the simulator end to end ------------------------------------------------------------------------------------------------------

def test_simulator_nested_key(world, tmp_path):
    import s3dis_simulator
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 4, yaw=0.6)
    key = {"period": 0.1, "objects": [
        {"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.4, 3.3, 1.4, 0.0, 140.0]]},
        {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]}]}
    sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}, "motion": {"speed": 0.5, "movers": key}})
    sim.load_scene(world.room, "room")
    out = sim.run_simulation(wps)
    assert out.get_total_frames() == 4
    tracks = out.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "room_mover_tracks.json"))
    assert disk == json.loads(json.dumps(tracks)) and disk["num_frames"] == 4
    T = 1.0 / sim.lidar_config.scan_frequency
    seen = np.zeros(3, np.int64)
    for f, fr in enumerate(out.frames):
        ids = fr.mover_ids
        assert ids.dtype == np.uint8 and len(ids) == len(fr.points) == len(fr.point_times) == len(fr.semantic_labels) > 0
        assert fr.point_times.min() >= 0.0 and fr.point_times.max() < T
        counts = np.bincount(ids, minlength=3)
        seen += counts
        assert (fr.semantic_labels[ids == 1] == 13).all() and (fr.instance_labels[ids == 1] == 1001).all()
        assert (fr.semantic_labels[ids == 2] == 12).all() and (fr.instance_labels[ids == 2] == 1002).all()
        d = disk["frames"][f]
        assert d["sweep_duration"] == T and np.isclose(d["time"], 0.1 * f) and d["static_points"] == counts[0]
        assert [m["num_points"] for m in d["movers"]] == counts[1:].tolist()
        walker, post = d["movers"]
        u0, u1 = 0.1 * f / 0.4, min((0.1 * f + T) / 0.4, 1.0)
        assert np.allclose([walker["pose"]["x"], walker["pose"]["yaw_deg"]], [1.8 + 1.5 * u0, 20.0 + 120.0 * u0])
        assert np.allclose([walker["end_pose"]["x"], walker["end_pose"]["yaw_deg"]], [1.8 + 1.5 * u1, 20.0 + 120.0 * u1])
        assert post["end_pose"] == {k: post["pose"][k] for k in ("x", "y", "z", "yaw_deg")} and post["record24"][12] == 1.0
    assert (seen > 0).all(), seen


# ---- 6: the physical check on the GPU's output ----------------------------------------------------------------------------------------

def test_points_on_a_moving_box_lie_on_the_box_at_their_own_time(world):
    from lidarcast.movers import MoverTrack, sweep_records
    k, dirs, fire, motion, path = ms.crossing_inputs()
    rec = sweep_records([MoverTrack(path)], [0.0], [ms.SWEEP_T])
    got = sweeps_dev(world.scene, world.sets[1], motion, dirs, fire, rec, k.max_range)
    on = got["mover"] == 1
    s = fire[np.flatnonzero(on) % len(dirs)]
    own = ms.box_distance(got["point3"][on], s, rec[0, 0])
    frozen = ms.box_distance(got["point3"][on], np.zeros(int(on.sum())), rec[0, 0])
    print(f"\n[mover sweeps] GPU: {int(on.sum())} of {len(on)} rays end on the box; by the pose at their own time they lie within "
          f"{own.max():.3e} m of its surface (bound {BOUND_ON_BOX:.3e} m), by the sweep-start pose within {frozen.max():.3f} m")
    assert on.sum() >= 50
    assert own.max() <= BOUND_ON_BOX
    assert frozen.max() > 0.1
