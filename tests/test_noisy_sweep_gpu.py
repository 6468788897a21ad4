"""-m gpu: seeded sensor noise under moving-sensor sweeps (lrc_scan_noisy_sweeps_dev / lrc_scan_noisy_sweeps_compact, GEN = 8 of
the trace kernel).

The noisy sweep rays are restated on the host (tests/noisy_sweep_restate.py: the composition of the noise and the sweep
restatements) and cast through the explicit-ray path with one segment per (frame, column) about its centre c(s), dropped rays as
NaN directions and the range term as the ``range_noise`` option: the in-kernel generator must give the same bytes.  The all-zero
model must give the bytes of the clean sweeps; static records and a zero fire table the bytes of the static noisy scan; the noise
of a frame must not depend on which call scans it; the simulator switches to it only with the nested ``motion: {noise: ...}``
key."""
import numpy as np
import pytest

import noise_restate as nr
from helpers import assert_bit_equal, sensor_32x2048, sensor_small
from noisy_sweep_restate import noisy_sweep_rays
from test_noise_gpu import _table
from test_sweep_gpu import FRAMES, HITS, MOTIONS, _assert_frames_equal, _host_frames

pytestmark = pytest.mark.gpu

NAME = "synth_A1_office"
SEED = 0xC0FFEE123456789


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


@pytest.fixture(scope="module")
def mesh():
    from lidarcast import synth
    return synth.make_scene(NAME)


@pytest.fixture(scope="module")
def tab():
    from lidarcast import noise
    return noise.table()


def _line_sweeps(a, b, P, speed, turn, freq=10.0, yaw=0.3):
    """(start poses, end poses) of P sweeps on the line a -> b, ``speed`` m/s, ``turn`` rad/s."""
    from trajectory import line_trajectory, poses_from_waypoints, sweep_end_poses
    wps = line_trajectory(a, b, P + 1, yaw=yaw)
    for w in wps:
        w.angular_velocity = turn
    return poses_from_waypoints(wps)[:P], sweep_end_poses(wps, freq, speed)[:P]


def _sweeps(P, speed, turn, near_wall=False):
    """Through the middle of the room, as tests/test_sweep_gpu.py; ``near_wall``: 0.3 m from the wall y = 0."""
    from lidarcast import synth
    Lx, Ly, _ = synth.scene_size(NAME)
    if near_wall:
        return _line_sweeps((1.0, 0.3, 1.0), (Lx - 1.0, 0.35, 1.2), P, speed, turn)
    return _line_sweeps((1.0, Ly / 2 - 0.3, 1.0), (Lx - 1.0, Ly / 2 + 0.3, 1.2), P, speed, turn)


def _fire(dirs, W):
    return (np.arange(len(dirs)) % W) / W


def _views(out):
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


def _dev(scene, rec, dirs, fire, model, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits, noise
    hits = DeviceHits(len(rec) * len(dirs), "cuda", want=want)
    noise.scan_noisy_sweeps_dev(scene, torch.from_numpy(np.ascontiguousarray(rec)).cuda(),
                                torch.from_numpy(np.ascontiguousarray(dirs)).cuda(),
                                torch.from_numpy(np.ascontiguousarray(fire, dtype=np.float64)).cuda(), hits, max_range, model)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def _sweeps_dev(scene, rec, dirs, fire, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    hits = DeviceHits(len(rec) * len(dirs), "cuda", want=want)
    scene.scan_sweeps_dev(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), torch.from_numpy(np.ascontiguousarray(dirs)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(fire, dtype=np.float64)).cuda(), hits, max_range)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def _noisy_dev(scene, poses, dirs, model, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P = len(poses)
    hits = DeviceHits(P * len(dirs), "cuda", want=want)
    scene.scan_noisy_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                         torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range, model)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def _explicit(scene, rec, dirs, fire, W, model, max_range, tab, min_range=0.0, incident_mode=0, ranged=True, want=HITS):
    """The restated noisy sweep rays through lrc_cast_segments, one segment per (frame, column) about c(s), the range term as
    the range_noise option (``ranged`` False: without it), back in (frame, ray) order -- the permutation of
    tests/test_sweep_gpu.py ``_explicit``."""
    rays, cen, term, keep, rows = noisy_sweep_rays(rec, dirs, fire, model, *tab)
    P, N = len(rec), len(dirs)
    H = N // W
    perm = (np.arange(P)[:, None, None] * N + np.arange(H)[None, None, :] * W + np.arange(W)[None, :, None]).reshape(-1)
    off = np.arange(0, P * N + 1, H, dtype=np.uint64)
    try:
        scene.set_options(min_range=min_range, range_noise=term[perm] if ranged and model.range_std != 0 else None,
                          incident_mode=incident_mode)
        out = scene.cast_segments(rays[perm], off, cen[perm][::H], max_range, want=want)
    finally:
        scene.reset_options()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return {k: v[inv] for k, v in out.items()}, dict(rays=rays, term=term, keep=keep, rows=rows)


# name: (lines, width, first_frame, range_std, angle_std, dropout, max_range, min_range, incident_mode, near_wall)
CASES = {
    "4x100, P = 3": (4, 100, 0, 0.02, 0.01, 0.05, 20.0, 0.0, 0, False),
    "4x96, frame ids carry into the high word": (4, 96, 2 ** 32 - 1, 0.02, 0.01, 0.05, 20.0, 0.0, 0, False),
    "max_range 2.2, min_range 0.9, normal incidence": (4, 100, 3, 0.02, 0.01, 0.05, 2.2, 0.9, 1, False),
    "range_std 0.5 close to a wall": (4, 96, 0, 0.5, 0.002, 0.02, 20.0, 0.0, 0, True),
}


@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("case", list(CASES))
def test_noisy_sweeps_bit_exact_against_explicit_rays(engine, mesh, tab, case, motion):
    from lidar import IndoorLidar
    from lidarcast import motion_records, noise
    lines, width, first, rs, sa, dr, max_range, min_range, inc_mode, near = CASES[case]
    dirs = _table(lines, width)
    fire = _fire(dirs, width)
    P, N = 3, len(dirs)
    starts, ends = _sweeps(P, *MOTIONS[motion], near_wall=near)
    rec = motion_records(starts, ends)
    scene = engine.scene_for(mesh)
    model = noise.NoiseModel(seed=SEED, range_std=rs, angle_std=sa, dropout=dr, first_frame=first)
    ref, aux = _explicit(scene, rec, dirs, fire, width, model, max_range, tab, min_range, inc_mode)
    # the case exercises what it is for: read from the explicit-path reference and the restatement alone
    what = f"{case} {motion}"
    hit = np.isfinite(ref["t"])
    assert 0.05 < hit.mean() < 1.0, what
    assert 0 < (~aux["keep"]).sum() < 0.2 * P * N, what
    static = nr.noisy_rays(starts, dirs, model.seed, model.first_frame, rs, sa, dr, *tab)[0]
    assert (aux["rays"][aux["keep"]][:, 3:] != static[aux["keep"]][:, 3:]).any(), what
    if near:       # returns lost to a non-positive noisy range: returns of the same rays without the term that are gone with it
        bare, _ = _explicit(scene, rec, dirs, fire, width, model, max_range, tab, min_range, inc_mode, ranged=False, want=("t",))
        lost = np.isfinite(bare["t"]) & ~hit
        print(f"\n[noisy sweep] {what}: {int(lost.sum())} returns of the reference lost to t' <= 0")
        assert ((bare["t"] + aux["term"])[lost] <= 0).all()
        assert lost.sum() >= 5
    try:
        scene.set_options(min_range=min_range, incident_mode=inc_mode)
        got = _dev(scene, rec, dirs, fire, model, max_range)
        fr = noise.scan_noisy_sweeps_compact(scene, rec, dirs, fire, max_range, model, want=FRAMES)
        # the engine surface over the resident table of a real sensor record, with per-point times
        k = sensor_small(lines, width)
        lid = IndoorLidar(k, np.eye(4))
        kd, kf = lid.sensor_directions(), lid.firing_fractions()
        fr2 = noise.scan_noisy_sweep_frames(engine, k, starts, ends, mesh, model, want=FRAMES)
        got2 = _dev(scene, rec, kd, kf, model, k.max_range)
    finally:
        scene.reset_options()
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"{what}: {a}")
    _assert_frames_equal(fr, _host_frames(got, P, N), f"{what} compact")
    _assert_frames_equal(fr2, _host_frames(got2, P, N), f"{what} engine")
    assert_bit_equal(fr2["point_times"], kf[fr2["index"]] * (1.0 / k.scan_frequency))


@pytest.mark.parametrize("shape", [(3, 50), (4, 96)], ids=["3x50", "4x96"])
def test_all_zero_model_is_the_clean_sweep(engine, mesh, shape):
    from lidar import IndoorLidar
    from lidarcast import motion_records, noise
    k = sensor_small(*shape)
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    scene = engine.scene_for(mesh)
    for motion in MOTIONS:
        starts, ends = _sweeps(3, *MOTIONS[motion])
        rec = motion_records(starts, ends)
        clean = _sweeps_dev(scene, rec, dirs, fire, 3.0)
        got = _dev(scene, rec, dirs, fire, noise.NoiseModel(seed=99, first_frame=17), 3.0)
        for a in HITS:
            assert_bit_equal(got[a], clean[a], f"zero model {motion}: {a}")
        fr = noise.scan_noisy_sweeps_compact(scene, rec, dirs, fire, 3.0, noise.NoiseModel(seed=99), want=FRAMES)
        _assert_frames_equal(fr, scene.scan_sweeps_compact(rec, dirs, fire, 3.0, want=FRAMES), f"zero model {motion} compact")


@pytest.mark.parametrize("width", [100, 96])
def test_static_sweeps_are_the_static_noisy_scan(engine, mesh, width):
    from lidarcast import motion_records, noise
    dirs = _table(4, width)
    fire = _fire(dirs, width)
    N = len(dirs)
    scene = engine.scene_for(mesh)
    starts, ends = _sweeps(3, *MOTIONS["extreme"])
    model = noise.NoiseModel(seed=SEED, range_std=0.02, angle_std=0.01, dropout=0.05, first_frame=2 ** 32 - 2)
    ref = _noisy_dev(scene, starts, dirs, model, 20.0)
    ref_fr = scene.scan_noisy_compact(starts, dirs, 20.0, model, want=FRAMES)
    assert 0.05 < np.isfinite(ref["t"]).mean() < 1.0
    for what, rec, f in (("end == start", motion_records(starts, starts), fire),
                         ("zero fire table", motion_records(starts, ends), np.zeros(N))):
        got = _dev(scene, rec, dirs, f, model, 20.0)
        for a in HITS:
            assert_bit_equal(got[a], ref[a], f"4x{width} {what}: {a}")
        fr = noise.scan_noisy_sweeps_compact(scene, rec, dirs, f, 20.0, model, want=FRAMES)
        _assert_frames_equal(fr, ref_fr, f"4x{width} {what} compact")


def test_noise_does_not_depend_on_chunking(engine, mesh):
    from lidarcast import motion_records, noise
    dirs = _table(4, 100)
    fire = _fire(dirs, 100)
    scene = engine.scene_for(mesh)
    rec = motion_records(*_sweeps(6, *MOTIONS["extreme"]))
    m = noise.NoiseModel(seed=77, range_std=0.02, angle_std=0.01, dropout=0.05, first_frame=2 ** 32 - 3)
    whole = _dev(scene, rec, dirs, fire, m, 20.0)
    a = _dev(scene, rec[:2], dirs, fire, m, 20.0)
    b = _dev(scene, rec[2:], dirs, fire, m.at_frame(m.first_frame + 2), 20.0)
    for k in HITS:
        assert_bit_equal(whole[k], np.concatenate([a[k], b[k]]), f"chunks: {k}")
    want = ("point3", "index")
    fw = noise.scan_noisy_sweeps_compact(scene, rec, dirs, fire, 20.0, m, want=want)
    fa = noise.scan_noisy_sweeps_compact(scene, rec[:2], dirs, fire, 20.0, m, want=want)
    fb = noise.scan_noisy_sweeps_compact(scene, rec[2:], dirs, fire, 20.0, m.at_frame(m.first_frame + 2), want=want)
    assert fw["counts"].tolist() == fa["counts"].tolist() + fb["counts"].tolist()
    assert_bit_equal(fw["point3"], np.concatenate([fa["point3"], fb["point3"]]))
    other = _dev(scene, rec, dirs, fire, noise.NoiseModel(seed=78, range_std=0.02, angle_std=0.01, dropout=0.05), 20.0)
    assert (other["t"] != whole["t"]).mean() > 0.5


def test_large_scan_in_pose_chunks(engine, mesh):
    """More than 2^20 rays of whole 64-ray tiles: lrc_scan_noisy_sweeps_compact scans in pose chunks, each with its own records
    and first frame id, and the launch deals tiles to the XCDs in stripes -- the records of ONE launch must compact to the same
    frames."""
    from lidar import IndoorLidar
    from lidarcast import motion_records, noise
    k = sensor_32x2048()
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    P, N = 17, len(dirs)
    assert P * N >= 1 << 20 and N % 64 == 0
    rec = motion_records(*_sweeps(P, *MOTIONS["realistic"]))
    scene = engine.scene_for(mesh)
    m = noise.NoiseModel(seed=2026, range_std=0.02, angle_std=0.003, dropout=0.05, first_frame=2 ** 32 - 5)
    got = _dev(scene, rec, dirs, fire, m, k.max_range)
    hit = np.isfinite(got["t"]).mean()
    assert 0.5 < hit < 1.0
    fr = noise.scan_noisy_sweeps_compact(scene, rec, dirs, fire, k.max_range, m, want=FRAMES)
    _assert_frames_equal(fr, _host_frames(got, P, N), "large compact")


def test_float32_node_route(engine, mesh):
    """LRC_QNODES=0 on a scene of its own (tests/test_float32_node_routes_gpu.py): trace_kernel<8, ..., 0> gives the bytes of the
    quantised route."""
    import lidarcast
    from lidarcast import motion_records, noise
    dirs = _table(4, 96)
    fire = _fire(dirs, 96)
    rec = motion_records(*_sweeps(3, *MOTIONS["realistic"]))
    m = noise.NoiseModel(seed=SEED, range_std=0.02, angle_std=0.01, dropout=0.05, first_frame=2 ** 32 - 1)
    near = engine.scene_for(mesh)
    assert near.info["quantised_nodes"] == 1
    with pytest.MonkeyPatch.context() as mp:          # the variable is read at every scene creation
        mp.setenv("LRC_QNODES", "0")
        env32 = lidarcast.Scene(engine.ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    try:
        assert env32.info["quantised_nodes"] == 0
        ref = _dev(near, rec, dirs, fire, m, 20.0)
        got = _dev(env32, rec, dirs, fire, m, 20.0)
        assert 0.05 < np.isfinite(ref["t"]).mean() < 1.0
        for a in HITS:
            assert_bit_equal(got[a], ref[a], f"float32 nodes: {a}")
        _assert_frames_equal(noise.scan_noisy_sweeps_compact(env32, rec, dirs, fire, 20.0, m, want=FRAMES),
                             _host_frames(ref, 3, len(dirs)), "float32 nodes compact")
    finally:
        env32.close()


def test_arguments_are_checked(engine, mesh):
    from lidarcast import DirectionTable, motion_records, noise
    dirs = _table(4, 96)
    fire = _fire(dirs, 96)
    rec = motion_records(*_sweeps(2, *MOTIONS["realistic"]))
    scene = engine.scene_for(mesh)
    ok = noise.NoiseModel(seed=1, range_std=0.01)
    for bad in (dict(range_std=-1.0), dict(range_std=float("nan")), dict(angle_std=float("inf")), dict(angle_std=-0.1),
                dict(dropout=1.0), dict(dropout=-0.5), dict(dropout=float("nan"))):
        with pytest.raises(ValueError, match="lrc_scan_noisy_sweeps_dev"):
            _dev(scene, rec, dirs, fire, noise.NoiseModel(seed=1, **bad), 20.0)
        with pytest.raises(ValueError, match="lrc_scan_noisy_sweeps_compact"):
            noise.scan_noisy_sweeps_compact(scene, rec, dirs, fire, 20.0, noise.NoiseModel(seed=1, **bad))
        with pytest.raises(ValueError, match="lrc_scan_noisy_sweeps_compact"):      # an empty call checks the model too
            noise.scan_noisy_sweeps_compact(scene, rec[:0], dirs, fire, 20.0, noise.NoiseModel(seed=1, **bad))
    try:        # one noise source per call
        scene.set_options(range_noise=np.zeros(2 * len(dirs), np.float32))
        with pytest.raises(ValueError, match="one noise source"):
            noise.scan_noisy_sweeps_compact(scene, rec, dirs, fire, 20.0, ok)
        with pytest.raises(ValueError, match="one noise source"):
            _dev(scene, rec, dirs, fire, ok, 20.0)
    finally:
        scene.reset_options()
    tab = DirectionTable(engine.ctx, dirs)           # a table without a fire table
    try:
        with pytest.raises(ValueError, match="firing fractions"):
            noise.scan_noisy_sweeps_compact(scene, rec, tab, None, 20.0, ok)
        fr = noise.scan_noisy_sweeps_compact(scene, rec, tab, fire, 20.0, ok)      # uploaded into the table once, then resident
        assert_bit_equal(fr["point3"], noise.scan_noisy_sweeps_compact(scene, rec, tab, None, 20.0, ok)["point3"])
    finally:
        tab.close()
    for j, v in ((12, 0.7), (5, np.inf), (17, np.nan), (13, 0.5)):      # 0.7 < cos(pi/4): more than pi/2 per sweep
        r = rec.copy()
        r[1, j] = v
        with pytest.raises(ValueError, match="lrc_scan_noisy_sweeps_compact"):
            noise.scan_noisy_sweeps_compact(scene, r, dirs, fire, 20.0, ok)
    with pytest.raises(ValueError, match="fire"):
        noise.scan_noisy_sweeps_compact(scene, rec, dirs, None, 20.0, ok)


def _sim(config, mesh, engine, **kw):
    """A simulator on the module's engine: every run scans the one cached scene of ``mesh``."""
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator(config, **kw)
    if engine is not None:
        sim.raycast_engine = engine
    sim.load_scene(mesh, "room")
    return sim


def test_simulator_nested_noise_key(engine, mesh, monkeypatch):
    from lidarcast import noise
    from trajectory import line_trajectory, poses_from_waypoints, sweep_end_poses
    wps = line_trajectory((1.0, 2.7, 1.0), (7.0, 3.3, 1.0), 5, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"seed": 7, "range_std": 0.02, "angle_std_deg": 0.3, "dropout": 0.1}
    run = lambda cfg: _sim(cfg, mesh, engine).run_simulation(wps)
    sim = _sim(dict(base, motion={"speed": 0.5, "noise": dict(key)}), mesh, engine)
    one, two = sim.run_simulation(wps), run(dict(base, motion={"speed": 0.5, "noise": dict(key)}))
    clean = run(dict(base, motion={"speed": 0.5}))
    T = 1.0 / sim.lidar_config.scan_frequency
    assert one.get_total_frames() == two.get_total_frames() == 5
    for a, b, c in zip(one.frames, two.frames, clean.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.incident_angles, b.incident_angles)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)          # lazy labels: from a noisy-sweep rescan
        assert_bit_equal(a.instance_labels, b.instance_labels)
        assert_bit_equal(a.point_times, b.point_times)
        assert a.scan_quality == b.scan_quality
        assert len(a.points) == len(a.semantic_labels) == len(a.point_times) < len(c.points)
        assert a.point_times.dtype == np.float64 and (a.point_times >= 0).all() and (a.point_times < T).all()
    other = run(dict(base, motion={"speed": 0.5, "noise": dict(key, seed=8)}))
    assert any(len(a.points) != len(b.points) or not np.array_equal(a.points, b.points) for a, b in zip(one.frames, other.frames))
    # labels brought with the points equal the labels of the noisy-sweep rescan
    eager = run({"raycast_engine": {"use_gpu": True, "eager_labels": True}, "motion": {"speed": 0.5, "noise": dict(key)}})
    for a, b in zip(one.frames, eager.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)
        assert_bit_equal(a.instance_labels, b.instance_labels)
        assert_bit_equal(a.point_times, b.point_times)
    # a sensor that does not move: the frames of the noise key
    still, noisy = run(dict(base, motion={"speed": 0.0, "noise": dict(key)})), run(dict(base, noise=dict(key)))
    for a, b in zip(still.frames, noisy.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.incident_angles, b.incident_angles)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)
        assert_bit_equal(a.instance_labels, b.instance_labels)
        assert a.scan_quality == b.scan_quality
    assert any(not np.array_equal(a.points, b.points) for a, b in zip(one.frames, still.frames))
    # the all-zero nested model: the frames of the motion key alone
    zero = run(dict(base, motion={"speed": 0.5, "noise": {"seed": 1, "range_std": 0, "angle_std_deg": 0, "dropout": 0}}))
    for a, b in zip(zero.frames, clean.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.incident_angles, b.incident_angles)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)
        assert_bit_equal(a.point_times, b.point_times)
        assert a.scan_quality == b.scan_quality
    # frame p of the run has frame id p: any subset of the records scans again to the same frames
    model = noise.NoiseModel(seed=7, range_std=0.02, angle_std=float(np.deg2rad(0.3)), dropout=0.1)
    k = sim.lidar_config
    motion, fire, period = engine.sweep_inputs(k, poses_from_waypoints(wps), sweep_end_poses(wps, k.scan_frequency, 0.5))
    fr = noise.scan_noisy_sweep_frames(engine, k, None, None, mesh, model.at_frame(2), want=("point3",),
                                       inputs=(motion[2:4], fire, period))
    assert_bit_equal(fr["point3"], np.concatenate([one.frames[2].points, one.frames[3].points]))
    assert_bit_equal(fr["point_times"], np.concatenate([one.frames[2].point_times, one.frames[3].point_times]))
    # omitted values come from the sensor record; the entries are those of the noise key
    dflt = _sim(dict(base, motion={"speed": 0.5, "noise": {"seed": 7}}), mesh, engine)._noise_model(nested=True)
    assert dflt == noise.NoiseModel(seed=7, range_std=k.range_noise_std, angle_std=float(np.deg2rad(k.angle_noise_std)),
                                    dropout=k.dropout_probability)
    with pytest.raises(ValueError, match="seed"):
        run(dict(base, motion={"speed": 0.5, "noise": {"range_std": 0.02}}))
    with pytest.raises(ValueError, match="unknown entries under the motion.noise key"):
        run(dict(base, motion={"speed": 0.5, "noise": dict(key, sigma=1)}))
    # what the nested key does not cover raises instead of quietly scanning something else
    nested = {"speed": 0.5, "noise": dict(key)}
    with pytest.raises(ValueError, match="motion"):
        run(dict(base, noise=dict(key), motion={"speed": 0.5}))
    with pytest.raises(ValueError, match="nested key motion"):
        run(dict(base, noise=dict(key), motion=dict(nested)))
    with pytest.raises(ValueError, match="beam"):
        run(dict(base, motion=dict(nested), beam={"divergence_mrad": 3.0}))
    with pytest.raises(ValueError, match="materials"):
        run(dict(base, motion=dict(nested), materials={"classes": {"window": {"kind": "glass"}}}))
    with pytest.raises(ValueError, match="movers"):
        run(dict(base, motion=dict(nested), movers={"objects": [{"path": [[0, 1, 1, 0, 0], [1, 2, 1, 0, 0]]}]}))
    with pytest.raises(NotImplementedError, match="dual-axis"):
        _sim(dict(base, motion=dict(nested)), mesh, None, use_blk2go=True).run_simulation(wps[:2])
    for export in (lambda: sim.evaluate_surface_coverage(wps), lambda: sim.export_occupancy_grid(wps, "unused"),
                   lambda: sim.export_frame_annotations(wps, "unused")):      # these passes would scan static, clean poses
        with pytest.raises(NotImplementedError, match="moving-sensor sweeps"):
            export()
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(NotImplementedError, match="multi-rank"):
        run(dict(base, motion=dict(nested)))
