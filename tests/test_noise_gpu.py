"""-m gpu: seeded sensor noise drawn in the trace kernel (lrc_scan_noisy_dev / lrc_scan_noisy_compact, GEN = 5).

The noisy rays are restated on the host op for op (tests/noise_restate.py: Philox, the table lookup, the jittered rows, the
keep flags, the range term) and cast through the explicit-ray path with one segment per pose, dropped rays as NaN
directions and the range term as the ``range_noise`` option: the in-kernel generator must give the same bytes.  The
all-zero model must give the bytes of the clean scan, each single-parameter model must change only what it should, and the
noise of a frame must not depend on which call scans it."""
import numpy as np
import pytest

import noise_restate as nr
from helpers import assert_bit_equal, pose, sensor_32x2048, sensor_small

pytestmark = pytest.mark.gpu

HITS = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg")
FRAMES = ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "range_origin_stats", "incident_stats")


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


@pytest.fixture(scope="module")
def room():
    from lidarcast import synth
    return synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)


@pytest.fixture(scope="module")
def tab():
    from lidarcast import noise
    return noise.table()


def _table(lines, width):
    """The small sensor's direction table with one row straight up and one straight down (h == 0: never jittered)."""
    from lidar import IndoorLidar
    k = sensor_small(lines, width)
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions().copy()
    dirs[7] = (0.0, 0.0, 1.0)
    dirs[11] = (0.0, 0.0, -1.0)
    return dirs


def _poses(P, near_wall=False):
    x0 = 0.3 if near_wall else 1.0
    ps = [pose(x0 + 0.45 * j, 1.2 + 0.1 * j, 1.0 + 0.05 * j) for j in range(P)]
    ps[1 % P] = pose(x0 + 0.45 * (1 % P), 1.3, 1.05, yaw=0.7)
    return np.stack(ps)


def _views(out):
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


def _noisy_dev(scene, poses, dirs, model, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    scene.scan_noisy_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                         torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range, model)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def _clean_dev(scene, poses, dirs, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    scene.scan_poses_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                         torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def _explicit(scene, poses, dirs, model, max_range, tab, min_range=0.0, incident_mode=0, want=HITS):
    """The restated noisy rays through lrc_cast_segments, one segment per pose; the range term as the range_noise option."""
    base, slope = tab
    rays, cen, term, keep, rows = nr.noisy_rays(poses, dirs, model.seed, model.first_frame, model.range_std,
                                                model.angle_std, model.dropout, base, slope)
    P, N = len(poses), len(dirs)
    off = np.arange(P + 1, dtype=np.uint64) * np.uint64(N)
    try:
        scene.set_options(min_range=min_range, range_noise=term if model.range_std != 0 else None,
                          incident_mode=incident_mode)
        out = scene.cast_segments(rays, off, cen, max_range, want=want)
    finally:
        scene.reset_options()
    return out, dict(rays=rays, term=term, keep=keep, rows=rows)


def _host_frames(rec, P, N):
    """Host compaction of fixed-stride records: what lrc_scan_noisy_compact must return."""
    keep = (rec["t"] != np.inf).reshape(P, N)
    sel = keep.reshape(-1)
    pts = rec["point3"][sel]
    ro = np.linalg.norm(pts, axis=1) if len(pts) else np.zeros(0, np.float32)
    counts = keep.sum(1)
    ends = np.cumsum(counts)
    out = {"counts": counts, "point3": pts, "sem": rec["sem"][sel], "ins": rec["ins"][sel],
           "incident_deg": rec["incident_deg"][sel], "index": np.nonzero(keep)[1].astype(np.uint32), "range_origin": ro}
    for col, a in (("range_origin", ro), ("incident", out["incident_deg"])):
        out[f"{col}_mean"] = np.array([np.mean(a[e - c:e]) if c else 0 for c, e in zip(counts, ends)], dtype=a.dtype)
        out[f"{col}_std"] = np.array([np.std(a[e - c:e]) if c else 0 for c, e in zip(counts, ends)], dtype=a.dtype)
    return out


def _assert_frames_equal(fr, want, what):
    assert fr["counts"].tolist() == want["counts"].tolist(), what
    for k in ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "range_origin_mean", "range_origin_std",
              "incident_mean", "incident_std"):
        assert_bit_equal(fr[k], want[k], f"{what}: {k}")


# name: (lines, width, first_frame, range_std, angle_std, dropout, max_range, min_range, incident_mode, near_wall)
CASES = {
    "N = 400 (not a multiple of 64)": (4, 100, 0, 0.02, 0.01, 0.05, 20.0, 0.0, 0, False),
    "N = 384, frame ids carry into the high word": (4, 96, 2 ** 32 - 1, 0.02, 0.01, 0.05, 20.0, 0.0, 0, False),
    "max_range cuts, min_range > 0, normal incidence": (4, 100, 3, 0.02, 0.01, 0.05, 2.2, 0.9, 1, False),
    "range_std 0.5 close to a wall": (4, 96, 0, 0.5, 0.002, 0.02, 20.0, 0.0, 0, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_noisy_scan_bit_exact_against_explicit_rays(engine, room, tab, case):
    from lidarcast.noise import NoiseModel
    lines, width, first, rs, sa, dr, max_range, min_range, inc_mode, near = CASES[case]
    dirs = _table(lines, width)
    P, N = 3, len(dirs)
    poses = _poses(P, near)
    scene = engine.scene_for(room)
    model = NoiseModel(seed=0xC0FFEE123456789, range_std=rs, angle_std=sa, dropout=dr, first_frame=first)
    ref, aux = _explicit(scene, poses, dirs, model, max_range, tab, min_range, inc_mode)
    try:
        scene.set_options(min_range=min_range, incident_mode=inc_mode)
        got = _noisy_dev(scene, poses, dirs, model, max_range)
        fr = scene.scan_noisy_compact(poses, dirs, max_range, model, want=FRAMES)
    finally:
        scene.reset_options()
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"{case}: {a}")
    hit = np.isfinite(got["t"])
    assert 0.05 < hit.mean() < 1.0
    # the case exercises what it is for
    rows = aux["rows"].reshape(-1, 3)
    assert_bit_equal(rows[7::N], np.tile(dirs[7], (P, 1)))               # h == 0 rows pass through
    assert_bit_equal(rows[11::N], np.tile(dirs[11], (P, 1)))
    assert (rows != np.tile(dirs, (P, 1))).any(axis=1).mean() > 0.95      # every other row is jittered
    assert 0 < (~aux["keep"]).sum() < 0.2 * P * N
    clean = _clean_dev(scene, poses, dirs, 1e9, want=("t",))["t"]
    if "cuts" in case:
        assert (np.isfinite(clean) & ~hit & aux["keep"]).sum() > 0.05 * P * N
    if near:       # returns lost to a non-positive noisy range: clean returns of kept rays that are gone
        lost = np.isfinite(clean) & ~hit & aux["keep"]
        print(f"\n[noise] range_std {rs}: {int(lost.sum())} returns lost to t' <= 0")
        assert lost.sum() >= 5
    _assert_frames_equal(fr, _host_frames(got, P, N), f"{case} compact")
    # the engine surface over the resident table of a real sensor record
    k = sensor_small(lines, width)
    from lidar import IndoorLidar
    kd = IndoorLidar(k, np.eye(4)).sensor_directions()
    fr2 = engine.scan_noisy_frames(k, poses, room, model, want=FRAMES)
    _assert_frames_equal(fr2, _host_frames(_noisy_dev(scene, poses, kd, model, k.max_range), P, N), f"{case} engine")


@pytest.mark.parametrize("width", [100, 96])
def test_all_zero_model_is_the_clean_scan(engine, room, width):
    from lidarcast.noise import NoiseModel
    dirs = _table(4, width)
    poses = _poses(3)
    scene = engine.scene_for(room)
    clean = _clean_dev(scene, poses, dirs, 3.0)
    got = _noisy_dev(scene, poses, dirs, NoiseModel(seed=99, first_frame=17), 3.0)
    for a in HITS:
        assert_bit_equal(got[a], clean[a], f"zero model: {a}")
    fr = scene.scan_noisy_compact(poses, dirs, 3.0, NoiseModel(seed=99), want=FRAMES)
    _assert_frames_equal(fr, scene.scan_poses_compact(poses, dirs, 3.0, want=FRAMES), "zero model compact")


def test_single_parameter_models_change_only_their_part(engine, room, tab):
    from lidarcast.noise import NoiseModel, draws
    dirs = _table(4, 100)
    P, N = 3, len(dirs)
    poses = _poses(P)
    scene = engine.scene_for(room)
    R = 20.0                                         # nothing in the 4 x 3 m room is cut
    clean = _clean_dev(scene, poses, dirs, R)
    ch = np.isfinite(clean["t"])
    # range only: same ray, same triangle; t moves by the term
    m = NoiseModel(seed=5, range_std=0.03)
    got = _noisy_dev(scene, poses, dirs, m, R)
    term = (np.float32(0.03) * draws(m, P, N)["z_range"]).reshape(-1)
    gh = np.isfinite(got["t"])
    assert not (gh & ~ch).any()
    for a in ("prim", "normal3", "sem", "ins"):
        assert_bit_equal(got[a][gh], clean[a][gh], f"range only: {a}")
    assert_bit_equal(got["t"][gh], (clean["t"] + term)[gh], "range only: t")
    assert ((clean["t"] + term)[ch & ~gh] <= 0).all()
    assert (got["t"][gh] != clean["t"][gh]).mean() > 0.95
    # angle only: t is the clean cast of the jittered rays
    m = NoiseModel(seed=5, angle_std=0.01)
    got = _noisy_dev(scene, poses, dirs, m, R)
    ref, aux = _explicit(scene, poses, dirs, m, R, tab)
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"angle only: {a}")
    assert aux["keep"].all() and not aux["term"].any()
    assert (got["t"] != clean["t"]).mean() > 0.5
    # dropout only: a subset of the clean records
    m = NoiseModel(seed=5, dropout=0.3)
    got = _noisy_dev(scene, poses, dirs, m, R)
    keep = draws(m, P, N)["keep"].reshape(-1)
    assert 0.2 < (~keep).mean() < 0.4
    for a in HITS:
        assert_bit_equal(got[a][keep], clean[a][keep], f"dropout only: {a}")
    assert not np.isfinite(got["t"][~keep]).any() and (got["prim"][~keep] == 0xFFFFFFFF).all()
    fr = scene.scan_noisy_compact(poses, dirs, R, m, want=FRAMES)
    cf = scene.scan_poses_compact(poses, dirs, R, want=FRAMES)
    gi = np.repeat(np.arange(P), fr["counts"]) * N + fr["index"]
    ci = np.repeat(np.arange(P), cf["counts"]) * N + cf["index"]
    pos = np.searchsorted(ci, gi)
    assert (ci[pos] == gi).all() and len(gi) < len(ci)
    assert_bit_equal(fr["point3"], cf["point3"][pos])


def test_noise_does_not_depend_on_chunking(engine, room):
    from lidarcast.noise import NoiseModel
    dirs = _table(4, 100)
    poses = _poses(6)
    scene = engine.scene_for(room)
    m = NoiseModel(seed=77, range_std=0.02, angle_std=0.01, dropout=0.05, first_frame=2 ** 32 - 3)
    whole = _noisy_dev(scene, poses, dirs, m, 20.0)
    a = _noisy_dev(scene, poses[:2], dirs, m, 20.0)
    b = _noisy_dev(scene, poses[2:], dirs, m.at_frame(m.first_frame + 2), 20.0)
    for k in HITS:
        assert_bit_equal(whole[k], np.concatenate([a[k], b[k]]), f"chunks: {k}")
    fw = scene.scan_noisy_compact(poses, dirs, 20.0, m, want=("point3", "index"))
    fa = scene.scan_noisy_compact(poses[:2], dirs, 20.0, m, want=("point3", "index"))
    fb = scene.scan_noisy_compact(poses[2:], dirs, 20.0, m.at_frame(m.first_frame + 2), want=("point3", "index"))
    assert fw["counts"].tolist() == fa["counts"].tolist() + fb["counts"].tolist()
    assert_bit_equal(fw["point3"], np.concatenate([fa["point3"], fb["point3"]]))
    other = _noisy_dev(scene, poses, dirs, NoiseModel(seed=78, range_std=0.02, angle_std=0.01, dropout=0.05), 20.0)
    assert (other["t"] != whole["t"]).mean() > 0.5


def test_large_scan_in_pose_chunks(engine, room, tab):
    """2^20 rays of whole 64-ray tiles: lrc_scan_noisy_compact scans in pose chunks (each with its own first frame id) and
    the launch deals tiles to the XCDs in stripes -- the records of ONE launch, themselves equal to the restated rays, must
    compact to the same frames."""
    from lidar import IndoorLidar
    from lidarcast.noise import NoiseModel
    k = sensor_32x2048()
    dirs = IndoorLidar(k, np.eye(4)).sensor_directions()
    P, N = 16, len(dirs)
    assert P * N == 1 << 20 and N % 64 == 0
    poses = np.stack([pose(0.6 + 0.18 * j, 1.5, 1.0, yaw=0.1 * j) for j in range(P)])
    scene = engine.scene_for(room)
    m = NoiseModel(seed=2026, range_std=0.02, angle_std=0.003, dropout=0.05, first_frame=2 ** 32 - 5)
    got = _noisy_dev(scene, poses, dirs, m, k.max_range)
    ref, _ = _explicit(scene, poses, dirs, m, k.max_range, tab)
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"large: {a}")
    fr = scene.scan_noisy_compact(poses, dirs, k.max_range, m, want=FRAMES)
    _assert_frames_equal(fr, _host_frames(got, P, N), "large compact")


def test_noisy_scan_arguments_are_checked(engine, room):
    from lidarcast.noise import NoiseModel
    dirs = _table(4, 96)
    poses = _poses(2)
    scene = engine.scene_for(room)
    for bad in (dict(range_std=-1.0), dict(range_std=float("nan")), dict(angle_std=float("inf")), dict(angle_std=-0.1),
                dict(dropout=1.0), dict(dropout=-0.5), dict(dropout=float("nan"))):
        with pytest.raises(ValueError, match="lrc_scan_noisy_dev"):
            _noisy_dev(scene, poses, dirs, NoiseModel(seed=1, **bad), 20.0)
        with pytest.raises(ValueError, match="lrc_scan_noisy_compact"):
            scene.scan_noisy_compact(poses, dirs, 20.0, NoiseModel(seed=1, **bad))
    try:        # one noise source per call
        scene.set_options(range_noise=np.zeros(2 * len(dirs), np.float32))
        with pytest.raises(ValueError, match="one noise source"):
            scene.scan_noisy_compact(poses, dirs, 20.0, NoiseModel(seed=1, range_std=0.01))
        with pytest.raises(ValueError, match="one noise source"):
            _noisy_dev(scene, poses, dirs, NoiseModel(seed=1, range_std=0.01), 20.0)
    finally:
        scene.reset_options()


def _sim(config, mesh, **kw):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator(config, **kw)
    sim.load_scene(mesh, "room")
    return sim


def test_simulator_noise_key(engine, room, monkeypatch):
    from lidarcast.noise import NoiseModel
    from trajectory import line_trajectory, poses_from_waypoints
    wps = line_trajectory((1.0, 1.2, 1.0), (3.0, 1.8, 1.0), 5, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"seed": 31, "range_std": 0.02, "angle_std_deg": 0.3, "dropout": 0.1}
    clean = _sim(dict(base), room).run_simulation(wps)
    sim = _sim(dict(base, noise=dict(key)), room)
    one, two = sim.run_simulation(wps), _sim(dict(base, noise=dict(key)), room).run_simulation(wps)
    assert one.get_total_frames() == two.get_total_frames() == 5
    for a, b, c in zip(one.frames, two.frames, clean.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.incident_angles, b.incident_angles)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)          # lazy labels: from a noisy rescan
        assert_bit_equal(a.instance_labels, b.instance_labels)
        assert a.scan_quality == b.scan_quality
        assert len(a.points) == len(a.semantic_labels) < len(c.points)
    other = _sim(dict(base, noise=dict(key, seed=32)), room).run_simulation(wps)
    assert any(len(a.points) != len(b.points) or not np.array_equal(a.points, b.points)
               for a, b in zip(one.frames, other.frames))
    # labels brought with the points equal the labels of the noisy rescan
    eager = _sim({"raycast_engine": {"use_gpu": True, "eager_labels": True}, "noise": dict(key)}, room).run_simulation(wps)
    for a, b in zip(one.frames, eager.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)
        assert_bit_equal(a.instance_labels, b.instance_labels)
    # frame p of the run has frame id p: any subset scans again to the same frames
    model = NoiseModel(seed=31, range_std=0.02, angle_std=float(np.deg2rad(0.3)), dropout=0.1)
    fr = engine.scan_noisy_frames(sim.lidar_config, poses_from_waypoints(wps)[2:4], room, model.at_frame(2), want=("point3",))
    assert_bit_equal(fr["point3"], np.concatenate([one.frames[2].points, one.frames[3].points]))
    # omitted values come from the sensor record
    k = sim.lidar_config
    dflt = _sim(dict(base, noise={"seed": 31}), room)._noise_model()
    assert dflt == NoiseModel(seed=31, range_std=k.range_noise_std, angle_std=float(np.deg2rad(k.angle_noise_std)),
                              dropout=k.dropout_probability)
    # what the key does not cover raises instead of quietly scanning something else
    with pytest.raises(ValueError, match="motion"):
        _sim(dict(base, noise=dict(key), motion={"speed": 0.5}), room).run_simulation(wps)
    with pytest.raises(ValueError, match="dual-axis"):
        _sim(dict(base, noise=dict(key)), room, use_blk2go=True).run_simulation(wps[:2])
    for export in (lambda: sim.evaluate_surface_coverage(wps), lambda: sim.export_occupancy_grid(wps, "unused"),
                   lambda: sim.export_frame_annotations(wps, "unused")):      # these passes would scan without the noise
        with pytest.raises(NotImplementedError, match="noise key"):
            export()
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(ValueError, match="multi-rank"):
        _sim(dict(base, noise=dict(key)), room).run_simulation(wps)
