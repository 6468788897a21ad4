"""-m gpu: moving-sensor sweeps (lrc_scan_sweeps_dev / lrc_scan_sweeps_compact, GEN = 4 of the trace kernel).

The sweep rays are restated on the host op for op (tests/sweep_restate.py) and cast through the explicit-ray path with
one range-filter centre per (frame, column): the in-kernel generator must give the same bytes.  Equal start and end poses,
or an all-zero fire table, must give the bytes of the static scan.  The float64 witness bounds what the nlerp rays differ
from slerp-exact poses.  The simulator switches to sweeps only with the ``motion`` config key."""
import numpy as np
import pytest

from helpers import assert_bit_equal, sensor_32x2048, sensor_8x512, sensor_small
from sweep_restate import exact_sweep_rays, sweep_rays

pytestmark = pytest.mark.gpu

HITS = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg")
FRAMES = ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "range_origin_stats", "incident_stats")


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def _sweeps(name, P, speed, turn, freq=10.0, yaw=0.3):
    """(start poses, end poses) of P sweeps on a line through the synth room, ``speed`` m/s, ``turn`` rad/s."""
    from lidarcast import synth
    from trajectory import line_trajectory, poses_from_waypoints, sweep_end_poses
    Lx, Ly, _ = synth.scene_size(name)
    wps = line_trajectory((1.0, Ly / 2 - 0.3, 1.0), (Lx - 1.0, Ly / 2 + 0.3, 1.2), P + 1, yaw=yaw)
    for w in wps:
        w.angular_velocity = turn
    return poses_from_waypoints(wps)[:P], sweep_end_poses(wps, freq, speed)[:P]


def _explicit(scene, rec, dirs, fire, W, max_range, want=HITS):
    """The restated sweep rays through lrc_cast_segments, one segment per (frame, column), back in (frame, ray) order."""
    rays, cen = sweep_rays(rec, dirs, fire)
    P, N = len(rec), len(dirs)
    H = N // W
    perm = (np.arange(P)[:, None, None] * N + np.arange(H)[None, None, :] * W + np.arange(W)[None, :, None]).reshape(-1)
    off = np.arange(0, P * N + 1, H, dtype=np.uint64)
    out = scene.cast_segments(rays[perm], off, cen[perm][::H], max_range, want=want)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return {k: v[inv] for k, v in out.items()}, rays


def _dev(scene, rec, dirs, fire, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    n = len(rec) * len(dirs)
    hits = DeviceHits(n, "cuda", want=want)
    m_t = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    f_t = torch.from_numpy(np.ascontiguousarray(fire, dtype=np.float64)).cuda()
    scene.scan_sweeps_dev(m_t, d_t, f_t, hits, max_range)
    torch.cuda.synchronize()
    out = {k: hits[k].cpu().numpy() for k in want}
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


def _host_frames(rec, P, N):
    """Host compaction of fixed-stride records: what lrc_scan_sweeps_compact must return."""
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


CASES = {
    # name: (sensor, lines/width note, poses)
    "small 4x96 (N % 64 == 0)": (lambda: sensor_small(4, 96), 5),
    "small 3x50 (N % 64 != 0)": (lambda: sensor_small(3, 50), 7),
    "8x512": (sensor_8x512, 4),
    "32x2048": (sensor_32x2048, 2),
}
MOTIONS = {"realistic": (0.5, 1.0), "extreme": (2.0, 4.0)}      # (m/s, rad/s) at 10 Hz: 0.1 and 0.4 rad per sweep


@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("case", list(CASES))
def test_sweeps_bit_exact_against_explicit_rays(engine, case, motion):
    from lidar import IndoorLidar
    from lidarcast import motion_records, synth
    mk, P = CASES[case]
    k = mk()
    name = "synth_A1_office"
    mesh = synth.make_scene(name)
    scene = engine.scene_for(mesh)
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire, W = lid.sensor_directions(), lid.firing_fractions(), int(k.horizontal_res)
    starts, ends = _sweeps(name, P, *MOTIONS[motion])
    rec = motion_records(starts, ends)
    if motion == "extreme":
        assert np.all(2 * np.arccos(rec[:, 12]) > 0.399)
    ref, rays = _explicit(scene, rec, dirs, fire, W, k.max_range)
    got = _dev(scene, rec, dirs, fire, k.max_range)
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"{case} {motion}: {a}")
    assert np.isfinite(ref["t"]).mean() > 0.5
    # the motion is real: rays of the last columns differ from the static scan's
    static = np.concatenate([IndoorLidar(k, m).get_rays() for m in starts])
    assert (rays[:, 3:] != static[:, 3:]).any()
    fr = scene.scan_sweeps_compact(rec, dirs, fire, k.max_range, want=FRAMES)
    _assert_frames_equal(fr, _host_frames(got, P, len(dirs)), f"{case} {motion} compact")
    # the same through a resident table, and the engine surface with per-point times
    fr2 = engine.scan_sweep_frames(k, starts, ends, mesh, want=FRAMES)
    _assert_frames_equal(fr2, _host_frames(got, P, len(dirs)), f"{case} {motion} engine")
    assert_bit_equal(fr2["point_times"], fire[fr2["index"]] * (1.0 / k.scan_frequency))


@pytest.mark.parametrize("case", ["small 3x50 (N % 64 != 0)", "8x512", "32x2048"])
def test_static_sweeps_are_the_static_scan(engine, case):
    import torch
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, motion_records, synth
    mk, P = CASES[case]
    k = mk()
    name = "synth_A1_office"
    mesh = synth.make_scene(name)
    scene = engine.scene_for(mesh)
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    starts, ends = _sweeps(name, P, 0.5, 1.0)
    hits = DeviceHits(P * len(dirs), "cuda", want=HITS)
    scene.scan_poses_dev(torch.from_numpy(starts.reshape(P, 16).copy()).cuda(), torch.from_numpy(dirs).cuda(), hits,
                         k.max_range)
    torch.cuda.synchronize()
    ref = {a: hits[a].cpu().numpy() for a in HITS}
    ref["prim"], ref["sem"], ref["ins"] = ref["prim"].view(np.uint32), ref["sem"].view(np.uint16), ref["ins"].view(np.uint16)
    ref_fr = scene.scan_poses_compact(starts, dirs, k.max_range, want=FRAMES)
    for what, rec, f in (("end == start", motion_records(starts, starts), fire),
                         ("zero fire table", motion_records(starts, ends), np.zeros(len(dirs)))):
        got = _dev(scene, rec, dirs, f, k.max_range)
        for a in HITS:
            assert_bit_equal(got[a], ref[a], f"{case} {what}: {a}")
        fr = scene.scan_sweeps_compact(rec, dirs, f, k.max_range, want=FRAMES)
        _assert_frames_equal(fr, ref_fr, f"{case} {what} compact")


def test_sweeps_against_the_float64_witness_of_slerp_poses(engine):
    """>= 10^5 rays of 10 Hz sweeps at 0.5 m/s and 1 rad/s (the C3 sensor on bench.SCENE): every motion point against the
    float64 witness cast along the slerp-exact pose of its column, on the rays where both hit the same triangle.
    The nlerp direction is at most 4.1e-6 rad off the exact one (0.1 rad per sweep), so the motion point lies within
    range * 4.1e-6 + float32 rounding <= 1e-4 m of the exact RAY; along the surface that offset grows as 1 / cos of the
    incidence angle, so |p - p64| <= 1e-4 m is asserted where the incidence is within 60 degrees of the normal, and the
    grazing remainder is counted and printed beside the edge leaks (measured on the MI355X: max |p - p64| 2.4e-4 m, on a
    grazing ray; p99.9 4.8e-5 m)."""
    import bench
    from lidar import IndoorLidar
    from lidarcast import motion_records, synth
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_scene(bench.SCENE)
    k = bench.c3_sensor()
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    starts, ends = _sweeps(bench.SCENE, 2, 0.5, 1.0)
    rec = motion_records(starts, ends)
    got = _dev(engine.scene_for(mesh), rec, dirs, fire, k.max_range, want=("t", "prim", "point3"))
    exact = exact_sweep_rays(rec, dirs, fire)
    assert len(exact) >= 100000
    r32 = exact.astype(np.float32)
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    t64, p64, m64 = om.witness(r32, threads=16)
    h32, h64 = np.isfinite(got["t"]), np.isfinite(t64)
    leaks_in, leaks_out = int((h64 & ~h32).sum()), int((h32 & ~h64).sum())
    same = h32 & h64 & (got["prim"] == p64)
    other = h32 & h64 & (got["prim"] != p64)
    o, d = r32[:, :3].astype(np.float64), r32[:, 3:].astype(np.float64)
    dh = d / np.linalg.norm(d, axis=1, keepdims=True)
    pt64 = o + dh * t64[:, None]
    p32 = got["point3"][same].astype(np.float64)
    err = np.linalg.norm(p32 - pt64[same], axis=1)
    off_ray = np.linalg.norm(np.cross(p32 - exact[same, :3], exact[same, 3:] / np.linalg.norm(exact[same, 3:], axis=1,
                                                                                                keepdims=True)), axis=1)
    cosi = np.abs((om.normals(p64[same]).astype(np.float64) * dh[same]).sum(1))
    steep = cosi >= 0.5
    print(f"\n[sweep witness] rays {len(r32)}: same triangle {int(same.sum())}, other triangle {int(other.sum())}, "
          f"f64-hit/f32-miss {leaks_in}, f32-hit/f64-miss {leaks_out}; |p - p64| max {err.max():.3e} m "
          f"(incidence within 60 deg: {err[steep].max():.3e} m; grazing rays above 1e-4 m: {int((err > 1e-4).sum())}), "
          f"p99.9 {np.percentile(err, 99.9):.3e} m, mean {err.mean():.3e} m; distance from the exact ray max "
          f"{off_ray.max():.3e} m")
    assert same.sum() >= 0.9 * len(r32)
    assert off_ray.max() <= 1e-4
    assert err[steep].max() <= 1e-4
    assert (err[~steep] * cosi[~steep]).max() <= 1e-4
    assert leaks_in + leaks_out + int(other.sum()) <= 0.05 * len(r32)


def test_sweep_options_equal_the_explicit_path(engine):
    import torch
    from lidar import IndoorLidar
    from lidarcast import motion_records, synth
    k = sensor_8x512()
    name = "synth_A1_office"
    mesh = synth.make_scene(name)
    scene = engine.scene_for(mesh)
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    starts, ends = _sweeps(name, 3, 0.5, 1.0)
    rec = motion_records(starts, ends)
    noise = np.random.default_rng(9).normal(scale=0.02, size=3 * len(dirs)).astype(np.float32)
    try:
        # the explicit path runs rays in (frame, column, line) order: the same noise per ray, permuted alike
        W, H, N = k.horizontal_res, len(dirs) // k.horizontal_res, len(dirs)
        perm = (np.arange(3)[:, None, None] * N + np.arange(H)[None, None, :] * W + np.arange(W)[None, :, None]).reshape(-1)
        scene.set_options(min_range=1.2, range_noise=noise[perm], incident_mode=1)
        ref, _ = _explicit(scene, rec, dirs, fire, W, k.max_range)
        noise_t = torch.from_numpy(noise).cuda()
        scene.set_options(min_range=1.2, range_noise=(noise_t.data_ptr(), noise_t.numel()), incident_mode=1)
        got = _dev(scene, rec, dirs, fire, k.max_range)
        scene.set_options(min_range=1.2, range_noise=noise, incident_mode=1)
        fr = scene.scan_sweeps_compact(rec, dirs, fire, k.max_range, want=FRAMES)
    finally:
        scene.reset_options()
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"options: {a}")
    dropped = np.isinf(got["t"]).mean()
    assert 0.0 < dropped < 0.9
    _assert_frames_equal(fr, _host_frames(got, 3, len(dirs)), "options compact")


def _sim(config, mesh, **kw):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator(config, **kw)
    sim.load_scene(mesh, "room")
    return sim


def test_simulator_motion(monkeypatch):
    from lidarcast import synth
    from trajectory import line_trajectory
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    wps = line_trajectory((1.0, 1.2, 1.0), (3.0, 1.8, 1.0), 5, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    static = _sim(dict(base), mesh).run_simulation(wps)
    still = _sim(dict(base, motion={"speed": 0.0}), mesh).run_simulation(wps)
    assert static.get_total_frames() == still.get_total_frames() == 5
    for a, b in zip(static.frames, still.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.incident_angles, b.incident_angles)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)
        assert_bit_equal(a.instance_labels, b.instance_labels)
        assert a.scan_quality == b.scan_quality
        assert (b.point_times >= 0).all() and (b.point_times < 0.1).all()
    sim = _sim(dict(base, motion={"speed": 0.5}), mesh)
    moving = sim.run_simulation(wps)
    T = 1.0 / sim.lidar_config.scan_frequency
    moved = 0
    for a, b in zip(static.frames, moving.frames):
        assert b.point_times.shape == (len(b.points),) and b.point_times.dtype == np.float64
        assert (b.point_times >= 0).all() and (b.point_times < T).all()
        moved += len(a.points) != len(b.points) or not np.array_equal(a.points, b.points)
    assert moved >= 4                           # the last waypoint's sweep is static
    assert_bit_equal(moving.frames[-1].points, static.frames[-1].points)
    # lazy labels rescan the same sweeps: equal to labels brought with the points
    eager = _sim({"raycast_engine": {"use_gpu": True, "eager_labels": True}, "motion": {"speed": 0.5}}, mesh).run_simulation(wps)
    for a, b in zip(moving.frames, eager.frames):
        assert_bit_equal(a.points, b.points)
        assert_bit_equal(a.semantic_labels, b.semantic_labels)
        assert_bit_equal(a.instance_labels, b.instance_labels)
        assert_bit_equal(a.point_times, b.point_times)
    # what sweeps do not cover raises instead of quietly scanning static poses
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(NotImplementedError, match="multi-rank"):
        _sim(dict(base, motion={"speed": 0.5}), mesh).run_simulation(wps)
    monkeypatch.undo()
    with pytest.raises(NotImplementedError, match="dual-axis"):
        _sim(dict(base, motion={"speed": 0.5}), mesh, use_blk2go=True).run_simulation(wps[:2])


def test_sweep_inputs_are_checked(engine):
    from lidar import IndoorLidar
    from lidarcast import DirectionTable, motion_records, synth
    k = sensor_small(4, 96)
    mesh = synth.make_scene("synth_A1_office")
    scene = engine.scene_for(mesh)
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    starts, ends = _sweeps("synth_A1_office", 2, 0.5, 1.0)
    rec = motion_records(starts, ends)
    for bad in (np.where(np.arange(len(fire)) == 3, 1.0, fire), np.where(np.arange(len(fire)) == 3, -0.1, fire),
                np.where(np.arange(len(fire)) == 3, np.nan, fire), fire[:-1]):
        with pytest.raises(ValueError, match="lrc_table_set_fire"):
            DirectionTable(engine.ctx, dirs, bad)
    for j, v in ((12, 0.7), (5, np.inf), (17, np.nan), (13, 0.5)):
        r = rec.copy()
        r[1, j] = v
        with pytest.raises(ValueError, match="lrc_scan_sweeps_compact"):
            scene.scan_sweeps_compact(r, dirs, fire, k.max_range)
    tab = DirectionTable(engine.ctx, dirs)
    with pytest.raises(ValueError, match="firing fractions"):
        scene.scan_sweeps_compact(rec, tab, None, k.max_range)
    fr = scene.scan_sweeps_compact(rec, tab, fire, k.max_range)       # uploaded into the table once, then resident
    fr2 = scene.scan_sweeps_compact(rec, tab, None, k.max_range)
    assert_bit_equal(fr["point3"], fr2["point3"])
    tab.close()
