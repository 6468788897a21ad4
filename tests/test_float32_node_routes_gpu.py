"""-m gpu: every ray generator and the scan pipeline on the float32 world-space nodes of the trace kernel.

The kernel walks the 32-byte quantised node images (template parameter QN = 1) for every room near the world origin, so
that is what the rest of the suite runs.  The float32 nodes are reached two ways:

  * the scene has no images -- LRC_QNODES=0 (``env32``), or the builder refuses a scene whose grid base is farther than
    8 W from the world origin (``shifted``: the room moved by +25 m on y) -- and launch_trace picks the Q = 0 instantiation
    of each generator;
  * inside the QN = 1 kernel a wave that holds a "far" ray (|o - base| > 6 W, |o| > 12 W or |d| > 2^60 on any axis) walks
    the float32 nodes: a sensor about one scene width outside the room (``far`` poses on the ``near`` scene), or a sweep
    whose origin crosses the bound inside a wave.

Every case is bit for bit: pose scans against the CPU oracle and against the explicit-ray cast of the same scene, sweeps
and seeded noise against their host restatements through the explicit-ray cast (sweeps against the oracle too), the
scan-angle generator differentially, the pipeline against the serial calls and the oracle.  The builder's grid and the
kernel's far predicate are restated here from the scene bounds, so that each case proves which route it took.

The far sensors stand 12-96 m outside a 4 x 3 x 2.5 m room, which they see under 1-12 degrees: a full-circle table would
return a handful of hits (N = 400 at 100 m: none), so the far cases scan ``helpers.beam_table`` tables of the same line
and column counts, aimed at the room; the reference hit share is then above 0.3 as asserted.  The dual-axis sensor draws a
full circle by construction: its far case asserts a hit count instead (see the test)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import full_parity as fp
import test_noise_gpu as tno
import test_sweep_gpu as tsw
from helpers import aimed_pose, assert_bit_equal, beam_table, pose, sensor_small, table_rays
from test_pipe_line_groups_gpu import _hook, _oracle_rows, _sensor, _widest
from test_pipe_two_line_gpu import _check_records, _line_tiles, _poses as _pipe_poses, _reference

pytestmark = pytest.mark.gpu

HITS, FRAMES = tsw.HITS, tsw.FRAMES
SHIFT = np.array([0.0, 25.0, 0.0])
CENTRE = (2.0, 1.5, 1.25)            # of the 4 x 3 x 2.5 m room
FAR_RANGE = 200.0
INSIDE, FAR = 0.9, 0.3               # reference hit share every case must exceed


# ---- the builder's grid and the kernel's far predicate, restated -------------------------------------------------------------
def qgrid(lo, hi):
    """make_qgrid_bounds (csrc/lrc_qnodes.cpp) from the scene bounds: per axis the float32 base and the power-of-two width
    W with the scene in [base + 2 W, base + 4 W); None where the builder refuses the scene (|base| > 8 W)."""
    base, W = np.empty(3, np.float32), np.empty(3, np.float32)
    for a in range(3):
        l, h = float(np.float32(lo[a])), float(np.float32(hi[a]))
        k = -20
        while k <= 16 and 2.0 * 2.0 ** k * (1.0 - 1.0 / 1024) < h - l:
            k += 1
        if k > 16:
            return None
        w = 2.0 ** k
        b = l - 8.0 * (w / 16384.0) - 2.0 * w
        bf = np.float32(b)
        if float(bf) > b:
            bf = np.nextafter(bf, np.float32(-np.inf))
        if not abs(float(bf)) <= 8.0 * w:
            return None
        base[a], W[a] = bf, w
    return base, W


def far_rays(rays, grid):
    """far1 of the trace kernel (csrc/lidarcast.hip) per ray of (n, 6) float32 rays, in float32 as the kernel forms it."""
    base, W = grid
    o, d = np.asarray(rays[:, :3], np.float32), np.asarray(rays[:, 3:], np.float32)
    with np.errstate(invalid="ignore"):
        return (~(np.abs(o - base) <= np.float32(6.0) * W) | ~(np.abs(o) <= np.float32(12.0) * W) |
                ~(np.abs(d) <= np.float32(2.0 ** 60))).any(axis=1)


def far_poses_of(poses, grid):
    o = np.asarray(poses, np.float64).reshape(-1, 4, 4)[:, :3, 3].astype(np.float32)
    return far_rays(np.concatenate([o, np.zeros_like(o)], 1), grid)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
class World:
    pass


@pytest.fixture(scope="module")
def world():
    import lidarcast
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    w = World()
    w.mesh = mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    w.sem, w.ins = mesh.triangle_sem, mesh.triangle_ins
    w.ctx = lidarcast.Context(0)
    w.v_shift = (mesh.vertices + SHIFT).astype(np.float32)
    mk = lambda v: lidarcast.Scene(w.ctx, v, mesh.triangles, w.sem, w.ins)
    w.near = mk(mesh.vertices)
    with pytest.MonkeyPatch.context() as mp:          # the variable is read at every scene creation
        mp.setenv("LRC_QNODES", "0")
        w.env32 = mk(mesh.vertices)
    w.shifted = mk(w.v_shift)
    assert w.near.info["quantised_nodes"] == 1
    assert w.env32.info["quantised_nodes"] == 0
    # |base_y| = 25 - 2 W - 8 cells = 21 m > 8 W = 16 m for the 3 m wide side (W = 2 m): refused without the variable
    assert w.shifted.info["quantised_nodes"] == 0
    w.grid = qgrid(w.near.info["bounds_lo"], w.near.info["bounds_hi"])
    assert w.grid is not None and w.grid[1].tolist() == [4.0, 2.0, 2.0]
    assert qgrid(w.shifted.info["bounds_lo"], w.shifted.info["bounds_hi"]) is None
    w.om = OracleMesh(mesh.vertices, mesh.triangles).build()
    w.om_shift = OracleMesh(w.v_shift, mesh.triangles).build()
    yield w
    for s in (w.near, w.env32, w.shifted):
        s.close()
    w.ctx.close()


def _inside_poses(shift=None):
    ps = np.stack([pose(1.0, 1.2, 1.0), pose(2.2, 1.7, 1.1, yaw=0.7), pose(3.1, 1.4, 0.9, yaw=-2.0)])
    if shift is not None:
        ps[:, :3, 3] += shift
    return ps


def _far_poses():
    """100 m away on x (far by |o| > 12 W = 48 m), x = 18 (far only by |o - base| > 6 W: the bound is at x = 16), and one
    rotated in yaw, pitch and roll, 30 m from the room's centre.  All look at the centre along the sensor's -x axis."""
    return np.stack([aimed_pose(CENTRE, 98.0), aimed_pose(CENTRE, 16.0), aimed_pose(CENTRE, 30.0, yaw=0.5, pitch=-0.3, roll=0.4)])


def _assert_far(w, poses):
    """Every far pose satisfies the restated predicate and no inside pose does; the second one by the base term alone."""
    base, W = w.grid
    assert far_poses_of(poses, w.grid).all()
    assert not far_poses_of(_inside_poses(), w.grid).any()
    o = poses[1, :3, 3].astype(np.float32)
    assert (np.abs(o) <= np.float32(12.0) * W).all() and o[0] - base[0] >= np.float32(6.0) * W[0] + np.float32(0.5)
    assert (np.abs(o[1:] - base[1:]) <= np.float32(6.0) * W[1:]).all()
    assert abs(float(poses[0, 0, 3])) > 12.0 * float(W[0])


def _kind(w, kind):
    """scene, oracle, poses, max_range override (None: the sensor's), required hit share, far?"""
    if kind == "env32":
        return w.env32, w.om, _inside_poses(), None, INSIDE, False
    if kind == "shifted":
        return w.shifted, w.om_shift, _inside_poses(SHIFT), None, INSIDE, False
    poses = _far_poses()
    _assert_far(w, poses)
    return w.near, w.om, poses, FAR_RANGE, FAR, True


def _ring(lines, width, max_range=20.0):
    from lidar import IndoorLidar
    return IndoorLidar(sensor_small(lines, width, max_range), np.eye(4)).sensor_directions()


def _beam(lines, width):
    return beam_table(np.linspace(1.0, -1.0, lines), width, 1.5)


def _report(what, rays, share):
    print(f"\n[f32 routes] {what}: rays compared {rays}, reference hit share {share:.4f}")


# ---- 1. pose scans (GEN = 1) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 100), (16, 1024)], ids=["N=400", "16x1024"])
@pytest.mark.parametrize("kind", ["env32", "shifted", "far"])
def test_pose_scans(world, kind, shape):
    """lrc_scan_poses_dev / lrc_scan_poses_compact: N = 400 (not whole tiles) and 16 x 1024 (256 tiles per pose: XCD
    striping and tiles_per_pose on), 3 poses."""
    from lidar import create_lidar
    w = world
    scene, om, poses, max_range, share_min, far = _kind(w, kind)
    lines, width = shape
    if far:
        dirs = _beam(lines, width)
    else:
        dirs = _ring(lines, width)
        max_range = 20.0
    P, N = len(poses), len(dirs)
    rays, cen = table_rays(dirs, poses)
    if not far:       # the table's rays ARE the sensor's: the reference generator itself
        assert_bit_equal(rays[:N], create_lidar(sensor_small(lines, width), poses[0]).get_rays(), "host rays")
    want = fp.expected_scan(om, rays, cen, max_range, P, w.sem, w.ins)
    share = float(want["keep"].mean())
    _report(f"pose scan, {kind}, {lines} x {width}", P * N, share)
    assert share > share_min
    got = tno._clean_dev(scene, poses, dirs, max_range)
    fp.assert_scan_equal(got, want, f"{kind} {lines} x {width} against the oracle", fields=fp.RECORDS)
    # incident_deg: device acos against numpy's (the bound of test_parity_gpu), and bit for bit against the explicit cast
    k = want["keep"]
    v = want["point3"][k].astype(np.float64) - np.repeat(cen, N, axis=0)[k]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.abs(got["incident_deg"][k] - np.degrees(np.arccos(np.abs(v[:, 2])))).max() < 1e-9
    ex = scene.cast_segments(rays, np.arange(P + 1, dtype=np.uint64) * np.uint64(N), cen, max_range, want=HITS)
    for a in HITS:
        assert_bit_equal(got[a], ex[a], f"{kind} {lines} x {width} against explicit rays: {a}")
    fr = scene.scan_poses_compact(poses, dirs, max_range, want=FRAMES)
    tsw._assert_frames_equal(fr, tsw._host_frames(got, P, N), f"{kind} {lines} x {width} compact")
    if kind == "env32":       # the float32 nodes and the quantised images of one tree: the same bytes
        near = tno._clean_dev(w.near, poses, dirs, max_range)
        for a in HITS:
            assert_bit_equal(got[a], near[a], f"env32 against near: {a}")


# ---- 2. sweeps (GEN = 4) ------------------------------------------------------------------------------------------------------
def _check_sweeps(w, scene, om, starts, ends, dirs, width, max_range, what, share_min):
    from lidarcast import motion_records
    fire = (np.arange(len(dirs)) % width) / width             # IndoorLidar.firing_fractions of a line-major table
    rec = motion_records(starts, ends)
    P, N = len(rec), len(dirs)
    ref, rays = tsw._explicit(scene, rec, dirs, fire, width, max_range)
    share = float(np.isfinite(ref["t"]).mean())
    _report(what, P * N, share)
    assert share > share_min
    got = tsw._dev(scene, rec, dirs, fire, max_range)
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"{what}: {a}")
    from sweep_restate import sweep_rays
    _, cen = sweep_rays(rec, dirs, fire)
    fp.assert_scan_equal(got, fp.expected_scan(om, rays, cen, max_range, P, w.sem, w.ins), f"{what} against the oracle",
                         fields=fp.RECORDS)
    fr = scene.scan_sweeps_compact(rec, dirs, fire, max_range, want=FRAMES)
    tsw._assert_frames_equal(fr, tsw._host_frames(got, P, N), f"{what} compact")
    return rec, rays


@pytest.mark.parametrize("shape", [(3, 50), (4, 96)], ids=["3x50", "4x96"])
@pytest.mark.parametrize("kind", ["env32", "shifted"])
def test_sweeps(world, kind, shape):
    """lrc_scan_sweeps_dev / lrc_scan_sweeps_compact at the "extreme" motion of test_sweep_gpu (2 m/s, 4 rad/s at 10 Hz)."""
    w = world
    scene, om, _, _, share_min, _ = _kind(w, kind)
    lines, width = shape
    sh = SHIFT if kind == "shifted" else np.zeros(3)
    starts = np.stack([pose(1.0 + 0.5 * j + sh[0], 1.2 + 0.1 * j + sh[1], 1.0 + 0.05 * j, yaw=0.3 + 0.2 * j) for j in range(4)])
    ends = np.stack([pose(1.19 + 0.5 * j + sh[0], 1.26 + 0.1 * j + sh[1], 1.02 + 0.05 * j, yaw=0.7 + 0.2 * j) for j in range(4)])
    rec, rays = _check_sweeps(w, scene, om, starts, ends, _ring(lines, width), width, 20.0,
                              f"sweeps, {kind}, {lines} x {width}", share_min)
    assert np.all(2 * np.arccos(rec[:, 12]) > 0.399)
    static, _ = table_rays(_ring(lines, width), starts)
    assert (rays[:, 3:] != static[:, 3:]).any()               # the motion is real


def test_sweep_crossing_the_far_bound_inside_a_wave(world):
    """Sweeps on ``near`` whose sensor crosses x = base + 6 W while a 128-column line fires: single waves hold origins on
    both sides of the bound, so they mix lanes the predicate sends to the float32 nodes with lanes it would not."""
    w = world
    base, W = w.grid
    xb = float(base[0]) + 6.0 * float(W[0])
    assert 15.9 < xb < 16.1
    dirs = beam_table(np.linspace(4.0, -4.0, 4), 128, 6.0)
    at = lambda x, y, yaw: pose(x, y, 1.25, yaw=yaw)
    starts = np.stack([at(xb - 0.08, 1.5, 0.0), at(xb + 0.13, 1.45, 0.01), at(30.0, 1.5, 0.0)])
    ends = np.stack([at(xb + 0.12, 1.56, 0.01), at(xb - 0.07, 1.5, -0.01), at(30.1, 1.5, 0.02)])
    rec, rays = _check_sweeps(w, w.near, w.om, starts, ends, dirs, 128, FAR_RANGE, "sweeps crossing the far bound on near", FAR)
    far = far_rays(rays, w.grid).reshape(len(rec), -1, 64)
    mixed = far.any(axis=2) & ~far.all(axis=2)
    print(f"[f32 routes] crossing sweeps: {int(mixed.sum())} of {mixed.size} tiles hold far and near rays, "
          f"{int(far.all(axis=2).sum())} are all far")
    assert mixed[0].any() and mixed[1].any() and far[2].all()


# ---- 3. seeded noise (GEN = 5) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 100), (4, 96)], ids=["N=400", "N=384"])
@pytest.mark.parametrize("kind", ["env32", "shifted", "far"])
def test_seeded_noise(world, kind, shape):
    """lrc_scan_noisy_dev / lrc_scan_noisy_compact, all three terms on, frame ids that carry into the high word."""
    from lidarcast import noise
    w = world
    scene, _, poses, max_range, share_min, far = _kind(w, kind)
    lines, width = shape
    # far: a range term small against the 12-96 m ranges, and a jitter small against the 3 degree beam
    dirs, rs, sa = (_beam(lines, width), 0.02, 0.002) if far else (_ring(lines, width), 0.02, 0.01)
    max_range = max_range or 20.0
    P, N = len(poses), len(dirs)
    model = noise.NoiseModel(seed=0xC0FFEE123456789, range_std=rs, angle_std=sa, dropout=0.05, first_frame=2 ** 32 - 1)
    ref, aux = tno._explicit(scene, poses, dirs, model, max_range, noise.table())
    clean = tno._clean_dev(scene, poses, dirs, max_range, want=("t",))["t"]
    share = float(np.isfinite(clean).mean())
    _report(f"seeded noise, {kind}, N = {N}", P * N, share)
    assert share > share_min                                   # of the clean scan: the noise then drops 5 % of it
    got = tno._noisy_dev(scene, poses, dirs, model, max_range)
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"noise {kind} N = {N}: {a}")
    hit = np.isfinite(got["t"])
    assert 0.9 * share * 0.9 < hit.mean() < 1.0
    # dropout and jitter acted, and the range term moved the returns
    rows = aux["rows"].reshape(-1, 3)
    assert (rows != np.tile(dirs, (P, 1))).any(axis=1).mean() > 0.95
    assert 0 < (~aux["keep"]).sum() < 0.2 * P * N
    assert not np.isfinite(got["t"][~aux["keep"]]).any()
    both = hit & np.isfinite(clean)
    assert (got["t"][both] != clean[both]).mean() > 0.95
    fr = scene.scan_noisy_compact(poses, dirs, max_range, model, want=FRAMES)
    tno._assert_frames_equal(fr, tno._host_frames(got, P, N), f"noise {kind} N = {N} compact")


# ---- 4. scan angles / dual axis (GEN = 2) -------------------------------------------------------------------------------------
DUAL = ("point3", "sem", "ins", "incident_deg", "index")


@pytest.fixture(scope="module")
def engines(world):
    """One engine holding ``near`` and one holding ``env32`` of the same mesh object (scene_for caches per mesh, so each
    engine builds its scene once, under its own environment)."""
    from raycast_engine import RaycastEngineGPU
    near = RaycastEngineGPU(prelock_bytes=())
    assert near.scene_for(world.mesh).info["quantised_nodes"] == 1
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LRC_QNODES", "0")
        env32 = RaycastEngineGPU(prelock_bytes=())
        assert env32.scene_for(world.mesh).info["quantised_nodes"] == 0
    yield near, env32
    near.clear_cache()
    env32.clear_cache()


def _dual(engine, mesh, k, poses, seed):
    from lidar import create_lidar
    np.random.seed(seed)
    fr = engine.scan_frames_dual_axis([create_lidar(k, m) for m in poses], mesh, want=DUAL)
    end = np.random.random()
    return {a: np.array(fr[a]) for a in DUAL + ("counts",)}, end


def test_dual_axis_inside(world, engines):
    from lidar import DualAxisLidarIntrinsics
    near, env32 = engines
    k = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
    poses = _inside_poses()[:2]
    a, end_a = _dual(near, world.mesh, k, poses, 11)
    b, end_b = _dual(env32, world.mesh, k, poses, 11)
    assert env32.scene_for(world.mesh).info["quantised_nodes"] == 0
    n = k.get_total_points_per_scan()
    share = a["counts"].sum() / (2 * n)
    _report("dual axis, env32 against near", 2 * n, share)
    assert share > INSIDE                                      # the sensor itself drops 2 %
    assert a["counts"].tolist() == b["counts"].tolist() and end_a == end_b
    for f in DUAL:
        assert_bit_equal(b[f], a[f], f"dual axis env32 against near: {f}")


def test_dual_axis_far(world, engines):
    """One pose at x = 18, max_range 200.  The scan pattern is a full circle with a 35 degree fan of elevations, of which
    the wall x = 4 (3 m x 2.5 m, 14 m away) covers 12.2 of 360 degrees and 10.2 of 35: about 64 000 x 0.034 x 0.29 = 630
    rays can return, whatever the poses.  The share guard of the other far cases cannot hold for this sensor; half of that
    estimate (the lines nod by +-5 degrees and 2 % of the rays are dropped) is asserted instead: at least 300 returns."""
    from lidar import DualAxisLidarIntrinsics, create_lidar
    near, env32 = engines
    k = dataclasses.replace(DualAxisLidarIntrinsics.create_blk2go_dual_axis(), max_range=FAR_RANGE)
    m = _far_poses()[1]
    m[:3, :3] = np.eye(3)                                      # the pattern turns a full circle: no aiming
    assert far_poses_of(m[None], world.grid).all()
    a, end_a = _dual(near, world.mesh, k, [m], 12)
    b, end_b = _dual(env32, world.mesh, k, [m], 12)
    total = int(a["counts"].sum())
    _report("dual axis, far pose on near against env32", k.get_total_points_per_scan(), total / k.get_total_points_per_scan())
    assert total >= 300
    assert a["counts"].tolist() == b["counts"].tolist() and end_a == end_b
    for f in DUAL:
        assert_bit_equal(b[f], a[f], f"dual axis far, env32 against near: {f}")
    # the frames' own rays from the host generator, cast as explicit rays: the 1e-5 m of test_dual_axis_device_generation
    np.random.seed(12)
    rays, _ = create_lidar(k, m).all_rays_and_mask()
    res = env32.cast_rays(rays[b["index"]], world.mesh, center=m[:3, 3], max_range=FAR_RANGE, want=("t", "point3"))
    assert np.isfinite(res["t_hit"]).all()
    worst = np.abs(res["points"].astype(np.float64) - b["point3"]).max()
    print(f"[f32 routes] dual axis far: largest coordinate difference to the host rays' cast {worst:.3e} m")
    assert worst <= 1e-5


# ---- 5. scan pipeline ---------------------------------------------------------------------------------------------------------
def _check_pipe(scene, dirs, batches, max_range, what, share_min, split, oracle=None, expect=None):
    """Three submits between waits with 0 (automatic), 1 and 4 lines per tile, against lrc_scan_poses_dev +
    lrc_compact_dev of the same scene; the serial rows themselves against the oracle's: ``oracle`` = (OracleMesh, sensor)
    for a sensor's table, ``expect`` = (OracleMesh, tri_sem, tri_ins) for any table (labels included)."""
    import torch
    import lidarcast
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    N, W = len(dirs), 128
    H, P = N // W, len(batches[0])
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    d_poses = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in batches]
    refs = [_reference(scene, dp, d_dirs, P, N, max_range, st) for dp in d_poses]
    share = float(np.mean([(hits["t"].cpu().numpy() != np.inf).mean() for hits, _, _ in refs]))
    _report(what, len(batches) * P * N, share)
    assert share > share_min
    if oracle is not None:
        for b, (hits, ref_rows, ref_counts) in enumerate(refs):
            rows = _oracle_rows(oracle[0], oracle[1], batches[b])
            assert [len(r) for r in rows] == ref_counts.cpu().tolist(), f"{what}, batch {b}: counts against the oracle"
            kk = int(ref_counts.sum().item())
            assert_bit_equal(ref_rows[:kk, :3].cpu().numpy(), np.concatenate(rows), f"{what}, batch {b}: rows against the oracle")
    if expect is not None:
        for b, (hits, ref_rows, ref_counts) in enumerate(refs):
            rays, cen = table_rays(dirs, batches[b].reshape(P, 4, 4))
            want = fp.expected_scan(expect[0], rays, cen, max_range, P, expect[1], expect[2])
            assert want["counts"].tolist() == ref_counts.cpu().tolist(), f"{what}, batch {b}: counts against the oracle"
            assert_bit_equal(ref_rows[:len(want["rows"])].cpu().numpy(), want["rows"], f"{what}, batch {b}: rows against the oracle")
    for lines in (0, 1, 4):
        pipe = lidarcast.ScanPipe(scene, P, N)
        pipe.set_tile_lines(lines)
        subs = []
        for dp in d_poses:
            rows = torch.full((P * N, 4), -7.0, dtype=torch.float32, device=dev)
            counts = torch.full((P,), -1, dtype=torch.int64, device=dev)
            ticket = pipe.submit(dp, d_dirs, max_range, out_rows_t=rows, counts_t=counts, stream=st)
            subs.append((ticket, rows, counts))
            ran = (_line_tiles(pipe), _hook(pipe, "lrc_internal_pipe_tile_lines"))
            assert ran == ((0, 1) if lines == 1 else (W // 64, _widest(H, split, 4))), (lines, ran)
        pipe.wait(st)
        torch.cuda.synchronize()
        for b, (ticket, rows, counts) in enumerate(subs):
            hits, ref_rows, ref_counts = refs[b]
            tag = f"{what}, lines {lines}, submit {b}"
            assert torch.equal(counts, ref_counts), f"{tag}: per-pose counts differ"
            kk = int(ref_counts.sum().item())
            assert kk > 0
            assert torch.equal(rows[:kk].view(torch.int32), ref_rows[:kk].view(torch.int32)), f"{tag}: rows differ"
            assert bool((rows[kk:] == -7.0).all()), f"{tag}: rows beyond the kept ones were touched"
            _check_records(pipe, ticket, hits, P * N)
        pipe.close()


@pytest.mark.parametrize("kind", ["env32", "shifted"])
def test_scan_pipeline(world, kind):
    """lidarcast.ScanPipe, 9 lines x 128 with the horizon crossing inside a would-be group of four."""
    from lidar import IndoorLidar
    w = world
    scene, om, _, _, share_min, _ = _kind(w, kind)
    sensor = _sensor(9, 2)
    dirs = IndoorLidar(sensor, np.eye(4)).sensor_directions()
    rng = np.random.default_rng(92)
    batches = [_pipe_poses(3, rng) for _ in range(3)]
    if kind == "shifted":
        for b in batches:
            b[:, [3, 7, 11]] += SHIFT
    _check_pipe(scene, dirs, batches, sensor.max_range, f"pipeline, {kind}", share_min, 2,
                oracle=(om, sensor) if kind == "shifted" else None, expect=(om, w.sem, w.ins))


def test_scan_pipeline_far_poses(world):
    """The same on ``near`` with every pose far: the QN = 1 kernel's float32 route under lean records and line groups."""
    w = world
    rng = np.random.default_rng(93)
    poses = np.stack([aimed_pose(CENTRE, d, yaw=y, pitch=-abs(p), roll=r)
                      for d, y, p, r in zip(rng.uniform(20.0, 98.0, 9), rng.uniform(-0.4, 0.4, 9), rng.uniform(0.0, 0.3, 9),
                                            rng.uniform(-0.5, 0.5, 9))])
    poses[0], poses[4] = _far_poses()[0], _far_poses()[1]
    assert far_poses_of(poses, w.grid).all()
    dirs = beam_table([1.0, 0.4] + list(np.linspace(-0.1, -1.1, 7)), 128, 1.5)      # 2 lines above the horizon, 7 below
    z = dirs[::128, 2]
    assert int(np.argmax((z < 0) != (z[0] < 0))) == 2
    _check_pipe(w.near, dirs, [poses[i:i + 3].reshape(3, 16) for i in (0, 3, 6)], FAR_RANGE, "pipeline, far poses on near",
                FAR, 2, expect=(w.om, w.sem, w.ins))


# ---- 6. traversal counters ----------------------------------------------------------------------------------------------------
def test_traversal_counters(world):
    """lrc_debug_scan_stats on ``env32``: trace_kernel<1, ..., STATS, 0>."""
    import lidarcast
    from lidarcast._capi import LRC_STATS_WORDS
    w = world
    poses, dirs = _inside_poses(), _ring(4, 100)
    P, N = len(poses), len(dirs)
    hit = np.isfinite(tno._clean_dev(w.env32, poses, dirs, 20.0, want=("t",))["t"])
    _report("traversal counters, env32", P * N, float(hit.mean()))
    assert hit.mean() > INSIDE
    st = w.env32.scan_stats(poses, dirs, 20.0)
    assert st.shape == (P * N, LRC_STATS_WORDS)
    assert (st[hit, 0] > 0).all() and (st[hit, 1] >= 1).all()
    assert not st[:, 4].any()                                   # the pad clause rejects nothing
    # exactly P * N rows are filled: a buffer with 64 more rows keeps them
    big = np.full((P * N + 64, LRC_STATS_WORDS), 0xA5A5A5A5, dtype=np.uint32)
    p64, d64 = np.ascontiguousarray(poses, np.float64).reshape(-1, 16), np.ascontiguousarray(dirs, np.float64)
    rc = lidarcast.load().lrc_debug_scan_stats(w.env32._h, C.c_void_p(p64.ctypes.data), P, C.c_void_p(d64.ctypes.data), N,
                                               20.0, C.c_void_p(big.ctypes.data))
    assert rc == 0
    assert np.array_equal(big[:P * N], st) and (big[P * N:] == 0xA5A5A5A5).all()
