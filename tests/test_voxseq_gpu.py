"""-m gpu: dynamic occupancy (csrc/lrc_voxseq.hip) against the numpy restatement (tests/voxseq_restate.py), bit for bit: the
hostile synthetic segments over frame slots with a skipped pose, STATIC_ONLY and min_returns; slot isolation; the tie to the
existing single grid (lrc_voxgrid) on a static scan; pose order and chunking; the analytic mover scene with its shadow; the
deforming and the noisy scan routes; the simulator's export."""
import json

import numpy as np
import pytest

import voxgrid_restate as VR
import voxseq_restate as SR

pytestmark = pytest.mark.gpu

ORIGIN, S, DIMS = (-0.5, 0.25, -1.0), 0.25, (5, 7, 33)
V = DIMS[0] * DIMS[1] * DIMS[2]
COLS = ("idx", "sem", "ins", "returns", "mover", "mover_returns")


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def device_records(t, point3, sem, ins):
    """A DeviceHits holding the given host columns."""
    import torch
    from lidarcast import DeviceHits
    h = DeviceHits(len(t), torch.device("cuda", 0), want=("t", "point3", "sem", "ins"))
    h["t"].copy_(torch.from_numpy(np.ascontiguousarray(t, np.float32)))
    h["point3"].copy_(torch.from_numpy(np.ascontiguousarray(point3, np.float32).reshape(-1, 3)))
    h["sem"].copy_(torch.from_numpy(np.ascontiguousarray(sem, np.uint16).view(np.int16)))
    h["ins"].copy_(torch.from_numpy(np.ascontiguousarray(ins, np.uint16).view(np.int16)))
    return h


def run(ctx, F, grid, origins, per_ray, fop, rec, mover, static_only=False, min_returns=(1,), chunk=None, order=None):
    """Accumulate host records into a fresh sequence of F slots (poses in ``order``, ``chunk`` poses per call) and finalize
    once per entry of ``min_returns``.  Returns ([results], free bits)."""
    import torch
    from lidarcast import OccupancySequence
    from lidarcast.deform import _HitsSlice
    t, p3, sem, ins = rec
    P = len(fop)
    N = len(t) // P
    order = np.arange(P) if order is None else np.asarray(order)
    rows = (order[:, None] * N + np.arange(N)[None, :]).reshape(-1)
    hits = device_records(np.asarray(t)[rows], np.asarray(p3).reshape(-1, 3)[rows], np.asarray(sem)[rows], np.asarray(ins)[rows])
    org = np.asarray(origins, np.float32).reshape(-1, 3)
    org_t = torch.from_numpy(np.ascontiguousarray(org[rows] if per_ray else org[order])).cuda()
    mv_t = None if mover is None else torch.from_numpy(np.ascontiguousarray(np.asarray(mover, np.uint8)[rows])).cuda()
    fop_t = torch.from_numpy(np.asarray(fop, np.int64)[order].astype(np.int32)).cuda()
    seq = OccupancySequence(ctx, grid[0], grid[1], grid[2], F)
    try:
        step = P if chunk is None else chunk
        for a in range(0, P, step):
            b = min(P, a + step)
            seq.accumulate_dev(org_t[a * N:b * N] if per_ray else org_t[a:b], _HitsSlice(hits, a * N, b * N), b - a, N,
                               mover_t=None if mv_t is None else mv_t[a * N:b * N], frame_of_pose_t=fop_t[a:b],
                               origin_per_ray=per_ray, static_only=static_only)
        return [seq.finalize(min_returns=m) for m in min_returns], seq.free_bits()
    finally:
        seq.close()


def assert_matches(res, bits, ref, what=""):
    for k in COLS + ("frame_offsets", "counts"):
        got = getattr(res, k)
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, (what, k, got.dtype, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), (what, k, int((got != ref[k]).sum()))
    assert res.skipped == ref["skipped"], what
    Vn = int(np.prod(res.dims))
    assert np.array_equal(res.state.reshape(res.frames, Vn), ref["state"]), what
    if bits is not None:
        assert np.array_equal(bits.reshape(-1), SR.pack_bits(ref["free"], Vn)), what


def same(a, b):
    for k in COLS + ("frame_offsets", "counts", "state"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.skipped == b.skipped


# ---- synthetic segments ----------------------------------------------------------------------------------------------------------
P5, N5, FOP5 = 5, 819, [2, 0, 0, 7, 1]             # 4095 of the 4096 segments; pose 3 has no slot (7 >= F = 3)


@pytest.fixture(scope="module")
def synthetic():
    o, e = SR.hostile_segments(origin=ORIGIN, s=S, dims=DIMS)
    o, e = o[:P5 * N5], e[:P5 * N5]
    rng = np.random.default_rng(11)
    n = len(o)
    t = np.ones(n, np.float32)
    t[400:][rng.random(n - 400) < 0.1] = np.inf                       # the special segments (the first 400) all return
    sem = rng.integers(0, 3, n).astype(np.uint16)
    ins = rng.integers(0, 3, n).astype(np.uint16)
    mover = rng.integers(0, 4, n).astype(np.uint8)
    refs = {}

    def ref(static_only, min_returns):
        key = (static_only, min_returns)
        if key not in refs:
            refs[key] = SR.sequence_from_records(o, True, FOP5, t, e, sem, ins, mover, 3, ORIGIN, S, DIMS, min_returns, static_only)
        return refs[key]
    return o, (t, e, sem, ins), mover, ref


@pytest.mark.parametrize("static_only", [False, True])
def test_synthetic_segments_equal_the_restatement(ctx, synthetic, static_only):
    o, rec, mover, ref = synthetic
    (r1, r2), bits = run(ctx, 3, (ORIGIN, S, DIMS), o, True, FOP5, rec, mover, static_only, min_returns=(1, 2))
    want = ref(static_only, 1)
    assert want["skipped"] == int(np.isfinite(rec[0][3 * N5:4 * N5]).sum()) > 700
    assert want["counts"][:, 4].sum() == 6 and (want["mover_returns"] > 0).any() != static_only
    assert_matches(r1, bits, want, f"static_only={static_only} min_returns=1")
    assert_matches(r2, None, ref(static_only, 2), f"static_only={static_only} min_returns=2")
    assert (r2.counts[:, 2] < r1.counts[:, 2]).any()
    if not static_only:                                     # the result object's views
        for f in range(3):
            fr = r1.frame(f)
            a, b = int(want["frame_offsets"][f]), int(want["frame_offsets"][f + 1])
            assert np.array_equal(fr.idx, want["idx"][a:b]) and fr.num_occupied == int(want["counts"][f, 2])
            i, m, n = r1.mover_of(f)
            assert np.array_equal(m, want["mover"][a:b]) and np.array_equal(n, want["mover_returns"][a:b])
            di, dm = r1.dynamic_voxels(f)
            assert np.array_equal(di, want["idx"][a:b][want["mover"][a:b] != 0]) and (dm != 0).all() and len(di) > 0


def test_null_mover_column_and_default_slots(ctx, synthetic):
    """mover NULL means all zero; a NULL frame array puts pose p into slot first_frame + p and refuses a run past the end."""
    import torch
    from lidarcast import OccupancySequence
    o, rec, mover, _ = synthetic
    t, e, sem, ins = rec
    want = SR.sequence_from_records(o, True, [1, 2, 3, 4, 5], t, e, sem, ins, None, 6, ORIGIN, S, DIMS)
    hits = device_records(t, e, sem, ins)
    org_t = torch.from_numpy(o).cuda()
    seq = OccupancySequence(ctx, ORIGIN, S, DIMS, 6)
    try:
        seq.accumulate_dev(org_t, hits, P5, N5, first_frame=1, origin_per_ray=True)
        assert_matches(seq.finalize(), seq.free_bits(), want, "first_frame=1")
        assert (want["mover"] == 0).all() and (want["counts"][0] == [0, 0, 0, V, 0, 0]).all()
        with pytest.raises(ValueError, match="exceeds num_frames"):
            seq.accumulate_dev(org_t, hits, P5, N5, first_frame=2, origin_per_ray=True)
        # the C call itself refuses records without one of t, point3, sem, ins, and an unknown flag, before any launch
        import ctypes as C
        from lidarcast import _capi
        for missing in ("t", "point3", "sem", "ins"):
            part = _capi.LrcHits()
            for a in ("t", "point3", "sem", "ins"):
                setattr(part, a, None if a == missing else hits[a].data_ptr())
            rc = seq._lib.lrc_voxseq_accumulate_dev(seq._h, org_t.data_ptr(), 1, P5, N5, None, 1, C.byref(part), None, 0, None)
            assert rc == _capi.LRC_ERR_INVALID_ARG and b"t, point3, sem and ins" in seq._lib.lrc_last_error(), missing
        rc = seq._lib.lrc_voxseq_accumulate_dev(seq._h, org_t.data_ptr(), 1, P5, N5, None, 1, C.byref(hits.struct), None, 2, None)
        assert rc == _capi.LRC_ERR_INVALID_ARG and b"unknown flag" in seq._lib.lrc_last_error()
        assert int(seq.info().reserved_keys) == P5 * N5                       # nothing was added by the refused calls
        seq.reset()
        z = seq.finalize()
        assert len(z.idx) == 0 and not z.state.any() and not seq.free_bits().any() and z.skipped == 0
        assert (z.frame_offsets == 0).all() and (z.counts[:, 3] == V).all()
    finally:
        seq.close()


# ---- slot isolation ----------------------------------------------------------------------------------------------------------------
def test_each_slot_equals_a_one_slot_sequence(ctx, synthetic):
    o, rec, mover, ref = synthetic
    (full,), bits = run(ctx, 3, (ORIGIN, S, DIMS), o, True, FOP5, rec, mover)
    for f in range(3):
        fop = [0 if x == f else 1 for x in FOP5]                     # every other pose has no slot in a one-slot sequence
        (one,), b1 = run(ctx, 1, (ORIGIN, S, DIMS), o, True, fop, rec, mover)
        a, b = int(full.frame_offsets[f]), int(full.frame_offsets[f + 1])
        for k in COLS:
            assert np.array_equal(getattr(one, k), getattr(full, k)[a:b]), (f, k)
        assert np.array_equal(one.state[0], full.state[f]) and np.array_equal(one.counts[0], full.counts[f])
        assert np.array_equal(b1[0], bits[f])


def test_a_saturated_slot_leaves_its_neighbour_clean(ctx, synthetic):
    o, rec, mover, _ = synthetic
    for full_slot in (1, 0):
        (r,), bits = run(ctx, 2, (ORIGIN, S, DIMS), o, True, [full_slot] * 5, rec, mover)
        other = 1 - full_slot
        assert not bits[other].any() and r.counts[other].tolist() == [0, 0, 0, V, 0, 0]
        assert (r.state[full_slot] != VR.UNKNOWN).mean() > 0.99         # the slot is (all but) saturated
        assert bits[full_slot, -1] >> (V % 32) == 0                     # ... and its last word has no bit at or past V


# ---- the tie to the existing grid ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static_scan(engine):
    import torch
    from helpers import pose, sensor_small
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, synth
    office = synth.make_scene("synth_A6_office2")
    dirs = np.ascontiguousarray(IndoorLidar(sensor_small(lines=8, width=64), np.eye(4)).sensor_directions(), dtype=np.float64)
    poses = np.stack([pose(0.9, 1.2, 1.0, 0.2), pose(2.0, 1.8, 1.1, 1.4), pose(3.1, 2.4, 0.9, -0.8), pose(4.1, 2.8, 1.2, 2.9)])
    scene = engine.scene_for(office)
    dev = torch.device("cuda", 0)
    hits = DeviceHits(len(poses) * len(dirs), dev, want=("t", "point3", "sem", "ins", "t_label"))
    poses_t = torch.from_numpy(poses.reshape(-1, 16)).to(dev)
    dirs_t = torch.from_numpy(dirs).to(dev)
    scene.scan_poses_dev(poses_t, dirs_t, hits, 20.0)
    torch.cuda.synchronize()
    rec = (hits["t"].cpu().numpy(), hits["point3"].cpu().numpy(), hits["sem"].cpu().numpy().view(np.uint16),
           hits["ins"].cpu().numpy().view(np.uint16))
    assert np.isfinite(rec[0]).mean() > 0.5
    return office, poses, dirs, (poses_t, dirs_t, hits), rec


def test_one_slot_without_movers_gives_the_bytes_of_the_existing_grid(ctx, engine, static_scan):
    from lidarcast import OccupancyGrid
    from lidarcast.voxgrid import default_extent
    from lidarcast.voxseq import pose_origins
    office, poses, dirs, (poses_t, dirs_t, hits), rec = static_scan
    g, dims = default_extent(office.vertices, 0.2)
    vg = OccupancyGrid(engine.ctx, g, 0.2, dims)
    try:
        vg.accumulate_dev(poses_t, dirs_t, hits["t_label"])
        want = vg.finalize()
        want_bits = vg.free_bits()
    finally:
        vg.close()
    assert want.num_occupied > 500 and want.num_free > 2000          # of 28 x 23 x 18 voxels
    org = pose_origins(poses)
    N = len(dirs)
    for per_ray, o in ((False, org), (True, np.repeat(org, N, axis=0))):
        (r,), bits = run(engine.ctx, 1, (g, 0.2, dims), o, per_ray, [0, 0, 0, 0], rec, None)
        fr = r.frame(0)
        assert np.array_equal(fr.idx, want.idx) and np.array_equal(fr.sem, want.sem) and np.array_equal(fr.ins, want.ins)
        assert np.array_equal(fr.returns, want.returns) and np.array_equal(fr.state, want.state)
        assert (fr.num_free, fr.num_occupied, fr.num_unknown, fr.rejected_rays) == \
            (want.num_free, want.num_occupied, want.num_unknown, want.rejected_rays)
        assert r.counts[0].tolist() == [len(want.idx), want.num_free, want.num_occupied, want.num_unknown, want.rejected_rays,
                                        int(want.returns.sum())]
        assert np.array_equal(bits[0], want_bits) and (r.mover == 0).all() and (r.mover_returns == 0).all()
        assert fr.per_class == want.per_class


def test_pose_order_and_chunking_do_not_matter(ctx, engine, static_scan):
    from lidarcast.voxgrid import default_extent
    from lidarcast.voxseq import pose_origins
    office, poses, dirs, _, rec = static_scan
    g, dims = default_extent(office.vertices, 0.2)
    org = pose_origins(poses)
    fop = [1, 0, 2, 1]
    mover = (np.arange(len(rec[0])) % 3 == 0).astype(np.uint8)
    (base,), bits = run(engine.ctx, 3, (g, 0.2, dims), org, False, fop, rec, mover)
    assert (base.counts[:, 2] > 0).all() and (base.mover != 0).any()
    for order, chunk in (([3, 1, 0, 2], None), (None, 1), ([2, 3, 1, 0], 1)):
        (r,), b = run(engine.ctx, 3, (g, 0.2, dims), org, False, fop, rec, mover, chunk=chunk, order=order)
        same(base, r)
        assert np.array_equal(bits, b)


# ---- the analytic mover scene -------------------------------------------------------------------------------------------------------
def sparse_dict(idx, sem, ins, mover):
    return {int(i): (int(s), int(n), int(m)) for i, s, n, m in zip(idx, sem, ins, mover)}


def test_analytic_mover_scene(engine):
    import torch
    from lidarcast import DeviceHits, Scene
    from lidarcast.movers import MoverSet
    sc = SR.analytic_scene()
    # the expectations hold on the CPU first (the oracle, lrc_mover_rays, lrc_mover_merge and the restatement)
    cpu = SR.analytic_records_on_cpu(sc)
    args = (cpu["t"], cpu["point3"], cpu["sem"], cpu["ins"], cpu["mover"])
    grid = (sc["origin"], sc["voxel"], sc["dims"])
    c2 = SR.sequence_from_records(cpu["origins"], False, [0, 1], *args, 2, *grid)
    c1 = SR.sequence_from_records(cpu["origins"], False, [0, 0], *args, 1, *grid, static_only=True)
    f = [c2["frames"][k]["sparse"] for k in (0, 1)]
    s0 = c1["frames"][0]["sparse"]
    SR.assert_axis(sc, c2["state"], lambda k: sparse_dict(f[k]["idx"], f[k]["sem"], f[k]["ins"], f[k]["mover"]), c1["state"][0],
                   sparse_dict(s0["idx"], s0["sem"], s0["ins"], s0["mover"]))
    # the GPU
    room, cube = sc["room"], sc["cube"]
    dev = torch.device("cuda", 0)
    scene = Scene(engine.ctx, room.vertices, room.triangles, room.triangle_sem, room.triangle_ins)
    mset = MoverSet(engine.ctx, [cube])
    from lidarcast import OccupancySequence, scan_dynamic_occupancy
    seq = OccupancySequence(engine.ctx, *grid, 2)
    stat = OccupancySequence(engine.ctx, *grid, 1)
    try:
        scan_dynamic_occupancy(scene, seq, sc["poses"], sc["dirs"], sc["max_range"], movers=mset, mover_poses=sc["mover_poses"],
                               static_seq=stat)
        r, s = seq.finalize(), stat.finalize()
        rbits, sbits = seq.free_bits(), stat.free_bits()
        # the scan's own records, for the restatement
        N = len(sc["dirs"])
        hits = DeviceHits(2 * N, dev, want=("t", "point3", "sem", "ins"))
        mover_t = torch.zeros(2 * N, dtype=torch.uint8, device=dev)
        scene.scan_movers_dev(torch.from_numpy(sc["poses"].reshape(-1, 16)).to(dev), torch.from_numpy(sc["dirs"]).to(dev), hits,
                              sc["max_range"], mset, torch.from_numpy(sc["mover_poses"]).to(dev), mover_t)
        torch.cuda.synchronize()
        rec = (hits["t"].cpu().numpy(), hits["point3"].cpu().numpy(), hits["sem"].cpu().numpy().view(np.uint16),
               hits["ins"].cpu().numpy().view(np.uint16), mover_t.cpu().numpy())
    finally:
        seq.close()
        stat.close()
        mset.close()
        scene.close()
    SR.assert_axis(sc, r.state.reshape(2, -1), lambda k: sparse_dict(r.frame(k).idx, r.frame(k).sem, r.frame(k).ins, r.mover_of(k)[1]),
                   s.state.reshape(-1), sparse_dict(s.idx, s.sem, s.ins, s.mover))
    org = sc["poses"][:, :3, 3].astype(np.float32)
    assert_matches(r, rbits, SR.sequence_from_records(org, False, [0, 1], *rec, 2, *grid), "per frame")
    assert_matches(s, sbits, SR.sequence_from_records(org, False, [0, 0], *rec, 1, *grid, static_only=True), "static map")
    assert (s.mover_returns == 0).all() and r.dynamic_per_mover(0).get(1, 0) > 5 and set(r.dynamic_per_mover(1)) <= {1}
    # the scan agrees with the CPU's casts on which surface every ray met
    assert np.array_equal(rec[4], cpu["mover"]) and np.array_equal(np.isfinite(rec[0]), np.isfinite(cpu["t"]))


# ---- the deforming and the noisy routes ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walker_world(engine):
    import mover_restate as mv
    from lidarcast import deform, synth
    from lidarcast.movers import MoverSet, MoverTrack
    room = mv.room_mesh()
    k, dirs, poses = mv.scan_inputs(width=100)
    w = synth.make_walker()
    d = deform.Deformable(engine.ctx, w.keyframes, w.triangles, w.triangle_sem, w.triangle_ins)
    mset = MoverSet(engine.ctx, [d])
    times = np.arange(3) * 0.2
    track = MoverTrack([[0.0, 1.8, 2.6, 0.0, 20.0], [0.4, 2.8, 1.8, 0.0, 100.0]])
    mp = track.poses12(times)[:, None, :]
    shapes = deform.Clip(len(w.keyframes), 1.0).shapes3(times)[:, None, :]
    yield room, dirs, poses, mset, mp, shapes
    mset.close()
    d.close()


def route_records(engine, world, noise):
    import torch
    from lidarcast import DeviceHits, deform
    room, dirs, poses, mset, mp, shapes = world
    dev = torch.device("cuda", 0)
    N = len(dirs)
    hits = DeviceHits(3 * N, dev, want=("t", "point3", "sem", "ins"))
    mover_t = torch.zeros(3 * N, dtype=torch.uint8, device=dev)
    deform.scan_deforming_dev(engine.scene_for(room), torch.from_numpy(poses.reshape(-1, 16)).to(dev),
                              torch.from_numpy(dirs).to(dev), hits, 20.0, mset, torch.from_numpy(np.ascontiguousarray(mp)).to(dev),
                              shapes, mover_t, noise=noise)
    torch.cuda.synchronize()
    return (hits["t"].cpu().numpy(), hits["point3"].cpu().numpy(), hits["sem"].cpu().numpy().view(np.uint16),
            hits["ins"].cpu().numpy().view(np.uint16), mover_t.cpu().numpy())


def route_result(engine, world, noise, chunk=None):
    from lidarcast import OccupancySequence, scan_dynamic_occupancy
    from lidarcast.voxgrid import default_extent
    room, dirs, poses, mset, mp, shapes = world
    g, dims = default_extent(room.vertices, 0.1)
    seq = OccupancySequence(engine.ctx, g, 0.1, dims, 3)
    try:
        scan_dynamic_occupancy(engine.scene_for(room), seq, poses, dirs, 20.0, movers=mset, mover_poses=mp, shapes=shapes,
                               noise=noise, chunk_poses=chunk)
        return seq.finalize(), seq.free_bits(), (g, 0.1, dims)
    finally:
        seq.close()


def test_deforming_route_equals_the_restatement(engine, walker_world):
    r, bits, grid = route_result(engine, walker_world, None)
    rec = route_records(engine, walker_world, None)
    org = walker_world[2][:, :3, 3].astype(np.float32)
    assert_matches(r, bits, SR.sequence_from_records(org, False, [0, 1, 2], *rec, 3, *grid), "deforming")
    assert all(r.dynamic_per_mover(f).get(1, 0) > 0 for f in range(3))
    r1, b1, _ = route_result(engine, walker_world, None, chunk=1)          # one frame per call: one shape set per chunk
    same(r, r1)
    assert np.array_equal(bits, b1)


def test_noisy_route_equals_the_restatement_and_zero_noise_is_clean(engine, walker_world):
    from lidarcast import NoiseModel
    noise = NoiseModel(seed=77, range_std=0.02, angle_std=0.002, dropout=0.1)
    r, bits, grid = route_result(engine, walker_world, noise)
    rec = route_records(engine, walker_world, noise)
    org = walker_world[2][:, :3, 3].astype(np.float32)
    assert_matches(r, bits, SR.sequence_from_records(org, False, [0, 1, 2], *rec, 3, *grid), "noisy")
    r2, b2, _ = route_result(engine, walker_world, noise, chunk=2)           # frame ids follow the chunk's first pose
    same(r, r2)
    clean, cbits, _ = route_result(engine, walker_world, None)
    assert not np.array_equal(clean.idx, r.idx)
    zero, zbits, _ = route_result(engine, walker_world, NoiseModel(seed=77))
    same(clean, zero)
    assert np.array_equal(cbits, zbits)


# ---- the simulator -------------------------------------------------------------------------------------------------------------------
def test_simulator_export_round_trips(engine, tmp_path):
    import mover_restate as mv
    import s3dis_simulator
    from lidarcast.movers import MoverSet, MoverTrack
    from lidarcast.synth import S3DIS_CLASSES, make_pedestrian
    from trajectory import line_trajectory, poses_from_waypoints
    room = mv.room_mesh()
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 3, yaw=0.6)
    path = [[0.0, 1.8, 2.6, 0.0, 20.0], [0.2, 2.8, 1.8, 0.0, 100.0]]
    key = {"period": 0.1, "objects": [{"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": path}]}
    sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}, "movers": key})
    sim.load_scene(room, "room")
    summary = sim.export_dynamic_occupancy(wps, tmp_path, voxel_size=0.2)
    poses = poses_from_waypoints(wps)
    mset = MoverSet(sim.raycast_engine.ctx, [make_pedestrian(semantic=13, instance=1001)])
    try:
        mp = MoverTrack(path).poses12(np.arange(3) * 0.1)[:, None, :]
        ref, sref = sim.raycast_engine.dynamic_occupancy(sim.lidar_config, poses, room, movers=mset, mover_poses=mp, voxel_size=0.2)
    finally:
        mset.close()
    z = np.load(tmp_path / "room_dynamic_occupancy.npz")
    zs = np.load(tmp_path / "room_static_map.npz")
    for k in COLS + ("frame_offsets", "counts", "state"):
        assert np.array_equal(z[k], getattr(ref, k)), k
        assert np.array_equal(zs[k], getattr(sref, k)), k
    assert z["state"].shape == (3,) + tuple(ref.dims) and zs["state"].shape == (1,) + tuple(ref.dims)
    assert float(z["voxel_size"]) == 0.2 and np.array_equal(z["origin"], ref.origin) and int(z["skipped"]) == 0
    with open(tmp_path / "room_dynamic_occupancy.json") as fh:
        j = json.load(fh)
    assert j == json.loads(json.dumps(summary)) and j["num_frames"] == 3 and j["num_poses"] == 3 and len(j["movers"]) == 1
    ped = dict(enumerate(S3DIS_CLASSES)).get(13, "13")                  # the summary names a class where the id is a known one
    for f in range(3):
        assert j["frames"][f]["counts"]["occupied"] == int(ref.counts[f, 2])
        assert j["frames"][f]["dynamic_voxels_per_mover"] == {str(k): v for k, v in ref.dynamic_per_mover(f).items()}
        assert j["frames"][f]["per_class_occupied_voxels"].get(ped, 0) > 0       # the pedestrian is seen
    assert sum(sum(fr["dynamic_voxels_per_mover"].values()) for fr in j["frames"]) > 0
    assert j["static_map"]["dynamic_voxels_per_mover"] == {} and (sref.mover_returns == 0).all()
    assert j["static_map"]["per_class_occupied_voxels"].get(ped, 0) == 0
    with pytest.raises(NotImplementedError, match="movers key"):
        sim.export_occupancy_grid(wps, tmp_path)
    # no feature key at all: the room alone, one grid per waypoint, no dynamic voxel
    plain = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    plain.load_scene(room, "plain")
    p = plain.export_dynamic_occupancy(wps, tmp_path, voxel_size=0.2)
    assert p["num_frames"] == 3 and p["movers"] == [] and all(fr["dynamic_voxels_per_mover"] == {} for fr in p["frames"])
    one = plain.raycast_engine.occupancy_grid(plain.lidar_config, poses[:1], room, voxel_size=0.2)
    assert p["frames"][0]["counts"]["occupied"] == one.num_occupied and p["frames"][0]["counts"]["free"] == one.num_free
