"""-m gpu: what the Python binding layer (lidarcast.core.Scene's *_compact methods, the engine's frame methods) promises
whatever its inside looks like.  One small closed room, P = 3 poses, N = 256 directions (4 lines x 64), max_range short enough
that part of every scan is cut off: an empty and an untouched compaction both fail the 10 % .. 95 % share each case asserts.

  - every table-driven family returns the same dict -- keys, key order, dtypes, every array bit for bit -- for a plain (N, 3)
    array and for a caller's DirectionTable of it, in the recorded key order, every per-row column ``total`` rows long, and
    leaves the caller's table usable;
  - a closed table and a table of another context are refused by every family with the binding's own messages;
  - the sweeps' fire rules; echoes and the engine's sweeps with and without ``index`` asked for;
  - ``keep`` as bool, as uint8 and as None (all ones) for the two generators that take a mask."""
import numpy as np
import pytest

import helpers
from helpers import pose, sensor_small, table_rays

pytestmark = pytest.mark.gpu

P, LINES, WIDTH = 3, 4, 64
N = LINES * WIDTH
MAX_RANGE = 2.3            # the room is 5 x 4 x 3 m: about half of the rays of a pose inside it end within 2.3 m
WANT = ("point3", "sem", "ins", "incident_deg", "index", "range_origin")
TAIL = ("counts", "total")
SIDE = {"poses": (), "sweeps": (), "noisy": (), "echoes": ("beam_index", "echo_index", "echo_weight"),
        "materials": ("intensity", "bounces", "surface_point3"), "movers": ("mover",)}
SIDE_DTYPES = {"beam_index": np.uint32, "echo_index": np.uint8, "echo_weight": np.uint8, "intensity": np.float32,
               "bounces": np.uint8, "surface_point3": np.float32, "mover": np.uint8}
FAMILIES = tuple(SIDE)


def assert_same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.itemsize == 1 or a.ndim == 0:
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), what
    else:
        helpers.assert_bit_equal(a, b, what)


def assert_same_dict(a, b, what):
    assert list(a) == list(b), (what, list(a), list(b))
    for k in a:
        assert_same(a[k], b[k], f"{what}: {k}")


def share(out, records, what):
    """The kept share of a case's records, printed, and held inside (10 %, 95 %)."""
    s = out["total"] / records
    print(f"\n[binding scaffold] {what}: kept {out['total']} of {records} = {100 * s:.1f} %")
    assert 0.10 < s < 0.95, (what, s)
    assert int(out["counts"].sum()) == out["total"] and (out["counts"] > 0).all(), what
    return s


class World:
    pass


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


@pytest.fixture(scope="module")
def world(engine):
    from lidar import IndoorLidar
    from lidarcast import motion_records, synth
    from lidarcast.echo import BeamModel
    from lidarcast.material import MaterialTable
    from lidarcast.movers import MoverSet, MoverTrack
    from lidarcast.noise import NoiseModel
    w = World()
    w.ctx = engine.ctx
    w.k = sensor_small(lines=LINES, width=WIDTH, max_range=MAX_RANGE)
    w.mesh = synth.make_room(size=(5.0, 4.0, 3.0), num_boxes=4, seed=6, cell=0.1)
    w.scene = engine.scene_for(w.mesh)
    sensor = IndoorLidar(w.k, np.eye(4))
    w.dirs, w.fire = sensor.sensor_directions(), sensor.firing_fractions()
    assert w.dirs.shape == (N, 3) and w.fire.shape == (N,)
    w.poses = np.stack([pose(1.5, 2.0, 1.2, 0.3), pose(2.5, 1.6, 1.0, 1.1), pose(3.5, 2.2, 1.4, -0.7)])
    w.ends = np.stack([pose(1.6, 2.0, 1.2, 0.35), pose(2.5, 1.7, 1.0, 1.15), pose(3.4, 2.2, 1.4, -0.75)])
    w.motion = motion_records(w.poses, w.ends)
    w.noise = NoiseModel(seed=7, range_std=0.01, angle_std=0.001, dropout=0.1, first_frame=5)
    w.beam = BeamModel(np.deg2rad(1.0), pattern="hex7", max_echoes=2, separation=0.05)
    w.materials = MaterialTable.from_classes({"table": {"kind": "glass", "albedo": 0.3, "pass": 0.7},
                                              "bookcase": {"kind": "mirror", "albedo": 0.1, "pass": 0.9},
                                              "wall": {"albedo": 0.8}})
    w.movers = MoverSet(w.ctx, [synth.make_pedestrian(semantic=13, instance=1001)])
    w.mover_poses = MoverTrack([[0.0, 1.8, 2.4, 0.0, 0.0], [2.0, 3.0, 1.8, 0.0, 90.0]]).poses12(np.arange(P)).reshape(P, 1, 12)
    yield w
    w.movers.close()
    w.materials.close()


def scan(w, family, dirs, want=WANT, scene=None):
    """One scan of ``family``; ``dirs`` a plain array or a DirectionTable (for sweeps: one that carries ``w.fire``)."""
    import lidarcast
    s = w.scene if scene is None else scene
    if family == "poses":
        return s.scan_poses_compact(w.poses, dirs, MAX_RANGE, want=want)
    if family == "sweeps":
        fire = None if isinstance(dirs, lidarcast.DirectionTable) else w.fire
        return s.scan_sweeps_compact(w.motion, dirs, fire, MAX_RANGE, want=want)
    if family == "noisy":
        return s.scan_noisy_compact(w.poses, dirs, MAX_RANGE, w.noise, want=want)
    if family == "echoes":
        return s.scan_echoes_compact(w.poses, dirs, MAX_RANGE, w.beam, want=want)
    if family == "materials":
        return s.scan_materials_compact(w.poses, dirs, MAX_RANGE, w.materials, want=want)
    if family == "movers":
        return s.scan_movers_compact(w.poses, dirs, MAX_RANGE, w.movers, w.mover_poses, want=want)
    raise KeyError(family)


@pytest.mark.parametrize("family", FAMILIES)
def test_plain_array_and_callers_table_give_the_same_dict(world, family):
    import lidarcast
    w = world
    table = lidarcast.DirectionTable(w.ctx, w.dirs, w.fire if family == "sweeps" else None)
    try:
        plain = scan(w, family, w.dirs)
        resident = scan(w, family, table)
        records = P * N * (w.beam.max_echoes if family == "echoes" else 1)
        share(plain, records, f"{family}, plain array")
        assert_same_dict(plain, resident, family)
        # the dict itself: the frame columns in the order asked for, counts and total, then the family's per-row columns
        assert tuple(plain) == WANT + TAIL + SIDE[family], (family, tuple(plain))
        assert plain["counts"].dtype == np.int64 and plain["counts"].shape == (P,) and type(plain["total"]) is int
        for key in WANT + SIDE[family]:
            assert len(plain[key]) == plain["total"], (family, key, plain[key].shape)
        for key in SIDE[family]:
            assert plain[key].dtype == SIDE_DTYPES[key], (family, key, plain[key].dtype)
        if family == "echoes":
            E = w.beam.max_echoes
            assert_same(plain["beam_index"], plain["index"] // np.uint32(E), "beam_index")
            assert_same(plain["echo_index"], (plain["index"] % np.uint32(E)).astype(np.uint8), "echo_index")
            assert plain["echo_weight"].min() >= 1 and plain["echo_weight"].max() <= w.beam.subrays
        if family == "materials":
            assert plain["surface_point3"].shape == (plain["total"], 3) and np.isfinite(plain["intensity"]).all()
        if family == "movers":
            assert set(np.unique(plain["mover"])) == {0, 1}        # the room and the one mover both return rays
        # the caller's table was neither closed nor replaced: it scans again, to the same rows
        assert table._h and table.n == N
        assert_same_dict(resident, scan(w, family, table), f"{family}, table used again")
    finally:
        table.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_closed_and_foreign_tables_are_refused(world, family):
    import lidarcast
    w = world
    fire = w.fire if family == "sweeps" else None
    closed = lidarcast.DirectionTable(w.ctx, w.dirs, fire)
    closed.close()
    with pytest.raises(ValueError, match="direction table handle is closed"):
        scan(w, family, closed)
    other = lidarcast.Context(w.ctx.device)
    try:
        foreign = lidarcast.DirectionTable(other, w.dirs, fire)
        with pytest.raises(ValueError, match=r"direction table belongs to another context \(device\)"):
            scan(w, family, foreign)
        foreign.close()
    finally:
        other.close()


def test_sweep_fire_rules(world):
    import lidarcast
    w = world
    with pytest.raises(ValueError, match="fire is required with a plain direction table"):
        w.scene.scan_sweeps_compact(w.motion, w.dirs, None, MAX_RANGE)
    table = lidarcast.DirectionTable(w.ctx, w.dirs)
    try:
        with pytest.raises(ValueError, match="the direction table has no firing fractions"):
            w.scene.scan_sweeps_compact(w.motion, table, None, MAX_RANGE)
        # a fire table passed beside a resident table is uploaded into it
        got = w.scene.scan_sweeps_compact(w.motion, table, w.fire, MAX_RANGE, want=WANT)
        assert table.fire is not None and np.array_equal(table.fire, w.fire)
        assert_same_dict(got, scan(w, "sweeps", w.dirs), "fire uploaded into the caller's table")
    finally:
        table.close()


def test_echoes_with_and_without_index(world):
    w = world
    want = ("point3", "sem", "ins")
    without = scan(w, "echoes", w.dirs, want=want)
    with_index = scan(w, "echoes", w.dirs, want=want + ("index",))
    share(without, P * N * w.beam.max_echoes, "echoes, index not asked for")
    assert tuple(without) == want + TAIL + SIDE["echoes"]
    assert tuple(with_index) == want + ("index",) + TAIL + SIDE["echoes"]
    for key in without:
        assert_same(without[key], with_index[key], f"echoes: {key}")
    E = np.uint32(w.beam.max_echoes)
    assert_same(with_index["index"], with_index["beam_index"] * E + with_index["echo_index"], "index")


def test_engine_sweep_frames_with_and_without_index(engine, world):
    w = world
    want = ("point3", "sem", "ins")
    without = engine.scan_sweep_frames(w.k, w.poses, w.ends, w.mesh, want=want)
    with_index = engine.scan_sweep_frames(w.k, w.poses, w.ends, w.mesh, want=want + ("index",))
    share(without, P * N, "engine sweeps, index not asked for")
    assert tuple(without) == want + TAIL + ("point_times",)
    assert tuple(with_index) == want + ("index",) + TAIL + ("point_times",)
    for key in without:
        assert_same(without[key], with_index[key], f"engine sweeps: {key}")
    assert_same(with_index["point_times"], w.fire[with_index["index"]] * (1.0 / float(w.k.scan_frequency)), "point_times")
    direct = scan(w, "sweeps", w.dirs, want=want + ("index",))       # the engine's resident table against a plain one
    for key in direct:
        assert_same(direct[key], with_index[key], f"engine sweeps against the binding: {key}")
    inputs = engine.sweep_inputs(w.k, w.poses, w.ends)
    again = engine.scan_sweep_frames(w.k, None, None, w.mesh, want=want, inputs=inputs)
    assert_same_dict(without, again, "engine sweeps from sweep_inputs")


@pytest.mark.parametrize("generator", ["angles", "rays"])
def test_keep_mask_as_bool_uint8_and_none(world, generator):
    w = world
    if generator == "angles":
        ang = np.empty((P, N, 2))
        ang[:, :, 0] = np.arctan2(w.dirs[:, 1], w.dirs[:, 0])[None, :]
        ang[:, :, 1] = np.arcsin(w.dirs[:, 2])[None, :]
        run = lambda keep: w.scene.scan_angles_compact(w.poses, ang, keep, MAX_RANGE, want=WANT)
    else:
        rays, centers = table_rays(w.dirs, w.poses)
        rays = rays.reshape(P, N, 6)
        run = lambda keep: w.scene.scan_rays_compact(rays, keep, centers, MAX_RANGE, want=WANT)
    mask = np.random.default_rng(11).random((P, N)) < 0.7
    as_bool, as_u8 = run(mask), run(mask.astype(np.uint8))
    share(as_bool, P * N, f"{generator}, 70 % mask")
    assert_same_dict(as_bool, as_u8, f"{generator}: bool against uint8 mask")
    assert_same_dict(as_bool, run(mask.reshape(-1)), f"{generator}: flat mask")
    assert_same_dict(as_bool, run(np.asfortranarray(mask)), f"{generator}: mask that is not C-contiguous")
    assert np.isin(as_bool["index"] % N + N * np.repeat(np.arange(P), as_bool["counts"]),
                   np.flatnonzero(mask)).all()                      # nothing the mask dropped comes back
    none, ones = run(None), run(np.ones((P, N), np.uint8))
    s = share(none, P * N, f"{generator}, no mask")
    assert_same_dict(none, ones, f"{generator}: None against all ones")
    assert none["total"] > as_bool["total"], s
