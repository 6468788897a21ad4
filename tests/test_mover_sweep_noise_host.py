"""CPU: the seeded sensor noise under movers in sweeps (lrc_scan_noisy_mover_sweeps_*, include/lidarcast.h "seeded sensor noise
under movers in sweeps") without a GPU.  The comparator of the GPU tests (tests/mover_sweep_noise_restate.py) runs here over the
CPU oracle's cast: the all-zero model must give mover_sweep_restate.scan, a set without movers the noisy-sweep restatement
assembled on its own, a sensor and movers that stand still mover_noise_restate.scan under the start poses; and on the inputs of the
GPU cases the oracle alone must show what those cases are for.  Then the new symbols and their signatures, the refusals that need no
device, the simulator entry ``motion: {movers: {sensor_noise: ...}}`` with everything it refuses, and the tracks file.

The physical check is the crossing box of tests/test_mover_sweeps_host.py under the sensor record's jitter and dropout with
range_std = 0.  Measured with the oracle on the inputs below (seed 1): 128 of the 1536 rays end on the box (132 in the clean
sweep, 4 of them dropped); mapped by the pose at their own time they lie within 5.001e-7 m of its surface (recorded as 5.01e-7 m;
bound 4 x that = 2.004e-6 m); mapped by the sweep-start pose the farthest lies 0.301 m off."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import mover_noise_restate as mnr
import mover_restate as mv
import mover_sweep_noise_restate as msn
import mover_sweep_restate as ms
import noisy_sweep_restate as nsr
import sweep_restate
from conftest import REPO
from helpers import assert_bit_equal
from test_mover_noise_host import COLUMNS, PATH, RIG, RIGID, WALKER, assert_same, key, oracle_cast, sim_with
from test_mover_sweeps_gpu import inputs, mover_records

MEASURED_ON_BOX = 5.01e-7          # metres: the largest distance over the oracle, measured here
BOUND_ON_BOX = 4.0 * MEASURED_ON_BOX

SHAPES = [(N, P, M) for N in (40, 64, 200) for P in (1, 3) for M in (1, 3)]


@pytest.fixture(scope="module")
def world():
    """The room and the three movers behind the oracle's cast: computed once, left unchanged."""
    return {"cs": oracle_cast(mv.room_mesh()), "cm": [oracle_cast(m) for m in msn.mover_meshes()], "tab": msn.table()}


def test_all_zero_model_is_the_clean_sweep_restatement(world):
    w = world
    dirs, fire, _, motion, rays, cen = inputs(200, 3)
    rec = mover_records(3, 3)
    for max_range, opts in ((2.2, {}), (20.0, {}), (20.0, dict(min_range=1.4, incident_mode=1))):
        want, win = ms.scan(w["cs"], w["cm"], rays, cen, fire, rec, 200, max_range, **opts)
        got, gwin, info = msn.scan(w["cs"], w["cm"], motion, dirs, fire, rec, msn.zero_model(9), max_range, tab=w["tab"], **opts)
        assert info["keep"].all() and not info["term"].any()
        assert_bit_equal(info["rays"], rays, "the clean swept rays")
        assert_same(got, want, f"all-zero model, max_range {max_range}, {opts}")
        assert_bit_equal(gwin["t"], win["t"], "winners")
        assert np.array_equal(gwin["mover"], win["mover"]) and (np.bincount(want["mover"], minlength=4) > 0).all()


def test_without_movers_it_is_the_noisy_sweep_restatement(world):
    """No mover: the restated noisy swept rays (NaN directions for the dropped ones) cast as they stand, the range term added, the
    record assembled about c(s) -- against mover_sweep_noise_restate.scan with an empty set."""
    w = world
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    model = msn.model_of(range_std=0.3)
    rays, cen, term, keep, _ = nsr.noisy_sweep_rays(motion, dirs, fire, model, *w["tab"])
    cast = w["cs"](rays)                              # a NaN direction meets nothing
    assert np.isinf(cast["t"][~keep]).all() and (~keep).sum() > 10
    t = (cast["t"] + term).astype(np.float32)
    t[~(t > 0)] = np.inf
    win = dict(cast, t=t, mover=np.zeros(len(t), np.uint8))
    want = mv.record(win, np.where(keep[:, None], rays, np.float32(1)), cen, 2.5)
    got, _, _ = msn.scan(w["cs"], [], motion, dirs, fire, None, model, 2.5, tab=w["tab"])
    assert not got["mover"].any() and 100 < got["keep"].sum() < keep.sum()
    assert_same(got, want, "no movers")


def test_all_standing_still_is_the_noisy_mover_restatement(world):
    """Records whose end is their start and still mover records: mover_noise_restate.scan under the start poses, every column."""
    w = world
    for N in (64, 200):
        dirs, fire, start, motion, _, _ = inputs(N, 3, moving=False)
        rec = mover_records(3, 3, moving=False)
        assert all(ms.still(r) for r in rec.reshape(-1, 24))
        model = msn.model_of(angle_std=msn.JITTER)
        want, _, winfo = mnr.scan(w["cs"], w["cm"], start, dirs, np.ascontiguousarray(rec[:, :, :12]), model, 2.2, tab=w["tab"])
        got, _, info = msn.scan(w["cs"], w["cm"], motion, dirs, fire, rec, model, 2.2, tab=w["tab"])
        assert np.array_equal(info["keep"], winfo["keep"]) and (np.bincount(want["mover"], minlength=4) > 0).all()
        assert_same(got, want, f"all still, N {N}")


@pytest.mark.parametrize("N,P,M", SHAPES)
def test_the_gpu_cases_exercise_every_step(world, N, P, M):
    """On the inputs of the GPU parity cases, over the oracle: a mover wins rays in every sweep, a ray the clean sweep gives to a
    mover is dropped, and -- from 64 rays per sweep on -- a jitter of 0.5 degrees changes a winner.  (At 40 rays and one sweep no
    seed below 12 moves a winner: the case then checks the jittered ranges only.)"""
    w = world
    dirs, fire, _, motion, _, _ = inputs(N, P)
    rec = mover_records(P, M)
    _, cwin, _ = msn.scan(w["cs"], w["cm"][:M], motion, dirs, fire, rec, msn.zero_model(), 2.2, tab=w["tab"])
    for name, model in (("sensor record", msn.model_of()), ("jitter", msn.model_of(angle_std=msn.JITTER))):
        want, win, info = msn.scan(w["cs"], w["cm"][:M], motion, dirs, fire, rec, model, 2.2, tab=w["tab"])
        per_sweep, dropped, moved = msn.conditions(want, win, info, cwin, N)
        print(f"\n[mover sweep noise] N {N}, P {P}, M {M}, {name}: movers win at least {per_sweep} rays per sweep, {dropped} of a "
              f"mover's rays are dropped, {moved} kept rays change their winner")
        assert per_sweep >= 1 and dropped >= 1
        assert np.isinf(want["t"][~info["keep"]]).all() and not want["mover"][~info["keep"]].any()
        if name == "jitter" and N >= 64:
            assert moved >= 1


def test_a_range_draw_as_large_as_the_room(world):
    """range_std = 3 m, max_range = 4 m: returns at t' <= 0 and beyond max_range occur on movers, and both lose their mover byte."""
    w = world
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    want, win, info = msn.scan(w["cs"], w["cm"], motion, dirs, fire, mover_records(3, 3), msn.model_of(range_std=3.0), 4.0, tab=w["tab"])
    with np.errstate(invalid="ignore"):
        tn = win["t"] + info["term"]
    hit = win["t"] < np.inf
    negative, far = hit & (tn <= 0), hit & (tn > 4.0)
    assert (negative & (win["mover"] != 0)).sum() >= 10 and (far & (win["mover"] != 0)).sum() >= 10
    assert not want["mover"][negative | far].any() and np.isinf(want["t"][negative | far]).all()
    assert (want["mover"] != 0).sum() >= 10


# ---- the physical check ---------------------------------------------------------------------------------------------------------------

def test_points_on_a_moving_box_lie_on_the_box_at_their_own_time(world):
    from lidarcast.movers import MoverTrack, sweep_records
    w = world
    k, dirs, fire, motion, path = ms.crossing_inputs()
    rec = sweep_records([MoverTrack(path)], [0.0], [ms.SWEEP_T])
    model = msn.model_of(range_std=0.0)
    _, cwin, _ = msn.scan(w["cs"], w["cm"][:1], motion, dirs, fire, rec, msn.zero_model(), k.max_range, tab=w["tab"])
    out, win, info = msn.scan(w["cs"], w["cm"][:1], motion, dirs, fire, rec, model, k.max_range, tab=w["tab"])
    assert (cwin["mover"] == 1).sum() == 132 and len(dirs) == 1536
    on = out["mover"] == 1
    dropped = int(((cwin["mover"] == 1) & ~info["keep"]).sum())
    s = fire[np.flatnonzero(on) % len(dirs)]
    own = ms.box_distance(out["point3"][on], s, rec[0, 0])
    frozen = ms.box_distance(out["point3"][on], np.zeros(int(on.sum())), rec[0, 0])
    print(f"\n[mover sweep noise] oracle: {int(on.sum())} of {len(on)} rays end on the box ({dropped} of the clean sweep's 132 are "
          f"dropped); by the pose at their own time they lie within {own.max():.3e} m of its surface (bound {BOUND_ON_BOX:.3e} m), by "
          f"the sweep-start pose within {frozen.max():.3f} m")
    assert on.sum() >= 50 and dropped >= 1
    assert own.max() < 1e-4                       # otherwise the arithmetic is wrong, not the bound
    assert own.max() <= BOUND_ON_BOX
    assert frozen.max() > 0.1                     # the box moves 1 m during the sweep: the frozen scan cannot pass
    assert np.ptp(s) > 0.05 and (out["ins"][on] == 77).all()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

NEW = ("lrc_scan_noisy_mover_sweeps_dev", "lrc_scan_noisy_mover_sweeps_compact")


def test_new_symbols_load_and_match_the_header():
    from lidarcast import _capi
    lib = _capi.load()
    header = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    width = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        args = [a.strip() for a in re.search(rf"\bint {name}\((.*?)\);", src, re.S).group(1).split(",")]
        got = getattr(lib, name).argtypes
        assert len(got) == len(args), (name, args)
        for a, g in zip(args, got):
            if "*" in a:
                assert g is C.c_void_p or issubclass(g, C._Pointer), (name, a, g)
            else:
                assert g is width[a.split()[0]], (name, a, g)
    assert "seeded sensor noise under movers in sweeps" in header and "DESIGN.md section 5t" in header


def test_refusals_that_need_no_device():
    from lidarcast import _capi
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    hits, fr, nz = _capi.LrcHits(), _capi.LrcFrames(), _capi.LrcNoise()
    total = C.c_uint64(5)
    assert lib.lrc_scan_noisy_mover_sweeps_dev(None, None, None, 0, None, None, 0, None, 1.0, C.byref(nz), C.byref(hits), None,
                                               None) == E
    assert b"lrc_scan_noisy_mover_sweeps_dev: NULL scene or output" in lib.lrc_last_error()
    assert lib.lrc_scan_noisy_mover_sweeps_compact(None, None, None, 0, None, None, 1.0, C.byref(nz), C.byref(fr), None, 0,
                                                   C.byref(total)) == E
    assert b"lrc_scan_noisy_mover_sweeps_compact: NULL scene or output" in lib.lrc_last_error() and total.value == 0


def test_python_entry_points_exist():
    from lidarcast import deform, movers
    for name in ("scan_noisy_mover_sweeps_dev", "scan_noisy_mover_sweeps_compact", "scan_noisy_mover_sweep_frames"):
        sig = inspect.signature(getattr(movers, name)).parameters
        assert "noise" in sig and sig["noise"].default is inspect.Parameter.empty, name
    assert list(inspect.signature(movers.scan_noisy_mover_sweeps_dev).parameters) == [
        "scene", "motion_t", "dirs_t", "fire_t", "hits", "max_range", "movers", "mover_records_t", "noise", "mover_t", "stream"]
    for f in (deform.scan_deforming_sweeps_dev, deform.scan_deforming_sweep_frames):
        assert inspect.signature(f).parameters["noise"].default is None


# ---- the simulator entry -----------------------------------------------------------------------------------------------------------

def nested(**kw):
    return {"motion": {"speed": 0.5, "movers": key(**kw)}}


def test_simulator_sensor_noise_entry():
    assert sim_with(nested())._mover_plan(nested=True)["noise"] is None
    got = sim_with(nested(sensor_noise={"seed": 7}))._mover_plan(nested=True)["noise"]
    assert (got.seed, got.range_std, got.dropout, got.first_frame) == (7, 0.01, 0.05, 0)          # the sensor record's defaults
    assert np.isclose(np.rad2deg(got.angle_std), 0.005)
    got = sim_with(nested(sensor_noise={"seed": 2 ** 40 + 1, "range_std": 0.2, "angle_std_deg": 0.5, "dropout": 0.0}))
    got = got._mover_plan(nested=True)["noise"]
    assert (got.seed, got.range_std, got.dropout) == (2 ** 40 + 1, 0.2, 0.0) and got.angle_std == float(np.deg2rad(0.5))
    # rigid, keyframed and skinned objects all stand under the entry; animated ones need per_ray_shape, as without it
    plan = sim_with(nested(objects=[RIGID, WALKER, RIG], sensor_noise={"seed": 1}, per_ray_shape=True))._mover_plan(nested=True)
    assert plan["noise"].seed == 1 and [c is not None for c in plan["clips"]] == [False, True, True] and plan["per_ray_shape"]
    assert plan["skins"][2] is not None and plan["keyframes"][1] is not None
    with pytest.raises(ValueError, match="animation is not available under motion.movers"):
        sim_with(nested(objects=[RIGID, WALKER], sensor_noise={"seed": 1}))._mover_plan(nested=True)
    import s3dis_simulator
    assert "sensor_noise" in s3dis_simulator.S3DISSimulator._mover_plan.__doc__
    assert "not called ``noise``" in s3dis_simulator.S3DISSimulator._mover_plan.__doc__


def test_simulator_sensor_noise_refusals():
    for bad in (7, "seven", [7], True):
        with pytest.raises(ValueError, match="motion.movers.sensor_noise key must be a mapping with a seed"):
            sim_with(nested(sensor_noise=bad))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.sensor_noise key needs a seed"):
        sim_with(nested(sensor_noise={"range_std": 0.1}))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="unknown entries under the motion.movers.sensor_noise key"):
        sim_with(nested(sensor_noise={"seed": 1, "angle_std": 0.1}))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.flow is not available beside motion.movers.sensor_noise.*its own surface "
                                         "would occlude it"):
        sim_with(nested(sensor_noise={"seed": 1}, flow=True))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.nonrigid_flow is not available beside motion.movers.sensor_noise.*its own "
                                         "surface would occlude it"):
        sim_with(nested(objects=[RIGID, WALKER], per_ray_shape=True, sensor_noise={"seed": 1}, nonrigid_flow=True))._mover_plan(nested=True)
    # without the entry flow under sweeps is refused as before
    with pytest.raises(ValueError, match="scene flow under moving-sensor sweeps is not built"):
        sim_with(nested(flow=True))._mover_plan(nested=True)
    # sensor_noise belongs under motion.movers only
    with pytest.raises(ValueError, match="unknown entries under the movers key"):
        sim_with({"movers": key(sensor_noise={"seed": 1})})._mover_plan()
    # the two pinned refusals still raise, with and without the new entry beside them
    with pytest.raises(ValueError, match="unknown entries under the motion.movers key"):
        sim_with(nested(noise={"seed": 1}))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="unknown entries under the motion.movers key"):
        sim_with(nested(noise={"seed": 1}, sensor_noise={"seed": 1}))._mover_plan(nested=True)
    for movers_key in (key(), key(sensor_noise={"seed": 2})):
        with pytest.raises(ValueError, match="motion.movers cannot be combined with motion.noise.*motion: {speed, movers: "
                                             "{sensor_noise"):
            sim_with({"motion": {"speed": 1.0, "movers": movers_key, "noise": {"seed": 1}}})._mover_plan(nested=True)
    for other in ("beam", "materials"):
        with pytest.raises(ValueError, match=f"motion.movers cannot be combined with the {other} key"):
            sim_with(dict(nested(sensor_noise={"seed": 1}), **{other: {}}))._mover_plan(nested=True)


class _Group:
    """stands for a multi-rank process group: the simulator asks no more of it before it refuses"""


def test_simulator_refuses_sensor_noise_on_other_sensors_groups_and_exporters(monkeypatch, tmp_path):
    import s3dis_simulator
    from lidar import DualAxisLidarIntrinsics, Indoor8LineLidarIntrinsics
    from trajectory import Waypoint

    class Scene:
        scene_name, room_mesh = "fab", None

        class room_bounds:
            @staticmethod
            def get_volume():
                return 1.0
    wp = [Waypoint(1.0, 1.0, 1.0, 0.0)]
    sim = sim_with(nested(sensor_noise={"seed": 7}))
    sim.scene, sim.raycast_engine, sim.bug_compatible = Scene(), object(), True
    sim.lidar_config = DualAxisLidarIntrinsics()
    with pytest.raises(NotImplementedError, match="moving-sensor sweeps need a multi-line sensor"):
        sim.run_simulation(wp, process_group=s3dis_simulator._NO_GROUP)
    sim.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
    import lidarcast.distributed as dist
    monkeypatch.setattr(dist, "active_group", lambda g: (object(), _Group()))
    with pytest.raises(NotImplementedError, match="moving-sensor sweeps are not available on a multi-rank process group"):
        sim.run_simulation(wp)
    # the coverage, occupancy and frame-annotation exporters keep raising, as they do under motion
    with pytest.raises(NotImplementedError, match="surface coverage of moving-sensor sweeps is outside its scope"):
        sim.evaluate_surface_coverage(wp)
    with pytest.raises(NotImplementedError, match="occupancy grids of moving-sensor sweeps are outside their scope"):
        sim.export_occupancy_grid(wp, tmp_path)
    with pytest.raises(NotImplementedError, match="frame annotations of moving-sensor sweeps are outside their scope"):
        sim.export_frame_annotations(wp, tmp_path)


def test_tracks_file_with_and_without_the_entry(tmp_path):
    from containers import S3DISSimScene
    from lidarcast.movers import sweep_records
    P, T = 3, 0.1
    files = {}
    for name, extra in (("noisy", dict(sensor_noise={"seed": 7, "dropout": 0.1})), ("plain", {})):
        plan = sim_with(nested(**extra))._mover_plan(nested=True)
        times = np.arange(P) * plan["period"]
        records = sweep_records(plan["tracks"], times, times + T)
        scene = S3DISSimScene("fab")
        scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                              "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1), "poses12": records[:, :, :12],
                              "end_states": np.stack([t.state(times + T) for t in plan["tracks"]], axis=1), "records24": records,
                              "sweep_duration": T}
        if plan["noise"] is not None:
            scene.mover_tracks["noise"] = plan["noise"]
        ids = [np.array([0, 0, 1, 1, 1], np.uint8), np.array([], np.uint8), np.array([1, 0], np.uint8)]

        class Frame:
            def __init__(self, m):
                self.mover_ids = m
        scene.frames = [Frame(m) for m in ids]
        out = scene.export_mover_tracks(tmp_path / name)
        files[name] = json.load(open(tmp_path / name / "fab_mover_tracks.json"))
        assert files[name] == json.loads(json.dumps(out))
    disk = files["noisy"]
    assert disk["noise"]["seed"] == 7 and disk["noise"]["range_std"] == 0.01 and disk["noise"]["dropout"] == 0.1
    assert np.isclose(disk["noise"]["angle_std_deg"], 0.005) and disk["noise"]["first_frame"] == 0
    assert [f["returns"] for f in disk["frames"]] == [5, 0, 2]
    assert all(f["returns"] == f["static_points"] + sum(m["num_points"] for m in f["movers"]) for f in disk["frames"])
    assert all(f["sweep_duration"] == T and "record24" in f["movers"][0] for f in disk["frames"])
    # without the entry the file is as it was: no model, no returns, everything else the same
    plain = files["plain"]
    assert "noise" not in plain and all("returns" not in f for f in plain["frames"])
    del disk["noise"]
    for f in disk["frames"]:
        del f["returns"]
    assert disk == plain
