"""CPU: the seeded sensor noise under movers (lrc_scan_noisy_movers_*, include/lidarcast.h "seeded sensor noise under movers")
without a GPU.  The comparator of the GPU tests (tests/mover_noise_restate.py) runs here over the CPU oracle's cast: the all-zero
model must give mover_restate.scan, a set without movers the noisy restatement of tests/noise_restate.py assembled on its own, and
the sensor record's model must show on these inputs what the GPU cases are for.  Then the new symbols and their signatures, the
refusals that need no device, and the simulator key ``movers: {noise: ...}`` with everything it refuses."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import mover_noise_restate as mnr
import mover_restate as mv
import noise_restate as nr
from conftest import REPO
from helpers import assert_bit_equal, table_rays

COLUMNS = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg", "intensity", "mover", "keep")


def oracle_cast(mesh):
    """A "cast these rays" function over the CPU oracle: t, prim, sem, ins, normal3 as the oracle gives them."""
    from oracle.c_oracle import OracleMesh
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    sem_t, ins_t = np.asarray(mesh.triangle_sem, np.uint16), np.asarray(mesh.triangle_ins, np.uint16)

    def cast(rays):
        t, prim = om.cast(np.ascontiguousarray(rays, np.float32))
        hit = t < np.inf
        safe = np.where(hit, prim, 0)
        prim = np.where(hit, prim, mv.INVALID).astype(np.uint32)
        return {"t": t, "prim": prim, "sem": np.where(hit, sem_t[safe], 0).astype(np.uint16),
                "ins": np.where(hit, ins_t[safe], 0).astype(np.uint16), "normal3": om.normals(prim)}
    return cast


def sensor_model(seed=7, first_frame=5, **kw):
    """The model of the dense 32-line sensor record: 0.01 m, 0.005 degrees, 5 % dropout."""
    import dataclasses
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast.noise import NoiseModel
    m = NoiseModel.from_intrinsics(Indoor8LineLidarIntrinsics.create_dense_32line(), seed, first_frame)
    assert (m.range_std, m.dropout) == (0.01, 0.05) and np.isclose(np.rad2deg(m.angle_std), 0.005)
    return dataclasses.replace(m, **kw)


def assert_same(got, want, what):
    for a in COLUMNS:
        g, w = np.asarray(got[a]), np.asarray(want[a])
        if g.dtype.itemsize == 1:
            assert np.array_equal(g, w), f"{what}: {a}"
        else:
            assert_bit_equal(g, w, f"{what}: {a}")


@pytest.fixture(scope="module")
def world():
    """The room, the pedestrian on its walk, the three poses and the two oracle casts: computed once, left unchanged."""
    from lidarcast import synth
    room, ped = mv.room_mesh(), synth.make_pedestrian(semantic=13, instance=1001)
    k, dirs, poses = mv.scan_inputs()
    mp = np.stack([mv.pose12(*mv.walker_state(f)) for f in range(3)]).reshape(3, 1, 12)
    return {"k": k, "dirs": dirs, "poses": poses, "mp": mp, "cs": oracle_cast(room), "cm": oracle_cast(ped)}


def test_all_zero_model_is_the_clean_mover_restatement(world):
    from lidarcast.noise import NoiseModel
    w = world
    N = len(w["dirs"])
    rays, cen = table_rays(w["dirs"], w["poses"])
    for max_range, opts in ((w["k"].max_range, {}), (1.6, {}), (w["k"].max_range, dict(min_range=1.2, incident_mode=1))):
        want, win = mv.scan(w["cs"], [w["cm"]], rays, np.repeat(cen, N, axis=0), w["mp"], N, max_range, **opts)
        got, gwin, info = mnr.scan(w["cs"], [w["cm"]], w["poses"], w["dirs"], w["mp"], NoiseModel(seed=3, first_frame=9), max_range,
                                   **opts)
        assert info["keep"].all() and not info["term"].any()
        assert_bit_equal(info["rays"], rays, "the clean rays")
        assert_same(got, want, f"all-zero model, max_range {max_range}, {opts}")
        assert_bit_equal(gwin["t"], win["t"], "winners") and np.array_equal(gwin["mover"], win["mover"])
        assert (want["mover"] == 1).sum() > 10


def test_without_movers_it_is_the_noisy_restatement(world):
    """No mover: the restated noisy rays (NaN directions for the dropped ones) cast as they stand, the range term added, the
    record assembled -- the noisy scan of tests/noise_restate.py -- against mover_noise_restate.scan with an empty set."""
    w = world
    N = len(w["dirs"])
    model = sensor_model(range_std=0.3)
    base, slope = mnr.table()
    rays, cen, term, keep, _ = nr.noisy_rays(w["poses"], w["dirs"], model.seed, model.first_frame, model.range_std, model.angle_std,
                                             model.dropout, base, slope)
    cast = w["cs"](rays)                              # a NaN direction meets nothing
    assert np.isinf(cast["t"][~keep]).all() and (~keep).sum() > 30
    t = (cast["t"] + term).astype(np.float32)
    t[~(t > 0)] = np.inf
    win = dict(cast, t=t, mover=np.zeros(len(t), np.uint8))
    want = mv.record(win, np.where(keep[:, None], rays, np.float32(1)), np.repeat(cen, N, axis=0), 2.5)
    got, _, _ = mnr.scan(w["cs"], [], w["poses"], w["dirs"], None, model, 2.5)
    assert not got["mover"].any() and 100 < got["keep"].sum() < keep.sum()
    assert_same(got, want, "no movers")


def test_the_sensor_records_model_exercises_every_step(world):
    """On the issue's inputs over the oracle: a mover wins rays, a ray the clean scan gives to the mover is dropped, and a jitter
    of 0.5 degrees changes a winner -- what the GPU cases assert on their own restatement."""
    from lidarcast.noise import NoiseModel
    w = world
    clean, cwin, _ = mnr.scan(w["cs"], [w["cm"]], w["poses"], w["dirs"], w["mp"], NoiseModel(seed=7, first_frame=5), w["k"].max_range)
    got, win, info = mnr.scan(w["cs"], [w["cm"]], w["poses"], w["dirs"], w["mp"], sensor_model(), w["k"].max_range)
    assert (got["mover"] == 1).sum() >= 10
    dropped_mover = (clean["mover"] == 1) & ~info["keep"]
    assert dropped_mover.sum() >= 1
    assert np.isinf(got["t"][~info["keep"]]).all() and not got["mover"][~info["keep"]].any()
    kept = got["keep"] & clean["keep"] & (win["prim"] == cwin["prim"]) & (win["mover"] == cwin["mover"])
    assert kept.sum() > 500 and (got["t"][kept] != clean["t"][kept]).mean() > 0.9           # the range draw moves the range
    _, jwin, _ = mnr.scan(w["cs"], [w["cm"]], w["poses"], w["dirs"], w["mp"],
                          NoiseModel(seed=7, angle_std=float(np.deg2rad(0.5)), first_frame=5), w["k"].max_range)
    assert (jwin["mover"] != cwin["mover"]).sum() >= 1
    # a large range draw: returns at t' <= 0 and beyond max_range, both without a mover byte
    far, fwin, finfo = mnr.scan(w["cs"], [w["cm"]], w["poses"], w["dirs"], w["mp"], sensor_model(range_std=3.0, dropout=0.0), 4.0)
    with np.errstate(invalid="ignore"):
        tn = fwin["t"] + finfo["term"]
    assert ((fwin["t"] < np.inf) & (tn <= 0)).sum() > 10 and ((fwin["mover"] == 1) & (tn <= 0)).sum() >= 1
    assert ((fwin["mover"] == 1) & (tn > 4.5)).sum() >= 1
    assert not far["mover"][~(tn > 0) | (tn > 4.5)].any()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

NEW = ("lrc_scan_noisy_movers_dev", "lrc_scan_noisy_movers_compact")


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
    assert "seeded sensor noise under movers" in header and "DESIGN.md section 5r" in header


def test_refusals_that_need_no_device():
    from lidarcast import _capi
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    hits, fr, nz = _capi.LrcHits(), _capi.LrcFrames(), _capi.LrcNoise()
    total = C.c_uint64(5)
    assert lib.lrc_scan_noisy_movers_dev(None, None, None, 0, None, 0, None, 1.0, C.byref(nz), C.byref(hits), None, None) == E
    assert b"lrc_scan_noisy_movers_dev: NULL scene or output" in lib.lrc_last_error()
    assert lib.lrc_scan_noisy_movers_compact(None, None, None, 0, None, None, 1.0, C.byref(nz), C.byref(fr), None, 0,
                                             C.byref(total)) == E
    assert b"lrc_scan_noisy_movers_compact: NULL scene or output" in lib.lrc_last_error() and total.value == 0


def test_python_entry_points_exist():
    import lidarcast
    from lidarcast import deform
    from raycast_engine.raycast_engine_hip import RaycastEngineHIP
    for name in ("scan_noisy_movers_dev", "scan_noisy_movers_compact"):
        assert "noise" in inspect.signature(getattr(lidarcast.Scene, name)).parameters
    assert "noise" in inspect.signature(RaycastEngineHIP.scan_noisy_mover_frames).parameters
    for f in (deform.scan_deforming_dev, deform.scan_deforming_frames):
        assert inspect.signature(f).parameters["noise"].default is None


# ---- the simulator key -------------------------------------------------------------------------------------------------------------

def sim_with(config):
    import s3dis_simulator
    from lidar import Indoor8LineLidarIntrinsics
    sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
    sim.config = config
    sim.scene = object()
    sim.lidar_config = Indoor8LineLidarIntrinsics.create_dense_32line()      # 0.01 m, 0.005 degrees, 5 % dropout
    return sim


PATH = [[0.0, 1.8, 2.6, 0.0, 20.0], [0.2, 2.8, 1.8, 0.0, 100.0]]
RIGID = {"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": PATH}
WALKER = {"mesh": "walker", "instance": 1002, "path": PATH, "animation": {"cycle": 0.8}}
RIG = {"mesh": "walker_rig", "instance": 1003, "path": PATH, "animation": {"cycle": 0.8}}


def key(**kw):
    return dict({"period": 0.1, "objects": [RIGID]}, **kw)


def test_simulator_movers_noise_key():
    assert sim_with({"movers": key()})._mover_plan()["noise"] is None
    got = sim_with({"movers": key(noise={"seed": 7})})._mover_plan()["noise"]
    assert (got.seed, got.range_std, got.dropout, got.first_frame) == (7, 0.01, 0.05, 0)          # the sensor record's defaults
    assert np.isclose(np.rad2deg(got.angle_std), 0.005)
    got = sim_with({"movers": key(noise={"seed": 2 ** 40 + 1, "range_std": 0.2, "angle_std_deg": 0.5, "dropout": 0.0})})._mover_plan()["noise"]
    assert (got.seed, got.range_std, got.dropout) == (2 ** 40 + 1, 0.2, 0.0) and got.angle_std == float(np.deg2rad(0.5))
    # rigid, keyframed and skinned objects all stand under the key
    plan = sim_with({"movers": key(objects=[RIGID, WALKER, RIG], noise={"seed": 1})})._mover_plan()
    assert plan["noise"].seed == 1 and [c is not None for c in plan["clips"]] == [False, True, True]
    assert plan["skins"][2] is not None and plan["keyframes"][1] is not None


def test_simulator_movers_noise_refusals():
    for bad in (7, "seven", [7], True):
        with pytest.raises(ValueError, match="movers.noise key must be a mapping with a seed"):
            sim_with({"movers": key(noise=bad)})._mover_plan()
    with pytest.raises(ValueError, match="movers.noise key needs a seed"):
        sim_with({"movers": key(noise={"range_std": 0.1})})._mover_plan()
    with pytest.raises(ValueError, match="unknown entries under the movers.noise key"):
        sim_with({"movers": key(noise={"seed": 1, "angle_std": 0.1})})._mover_plan()
    with pytest.raises(ValueError, match="movers.flow is not available beside movers.noise.*its own surface would occlude it"):
        sim_with({"movers": key(noise={"seed": 1}, flow=True)})._mover_plan()
    with pytest.raises(ValueError, match="movers.nonrigid_flow is not available beside movers.noise.*its own surface would occlude it"):
        sim_with({"movers": key(objects=[RIGID, WALKER], noise={"seed": 1}, nonrigid_flow=True)})._mover_plan()
    # what stayed refused: a top-level noise key beside movers, motion.noise beside motion.movers (and no noise under motion.movers)
    with pytest.raises(ValueError, match="movers key cannot be combined with the noise key"):
        sim_with({"movers": key(), "noise": {"seed": 1}})._mover_plan()
    with pytest.raises(ValueError, match="movers key cannot be combined with the noise key"):
        sim_with({"movers": key(noise={"seed": 2}), "noise": {"seed": 1}})._mover_plan()
    with pytest.raises(ValueError, match="motion.movers cannot be combined with motion.noise"):
        sim_with({"motion": {"speed": 1.0, "movers": key(), "noise": {"seed": 1}}})._mover_plan(nested=True)
    with pytest.raises(ValueError, match="unknown entries under the motion.movers key"):
        sim_with({"motion": {"speed": 1.0, "movers": key(noise={"seed": 1})}})._mover_plan(nested=True)


class _Group:
    """stands for a multi-rank process group: the simulator asks no more of it before it refuses"""


def test_simulator_refuses_movers_noise_on_other_sensors_and_groups(monkeypatch):
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
    sim = sim_with({"movers": key(noise={"seed": 7})})
    sim.scene, sim.raycast_engine, sim.bug_compatible = Scene(), object(), True
    sim.lidar_config = DualAxisLidarIntrinsics()
    with pytest.raises(ValueError, match="movers key needs a multi-line sensor.*not the dual-axis sensor"):
        sim.run_simulation(wp, process_group=s3dis_simulator._NO_GROUP)
    sim.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
    import lidarcast.distributed as dist
    monkeypatch.setattr(dist, "active_group", lambda g: (object(), _Group()))
    with pytest.raises(ValueError, match="movers key is not available on a multi-rank process group"):
        sim.run_simulation(wp)


def test_tracks_file_holds_the_noise_model(tmp_path):
    from containers import S3DISSimScene
    plan = sim_with({"movers": key(noise={"seed": 7, "dropout": 0.1})})._mover_plan()
    P = 3
    times = np.arange(P) * plan["period"]
    scene = S3DISSimScene("fab")
    scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                          "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1),
                          "poses12": np.stack([t.poses12(times) for t in plan["tracks"]], axis=1), "noise": plan["noise"]}
    ids = [np.array([0, 0, 1, 1, 1], np.uint8), np.array([], np.uint8), np.array([1, 0], np.uint8)]

    class Frame:
        def __init__(self, m):
            self.mover_ids = m
    scene.frames = [Frame(m) for m in ids]
    out = scene.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "fab_mover_tracks.json"))
    assert disk == json.loads(json.dumps(out))
    assert disk["noise"]["seed"] == 7 and disk["noise"]["range_std"] == 0.01 and disk["noise"]["dropout"] == 0.1
    assert np.isclose(disk["noise"]["angle_std_deg"], 0.005) and disk["noise"]["first_frame"] == 0
    assert [f["returns"] for f in disk["frames"]] == [5, 0, 2]
    assert all(f["returns"] == f["static_points"] + sum(m["num_points"] for m in f["movers"]) for f in disk["frames"])
    # without the noise entry the file is as it was
    del scene.mover_tracks["noise"]
    plain = scene.export_mover_tracks(tmp_path)
    assert "noise" not in plain and all("returns" not in f for f in plain["frames"])
