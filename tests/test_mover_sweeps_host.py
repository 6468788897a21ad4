"""CPU: the host side of the movers under moving-sensor sweeps (lrc_mover_sweep_rays, lrc_mover_sweep_normals, the checks that
need no device, lidarcast.movers.sweep_records, the simulator's nested key, the tracks file).  The two host functions are
compared bit for bit with the numpy restatement of the header's text (tests/mover_sweep_restate.py).

The physical check runs the whole composition on the CPU -- lidarcast.movers.sweep_rays -> the oracle's explicit-ray cast ->
sweep_normals -> merge -> the write-back restatement -- on a box that crosses the line of sight at 10 m/s during one 0.1 s
sweep, and maps every point the box returned into the box's frame in float64 by the pose at the point's own time.

Measured with the oracle on the inputs below: 132 of the 1536 rays end on the box; mapped by the pose at their own time they lie
within 2.971e-7 m of its surface (recorded as 2.98e-7 m; bound 4 x that = 1.192e-6 m); mapped by the sweep-start pose the
farthest lies 0.301 m off."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import mover_restate as mv
import mover_sweep_restate as ms
import sweep_restate
from conftest import REPO
from helpers import assert_bit_equal, random_rays
from test_movers_host import KEY, oracle_cast, pose12_of, rotations, sim_with

MEASURED_ON_BOX = 2.98e-7          # metres: the largest distance of the host composition, measured here
BOUND_ON_BOX = 4.0 * MEASURED_ON_BOX


def quat_of(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * a])


def record_of(R, c, dq=(1.0, 0.0, 0.0, 0.0), dc=(0.0, 0.0, 0.0)):
    out = np.zeros(24, np.float32)
    out[:12] = pose12_of(R, c)
    out[12:16] = np.asarray(dq, np.float64).astype(np.float32)
    out[16:19] = np.asarray(dc, np.float64).astype(np.float32)
    return out


RECORDS = {      # name -> (dq, dc)
    "general": (quat_of((0.3, -0.5, 0.8), 0.9), (0.7, -0.4, 0.15)),
    "rotation only": (quat_of((0.0, 0.0, 1.0), -1.3), (0.0, 0.0, 0.0)),
    "translation only": ((1.0, 0.0, 0.0, 0.0), (1.0, 0.25, -0.5)),
    "quarter turn": (quat_of((1.0, 1.0, 0.0), np.pi / 2), (-0.2, 0.0, 0.3)),
}


def fires(n, seed):
    """firing fractions in [0, 1) with s = 0 and the largest float64 below 1 among them"""
    f = np.random.default_rng(seed).random(n)
    f[::17] = 0.0
    f[5] = np.nextafter(1.0, 0.0)
    return f


# ---- 1: the two host functions against the restatement --------------------------------------------------------------------------

@pytest.mark.parametrize("which", sorted(RECORDS))
@pytest.mark.parametrize("start", ["identity", "yaw", "general"])
def test_sweep_rays_and_normals_equal_the_restatement_bit_for_bit(which, start):
    from lidarcast import movers
    dq, dc = RECORDS[which]
    for seed, c in ((1, (0.0, 0.0, 0.0)), (2, (1.8, -2.6, 0.4)), (3, (-31.5, 12.25, 7.0))):
        rec = record_of(rotations()[start], c, dq, dc)
        assert not ms.still(rec)
        rays = random_rays(777, -6.0, 6.0, seed=seed, unit=seed != 2)
        fire = fires(len(rays), seed)
        rays[0:40:4, :3] = rec[[3, 7, 11]]                         # origins at the mover's start centre (s = 0 among them: e = 0)
        s32 = fire.astype(np.float32)
        at = np.stack([rec[3] + s32 * rec[16], rec[7] + s32 * rec[17], rec[11] + s32 * rec[18]], 1)
        rays[100:140] = np.concatenate([at[100:140], rays[100:140, 3:]], 1)       # ... and at its centre at the ray's own s
        rays[200:230, 3] = 0.0                                     # direction components of +0.0 and -0.0
        rays[215:245, 4] = -0.0
        rays[240:260, 5] = 0.0
        got = movers.sweep_rays(rays, fire, rec)
        assert_bit_equal(got, ms.to_object_at(rays, fire, rec), f"{which}, {start} start, centre {c}: rays")
        assert (fire == 0.0).sum() > 40 and not got[100:140, :3].any()
        n3 = random_rays(777, 0.0, 0.0, seed=seed + 10)[:, 3:].copy()
        n3[::9, 0], n3[::11, 2] = 0.0, -0.0
        assert_bit_equal(movers.sweep_normals(n3, fire, rec), ms.to_world_at(n3, fire, rec), f"{which}, {start} start: normals")


def test_the_sweep_moves_the_mover_as_the_record_says():
    """Not bits: at s the object-frame ray is the world ray under the inverse of the float64 pose at s, to float32 rounding."""
    from lidarcast import movers
    dq, dc = RECORDS["general"]
    R0, c0 = rotations()["general"], np.array([1.8, -2.6, 0.4])
    rec = record_of(R0, c0, dq, dc)
    rays = random_rays(300, -6.0, 6.0, seed=8)
    fire = fires(300, 8)
    got = movers.sweep_rays(rays, fire, rec).astype(np.float64)
    back = movers.sweep_normals(got[:, 3:].astype(np.float32), fire, rec).astype(np.float64)
    for i in range(300):
        q = np.array([(1 - fire[i]) + fire[i] * dq[0], *(fire[i] * np.asarray(dq[1:]))])
        R = sweep_restate.quat_matrix(q / np.linalg.norm(q)) @ R0
        c = c0 + fire[i] * np.asarray(dc)
        assert np.abs(got[i, :3] - R.T @ (rays[i, :3].astype(np.float64) - c)).max() < 2e-5
        assert np.abs(got[i, 3:] - R.T @ rays[i, 3:].astype(np.float64)).max() < 2e-6
        assert np.abs(back[i] - rays[i, 3:]).max() < 2e-6           # to_world_at undoes to_object_at on a direction


# ---- 2: a still record --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", ["identity", "yaw", "general"])
def test_a_still_record_is_the_frozen_mover_for_every_s(start):
    from lidarcast import movers
    p12 = pose12_of(rotations()[start], (1.8, -2.6, 0.4))
    rec = ms.still_record(p12)
    assert ms.still(rec)
    rays = random_rays(500, -6.0, 6.0, seed=4)
    n3 = random_rays(500, 0.0, 0.0, seed=5)[:, 3:].copy()
    frozen = movers.rays(rays, p12)
    for fire in (np.zeros(500), fires(500, 6), np.full(500, np.nextafter(1.0, 0.0))):
        assert_bit_equal(movers.sweep_rays(rays, fire, rec), frozen, f"{start}: rays")
        assert_bit_equal(movers.sweep_normals(n3, fire, rec), mv.to_world(n3, p12), f"{start}: normals")
    minus = rec.copy()
    minus[13] = -0.0                 # a -0.0 is no still record: the general path, which differs in signed zeros at most
    assert not ms.still(minus)
    assert_bit_equal(movers.sweep_rays(rays, fires(500, 6), minus), ms.to_object_at(rays, fires(500, 6), minus))
    assert np.array_equal(movers.sweep_rays(rays, fires(500, 6), minus), frozen) or start != "identity"


# ---- 3: the records of tracks ---------------------------------------------------------------------------------------------------------

def test_sweep_records():
    from lidarcast.movers import MoverTrack, sweep_records
    walk = MoverTrack([[0.0, 1.0, 2.0, 0.0, 170.0], [0.4, 3.0, 1.0, 0.5, -170.0]])        # 20 degrees across +-180 in 0.4 s
    post = MoverTrack([[0.0, 3.0, 1.0, 0.0, 45.0]])
    t0 = np.array([0.0, 0.1, 0.3, 1.0])
    t1 = t0 + 0.1
    rec = sweep_records([walk, post], t0, t1)
    assert rec.shape == (4, 2, 24) and rec.dtype == np.float32 and not rec[..., 19:].any()
    assert_bit_equal(rec[:, 0, :12], walk.poses12(t0))
    for k in range(4):                               # the post stands still, and so does the walker once its path has ended
        assert ms.still(rec[k, 1])
    assert ms.still(rec[3, 0]) and not ms.still(rec[0, 0])
    a, b = walk.state(t0), walk.state(t1)
    for k in range(3):
        r = rec[k, 0].astype(np.float64)
        half = np.deg2rad(5.0) / 2                    # the shorter arc: +5 degrees per 0.1 s, not -345
        assert np.allclose(r[12:16], [np.cos(half), 0.0, 0.0, np.sin(half)], atol=1e-7) and r[15] > 0
        R_end = sweep_restate.quat_matrix(r[12:16] / np.linalg.norm(r[12:16])) @ r[:12].reshape(3, 4)[:, :3]
        want = mv.pose12(*b[k]).astype(np.float64).reshape(3, 4)
        assert np.abs(R_end - want[:, :3]).max() < 4 * 2.0 ** -24          # float32 rounding of the entries of two factors
        assert np.abs((r[[3, 7, 11]] + r[16:19]) - want[:, 3]).max() < 4 * 2.0 ** -24 * 4.0
        assert np.allclose(r[16:19], b[k, :3] - a[k, :3], atol=1e-7)
    # the track's own yaw jumps by a full turn at a knot behind +-180 (180 at t = 0.05, -160 at t = 0.15): still the shorter arc
    turn = MoverTrack([[0.0, 0.0, 0.0, 0.0, 170.0], [0.1, 0.0, 0.0, 0.0, -170.0], [0.2, 0.0, 0.0, 0.0, -150.0]])
    a, b = turn.state([0.05]), turn.state([0.15])
    assert np.isclose(np.rad2deg(b[0, 3] - a[0, 3]), -340.0)
    r = sweep_records([turn], [0.05], [0.15])[0, 0].astype(np.float64)
    assert np.allclose(r[12:16], [np.cos(np.deg2rad(10.0)), 0.0, 0.0, np.sin(np.deg2rad(10.0))], atol=1e-7)
    # across the knot of a path the record cuts straight from the pose at the start to the pose at the end
    bend = MoverTrack([[0.0, 0.0, 0.0, 0.0, 0.0], [0.05, 1.0, 0.0, 0.0, 0.0], [0.1, 1.0, 1.0, 0.0, 0.0]])
    r = sweep_records([bend], [0.0], [0.1])[0, 0]
    assert r[16:19].tolist() == [1.0, 1.0, 0.0]
    spin = MoverTrack([[0.0, 0.0, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0, 91.0]])
    with pytest.raises(ValueError, match="at most pi/2 per sweep"):
        sweep_records([spin], [0.0], [0.1])
    assert sweep_records([spin], [0.0], [0.09]).shape == (1, 1, 24)
    with pytest.raises(ValueError):
        sweep_records([spin], [0.0, 0.1], [0.1])


# ---- 4: the physical check ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crossing():
    """The box crossing the line of sight during one sweep, scanned by the host composition over the oracle: computed once."""
    from lidarcast.movers import MoverTrack, sweep_records
    k, dirs, fire, motion, path = ms.crossing_inputs()
    room, box = mv.room_mesh(), ms.box_mover()
    assert len(box.triangles) == 12
    rec = sweep_records([MoverTrack(path)], [0.0], [ms.SWEEP_T])
    rays, cen = sweep_restate.sweep_rays(motion, dirs, fire)
    out, win = ms.compose_host(oracle_cast(room), [oracle_cast(box)], rays, cen, fire, rec, len(dirs), k.max_range)
    return {"k": k, "dirs": dirs, "fire": fire, "motion": motion, "rec": rec, "rays": rays, "cen": cen, "out": out, "win": win,
            "room": room, "box": box}


def test_points_on_a_moving_box_lie_on_the_box_at_their_own_time(crossing):
    w = crossing
    on = w["out"]["mover"] == 1
    s = w["fire"][np.flatnonzero(on) % len(w["dirs"])]
    point_times = s * ms.SWEEP_T
    pts = w["out"]["point3"][on]
    own = ms.box_distance(pts, point_times / ms.SWEEP_T, w["rec"][0, 0])
    frozen = ms.box_distance(pts, np.zeros(len(pts)), w["rec"][0, 0])
    print(f"\n[mover sweeps] host composition: {int(on.sum())} of {len(on)} rays end on the box; by the pose at their own time they "
          f"lie within {own.max():.3e} m of its surface (bound {BOUND_ON_BOX:.3e} m), by the sweep-start pose within {frozen.max():.3f} m")
    assert on.sum() >= 50
    assert own.max() < 1e-4                       # otherwise the arithmetic is wrong, not the bound
    assert own.max() <= BOUND_ON_BOX
    assert frozen.max() > 0.1                     # the box moves 1 m during the sweep: the frozen scan cannot pass
    assert np.ptp(s) > 0.05 and (w["out"]["ins"][on] == 77).all()


def test_the_host_composition_is_the_restatement(crossing):
    """the library's host steps and the numpy restatement of the header give the same record, bit for bit"""
    w = crossing
    want, _ = ms.scan(oracle_cast(w["room"]), [oracle_cast(w["box"])], w["rays"], w["cen"], w["fire"], w["rec"], len(w["dirs"]),
                      w["k"].max_range)
    for a in ("t", "prim", "normal3", "point3", "sem", "ins", "intensity", "mover"):
        assert np.array_equal(w["out"][a].view(np.uint8), want[a].view(np.uint8)), a


# ---- symbols, layouts, refusals ---------------------------------------------------------------------------------------------------

NEW = ("lrc_scan_mover_sweeps_dev", "lrc_scan_mover_sweeps_compact", "lrc_mover_sweep_rays", "lrc_mover_sweep_normals")


def test_new_symbols_and_signatures():
    from lidarcast import _capi
    lib = _capi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lidarcast.h")).read(), flags=re.S)
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


def test_refusals_that_need_no_device():
    from lidarcast import _capi
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    hits, fr = _capi.LrcHits(), _capi.LrcFrames()
    assert lib.lrc_scan_mover_sweeps_dev(None, None, None, 0, None, None, 0, None, 1.0, C.byref(hits), None, None) == E
    assert lib.lrc_scan_mover_sweeps_compact(None, None, None, 0, None, None, 1.0, C.byref(fr), None, 0, None) == E
    rays, out = np.zeros((2, 6), np.float32), np.zeros((2, 6), np.float32)
    fire, rec = np.zeros(2), ms.still_record(mv.pose12(0, 0, 0, 0))
    for fn, width in ((lib.lrc_mover_sweep_rays, 6), (lib.lrc_mover_sweep_normals, 3)):
        a, b = rays[:, :width].copy(), out[:, :width].copy()
        assert fn(a.ctypes.data, fire.ctypes.data, 2, rec.ctypes.data, b.ctypes.data) == 0
        assert fn(a.ctypes.data, fire.ctypes.data, 2, None, b.ctypes.data) == E
        assert fn(a.ctypes.data, None, 2, rec.ctypes.data, b.ctypes.data) == E
        assert fn(None, fire.ctypes.data, 2, rec.ctypes.data, b.ctypes.data) == E
        assert fn(None, None, 0, rec.ctypes.data, None) == 0
    from lidarcast import movers
    with pytest.raises(ValueError, match="one firing fraction per row"):
        movers.sweep_rays(rays, np.zeros(3), rec)


def test_no_public_method_was_added():
    """the feature lives in lidarcast.movers: module functions, the scene and the engine are arguments"""
    import inspect
    from lidarcast import movers
    for name, first in (("sweep_records", "tracks"), ("sweep_rays", "rays6"), ("sweep_normals", "normal3"),
                        ("scan_mover_sweeps_dev", "scene"), ("scan_mover_sweeps_compact", "scene"),
                        ("scan_mover_sweep_frames", "engine")):
        assert list(inspect.signature(getattr(movers, name)).parameters)[0] == first, name


# ---- 5: the simulator key -----------------------------------------------------------------------------------------------------------

def test_simulator_nested_key():
    assert sim_with({"motion": {"speed": 0.5}})._mover_plan(nested=True) is None
    plan = sim_with({"motion": {"speed": 0.5, "movers": KEY}})._mover_plan(nested=True)
    assert plan["period"] == 0.1 and len(plan["meshes"]) == 2 and len(plan["tracks"]) == 2 and plan["flow"] is False
    assert sim_with({"motion": {"speed": 0.5, "movers": KEY}})._mover_plan() is None          # the top-level key is another key
    with pytest.raises(ValueError, match="movers key cannot be combined with the motion key"):
        sim_with({"movers": KEY, "motion": {"speed": 1.0}})._mover_plan()
    with pytest.raises(ValueError, match="motion.movers cannot be combined with motion.noise"):
        sim_with({"motion": {"speed": 0.5, "movers": KEY, "noise": {"seed": 1}}})._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.flow is not available"):
        sim_with({"motion": {"speed": 0.5, "movers": dict(KEY, flow=True)}})._mover_plan(nested=True)
    for other, cfg in (("beam", {"divergence_mrad": 3.0}), ("materials", {"classes": {}})):
        with pytest.raises(ValueError, match=f"motion.movers cannot be combined with the {other} key"):
            sim_with({"motion": {"speed": 0.5, "movers": KEY}, other: cfg})._mover_plan(nested=True)
    with pytest.raises(ValueError, match=r"unknown entries under the motion.movers key: \['speed'\]"):
        sim_with({"motion": {"movers": dict(KEY, speed=1.0)}})._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.period must be a positive number"):
        sim_with({"motion": {"movers": dict(KEY, period=0.0)}})._mover_plan(nested=True)
    sim = sim_with({"motion": {"speed": 0.5, "movers": KEY}})
    for export in (lambda: sim.evaluate_surface_coverage([]), lambda: sim.export_occupancy_grid([], "unused"),
                   lambda: sim.export_frame_annotations([], "unused")):
        with pytest.raises(NotImplementedError, match="moving-sensor sweeps"):
            export()


class _Group:
    """stands for a multi-rank process group: the simulator asks no more of it before it refuses"""


def test_simulator_refuses_the_nested_key_on_other_sensors_groups_and_keys(monkeypatch):
    import s3dis_simulator
    from lidar import DualAxisLidarIntrinsics, Indoor8LineLidarIntrinsics
    from trajectory import Waypoint

    class Scene:
        scene_name, room_mesh = "fab", None

        class room_bounds:
            @staticmethod
            def get_volume():
                return 1.0

    class Engine:
        def sweep_inputs(self, *a):
            return "motion", "fire", 0.1
    wp = [Waypoint(1.0, 1.0, 1.0, 0.0)]

    def sim_of(config, sensor):
        sim = sim_with(config)
        sim.scene, sim.raycast_engine, sim.bug_compatible, sim.lidar_config = Scene(), Engine(), True, sensor
        return sim
    nested = {"motion": {"speed": 0.5, "movers": KEY}}
    line = Indoor8LineLidarIntrinsics.create_standard_8line()
    with pytest.raises(NotImplementedError, match="moving-sensor sweeps need a multi-line sensor"):
        sim_of(nested, DualAxisLidarIntrinsics()).run_simulation(wp, process_group=s3dis_simulator._NO_GROUP)
    for config, message in ((dict(nested, beam={"divergence_mrad": 3.0}), "motion.movers cannot be combined with the beam key"),
                            (dict(nested, materials={"classes": {}}), "materials key cannot be combined with the motion key"),
                            ({"motion": dict(nested["motion"], noise={"seed": 1})}, "motion.movers cannot be combined with motion.noise"),
                            ({"motion": {"movers": dict(KEY, flow=True)}}, "motion.movers.flow is not available"),
                            (dict(nested, movers=KEY), "movers key cannot be combined with the motion key")):
        with pytest.raises(ValueError, match=message):
            sim_of(config, line).run_simulation(wp, process_group=s3dis_simulator._NO_GROUP)
    import lidarcast.distributed as dist
    monkeypatch.setattr(dist, "active_group", lambda g: (object(), _Group()))
    with pytest.raises(NotImplementedError, match="moving-sensor sweeps are not available on a multi-rank process group"):
        sim_of(nested, line).run_simulation(wp)


def test_tracks_file_carries_the_end_poses(tmp_path):
    from containers import S3DISSimScene
    from lidarcast.movers import sweep_records
    plan = sim_with({"motion": {"movers": KEY}})._mover_plan(nested=True)
    P, T = 2, 0.05
    times = np.arange(P) * plan["period"]
    rec = sweep_records(plan["tracks"], times, times + T)
    scene = S3DISSimScene("fab")
    scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                          "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1), "poses12": rec[:, :, :12],
                          "end_states": np.stack([t.state(times + T) for t in plan["tracks"]], axis=1), "records24": rec,
                          "sweep_duration": T}

    class Frame:
        def __init__(self, m):
            self.mover_ids = m
    scene.frames = [Frame(np.array([0, 1, 1], np.uint8)), Frame(np.array([2], np.uint8))]
    out = scene.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "fab_mover_tracks.json"))
    assert disk == json.loads(json.dumps(out))
    assert [f["sweep_duration"] for f in disk["frames"]] == [T, T]
    m0 = disk["frames"][0]["movers"][0]          # the first mover walks (1.0, -0.8) m and turns 80 degrees in 0.2 s
    assert np.allclose([m0["end_pose"]["x"], m0["end_pose"]["y"], m0["end_pose"]["yaw_deg"]], [1.8 + 0.25, 2.6 - 0.2, 20.0 + 20.0])
    assert np.allclose(m0["record24"], rec[0, 0]) and len(m0["record24"]) == 24
    still = disk["frames"][1]["movers"][1]
    assert still["end_pose"]["x"] == still["pose"]["x"] and still["record24"][12] == 1.0 and not any(still["record24"][13:])
