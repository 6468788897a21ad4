"""CPU: the host side of the moving objects (lrc_mover_rays, lrc_mover_merge, the checks that need no device,
lidarcast.movers.MoverTrack, the simulator key, the tracks file).  The two host functions are compared bit for bit with the numpy
restatement of the header's text (tests/mover_restate.py); the restatement over the CPU oracle is compared with the oracle on
the BAKED mesh -- the room with the mover's vertices moved in float64 and appended -- which is what a rebuild per frame would
scan.

Measured with the oracle on the inputs below: the mover wins 18 / 204 / 25 rays of the three frames, no ray ends on a different
triangle, max |t - t_baked| = 1.55e-6 m (bound 2^-18 m = 3.81e-6 m: the next power of two above twice that figure, a few
float32 ulps at 5 m)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import mover_restate as mv
from conftest import REPO
from helpers import assert_bit_equal, random_rays, table_rays


def oracle_cast(mesh):
    """A "cast these rays" function over the CPU oracle: t, prim, sem, ins, normal3 as the oracle gives them."""
    from oracle.c_oracle import OracleMesh
    om = OracleMesh(mesh.vertices, mesh.triangles).build()
    sem_t = np.zeros(len(mesh.triangles), np.uint16) if mesh.triangle_sem is None else np.asarray(mesh.triangle_sem, np.uint16)
    ins_t = np.zeros(len(mesh.triangles), np.uint16) if mesh.triangle_ins is None else np.asarray(mesh.triangle_ins, np.uint16)

    def cast(rays):
        rays = np.ascontiguousarray(rays, np.float32)
        t, prim = om.cast(rays)
        hit = t < np.inf
        safe = np.where(hit, prim, 0)
        prim = np.where(hit, prim, mv.INVALID).astype(np.uint32)
        return {"t": t, "prim": prim, "sem": np.where(hit, sem_t[safe], 0).astype(np.uint16),
                "ins": np.where(hit, ins_t[safe], 0).astype(np.uint16), "normal3": om.normals(prim)}
    return cast


@pytest.fixture(scope="module")
def world():
    """The room, the pedestrian, the three poses, the restatement over the oracle: computed once, left unchanged."""
    from lidarcast import synth
    room, ped = mv.room_mesh(), synth.make_pedestrian()
    k, dirs, poses = mv.scan_inputs()
    rays, cen = table_rays(dirs, poses)
    N = len(dirs)
    mp = np.stack([mv.pose12(*mv.walker_state(f)) for f in range(3)]).reshape(3, 1, 12)
    cs, cm = oracle_cast(room), oracle_cast(ped)
    rec, win = mv.scan(cs, [cm], rays, np.repeat(cen, N, axis=0), mp, N, k.max_range)
    return {"room": room, "ped": ped, "k": k, "N": N, "rays": rays, "cen": np.repeat(cen, N, axis=0), "mp": mp, "cs": cs, "cm": cm,
            "rec": rec, "win": win}


def rotations():
    """identity, yaw only, general (float64 matrices)"""
    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])

    def ry(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1.0, 0], [-np.sin(a), 0, np.cos(a)]])

    def rx(a):
        return np.array([[1.0, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    return {"identity": np.eye(3), "yaw": rz(0.83), "general": rz(-2.1) @ ry(0.6) @ rx(1.9)}


def pose12_of(R, c):
    m = np.zeros((3, 4))
    m[:, :3], m[:, 3] = R, c
    return mv.pose12_of(m)


# ---- the two host functions against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["identity", "yaw", "general"])
def test_mover_rays_equal_the_restatement_bit_for_bit(which):
    from lidarcast import movers
    R = rotations()[which]
    for seed, c in ((1, (0.0, 0.0, 0.0)), (2, (1.8, -2.6, 0.4)), (3, (-31.5, 12.25, 7.0))):
        rays = random_rays(777, -6.0, 6.0, seed=seed, unit=seed != 2)
        p12 = pose12_of(R, c)
        assert_bit_equal(movers.rays(rays, p12), mv.to_object(rays, p12), f"{which} rotation, centre {c}")
    if which == "identity":      # the identity at the origin changes nothing but the sign of a zero
        rays = random_rays(64, -3.0, 3.0, seed=9)
        assert np.array_equal(movers.rays(rays, pose12_of(np.eye(3), (0, 0, 0))), rays)


def fabricated_casts(n, M, seed):
    """Static and mover columns with every case of the merge: misses, a mover nearer, the static scene nearer, exact ties
    between the static scene and a mover and between two movers, misses everywhere."""
    rng = np.random.default_rng(seed)
    ts = rng.uniform(0.5, 9.0, n).astype(np.float32)
    tm = rng.uniform(0.5, 9.0, (M, n)).astype(np.float32)
    ts[rng.random(n) < 0.2] = np.inf
    tm[rng.random((M, n)) < 0.4] = np.inf
    tie_s = np.arange(n) % 7 == 0                   # static == mover 0
    tm[0, tie_s] = ts[tie_s]
    if M > 1:
        tie_m = np.arange(n) % 11 == 0              # mover 0 == mover M - 1, both nearer than anything else
        tm[0, tie_m] = tm[M - 1, tie_m] = np.float32(0.25)
    none = np.arange(n) % 13 == 0                   # misses everywhere
    ts[none] = np.inf
    tm[:, none] = np.inf

    def unit_rows(shape):
        v = rng.normal(size=shape + (3,))
        return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    ns, nm = unit_rows((n,)), unit_rows((M, n))
    ns[~(ts < np.inf)] = 0
    nm[~(tm < np.inf)] = 0
    return ts, ns, tm, nm


@pytest.mark.parametrize("M", [1, 3, 255])
def test_mover_merge_equals_the_restatement_bit_for_bit(M):
    from lidarcast import movers
    n = 500 if M < 255 else 64
    ts, ns, tm, nm = fabricated_casts(n, M, seed=M)
    rot = list(rotations().values())
    p12 = np.stack([pose12_of(rot[m % 3], (0.3 * m, -0.2 * m, 0.1)) for m in range(M)])
    z = np.zeros(n, np.uint16)
    static = {"t": ts, "prim": np.arange(n, dtype=np.uint32), "sem": z, "ins": z, "normal3": ns}
    casts = [{"t": tm[m], "prim": np.arange(n, dtype=np.uint32), "sem": z, "ins": z, "normal3": nm[m]} for m in range(M)]
    want = mv.merge(static, casts, p12)
    t, n3, who = movers.merge(ts, ns, tm, nm, p12)
    assert_bit_equal(t, want["t"], "t")
    assert_bit_equal(n3, want["normal3"], "normal3")
    assert who.tolist() == want["mover"].tolist()
    # the cases are all there, and the tie rules hold
    tie_s = (np.arange(n) % 7 == 0) & (ts < np.inf) & (np.arange(n) % 11 != 0)
    assert tie_s.any() and (who[tie_s] != 1).all()                # the static scene keeps an exact tie with mover 0
    if M > 1:
        tie_m = (np.arange(n) % 11 == 0) & (np.arange(n) % 13 != 0)
        assert tie_m.any() and (who[tie_m] == 1).all()            # the smaller m wins among movers
    none = np.arange(n) % 13 == 0
    assert (who[none] == 0).all() and np.isinf(t[none]).all() and (n3[none] == 0).all()
    assert (who == 0).any() and (who > 0).any()


def test_merge_without_movers_is_the_static_cast():
    from lidarcast import movers
    ts, ns, _, _ = fabricated_casts(100, 1, seed=5)
    t, n3, who = movers.merge(ts, ns, np.zeros((0, 100), np.float32), np.zeros((0, 100, 3), np.float32), np.zeros((0, 12), np.float32))
    assert_bit_equal(t, ts)
    assert_bit_equal(n3, ns)
    assert not who.any()


def test_filters_apply_to_the_merged_record(world):
    """min_range and max_range act on the winner's point.  Fabricated columns: rays from one centre, the static scene at
    0.3 m / 1.0 m / 4.0 m / nowhere, the mover at 2.0 m / 2.5 m / nowhere.  A near static hit that min_range removes leaves
    no return -- it does not uncover the mover behind it -- and a winning mover beyond max_range is dropped like any far return."""
    from lidarcast import movers
    ts = np.array([0.3, 0.3, 1.0, 4.0, 4.0, np.inf, np.inf, 1.0], np.float32)
    tm = np.array([2.0, np.inf, 2.0, 2.0, 2.5, 2.0, np.inf, 1.0], np.float32)
    n = len(ts)
    rays = random_rays(n, 0.0, 0.0, seed=4)
    cen = np.zeros((n, 3))
    ns = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n, 1)) * (ts < np.inf)[:, None]
    nm = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (n, 1)) * (tm < np.inf)[:, None]
    p12 = pose12_of(rotations()["yaw"], (0.5, 0.5, 0.0))
    t, n3, who = movers.merge(ts, ns, tm[None], nm[None], p12[None])
    assert who.tolist() == [0, 0, 0, 1, 1, 1, 0, 0]                      # the last ray: an exact tie, the static scene's
    z = np.zeros(n, np.uint16)
    win = {"t": t, "prim": np.arange(n, dtype=np.uint32), "sem": z, "ins": z, "normal3": n3, "mover": who}
    rec = mv.record(win, rays, cen, max_range=2.25, min_range=0.5)
    assert rec["keep"].tolist() == [False, False, True, True, False, True, False, True]
    assert rec["mover"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0]
    assert np.isinf(rec["t"][[0, 1, 4, 6]]).all() and (rec["prim"][[0, 1, 4, 6]] == mv.INVALID).all()
    assert_bit_equal(rec["normal3"][3], mv.to_world(nm[3:4], p12)[0])
    # on the scan's own inputs the host merge gives the winners the restatement filtered
    w = world
    sl = slice(w["N"], 2 * w["N"])                                      # frame 1: the mover wins 204 rays
    static, mover = w["cs"](w["rays"][sl]), w["cm"](mv.to_object(w["rays"][sl], w["mp"][1, 0]))
    t, n3, who = movers.merge(static["t"], static["normal3"], mover["t"][None], mover["normal3"][None], w["mp"][1])
    assert_bit_equal(t, w["win"]["t"][sl])
    assert_bit_equal(n3, w["win"]["normal3"][sl])
    assert who.tolist() == w["win"]["mover"][sl].tolist() and int(who.sum()) == 204
    near = float(np.median(t[who == 1]))
    rec = mv.record({k: v[sl] for k, v in w["win"].items()}, w["rays"][sl], w["cen"][sl], near)
    assert (rec["mover"][who == 1] == 1).any() and (rec["mover"][who == 1] == 0).any()      # max_range decides among the mover's rays


# ---- the restatement against the baked mesh ------------------------------------------------------------------------------------

def test_restatement_over_the_oracle_equals_the_baked_mesh(world):
    from oracle.c_oracle import OracleMesh
    w = world
    N = w["N"]
    assert len(w["room"].triangles) == 3406 and len(w["ped"].triangles) == 288
    wins, worst, differ, hits = [], 0.0, 0, 0
    for p in range(3):
        sl = slice(p * N, (p + 1) * N)
        v, t, first = mv.baked(w["room"], w["ped"], mv.walker_state(p))
        tb, pb = OracleMesh(v, t).build().cast(w["rays"][sl])
        win = {k: a[sl] for k, a in w["win"].items()}
        hit = tb < np.inf
        assert (hit == (win["t"] < np.inf)).all(), f"frame {p}: the rays with a hit differ"
        want_prim = np.where(win["mover"] == 1, win["prim"] + np.uint32(first), win["prim"])
        same = want_prim[hit] == pb[hit]
        differ += int((~same).sum())
        hits += int(hit.sum())
        worst = max(worst, float(np.abs(win["t"][hit][same].astype(np.float64) - tb[hit][same]).max()))
        wins.append(int((win["mover"] == 1).sum()))
    print(f"\n[movers] baked comparison: the mover wins {wins} rays, {differ} of {hits} rays end on a different triangle, "
          f"max |t - t_baked| = {worst:.3e} m (bound 2^-18 = {2.0 ** -18:.3e} m)")
    assert wins == [18, 204, 25]
    assert differ <= hits // 100 and differ == 0          # at most 1 % may be left out; these inputs use none of that
    assert worst <= 2.0 ** -18


# ---- symbols, layouts, refusals ------------------------------------------------------------------------------------------------

NEW = ("lrc_movers_create", "lrc_movers_destroy", "lrc_scan_movers_dev", "lrc_scan_movers_compact", "lrc_mover_rays", "lrc_mover_merge")


def test_new_symbols_load():
    from lidarcast import _capi
    lib = _capi.load()
    header = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(rf"\bint {name}\(", header), name


def test_signatures_match_the_header():
    """Every new entry point: the ctypes argument list has the header's arity, pointers as pointers, the rest by width."""
    from lidarcast import _capi
    lib = _capi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lidarcast.h")).read(), flags=re.S)
    width = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double}
    for name in NEW:
        args = [a.strip() for a in re.search(rf"\bint {name}\((.*?)\);", src, re.S).group(1).split(",")]
        got = getattr(lib, name).argtypes
        assert len(got) == len(args), (name, args)
        for a, g in zip(args, got):
            if "*" in a:
                assert g is C.c_void_p or issubclass(g, C._Pointer), (name, a, g)
            else:
                assert g is width[a.split()[0]], (name, a, g)
    from lidarcast._capi import LrcFrames, LrcHits
    assert C.sizeof(LrcHits) == 80 and C.sizeof(LrcFrames) == 96          # the structs the new calls take: unchanged


def test_refusals_that_need_no_device():
    from lidarcast import _capi
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    h = C.c_void_p()
    one = (C.c_void_p * 1)(None)
    for M in (0, 256, 1000):
        assert lib.lrc_movers_create(None, one, M, C.byref(h)) == E
        assert b"[1, 255]" in lib.lrc_last_error() and b"context" not in lib.lrc_last_error()
    assert lib.lrc_movers_create(None, one, 1, C.byref(h)) == E and b"NULL context" in lib.lrc_last_error()
    assert lib.lrc_movers_destroy(None) == 0
    hits, fr = _capi.LrcHits(), _capi.LrcFrames()
    assert lib.lrc_scan_movers_dev(None, None, None, 0, None, 0, None, 1.0, C.byref(hits), None, None) == E
    assert lib.lrc_scan_movers_compact(None, None, None, 0, None, None, 1.0, C.byref(fr), None, 0, None) == E
    rays, p12, out = np.zeros((2, 6), np.float32), mv.pose12(0, 0, 0, 0), np.zeros((2, 6), np.float32)
    assert lib.lrc_mover_rays(rays.ctypes.data, 2, p12.ctypes.data, out.ctypes.data) == 0
    assert lib.lrc_mover_rays(rays.ctypes.data, 2, None, out.ctypes.data) == E
    assert lib.lrc_mover_rays(None, 2, p12.ctypes.data, out.ctypes.data) == E
    assert lib.lrc_mover_rays(None, 0, p12.ctypes.data, None) == 0
    t, n3, who = np.zeros(2, np.float32), np.zeros((2, 3), np.float32), np.zeros(2, np.uint8)
    args = (t.ctypes.data, n3.ctypes.data, t.ctypes.data, n3.ctypes.data, p12.ctypes.data, t.ctypes.data, n3.ctypes.data, who.ctypes.data)
    assert lib.lrc_mover_merge(2, 256, *args) == E and b"255" in lib.lrc_last_error()
    assert lib.lrc_mover_merge(2, 1, None, *args[1:]) == E
    assert lib.lrc_mover_merge(2, 1, *args[:4], None, *args[5:]) == E
    assert lib.lrc_mover_merge(0, 0, *([None] * 8)) == 0


# ---- tracks ---------------------------------------------------------------------------------------------------------------------

def test_mover_track():
    from lidarcast.movers import MoverTrack, pose12
    tr = MoverTrack([[1.0, 0.0, 0.0, 0.0, 170.0], [3.0, 2.0, -4.0, 1.0, -170.0], [4.0, 2.0, -4.0, 1.0, -80.0]])
    s = tr.state([0.0, 1.0, 2.0, 3.0, 3.5, 4.0, 99.0])
    assert s[0].tolist() == s[1].tolist() and s[-1].tolist() == s[-2].tolist()            # held at both ends
    assert np.allclose(s[2, :3], [1.0, -2.0, 0.5])                                       # linear in time
    assert np.isclose(np.rad2deg(s[2, 3]), 180.0)                                        # the shorter arc: 170 -> 190, not -> -170 by way of 0
    assert np.isclose(np.rad2deg(s[3, 3]) % 360.0, 190.0) and np.isclose(np.rad2deg(s[4, 3]) % 360.0, 235.0)
    p = tr.poses12([2.0])
    assert p.dtype == np.float32 and p.shape == (1, 12)
    c, sn = np.cos(s[2, 3]), np.sin(s[2, 3])
    want = np.array([c, -sn, 0, 1.0, sn, c, 0, -2.0, 0, 0, 1, 0.5], np.float64).astype(np.float32)       # float64, narrowed last
    assert_bit_equal(p[0], want)
    assert_bit_equal(pose12(s[2:3])[0], mv.pose12(*s[2]))
    single = MoverTrack([[0.0, 1.0, 2.0, 3.0, 45.0]]).state([-1.0, 5.0])
    assert single.tolist() == [[1.0, 2.0, 3.0, np.deg2rad(45.0)]] * 2
    for bad in ([], [[0, 0, 0, 0]], [[0, 0, 0, 0, 0], [0, 1, 1, 1, 1]], [[1, 0, 0, 0, 0], [0, 1, 1, 1, 1]], [[0, np.nan, 0, 0, 0]]):
        with pytest.raises(ValueError):
            MoverTrack(bad)


def test_pedestrian_mesh():
    from lidarcast import synth
    m = synth.make_pedestrian()
    assert len(m.triangles) == 288 and m.vertices[:, 2].min() == 0.0 and m.vertices[:, 2].max() == 1.7
    v = m.vertices[m.triangles]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert (np.einsum("ij,ij->i", nrm, v.mean(1) - np.array([0, 0, 0.85])) > 0).all()          # wound outward
    e = np.sort(np.concatenate([m.triangles[:, [0, 1]], m.triangles[:, [1, 2]], m.triangles[:, [2, 0]]]), axis=1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all()                            # closed
    assert np.allclose(m.vertices[:, :2].mean(0), 0.0) and (m.triangle_sem == 13).all()
    assert len(synth.make_pedestrian(segments=5, rings=2).triangles) == 30


# ---- the simulator key ---------------------------------------------------------------------------------------------------------

def sim_with(config):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
    sim.config = config
    sim.scene = object()
    return sim


KEY = {"period": 0.1, "objects": [{"mesh": "pedestrian", "semantic": 13, "instance": 1001,
                                   "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.2, 2.8, 1.8, 0.0, 100.0]]},
                                  {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.0, 1.0, 0.0, 0.0]]}]}


def test_simulator_movers_key():
    assert sim_with({})._mover_plan() is None
    plan = sim_with({"movers": KEY})._mover_plan()
    assert plan["period"] == 0.1 and len(plan["meshes"]) == 2 and len(plan["tracks"]) == 2
    assert (plan["meshes"][0].triangle_sem == 13).all() and (plan["meshes"][0].triangle_ins == 1001).all()
    assert (plan["meshes"][1].triangle_sem == 12).all()                   # "clutter" by name
    assert plan["objects"][0]["num_triangles"] == 288 and plan["objects"][0]["box_max"][2] == 1.7
    for other, cfg in (("motion", {"speed": 1.0}), ("noise", {"seed": 1}), ("beam", {"divergence_mrad": 3.0}),
                       ("materials", {"classes": {}})):
        with pytest.raises(ValueError, match=f"movers key cannot be combined with the {other} key"):
            sim_with({"movers": KEY, other: cfg})._mover_plan()
    with pytest.raises(ValueError, match="unknown entries under the movers key"):
        sim_with({"movers": dict(KEY, speed=1.0)})._mover_plan()
    with pytest.raises(ValueError, match="unknown entries of mover 0"):
        sim_with({"movers": {"objects": [dict(KEY["objects"][0], colour="red")]}})._mover_plan()
    for bad in ({"objects": []}, {"period": 0.0, "objects": KEY["objects"]}, {"objects": [{"mesh": "pedestrian"}]},
                {"objects": [{"path": [[0, 0, 0, 0, 0]], "semantic": "person"}]}, {"objects": [{"path": [[0, 0, 0, 0]]}]},
                {"objects": [{"path": [[0, 0, 0, 0, 0]], "instance": 70000}]}, {"objects": KEY["objects"][:1] * 256}):
        with pytest.raises(ValueError):
            sim_with({"movers": bad})._mover_plan()
    sim = sim_with({"movers": KEY})
    for export in (lambda: sim.evaluate_surface_coverage([]), lambda: sim.export_occupancy_grid([], "unused"),
                   lambda: sim.export_frame_annotations([], "unused")):
        with pytest.raises(NotImplementedError, match="movers key"):
            export()


class _Group:
    """stands for a multi-rank process group: the simulator asks no more of it before it refuses"""


def test_simulator_refuses_movers_on_other_sensors_and_groups(monkeypatch):
    """the dual-axis sensor and a multi-rank group are refused before anything is scanned"""
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
    sim = sim_with({"movers": KEY})
    sim.scene, sim.raycast_engine, sim.bug_compatible = Scene(), object(), True
    sim.lidar_config = DualAxisLidarIntrinsics()
    with pytest.raises(ValueError, match="movers key needs a multi-line sensor"):
        sim.run_simulation(wp, process_group=s3dis_simulator._NO_GROUP)
    sim.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
    import lidarcast.distributed as dist
    monkeypatch.setattr(dist, "active_group", lambda g: (object(), _Group()))
    with pytest.raises(ValueError, match="movers key is not available on a multi-rank process group"):
        sim.run_simulation(wp)


def test_tracks_file_from_a_fabricated_frame_list(tmp_path):
    from containers import S3DISSimScene
    from lidarcast.movers import MoverTrack
    plan = sim_with({"movers": KEY})._mover_plan()
    P = 3
    times = np.arange(P) * plan["period"]
    scene = S3DISSimScene("fab")
    with pytest.raises(ValueError, match="movers key"):
        scene.export_mover_tracks(tmp_path)
    scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                          "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1),
                          "poses12": np.stack([t.poses12(times) for t in plan["tracks"]], axis=1)}
    ids = [np.array([0, 0, 1, 1, 1, 2], np.uint8), np.array([], np.uint8), np.array([2, 2, 0], np.uint8)]

    class Frame:
        def __init__(self, m):
            self.mover_ids = m
    scene.frames = [Frame(m) for m in ids]
    out = scene.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "fab_mover_tracks.json"))
    assert disk == json.loads(json.dumps(out)) and disk["num_frames"] == P and disk["period"] == 0.1
    for f in range(P):
        counts = np.bincount(ids[f], minlength=3)
        assert disk["frames"][f]["static_points"] == counts[0]
        assert [m["num_points"] for m in disk["frames"][f]["movers"]] == counts[1:].tolist()
        assert [m["mover"] for m in disk["frames"][f]["movers"]] == [1, 2]
    m1 = disk["frames"][1]["movers"][0]                      # t = 0.1: half way along the first mover's path
    assert np.allclose([m1["pose"]["x"], m1["pose"]["y"], m1["pose"]["yaw_deg"]], [2.3, 2.2, 60.0])
    assert np.allclose(m1["box7"], [2.3, 2.2, 0.85, 0.5, 0.5, 1.7, np.deg2rad(60.0)])
    assert np.allclose(m1["pose"]["matrix12"], MoverTrack(KEY["objects"][0]["path"]).poses12([0.1])[0])
    assert disk["objects"][0]["instance"] == 1001 and disk["objects"][1]["semantic"] == 12
