"""CPU: the host side of the scene flow under movers (lrc_flow_rays, lrc_flow_status, the checks that need no device,
lidarcast.flow, the simulator key, the scene-flow file).  The two host functions are compared bit for bit with the numpy
restatement of the header's text (tests/flow_restate.py); the restatement over the CPU oracle is compared with the oracle on the
BAKED mesh of the next frame -- the room with the pedestrian's vertices moved in float64 to its next pose and appended.

Measured with the oracle on the inputs below (widths 100 / 128, max_range 3.0 / 20.0, frames 0 -> 1 and 1 -> 2): no row's status
disagrees with the baked mesh; at most one row per case lies in the band (L - 2 margin, L - margin / 2) in which the two may
differ; outside the band the baked range of a visible row's own surface differs from L by at most 3.5e-5 m against a margin of at
least 2.44e-4 m."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flow_restate as fl
import mover_restate as mv
from conftest import REPO
from helpers import assert_bit_equal, table_rays
from test_movers_host import KEY, oracle_cast, sim_with

COLUMNS = ("flow3", "rays6", "keep", "thr", "status")


def assert_same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.itemsize == 1:
        assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} entries differ"
    else:
        assert_bit_equal(a, b, what)


@pytest.fixture(scope="module")
def world():
    """The room, the pedestrian and their oracle casts: built once, left unchanged."""
    from lidarcast import synth
    room, ped = mv.room_mesh(), synth.make_pedestrian()
    return {"room": room, "ped": ped, "cs": oracle_cast(room), "cm": oracle_cast(ped), "cases": {}}


def case(world, width, max_range):
    """The mover scan of the three frames by the restatement over the oracle and the flow k -> k + 1 on top of it."""
    key = (width, max_range)
    if key not in world["cases"]:
        k, dirs, poses = mv.scan_inputs(width)
        rays, cen = table_rays(dirs, poses)
        N = len(dirs)
        mp = np.stack([mv.pose12(*mv.walker_state(f)) for f in range(3)]).reshape(3, 1, 12)
        rec, _ = mv.scan(world["cs"], [world["cm"]], rays, np.repeat(cen, N, axis=0), mp, N, max_range)
        nxt, nmp, has = fl.pair_next(poses, mp)
        flow3, status, d = fl.scan(world["cs"], [world["cm"]], rec["t"], rec["point3"], rec["mover"], mp, nmp, nxt, has, N, max_range)
        world["cases"][key] = {"N": N, "rec": rec, "mp": mp, "nmp": nmp, "nxt": nxt, "has": has, "flow3": flow3, "status": status,
                               "d": d, "poses": poses}
    return world["cases"][key]


# ---- the two host functions against the restatement ---------------------------------------------------------------------------

def general_pose(rng, scale=4.0):
    a, b, c = rng.uniform(-3.1, 3.1, 3)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1.0, 0], [-np.sin(b), 0, np.cos(b)]])
    rx = np.array([[1.0, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    m = np.zeros((3, 4))
    m[:, :3], m[:, 3] = rz @ ry @ rx, rng.uniform(-scale, scale, 3)
    return mv.pose12_of(m)


def sensor_pose(rng):
    m = np.eye(4)
    m[:3, :4] = general_pose(rng, 3.0).astype(np.float64).reshape(3, 4)
    m[:3, 3] += rng.uniform(-1e-4, 1e-4, 3)              # a translation that is no float32
    return m


@pytest.mark.parametrize("M", [1, 3, 255])
def test_flow_rays_equal_the_restatement_on_random_columns(M):
    from lidarcast import flow
    rng = np.random.default_rng(100 + M)
    P, N = 4, 157
    n = P * N
    t = rng.uniform(0.2, 9.0, n).astype(np.float32)
    t[rng.random(n) < 0.15] = np.inf
    x = rng.uniform(-6.0, 6.0, (n, 3)).astype(np.float32)
    w = np.where(rng.random(n) < 0.5, 0, rng.integers(1, M + 1, n)).astype(np.uint8)
    w[::17] = M                                           # the last mover's row
    A = np.stack([[general_pose(rng) for _ in range(M)] for _ in range(P)])
    B = np.stack([[general_pose(rng) for _ in range(M)] for _ in range(P)])
    B[1] = A[1]                                           # a frame in which every mover stands still
    nxt = np.stack([sensor_pose(rng) for _ in range(P)])
    has = np.array([1, 1, 0, 1], np.uint8)
    for min_range in (0.0, 2.5):
        want = fl.rays(t, x, w, A, B, nxt, has, N, 7.0, min_range)
        got = flow.rays(t, x, w, A, B, nxt, has, 7.0, min_range)
        for c in COLUMNS:
            assert_same(got[c], want[c], f"M = {M}, min_range {min_range}: {c}")
        counts = np.bincount(want["status"], minlength=4)
        assert (counts[[0, 1, 3]] > 0).all() and counts[2] == 0, counts      # none, to be cast, out of range; 2 is step 5's
    still = np.repeat(np.arange(P), N) == 1
    assert not want["flow3"][still].view(np.uint32).any()
    assert (want["flow3"][(w > 0) & (t < np.inf) & ~still & (np.repeat(has, N) != 0)] != 0).any(axis=1).all()
    assert not want["flow3"][w == 0].view(np.uint32).any()
    none = fl.rays(t, x, w, A, B, nxt, None, N, 7.0)      # a NULL has_next: all ones
    got = flow.rays(t, x, w, A, B, nxt, None, 7.0)
    assert (none["status"][t < np.inf] != 0).all()
    for c in COLUMNS:
        assert_same(got[c], none[c], f"no has_next: {c}")


def test_flow_rays_on_crafted_columns():
    """Byte-equal pose pairs (also a pair that differs only in the sign of a zero: not equal), w = 0 / 1 / 255, rows without a
    return, has_next = 0, L below and above 1, a mover id above M."""
    from lidarcast import flow
    rng = np.random.default_rng(7)
    M, P, N = 255, 2, 8
    A = np.stack([[general_pose(rng) for _ in range(M)] for _ in range(P)])
    B = A.copy()
    B[0, 254] = general_pose(rng)                                   # mover 255 moves in frame 0
    B[0, 0] = mv.pose12(1.0, 2.0, 0.0, 0.0)
    A[0, 0] = B[0, 0].copy()
    A[0, 0, 2] = np.float32(-0.0)                                   # R[0][2]: -0 against +0 -- other bytes, the same rotation
    x = np.zeros((P * N, 3), np.float32)
    x[:] = [0.3, 0.2, 0.1]
    x[4] = [5.0, 4.0, 3.0]                                          # L above 1
    t = np.full(P * N, 1.0, np.float32)
    w = np.array([0, 1, 255, 2, 0, 255, 0, 1] * 2, np.uint8)
    t[6] = np.inf                                                   # no return
    nxt = np.stack([np.eye(4), np.eye(4)])
    nxt[:, :3, 3] = [0.1, 0.1, 0.1]
    has = np.array([1, 0], np.uint8)
    want = fl.rays(t, x, w, A, B, nxt, has, N, 10.0)
    got = flow.rays(t, x, w, A, B, nxt, has, 10.0)
    for c in COLUMNS:
        assert_same(got[c], want[c], c)
    f = got["flow3"]
    assert not f[0].view(np.uint32).any() and not f[3].view(np.uint32).any() and not f[4].view(np.uint32).any()
    assert (f[2] != 0).any() and (f[5] != 0).any()                  # w = 255 moved
    assert np.abs(f[1]).max() < 1e-6 and got["status"][1] == 1      # the -0 pair: through the arithmetic, (almost) no flow
    assert got["status"][:8].tolist() == [1, 1, 1, 1, 1, 1, 0, 1] and not got["status"][8:].any()
    assert not f[8:].view(np.uint32).any() and not got["keep"][8:].any()
    L = np.linalg.norm(x[[0, 4]].astype(np.float64) - 0.1, axis=1)
    assert L[0] < 1 < L[1]
    assert got["thr"][0] == np.float32(np.float32(L[0]) - np.float32(2.0 ** -12))
    assert got["thr"][4] == np.float32(np.float32(L[1]) - np.float32(2.0 ** -12) * np.float32(L[1]))
    few = flow.rays(t, x, w, A[:, :1], B[:, :1], nxt, has, 10.0)    # M = 1: the ids 2 and 255 name no mover -- read as the room
    assert not few["flow3"][[2, 3, 5]].view(np.uint32).any() and few["status"][:8].tolist() == got["status"][:8].tolist()
    assert_same(few["flow3"], fl.rays(t, x, w, A[:, :1], B[:, :1], nxt, has, N, 10.0)["flow3"], "ids above M")
    far = flow.rays(t, x, w, A, B, nxt, has, 1.0)                   # max_range 1: row 4 out of range, and not cast
    assert far["status"][4] == 3 and far["keep"][4] == 0 and not far["rays6"][4].any()


def test_flow_status_equals_the_restatement_with_ranges_exactly_at_thr():
    from lidarcast import flow
    rng = np.random.default_rng(11)
    n, M = 600, 4
    thr = rng.uniform(0.3, 8.0, n).astype(np.float32)
    st = rng.choice([0, 1, 1, 1, 3], n).astype(np.uint8)
    ts = (thr * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    tm = (thr[None] * rng.uniform(0.5, 2.5, (M, n))).astype(np.float32)
    ts[rng.random(n) < 0.3] = np.inf
    tm[rng.random((M, n)) < 0.5] = np.inf
    exact = np.arange(n) % 5 == 0                                   # the nearest range IS thr: not below it, visible
    ts[exact] = thr[exact]
    tm[:, exact] = np.inf
    below = np.arange(n) % 5 == 1                                   # one ulp below, by the last mover alone
    ts[below] = np.inf
    tm[:, below] = np.inf
    tm[M - 1, below] = np.nextafter(thr[below], np.float32(0))
    want, _ = fl.judge(ts, tm, thr, st)
    got = flow.status(ts, tm, thr, st)
    assert got.tolist() == want.tolist()
    assert (got[exact & (st == 1)] == 1).all() and (got[below & (st == 1)] == 2).all()
    assert (got[st != 1] == st[st != 1]).all() and (np.bincount(got, minlength=4) > 0).all()
    assert flow.status(ts, None, thr, st).tolist() == fl.judge(ts, None, thr, st)[0].tolist()      # no movers


# ---- the restatement against the baked mesh ------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_range", [3.0, 20.0])
@pytest.mark.parametrize("width", [100, 128])
def test_restatement_over_the_oracle_equals_the_baked_mesh(world, width, max_range):
    from lidarcast import flow
    from oracle.c_oracle import OracleMesh
    c = case(world, width, max_range)
    N, d, rec = c["N"], c["d"], c["rec"]
    got = flow.rays(rec["t"], rec["point3"], rec["mover"], c["mp"], c["nmp"], c["nxt"], c["has"], max_range)
    for col in COLUMNS:                                              # the host function on the scan's own columns
        assert_same(got[col], d[col], f"width {width}, max_range {max_range}: {col}")
    assert flow.status(d["t_static"], d["t_movers"], d["thr"], d["status"]).tolist() == c["status"].tolist()
    counts = []
    for p in range(2):
        sl = slice(p * N, (p + 1) * N)
        v, tri, _ = mv.baked(world["room"], world["ped"], mv.walker_state(p + 1))
        keep = d["keep"][sl].astype(bool)
        tb = np.full(N, np.inf, np.float32)
        tb[keep] = OracleMesh(v, tri).build().cast(np.ascontiguousarray(d["rays6"][sl][keep]))[0]
        L, thr, st = d["L"][sl], d["thr"][sl], c["status"][sl]
        margin = fl.MARGIN * np.maximum(L, np.float32(1))
        in_band = lambda t: (t > L - 2 * margin) & (t < L - margin / 2)
        band = keep & (in_band(tb) | in_band(d["t_min"][sl]))
        baked = np.where(keep, np.where(tb < thr, fl.OCCLUDED, fl.VISIBLE), st)
        own = keep & ~band & (baked == fl.VISIBLE) & np.isfinite(tb)
        worst = float(np.abs(tb[own].astype(np.float64) - L[own]).max())
        rows = int((rec["t"][sl] < np.inf).sum())
        counts.append(np.bincount(st[rec["keep"][sl]], minlength=4).tolist())
        print(f"\n[flow] width {width}, max_range {max_range}, frame {p} -> {p + 1}: status {counts[-1]}, {int(band.sum())} of {rows} "
              f"rows in the ambiguous band, {int((baked != st)[~band].sum())} disagree with the baked mesh, max |t_baked - L| of a "
              f"visible row {worst:.3e} m, least margin {float(margin[keep].min()):.3e} m")
        assert band.sum() * 100 < rows and band.sum() <= 1
        assert (baked == st)[~band].all()
        # the row's own surface is met within half the least margin of L, on either side: the margin has a factor 2 to spare
        assert margin[keep].min() >= 2.0 ** -12 and worst < 2.0 ** -13
    last = slice(2 * N, 3 * N)
    assert not c["status"][last].any() and not c["flow3"][last].view(np.uint32).any()          # the last frame has no next
    room = rec["mover"] == 0
    assert not c["flow3"][room].view(np.uint32).any()
    if (width, max_range) == (100, 3.0):
        assert counts == [[0, 312, 144, 44], [0, 379, 50, 134]]
        for p, rows, own_hidden in ((0, 18, 9), (1, 204, None)):
            sl = slice(p * N, (p + 1) * N)
            mover = rec["mover"][sl] == 1
            assert mover.sum() == rows and (c["flow3"][sl][mover] != 0).any(axis=1).all()
            if own_hidden is not None:          # hidden by the pedestrian itself: its own cast is the one below thr
                assert int((mover & (d["t_movers"][0][sl] < d["thr"][sl]) & (c["status"][sl] == fl.OCCLUDED)).sum()) == own_hidden


def test_sensor_flow():
    from lidarcast import flow
    rng = np.random.default_rng(3)
    T0, T1 = sensor_pose(rng), sensor_pose(rng)
    x = rng.uniform(-3, 3, (50, 3))
    f = rng.uniform(-0.5, 0.5, (50, 3))
    got = flow.sensor_flow(x.astype(np.float32), f.astype(np.float32), T0, T1)
    h = lambda T, p: (np.linalg.inv(T) @ np.concatenate([p, np.ones((len(p), 1))], axis=1).T).T[:, :3]
    x32, f32 = x.astype(np.float32).astype(np.float64), f.astype(np.float32).astype(np.float64)
    assert got.dtype == np.float64 and np.allclose(got, h(T1, x32 + f32) - h(T0, x32), atol=1e-5)
    assert np.allclose(flow.sensor_flow(x, np.zeros_like(x), T0, T0), 0.0, atol=1e-12)       # nothing moves: no flow
    assert (flow.NONE, flow.VISIBLE, flow.OCCLUDED, flow.OUT_OF_RANGE) == (0, 1, 2, 3)
    nxt, nmp, has = flow.pair_next(np.stack([T0, T1, T0]), np.arange(3 * 2 * 12, dtype=np.float32).reshape(3, 2, 12))
    assert has.tolist() == [1, 1, 0] and np.array_equal(nxt, np.stack([T1, T0, T0]))
    assert np.array_equal(nmp[:, 0, 0], [24.0, 48.0, 48.0])


# ---- symbols, layouts, refusals ------------------------------------------------------------------------------------------------

NEW = ("lrc_scan_flow_dev", "lrc_scan_flow_compact", "lrc_flow_rays", "lrc_flow_status")


def test_new_symbols_load():
    from lidarcast import _capi
    import __graft_entry__ as entry
    lib = _capi.load()
    header = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(rf"\bint {name}\(", header), name
    assert "lrc_flow.hip" in entry.SOURCES
    for name, value in (("NONE", 0), ("VISIBLE", 1), ("OCCLUDED", 2), ("OUT_OF_RANGE", 3)):
        assert re.search(rf"#define LRC_FLOW_{name} {value}\b", header)


def test_signatures_match_the_header():
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
    hits, fr = _capi.LrcHits(), _capi.LrcFrames()
    assert lib.lrc_scan_flow_dev(None, None, C.byref(hits), None, 0, 0, None, None, None, None, 1.0, None, None, None) == E
    assert b"NULL scene" in lib.lrc_last_error()
    assert lib.lrc_scan_flow_compact(None, None, None, 0, None, None, None, None, None, 1.0, C.byref(fr), None, None, None, 0, None) == E
    assert b"NULL scene" in lib.lrc_last_error()
    n = 4
    t, x, w = np.ones(n, np.float32), np.ones((n, 3), np.float32), np.zeros(n, np.uint8)
    p12 = np.tile(mv.pose12(0, 0, 0, 0), (1, 1, 1))
    nxt = np.eye(4).reshape(1, 16).copy()
    f3, r6, keep, thr, st = np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data
    outs = (p(f3), p(r6), p(keep), p(thr), p(st))
    assert lib.lrc_flow_rays(p(t), p(x), p(w), 1, n, 1, p(p12), p(p12), p(nxt), None, 9.0, 0.0, *outs) == 0 and (st == 1).all()
    assert lib.lrc_flow_rays(p(t), p(x), None, 1, n, 0, None, None, p(nxt), None, 9.0, 0.0, *outs) == 0          # no movers
    assert lib.lrc_flow_rays(p(t), p(x), p(w), 1, n, 256, p(p12), p(p12), p(nxt), None, 9.0, 0.0, *outs) == E and b"255" in lib.lrc_last_error()
    assert lib.lrc_flow_rays(p(t), p(x), None, 1, n, 1, p(p12), p(p12), p(nxt), None, 9.0, 0.0, *outs) == E
    assert lib.lrc_flow_rays(p(t), p(x), p(w), 1, n, 1, p(p12), None, p(nxt), None, 9.0, 0.0, *outs) == E
    assert lib.lrc_flow_rays(p(t), p(x), p(w), 1, n, 1, p(p12), p(p12), None, None, 9.0, 0.0, *outs) == E
    assert lib.lrc_flow_rays(p(t), p(x), p(w), 1, n, 1, p(p12), p(p12), p(nxt), None, 9.0, 0.0, None, *outs[1:]) == E
    assert lib.lrc_flow_rays(None, None, None, 0, 0, 0, None, None, None, None, 9.0, 0.0, *([None] * 5)) == 0
    assert lib.lrc_flow_status(n, 1, p(t), p(t), p(thr), p(st), p(keep)) == 0
    assert lib.lrc_flow_status(n, 256, p(t), p(t), p(thr), p(st), p(keep)) == E and b"255" in lib.lrc_last_error()
    assert lib.lrc_flow_status(n, 1, p(t), None, p(thr), p(st), p(keep)) == E
    assert lib.lrc_flow_status(n, 0, p(t), None, p(thr), p(st), p(keep)) == 0
    assert lib.lrc_flow_status(n, 0, None, None, p(thr), p(st), p(keep)) == E
    assert lib.lrc_flow_status(0, 0, None, None, None, None, None) == 0


# ---- the simulator key and the scene-flow file -----------------------------------------------------------------------------------

class _Engine:
    """stands for the GPU engine: records which scan the simulator asked for and returns fabricated frames"""

    def __init__(self):
        self.ctx, self.calls = object(), []

    def _frames(self, name, poses, mover_poses, want):
        self.calls.append(name)
        P = len(poses)
        counts = np.array([3, 0, 2, 4][:P], np.int64)
        K = int(counts.sum())
        rng = np.random.default_rng(1)
        fr = {"counts": counts, "total": K, "point3": rng.uniform(0, 3, (K, 3)).astype(np.float32),
              "sem": np.full(K, 13, np.uint16), "ins": np.full(K, 1001, np.uint16), "incident_deg": np.zeros(K),
              "range_origin": np.ones(K, np.float32), "mover": (np.arange(K) % 3).astype(np.uint8)}
        for k in ("range_origin_mean", "range_origin_std", "incident_mean", "incident_std"):
            fr[k] = np.zeros(P)
        if name == "flow":
            fr["flow"] = rng.uniform(-1, 1, (K, 3)).astype(np.float32)
            fr["flow_status"] = (np.arange(K) % 4).astype(np.uint8)
        return fr

    def scan_mover_frames(self, k, poses, mesh, mset, mover_poses, want):
        return self._frames("movers", poses, mover_poses, want)

    def scan_flow_frames(self, k, poses, mesh, mset, mover_poses, want):
        return self._frames("flow", poses, mover_poses, want)


def _run(config, monkeypatch):
    import s3dis_simulator
    import lidarcast.movers as lm
    from lidar import Indoor8LineLidarIntrinsics
    from trajectory import Waypoint

    class Scene:
        scene_name, room_mesh = "fab", None

        class room_bounds:
            @staticmethod
            def get_volume():
                return 1.0

    class Set:
        def __init__(self, ctx, meshes):
            self.n = len(meshes)

        def close(self):
            pass
    monkeypatch.setattr(lm, "MoverSet", Set)
    sim = sim_with(config)
    sim.scene, sim.raycast_engine, sim.bug_compatible = Scene(), _Engine(), True
    sim.lidar_config = Indoor8LineLidarIntrinsics(vertical_res=4, horizontal_res=16, max_range=20.0,
                                                  vertical_degrees=[20.0, 5.0, -10.0, -25.0])
    wps = [Waypoint(1.0 + 0.5 * i, 1.0, 1.0, 0.0) for i in range(4)]
    return sim, sim.run_simulation(wps, process_group=s3dis_simulator._NO_GROUP)


def test_simulator_flow_entry_on_a_fabricated_engine(monkeypatch, tmp_path):
    assert sim_with({"movers": KEY})._mover_plan()["flow"] is False
    assert sim_with({"movers": dict(KEY, flow=True)})._mover_plan()["flow"] is True
    with pytest.raises(ValueError, match="movers.flow must be true or false"):
        sim_with({"movers": dict(KEY, flow="yes")})._mover_plan()
    with pytest.raises(ValueError, match="unknown entries under the movers key"):
        sim_with({"movers": dict(KEY, flow=True, speed=1.0)})._mover_plan()
    for other, cfg in (("motion", {"speed": 1.0}), ("noise", {"seed": 1}), ("beam", {"divergence_mrad": 3.0}),
                       ("materials", {"classes": {}})):
        with pytest.raises(ValueError, match=f"movers key cannot be combined with the {other} key"):
            sim_with({"movers": dict(KEY, flow=True), other: cfg})._mover_plan()
    sim, plain = _run({"movers": KEY}, monkeypatch)
    assert sim.raycast_engine.calls == ["movers"]
    assert all(hasattr(f, "mover_ids") and not hasattr(f, "flow") and not hasattr(f, "flow_status") for f in plain.frames)
    with pytest.raises(ValueError, match="flow: true"):
        plain.export_scene_flow(tmp_path)
    sim, scene = _run({"movers": dict(KEY, flow=True)}, monkeypatch)
    assert sim.raycast_engine.calls == ["flow"] and scene.get_total_frames() == 4
    for f, count in zip(scene.frames, (3, 0, 2, 4)):
        assert len(f.points) == len(f.flow) == len(f.flow_status) == len(f.mover_ids) == count
        assert f.flow.dtype == np.float32 and f.flow.shape == (count, 3) and f.flow_status.dtype == np.uint8
    out = scene.export_scene_flow(tmp_path)
    disk = np.load(tmp_path / "fab_scene_flow.npz")
    assert sorted(disk.files) == sorted(out) == ["flow", "frame_offsets", "mover_ids", "mover_poses12", "points", "sensor_poses",
                                                   "status", "times"]
    assert disk["frame_offsets"].tolist() == [0, 3, 3, 5, 9] and disk["sensor_poses"].shape == (4, 4, 4)
    assert disk["mover_poses12"].shape == (4, 2, 12) and np.allclose(disk["times"], [0.0, 0.1, 0.2, 0.3])
    assert np.allclose(disk["sensor_poses"][2, :3, 3], [2.0, 1.0, 1.0])
    for key, col in (("points", "points"), ("flow", "flow"), ("status", "flow_status"), ("mover_ids", "mover_ids")):
        want = np.concatenate([getattr(f, col) for f in scene.frames])
        assert disk[key].dtype == want.dtype and np.array_equal(disk[key], want), key


def test_scene_flow_file_from_a_fabricated_frame_list(tmp_path):
    from containers import S3DISSimScene
    scene = S3DISSimScene("fab")
    with pytest.raises(ValueError, match="movers key"):
        scene.export_scene_flow(tmp_path)
    P = 3
    scene.mover_tracks = {"period": 0.1, "objects": [], "times": np.arange(P) * 0.1, "states": np.zeros((P, 1, 4)),
                          "poses12": np.tile(mv.pose12(0, 0, 0, 0), (P, 1, 1)), "sensor_poses": np.tile(np.eye(4), (P, 1, 1))}

    class Frame:
        def __init__(self, k, with_flow=True):
            self.points = np.full((k, 3), 1.5, np.float32)
            self.mover_ids = np.arange(k, dtype=np.uint8) % 2
            if with_flow:
                self.flow = np.full((k, 3), 0.25, np.float32) * self.mover_ids[:, None]
                self.flow_status = np.full(k, 1, np.uint8)
    scene.frames = [Frame(4), Frame(0), Frame(2)]
    scene.frames[2].flow_status[:] = 0
    out = scene.export_scene_flow(tmp_path / "deep" / "er")
    disk = np.load(tmp_path / "deep" / "er" / "fab_scene_flow.npz")
    assert disk["frame_offsets"].tolist() == [0, 4, 4, 6] and disk["points"].shape == (6, 3) and disk["flow"].dtype == np.float32
    assert disk["status"].tolist() == [1, 1, 1, 1, 0, 0] and disk["mover_ids"].tolist() == [0, 1, 0, 1, 0, 1]
    assert all(np.array_equal(disk[k], out[k]) for k in out)
    scene.frames[1] = Frame(3, with_flow=False)
    with pytest.raises(ValueError, match="frame 1 carries no flow"):
        scene.export_scene_flow(tmp_path)
    scene.frames[1] = Frame(3)
    scene.frames[1].flow = scene.frames[1].flow[:2]
    with pytest.raises(ValueError, match="differ in length"):
        scene.export_scene_flow(tmp_path)
