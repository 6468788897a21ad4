"""-m gpu: scene flow under movers (lrc_scan_flow_dev / lrc_scan_flow_compact: the ray kernel, the explicit-ray launch on the room
and per mover at its NEXT pose, the merge kernel), on both node routes for the room and for the movers.

The comparator is the numpy restatement of the header's steps (tests/flow_restate.py) over the EXISTING explicit-ray cast
(Scene.cast, no centre, no filter, which never culls), applied to the records the mover scan left on the device (their own
parity is tests/test_movers_gpu.py's).  flow3 and status must agree bit for bit.  Each case asserts on the restatement that it
exercises what it is for.  Three frames; frame k is paired with k + 1 and the last has no next, unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import flow_restate as fl
import mover_restate as mv
from helpers import assert_bit_equal
from test_movers_gpu import ROUTES, _sim, engine, inputs, walker_poses, world  # noqa: F401  (engine, world: fixtures)

pytestmark = pytest.mark.gpu

FRAMES = ("point3", "sem", "ins", "index")


def flow_dev(scene, mset, poses, dirs, mp, nxt, nmp, has, max_range, with_status=True, stream=None):
    """The mover scan and the flow on device tensors: t, point3, mover of the records, flow3 and status (None without)."""
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3"))
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    flow = torch.full((P * N, 3), 7.0, dtype=torch.float32, device="cuda")
    status = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda") if with_status else None
    pt, dt, mt = dev(np.asarray(poses).reshape(P, 16), np.float64), dev(dirs, np.float64), dev(mp, np.float32)
    nt, nmt, ht = dev(np.asarray(nxt).reshape(P, 16), np.float64), dev(nmp, np.float32), dev(has, np.uint8)

    def run(st):
        scene.scan_movers_dev(pt, dt, hits, max_range, mset, mt, mover_t=who, stream=st)
        scene.scan_flow_dev(hits, who if mset is not None else None, P, N, max_range, mset, mt, nmt, nt, flow, status_t=status,
                            has_next_t=ht, stream=st)
    if stream is None:
        run(0)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            run(stream.cuda_stream)
    torch.cuda.synchronize()
    return {"t": hits["t"].cpu().numpy(), "point3": hits["point3"].cpu().numpy(), "mover": who.cpu().numpy(),
            "flow3": flow.cpu().numpy(), "status": None if status is None else status.cpu().numpy()}


def assert_same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), f"{what}: the bytes differ"


def restated(world, got, casts, mp, nxt, nmp, has, N, max_range, min_range=0.0):
    mover = got["mover"] if casts else None
    return fl.scan(world.static, casts, got["t"], got["point3"], mover, mp if casts else None, nmp if casts else None, nxt, has, N,
                   max_range, min_range)


def assert_flow(got, flow3, status, what):
    assert_bit_equal(got["flow3"], flow3, f"{what}: flow3")
    ne = got["status"] != status
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} status bytes differ; first at {np.argwhere(ne)[0]}"


def counts_per_frame(got, status, N):
    kept = got["t"] < np.inf
    return [np.bincount(status[p * N:(p + 1) * N][kept[p * N:(p + 1) * N]], minlength=4).tolist() for p in range(len(status) // N)]


def hidden_by(got, d, status, N):
    """{(row's owner w, occluder): rows}: occluder 0 the room, m + 1 mover m; a row hidden by several counts for each"""
    out = {}
    occ = status == fl.OCCLUDED
    below = [d["t_static"] < d["thr"]] + [tm < d["thr"] for tm in d["t_movers"]]
    for w in range(len(below)):
        for k, b in enumerate(below):
            out[(w, k)] = int((occ & (got["mover"] == w) & b).sum())
    return out


# ---- 1: the room with one pedestrian --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_range", [3.0, None])
@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_room_with_one_pedestrian(world, route, width, max_range):
    k, dirs, poses, rays, cen = inputs(width)
    reach = k.max_range if max_range is None else max_range
    mp = walker_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    N = len(dirs)
    got = flow_dev(world.scenes[route], world.one[route], poses, dirs, mp, nxt, nmp, has, reach)
    flow3, status, d = restated(world, got, world.casts[:1], mp, nxt, nmp, has, N, reach)
    counts, by = counts_per_frame(got, status, N), hidden_by(got, d, status, N)
    print(f"\n[flow] one pedestrian, width {width}, max_range {reach}, {route}: status per frame {counts}, hidden (owner, by) {by}")
    assert (N % 64 == 0) == (width == 128)
    assert by[(0, 0)] > 0 and by[(0, 1)] > 0 and by[(1, 1)] > 0            # the room by itself and by the mover, the mover by itself
    assert (np.array(counts[:2])[:, 1:3] > 0).all() and counts[2][1:] == [0, 0, 0]
    assert (np.array(counts[:2])[:, 3] > 0).all() == (max_range == 3.0)
    moved = (got["mover"] == 1) & (np.repeat(has, N) != 0)
    assert moved.sum() > 200 and (flow3[moved] != 0).any(axis=1).all()
    assert not flow3[got["mover"] == 0].view(np.uint32).any()              # room rows: +0 in every component
    if width == 100 and max_range == 3.0:
        assert counts == [[0, 312, 144, 44], [0, 379, 50, 134], [499, 0, 0, 0]]
    assert_flow(got, flow3, status, f"one pedestrian, width {width}, {route} nodes")


# ---- 2: three movers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_three_movers(world, route, width):
    k, dirs, poses, rays, cen = inputs(width)
    mp = fl.three_mover_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    N = len(dirs)
    got = flow_dev(world.scenes[route], world.sets[route], poses, dirs, mp, nxt, nmp, has, 3.0)
    flow3, status, d = restated(world, got, world.casts, mp, nxt, nmp, has, N, 3.0)
    counts, by = counts_per_frame(got, status, N), hidden_by(got, d, status, N)
    print(f"\n[flow] three movers, width {width}, {route}: status per frame {counts}, hidden (owner, by) {by}")
    assert all(by[(0, k)] > 0 for k in range(4))                           # room rows hidden by the room and by each mover
    assert all(by[(m, m)] > 0 for m in (2, 3))                             # mover rows hidden by their own mover
    assert by[(1, 2)] > 0 and by[(3, 2)] > 0 and by[(3, 1)] > 0            # ... and by ANOTHER mover
    if width == 100:
        assert counts == [[0, 231, 253, 44], [0, 109, 382, 95], [520, 0, 0, 0]]
        assert by[(1, 2)] == 204 and by[(3, 2)] == 54
    assert_flow(got, flow3, status, f"three movers, width {width}, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_a_mover_hidden_by_the_room(world, route):
    """The pedestrian's next pose lies OUTSIDE the room behind the wall x = 0: every one of its rows flows there, and the wall
    stands in the line of sight."""
    k, dirs, poses, rays, cen = inputs(128)
    mp = walker_poses()
    nxt, _, has = fl.pair_next(poses, mp)
    nmp = np.tile(mv.pose12(-0.6, 1.0, 0.0, 0.2), (3, 1, 1))
    N = len(dirs)
    got = flow_dev(world.scenes[route], world.one[route], poses, dirs, mp, nxt, nmp, has, k.max_range)
    flow3, status, d = restated(world, got, world.casts[:1], mp, nxt, nmp, has, N, k.max_range)
    by = hidden_by(got, d, status, N)
    alone = int(((status == fl.OCCLUDED) & (got["mover"] == 1) & (d["t_static"] < d["thr"]) & ~(d["t_movers"][0] < d["thr"])).sum())
    print(f"\n[flow] behind the wall, {route}: hidden (owner, by) {by}, {alone} mover rows hidden by the room alone")
    assert by[(1, 0)] > 200 and alone > 0
    assert_flow(got, flow3, status, f"behind the wall, {route} nodes")


# ---- 3: properties -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["one", "three"])
@pytest.mark.parametrize("route", ROUTES)
def test_identity_pairing(world, route, layout):
    """Next sensor pose = own pose and B = A: every kept row is visible with +0 flow -- the margin clears every row's own
    surface, grazing ones included."""
    k, dirs, poses, rays, cen = inputs(100)
    mset, mp = (world.one[route], walker_poses()) if layout == "one" else (world.sets[route], fl.three_mover_poses())
    got = flow_dev(world.scenes[route], mset, poses, dirs, mp, poses, mp, None, 3.0)
    kept = got["t"] < np.inf
    assert kept.reshape(3, -1).sum(1).tolist() == ([500, 563, 499] if layout == "one" else [528, 586, 520])
    assert (got["status"][kept] == fl.VISIBLE).all() and not got["status"][~kept].any()
    assert not got["flow3"].view(np.uint32).any()


@pytest.mark.parametrize("route", ROUTES)
def test_null_set(world, route):
    k, dirs, poses, rays, cen = inputs(100)
    nxt, _, has = fl.pair_next(poses, walker_poses())
    N = len(dirs)
    got = flow_dev(world.scenes[route], None, poses, dirs, None, nxt, None, has, 3.0)
    flow3, status, d = restated(world, got, [], None, nxt, None, has, N, 3.0)
    counts = counts_per_frame(got, status, N)
    print(f"\n[flow] NULL set, {route}: status per frame {counts}")
    assert (np.array(counts[:2])[:, 1:] > 0).all() and not got["flow3"].view(np.uint32).any() and not got["mover"].any()
    assert_flow(got, flow3, status, f"NULL set, {route} nodes")


def test_flow_alone_gives_the_same_flow_bytes(world):
    k, dirs, poses, rays, cen = inputs(100)
    mp = fl.three_mover_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    scene, mset = world.scenes["quantised"], world.sets["quantised"]
    both = flow_dev(scene, mset, poses, dirs, mp, nxt, nmp, has, 3.0)
    alone = flow_dev(scene, mset, poses, dirs, mp, nxt, nmp, has, 3.0, with_status=False)
    assert alone["status"] is None and (both["flow3"] != 0).any()
    assert_bit_equal(alone["flow3"], both["flow3"], "d_status == NULL: flow3")


@pytest.mark.parametrize("width", [100, 128])
def test_six_frames_equal_two_then_four(world, width):
    """"Next" is given per frame: any pairing, any split.  Here frames flow to the one before them as well as after."""
    k, dirs, poses, rays, cen = inputs(width)
    trio = fl.three_mover_poses()
    poses6, mp6 = np.concatenate([poses, poses[::-1]]), np.concatenate([trio, trio[::-1]])
    nxt6, nmp6 = np.roll(poses6, -1, axis=0), np.roll(mp6, -1, axis=0)
    has6 = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    scene, mset = world.scenes["quantised"], world.sets["quantised"]
    whole = flow_dev(scene, mset, poses6, dirs, mp6, nxt6, nmp6, has6, 3.0)
    a = flow_dev(scene, mset, poses6[:2], dirs, mp6[:2], nxt6[:2], nmp6[:2], has6[:2], 3.0)
    b = flow_dev(scene, mset, poses6[2:], dirs, mp6[2:], nxt6[2:], nmp6[2:], has6[2:], 3.0)
    assert (np.bincount(whole["status"], minlength=4) > 0).all()
    assert_bit_equal(whole["flow3"], np.concatenate([a["flow3"], b["flow3"]]), f"2 + 4 frames, width {width}: flow3")
    assert whole["status"].tolist() == np.concatenate([a["status"], b["status"]]).tolist()


def test_non_default_stream(world):
    import torch
    k, dirs, poses, rays, cen = inputs(128)
    mp = fl.three_mover_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    scene, mset = world.scenes["quantised"], world.sets["quantised"]
    ref = flow_dev(scene, mset, poses, dirs, mp, nxt, nmp, has, 3.0)
    got = flow_dev(scene, mset, poses, dirs, mp, nxt, nmp, has, 3.0, stream=torch.cuda.Stream())
    assert_flow(got, ref["flow3"], ref["status"], "own stream")


@pytest.mark.parametrize("route", ROUTES)
def test_min_range_of_the_static_scene(world, route):
    """min_range 1.6 m on the room: a place nearer than that to the NEXT sensor pose is out of range, like a place too far."""
    k, dirs, poses, rays, cen = inputs(100)
    mp = walker_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    N = len(dirs)
    scene = world.scenes[route]
    try:
        scene.set_options(min_range=1.6)
        got = flow_dev(scene, world.one[route], poses, dirs, mp, nxt, nmp, has, 3.0)
    finally:
        scene.reset_options()
    flow3, status, d = restated(world, got, world.casts[:1], mp, nxt, nmp, has, N, 3.0, min_range=1.6)
    plain = fl.rays(got["t"], got["point3"], got["mover"], mp, nmp, nxt, has, N, 3.0)["status"]
    near = (status == fl.OUT_OF_RANGE) & (plain == fl.VISIBLE)
    print(f"\n[flow] min_range, {route}: {int(near.sum())} rows too near to the next pose, status {np.bincount(status, minlength=4).tolist()}")
    assert near.sum() > 20 and (np.bincount(status, minlength=4) > 0).all()
    assert_flow(got, flow3, status, f"min_range, {route} nodes")


# ---- 4: frames ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_compact_frames(world, route):
    k, dirs, poses, rays, cen = inputs(100)
    scene, mset, mp = world.scenes[route], world.sets[route], fl.three_mover_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    N = len(dirs)
    rec = flow_dev(scene, mset, poses, dirs, mp, nxt, nmp, has, 3.0)
    keep = rec["t"] < np.inf
    fr = scene.scan_flow_compact(poses, dirs, 3.0, mset, mp, nxt, nmp, has, want=FRAMES)
    plain = scene.scan_movers_compact(poses, dirs, 3.0, mset, mp, want=FRAMES)
    assert fr["counts"].tolist() == keep.reshape(3, N).sum(1).tolist() == plain["counts"].tolist() and 0 < fr["total"] < 3 * N
    for a in FRAMES + ("mover",):                                  # the mover scan's frames, unchanged
        assert_same_bytes(fr[a], plain[a], f"compact, {route}: {a}")
    assert_bit_equal(fr["flow"], rec["flow3"][keep], f"compact, {route}: flow")
    assert fr["flow_status"].dtype == np.uint8 and fr["flow_status"].tolist() == rec["status"][keep].tolist()
    assert (np.bincount(fr["flow_status"], minlength=4) > 0).all() and (fr["flow"] != 0).any()
    small = scene.scan_flow_compact(poses, dirs, 3.0, mset, mp, nxt, nmp, has, want=("point3",))          # no index column asked for
    assert "index" not in small
    assert_bit_equal(small["flow"], fr["flow"])
    assert small["flow_status"].tolist() == fr["flow_status"].tolist() and small["mover"].tolist() == fr["mover"].tolist()
    bare = scene.scan_flow_compact(poses, dirs, 3.0, mset, mp, nxt, nmp, has, want=("sem",), with_status=False)   # no point column either
    assert "flow_status" not in bare
    assert_bit_equal(bare["flow"], fr["flow"])
    with pytest.raises(ValueError, match="capacity"):
        scene.scan_flow_compact(poses, dirs, 3.0, mset, mp, nxt, nmp, has, want=FRAMES, capacity=10)
    none = scene.scan_flow_compact(poses, dirs, 3.0, None, None, nxt, None, has, want=FRAMES)
    null = flow_dev(scene, None, poses, dirs, None, nxt, None, has, 3.0)
    assert not none["mover"].any() and not none["flow"].view(np.uint32).any()
    assert none["flow_status"].tolist() == null["status"][null["t"] < np.inf].tolist()


def test_engine_scan_flow_frames(engine, world):
    from lidarcast.movers import MoverSet
    k, dirs, poses, rays, cen = inputs(100)
    mp = fl.three_mover_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    mset = MoverSet(engine.ctx, world.meshes)
    try:
        fr = engine.scan_flow_frames(k, poses, world.room, mset, mp, want=FRAMES)
        ref = engine.scene_for(world.room).scan_flow_compact(poses, dirs, k.max_range, mset, mp, nxt, nmp, has, want=FRAMES)
    finally:
        mset.close()
    for a in FRAMES + ("mover", "flow", "flow_status"):
        assert_same_bytes(fr[a], ref[a], f"engine: {a}")
    last = int(fr["counts"][:2].sum())
    assert not fr["flow_status"][last:].any() and (fr["flow_status"][:last] != 0).all() and (fr["flow"][:last] != 0).any()
    with pytest.raises(ValueError, match="direction table"):
        engine.scan_flow_frames(object(), poses, world.room, None, None)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(engine, world):
    import torch
    import lidarcast
    from lidarcast import DeviceHits, _capi
    from lidarcast.movers import MoverSet
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    k, dirs, poses, rays, cen = inputs(100)
    P, N = 3, len(dirs)
    scene, mset, mp = world.scenes["quantised"], world.one["quantised"], walker_poses()
    nxt, nmp, has = fl.pair_next(poses, mp)
    nt = torch.from_numpy(nxt.reshape(P, 16).copy()).cuda()
    mt, nmt = torch.from_numpy(mp).cuda(), torch.from_numpy(nmp).cuda()
    hits = DeviceHits(P * N, "cuda", want=("t", "point3"))
    who = torch.zeros(P * N, dtype=torch.uint8, device="cuda")
    flow = torch.zeros((P * N, 3), dtype=torch.float32, device="cuda")
    status = torch.zeros(P * N, dtype=torch.uint8, device="cuda")

    def call(s=scene._h, h=None, rec=hits, w=who, a=mt, b=nmt, n=nt, f=flow):
        h = mset._h if h is None else h
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return lib.lrc_scan_flow_dev(s, h, C.byref(rec.struct), p(w), P, N, p(a), p(b), p(n), None, 20.0, p(f), p(status), None)
    assert call() == 0
    torch.cuda.synchronize()
    for kw, text in ((dict(f=None), b"flow3 is NULL"), (dict(w=None), b"mover column is NULL"), (dict(n=None), b"next_poses16 is NULL"),
                     (dict(a=None), b"mover_poses12"), (dict(b=None), b"next_mover_poses12"),
                     (dict(rec=DeviceHits(P * N, "cuda", want=("t",))), b"t and point3"),
                     (dict(rec=DeviceHits(P * N, "cuda", want=("point3", "prim"))), b"t and point3"), (dict(s=None), b"NULL scene")):
        assert call(**kw) == E and text in lib.lrc_last_error(), (kw.keys(), lib.lrc_last_error())
    # what the mover scan refuses: the static scene among its movers, another context, a range_noise option
    h = C.c_void_p()
    arr = (C.c_void_p * 1)(scene._h)
    assert lib.lrc_movers_create(engine.ctx._h, arr, 1, C.byref(h)) == 0
    try:
        assert call(h=h) == E and b"one of its own movers" in lib.lrc_last_error()
    finally:
        lib.lrc_movers_destroy(h)
    other = lidarcast.Context(0)
    try:
        foreign = MoverSet(other, world.meshes[:1])
        assert call(h=foreign._h) == E and b"different contexts" in lib.lrc_last_error()
        with pytest.raises(ValueError, match="another context"):
            scene.scan_flow_dev(hits, who, P, N, 20.0, foreign, mt, nmt, nt, flow)
        with pytest.raises(ValueError, match="another context"):
            scene.scan_flow_compact(poses, dirs, 20.0, foreign, mp, nxt, nmp, has)
        foreign.close()
    finally:
        other.close()
    noise = torch.zeros(P * N, dtype=torch.float32, device="cuda")
    try:
        scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_flow_dev(hits, who, P, N, 20.0, mset, mt, nmt, nt, flow)
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_flow_compact(poses, dirs, 20.0, mset, mp, nxt, nmp, has)
    finally:
        scene.reset_options()
    # both mover pose tables get the host checks
    for which in (0, 1):
        for edit, text in ((lambda a: a.__setitem__((1, 0, 3), np.nan), "not finite"),
                           (lambda a: a.__setitem__((2, 0, 0), a[2, 0, 0] + np.float32(2.0 ** -14)), "no rotation")):
            tables = [mp.copy(), nmp.copy()]
            edit(tables[which])
            with pytest.raises(ValueError, match=text):
                scene.scan_flow_compact(poses, dirs, 20.0, mset, tables[0], nxt, tables[1], has)
    with pytest.raises(ValueError, match=r"next_mover_poses must be \(P, M, 12\)"):
        scene.scan_flow_compact(poses, dirs, 20.0, mset, mp, nxt, nmp[:2], has)
    with pytest.raises(ValueError, match=r"next_poses must be \(P, 4, 4\)"):
        scene.scan_flow_compact(poses, dirs, 20.0, mset, mp, nxt[:2], nmp, has)
    with pytest.raises(ValueError, match="has_next must hold"):
        scene.scan_flow_compact(poses, dirs, 20.0, mset, mp, nxt, nmp, has[:2])
    with pytest.raises(ValueError, match="P \\* N records"):
        scene.scan_flow_dev(DeviceHits(P * N + 1, "cuda", want=("t", "point3")), who, P, N, 20.0, mset, mt, nmt, nt, flow)
    for kw, what in ((dict(status_t=torch.zeros(P * N, dtype=torch.int32, device="cuda")), "status_t must be torch.uint8"),
                     (dict(status_t=torch.zeros(3, dtype=torch.uint8, device="cuda")), "status_t must hold"),
                     (dict(has_next_t=torch.zeros(P, dtype=torch.uint8)), "has_next_t must lie on the device")):
        with pytest.raises(ValueError, match=what):
            scene.scan_flow_dev(hits, who, P, N, 20.0, mset, mt, nmt, nt, flow, **kw)
    with pytest.raises(ValueError, match="flow_t must be"):
        scene.scan_flow_dev(hits, who, P, N, 20.0, mset, mt, nmt, nt, flow[:5])
    with pytest.raises(ValueError, match="next_mover_poses_t must be torch.float32"):
        scene.scan_flow_dev(hits, who, P, N, 20.0, mset, mt, nmt.double(), nt, flow)


# ---- 6: the simulator end to end ---------------------------------------------------------------------------------------------------

def test_simulator_flow_entry(world, tmp_path):
    from lidarcast import flow as lf
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 4, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"period": 0.1, "objects": [
        {"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.3, 3.3, 1.4, 0.0, 140.0]]},
        {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]}]}
    plain = _sim(dict(base, movers=key), world.room).run_simulation(wps)
    one = _sim(dict(base, movers=dict(key, flow=True)), world.room).run_simulation(wps)
    assert one.get_total_frames() == 4
    seen = np.zeros(4, np.int64)
    for f, (a, b) in enumerate(zip(one.frames, plain.frames)):
        assert not hasattr(b, "flow") and not hasattr(b, "flow_status")             # without the entry nothing changes
        assert_bit_equal(a.points, b.points, f"frame {f}: points")
        assert a.mover_ids.tolist() == b.mover_ids.tolist()
        assert a.flow.dtype == np.float32 and a.flow_status.dtype == np.uint8
        assert len(a.flow) == len(a.flow_status) == len(a.mover_ids) == len(a.points) > 0 and a.flow.shape[1] == 3
        if f == 3:
            assert not a.flow_status.any() and not a.flow.view(np.uint32).any()     # the last frame has no next
            continue
        seen += np.bincount(a.flow_status, minlength=4)
        assert (a.flow_status != 0).all()
        walker, still = a.mover_ids == 1, a.mover_ids != 1
        assert not a.flow[still].view(np.uint32).any()                              # the room and the mover that stands still
        assert (a.flow[walker] != 0).any(axis=1).all()
        # a rigid step of 0.5 m and 40 degrees about z: no point of the pedestrian moves further than |step| + its radius * angle
        assert np.linalg.norm(a.flow[walker], axis=1).max() < 0.65 + 0.6 * np.deg2rad(40.0) + 1e-3 if walker.any() else True
        assert (a.flow[walker][:, 2] == 0).all()
        sf = lf.sensor_flow(a.points, a.flow, wps[f].to_pose_matrix(), wps[f + 1].to_pose_matrix())
        assert sf.shape == a.flow.shape and np.abs(sf[still]).max() > 0.1           # the sensor moves: static points flow in its frame
    assert seen[1] > 0 and seen[2] > 0 and seen[0] == 0, seen
    out = one.export_scene_flow(tmp_path)
    disk = np.load(tmp_path / "room_scene_flow.npz")
    off = disk["frame_offsets"]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(f.points) for f in one.frames])]).tolist()
    for f, a in enumerate(one.frames):
        sl = slice(off[f], off[f + 1])
        assert_bit_equal(disk["points"][sl], np.asarray(a.points, np.float32))
        assert_bit_equal(disk["flow"][sl], a.flow)
        assert disk["status"][sl].tolist() == a.flow_status.tolist() and disk["mover_ids"][sl].tolist() == a.mover_ids.tolist()
        assert np.array_equal(disk["sensor_poses"][f], wps[f].to_pose_matrix())
    assert disk["mover_poses12"].shape == (4, 2, 12) and sorted(out) == sorted(disk.files)
    with pytest.raises(ValueError, match="flow: true"):
        plain.export_scene_flow(tmp_path)
    for other, cfg in (("motion", {"speed": 0.5}), ("noise", {"seed": 1}), ("beam", {"divergence_mrad": 3.0}),
                       ("materials", {"classes": {}})):
        with pytest.raises(ValueError, match=f"movers key cannot be combined with the {other} key"):
            _sim(dict(base, movers=dict(key, flow=True), **{other: cfg}), world.room).run_simulation(wps)
