"""-m gpu: moving objects (lrc_scan_movers_dev / lrc_scan_movers_compact: the ray kernel, the explicit-ray launch per mover, the
merge kernel), on both node routes for the room and for the movers: the quantised images where a scene has them, and the float32
nodes of scenes created under LRC_QNODES=0.

The comparator is the numpy restatement of the header's steps (tests/mover_restate.py) over the EXISTING explicit-ray cast
(Scene.cast, no centre, no filter, which never culls): the static cast, one cast per mover of the rays taken into its frame, the
merge, and the record assembled on the host with the range filter in float64.  Every column must agree bit for bit -- t, prim,
normal3, point3, sem, ins, intensity and the mover column -- except incident_deg, where the device's acos meets libm's on
identical inputs: rtol 1e-13, as in tests/test_material_gpu.py.  Each case asserts on the restatement that it exercises what it
is for."""
import ctypes as C
import json

import numpy as np
import pytest

import helpers
import mover_restate as mv
from helpers import table_rays

pytestmark = pytest.mark.gpu

HITS = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg", "intensity")
CAST = ("t", "prim", "sem", "ins", "normal3")
FRAMES = ("point3", "sem", "ins", "incident_deg", "index", "range_origin")
ROUTES = ("quantised", "float32")


def assert_bit_equal(a, b, what=""):
    """helpers.assert_bit_equal, and plain equality for the one-byte column (mover)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.itemsize != 1:
        return helpers.assert_bit_equal(a, b, what)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ne = a != b
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} entries differ; first at {np.argwhere(ne)[0]}"


def _views(out):
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def scene_of(ctx, mesh):
    import lidarcast
    return lidarcast.Scene(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)


def cast_of(scene):
    return lambda rays: scene.cast(rays, center=None, max_range=np.inf, want=CAST)


def labelled(mesh, sem, ins):
    from lidarcast.synth import TriangleMesh
    n = len(mesh.triangles)
    return TriangleMesh(vertices=np.asarray(mesh.vertices, np.float64), triangles=np.asarray(mesh.triangles, np.int32),
                        triangle_sem=np.full(n, sem, np.uint16), triangle_ins=np.full(n, ins, np.uint16))


class World:
    """The room on both node routes, the mover meshes, and per route a mover set of all of them."""


@pytest.fixture(scope="module")
def world(engine):
    from lidarcast import synth
    from lidarcast.movers import MoverSet
    w = World()
    w.ctx = engine.ctx
    w.room = mv.room_mesh()
    cube = synth.unit_cube(-0.3, 0.3)                       # 0.6 m, 12 triangles: the host builder's tiny scene
    w.meshes = [synth.make_pedestrian(semantic=13, instance=1001), labelled(cube, 12, 1002),
                synth.make_pedestrian(semantic=13, instance=1003)]
    w.scenes = {"quantised": scene_of(w.ctx, w.room)}
    w.sets = {"quantised": MoverSet(w.ctx, w.meshes)}
    with pytest.MonkeyPatch.context() as mp:              # the variable is read at every scene creation
        mp.setenv("LRC_QNODES", "0")
        w.scenes["float32"] = scene_of(w.ctx, w.room)
        w.sets["float32"] = MoverSet(w.ctx, w.meshes)
    assert w.scenes["quantised"].info["quantised_nodes"] == 1 and w.scenes["float32"].info["quantised_nodes"] == 0
    assert all(s.info["quantised_nodes"] == 0 for s in w.sets["float32"].scenes)
    print("\n[movers] quantised nodes of the movers' scenes:", [s.info["quantised_nodes"] for s in w.sets["quantised"].scenes])
    w.one = {r: MoverSet(w.ctx, w.meshes[:1]) for r in ROUTES}      # (the route of a scene is fixed at its creation)
    w.casts = [cast_of(s) for s in w.sets["quantised"].scenes]
    w.static = cast_of(w.scenes["quantised"])
    yield w
    for d in (w.sets, w.one, w.scenes):
        for x in d.values():
            x.close()


def inputs(width):
    k, dirs, poses = mv.scan_inputs(width)
    rays, cen = table_rays(dirs, poses)
    return k, dirs, poses, rays, np.repeat(cen, len(dirs), axis=0)


def walker_poses(P=3):
    return np.stack([mv.pose12(*mv.walker_state(f)) for f in range(P)]).reshape(P, 1, 12)


def trio_poses(P=3):
    """the pedestrian on its walk, the cube beside it at chest height and turned, a second pedestrian 0.2 m into the first"""
    out = np.empty((P, 3, 12), np.float32)
    for f in range(P):
        x, y, z, yaw = mv.walker_state(f)
        out[f, 0] = mv.pose12(x, y, z, yaw)
        out[f, 1] = mv.pose12(x + 0.6, y + 0.5, 1.0, 0.3 + f)
        out[f, 2] = mv.pose12(x + 0.2, y - 0.1, 0.0, -yaw)
    return out


def movers_dev(scene, mset, poses, dirs, mover_poses, max_range, want=HITS, stream=None):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    mp = None if mover_poses is None else torch.from_numpy(np.ascontiguousarray(mover_poses, np.float32)).cuda()
    pt = torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    if stream is None:
        scene.scan_movers_dev(pt, dt, hits, max_range, mset, mp, mover_t=who)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            scene.scan_movers_dev(pt, dt, hits, max_range, mset, mp, mover_t=who, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["mover"] = who.cpu().numpy()
    return out


def clean_dev(scene, poses, dirs, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    scene.scan_poses_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                         torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def assert_records(got, want, what, columns=HITS + ("mover",)):
    for a in columns:
        if a == "incident_deg":
            g, w = got[a], want[a]
            err = np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)
            print(f"\n[movers] {what}: incident_deg of {len(g)} records, max relative difference {err.max() if len(g) else 0:.3g}")
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=0, err_msg=f"{what}: incident_deg")
        else:
            assert_bit_equal(got[a], want[a], f"{what}: {a}")


# ---- 1: the room with one pedestrian --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_room_with_one_pedestrian(world, route, width):
    """Width 100: 600 rays per pose, waves straddle poses; width 128: 768 rays, a pose is 12 whole waves.  max_range 1.6 m: the
    mover, the room and the filter each decide some rays (the filter removes returns of the mover and of the room)."""
    k, dirs, poses, rays, cen = inputs(width)
    mp = walker_poses()
    want, win = mv.scan(world.static, world.casts[:1], rays, cen, mp, len(dirs), 1.6)
    n_mover, n_room = int((want["mover"] == 1).sum()), int((want["keep"] & (want["mover"] == 0)).sum())
    n_far_mover = int(((win["mover"] == 1) & ~want["keep"]).sum())
    n_far_room = int(((win["mover"] == 0) & (win["t"] < np.inf) & ~want["keep"]).sum())
    print(f"\n[movers] one pedestrian, width {width}: mover {n_mover}, room {n_room}, filtered mover {n_far_mover}, filtered room {n_far_room}")
    assert n_mover > 100 and n_room > 100 and n_far_mover > 0 and n_far_room > 100
    assert (len(dirs) % 64 == 0) == (width == 128)
    got = movers_dev(world.scenes[route], world.one[route], poses, dirs, mp, 1.6)
    assert_records(got, want, f"one pedestrian, width {width}, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_incident_mode_1_uses_the_written_normal(world, route):
    k, dirs, poses, rays, cen = inputs(100)
    mp = walker_poses()
    want, _ = mv.scan(world.static, world.casts[:1], rays, cen, mp, len(dirs), k.max_range, incident_mode=1)
    scene = world.scenes[route]
    try:
        scene.set_options(incident_mode=1)
        got = movers_dev(scene, world.one[route], poses, dirs, mp, k.max_range)
    finally:
        scene.reset_options()
    assert (want["mover"] == 1).sum() > 200
    assert_records(got, want, f"incident_mode 1, {route} nodes")


# ---- 2: three movers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_three_movers(world, route, width):
    k, dirs, poses, rays, cen = inputs(width)
    mp = trio_poses()
    want, win = mv.scan(world.static, world.casts, rays, cen, mp, len(dirs), k.max_range)
    wins = np.bincount(want["mover"], minlength=4)
    # the second pedestrian stands inside the first: some rays meet both, and each wins some of those
    both = np.zeros(len(rays), bool)
    N = len(dirs)
    for p in range(3):
        sl = slice(p * N, (p + 1) * N)
        t0 = world.casts[0](mv.to_object(rays[sl], mp[p, 0]))["t"]
        t2 = world.casts[2](mv.to_object(rays[sl], mp[p, 2]))["t"]
        both[sl] = (t0 < np.inf) & (t2 < np.inf)
    print(f"\n[movers] three movers, width {width}: room / pedestrian / cube / second pedestrian win {wins.tolist()} rays, "
          f"{int(both.sum())} rays meet both pedestrians")
    assert (wins > 0).all() and len(world.meshes[1].triangles) == 12
    assert (want["mover"][both] == 1).any() and (want["mover"][both] == 3).any()
    assert set(want["ins"][want["mover"] == 2].tolist()) == {1002} and set(want["ins"][want["mover"] == 3].tolist()) == {1003}
    assert want["prim"][want["mover"] == 2].max() < 12               # the row in the winner's own mesh
    got = movers_dev(world.scenes[route], world.sets[route], poses, dirs, mp, k.max_range)
    assert_records(got, want, f"three movers, width {width}, {route} nodes")


# ---- 3: ties -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_a_copy_of_the_room_never_wins(world, route):
    """Every ray meets the room and its copy at the same float32 range: the static scene keeps every tie."""
    from lidarcast.movers import MoverSet
    k, dirs, poses, rays, cen = inputs(100)
    ident = np.tile(mv.pose12(0.0, 0.0, 0.0, 0.0), (3, 1, 1))
    with pytest.MonkeyPatch.context() as mp:
        if route == "float32":
            mp.setenv("LRC_QNODES", "0")
        copy = MoverSet(world.ctx, [labelled(world.room, 99, 9999)])
    try:
        moved = mv.to_object(rays, ident[0, 0])
        assert np.array_equal(moved, rays)                               # the identity: the same rays, hence the same ranges
        clean = clean_dev(world.scenes[route], poses, dirs, k.max_range)
        assert (clean["t"] < np.inf).sum() > 1500
        got = movers_dev(world.scenes[route], copy, poses, dirs, ident, k.max_range)
        assert not got["mover"].any()
        assert_records(got, clean, f"copy of the room, {route} nodes", columns=HITS)
        assert_bit_equal(got["incident_deg"], clean["incident_deg"], "the clean scan's own bytes")
        assert 99 not in got["sem"]
    finally:
        copy.close()


@pytest.mark.parametrize("route", ROUTES)
def test_two_identical_movers_give_only_the_first(world, route):
    from lidarcast.movers import MoverSet
    k, dirs, poses, rays, cen = inputs(100)
    with pytest.MonkeyPatch.context() as mp:
        if route == "float32":
            mp.setenv("LRC_QNODES", "0")
        twins = MoverSet(world.ctx, [world.meshes[0], labelled(world.meshes[0], 14, 2002)])
    try:
        mp2 = np.repeat(walker_poses(), 2, axis=1)
        want, _ = mv.scan(world.static, [world.casts[0], world.casts[0]], rays, cen, mp2, len(dirs), k.max_range)
        got = movers_dev(world.scenes[route], twins, poses, dirs, mp2, k.max_range)
        assert (got["mover"] == 1).sum() == 18 + 204 + 25 and not (got["mover"] == 2).any()
        assert 14 not in got["sem"] and 2002 not in got["ins"]
        assert_records(got, want, f"twins, {route} nodes", columns=("t", "prim", "normal3", "point3", "mover", "intensity"))
    finally:
        twins.close()


# ---- 4: no movers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_no_movers_is_the_clean_scan(world, route):
    k, dirs, poses, rays, cen = inputs(100)
    clean = clean_dev(world.scenes[route], poses, dirs, k.max_range)
    got = movers_dev(world.scenes[route], None, poses, dirs, None, k.max_range)
    assert not got["mover"].any()
    for a in HITS:
        assert_bit_equal(got[a], clean[a], f"NULL set, {route} nodes: {a}")
    # a mover every ray of which lies beyond max_range: in sight, hit, and filtered with what stands behind it
    far = np.tile(mv.pose12(2.6, 0.5, 0.0, 0.5), (3, 1, 1))
    want, win = mv.scan(world.static, world.casts[:1], rays, cen, far, len(dirs), 1.0)
    assert (win["mover"] == 1).sum() > 20 and not want["mover"].any() and want["keep"].sum() > 50
    clean = clean_dev(world.scenes[route], poses, dirs, 1.0)
    got = movers_dev(world.scenes[route], world.one[route], poses, dirs, far, 1.0)
    assert not got["mover"].any()
    for a in HITS:
        assert_bit_equal(got[a], clean[a], f"mover beyond max_range, {route} nodes: {a}")


# ---- 5: min_range ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_min_range_does_not_uncover_a_mover(world, route):
    """The pedestrian stands OUTSIDE the room behind the wall x = 0, 1.2 m from the first pose; min_range 1.6 m removes the
    wall's near returns.  The pedestrian behind them, beyond 1.6 m, stays hidden."""
    k, dirs, poses, rays, cen = inputs(100)
    outside = np.tile(mv.pose12(-0.6, 1.0, 0.0, 0.2), (3, 1, 1))
    want, win = mv.scan(world.static, world.casts[:1], rays, cen, outside, len(dirs), k.max_range, min_range=1.6)
    N = len(dirs)
    tm = world.casts[0](mv.to_object(rays[:N], outside[0, 0]))["t"]
    ts = win["t"][:N]
    hidden = (ts < tm) & (tm < np.inf) & ~want["keep"][:N] & (tm > 1.6)
    print(f"\n[movers] min_range: {int(hidden.sum())} rays have a removed wall return in front of the pedestrian")
    assert hidden.sum() >= 5 and not want["mover"].any()
    assert np.isinf(want["t"][:N][hidden]).all()
    scene = world.scenes[route]
    try:
        scene.set_options(min_range=1.6)
        got = movers_dev(scene, world.one[route], poses, dirs, outside, k.max_range)
    finally:
        scene.reset_options()
    assert_records(got, want, f"min_range, {route} nodes")


# ---- 6: chunking -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
def test_six_poses_equal_two_then_four(world, width):
    k, dirs, poses, rays, cen = inputs(width)
    poses6 = np.concatenate([poses, poses[::-1]])
    mp6 = np.concatenate([trio_poses(), trio_poses()[[1, 2, 0]]])
    scene, mset = world.scenes["quantised"], world.sets["quantised"]
    whole = movers_dev(scene, mset, poses6, dirs, mp6, k.max_range)
    a = movers_dev(scene, mset, poses6[:2], dirs, mp6[:2], k.max_range)
    b = movers_dev(scene, mset, poses6[2:], dirs, mp6[2:], k.max_range)
    assert (np.bincount(whole["mover"], minlength=4) > 0).all()
    for col in HITS + ("mover",):
        assert_bit_equal(whole[col], np.concatenate([a[col], b[col]]), f"2 + 4 poses, width {width}: {col}")


# ---- 7: frames ---------------------------------------------------------------------------------------------------------------------

def host_frames(rec, P, N):
    """Host compaction of fixed-stride records: what lrc_scan_movers_compact must return."""
    keep = (rec["t"] != np.inf).reshape(P, N)
    sel = keep.reshape(-1)
    pts = rec["point3"][sel]
    return {"counts": keep.sum(1), "point3": pts, "sem": rec["sem"][sel], "ins": rec["ins"][sel],
            "incident_deg": rec["incident_deg"][sel], "index": np.nonzero(keep)[1].astype(np.uint32),
            "range_origin": np.linalg.norm(pts, axis=1) if len(pts) else np.zeros(0, np.float32), "mover": rec["mover"][sel]}


def assert_frames_equal(fr, want, what):
    assert fr["counts"].tolist() == want["counts"].tolist(), what
    for k in ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "mover"):
        assert_bit_equal(fr[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("route", ROUTES)
def test_compact_frames(world, route):
    k, dirs, poses, rays, cen = inputs(100)
    scene, mset, mp = world.scenes[route], world.sets[route], trio_poses()
    rec = movers_dev(scene, mset, poses, dirs, mp, 3.0)
    want = host_frames(rec, 3, len(dirs))
    assert (np.bincount(want["mover"], minlength=4) > 0).all() and 0 < want["counts"].sum() < 3 * len(dirs)
    fr = scene.scan_movers_compact(poses, dirs, 3.0, mset, mp, want=FRAMES)
    assert_frames_equal(fr, want, f"compact, {route} nodes")
    small = scene.scan_movers_compact(poses, dirs, 3.0, mset, mp, want=("point3",))          # no index column asked for
    assert "index" not in small
    assert_bit_equal(small["point3"], want["point3"])
    assert_bit_equal(small["mover"], want["mover"])
    with pytest.raises(ValueError, match="capacity"):
        scene.scan_movers_compact(poses, dirs, 3.0, mset, mp, want=FRAMES, capacity=10)
    none = scene.scan_movers_compact(poses, dirs, 3.0, None, None, want=FRAMES)
    clean = scene.scan_poses_compact(poses, dirs, 3.0, want=FRAMES)
    assert none["counts"].tolist() == clean["counts"].tolist() and not none["mover"].any() and len(none["mover"]) == clean["total"]
    for a in FRAMES:
        assert_bit_equal(none[a], clean[a], f"NULL set, compact: {a}")


def test_engine_scan_mover_frames(engine, world):
    from lidarcast.movers import MoverSet
    k, dirs, poses, rays, cen = inputs(100)
    mp = trio_poses()
    mset = MoverSet(engine.ctx, world.meshes)
    try:
        fr = engine.scan_mover_frames(k, poses, world.room, mset, mp, want=FRAMES)
        want, _ = mv.scan(world.static, world.casts, rays, cen, mp, len(dirs), k.max_range)
        ref = host_frames(want, 3, len(dirs))
        assert fr["counts"].tolist() == ref["counts"].tolist()
        for a in ("point3", "sem", "ins", "index", "mover"):
            assert_bit_equal(fr[a], ref[a], f"engine: {a}")
    finally:
        mset.close()
    with pytest.raises(ValueError, match="direction table"):
        engine.scan_mover_frames(object(), poses, world.room, None, None)


# ---- 8: a stream of the caller's ---------------------------------------------------------------------------------------------------

def test_non_default_stream(world):
    import torch
    k, dirs, poses, rays, cen = inputs(128)
    mp = trio_poses()
    scene, mset = world.scenes["quantised"], world.sets["quantised"]
    ref = movers_dev(scene, mset, poses, dirs, mp, k.max_range)
    got = movers_dev(scene, mset, poses, dirs, mp, k.max_range, stream=torch.cuda.Stream())
    for col in HITS + ("mover",):
        assert_bit_equal(got[col], ref[col], f"own stream: {col}")


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------------

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
    pt = torch.from_numpy(poses.reshape(P, 16).copy()).cuda()
    dt = torch.from_numpy(dirs).cuda()
    mt = torch.from_numpy(mp).cuda()
    with pytest.raises(ValueError, match="1 to 255"):
        MoverSet(engine.ctx, [])
    with pytest.raises(ValueError, match="1 to 255"):
        MoverSet(engine.ctx, [world.meshes[1]] * 256)
    h = C.c_void_p()
    arr = (C.c_void_p * 1)(scene._h)
    assert lib.lrc_movers_create(engine.ctx._h, arr, 0, C.byref(h)) == E and b"[1, 255]" in lib.lrc_last_error()
    # the static scene as one of its own movers
    assert lib.lrc_movers_create(engine.ctx._h, arr, 1, C.byref(h)) == 0
    try:
        hits = DeviceHits(P * N, "cuda", want=("t",))
        assert lib.lrc_scan_movers_dev(scene._h, h, pt.data_ptr(), P, dt.data_ptr(), N, mt.data_ptr(), 20.0, C.byref(hits.struct), None,
                                       None) == E
        assert b"one of its own movers" in lib.lrc_last_error()
    finally:
        lib.lrc_movers_destroy(h)
    # a mover scene, and a set, of another context
    other = lidarcast.Context(0)
    try:
        assert lib.lrc_movers_create(other._h, arr, 1, C.byref(h)) == E and b"another context" in lib.lrc_last_error()
        foreign = MoverSet(other, world.meshes[:1])
        with pytest.raises(ValueError, match="another context"):
            scene.scan_movers_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, foreign, mt)
        hits = DeviceHits(P * N, "cuda", want=("t",))
        assert lib.lrc_scan_movers_dev(scene._h, foreign._h, pt.data_ptr(), P, dt.data_ptr(), N, mt.data_ptr(), 20.0,
                                       C.byref(hits.struct), None, None) == E
        assert b"different contexts" in lib.lrc_last_error()
        foreign.close()
    finally:
        other.close()
    with pytest.raises(ValueError, match="tile_count"):
        scene.scan_movers_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t", "tile_count")), 20.0, mset, mt)
    noise = torch.zeros(P * N, dtype=torch.float32, device="cuda")
    try:
        scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_movers_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, mset, mt)
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_movers_compact(poses, dirs, 20.0, mset, mp)
    finally:
        scene.reset_options()
    bad = mp.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        scene.scan_movers_compact(poses, dirs, 20.0, mset, bad)
    bad = mp.copy()
    bad[2, 0, 0] += np.float32(2.0 ** -14)                 # R^T R - I of about 2^-13 cos(yaw): no rotation
    with pytest.raises(ValueError, match="no rotation"):
        scene.scan_movers_compact(poses, dirs, 20.0, mset, bad)
    ok = mp.copy()
    ok[2, 0, 0] = np.nextafter(ok[2, 0, 0], np.float32(2))        # one ulp: within 2^-16
    assert scene.scan_movers_compact(poses, dirs, 20.0, mset, ok)["total"] > 0
    with pytest.raises(ValueError, match=r"\(P, M, 12\)"):
        scene.scan_movers_compact(poses, dirs, 20.0, mset, mp[:2])
    with pytest.raises(ValueError, match="P \\* N records"):
        scene.scan_movers_dev(pt, dt, DeviceHits(P * N + 1, "cuda", want=("t",)), 20.0, mset, mt)
    for kw, what in ((dict(mover_t=torch.zeros(P * N, dtype=torch.int32, device="cuda")), "mover_t must be torch.uint8"),
                     (dict(mover_t=torch.zeros(P * N, dtype=torch.uint8)), "mover_t must lie on the device"),
                     (dict(mover_t=torch.zeros(3, dtype=torch.uint8, device="cuda")), "mover_t must hold")):
        with pytest.raises(ValueError, match=what):
            scene.scan_movers_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, mset, mt, **kw)
    with pytest.raises(ValueError, match="mover_poses_t must be torch.float32"):
        scene.scan_movers_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, mset, mt.double())


# ---- 10: the simulator end to end --------------------------------------------------------------------------------------------------

def _sim(config, mesh, **kw):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator(config, **kw)
    sim.load_scene(mesh, "room")
    return sim


def test_simulator_movers_key(world, tmp_path, monkeypatch):
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 4, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"period": 0.1, "objects": [
        {"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.3, 3.3, 1.4, 0.0, 140.0]]},
        {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]}]}
    clean = _sim(dict(base), world.room).run_simulation(wps)
    sim = _sim(dict(base, movers=key), world.room)
    one = sim.run_simulation(wps)
    assert one.get_total_frames() == 4
    tracks = one.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "room_mover_tracks.json"))
    assert disk["num_frames"] == 4 and len(disk["objects"]) == 2 and disk == json.loads(json.dumps(tracks))
    seen = np.zeros(3, np.int64)
    for f, (a, c) in enumerate(zip(one.frames, clean.frames)):
        ids = a.mover_ids
        assert ids.dtype == np.uint8 and len(ids) == len(a.points) == len(a.semantic_labels) > 0
        counts = np.bincount(ids, minlength=3)
        seen += counts
        assert disk["frames"][f]["static_points"] == counts[0]
        assert [m["num_points"] for m in disk["frames"][f]["movers"]] == counts[1:].tolist()
        assert (a.semantic_labels[ids == 1] == 13).all() and (a.instance_labels[ids == 1] == 1001).all()
        assert (a.semantic_labels[ids == 2] == 12).all() and (a.instance_labels[ids == 2] == 1002).all()
        assert not np.isin(a.instance_labels[ids == 0], (1001, 1002)).any()
        assert not hasattr(c, "mover_ids")                                     # without the key nothing changes
        assert np.isclose(disk["frames"][f]["time"], 0.1 * f)
    assert (seen > 0).all(), seen
    assert np.allclose([disk["frames"][3]["movers"][0]["pose"][a] for a in ("x", "y", "yaw_deg")], [3.3, 1.4, 140.0])
    # what the key does not cover raises instead of quietly scanning something else
    for other, cfg in (("motion", {"speed": 0.5}), ("noise", {"seed": 1}), ("beam", {"divergence_mrad": 3.0}),
                       ("materials", {"classes": {}})):
        with pytest.raises(ValueError, match=f"movers key cannot be combined with the {other} key"):
            _sim(dict(base, movers=key, **{other: cfg}), world.room).run_simulation(wps)
    with pytest.raises(ValueError, match="dual-axis"):
        _sim(dict(base, movers=key), world.room, use_blk2go=True).run_simulation(wps[:2])
    with pytest.raises(ValueError, match="unknown entries under the movers key"):
        _sim(dict(base, movers=dict(key, speed=2)), world.room).run_simulation(wps)
    for export in (lambda: sim.evaluate_surface_coverage(wps), lambda: sim.export_occupancy_grid(wps, "unused"),
                   lambda: sim.export_frame_annotations(wps, "unused")):
        with pytest.raises(NotImplementedError, match="movers key"):
            export()
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(ValueError, match="multi-rank"):
        sim.run_simulation(wps)
