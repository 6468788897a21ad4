"""-m gpu: non-rigid scene flow (lrc_scan_nonrigid_flow_dev: nonrigid_target_kernel in front of the passes of lrc_scan_flow_dev;
lrc_deform_snapshot_dev; lidarcast.deform.scan_deforming_flow_dev / scan_deforming_flow_frames; the simulator's nonrigid_flow key).

The comparator is the numpy restatement of the header's steps (tests/nonrigid_flow_restate.py) applied to the records the scan
left on the device.  Its casts are the EXISTING explicit-ray cast (Scene.cast) on the room and, for a deformable, on a FRESH scene
built from Deformable.vertices() of the next shape: the refit is not its own witness.  flow3 and status must agree bit for bit.
Three frames; frame k is paired with k + 1 and the last has no next.  The deformable always has float32 nodes; the room is
scanned on both node routes."""
import ctypes as C

import numpy as np
import pytest

import flow_restate as fl
import mover_restate as mv
import nonrigid_flow_restate as nr
from helpers import assert_bit_equal
from test_deform_gpu import case as deform_case
from test_flow_gpu import assert_same_bytes, counts_per_frame, hidden_by
from test_movers_gpu import ROUTES, _sim, cast_of, engine, inputs, walker_poses, world  # noqa: F401  (engine, world: fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
HITS = ("t", "point3", "prim")
SHAPES = np.array([[[0, 1, 0.37]], [[2, 3, 0.8]], [[5, 6, 0.5]]], np.float64)
WALK = [(2.2, 1.3, 0.5), (3.2, 2.6, 1.2), (5.5, 3.0, 1.9)]          # the last pose lies outside the room, behind the wall x = 5


class Cast:
    """The walker as a deformable, a rigid pedestrian, their set, and fresh scenes of the walker's shapes by request."""


@pytest.fixture(scope="module")
def cast(world):
    import lidarcast
    from lidarcast import deform, synth
    from lidarcast.movers import MoverSet
    c = Cast()
    c.ctx = world.ctx
    c.walker = synth.make_walker(instance=1001)
    c.keys, c.tris = c.walker.keyframes, np.asarray(c.walker.triangles, np.uint32)
    c.d = deform.Deformable(c.ctx, c.keys, c.walker.triangles, c.walker.triangle_sem, c.walker.triangle_ins)
    c.ped = world.meshes[0]
    c.mset = MoverSet(c.ctx, [c.d, c.ped])
    c.ped_cast = cast_of(c.mset.scenes[1])
    c.fresh = {}

    def shape(s3):
        """(vertices read back from the deformable set to s3, the cast of a fresh scene of them): built once per shape"""
        key = (int(s3[0]), int(s3[1]), float(F32(s3[2])))
        if key not in c.fresh:
            c.d.set(*key)
            v = c.d.vertices()
            assert_bit_equal(v, deform.blend(c.keys[key[0]], c.keys[key[1]], key[2]), f"vertices of shape {key}")
            sc = lidarcast.Scene(c.ctx, v, c.walker.triangles, c.walker.triangle_sem, c.walker.triangle_ins)
            c.fresh[key] = (v, sc, cast_of(sc))
        return c.fresh[key][0], c.fresh[key][2]
    c.shape = shape
    yield c
    c.mset.close()
    c.d.close()
    for _, sc, _ in c.fresh.values():
        sc.close()


def mover_poses(walk=WALK):
    ped = walker_poses()
    out = np.empty((3, 2, 12), F32)
    for f in range(3):
        out[f, 0] = mv.pose12(walk[f][0], walk[f][1], 0.0, walk[f][2])
        out[f, 1] = ped[f, 0]
    return out


def tensors(poses, dirs, mp):
    import torch
    P = len(poses)
    return (torch.from_numpy(np.ascontiguousarray(poses, np.float64).reshape(P, 16)).cuda(),
            torch.from_numpy(np.ascontiguousarray(dirs, np.float64)).cuda(), torch.from_numpy(np.ascontiguousarray(mp, F32)).cuda())


def outputs(n):
    import torch
    from lidarcast import DeviceHits
    return (DeviceHits(n, "cuda", want=HITS), torch.full((n,), 255, dtype=torch.uint8, device="cuda"),
            torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda"), torch.full((n,), 255, dtype=torch.uint8, device="cuda"))


def read(hits, who, flow, status):
    import torch
    torch.cuda.synchronize()
    return {"t": hits["t"].cpu().numpy(), "point3": hits["point3"].cpu().numpy(), "prim": hits["prim"].cpu().numpy().view(np.uint32),
            "mover": who.cpu().numpy(), "flow3": flow.cpu().numpy(), "status": None if status is None else status.cpu().numpy()}


def loop_dev(scene, mset, poses, dirs, mp, shapes, max_range, with_status=True, stream=None):
    """scan_deforming_flow_dev on fresh outputs; the records and the two columns as numpy arrays"""
    import torch
    from lidarcast import deform
    pt, dt, mt = tensors(poses, dirs, mp)
    hits, who, flow, status = outputs(len(poses) * len(dirs))
    status = status if with_status else None
    if stream is None:
        deform.scan_deforming_flow_dev(scene, pt, dt, hits, max_range, mset, mt, shapes, flow, status, mover_t=who)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            deform.scan_deforming_flow_dev(scene, pt, dt, hits, max_range, mset, mt, shapes, flow, status, mover_t=who,
                                           stream=stream.cuda_stream)
    return read(hits, who, flow, status)


def restated(world, cast, got, poses, mp, shapes, N, max_range):
    """The restatement frame by frame: the pair is (vertices of shape k, vertices of shape k + 1) when the shape changes, the
    walker's cast that of a fresh scene of shape k + 1."""
    P = len(poses)
    flow3, status = np.zeros((P * N, 3), F32), np.zeros(P * N, np.uint8)
    details = []
    for k in range(P - 1):
        sl = slice(k * N, (k + 1) * N)
        va, _ = cast.shape(shapes[k, 0])
        vb, walker_cast = cast.shape(shapes[k + 1, 0])
        pairs = [] if np.array_equal(shapes[k], shapes[k + 1]) else [(0, va, vb, cast.tris)]
        flow3[sl], status[sl], d = nr.scan(world.static, [walker_cast, cast.ped_cast], got["t"][sl], got["point3"][sl], got["mover"][sl],
                                           got["prim"][sl], mp[k:k + 1], mp[k + 1:k + 2], poses[k + 1:k + 2], None, N, max_range, pairs)
        details.append(d)
    last = {k: np.zeros_like(v) for k, v in details[0].items() if k != "t_movers"}
    last["t_movers"] = np.zeros_like(details[0]["t_movers"])
    details.append(last)
    d = {k: np.concatenate([x[k] for x in details], axis=1 if k == "t_movers" else 0) for k in details[0]}
    return flow3, status, d


def assert_flow(got, flow3, status, what):
    assert_bit_equal(got["flow3"], flow3, f"{what}: flow3")
    ne = got["status"] != status
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} status bytes differ; first at {np.argwhere(ne)[0]}"


def rigid_flow(scene, mset, got, poses, mp, N, max_range, with_status=True):
    """lrc_scan_flow_dev on the records ``got`` holds, frame k paired with k + 1"""
    import torch
    from lidarcast import DeviceHits
    P = len(poses)
    nxt, nmp, has = fl.pair_next(poses, mp)
    hits = DeviceHits(P * N, "cuda", want=HITS)
    for a in HITS:
        hits[a].copy_(torch.from_numpy(got[a].view(np.int32) if a == "prim" else got[a]).cuda())
    _, _, flow, status = outputs(P * N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    scene.scan_flow_dev(hits, dev(got["mover"]), P, N, max_range, mset, dev(mp), dev(nmp), dev(nxt.reshape(P, 16)), flow,
                        status_t=status if with_status else None, has_next_t=dev(has))
    torch.cuda.synchronize()
    return flow.cpu().numpy(), status.cpu().numpy()


# ---- 1: the room with the walker and a rigid pedestrian ------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_room_with_the_walker_and_a_pedestrian(world, cast, route, width):
    k, dirs, poses, rays, cen = inputs(width)
    mp, N = mover_poses(), len(dirs)
    got = loop_dev(world.scenes[route], cast.mset, poses, dirs, mp, SHAPES, 3.0)
    flow3, status, d = restated(world, cast, got, poses, mp, SHAPES, N, 3.0)
    counts, by = counts_per_frame(got, status, N), hidden_by(got, d, status, N)
    print(f"\n[nonrigid] walker and pedestrian, width {width}, {route}: status per frame {counts}, hidden (owner, by) {by}, "
          f"{int(d['paired'].sum())} paired rows")
    assert (N % 64 == 0) == (width == 128)
    assert by[(1, 1)] > 0 and by[(1, 0)] > 0 and by[(0, 1)] > 0           # the walker by itself and by the room, the room by the walker
    seen = np.bincount(status, minlength=4)
    assert seen[fl.VISIBLE] > 0 and seen[fl.OCCLUDED] > 0 and seen[fl.NONE] > 0
    assert counts[2][1:] == [0, 0, 0]
    walker = (got["mover"] == 1) & (got["t"] < np.inf)
    assert d["paired"].sum() == walker[:2 * N].sum() > 50 and (got["mover"] == 2).sum() > 10
    assert (flow3[:2 * N][walker[:2 * N]] != 0).any(axis=1).all()
    assert_flow(got, flow3, status, f"walker and pedestrian, width {width}, {route} nodes")


# ---- 2: the shape changes, the pose stands --------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_the_shape_changes_and_the_pose_stands(world, cast, route):
    """The rigid flow of the same records is +0 on every walker row; the non-rigid flow of the limb rows is not."""
    k, dirs, poses, rays, cen = inputs(100)
    mp, N = mover_poses([WALK[0]] * 3), len(dirs)
    poses = np.stack([poses[0]] * 3)                                      # the sensor stands as well: the walker stays in view
    shapes = np.array([[[1, 1, 0.0]], [[7, 7, 0.0]], [[2, 3, 0.5]]], np.float64)
    scene = world.scenes[route]
    got = loop_dev(scene, cast.mset, poses, dirs, mp, shapes, 3.0)
    flow3, status, d = restated(world, cast, got, poses, mp, shapes, N, 3.0)
    assert_flow(got, flow3, status, f"shape changes, pose stands, {route} nodes")
    rigid3, _ = rigid_flow(scene, cast.mset, got, poses, mp, N, 3.0)
    walker = (got["mover"] == 1) & (got["t"] < np.inf)
    walker[2 * N:] = False
    assert walker.sum() > 30 and not rigid3[walker].view(np.uint32).any()
    # keyframes 1 -> 7 (frame 0): torso and head keep their bits, the limbs move
    va, vb = cast.shape(shapes[0, 0])[0], cast.shape(shapes[1, 0])[0]
    moves = (va.view(np.uint32) != vb.view(np.uint32)).any(axis=1)[cast.tris.astype(np.int64)]
    first = walker.copy()
    first[N:] = False
    limb, still = first & moves.all(axis=1)[got["prim"] % len(cast.tris)], first & ~moves.any(axis=1)[got["prim"] % len(cast.tris)]
    print(f"\n[nonrigid] pose stands, {route}: {int(walker.sum())} walker rows, frame 0: {int(limb.sum())} limb rows, {int(still.sum())} "
          f"rows on triangles that stand, largest limb flow {np.abs(got['flow3'][limb]).max():.4f} m")
    assert limb.sum() > 5 and still.sum() > 5
    assert (got["flow3"][limb] != 0).any(axis=1).all() and not got["flow3"][still].view(np.uint32).any()
    assert (got["flow3"][walker & (np.arange(3 * N) >= N)] != 0).any()     # frame 1: every vertex moves


# ---- 3: properties ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_equal_shapes_give_the_rigid_bytes(world, cast, route):
    k, dirs, poses, rays, cen = inputs(100)
    mp, N = mover_poses(), len(dirs)
    shapes = np.repeat(SHAPES[1:2], 3, axis=0)
    scene = world.scenes[route]
    got = loop_dev(scene, cast.mset, poses, dirs, mp, shapes, 3.0)
    rigid3, rigid_status = rigid_flow(scene, cast.mset, got, poses, mp, N, 3.0)
    assert (got["flow3"] != 0).any() and (np.bincount(got["status"], minlength=4)[:3] > 0).all()
    assert_flow(got, rigid3, rigid_status, f"equal shapes, {route} nodes")


def direct(scene, cast, poses, dirs, mp, shapes, max_range, pairs_of, with_status=True):
    """One frame 0 -> 1 by the device calls themselves: set, scan, snapshot, set, flow with ``pairs_of(snapshot)``."""
    import torch
    N = len(dirs)
    pt, dt, mt = tensors(poses, dirs, mp)
    hits, who, flow, status = outputs(N)
    cast.d.set(int(shapes[0, 0, 0]), int(shapes[0, 0, 1]), shapes[0, 0, 2])
    scene.scan_movers_dev(pt[:1], dt, hits, max_range, cast.mset, mt[:1], mover_t=who)
    snap = cast.d.snapshot()
    cast.d.set(int(shapes[1, 0, 0]), int(shapes[1, 0, 1]), shapes[1, 0, 2])
    scene.scan_nonrigid_flow_dev(hits, who, 1, N, max_range, cast.mset, mt[:1], mt[1:2], pt[1:2], flow, pairs=pairs_of(snap),
                                 status_t=status if with_status else None)
    out = read(hits, who, flow, status if with_status else None)
    out["snapshot"] = snap.cpu().numpy()
    return out


def test_no_pairs_give_the_rigid_bytes(world, cast):
    k, dirs, poses, rays, cen = inputs(100)
    mp, N = mover_poses(), len(dirs)
    scene = world.scenes["quantised"]
    got = direct(scene, cast, poses, dirs, mp, SHAPES, 3.0, lambda snap: [])
    twice = {a: np.concatenate([got[a], got[a]]) for a in HITS + ("mover",)}          # frame 0 of two: it flows to frame 1
    rigid3, rigid_status = rigid_flow(scene, cast.mset, twice, poses[:2], mp[:2], N, 3.0)
    assert_flow(got, rigid3[:N], rigid_status[:N], "num_pairs == 0")
    assert (got["flow3"] != 0).any()
    both = direct(scene, cast, poses, dirs, mp, SHAPES, 3.0, lambda snap: [(0, snap, None)])
    assert_bit_equal(both["snapshot"], cast.shape(SHAPES[0, 0])[0], "snapshot")
    assert not np.array_equal(both["flow3"], got["flow3"])                 # the pair matters
    explicit = direct(scene, cast, poses, dirs, mp, SHAPES, 3.0, lambda snap: [(0, snap, cast.d.snapshot())])
    assert_flow(explicit, both["flow3"], both["status"], "an explicit next shape equals the current vertices")


def test_status_null_gives_the_same_flow_bytes(world, cast):
    k, dirs, poses, rays, cen = inputs(100)
    mp = mover_poses()
    scene = world.scenes["quantised"]
    both = loop_dev(scene, cast.mset, poses, dirs, mp, SHAPES, 3.0)
    alone = loop_dev(scene, cast.mset, poses, dirs, mp, SHAPES, 3.0, with_status=False)
    assert alone["status"] is None and (both["flow3"] != 0).any()
    assert_bit_equal(alone["flow3"], both["flow3"], "status NULL: flow3")


@pytest.mark.parametrize("width", [100, 128])
def test_three_frames_equal_one_frame_plus_two(world, cast, width):
    """The loop over frames 0, 1, 2 against the loop over 0, 1 (its frame 0: one frame) and the loop over 1, 2 (two frames)."""
    k, dirs, poses, rays, cen = inputs(width)
    mp, N = mover_poses(), len(dirs)
    scene = world.scenes["quantised"]
    whole = loop_dev(scene, cast.mset, poses, dirs, mp, SHAPES, 3.0)
    a = loop_dev(scene, cast.mset, poses[:2], dirs, mp[:2], SHAPES[:2], 3.0)
    b = loop_dev(scene, cast.mset, poses[1:], dirs, mp[1:], SHAPES[1:], 3.0)
    for c in ("t", "point3", "prim", "mover", "flow3", "status"):
        assert_same_bytes(whole[c], np.concatenate([a[c][:N], b[c]]), f"1 + 2 frames, width {width}: {c}")
    assert not a["flow3"][N:].view(np.uint32).any() and not a["status"][N:].any()       # a's last frame has no next


def test_a_strip_past_the_launch_edge_as_the_only_mover(world):
    """strip257: V = 257 and 255 triangles, slots past the 256-wide launches of the refit."""
    import lidarcast
    from lidarcast import deform
    from lidarcast.movers import MoverSet
    keys, t, sem, ins, _ = deform_case("strip257")
    d = deform.Deformable(world.ctx, keys, t, sem, ins)
    mset = MoverSet(world.ctx, [d])
    fresh = None
    try:
        k, dirs, poses, rays, cen = inputs(100)
        N = len(dirs)
        poses = np.stack([poses[0], poses[0]])
        mp = np.stack([mv.pose12(0.8, 0.8, 0.5, 0.2), mv.pose12(0.9, 0.9, 0.55, 0.4)]).reshape(2, 1, 12)
        shapes = np.array([[[0, 1, 0.6]], [[1, 2, 0.3]]], np.float64)
        scene = world.scenes["quantised"]
        got = loop_dev(scene, mset, poses, dirs, mp, shapes, 4.0)
        va = deform.blend(keys[0], keys[1], 0.6)
        d.set(1, 2, 0.3)
        vb = d.vertices()
        fresh = lidarcast.Scene(world.ctx, vb, t, sem, ins)
        flow3, status, det = nr.scan(world.static, [cast_of(fresh)], got["t"][:N], got["point3"][:N], got["mover"][:N], got["prim"][:N],
                                     mp[:1], mp[1:], poses[1:], None, N, 4.0, [(0, va, vb, t)])
        print(f"\n[nonrigid] strip257: {int(det['paired'].sum())} paired rows, status {np.bincount(status, minlength=4).tolist()}")
        assert det["paired"].sum() > 15 and (flow3[det["paired"]] != 0).any(axis=1).all()
        assert_bit_equal(got["flow3"][:N], flow3, "strip257: flow3")
        assert got["status"][:N].tolist() == status.tolist()
        assert not got["flow3"][N:].view(np.uint32).any() and not got["status"][N:].any()
    finally:
        mset.close()
        d.close()
        if fresh is not None:
            fresh.close()


def test_one_stream_without_a_wait_equals_the_synchronised_run(world, cast):
    import torch
    k, dirs, poses, rays, cen = inputs(128)
    mp, N = mover_poses(), len(dirs)
    scene = world.scenes["quantised"]
    got = loop_dev(scene, cast.mset, poses, dirs, mp, SHAPES, 3.0, stream=torch.cuda.Stream())
    # the same steps on the default stream with a synchronise after each
    pt, dt, mt = tensors(poses, dirs, mp)
    parts = []
    for f in range(2):
        hits, who, flow, status = outputs(N)
        cast.d.set(int(SHAPES[f, 0, 0]), int(SHAPES[f, 0, 1]), SHAPES[f, 0, 2])
        torch.cuda.synchronize()
        scene.scan_movers_dev(pt[f:f + 1], dt, hits, 3.0, cast.mset, mt[f:f + 1], mover_t=who)
        torch.cuda.synchronize()
        snap = cast.d.snapshot()
        torch.cuda.synchronize()
        cast.d.set(int(SHAPES[f + 1, 0, 0]), int(SHAPES[f + 1, 0, 1]), SHAPES[f + 1, 0, 2])
        torch.cuda.synchronize()
        scene.scan_nonrigid_flow_dev(hits, who, 1, N, 3.0, cast.mset, mt[f:f + 1], mt[f + 1:f + 2], pt[f + 1:f + 2], flow,
                                     pairs=[(0, snap, None)], status_t=status)
        parts.append(read(hits, who, flow, status))
    for c in ("t", "point3", "prim", "mover", "flow3", "status"):
        assert_same_bytes(got[c][:2 * N], np.concatenate([p[c] for p in parts]), f"own stream: {c}")
    assert (got["flow3"][:2 * N] != 0).any() and not got["status"][2 * N:].any()


# ---- 4: frames ---------------------------------------------------------------------------------------------------------------------

def test_scan_deforming_flow_frames(engine, world):
    from lidarcast import deform, synth
    from lidarcast.movers import MoverSet
    FRAMES = ("point3", "sem", "ins", "index", "range_origin")
    k, dirs, poses, rays, cen = inputs(100)
    mp, N = mover_poses(), len(dirs)
    walker = synth.make_walker(instance=1001)
    d = deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
    mset = MoverSet(engine.ctx, [d, world.meshes[0]])
    try:
        fr = deform.scan_deforming_flow_frames(engine, k, poses, world.room, mset, mp, SHAPES, want=FRAMES)
        plain = deform.scan_deforming_frames(engine, k, poses, world.room, mset, mp, SHAPES, want=FRAMES)
        dev = loop_dev(engine.scene_for(world.room), mset, poses, dirs, mp, SHAPES, k.max_range)
        small = deform.scan_deforming_flow_frames(engine, k, poses, world.room, mset, mp, SHAPES, want=("point3",))
    finally:
        mset.close()
        d.close()
    assert fr["total"] == plain["total"] and fr["counts"].tolist() == plain["counts"].tolist()
    for a in FRAMES + ("mover",):
        assert_same_bytes(fr[a], plain[a], f"frames: {a}")
    row = np.repeat(np.arange(3) * N, fr["counts"]) + fr["index"]
    assert (dev["t"][row] < np.inf).all() and len(row) == int((dev["t"] < np.inf).sum())
    assert_bit_equal(fr["flow"], dev["flow3"][row], "frames: flow")
    assert fr["flow_status"].dtype == np.uint8 and fr["flow_status"].tolist() == dev["status"][row].tolist()
    last = int(fr["counts"][:2].sum())
    assert not fr["flow_status"][last:].any() and (fr["flow_status"][:last] != 0).all() and (fr["flow"][:last] != 0).any()
    assert "index" not in small
    assert_bit_equal(small["flow"], fr["flow"], "frames without index: flow")


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(world, cast):
    import torch
    from lidarcast import DeviceHits, _capi
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    k, dirs, poses, rays, cen = inputs(100)
    P, N = 1, len(dirs)
    scene, mset, mp = world.scenes["quantised"], cast.mset, mover_poses()
    pt, dt, mt = tensors(poses, dirs, mp)
    hits, who, flow, status = outputs(N)
    cast.d.set(0, 0, 0.0)
    scene.scan_movers_dev(pt[:1], dt, hits, 3.0, mset, mt[:1], mover_t=who)
    snap = cast.d.snapshot()
    torch.cuda.synchronize()
    flow.fill_(7.0)
    status.fill_(255)
    Pair = _capi.LrcSurfacePair
    good = [Pair(0, snap.data_ptr(), None)]

    def call(s=scene._h, h=mset._h, rec=hits, w=who, a=mt[:1], b=mt[1:2], n=pt[1:2], f=flow, pairs=good, num=None):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        table = None if pairs is None else C.cast((Pair * max(len(pairs), 1))(*pairs), C.c_void_p)
        return lib.lrc_scan_nonrigid_flow_dev(s, h, C.byref(rec.struct), p(w), P, N, p(a), p(b), p(n), None, 20.0, table,
                                              len(pairs or []) if num is None else num, p(f), p(status), None)
    cases = [(dict(f=None), b"flow3 is NULL"), (dict(w=None), b"mover column is NULL"), (dict(n=None), b"next_poses16 is NULL"),
             (dict(a=None), b"mover_poses12"), (dict(b=None), b"next_mover_poses12"), (dict(s=None), b"NULL scene"),
             (dict(rec=DeviceHits(N, "cuda", want=("t", "point3"))), b"t, point3 and prim"),
             (dict(rec=DeviceHits(N, "cuda", want=("t", "prim"))), b"t, point3 and prim"),
             (dict(pairs=good * 17), b"at most 16"), (dict(pairs=None, num=1), b"pairs is NULL"),
             (dict(pairs=[Pair(2, snap.data_ptr(), None)]), b"names mover 2 of 2"),
             (dict(pairs=[Pair(1, snap.data_ptr(), None)]), b"not a deformable's scene"),
             (dict(pairs=good * 2), b"listed twice"), (dict(pairs=[Pair(0, None, snap.data_ptr())]), b"verts_a3 is NULL"),
             (dict(h=None), b"names mover 0 of 0")]
    for kw, text in cases:
        assert call(**kw) == E and text in lib.lrc_last_error(), (kw.keys(), lib.lrc_last_error())
    torch.cuda.synchronize()
    assert (flow == 7.0).all() and (status == 255).all()                 # nothing was launched
    assert lib.lrc_deform_snapshot_dev(cast.d._h, None, None) == E and lib.lrc_deform_snapshot_dev(None, C.c_void_p(snap.data_ptr()), None) == E
    assert call() == 0
    torch.cuda.synchronize()
    assert not (status == 255).any()
    with pytest.raises(ValueError, match="t, point3 and prim"):
        from lidarcast import deform
        deform.scan_deforming_flow_dev(scene, pt, dt, DeviceHits(3 * N, "cuda", want=("t", "point3")), 3.0, mset, mt, SHAPES,
                                       torch.zeros((3 * N, 3), device="cuda"))
    with pytest.raises(ValueError, match=r"be \(V, 3\)"):
        scene.scan_nonrigid_flow_dev(hits, who, 1, N, 3.0, mset, mt[:1], mt[1:2], pt[1:2], flow, pairs=[(0, snap[:5], None)])
    with pytest.raises(ValueError, match="out_t must be"):
        cast.d.snapshot(torch.zeros(5, device="cuda"))


# ---- 6: the simulator end to end ---------------------------------------------------------------------------------------------------

def test_simulator_nonrigid_flow_entry(world, tmp_path):
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 4, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"period": 0.1, "objects": [
        {"mesh": "walker", "semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.3, 3.3, 1.4, 0.0, 140.0]],
         "animation": {"cycle": 0.8}},
        {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]}]}
    plain = _sim(dict(base, movers=key), world.room).run_simulation(wps)
    one = _sim(dict(base, movers=dict(key, nonrigid_flow=True)), world.room).run_simulation(wps)
    assert one.get_total_frames() == 4
    seen, rows, swing = np.zeros(4, np.int64), 0, 0
    for f, (a, b) in enumerate(zip(one.frames, plain.frames)):
        assert not hasattr(b, "flow") and not hasattr(b, "flow_status")
        assert_bit_equal(a.points, b.points, f"frame {f}: points")
        assert a.mover_ids.tolist() == b.mover_ids.tolist()
        assert a.flow.dtype == np.float32 and a.flow_status.dtype == np.uint8
        assert len(a.flow) == len(a.flow_status) == len(a.mover_ids) == len(a.points) > 0 and a.flow.shape[1] == 3
        if f == 3:
            assert not a.flow_status.any() and not a.flow.view(np.uint32).any()
            continue
        seen += np.bincount(a.flow_status, minlength=4)
        assert (a.flow_status != 0).all()
        walker = a.mover_ids == 1
        rows += int(walker.sum())
        swing += int((a.flow[walker][:, 2] != 0).sum())                    # a rigid step about z has none: the limbs swing
        assert not a.flow[~walker].view(np.uint32).any() and (a.flow[walker] != 0).any(axis=1).all()
    assert seen[1] > 0 and seen[0] == 0 and rows > 10 and swing > 0, (seen, rows, swing)
    out = one.export_scene_flow(tmp_path)
    disk = np.load(tmp_path / "room_scene_flow.npz")
    off = disk["frame_offsets"]
    for f, a in enumerate(one.frames):
        sl = slice(off[f], off[f + 1])
        assert_bit_equal(disk["flow"][sl], a.flow)
        assert disk["status"][sl].tolist() == a.flow_status.tolist()
    from lidarcast.deform import Clip
    assert disk["animated_movers"].tolist() == [0] and sorted(out) == sorted(disk.files)
    assert np.array_equal(disk["mover_shapes"][:, 0], Clip(8, 0.8).shapes3(np.arange(4) * 0.1))
    # a set without an animated mover: the bytes of flow: true
    rigid = {"period": 0.1, "objects": [dict(key["objects"][0], mesh="pedestrian"), key["objects"][1]]}
    del rigid["objects"][0]["animation"]
    a = _sim(dict(base, movers=dict(rigid, flow=True)), world.room).run_simulation(wps)
    b = _sim(dict(base, movers=dict(rigid, nonrigid_flow=True)), world.room).run_simulation(wps)
    for fa, fb in zip(a.frames, b.frames):
        assert_bit_equal(fa.flow, fb.flow)
        assert fa.flow_status.tolist() == fb.flow_status.tolist()
    with pytest.raises(ValueError, match="exclude each other"):
        _sim(dict(base, movers=dict(key, nonrigid_flow=True, flow=True)), world.room).run_simulation(wps)
