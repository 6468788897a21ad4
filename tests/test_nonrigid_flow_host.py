"""CPU: the host side of the non-rigid scene flow (lrc_nonrigid_flow_rays, lidarcast.flow.nonrigid_rays, the simulator key).
The host function runs the inline functions the kernel calls and is compared bit for bit with the numpy restatement of the
header's text (tests/nonrigid_flow_restate.py).

The rows lie on the triangles of shape A: float32 roundings of random barycentric points, of the three vertices and of the three
edge midpoints of every triangle, taken to the world by pose A in float64.  Mover 0 is the deformable with a surface pair, mover 1
a rigid mover without one; rows of the room, rows without a return, rows with prim >= T and rows of mover 1 are mixed in.

The geometric bound: |distance of y from the plane of the NEXT shape's triangle at pose B|, float64, must stay below a quarter of
the status margin, 2^-12 max(L, 1) / 4 >= 6.1e-5 m, on every row.  Expected from the arithmetic: the float32 point lies within
half an ulp of its coordinates off the plane of shape A (3e-7 m at 5 m), and the interpolated displacement carries that residual
to the next plane turned by at most the angle between the two triangles; measured below, printed per mesh."""
import numpy as np
import pytest

import flow_restate as fl
import nonrigid_flow_restate as nr
from test_deform_gpu import case as deform_case
from test_flow_host import COLUMNS, assert_same, general_pose, sensor_pose
from test_movers_host import KEY, sim_with

F32, F64 = np.float32, np.float64
MESHES = ("walker", "cube", "tetra")
REACH = 50.0


def to_world(p, pose12):
    m = np.asarray(pose12, F64).reshape(3, 4)
    return p @ m[:, :3].T + m[:, 3]


def rows_on(va, tris, rng, per=3):
    """(object-frame float64 points on the triangles of va, their triangle rows): per random interior points, the three
    vertices and the three edge midpoints of every triangle."""
    a = va.astype(F64)[tris]                                   # (T, 3, 3)
    T = len(tris)
    bary = [rng.dirichlet([1.0, 1.0, 1.0], T) for _ in range(per)]
    bary += [np.tile(b, (T, 1)) for b in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5])]
    pts = np.concatenate([np.einsum("tk,tkc->tc", np.asarray(b, F64), a) for b in bary])
    return pts, np.tile(np.arange(T), len(bary))


class Setup:
    pass


def make(name, shape_a, shape_b, same_pose=False, seed=5):
    """One frame of rows on mesh ``name`` between two shapes ((k0, k1, w) each), M = 2, the pair on mover 0."""
    from lidarcast import deform
    keys, tris, _, _, _ = deform_case(name)
    tris = np.asarray(tris, np.uint32)
    rng = np.random.default_rng(seed)
    s = Setup()
    s.va = deform.blend(keys[shape_a[0]], keys[shape_a[1]], shape_a[2])
    s.vb = deform.blend(keys[shape_b[0]], keys[shape_b[1]], shape_b[2])
    s.tris = tris
    s.A = np.stack([general_pose(rng), general_pose(rng)]).reshape(1, 2, 12)
    s.B = s.A.copy() if same_pose else np.stack([general_pose(rng), general_pose(rng)]).reshape(1, 2, 12)
    pts, prim = rows_on(s.va, tris, rng)
    s.on = len(pts)                                            # rows [0, on): mover 1 (w = 1), on their triangle
    x = to_world(pts, s.A[0, 0]).astype(F32)
    extra = 40                                                 # then: the room, mover 2 (no pair), prim >= T, no return
    xe = rng.uniform(-5, 5, (4 * extra, 3)).astype(F32)
    s.x = np.concatenate([x, xe])
    s.w = np.concatenate([np.ones(s.on), np.zeros(extra), np.full(extra, 2), np.ones(extra), np.ones(extra)]).astype(np.uint8)
    T = len(tris)
    s.prim = np.concatenate([prim, rng.integers(0, T, 2 * extra), np.array([T, T + 1, 0xFFFFFFFF, 2 ** 31] * (extra // 4)),
                             rng.integers(0, T, extra)]).astype(np.uint32)
    s.t = np.ones(len(s.x), F32)
    s.t[-extra:] = np.inf
    s.N = len(s.x)
    s.nxt = sensor_pose(rng)[None]
    s.pairs = [(0, s.va, s.vb, tris)]
    return s


def both(s, pairs=None, has=None):
    from lidarcast import flow
    pairs = s.pairs if pairs is None else pairs
    want = nr.rays(s.t, s.x, s.w, s.prim, s.A, s.B, s.nxt, has, s.N, REACH, pairs)
    got = flow.nonrigid_rays(s.t, s.x, s.w, s.prim, s.A, s.B, s.nxt, has, REACH, pairs)
    return got, want


SHAPES = {"walker": ((0, 1, 0.37), (2, 3, 0.8)), "cube": ((0, 1, 0.37), (1, 2, 0.5)), "tetra": ((0, 1, 0.37), (1, 2, 0.5))}


@pytest.mark.parametrize("name", MESHES)
def test_host_function_equals_the_restatement(name):
    s = make(name, *SHAPES[name])
    assert (name != "walker") or len(s.tris) == 384
    got, want = both(s)
    for c in COLUMNS:
        assert_same(got[c], want[c], f"{name}: {c}")
    assert want["paired"][:s.on].all() and not want["paired"][s.on:].any()
    assert (want["flow3"][:s.on] != 0).any(axis=1).all() and np.isfinite(want["flow3"]).all()
    assert (want["status"][:s.on] == fl.VISIBLE).all() and (want["status"][-40:] == fl.NONE).all()
    # rows without a pair (the room, mover 2, prim >= T, no return) take the rigid bytes
    from lidarcast import flow
    rigid = flow.rays(s.t, s.x, s.w, s.A, s.B, s.nxt, None, REACH)
    for c in COLUMNS:
        assert_same(got[c][s.on:], rigid[c][s.on:], f"{name}: rows without a pair: {c}")
    assert (rigid["flow3"][s.on + 40:s.on + 120] != 0).any()                 # ... which moved: mover 2 and mover 1 with prim >= T
    assert not np.array_equal(got["flow3"][:s.on], rigid["flow3"][:s.on])
    # has_next == 0: nothing flows
    got0, want0 = both(s, has=np.zeros(1, np.uint8))
    for c in COLUMNS:
        assert_same(got0[c], want0[c], f"{name}, no next: {c}")
    assert not got0["flow3"].view(np.uint32).any() and not got0["status"].any()


@pytest.mark.parametrize("name", MESHES)
def test_the_target_lies_on_the_next_triangle(name):
    """The geometric check of the module docstring."""
    s = make(name, *SHAPES[name])
    _, want = both(s)
    idx = s.tris[s.prim[:s.on]].astype(np.int64)
    b = to_world(s.vb.astype(F64)[idx].reshape(-1, 3), s.B[0, 0]).reshape(-1, 3, 3)
    nrm = np.cross(b[:, 1] - b[:, 0], b[:, 2] - b[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    assert (area > 0).all()
    off = np.abs(np.einsum("nc,nc->n", nrm / area[:, None], want["y"][:s.on] - b[:, 0]))
    bound = (2.0 ** -12) * np.maximum(want["L"][:s.on].astype(F64), 1.0) / 4.0
    print(f"\n[nonrigid] {name}: max distance from the next plane {off.max():.3e} m, smallest bound {bound.min():.3e} m, "
          f"largest ratio {np.max(off / bound):.3e}")
    assert (want["keep"][:s.on] == 1).all()
    assert (off < bound).all(), (off.max(), bound.min())


@pytest.mark.parametrize("name", MESHES)
def test_equal_shapes_give_the_rigid_bytes(name):
    from lidarcast import flow
    s = make(name, SHAPES[name][0], SHAPES[name][0])
    assert np.array_equal(s.va.view(np.uint32), s.vb.view(np.uint32))
    got, want = both(s)
    rigid = flow.rays(s.t, s.x, s.w, s.A, s.B, s.nxt, None, REACH)
    for c in COLUMNS:
        assert_same(got[c], rigid[c], f"{name}, VA == VB: {c}")
        assert_same(got[c], want[c], f"{name}, VA == VB, restatement: {c}")
    assert want["paired"][:s.on].all() and (got["flow3"][:s.on] != 0).any(axis=1).all()


@pytest.mark.parametrize("name", MESHES)
def test_equal_poses_and_equal_shapes_give_zero_bits(name):
    s = make(name, SHAPES[name][0], SHAPES[name][0], same_pose=True)
    got, want = both(s)
    assert not got["flow3"].view(np.uint32).any() and not want["flow3"].view(np.uint32).any()
    assert_same(got["status"], want["status"], name)


def test_equal_poses_with_different_shapes_on_the_walker():
    """Keyframes 1 and 7 mirror the limbs and leave torso and head where they are: those 128 triangles keep their bits; of the
    256 limb triangles 200 move in every vertex (a vertex on a pivot axis may keep its place)."""
    s = make("walker", (1, 1, 0.0), (7, 7, 0.0), same_pose=True)
    got, want = both(s)
    for c in COLUMNS:
        assert_same(got[c], want[c], f"walker 1 -> 7: {c}")
    moves = (s.va.view(np.uint32) != s.vb.view(np.uint32)).any(axis=1)[s.tris.astype(np.int64)]       # (T, 3)
    limb, still = moves.all(axis=1), ~moves.any(axis=1)
    assert limb.sum() == 200 and still.sum() == 128
    row = s.prim[:s.on].astype(np.int64)
    flow3 = got["flow3"][:s.on]
    assert (flow3[limb[row]] != 0).any(axis=1).all()
    assert not flow3[still[row]].view(np.uint32).any()
    assert not got["flow3"][s.on:].view(np.uint32).any()            # every other row stands still as well


def test_a_triangle_without_area_takes_its_first_vertex():
    from lidarcast import flow
    rng = np.random.default_rng(3)
    va = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0, 0], [0.5, 1, 0]], F32)          # 0-1-2 collinear, 1-3-? doubled
    tris = np.array([[0, 1, 2], [1, 3, 4], [1, 1, 1], [0, 1, 4]], np.uint32)
    vb = va + rng.uniform(0.1, 0.3, va.shape).astype(F32)
    A = np.stack([general_pose(rng)]).reshape(1, 1, 12)
    B = np.stack([general_pose(rng)]).reshape(1, 1, 12)
    obj = np.array([[0.7, 0, 0], [1, 0, 0], [1, 0, 0], [0.4, 0.3, 0]], F64)
    x = to_world(obj, A[0, 0]).astype(F32)
    t, w, prim = np.ones(4, F32), np.ones(4, np.uint8), np.arange(4, dtype=np.uint32)
    nxt = sensor_pose(rng)[None]
    pairs = [(0, va, vb, tris)]
    want = nr.rays(t, x, w, prim, A, B, nxt, None, 4, REACH, pairs)
    got = flow.nonrigid_rays(t, x, w, prim, A, B, nxt, None, REACH, pairs)
    for c in COLUMNS:
        assert_same(got[c], want[c], f"degenerate: {c}")
    assert np.isfinite(got["flow3"]).all() and np.isfinite(got["rays6"]).all()
    # u = v = 0: z = q + D0, so y is the rigid target of q + D0
    q = nr.rest(x[:3], np.repeat(A[0], 3, 0))
    D0 = vb.astype(F64)[tris[:3, 0]] - va.astype(F64)[tris[:3, 0]]
    y = nr.world(q + ((1.0 * D0 + 0.0 * D0) + 0.0 * D0), np.repeat(B[0], 3, 0))
    assert np.array_equal(want["y"][:3], y)
    s, u, v = nr.barycentric(nr.rest(x[3:], A[0]), va.astype(F64)[tris[3:]])
    assert u[0] > 0.1 and v[0] > 0.1                                # the fourth triangle has area: real coordinates


def test_refusals_of_the_host_function():
    from lidarcast import flow
    s = make("tetra", *SHAPES["tetra"])
    pair = s.pairs[0]
    call = lambda pairs: flow.nonrigid_rays(s.t, s.x, s.w, s.prim, s.A, s.B, s.nxt, None, REACH, pairs)
    with pytest.raises(ValueError, match="at most 16"):
        call([pair] * 17)
    with pytest.raises(ValueError, match="listed twice"):
        call([pair, pair])
    with pytest.raises(ValueError, match="names mover 2 of 2"):
        call([(2,) + pair[1:]])
    with pytest.raises(ValueError, match="triangle index out of range"):
        call([(0, s.va, s.vb, s.tris + 2)])
    with pytest.raises(ValueError, match="same shape"):
        call([(0, s.va, s.vb[:3], s.tris)])
    none = call([])                                                   # no pairs: lrc_flow_rays
    rigid = flow.rays(s.t, s.x, s.w, s.A, s.B, s.nxt, None, REACH)
    for c in COLUMNS:
        assert_same(none[c], rigid[c], f"no pairs: {c}")


def test_three_frames_paired_by_a_clip():
    """Clip.shapes3 gives the shapes of three frames; frame k flows from shape k to shape k + 1 and the last frame has no next.
    The walker's rows of each frame lie on that frame's shape."""
    from lidarcast import deform, flow, synth
    walker = synth.make_walker()
    keys, tris = walker.keyframes, np.asarray(walker.triangles, np.uint32)
    shapes = deform.Clip(len(keys), cycle=1.0, phase=0.05).shapes3(np.arange(3) * 0.125)
    assert shapes[:, :2].astype(int).tolist() == [[0, 1], [1, 2], [2, 3]] and (shapes[:, 2] > 0).all()
    verts = [deform.blend(keys[int(a)], keys[int(b)], c) for a, b, c in shapes]
    rng = np.random.default_rng(9)
    mp = np.stack([general_pose(rng) for _ in range(3)]).reshape(3, 1, 12)
    poses = np.stack([sensor_pose(rng) for _ in range(3)])
    nxt, nmp, has = fl.pair_next(poses, mp)
    flows = []
    for k in range(3):
        pts, prim = rows_on(verts[k], tris, rng, per=1)
        x = to_world(pts, mp[k, 0]).astype(F32)
        n = len(x)
        pairs = [(0, verts[k], verts[min(k + 1, 2)], tris)]
        args = (np.ones(n, F32), x, np.ones(n, np.uint8), prim.astype(np.uint32), mp[k:k + 1], nmp[k:k + 1], nxt[k:k + 1], has[k:k + 1])
        want = nr.rays(*args, n, REACH, pairs)
        got = flow.nonrigid_rays(*args, REACH, pairs)
        for c in COLUMNS:
            assert_same(got[c], want[c], f"frame {k}: {c}")
        flows.append(got)
    assert all((f["flow3"] != 0).any(axis=1).all() and (f["status"] == fl.VISIBLE).all() for f in flows[:2])
    assert not flows[2]["flow3"].view(np.uint32).any() and not flows[2]["status"].any()


# ---- the simulator key ---------------------------------------------------------------------------------------------------------

WALKER = {"mesh": "walker", "semantic": 13, "instance": 1003, "path": [[0.0, 2.0, 2.0, 0.0, 0.0], [0.3, 3.0, 2.0, 0.0, 0.0]],
          "animation": {"cycle": 0.8}}


def test_simulator_key_and_its_refusals():
    mixed = dict(KEY, objects=KEY["objects"] + [WALKER])
    assert sim_with({"movers": KEY})._mover_plan()["nonrigid_flow"] is False
    plan = sim_with({"movers": dict(mixed, nonrigid_flow=True)})._mover_plan()
    assert plan["nonrigid_flow"] is True and plan["flow"] is False and [c is not None for c in plan["clips"]] == [False, False, True]
    assert sim_with({"movers": dict(KEY, nonrigid_flow=True)})._mover_plan()["nonrigid_flow"] is True      # no animated mover: allowed
    with pytest.raises(ValueError, match="movers.nonrigid_flow must be true or false"):
        sim_with({"movers": dict(mixed, nonrigid_flow=1)})._mover_plan()
    with pytest.raises(ValueError, match="exclude each other"):
        sim_with({"movers": dict(KEY, nonrigid_flow=True, flow=True)})._mover_plan()
    with pytest.raises(ValueError, match="motion.movers.nonrigid_flow is not available"):
        sim_with({"motion": {"speed": 0.5, "movers": dict(KEY, nonrigid_flow=True)}})._mover_plan(nested=True)
    with pytest.raises(ValueError, match="at most 16 animated movers"):
        sim_with({"movers": dict(KEY, nonrigid_flow=True, objects=[WALKER] * 17)})._mover_plan()
    assert len(sim_with({"movers": dict(KEY, objects=[WALKER] * 17)})._mover_plan()["clips"]) == 17        # without the key: as before
    # the present refusal stands
    with pytest.raises(ValueError, match="movers.flow is not available in a set with an animated mover"):
        sim_with({"movers": dict(mixed, flow=True)})._mover_plan()


def test_scene_flow_file_carries_the_shapes(tmp_path):
    from containers import S3DISSimScene
    scene = S3DISSimScene("fab")
    P = 3
    shapes = np.array([[0, 1, 0.25], [1, 2, 0.5], [2, 3, 0.75]])
    scene.mover_tracks = {"period": 0.1, "objects": [], "times": np.arange(P) * 0.1, "states": np.zeros((P, 2, 4)),
                          "poses12": np.zeros((P, 2, 12), F32), "sensor_poses": np.tile(np.eye(4), (P, 1, 1)),
                          "shapes": {1: shapes}, "keyframes": {1: np.zeros((4, 5, 3), F32)}}

    class Frame:
        points = np.ones((2, 3), F32)
        mover_ids = np.array([0, 2], np.uint8)
        flow = np.full((2, 3), 0.5, F32)
        flow_status = np.array([1, 2], np.uint8)
    scene.frames = [Frame(), Frame(), Frame()]
    out = scene.export_scene_flow(tmp_path)
    disk = np.load(tmp_path / "fab_scene_flow.npz")
    assert sorted(disk.files) == sorted(out)
    assert disk["animated_movers"].tolist() == [1] and np.array_equal(disk["mover_shapes"], shapes[:, None, :])
