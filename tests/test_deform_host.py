"""CPU: the host side of the deforming movers (lidarcast.deform).  lrc_deform_blend and lrc_deform_refit
run the inline functions the kernels call, so what is checked here bit for bit is the kernels' arithmetic:

  blend   against a numpy float32 restatement (v = a + w * (b - a), clamped into [min, max] of a and b), on signed zeros, equal
          coordinates and w in {0, 2^-24, 0.5, 1 - 2^-24, 1}; the copies of w == 0 / w == 1 / a is b; the box property.
  refit   on trees this file writes itself in the documented node layout (a numpy median-split builder with leaves <= 4, the
          wrapped single leaf with its empty sibling, a degenerate chain): every child box equals the min / max, in the
          builders' total order (-0 below +0), over the vertices below it; records equal the restated v0, e1, e2, Ng;
          references are untouched; the empty leaf's box is still zero.
  Clip, make_walker, the simulator's `animation` key with its refusals, and the tracks file's shape field.
No tolerance anywhere."""
import json

import numpy as np
import pytest

from helpers import assert_bit_equal, bits

from deform_restate import (blend_restate, check_box_invariant, leaf_ref, records_restate, set_refs, slot_boxes_restate)

from lidarcast import deform, synth

F = np.float32
WS = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0]


# ---- blend -------------------------------------------------------------------------------------------------------------------

def blend_inputs():
    rng = np.random.default_rng(5)
    a = rng.uniform(-3, 3, (64, 3)).astype(F)
    b = rng.uniform(-3, 3, (64, 3)).astype(F)
    b[:8] = a[:8]                                   # equal coordinates
    a[8], b[8] = [0.0, -0.0, 0.0], [-0.0, 0.0, 0.0]  # signed zeros against each other
    a[9], b[9] = [-0.0, -0.0, 1.0], [1.0, -1.0, -0.0]
    a[10], b[10] = [1e6, -1e6, 1e-30], [-1e6, 1e6, -1e-30]
    a[11], b[11] = [1.0, 1.0 + 2.0 ** -23, 0.1], [1.0 + 2.0 ** -23, 1.0, np.nextafter(F(0.1), F(1))]   # neighbours
    return a, b


@pytest.mark.parametrize("w", WS)
def test_blend_equals_numpy_restatement(w):
    a, b = blend_inputs()
    got = deform.blend(a, b, w)
    assert_bit_equal(got, blend_restate(a, b, w), f"blend w={w}")
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert (got >= lo).all() and (got <= hi).all()          # inside the keyframes' box on every coordinate


def test_blend_copies_are_bitwise():
    a, b = blend_inputs()
    assert_bit_equal(deform.blend(a, b, 0.0), a, "w == 0")
    assert_bit_equal(deform.blend(a, b, 1.0), b, "w == 1")
    assert_bit_equal(deform.blend(a, a, 0.5), a, "equal keyframes")
    assert bits(deform.blend(a, b, 0.0))[8, 1] == 0x80000000          # the sign of a zero survives the copy


@pytest.mark.parametrize("w", [-2.0 ** -24, 1.0 + 2.0 ** -23, np.nan, np.inf])
def test_blend_refuses_w_outside_unit_interval(w):
    a, b = blend_inputs()
    with pytest.raises(ValueError, match="w must lie in"):
        deform.blend(a, b, w)


# ---- refit -------------------------------------------------------------------------------------------------------------------

def median_tree(verts, tris, rng):
    """A median-split tree over the triangles' centroids with leaves of <= 4 slots, nodes numbered in the order a depth-first
    walk makes them (children after parents).  Boxes are left as junk: refit must write every one."""
    cen = verts[tris].mean(1)
    nodes, slot_prim = [], []

    def build(ids):
        if len(ids) <= 4:
            first = len(slot_prim)
            slot_prim.extend(sorted(ids))
            return leaf_ref(first, len(ids))
        ax = int(np.argmax(np.ptp(cen[ids], 0)))
        ids = [ids[i] for i in np.argsort(cen[ids, ax], kind="stable")]
        me = len(nodes)
        nodes.append(rng.uniform(-9, 9, 16).astype(F))
        nodes[me][14:] = 0
        r0 = build(ids[:(len(ids) + 1) // 2])
        r1 = build(ids[(len(ids) + 1) // 2:])
        set_refs(nodes[me], r0, r1)
        return np.int32(me)

    root = build(list(range(len(tris))))
    assert root == 0
    return np.stack(nodes), np.array(slot_prim, np.uint32)


def wrapped_leaf(T):
    """The tree of a mesh of <= 4 triangles: node 0 holds the one leaf and an empty sibling with an all-zero box."""
    node = np.zeros(16, F)
    node[:6] = 7.0        # junk in the real child's box
    set_refs(node, leaf_ref(0, T), leaf_ref(0, 0))
    return node[None], np.arange(T, dtype=np.uint32)


def chain_tree(T):
    """A degenerate chain: node i holds the single-slot leaf i and node i + 1; the last node holds the last two slots.  The
    chain is written BOTTOM UP (node 0 is the root, its inner child is the LAST row, ...) so that parents do not precede their
    children in the array."""
    n = T - 1
    nodes = np.full((n, 16), 3.0, F)
    nodes[:, 14:] = 0
    order = [0] + list(range(n - 1, 0, -1))          # order[d] = row of the node at depth d
    for d, row in enumerate(order):
        if d == n - 1:
            set_refs(nodes[row], leaf_ref(d, 1), leaf_ref(d + 1, 1))
        else:
            set_refs(nodes[row], leaf_ref(d, 1), np.int32(order[d + 1]))
    return nodes, np.arange(T, dtype=np.uint32)


def mesh_case(name):
    rng = np.random.default_rng(11)
    if name == "walker":
        m = synth.make_walker()
        return m.keyframes[2].copy(), np.asarray(m.triangles, np.uint32)
    if name == "zeros":                  # a strip in the plane z = +-0 around the origin: signed zeros in every box
        n = 21
        v = np.zeros((2 * n, 3), F)
        v[:n, 0] = v[n:, 0] = np.linspace(-1, 1, n)
        v[n:, 1] = 1.0
        v[::2, 2] = -0.0
        v[n // 2, 0] = -0.0
        t = np.array([(i, i + 1, n + i) for i in range(n - 1)] + [(i + 1, n + i + 1, n + i) for i in range(n - 1)], np.uint32)
        return v, t
    v = rng.uniform(-2, 2, (40, 3)).astype(F)
    return v, rng.integers(0, 40, (57, 3)).astype(np.uint32)


@pytest.mark.parametrize("tree", ["median", "chain"])
@pytest.mark.parametrize("mesh", ["walker", "zeros", "random"])
def test_refit_boxes_records_and_refs(mesh, tree):
    verts, tris = mesh_case(mesh)
    if tree == "chain":
        tris = tris[:23]
        nodes, slot_prim = chain_tree(len(tris))
    else:
        nodes, slot_prim = median_tree(verts, tris, np.random.default_rng(3))
    out, rec, box = deform.refit(nodes, slot_prim, tris, verts)
    assert_bit_equal(out[:, 12:], nodes[:, 12:], "references and padding")
    check_box_invariant(out, slot_prim, tris, verts, f"{mesh}/{tree}")
    assert_bit_equal(rec, records_restate(slot_prim, tris, verts), "records")
    assert_bit_equal(box, slot_boxes_restate(slot_prim, tris, verts), "slot boxes")
    if mesh == "zeros":
        assert (bits(out[:, :12]) == 0x80000000).any()        # a -0 plane really occurs


@pytest.mark.parametrize("T", [1, 3, 4])
def test_refit_wrapped_single_leaf_keeps_the_empty_box(T):
    verts = np.random.default_rng(T).uniform(-1, 1, (6, 3)).astype(F)
    tris = np.random.default_rng(T + 9).integers(0, 6, (T, 3)).astype(np.uint32)
    nodes, slot_prim = wrapped_leaf(T)
    out, rec, box = deform.refit(nodes, slot_prim, tris, verts)
    assert_bit_equal(out[:, 12:], nodes[:, 12:], "references")
    assert not bits(out[0, 6:12]).any()
    check_box_invariant(out, slot_prim, tris, verts, "wrapped leaf")
    assert_bit_equal(rec, records_restate(slot_prim, tris, verts), "records")


def test_refit_refuses_what_is_no_tree():
    verts, tris = mesh_case("random")
    nodes, slot_prim = median_tree(verts, tris, np.random.default_rng(3))
    bad = nodes.copy()
    set_refs(bad[1], np.int32(len(nodes)), bad[1, 13:14].view(np.int32)[0])          # a reference past the nodes
    with pytest.raises(ValueError, match="no tree"):
        deform.refit(bad, slot_prim, tris, verts)
    bad = nodes.copy()
    set_refs(bad[1], np.int32(0), bad[1, 13:14].view(np.int32)[0])                   # a cycle
    with pytest.raises(ValueError, match="no tree"):
        deform.refit(bad, slot_prim, tris, verts)
    bad = nodes.copy()
    set_refs(bad[0], leaf_ref(len(slot_prim) - 1, 3), bad[0, 13:14].view(np.int32)[0])   # a leaf past the slots
    with pytest.raises(ValueError, match="no tree"):
        deform.refit(bad, slot_prim, tris, verts)
    with pytest.raises(ValueError, match="triangle index"):
        deform.refit(nodes, slot_prim, tris, verts[:5])
    with pytest.raises(ValueError, match="triangle row"):
        deform.refit(nodes, slot_prim, tris[:5], verts)


# ---- Clip --------------------------------------------------------------------------------------------------------------------

def test_clip_knots_wrap_and_ends():
    c = deform.Clip(4, cycle=2.0)
    k0, k1, w = c.shape([0.0, 0.5, 1.0, 1.5, 2.0, 1.75, 0.25, -0.25, 4.5])
    assert k0.dtype == np.uint32 and k1.dtype == np.uint32 and w.dtype == np.float32
    assert k0.tolist() == [0, 1, 2, 3, 0, 3, 0, 3, 1]
    assert k1.tolist() == [1, 2, 3, 0, 1, 0, 1, 0, 2]             # the last keyframe blends back into the first
    assert w.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.0]
    k0, k1, w = deform.Clip(4, cycle=2.0, phase=0.25).shape([0.0, 1.5])
    assert (k0.tolist(), k1.tolist(), w.tolist()) == ([1, 0], [2, 1], [0.0, 0.0])
    once = deform.Clip(4, cycle=2.0, loop=False)
    k0, k1, w = once.shape([-1.0, 0.0, 0.25, 1.5, 1.75, 9.0])
    assert k0.tolist() == [0, 0, 0, 3, 3, 3]
    assert k1.tolist() == [1, 1, 1, 3, 3, 3]                      # held at the last keyframe
    assert w.tolist() == [0.0, 0.0, 0.5, 0.0, 0.0, 0.0]
    # w is computed in float64 and narrowed last
    t = 0.3
    x = (t / 2.0) * 4
    assert deform.Clip(4, 2.0).shape(t)[2][0] == np.float32(x - np.floor(x))
    assert deform.Clip(4, 2.0).shapes3([0.25]).tolist() == [[0.0, 1.0, 0.5]]
    assert deform.Clip(1, 1.0).shape([0.3])[:2] == (np.array([0], np.uint32), np.array([0], np.uint32))
    with pytest.raises(ValueError):
        deform.Clip(0, 1.0)
    with pytest.raises(ValueError):
        deform.Clip(4, 0.0)


# ---- make_walker -------------------------------------------------------------------------------------------------------------

def test_walker_is_closed_with_constant_topology():
    m = synth.make_walker(height=1.7, keyframes=8, swing_deg=25)
    K, V, _ = m.keyframes.shape
    assert K == 8 and m.keyframes.dtype == np.float32 and V == len(m.vertices)
    assert 200 <= len(m.triangles) <= 600
    assert_bit_equal(m.vertices.astype(np.float32), m.keyframes[0], "keyframe 0 is the mesh")
    assert m.triangles.min() == 0 and m.triangles.max() == V - 1
    # closed and consistently wound: every directed edge occurs once and its reverse once
    t = np.asarray(m.triangles, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 0)
    key = e[:, 0] * V + e[:, 1]
    assert len(np.unique(key)) == len(key)
    assert np.array_equal(np.sort(key), np.sort(e[:, 1] * V + e[:, 0]))
    # wound outward: positive enclosed volume in every keyframe; feet on the floor; the limbs really move
    for k in range(K):
        v = m.keyframes[k].astype(np.float64)
        vol = np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0
        assert vol > 0.01
        # a leg of half the height swung by 25 degrees lifts its foot by at most 0.5 H (1 - cos 25 deg); the body sinks by that
        assert v[:, 2].min() == 0.0 and 0.0 <= float(np.float32(1.7)) - v[:, 2].max() <= 0.85 * (1 - np.cos(np.deg2rad(25))) + 1e-6
    assert np.abs(m.keyframes[2] - m.keyframes[0]).max() > 0.2
    assert np.abs(m.keyframes[2] - m.keyframes[6])[:, 0].max() > 0.4          # opposite sides in antiphase
    assert (m.triangle_sem == 13).all() and (m.triangle_ins == 1).all()


# ---- the simulator key ---------------------------------------------------------------------------------------------------------

def sim_with(config):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
    sim.config = config
    sim.scene = object()
    return sim


PATH = [[0.0, 1.8, 2.6, 0.0, 20.0], [0.2, 2.8, 1.8, 0.0, 100.0]]
WALKER = {"mesh": "walker", "semantic": 13, "instance": 1001, "path": PATH, "animation": {"cycle": 0.8, "phase": 0.25}}
RIGID = {"mesh": "pedestrian", "instance": 1002, "path": [[0.0, 3.0, 1.0, 0.0, 0.0]]}


def test_simulator_animation_key(tmp_path):
    plan = sim_with({"movers": {"period": 0.1, "objects": [WALKER, RIGID]}})._mover_plan()
    walker = synth.make_walker(semantic=13, instance=1001)
    clip = plan["clips"][0]
    assert plan["clips"][1] is None and plan["keyframes"][1] is None
    assert (clip.K, clip.cycle, clip.phase, clip.loop) == (8, 0.8, 0.25, True)
    assert_bit_equal(plan["keyframes"][0], walker.keyframes, "walker keyframes")
    assert plan["objects"][0]["animation"] == {"cycle": 0.8, "phase": 0.25, "loop": True, "num_keyframes": 8}
    assert "animation" not in plan["objects"][1]
    assert plan["objects"][0]["box_min"] == [float(x) for x in walker.keyframes.reshape(-1, 3).min(0)]      # all keyframes
    # a keyframes file serves the mesh file's own topology
    from lidarcast.ply import write_triangle_mesh
    cube = synth.unit_cube(-0.3, 0.3)
    ply, npy = str(tmp_path / "cube.ply"), str(tmp_path / "cube_keys.npy")
    write_triangle_mesh(ply, cube)
    keys = np.stack([cube.vertices, cube.vertices * 1.5]).astype(np.float32)
    np.save(npy, keys)
    obj = {"mesh": ply, "keyframes": npy, "path": PATH, "animation": {"cycle": 1.0, "loop": False}}
    plan = sim_with({"movers": {"objects": [obj]}})._mover_plan()
    assert_bit_equal(plan["keyframes"][0], keys, "keyframes file")
    assert (plan["clips"][0].K, plan["clips"][0].loop) == (2, False)
    np.save(npy, keys[:, :5])
    with pytest.raises(ValueError, match=r"keyframes must be \(K, V, 3\)"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()


def test_simulator_animation_refusals():
    with pytest.raises(ValueError, match="animation is not available under motion.movers"):
        sim_with({"motion": {"speed": 1.0, "movers": {"objects": [WALKER]}}})._mover_plan(nested=True)
    with pytest.raises(ValueError, match="flow is not available in a set with an animated mover"):
        sim_with({"movers": {"flow": True, "objects": [RIGID, WALKER]}})._mover_plan()
    assert sim_with({"movers": {"flow": True, "objects": [RIGID]}})._mover_plan()["flow"] is True      # untouched without one
    for bad, match in [({"cycle": 0.8, "speed": 2}, "animation is"), ({"phase": 0.1}, "animation is"), ({"cycle": 0.0}, "cycle"),
                       ({"cycle": 1.0, "loop": 1}, "loop must be")]:
        with pytest.raises(ValueError, match=match):
            sim_with({"movers": {"objects": [dict(WALKER, animation=bad)]}})._mover_plan()
    with pytest.raises(ValueError, match="needs mesh: walker or a keyframes file"):
        sim_with({"movers": {"objects": [dict(RIGID, animation={"cycle": 1.0})]}})._mover_plan()
    with pytest.raises(ValueError, match="keyframes need an animation"):
        sim_with({"movers": {"objects": [dict(RIGID, keyframes="x.npy")]}})._mover_plan()


def test_tracks_file_carries_the_shape_and_the_blended_box(tmp_path):
    from containers import S3DISSimScene
    plan = sim_with({"movers": {"period": 0.1, "objects": [WALKER, RIGID]}})._mover_plan()
    P = 3
    times = np.arange(P) * plan["period"]
    scene = S3DISSimScene("fab")
    scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                          "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1),
                          "poses12": np.stack([t.poses12(times) for t in plan["tracks"]], axis=1),
                          "shapes": {0: plan["clips"][0].shapes3(times)}, "keyframes": {0: plan["keyframes"][0]}}

    class Frame:
        mover_ids = np.array([0, 1, 1, 2], np.uint8)
    scene.frames = [Frame() for _ in range(P)]
    out = scene.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "fab_mover_tracks.json"))
    assert disk == json.loads(json.dumps(out))
    keys = plan["keyframes"][0]
    # x = (t / 0.8 + 0.25) * 8 = 2, 3, 4 at t = 0, 0.1, 0.2: exact knots
    assert [fr["movers"][0]["shape"] for fr in disk["frames"]] == [[2, 3, 0.0], [3, 4, 0.0], [4, 5, 0.0]]
    assert all("shape" not in fr["movers"][1] for fr in disk["frames"])
    for f, fr in enumerate(disk["frames"]):
        k0, k1, w = fr["movers"][0]["shape"]
        v = deform.blend(keys[k0], keys[k1], w).astype(np.float64)
        assert fr["movers"][0]["box7"][3:6] == [float(x) for x in (v.max(0) - v.min(0))]
        assert fr["movers"][1]["box7"][3:6] == [0.5, 0.5, 1.7]
    assert disk["frames"][0]["movers"][0]["box7"][3] > disk["frames"][2]["movers"][0]["box7"][3]      # the stride closes again
