"""CPU: the host side of the animated movers under sweeps (lidarcast.deform span_vertices / span_refit).
lrc_span_vertices and lrc_deform_span_refit run the inline functions the kernels call, so what is checked here bit for bit is the
kernels' arithmetic:

  span_vertices  against the numpy restatement (tests/span_restate.py) on random values, signed zeros, equal bits, denormals and
                 s in {0, 1, 2^-24, 1 - 2^-24} and a few between
  span_refit     on trees this file's neighbours write in the documented node layout: every child box is the exact min / max,
                 in the builders' total order, over BOTH shapes' vertices below it; references are untouched; the empty leaf's
                 inverted box is kept
  containment    for 1000 fractions every blended triangle's vertex box lies inside its slot's span box, compared exactly
  the physical sanity of the definition: the sweep composition over the CPU oracle with the walker cast per firing fraction on
                 a fresh mesh of the blended vertices; every return of the walker lies on triangle ``prim`` of the shape and
                 pose at its own s (float64 witness).
  the simulator's ``per_ray_shape`` entry with its refusals, and the tracks file's end shapes.

Measured with the oracle on the inputs below (N = 200, three sweeps): 127 of the 600 rays end on the walker; by the shape and pose
at their own time they lie within 2.748e-7 m of their triangle (recorded as 2.75e-7 m; bound 4 x that = 1.1e-6 m); by the shape
frozen at the sweep's start the farthest lies 0.078 m off its triangle."""
import json

import numpy as np
import pytest

import mover_restate as mv
import mover_sweep_restate as ms
import span_restate as sp
import sweep_restate
from deform_restate import leaf_ref, set_refs, slot_boxes_restate, tmax, tmin
from helpers import aimed_pose, assert_bit_equal, beam_table, bits
from test_deform_host import chain_tree, median_tree
from test_movers_host import oracle_cast, sim_with

from lidarcast import deform, synth

F = np.float32
FRACTIONS = [0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5, 0.3, 0.999]

MEASURED_ON_WALKER = 2.75e-7          # metres: the largest distance of the host composition over the oracle, measured here
BOUND_ON_WALKER = 4.0 * MEASURED_ON_WALKER      # a factor 4 for the spread between scenes


# ---- span_vertices -------------------------------------------------------------------------------------------------------------

def vertex_inputs():
    rng = np.random.default_rng(17)
    a = rng.uniform(-3, 3, (96, 3)).astype(F)
    b = rng.uniform(-3, 3, (96, 3)).astype(F)
    b[:8] = a[:8]                                                # equal bits
    a[8], b[8] = [0.0, -0.0, 0.0], [-0.0, 0.0, 0.0]              # signed zeros against each other
    a[9], b[9] = [-0.0, -0.0, 0.0], [-0.0, 1.0, -1.0]            # ... and against themselves
    a[10], b[10] = [1e6, -1e6, 1e-30], [-1e6, 1e6, -1e-30]
    a[11], b[11] = [1.0, 1.0 + 2.0 ** -23, 0.1], [1.0 + 2.0 ** -23, 1.0, np.nextafter(F(0.1), F(1))]      # neighbours
    den = np.array([1, 2, 3, 0x7FFFFF, 0x400000, 5], np.uint32).view(F)                                      # denormals
    a[12], b[12] = den[:3], den[3:]
    a[13], b[13] = -den[:3], den[3:]
    a[14], b[14] = den[3:], [0.0, -0.0, 1e-38]
    return a, b


@pytest.mark.parametrize("s", FRACTIONS)
def test_span_vertices_equal_the_restatement_bit_for_bit(s):
    a, b = vertex_inputs()
    got = deform.span_vertices(a, b, s)
    assert_bit_equal(got, sp.span_vertices_restate(a, b, s), f"span_vertices s={s}")
    assert (got >= np.minimum(a, b)).all() and (got <= np.maximum(a, b)).all()


def test_span_vertices_copies_are_bitwise():
    a, b = vertex_inputs()
    assert_bit_equal(deform.span_vertices(a, b, 0.0), a, "s == 0")
    assert_bit_equal(deform.span_vertices(a, b, 1.0), b, "s == 1")
    for s in FRACTIONS:
        assert_bit_equal(deform.span_vertices(a, a, s), a, f"a shape that does not change, s = {s}")
    assert bits(deform.span_vertices(a, a, 0.5))[9, 0] == 0x80000000          # -0 against -0 stays -0 (the blend would give +0)
    for s in (-2.0 ** -24, 1.0 + 2.0 ** -23, np.nan):
        with pytest.raises(ValueError, match="s must lie in"):
            deform.span_vertices(a, b, s)
    with pytest.raises(ValueError, match="same shape"):
        deform.span_vertices(a, b[:5], 0.5)


# ---- span_refit ----------------------------------------------------------------------------------------------------------------

def walker_ends():
    m = synth.make_walker()
    return deform.blend(m.keyframes[1], m.keyframes[2], 0.25), deform.blend(m.keyframes[2], m.keyframes[3], 0.25), \
        np.asarray(m.triangles, np.uint32)


def five_triangles():
    rng = np.random.default_rng(23)
    va = rng.uniform(-2, 2, (9, 3)).astype(F)
    vb = (va + rng.uniform(-0.3, 0.3, (9, 3))).astype(F)
    vb[2] = va[2]
    va[4, 0], vb[4, 0] = 0.0, -0.0
    return va, vb, rng.integers(0, 9, (5, 3)).astype(np.uint32)


@pytest.mark.parametrize("tree", ["median", "chain"])
@pytest.mark.parametrize("mesh", ["five", "walker"])
def test_span_refit_boxes_hold_both_shapes_exactly(mesh, tree):
    va, vb, tris = five_triangles() if mesh == "five" else walker_ends()
    if tree == "chain":
        tris = tris[:23]
        nodes, slot_prim = chain_tree(len(tris))
    else:
        nodes, slot_prim = median_tree(va, tris, np.random.default_rng(3))
    before = nodes.copy()
    out, box, rec = deform.span_refit(nodes, slot_prim, tris, va, vb)
    assert_bit_equal(nodes, before, "the input nodes are not written")
    assert_bit_equal(out[:, 12:], nodes[:, 12:], "references and padding")
    sp.check_span_invariant(out, before, slot_prim, tris, va, vb, f"{mesh}/{tree}")
    assert_bit_equal(box, sp.span_boxes_restate(slot_prim, tris, va, vb), "span boxes")
    assert_bit_equal(rec, np.concatenate([va[tris[slot_prim]].reshape(-1, 9), vb[tris[slot_prim]].reshape(-1, 9)], 1), "slot vertices")
    # the span box is the union of the two exact slot boxes
    ba, bb = slot_boxes_restate(slot_prim, tris, va), slot_boxes_restate(slot_prim, tris, vb)
    assert_bit_equal(box[:, :3], tmin(np.stack([ba[:, :3], bb[:, :3]]), 0), "lo = tmin(A, B)")
    assert_bit_equal(box[:, 3:], tmax(np.stack([ba[:, 3:], bb[:, 3:]]), 0), "hi = tmax(A, B)")


def test_span_refit_one_triangle_keeps_the_inverted_box_of_the_empty_leaf():
    va = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, -0.0]], F)
    vb = np.array([[0.1, -0.2, 0.0], [1.0, 0.0, 0.25], [0.0, 1.5, 0.0]], F)
    tris = np.array([[0, 1, 2]], np.uint32)
    node = np.full(16, 7.0, F)
    node[6:9], node[9:12], node[14:] = np.inf, -np.inf, 0.0            # the empty sibling: an inverted box
    set_refs(node, leaf_ref(0, 1), leaf_ref(0, 0))
    nodes = node[None]
    out, box, _ = deform.span_refit(nodes, np.zeros(1, np.uint32), tris, va, vb)
    sp.check_span_invariant(out, nodes, np.zeros(1, np.uint32), tris, va, vb, "one triangle")
    assert_bit_equal(out[0, 6:12], nodes[0, 6:12], "the empty leaf keeps its inverted box")
    assert_bit_equal(out[0, :6], box[0], "the leaf's box is its one slot's span box")
    assert bits(box)[0, 2] == 0x80000000 and box[0, 1] == F(-0.2) and box[0, 4] == 1.5


def test_span_refit_refusals():
    va, vb, tris = five_triangles()
    nodes, slot_prim = median_tree(va, tris, np.random.default_rng(3))
    bad = nodes.copy()
    set_refs(bad[0], np.int32(len(nodes)), bad[0, 13:14].view(np.int32)[0])
    with pytest.raises(ValueError, match="no tree"):
        deform.span_refit(bad, slot_prim, tris, va, vb)
    with pytest.raises(ValueError, match="triangle index"):
        deform.span_refit(nodes, slot_prim, tris, va[:3], vb[:3])
    with pytest.raises(ValueError, match="triangle row"):
        deform.span_refit(nodes, slot_prim, tris[:2], va, vb)
    with pytest.raises(ValueError, match="same shape"):
        deform.span_refit(nodes, slot_prim, tris, va, vb[:4])


# ---- containment ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh", ["five", "walker"])
def test_every_blended_triangle_lies_inside_its_span_box(mesh):
    """1000 fractions, the ends and their float32 neighbours among them; the compare is exact, in the builders' total order"""
    from deform_restate import enc
    va, vb, tris = five_triangles() if mesh == "five" else walker_ends()
    nodes, slot_prim = median_tree(va, tris, np.random.default_rng(3))
    _, box, _ = deform.span_refit(nodes, slot_prim, tris, va, vb)
    lo, hi = enc(box[:, :3]), enc(box[:, 3:])
    fr = np.random.default_rng(2).random(1000).astype(F)
    fr[:6] = [0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 2.0 ** -149, 0.5]
    for s in fr:
        now = slot_boxes_restate(slot_prim, tris, deform.span_vertices(va, vb, s))
        assert (enc(now[:, :3]) >= lo).all() and (enc(now[:, 3:]) <= hi).all(), f"s = {s}"


# ---- the scene the parity tests and the physical check share ----------------------------------------------------------------------

TARGET = (2.5, 2.0, 0.9)
WIDTH = {40: 10, 64: 16, 200: 50}          # four lines each: the shapes of tests/test_mover_sweeps_gpu.py
SWEEP_T = 0.1                               # seconds: one sweep of a 10 Hz sensor, and the period between sweeps
CLIP = dict(cycle=0.8, phase=0.03)          # one keyframe per sweep: every sweep crosses a keyframe boundary


def sweep_inputs(N, P):
    """tests/test_mover_sweeps_gpu.py's inputs: four lines x N / 4 columns about the sensor's -x axis, fire = column / width, P
    sweeps that look at TARGET from 1.5 m while the sensor moves 0.12 m and turns 0.05 rad"""
    from lidarcast import motion_records
    W = WIDTH[N]
    dirs = beam_table([18.0, 4.0, -10.0, -24.0], W, 40.0)
    fire = (np.arange(N) % W) / W
    yaws = (0.3, -1.0, 2.2)[:P]
    start = np.stack([aimed_pose(TARGET, 1.5, yaw=y) for y in yaws])
    end = start.copy()
    for p, y in enumerate(yaws):
        end[p] = aimed_pose(TARGET, 1.5, yaw=y + 0.05)
        end[p, :3, 3] = start[p, :3, 3] + (0.08, -0.09, 0.02)
    motion = motion_records(start, end)
    rays, cen = sweep_restate.sweep_rays(motion, dirs, fire)
    return dirs, fire, motion, rays, cen


WALKER_AT = ((2.79, 2.09, 0.9), (3.08, 1.37, 2.2), (2.32, 2.24, 3.5))       # x, y, yaw per sweep: in front of the sensor, chosen on the CPU


def walker_records(P):
    """the walker between the sensor and TARGET (where the room's furniture does not hide it), walking 0.12 m and turning 0.1
    rad per sweep"""
    return np.stack([ms.record24(x, y, 0.0, yaw, 0.1, 0.06, 0.0, 0.1) for x, y, yaw in WALKER_AT[:P]])[:, None, :]


BOX_AT = ((2.82, 1.63), (2.63, 0.96), (2.75, 2.43))          # the rigid box and the rig of the set of three, beside the walker
RIG_AT = ((2.46, 2.46), (3.39, 1.44), (2.08, 1.82))
RIG_PHASE = 0.4                                                # the rig's clip runs 0.4 cycles ahead of the walker's


def trio_records(P):
    """(P, 3, 24): the walker, a 12-triangle box crossing on one side of it, the rig walking and turning on the other"""
    out = np.zeros((P, 3, 24), F)
    out[:, 0] = walker_records(P)[:, 0]
    for p in range(P):
        out[p, 1] = ms.record24(BOX_AT[p][0], BOX_AT[p][1], 0.0, 0.2 + p, 0.3, 0.2, 0.0, 0.3)
        out[p, 2] = ms.record24(RIG_AT[p][0], RIG_AT[p][1], 0.0, 2.0 + p, -0.05, 0.08, 0.0, -0.2)
    return out


def triangle_keyframes():
    """a deformable of ONE triangle (the wrapped leaf with its empty sibling): two keyframes of a standing sheet"""
    a = np.array([[-0.4, -0.3, 0.3], [0.4, 0.3, 0.4], [0.0, 0.05, 1.5]], F)
    b = np.array([[-0.35, -0.2, 0.4], [0.45, 0.25, 0.3], [0.1, -0.05, 1.4]], F)
    return np.stack([a, b]), np.array([[0, 1, 2]], np.int32)


def clip_shapes(K, P, phase_shift=0.0):
    """(shapes_a, shapes_b), (P, 3) each: the clip at the start and at the end of every sweep"""
    clip = deform.Clip(K, CLIP["cycle"], phase=CLIP["phase"] + phase_shift)
    t = np.arange(P) * SWEEP_T
    return clip.shapes3(t), clip.shapes3(t + SWEEP_T)


def shape_vertices(keyframes, shape3):
    """the vertices Deformable.set(k0, k1, w) gives: a keyframe's own bits for w == 0, w == 1 and k0 == k1, else the blend"""
    k0, k1, w = int(shape3[0]), int(shape3[1]), F(shape3[2])
    if w == 0 or k0 == k1:
        return keyframes[k0].copy()
    if w == 1:
        return keyframes[k1].copy()
    return deform.blend(keyframes[k0], keyframes[k1], w)


def mesh_of(template, verts):
    return synth.TriangleMesh(vertices=np.asarray(verts, np.float64), triangles=np.asarray(template.triangles, np.int32),
                              triangle_sem=template.triangle_sem, triangle_ins=template.triangle_ins)


@pytest.fixture(scope="module")
def walking():
    """The walker under three sweeps, scanned by the host composition over the oracle: per ray shape, and frozen at A."""
    N, P = 200, 3
    walker = synth.make_walker(semantic=13, instance=1001)
    dirs, fire, motion, rays, cen = sweep_inputs(N, P)
    rec = walker_records(P)
    sa, sb = clip_shapes(len(walker.keyframes), P)
    ends = [(shape_vertices(walker.keyframes, sa[p]), shape_vertices(walker.keyframes, sb[p])) for p in range(P)]
    room = oracle_cast(mv.room_mesh())
    of = lambda v: oracle_cast(mesh_of(walker, v))
    out, win = sp.compose_sweeps(room, lambda p: [sp.fraction_cast(of, ends[p][0], ends[p][1], fire)], rays, cen, fire, rec, N, 20.0)
    frozen, _ = sp.compose_sweeps(room, lambda p: [of(ends[p][0])], rays, cen, fire, rec, N, 20.0)
    return {"N": N, "P": P, "walker": walker, "fire": fire, "rec": rec, "ends": ends, "out": out, "win": win, "frozen": frozen}


def test_walker_returns_lie_on_their_triangle_at_their_own_time(walking):
    w = walking
    N, tris = w["N"], np.asarray(w["walker"].triangles)
    own, off, hits = [], [], 0
    for p in range(w["P"]):
        sl = slice(p * N, (p + 1) * N)
        on = np.flatnonzero(w["out"]["mover"][sl] == 1)
        s = w["fire"][on].astype(F).astype(np.float64)
        pts, prim = w["out"]["point3"][sl][on], w["out"]["prim"][sl][on]
        va, vb = w["ends"][p]
        own.append(sp.triangle_distance(pts, prim, s, w["rec"][p, 0], tris, va, vb))
        off.append(sp.triangle_distance(pts, prim, s, w["rec"][p, 0], tris, va, va))
        hits += len(on)
        differs = (w["out"]["t"][sl] != w["frozen"]["t"][sl]) | (w["out"]["prim"][sl] != w["frozen"]["prim"][sl])
        assert len(on) >= 20 and (differs & (w["out"]["mover"][sl] == 1)).any(), f"sweep {p}"
        assert (w["out"]["ins"][sl][on] == 1001).all() and np.ptp(s) > 0.2        # the returns span a fifth of the sweep and more
    own, off = np.concatenate(own), np.concatenate(off)
    print(f"\n[span] host composition: {hits} of {w['P'] * N} rays end on the walker; by the shape and pose at their own time they "
          f"lie within {own.max():.3e} m of their triangle (bound {BOUND_ON_WALKER:.3e} m), by the shape frozen at the sweep's "
          f"start within {off.max():.4f} m")
    assert own.max() < 1e-4                       # otherwise the arithmetic is wrong, not the bound
    assert own.max() <= BOUND_ON_WALKER
    assert off.max() > 0.01                       # a swinging limb: the frozen shape cannot pass


# ---- the simulator key ---------------------------------------------------------------------------------------------------------

PATH = [[0.0, 1.8, 2.6, 0.0, 20.0], [0.4, 2.8, 1.8, 0.0, 100.0]]
WALKER = {"mesh": "walker", "semantic": 13, "instance": 1001, "path": PATH, "animation": {"cycle": 0.8, "phase": 0.25}}
RIG = {"mesh": "walker_rig", "semantic": 13, "instance": 1003, "path": [[0.0, 3.0, 2.0, 0.0, 0.0]], "animation": {"cycle": 0.8}}
RIGID = {"mesh": "pedestrian", "instance": 1002, "path": [[0.0, 3.0, 1.0, 0.0, 0.0]]}


def nested(**key):
    return {"motion": {"speed": 0.5, "movers": dict({"period": 0.1, "objects": [WALKER, RIGID, RIG]}, **key)}}


def test_simulator_per_ray_shape_key():
    plan = sim_with(nested(per_ray_shape=True))._mover_plan(nested=True)
    assert plan["per_ray_shape"] is True and [c is not None for c in plan["clips"]] == [True, False, True]
    assert plan["keyframes"][0].shape == (8, len(plan["meshes"][0].vertices), 3) and plan["keyframes"][2] is None
    assert plan["skins"][2] is not None and plan["skins"][0] is None
    rigid_only = {"motion": {"movers": {"objects": [RIGID], "per_ray_shape": True}}}
    assert sim_with(rigid_only)._mover_plan(nested=True)["clips"] == [None]


def test_simulator_per_ray_shape_refusals():
    old = "animation is not available under motion.movers: deformation within a sweep is not built"
    with pytest.raises(ValueError, match=old):
        sim_with(nested())._mover_plan(nested=True)
    with pytest.raises(ValueError, match=old):
        sim_with(nested(per_ray_shape=False))._mover_plan(nested=True)
    for bad in (1, "yes", None, 0):
        with pytest.raises(ValueError, match="motion.movers.per_ray_shape must be true or false"):
            sim_with(nested(per_ray_shape=bad))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.flow is not available"):
        sim_with(nested(per_ray_shape=True, flow=True))._mover_plan(nested=True)
    with pytest.raises(ValueError, match="motion.movers.nonrigid_flow is not available"):
        sim_with(nested(per_ray_shape=True, nonrigid_flow=True))._mover_plan(nested=True)
    cfg = nested(per_ray_shape=True)
    cfg["motion"]["noise"] = {"seed": 1}
    with pytest.raises(ValueError, match="motion.movers cannot be combined with motion.noise"):
        sim_with(cfg)._mover_plan(nested=True)
    for other, val in (("beam", {"divergence_mrad": 3.0}), ("materials", {"classes": {}})):
        with pytest.raises(ValueError, match=f"motion.movers cannot be combined with the {other} key"):
            sim_with(dict(nested(per_ray_shape=True), **{other: val}))._mover_plan(nested=True)
    with pytest.raises(ValueError, match=r"unknown entries under the movers key: \['per_ray_shape'\]"):
        sim_with({"movers": {"objects": [WALKER], "per_ray_shape": True}})._mover_plan()
    with pytest.raises(ValueError, match="mover 0: animation is"):
        sim_with({"motion": {"movers": {"per_ray_shape": True, "objects": [dict(WALKER, animation={"phase": 0.1})]}}})._mover_plan(nested=True)


def test_tracks_file_carries_the_end_shapes_and_joints(tmp_path):
    from containers import S3DISSimScene
    from lidarcast.movers import sweep_records
    plan = sim_with(nested(per_ray_shape=True))._mover_plan(nested=True)
    P, T = 2, 0.1
    times = np.arange(P) * plan["period"]
    rec = sweep_records(plan["tracks"], times, times + T)
    animated = [0, 2]
    scene = S3DISSimScene("fab")
    scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                          "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1), "poses12": rec[:, :, :12],
                          "end_states": np.stack([t.state(times + T) for t in plan["tracks"]], axis=1), "records24": rec,
                          "sweep_duration": T,
                          "shapes": {m: plan["clips"][m].shapes3(times) for m in animated},
                          "end_shapes": {m: plan["clips"][m].shapes3(times + T) for m in animated},
                          "keyframes": {0: plan["keyframes"][0]}, "skins": {2: plan["skins"][2]}}

    class Frame:
        def __init__(self, m):
            self.mover_ids = m
    scene.frames = [Frame(np.array([0, 1, 3], np.uint8)), Frame(np.array([2], np.uint8))]
    out = scene.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "fab_mover_tracks.json"))
    assert disk == json.loads(json.dumps(out))
    for f in range(P):
        walker, rigid, rig = disk["frames"][f]["movers"]
        assert "end_shape" not in rigid and "shape" not in rigid
        for m, who in ((0, walker), (2, rig)):
            k0, k1, w = plan["clips"][m].shape([times[f] + T])
            assert who["end_shape"] == [int(k0[0]), int(k1[0]), float(w[0])] and who["end_shape"] != who["shape"]
        assert "end_joints" not in walker and len(rig["end_joints"]) == len(rig["joints"]) == 6
        assert rig["end_joints"] != rig["joints"]
        # the rig stands still: its root joint moves only by what the clip lowers the body
        assert np.allclose(rig["end_joints"][0][:2], rig["joints"][0][:2])
