"""-m gpu: animated movers under sweeps (lrc_deform_span_dev, the per-ray-shape cast of lrc_scan_mover_sweeps_dev: k_span_slots,
the node refit from the span boxes, span_trace_kernel).

The comparator is the composition the feature is defined by: tests/mover_sweep_restate.py's compose_host, sweep by sweep
(tests/span_restate.py, compose_sweeps), whose cast for an animated mover groups the rays by firing fraction and casts each group
with the EXISTING explicit-ray cast (Scene.cast, no centre, no filter) on a FRESH scene built from span_vertices(VA, VB, s).
Every column must agree bit for bit -- t, prim, normal3, point3, sem, ins, intensity and the mover column -- except
incident_deg, at the rtol of tests/test_mover_sweeps_gpu.py.

Shapes are that file's: N in {40, 64, 200} rays per sweep in four lines (10, 16, 50 distinct firing fractions; 64: a wave lies in
one sweep), P in {1, 3} sweeps; no P * N is a multiple of 256.  Sets: the walker alone (keyframes), the walker rig alone
(skinned), the walker, a rigid box and the rig together, and a deformable of one triangle.  The walker's place and the clip's
phase were chosen on the CPU with the oracle composition (tests/test_span_host.py) so that in every sweep the animated mover wins
rays whose record differs from the scan with its shape frozen at the sweep's start; the test asserts it."""
import json

import numpy as np
import pytest

import mover_restate as mv
import mover_sweep_restate as ms
import span_restate as sp
from test_mover_sweeps_gpu import sweeps_dev
from test_movers_gpu import CAST, HITS, _views, assert_bit_equal, assert_records, cast_of, scene_of
from test_span_host import (RIG_PHASE, clip_shapes, mesh_of, shape_vertices, sweep_inputs, triangle_keyframes, trio_records,
                            walker_records)

pytestmark = pytest.mark.gpu

F = np.float32
ALL = HITS + ("mover",)


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


class Member:
    """One mover of a set: ``keys`` (K, V, 3) float32 keyframes (None: rigid), the mesh that gives topology and labels, the clip's
    phase shift, and what goes into the MoverSet (a deformable, or the mesh)."""

    def __init__(self, mesh, keys=None, phase=0.0, entry=None):
        self.mesh, self.keys, self.phase, self.entry = mesh, keys, phase, mesh if entry is None else entry


class World:
    pass


@pytest.fixture(scope="module")
def world(engine):
    from lidarcast import deform, skin, synth
    from lidarcast.movers import MoverSet
    w = World()
    w.ctx = engine.ctx
    w.room = mv.room_mesh()
    w.scene = scene_of(w.ctx, w.room)
    w.static = cast_of(w.scene)
    walker = synth.make_walker(semantic=13, instance=1001)
    rig = synth.make_walker_rig(semantic=13, instance=1003, smooth=0.1)
    rig_keys = skin.keyframes(rig.vertices, rig.bone_index, rig.bone_weight, rig.poses12)
    tri_keys, tri_f = triangle_keyframes()
    tri = synth.TriangleMesh(vertices=tri_keys[0].astype(np.float64), triangles=tri_f, triangle_sem=np.array([7], np.uint16),
                             triangle_ins=np.array([31], np.uint16))
    w.d_walker = deform.Deformable(w.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
    w.d_rig = deform.SkinnedDeformable(w.ctx, rig.vertices, rig.triangles, rig.bone_index, rig.bone_weight, rig.poses12,
                                       rig.triangle_sem, rig.triangle_ins)
    w.d_rig_keys = deform.Deformable(w.ctx, rig_keys, rig.triangles, rig.triangle_sem, rig.triangle_ins)
    w.d_tri = deform.Deformable(w.ctx, tri_keys, tri_f, tri.triangle_sem, tri.triangle_ins)
    m_walker = Member(walker, walker.keyframes, 0.0, w.d_walker)
    m_rig = Member(rig, rig_keys, RIG_PHASE, w.d_rig)
    w.members = {"walker": [m_walker], "rig": [m_rig], "trio": [m_walker, Member(ms.box_mover(12, 77)), m_rig],
                 "triangle": [Member(tri, tri_keys, 0.0, w.d_tri)], "rig keyframes": [Member(rig, rig_keys, RIG_PHASE, w.d_rig_keys)]}
    w.sets = {name: MoverSet(w.ctx, [m.entry for m in ms_]) for name, ms_ in w.members.items()}
    yield w
    for s in w.sets.values():
        s.close()
    for d in (w.d_walker, w.d_rig, w.d_rig_keys, w.d_tri):
        d.close()
    w.scene.close()


def records_of(name, P):
    return trio_records(P) if name == "trio" else walker_records(P)


def shapes_of(members, P):
    """(shapes_a, shapes_b) (P, D, 3) of the animated members, and per animated member and sweep the two vertex arrays"""
    anim = [m for m in members if m.keys is not None]
    ab = [clip_shapes(len(m.keys), P, m.phase) for m in anim]
    sa, sb = np.stack([a for a, _ in ab], 1), np.stack([b for _, b in ab], 1)
    ends = {id(m): [(shape_vertices(m.keys, sa[p, j]), shape_vertices(m.keys, sb[p, j])) for p in range(P)] for j, m in enumerate(anim)}
    return sa, sb, ends


def fresh_cast(ctx, template):
    """vertices -> a cast function on a fresh scene of them (built, cast once, closed)"""
    def of(verts):
        def cast(rays):
            sc = scene_of(ctx, mesh_of(template, verts))
            try:
                return sc.cast(rays, center=None, max_range=np.inf, want=CAST)
            finally:
                sc.close()
        return cast
    return of


def tensors(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def span_sweeps_dev(scene, mset, motion, dirs, fire, rec, sa, sb, max_range, stream=None):
    import torch
    from lidarcast import DeviceHits, deform
    P, N = len(motion), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=HITS)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    mt, dt, ft, rt = tensors(motion, dirs, fire, np.asarray(rec, F))
    if stream is None:
        deform.scan_deforming_sweeps_dev(scene, mt, dt, ft, hits, max_range, mset, rt, sa, sb, mover_t=who)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            deform.scan_deforming_sweeps_dev(scene, mt, dt, ft, hits, max_range, mset, rt, sa, sb, mover_t=who, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in HITS})
    out["mover"] = who.cpu().numpy()
    return out


def composition(world, members, ends, rays, cen, fire, rec, N, max_range, frozen=False):
    def casts(p):
        out = []
        for m in members:
            if m.keys is None:
                out.append(fresh_cast(world.ctx, m.mesh)(np.asarray(m.mesh.vertices, F)))
            elif frozen:
                out.append(fresh_cast(world.ctx, m.mesh)(ends[id(m)][p][0]))
            else:
                out.append(sp.fraction_cast(fresh_cast(world.ctx, m.mesh), ends[id(m)][p][0], ends[id(m)][p][1], fire))
        return out
    return sp.compose_sweeps(world.static, casts, rays, cen, fire, rec, N, max_range)


# ---- 1: parity with the composition -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["walker", "rig", "trio", "triangle"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N", [40, 64, 200])
def test_parity_with_the_composition(world, N, P, name):
    members = world.members[name]
    dirs, fire, motion, rays, cen = sweep_inputs(N, P)
    rec = records_of(name, P)
    sa, sb, ends = shapes_of(members, P)
    assert (P * N) % 256 != 0 and (N % 64 == 0) == (N == 64)
    want, win = composition(world, members, ends, rays, cen, fire, rec, N, 2.2)
    frozen, _ = composition(world, members, ends, rays, cen, fire, rec, N, 2.2, frozen=True)
    animated = [j + 1 for j, m in enumerate(members) if m.keys is not None]
    differs = np.zeros(P * N, bool)
    for a in ("t", "prim", "normal3", "point3"):
        differs |= (want[a].view(np.uint32).reshape(P * N, -1) != frozen[a].view(np.uint32).reshape(P * N, -1)).any(1)
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        for j in animated:
            n = int((differs[sl] & (want["mover"][sl] == j)).sum())
            assert n >= 1, f"sweep {p}: no ray is won by animated mover {j} with a record that differs from the frozen scan"
    wins = np.bincount(want["mover"], minlength=len(members) + 1)
    print(f"\n[span] {name}, N {N}, P {P}: room / movers win {wins.tolist()} rays, {int(differs.sum())} records differ from the "
          f"scan frozen at A, the filter removes {int(((win['t'] < np.inf) & ~want['keep']).sum())}")
    assert (wins > 0).all()
    got = span_sweeps_dev(world.scene, world.sets[name], motion, dirs, fire, rec, sa, sb, 2.2)
    assert_records(got, want, f"{name}, N {N}, P {P}")


# ---- 2: identities ------------------------------------------------------------------------------------------------------------------

def plain_set_scan(world, members, verts_of, motion, dirs, fire, rec, max_range):
    """lrc_scan_mover_sweeps_dev with every animated member replaced by a plain scene of ``verts_of(member)``"""
    from lidarcast.movers import MoverSet
    plain = MoverSet(world.ctx, [m.mesh if m.keys is None else mesh_of(m.mesh, verts_of(m)) for m in members])
    try:
        return sweeps_dev(world.scene, plain, motion, dirs, fire, rec, max_range)
    finally:
        plain.close()


def one_shape(members, P, which=0):
    """the same (A, B) in every sweep: sweep 0's shapes"""
    sa, sb, ends = shapes_of(members, 1)
    return np.repeat(sa, P, 0), np.repeat(sb, P, 0), {k: v[0] for k, v in ends.items()}


@pytest.mark.parametrize("name", ["walker", "trio", "triangle"])
@pytest.mark.parametrize("N", [64, 200])
def test_a_shape_that_does_not_change_is_the_plain_mover(world, name, N):
    members = world.members[name]
    dirs, fire, motion, _, _ = sweep_inputs(N, 3)
    rec = records_of(name, 3)
    sa, _, ends = one_shape(members, 3)
    want = plain_set_scan(world, members, lambda m: ends[id(m)][0], motion, dirs, fire, rec, 2.2)
    got = span_sweeps_dev(world.scene, world.sets[name], motion, dirs, fire, rec, sa, sa, 2.2)
    assert (np.bincount(want["mover"], minlength=len(members) + 1) > 0).all()
    for a in ALL:
        assert_bit_equal(got[a], want[a], f"A == B, {name}, N {N}: {a}")


@pytest.mark.parametrize("name", ["walker", "trio"])
def test_constant_fire_tables(world, name):
    """all zeros: shape A's bytes; a constant c: the bytes of the fresh scene of span_vertices(VA, VB, c)"""
    from lidarcast import deform
    members = world.members[name]
    dirs, _, motion, _, _ = sweep_inputs(200, 3)
    rec = records_of(name, 3)
    sa, sb, ends = one_shape(members, 3)
    for c in (0.0, 0.37, 1.0 - 2.0 ** -24):
        fire = np.full(200, c)
        want = plain_set_scan(world, members, lambda m: deform.span_vertices(ends[id(m)][0], ends[id(m)][1], c), motion, dirs, fire,
                              rec, 2.2)
        got = span_sweeps_dev(world.scene, world.sets[name], motion, dirs, fire, rec, sa, sb, 2.2)
        assert (want["mover"] == 1).sum() > 20
        for a in ALL:
            assert_bit_equal(got[a], want[a], f"fire == {c}, {name}: {a}")
    zero = plain_set_scan(world, members, lambda m: ends[id(m)][0], motion, dirs, np.zeros(200), rec, 2.2)
    got = span_sweeps_dev(world.scene, world.sets[name], motion, dirs, np.zeros(200), rec, sa, sb, 2.2)
    for a in ALL:
        assert_bit_equal(got[a], zero[a], f"fire == 0 is shape A, {name}: {a}")


def test_every_other_entry_point_sees_shape_a(world):
    """after span, Scene.cast on the deformable's scene gives the bytes it gives after set(A): only the node boxes are larger"""
    import torch
    sa, sb, _ = shapes_of(world.members["walker"], 3)
    d = world.d_walker
    rays = sweep_inputs(200, 3)[3]
    to_obj = ms.to_object_at(rays, np.zeros(len(rays)), walker_records(1)[0, 0])
    for p in range(3):
        d.set(int(sa[p, 0, 0]), int(sa[p, 0, 1]), sa[p, 0, 2])
        torch.cuda.synchronize()
        want = d.scene.cast(to_obj, center=None, max_range=np.inf, want=CAST)
        verts = d.vertices()
        d.span(sa[p, 0], sb[p, 0])
        torch.cuda.synchronize()
        got = d.scene.cast(to_obj, center=None, max_range=np.inf, want=CAST)
        assert (want["t"] < np.inf).sum() > 20
        for a in CAST:
            assert_bit_equal(got[a], want[a], f"cast after span, sweep {p}: {a}")
        assert_bit_equal(d.vertices(), verts, "the vertices are shape A's")


def test_set_after_span_restores_the_frozen_route(world):
    members = world.members["walker"]
    dirs, fire, motion, _, _ = sweep_inputs(200, 3)
    rec = walker_records(3)
    sa, sb, ends = one_shape(members, 3)
    d = world.d_walker
    d.span(sa[0, 0], sb[0, 0])
    d.set(int(sb[0, 0, 0]), int(sb[0, 0, 1]), sb[0, 0, 2])
    got = sweeps_dev(world.scene, world.sets["walker"], motion, dirs, fire, rec, 2.2)
    want = plain_set_scan(world, members, lambda m: ends[id(m)][1], motion, dirs, fire, rec, 2.2)
    assert (want["mover"] == 1).sum() > 20
    for a in ALL:
        assert_bit_equal(got[a], want[a], f"set after span: {a}")


def test_skinned_and_keyframe_deformables_agree(world):
    dirs, fire, motion, _, _ = sweep_inputs(200, 3)
    rec = walker_records(3)
    sa, sb, _ = shapes_of(world.members["rig"], 3)
    skinned = span_sweeps_dev(world.scene, world.sets["rig"], motion, dirs, fire, rec, sa, sb, 2.2)
    keyed = span_sweeps_dev(world.scene, world.sets["rig keyframes"], motion, dirs, fire, rec, sa, sb, 2.2)
    assert (skinned["mover"] == 1).sum() > 20
    for a in ALL:
        assert_bit_equal(skinned[a], keyed[a], f"skinned against keyframes: {a}")
    assert world.d_rig.span_launches()[0] == world.d_rig.launches()[0] + 2
    assert world.d_walker.span_launches() == (world.d_walker.launches()[0] + 2, world.d_walker.launches()[1] + 1)


# ---- 3: no host wait ------------------------------------------------------------------------------------------------------------------

def test_spans_and_scans_on_one_stream_need_no_wait(world):
    import torch
    members = world.members["trio"]
    dirs, fire, motion, _, _ = sweep_inputs(200, 3)
    rec = trio_records(3)
    sa, sb, _ = shapes_of(members, 3)
    assert len({sa[p].tobytes() + sb[p].tobytes() for p in range(3)}) == 3            # three runs: span, scan, span, scan, ...
    got = span_sweeps_dev(world.scene, world.sets["trio"], motion, dirs, fire, rec, sa, sb, 2.2, stream=torch.cuda.Stream())
    parts = []
    for p in range(3):
        for j, d in enumerate(world.sets["trio"].deformables):
            d.span(sa[p, j], sb[p, j])
            torch.cuda.synchronize()
        parts.append(sweeps_dev(world.scene, world.sets["trio"], motion[p:p + 1], dirs, fire, rec[p:p + 1], 2.2))
    for a in ALL:
        assert_bit_equal(got[a], np.concatenate([q[a] for q in parts]), f"one stream against synchronised steps: {a}")
    assert (np.bincount(got["mover"], minlength=4) > 0).all()


def test_refusals(world):
    d = world.d_walker
    with pytest.raises(ValueError, match="shape B out of range"):
        d.span((0, 1, 0.5), (0, 8, 0.5))
    with pytest.raises(ValueError, match="w of shape A must lie in"):
        d.span((0, 1, 1.5), (0, 1, 0.5))
    with pytest.raises(ValueError, match="a shape is"):
        d.span((0, 1), (0, 1, 0.5))
    before = d.scene.info["device_bytes"]
    d.span((0, 1, 0.5), (1, 2, 0.5))
    d.span((1, 2, 0.5), (2, 3, 0.5))
    assert d.scene.info["device_bytes"] == before          # the extra arrays were counted when the first span made them
    d.set(0, 0, 0.0)


# ---- 4: the simulator end to end ------------------------------------------------------------------------------------------------------

def test_simulator_per_ray_shape(world, tmp_path):
    import s3dis_simulator
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 3, yaw=0.6)
    key = {"period": 0.1, "per_ray_shape": True, "objects": [
        {"mesh": "walker", "semantic": 13, "instance": 1001, "animation": {"cycle": 0.8, "phase": 0.03},
         "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.4, 3.3, 1.4, 0.0, 140.0]]},
        {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]},
        {"mesh": "walker_rig", "semantic": 13, "instance": 1003, "animation": {"cycle": 1.0}, "path": [[0.0, 2.6, 1.2, 0.0, 90.0]]}]}
    sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}, "motion": {"speed": 0.5, "movers": key}})
    sim.load_scene(world.room, "room")
    out = sim.run_simulation(wps)
    assert out.get_total_frames() == 3
    tracks = out.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "room_mover_tracks.json"))
    assert disk == json.loads(json.dumps(tracks))
    T = 1.0 / sim.lidar_config.scan_frequency
    seen = np.zeros(4, np.int64)
    for f, fr in enumerate(out.frames):
        ids = fr.mover_ids
        assert ids.dtype == np.uint8 and len(ids) == len(fr.points) == len(fr.point_times) == len(fr.semantic_labels) > 0
        assert fr.point_times.min() >= 0.0 and fr.point_times.max() < T
        seen += np.bincount(ids, minlength=4)
        assert (fr.instance_labels[ids == 1] == 1001).all() and (fr.instance_labels[ids == 3] == 1003).all()
        walker, post, rig = disk["frames"][f]["movers"]
        assert walker["end_shape"] != walker["shape"] and len(walker["end_shape"]) == 3 and "end_shape" not in post
        assert len(rig["end_joints"]) == len(rig["joints"]) == 6 and "end_pose" in walker
    assert (seen > 0).all(), seen
