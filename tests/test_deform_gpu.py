"""-m gpu: deforming movers on the device (lrc_deform_create / lrc_deform_set_dev: the blend kernel, the slot kernel, one node
kernel per height and the single-workgroup tail).  Every comparison is bit for bit.

For each mesh (the walker, a 12-triangle cube, a 4-triangle tetrahedron whose tree is the wrapped single leaf, triangle strips
with the vertex count and with the slot count at 255, 256 and 257: the edges of the 256-wide launches), each shape (keyframe 0,
a mid blend, the extreme keyframe) and each ray set (random rays, rays aimed at vertices):
  * the cast on the deformable scene equals the cast on a fresh Scene of Deformable.vertices() on both node routes of the
    fresh scene, and the oracle's brute force on those vertices;
  * the exported tree satisfies the box invariant of tests/test_deform_host.py; the triangle records equal the fresh scene's
    gathered through slot_prim; vertices() equals the host blend.
Then: set(0, 0, 0) after other shapes restores the bytes of creation (those of a fresh LRC_QNODES=0 scene); a room with the
walker and a rigid pedestrian scanned over three frames of three shapes equals per-frame scans of fresh rigid scenes; two sets
and two scans enqueued on one stream equal the same with a synchronise between them; the refusals."""
import numpy as np
import pytest

import helpers
import mover_restate as mv
from deform_restate import check_box_invariant
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
CAST = ("t", "prim", "sem", "ins", "normal3")
HITS = ("t", "prim", "normal3", "point3", "sem", "ins")
FRAMES = ("point3", "sem", "ins", "index", "range_origin")


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def strip(V):
    """A zig-zag triangle strip of V vertices (V - 2 triangles) along x, bent into three keyframes."""
    i = np.arange(V)
    x, y = (5.0 / V) * i, (i % 2) * 0.5
    k0 = np.stack([x, y, np.zeros(V)], 1)
    k1 = np.stack([x, y, 0.3 * np.sin(28.0 / V * i)], 1)
    k2 = np.stack([0.8 * x, y + 0.1 * np.cos(18.0 / V * i), 0.6 * np.sin(13.0 / V * i) - 0.2], 1)
    t = np.array([(j, j + 1, j + 2) if j % 2 == 0 else (j + 1, j, j + 2) for j in range(V - 2)], np.int32)
    return np.stack([k0, k1, k2]).astype(F), t


def case(name):
    """(keyframes (K, V, 3) float32, triangles, sem, ins, index of the extreme keyframe)."""
    from lidarcast import synth
    rng = np.random.default_rng(17)
    if name == "walker":
        m = synth.make_walker()
        return m.keyframes, np.asarray(m.triangles, np.int32), m.triangle_sem, m.triangle_ins, 2
    if name == "cube":
        m = synth.unit_cube(-0.3, 0.3)
        v = np.asarray(m.vertices)
        keys = np.stack([v, v * [1.3, 0.8, 1.0] + rng.normal(0, 0.05, v.shape), v * [0.6, 1.4, 1.2] + [0.2, 0.0, -0.1]]).astype(F)
        t = np.asarray(m.triangles, np.int32)
    elif name == "tetra":
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) - 0.25
        keys = np.stack([v, v * [1.5, 1.0, 0.7], v[:, ::-1] * 1.2 + 0.1]).astype(F)
        t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    else:
        keys, t = strip(int(name[5:]))
    return keys, t, np.full(len(t), 12, np.uint16), (np.arange(len(t)) % 7 + 1).astype(np.uint16), 2


# strips: T = V - 2 = 253 .. 257; 4096 triangles have more than 256 nodes of height 0, so level launches precede the tail
CASES = ["walker", "cube", "tetra"] + [f"strip{v}" for v in (255, 256, 257, 258, 259, 4098)]


def ray_sets(verts):
    lo, hi = verts.min(0) - 1.0, verts.max(0) + 1.0
    rnd = helpers.random_rays(2000, lo, hi, seed=3)
    rng = np.random.default_rng(4)
    pick = verts[rng.integers(0, len(verts), 800)].astype(np.float64)
    o = rng.uniform(lo, hi, (800, 3))
    aimed = np.concatenate([o, pick - o], 1).astype(F)          # aimed at vertices, not normalised
    return {"random": rnd, "aimed": aimed}


def fresh_scene(ctx, verts, t, sem, ins, float32_nodes):
    import lidarcast
    with pytest.MonkeyPatch.context() as mp:              # read at every scene creation
        mp.setenv("LRC_QNODES", "0" if float32_nodes else "2")
        return lidarcast.Scene(ctx, verts, t, sem, ins)


def views(out):
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


@pytest.mark.parametrize("name", CASES)
def test_deformed_scene_equals_fresh_scene_and_brute_force(engine, name):
    check_case(engine, name)


@pytest.mark.parametrize("name", ["walker", "tetra", "strip257"])
def test_one_launch_per_height_to_the_top(engine, name, monkeypatch):
    """LRC_DEFORM_TAIL=0 (read at creation): no single-workgroup tail, k_level climbs every height."""
    monkeypatch.setenv("LRC_DEFORM_TAIL", "0")
    check_case(engine, name, tail=False)


def check_case(engine, name, tail=True):
    from lidarcast import deform
    from oracle.c_oracle import OracleMesh
    keys, t, sem, ins, ext = case(name)
    d = deform.Deformable(engine.ctx, keys, t, sem, ins)
    try:
        assert d.scene.info["quantised_nodes"] == 0
        heights = d.launches()[1] - 1          # without a tail: the slot kernel and one launch per height
        assert tail or heights >= (1 if name == "tetra" else 4), d.launches()
        if name == "strip4098":                # more than 256 nodes of height 0: level launches below the tail
            assert d.launches()[1] > 2, d.launches()
        print(f"\n[deform] {name}: V {keys.shape[1]} T {len(t)} nodes {d.scene.info['num_nodes']} launches {d.launches()}")
        for shape in [(0, 0, 0.0), (0, 1, 0.37), (1, ext, 0.5), (ext, ext, 0.0), (1, ext, 1.0)]:
            d.set(*shape)
            verts = d.vertices()                                  # synchronises: the host-pointer casts below may follow
            want_v = keys[shape[0]] if shape[2] == 0 else keys[shape[1]] if shape[2] == 1 else deform.blend(keys[shape[0]], keys[shape[1]], shape[2])
            assert_bit_equal(verts, want_v, f"{name} {shape}: vertices")
            nodes, slot_prim = d.scene.export_bvh()
            check_box_invariant(nodes, slot_prim, t.astype(np.uint32), verts, f"{name} {shape}")
            om = OracleMesh(verts, t)
            fresh = {r: fresh_scene(engine.ctx, verts, t, sem, ins, r == "float32") for r in ("float32", "quantised")}
            try:
                # the records, through slot_prim (each triangle sits in exactly one slot of either scene)
                rec = d.scene.export_array("tris").view(F).reshape(-1, 12)
                frec = fresh["float32"].export_array("tris").view(F).reshape(-1, 12)
                by_prim = np.empty_like(frec)
                by_prim[fresh["float32"].export_bvh()[1]] = frec
                assert_bit_equal(rec, by_prim[slot_prim], f"{name} {shape}: triangle records")
                for rname, rays in ray_sets(verts).items():
                    got = views(d.scene.cast(rays, want=CAST))
                    assert (got["t"] != np.inf).sum() > (100 if rname == "aimed" else 0), (name, shape, rname)
                    for r, sc in fresh.items():
                        ref = views(sc.cast(rays, want=CAST))
                        for a in CAST:
                            assert_bit_equal(got[a], ref[a], f"{name} {shape} {rname} vs fresh {r}: {a}")
                    bt, bp = om.brute(rays)
                    assert_bit_equal(got["t"], bt, f"{name} {shape} {rname} vs brute force: t")
                    assert_bit_equal(got["prim"], bp, f"{name} {shape} {rname} vs brute force: prim")
            finally:
                for sc in fresh.values():
                    sc.close()
    finally:
        d.close()


@pytest.mark.parametrize("name", ["walker", "tetra", "strip257"])
def test_set_keyframe_0_restores_the_bytes_of_creation(engine, name):
    from lidarcast import deform
    keys, t, sem, ins, ext = case(name)
    d = deform.Deformable(engine.ctx, keys, t, sem, ins)
    fresh = fresh_scene(engine.ctx, keys[0], t, sem, ins, True)
    try:
        arrays = ("nodes", "tris", "slot_prim", "slot_label")
        born = {a: d.scene.export_array(a) for a in arrays}
        for a in arrays:
            assert np.array_equal(born[a], fresh.export_array(a)), f"{name}: {a} differs from a fresh LRC_QNODES=0 scene"
        for shape in [(0, 1, 0.25), (ext, ext, 0.0), (1, ext, 0.8)]:
            d.set(*shape)
        d.vertices()
        assert not np.array_equal(born["nodes"], d.scene.export_array("nodes"))
        assert not np.array_equal(born["tris"], d.scene.export_array("tris"))
        d.set(0, 0, 0.0)
        d.vertices()
        for a in arrays:
            assert np.array_equal(born[a], d.scene.export_array(a)), f"{name}: {a} not restored"
        # bounds: the union of all keyframes, whatever the shape
        lo, hi = keys[:, np.unique(t)].reshape(-1, 3).min(0), keys[:, np.unique(t)].reshape(-1, 3).max(0)
        assert np.array_equal(np.array(d.scene.info["bounds_lo"], F), lo) and np.array_equal(np.array(d.scene.info["bounds_hi"], F), hi)
    finally:
        fresh.close()
        d.close()


def scan_world():
    from lidarcast import synth
    room = mv.room_mesh()
    walker = synth.make_walker(instance=1001)
    ped = synth.make_pedestrian(semantic=13, instance=1002)
    k = helpers.sensor_small(lines=4, width=128)
    poses = np.stack([helpers.pose(1.2, 1.0, 1.0, 0.3)] * 3)
    mp = np.empty((3, 2, 12), F)
    for f in range(3):
        mp[f, 0] = mv.pose12(2.4, 1.6, 0.0, 0.4)                 # the walker stays where it is: only its shape changes
        mp[f, 1] = mv.pose12(1.9 + 0.3 * f, 2.7, 0.0, 0.2 * f)
    shapes = np.array([[[0, 1, 0.0]], [[1, 2, 0.5]], [[2, 2, 0.0]]], np.float64)
    return room, walker, ped, k, poses, mp, shapes


def test_three_frames_of_three_shapes_equal_fresh_rigid_scenes(engine):
    from lidarcast import deform
    from lidarcast.movers import MoverSet
    from lidarcast.synth import TriangleMesh
    room, walker, ped, k, poses, mp, shapes = scan_world()
    d = deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
    mset = MoverSet(engine.ctx, [d, ped])
    try:
        assert mset.deformables == [d] and len(mset) == 2
        got = deform.scan_deforming_frames(engine, k, poses, room, mset, mp, shapes, want=FRAMES)
        off = np.concatenate([[0], np.cumsum(got["counts"])])
        walker_pts = []
        for f in range(3):
            verts = deform.blend(walker.keyframes[int(shapes[f, 0, 0])], walker.keyframes[int(shapes[f, 0, 1])], shapes[f, 0, 2])
            rigid = TriangleMesh(vertices=verts.astype(np.float64), triangles=walker.triangles, triangle_sem=walker.triangle_sem,
                                 triangle_ins=walker.triangle_ins)
            ref_set = MoverSet(engine.ctx, [rigid, ped])
            try:
                ref = engine.scan_mover_frames(k, poses[f:f + 1], room, ref_set, mp[f:f + 1], want=FRAMES)
            finally:
                ref_set.close()
            assert got["counts"][f] == ref["total"]
            for a in FRAMES + ("mover",):
                g, w = got[a][off[f]:off[f + 1]], ref[a]
                assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"frame {f}: {a}"
            won = ref["mover"] == 1
            assert won.sum() > 10 and (ref["mover"] == 2).any() and (ref["mover"] == 0).any(), f      # everyone wins rays
            walker_pts.append(ref["point3"][won].tobytes())
        assert len(set(walker_pts)) == 3            # the three shapes put the walker's points elsewhere
        assert got["total"] == off[-1]
    finally:
        mset.close()
        d.close()


def test_sets_and_scans_on_one_stream_need_no_wait(engine):
    import torch
    from lidarcast import DeviceHits, deform
    from lidarcast.movers import MoverSet
    room, walker, ped, k, poses, mp, shapes = scan_world()
    poses, mp, shapes = poses[:2], mp[:2], shapes[1:]           # shape A = a blend, shape B = the extreme keyframe
    from lidar import IndoorLidar
    dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
    N = len(dirs)
    scene = engine.scene_for(room)
    d = deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins)
    mset = MoverSet(engine.ctx, [d, ped])
    try:
        pt = torch.from_numpy(poses.reshape(2, 16).copy()).cuda()
        dt = torch.from_numpy(dirs).cuda()
        mt = torch.from_numpy(mp).cuda()

        def read(hits, who):
            out = views({a: hits[a].cpu().numpy() for a in HITS})
            out["mover"] = who.cpu().numpy()
            return out

        # one stream, one synchronise
        hits = DeviceHits(2 * N, "cuda", want=HITS)
        who = torch.full((2 * N,), 255, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            deform.scan_deforming_dev(scene, pt, dt, hits, k.max_range, mset, mt, shapes, mover_t=who, stream=st.cuda_stream)
        torch.cuda.synchronize()
        got = read(hits, who)

        # the same two scans with a synchronise after every step
        parts = []
        for f in range(2):
            d.set(int(shapes[f, 0, 0]), int(shapes[f, 0, 1]), shapes[f, 0, 2])
            torch.cuda.synchronize()
            h1 = DeviceHits(N, "cuda", want=HITS)
            w1 = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
            scene.scan_movers_dev(pt[f:f + 1], dt, h1, k.max_range, mset, mt[f:f + 1], mover_t=w1)
            torch.cuda.synchronize()
            parts.append(read(h1, w1))
        for a in HITS + ("mover",):
            w = np.concatenate([p[a] for p in parts])
            assert got[a].dtype == w.dtype and np.array_equal(got[a].view(np.uint8), w.view(np.uint8)), a
        assert (parts[0]["mover"] == 1).sum() > 10 and (parts[1]["mover"] == 1).sum() > 10
        assert parts[0]["point3"][parts[0]["mover"] == 1].tobytes() != parts[1]["point3"][parts[1]["mover"] == 1].tobytes()
    finally:
        mset.close()
        d.close()


def test_refusals(engine):
    import torch
    import lidarcast
    from lidarcast import deform
    keys, t, sem, ins, _ = case("cube")
    lib = lidarcast.load()
    with pytest.raises(ValueError, match="at least one keyframe"):
        deform.Deformable(engine.ctx, keys[:0], t)
    with pytest.raises(ValueError, match="at least one keyframe"):
        deform.Deformable(engine.ctx, keys, t[:0])
    with pytest.raises(ValueError, match="triangle index out of range"):
        deform.Deformable(engine.ctx, keys, t + 1)
    for badv in (np.nan, np.inf, 1.5e6):
        bad = keys.copy()
        bad[2, 3, 1] = badv
        with pytest.raises(ValueError, match="keyframe 2 has a coordinate"):
            deform.Deformable(engine.ctx, bad, t)
    d = deform.Deformable(engine.ctx, keys, t, sem, ins)
    try:
        for k0, k1, w in [(3, 0, 0.5), (0, 3, 0.5), (0, 1, -0.1), (0, 1, 1.5), (0, 1, np.nan)]:
            with pytest.raises(ValueError):
                d.set(k0, k1, w)
        # the scene belongs to the deformable
        assert lib.lrc_scene_destroy(d.scene._h) == lidarcast._capi.LRC_ERR_INVALID_ARG
        assert b"belongs to a deformable" in lib.lrc_last_error()
        assert (d.scene.cast(helpers.random_rays(64, -1, 1, seed=1), want=("t",))["t"] != np.inf).any()      # still alive
        # entry points that cache per-triangle geometry
        with pytest.raises(ValueError, match="deformable scene"):
            d.scene.export_array("prim_plane")
        poses = torch.eye(4, dtype=torch.float64, device="cuda").reshape(1, 16)
        dirs = torch.zeros((64, 3), dtype=torch.float64, device="cuda")
        dirs[:, 0] = 1.0
        prim = torch.zeros(64, dtype=torch.int32, device="cuda")
        rows = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError, match="deformable scene"):
            d.scene.cloud_from_prims_dev(poses, dirs, prim, rows)
    finally:
        d.close()
