"""-m gpu: skinned deforming movers on the device (lrc_deform_create_skinned / lrc_deform_set_dev: k_skin in front of the refit).
Every comparison is bit for bit.  The reference R is the keyframe route that already exists: a ``Deformable`` built from the
host-skinned keyframes ``skin.keyframes(...)`` and set to the same shape; its equality with a fresh scene and with brute force is
tests/test_deform_gpu.py's and is not repeated.

Rigs (tests/skin_restate.py), the smallest at which the kernel can go wrong: the walker rig, rigid and with smooth weights; a
tetrahedron with B = 1 (the wrapped single leaf); zig-zag strips of V = 255, 256, 257 with B = 3, K = 3 and random
four-influence weights (the edges of the 256-wide launch); a strip of V = 257 with B = 255 and K = 2 (the staging loop's last
partial pass, the largest table); a strip of V = 4098 (level launches below the tail).  For each rig and five shapes: vertices,
bounds, exported tree and triangle records, the casts of test_deform_gpu.py's two ray sets, and the launch counts.
Then: set(0, 0, 0) restores the bytes of creation; sets and scans on one stream need no wait; three frames of three shapes with
and without flow; the simulator's walker_rig against a keyframes file, with the joints of the tracks file; device_bytes; the
refusals that need a context."""
import json

import numpy as np
import pytest

import helpers
from helpers import assert_bit_equal
from skin_restate import rig
from test_deform_gpu import CAST, FRAMES, HITS, ray_sets, scan_world, views
from test_movers_gpu import _sim, engine  # noqa: F401  (engine: fixture)

pytestmark = pytest.mark.gpu

F = np.float32
RIGS = ["walker", "walker_smooth", "tetra", "strip255", "strip256", "strip257", "strip257b255", "strip4098"]
SHAPES3 = [(0, 0, 0.0), (0, 1, 0.37), (1, 2, 0.5), (2, 2, 0.0), (1, 2, 1.0)]
SHAPES2 = [(0, 0, 0.0), (0, 1, 0.37), (0, 1, 0.5), (1, 1, 0.0), (0, 1, 1.0)]          # K = 2 rigs use their two poses


def same_bytes(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def pair(ctx, g):
    """(the skinned deformable, the keyframe deformable R of the host-skinned keyframes, those keyframes)."""
    from lidarcast import deform, skin
    keys = skin.keyframes(g["rest"], g["idx"], g["wgt"], g["poses"])
    s = deform.SkinnedDeformable(ctx, g["rest"], g["tris"], g["idx"], g["wgt"], g["poses"], g["sem"], g["ins"])
    try:
        return s, deform.Deformable(ctx, keys, g["tris"], g["sem"], g["ins"]), keys
    except Exception:
        s.close()
        raise


@pytest.mark.parametrize("name", RIGS)
def test_skinned_equals_the_keyframe_route(engine, name):
    from lidarcast import deform
    g = rig(name)
    s, r, keys = pair(engine.ctx, g)
    try:
        assert isinstance(s, deform.Deformable) and s.num_keyframes == len(g["poses"]) == r.num_keyframes
        assert s.scene.info["quantised_nodes"] == 0
        refit = r.launches()[1]
        assert s.launches() == (1 + refit, 1 + refit) and r.launches() == (1 + refit, refit)
        if name == "strip4098":
            assert refit > 2, r.launches()                     # level launches below the tail
        if name == "tetra":
            assert s.scene.info["num_nodes"] == 1              # the wrapped single leaf
        print(f"\n[skin] {name}: V {len(g['rest'])} B {g['poses'].shape[1]} K {len(g['poses'])} launches {s.launches()} "
              f"device_bytes {s.scene.info['device_bytes']} vs keyframes {r.scene.info['device_bytes']}")
        for a in ("nodes", "tris", "slot_prim", "slot_label"):          # born equal: both built from key pose 0
            same_bytes(s.scene.export_array(a), r.scene.export_array(a), f"{name} at creation: {a}")
        assert_bit_equal(s.vertices(), keys[0], f"{name} at creation: vertices")
        for shape in (SHAPES2 if len(g["poses"]) == 2 else SHAPES3):
            s.set(*shape)
            r.set(*shape)
            k0, k1, w = shape
            want = keys[k0] if w == 0 or k0 == k1 else keys[k1] if w == 1 else deform.blend(keys[k0], keys[k1], w)
            verts = s.vertices()                                  # synchronises: the host-pointer casts below may follow
            assert_bit_equal(verts, want, f"{name} {shape}: vertices against the host blend of host-skinned key poses")
            assert_bit_equal(s.keyframe(k0), keys[k0], f"{name}: keyframe({k0})")
            assert_bit_equal(verts, r.vertices(), f"{name} {shape}: vertices against R")
            for b in ("bounds_lo", "bounds_hi"):
                assert s.scene.info[b] == r.scene.info[b], (name, shape, b)
            (sn, sp), (rn, rp) = s.scene.export_bvh(), r.scene.export_bvh()
            same_bytes(sn, rn, f"{name} {shape}: nodes")
            same_bytes(sp, rp, f"{name} {shape}: slot_prim")
            same_bytes(s.scene.export_array("tris"), r.scene.export_array("tris"), f"{name} {shape}: triangle records")
            for rname, rays in ray_sets(verts).items():
                got, ref = views(s.scene.cast(rays, want=CAST)), views(r.scene.cast(rays, want=CAST))
                assert (got["t"] != np.inf).sum() > (100 if rname == "aimed" else 0), (name, shape, rname)
                for a in CAST:
                    same_bytes(got[a], ref[a], f"{name} {shape} {rname}: {a}")
    finally:
        s.close()
        r.close()


@pytest.mark.parametrize("name", ["walker_smooth", "tetra", "strip257"])
def test_set_key_pose_0_restores_the_bytes_of_creation(engine, name):
    g = rig(name)
    s, r, keys = pair(engine.ctx, g)
    try:
        arrays = ("nodes", "tris", "slot_prim", "slot_label")
        born = {a: s.scene.export_array(a) for a in arrays}
        for shape in [(0, 1, 0.25), (2, 2, 0.0), (1, 2, 0.8)]:
            s.set(*shape)
        s.vertices()
        assert not np.array_equal(born["nodes"], s.scene.export_array("nodes"))
        assert not np.array_equal(born["tris"], s.scene.export_array("tris"))
        s.set(0, 0, 0.0)
        assert_bit_equal(s.vertices(), keys[0], f"{name}: vertices restored")
        for a in arrays:
            assert np.array_equal(born[a], s.scene.export_array(a)), f"{name}: {a} not restored"
        used = np.unique(g["tris"])
        lo, hi = keys[:, used].reshape(-1, 3).min(0), keys[:, used].reshape(-1, 3).max(0)
        assert np.array_equal(np.array(s.scene.info["bounds_lo"], F), lo) and np.array_equal(np.array(s.scene.info["bounds_hi"], F), hi)
    finally:
        s.close()
        r.close()


def walker_pair(ctx, smooth=0.08):
    g = rig("walker_smooth" if smooth else "walker")
    return pair(ctx, g)


def test_sets_and_scans_on_one_stream_need_no_wait(engine):
    import torch
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, deform
    from lidarcast.movers import MoverSet
    room, _, ped, k, poses, mp, shapes = scan_world()
    poses, mp, shapes = poses[:2], mp[:2], shapes[1:]           # shape A = a blend, shape B = a key pose
    dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
    N = len(dirs)
    scene = engine.scene_for(room)
    s, r, _ = walker_pair(engine.ctx)
    mset = MoverSet(engine.ctx, [s, ped])
    try:
        pt = torch.from_numpy(poses.reshape(2, 16).copy()).cuda()
        dt = torch.from_numpy(dirs).cuda()
        mt = torch.from_numpy(mp).cuda()

        def read(hits, who):
            out = views({a: hits[a].cpu().numpy() for a in HITS})
            out["mover"] = who.cpu().numpy()
            return out

        hits = DeviceHits(2 * N, "cuda", want=HITS)
        who = torch.full((2 * N,), 255, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            deform.scan_deforming_dev(scene, pt, dt, hits, k.max_range, mset, mt, shapes, mover_t=who, stream=st.cuda_stream)
        torch.cuda.synchronize()
        got = read(hits, who)
        parts = []
        for f in range(2):
            s.set(int(shapes[f, 0, 0]), int(shapes[f, 0, 1]), shapes[f, 0, 2])
            torch.cuda.synchronize()
            h1 = DeviceHits(N, "cuda", want=HITS)
            w1 = torch.full((N,), 255, dtype=torch.uint8, device="cuda")
            scene.scan_movers_dev(pt[f:f + 1], dt, h1, k.max_range, mset, mt[f:f + 1], mover_t=w1)
            torch.cuda.synchronize()
            parts.append(read(h1, w1))
        for a in HITS + ("mover",):
            same_bytes(got[a], np.concatenate([p[a] for p in parts]), a)
        assert (parts[0]["mover"] == 1).sum() > 10 and (parts[1]["mover"] == 1).sum() > 10
        assert parts[0]["point3"][parts[0]["mover"] == 1].tobytes() != parts[1]["point3"][parts[1]["mover"] == 1].tobytes()
    finally:
        mset.close()
        s.close()
        r.close()


@pytest.mark.parametrize("flow", [False, True])
def test_three_frames_of_three_shapes_equal_the_keyframe_route(engine, flow):
    from lidarcast import deform
    from lidarcast.movers import MoverSet
    room, _, ped, k, poses, mp, shapes = scan_world()
    if flow:                       # the walker and the sensor move as well, so that the flow has something to say
        poses = np.stack([helpers.pose(1.2 + 0.1 * f, 1.0, 1.0, 0.3) for f in range(3)])
        mp = mp.copy()
        for f in range(3):
            mp[f, 0, 3] += F(0.1 * f)
    s, r, _ = walker_pair(engine.ctx)
    scan = deform.scan_deforming_flow_frames if flow else deform.scan_deforming_frames
    out = {}
    try:
        for who, d in (("skinned", s), ("keyframes", r)):
            mset = MoverSet(engine.ctx, [d, ped])
            try:
                assert mset.deformables == [d]
                out[who] = scan(engine, k, poses, room, mset, mp, shapes, want=FRAMES)
            finally:
                mset.close()
    finally:
        s.close()
        r.close()
    got, ref = out["skinned"], out["keyframes"]
    assert got["total"] == ref["total"] > 0 and sorted(got) == sorted(ref)
    for a in ref:
        if a != "total":
            same_bytes(got[a], ref[a], f"frames: {a}")
    assert (ref["mover"] == 1).sum() > 30 and (ref["mover"] == 2).any() and (ref["mover"] == 0).any()
    if flow:
        walker = ref["mover"] == 1
        assert "flow" in ref and "flow_status" in ref and (ref["flow"][walker] != 0).any() and (ref["flow_status"] != 0).any()


def test_simulator_walker_rig_equals_a_keyframes_file_and_exports_joints(engine, tmp_path):
    import mover_restate as mv
    from lidarcast import skin, synth
    from lidarcast.deform import Clip
    from lidarcast.ply import write_triangle_mesh
    from trajectory import line_trajectory
    room = mv.room_mesh()
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 4, yaw=0.6)
    m = synth.make_walker_rig(semantic=13, instance=1001)
    ply, npy = str(tmp_path / "walker.ply"), str(tmp_path / "walker_keys.npy")
    write_triangle_mesh(ply, m)
    keys = skin.keyframes(m.vertices, m.bone_index, m.bone_weight, m.poses12)
    np.save(npy, keys)
    walk = {"semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.3, 3.3, 1.4, 0.0, 140.0]],
            "animation": {"cycle": 0.8, "phase": 0.05}}
    ped = {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]}
    base = {"raycast_engine": {"use_gpu": True}}
    key = lambda obj: {"period": 0.1, "nonrigid_flow": True, "objects": [obj, ped]}
    one = _sim(dict(base, movers=key(dict(walk, mesh="walker_rig"))), room).run_simulation(wps)
    ref = _sim(dict(base, movers=key(dict(walk, mesh=ply, keyframes=npy))), room).run_simulation(wps)
    assert one.get_total_frames() == ref.get_total_frames() == 4
    rows = 0
    for f, (a, b) in enumerate(zip(one.frames, ref.frames)):
        assert_bit_equal(a.points, b.points, f"frame {f}: points")
        assert_bit_equal(a.flow, b.flow, f"frame {f}: flow")
        for col in ("mover_ids", "flow_status", "semantic_labels", "instance_labels"):
            assert getattr(a, col).tolist() == getattr(b, col).tolist(), (f, col)
        rows += int((a.mover_ids == 1).sum())
    assert rows > 10
    # the tracks file: shape, box and joints of the skinned mover
    tracks = one.export_mover_tracks(tmp_path / "skinned")
    disk = json.load(open(tmp_path / "skinned" / "room_mover_tracks.json"))
    assert disk == json.loads(json.dumps(tracks))
    ref_tracks = ref.export_mover_tracks(tmp_path / "keyframes")
    shapes = Clip(8, 0.8, phase=0.05).shapes3(np.arange(4) * 0.1)
    joints = np.array([fr["movers"][0]["joints"] for fr in disk["frames"]])
    assert joints.shape == (4, 6, 3)
    for f, fr in enumerate(disk["frames"]):
        me, other = fr["movers"][0], ref_tracks["frames"][f]["movers"][0]
        assert me["shape"] == [int(shapes[f, 0]), int(shapes[f, 1]), float(shapes[f, 2])] == other["shape"]
        assert me["box7"] == other["box7"] and me["num_points"] == other["num_points"]
        assert "joints" not in other and "joints" not in fr["movers"][1]
        k0, k1, w = me["shape"]
        j0, j1 = m.skeleton.joints(m.poses12[k0]), m.skeleton.joints(m.poses12[k1])
        m12 = np.asarray(me["pose"]["matrix12"], np.float64).reshape(3, 4)
        assert np.array_equal(joints[f], (j0 + w * (j1 - j0)) @ m12[:, :3].T + m12[:, 3]), f"frame {f}: joints"
        # the hip joints (bones 2 and 3) lie inside the mover's oriented box
        cx, cy, cz, ex, ey, ez, yaw = me["box7"]
        c, s_ = np.cos(yaw), np.sin(yaw)
        for hip in joints[f, 2:4]:
            dx, dy, dz = hip[0] - cx, hip[1] - cy, hip[2] - cz
            local = np.array([c * dx + s_ * dy, -s_ * dx + c * dy, dz])
            assert (np.abs(local) <= 0.5 * np.array([ex, ey, ez])).all(), (f, local, me["box7"])
    assert np.abs(joints[3] - joints[0]).max() > 0.1              # the walker walks


def test_a_long_clip_takes_fewer_device_bytes_than_its_keyframes(engine):
    g = rig("strip4098k64")
    s, r, _ = pair(engine.ctx, g)
    try:
        sb, rb = s.scene.info["device_bytes"], r.scene.info["device_bytes"]
        print(f"\n[skin] V 4098, K 64, B 3: skinned {sb} B, keyframes {rb} B")
        V, K, B = 4098, 64, 3
        assert rb - sb == K * V * 12 - (V * 32 + K * B * 48) and sb < rb
        s.set(62, 63, 0.25)
        r.set(62, 63, 0.25)
        assert_bit_equal(s.vertices(), r.vertices(), "the last two key poses")
    finally:
        s.close()
        r.close()


def test_refusals(engine):
    from lidarcast import deform
    g = rig("strip257")

    def create(**change):
        a = dict(g)
        a.update(change)
        return deform.SkinnedDeformable(engine.ctx, a["rest"], a["tris"], a["idx"], a["wgt"], a["poses"], a["sem"], a["ins"])
    idx = g["idx"].copy()
    idx[256, 0] = 3
    with pytest.raises(ValueError, match="vertex 256 names bone 3 of 3"):
        create(idx=idx)
    wgt = g["wgt"].copy()
    wgt[5, 1] = -0.125
    with pytest.raises(ValueError, match="vertex 5 has a weight that is not finite or is negative"):
        create(wgt=wgt)
    wgt = g["wgt"].copy()
    wgt[9] = [0.5, 0.4, 0.0, 0.0]
    with pytest.raises(ValueError, match="the weights of vertex 9 sum to 0.9"):
        create(wgt=wgt)
    poses = g["poses"].copy()
    poses[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="key pose 1, bone 2 has an entry that is not finite"):
        create(poses=poses)
    poses = g["poses"].copy()
    poses[2, :, 7] = -3.0e6
    with pytest.raises(ValueError, match="key pose 2 puts vertex 0 at a coordinate that is not finite or exceeds 1e6"):
        create(poses=poses)
    with pytest.raises(ValueError, match="B = 0 bones"):
        create(poses=np.zeros((3, 0, 12), F))
    with pytest.raises(ValueError, match="B = 256 bones"):
        create(poses=np.tile(g["poses"][:, :1], (1, 256, 1)))
    s = create()
    try:
        for k0, k1, w in [(3, 0, 0.5), (0, 3, 0.5), (0, 1, -0.1), (0, 1, 1.5), (0, 1, np.nan)]:
            with pytest.raises(ValueError):
                s.set(k0, k1, w)
        with pytest.raises(ValueError, match="keyframe index out of range"):
            s.set(0, 3, 0.0)
        assert (s.scene.cast(helpers.random_rays(256, -1, 6, seed=1), want=("t",))["t"] != np.inf).any()      # still alive
    finally:
        s.close()
