"""CPU: the host side of the skinned deforming movers (lidarcast.skin, lidarcast.deform.SkinnedDeformable).
lrc_skin_apply runs the inline function the kernel calls, so what is checked here bit for bit is the kernel's arithmetic:

  skin      against the numpy float32 restatement (tests/skin_restate.py) on random affine poses with 1 to 4 non-zero weights per
            row, on signed zeros in coordinates and matrices, and under the identity.
  rig       make_walker_rig against make_walker: within 2^-20 m (the rigid float32 skin against float64-then-narrowed keyframes
            measured 2^-23 m, so the cap leaves a factor of 8), equal topology and labels; smooth weights; the skeleton.
  refusals  of lrc_deform_create_skinned: the arrays are checked before the context, so a NULL context reaches every one of them;
            of the simulator's keys; the tracks file's joints.
No tolerance but the one named above."""
import ctypes as C
import json

import numpy as np
import pytest

from helpers import assert_bit_equal, bits
from skin_restate import affine_poses, random_influences, rig, skin_restate

from lidarcast import _capi, deform, skin, synth

F = np.float32


# ---- skin -----------------------------------------------------------------------------------------------------------------------

def test_apply_equals_numpy_restatement():
    rng = np.random.default_rng(7)
    V, B = 1000, 5
    rest = rng.uniform(-3, 3, (V, 3)).astype(F)
    idx, wgt = random_influences(rng, V, B)
    assert sorted(set((wgt != 0).sum(1).tolist())) == [1, 2, 3, 4]
    bones = affine_poses(rng, 1, B)[0]
    got = skin.apply(rest, idx, wgt, bones)
    assert got.dtype == F and got.shape == (V, 3)
    assert_bit_equal(got, skin_restate(rest, idx, wgt, bones), "random affine poses")
    keys = skin.keyframes(rest, idx, wgt, affine_poses(rng, 3, B))
    assert keys.shape == (3, V, 3) and keys.dtype == F


def test_apply_signed_zeros():
    rng = np.random.default_rng(8)
    V, B = 64, 4
    rest = rng.uniform(-2, 2, (V, 3)).astype(F)
    rest[::3, 0] = -0.0
    rest[1::5, 2] = 0.0
    rest[2::7] = -0.0
    idx, wgt = random_influences(rng, V, B)
    bones = affine_poses(rng, 1, B)[0]
    bones[0, [1, 2, 3]] = -0.0
    bones[1, [4, 7, 11]] = [-0.0, 0.0, -0.0]
    bones[2, :] = -0.0
    got = skin.apply(rest, idx, wgt, bones)
    assert_bit_equal(got, skin_restate(rest, idx, wgt, bones), "signed zeros")
    assert (bits(got) == 0x80000000).any() or (bits(got) == 0).any()


def test_single_influence_under_the_identity_gives_the_rest_bits():
    rng = np.random.default_rng(9)
    rest = rng.uniform(-5, 5, (40, 3)).astype(F)
    rest[3] = [-0.0, 1.0, -2.0]
    rest[4] = [-0.0, -0.0, -0.0]
    idx = np.zeros((40, 4), np.uint8)
    wgt = np.tile(np.array([1, 0, 0, 0], F), (40, 1))
    eye = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)
    got = skin.apply(rest, idx, wgt, eye)
    assert_bit_equal(got, skin_restate(rest, idx, wgt, eye), "identity")
    want = rest.copy()
    want[want == 0] = 0.0              # the formula ends in "+ m[4i+3]" = +0 and "+ 0 * p": -0 becomes +0
    assert_bit_equal(got, want, "identity gives the rest bits, -0 as +0")
    assert bits(got)[4].tolist() == [0, 0, 0]


def test_apply_refusals():
    rest, idx, wgt = np.zeros((2, 3), F), np.zeros((2, 4), np.uint8), np.zeros((2, 4), F)
    bones = np.zeros((3, 12), F)
    idx[1, 2] = 3
    with pytest.raises(ValueError, match="vertex 1 names bone 3 of 3"):
        skin.apply(rest, idx, wgt, bones)
    with pytest.raises(ValueError, match="1 <= B <= 255"):
        skin.apply(rest, idx, wgt, np.zeros((0, 12), F))
    with pytest.raises(ValueError, match="1 <= B <= 255"):
        skin.apply(rest, idx, wgt, np.zeros((256, 12), F))
    for bad in [dict(rest=np.zeros((2, 2))), dict(idx=np.zeros((2, 3), np.uint8)), dict(wgt=np.zeros((3, 4))),
                dict(idx=np.full((2, 4), 256)), dict(idx=np.zeros((2, 4))), dict(bones=np.zeros((3, 11)))]:
        kw = dict(rest=rest, idx=np.zeros((2, 4), np.uint8), wgt=wgt, bones=bones)
        kw.update(bad)
        with pytest.raises(ValueError):
            skin.apply(kw["rest"], kw["idx"], kw["wgt"], kw["bones"])


# ---- the walker rig -------------------------------------------------------------------------------------------------------------

def test_walker_rig_against_walker_keyframes():
    w, r = synth.make_walker(), synth.make_walker_rig()
    keys = skin.keyframes(r.vertices, r.bone_index, r.bone_weight, r.poses12)
    assert keys.shape == w.keyframes.shape and r.poses12.shape == (8, 6, 12) and r.poses12.dtype == F
    worst = np.abs(keys.astype(np.float64) - w.keyframes.astype(np.float64)).max()
    print(f"\n[skin] walker rig against make_walker keyframes: worst difference {worst:.3e} m (cap 2^-20 = {2.0 ** -20:.3e})")
    assert worst <= 2.0 ** -20
    assert_bit_equal(r.vertices.astype(F), w.keyframes[0], "the rest shape is keyframe 0")
    assert np.array_equal(r.triangles, w.triangles)
    assert np.array_equal(r.triangle_sem, w.triangle_sem) and np.array_equal(r.triangle_ins, w.triangle_ins)
    assert r.bone_index.dtype == np.uint8 and r.bone_weight.dtype == F
    assert ((r.bone_weight != 0).sum(1) == 1).all() and (r.bone_weight[:, 0] == 1).all()      # smooth = 0: one influence of 1
    assert sorted(set(r.bone_index[:, 0].tolist())) == [0, 1, 2, 3, 4, 5]
    other = synth.make_walker_rig(height=1.2, keyframes=5, swing_deg=40, semantic=7, instance=9)
    ref = synth.make_walker(height=1.2, keyframes=5, swing_deg=40)
    keys = skin.keyframes(other.vertices, other.bone_index, other.bone_weight, other.poses12)
    assert np.abs(keys.astype(np.float64) - ref.keyframes).max() <= 2.0 ** -20
    assert (other.triangle_sem == 7).all() and (other.triangle_ins == 9).all()


def test_walker_rig_smooth_weights():
    r = synth.make_walker_rig(smooth=0.08)
    sums = r.bone_weight.astype(np.float64).sum(1)
    assert (np.abs(sums - 1.0) <= 2.0 ** -10).all()
    two = (r.bone_weight != 0).sum(1) == 2
    assert two.any() and (r.bone_weight >= 0).all()
    assert (r.bone_index[two, 0] >= 2).all() and (r.bone_index[two, 1] == 0).all()      # a limb shares with the torso
    rigid = synth.make_walker_rig()
    same = (r.bone_weight == rigid.bone_weight).all(1)
    assert_bit_equal(skin.keyframes(r.vertices, r.bone_index, r.bone_weight, r.poses12)[:, same],
                     skin.keyframes(rigid.vertices, rigid.bone_index, rigid.bone_weight, rigid.poses12)[:, same], "untouched rows")
    assert_bit_equal(r.poses12, rigid.poses12, "the poses do not depend on smooth")


def test_skeleton_matrices_and_joints():
    r = synth.make_walker_rig()
    sk = r.skeleton
    eye = np.broadcast_to(np.eye(3), (6, 3, 3))
    assert_bit_equal(sk.matrices(eye), np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (6, 1)), "identity rotations")
    assert sk.matrices(np.broadcast_to(np.eye(3), (4, 2, 6, 3, 3))).shape == (4, 2, 6, 12)
    moved = sk.matrices(eye, root_translation=[0.5, 0.0, -0.25])
    assert_bit_equal(moved[:, [3, 7, 11]], np.tile(np.array([0.5, 0.0, -0.25], F), (6, 1)), "the root translation reaches every bone")
    # every joint stays on its pivot: the rest joint moved by the pose's root translation (float32 matrices: a few ulps of 1.7)
    j = sk.joints(r.poses12)
    assert j.shape == (8, 6, 3) and j.dtype == np.float64
    drop = r.poses12[:, 0, [3, 7, 11]].astype(np.float64)
    assert (r.poses12[:, 0, [3, 7]] == 0).all() and (drop[:, 2] <= 0).all() and drop[2, 2] < -0.01     # lowered, never sideways
    assert np.abs(j - (sk.joints_rest[None] + drop[:, None])).max() <= 2.0 ** -20
    # a child turns about its own joint and carries its children along
    chain = skin.Skeleton([-1, 0, 1], [[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    m = chain.matrices(np.stack([np.eye(3), rz, np.eye(3)]))
    assert np.allclose(chain.joints(m), [[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    with pytest.raises(ValueError, match="precede"):
        skin.Skeleton([1, -1], np.zeros((2, 3)))
    with pytest.raises(ValueError):
        sk.matrices(np.eye(3))
    with pytest.raises(ValueError):
        sk.joints(np.zeros((5, 12)))


# ---- lrc_deform_create_skinned: every refusal is reached without a context ------------------------------------------------------------

class NoContext:
    _h = None
    device = 0


def create(name="tetra", **change):
    g = dict(rig(name))
    g.update(change)
    return deform.SkinnedDeformable(NoContext(), g["rest"], g["tris"], g["idx"], g["wgt"], g["poses"], g["sem"], g["ins"])


def test_create_skinned_refusals():
    g = rig("strip257")
    with pytest.raises(ValueError, match="ctx is NULL"):          # a good rig passes every array check and stops at the context
        create("strip257")
    with pytest.raises(ValueError, match="ctx is NULL"):
        create("walker_smooth")
    idx = g["idx"].copy()
    idx[200, 3] = 3
    with pytest.raises(ValueError, match="vertex 200 names bone 3 of 3"):
        create("strip257", idx=idx)
    for badw, text in [(-0.25, "vertex 17 has a weight that is not finite or is negative"), (np.nan, "vertex 17 has a weight"),
                       (np.inf, "vertex 17 has a weight")]:
        wgt = g["wgt"].copy()
        wgt[17, 2] = badw
        with pytest.raises(ValueError, match=text):
            create("strip257", wgt=wgt)
    wgt = g["wgt"].copy()
    wgt[31] = [0.5, 0.4, 0.0, 0.0]
    with pytest.raises(ValueError, match="the weights of vertex 31 sum to 0.9"):
        create("strip257", wgt=wgt)
    wgt[31] = [0.5, 0.5 + 2.0 ** -11, 0.0, 0.0]                    # inside 2^-10: accepted
    with pytest.raises(ValueError, match="ctx is NULL"):
        create("strip257", wgt=wgt)
    wgt[31] = [0.5, 0.5 + 2.0 ** -9, 0.0, 0.0]
    with pytest.raises(ValueError, match="the weights of vertex 31"):
        create("strip257", wgt=wgt)
    for badp in (np.nan, -np.inf):
        poses = g["poses"].copy()
        poses[2, 1, 7] = badp
        with pytest.raises(ValueError, match="key pose 2, bone 1 has an entry that is not finite"):
            create("strip257", poses=poses)
    poses = g["poses"].copy()
    poses[1, :, 3] = 2.0e6                                          # key pose 1 throws every vertex beyond 1e6
    with pytest.raises(ValueError, match="key pose 1 puts vertex 0 at a coordinate that is not finite or exceeds 1e6"):
        create("strip257", poses=poses)
    poses = g["poses"].copy()
    poses[2, :, :] = F(3e38)                                         # finite entries, an infinite vertex
    with pytest.raises(ValueError, match="key pose 2 puts vertex"):
        create("strip257", poses=poses)
    with pytest.raises(ValueError, match=r"B = 0 bones"):
        create("strip257", poses=np.zeros((3, 0, 12), F))
    with pytest.raises(ValueError, match=r"B = 256 bones"):
        create("strip257", poses=np.tile(g["poses"][:, :1], (1, 256, 1)))
    with pytest.raises(ValueError, match="at least one key pose"):
        create("strip257", poses=g["poses"][:0])
    with pytest.raises(ValueError, match="at least one key pose and one triangle"):
        create("strip257", tris=g["tris"][:0], sem=None, ins=None)
    with pytest.raises(ValueError, match="triangle index out of range"):
        create("strip257", tris=g["tris"] + 1)
    # the Python layer's own shape checks
    for change in [dict(rest=g["rest"][:, :2]), dict(idx=g["idx"][:, :3]), dict(wgt=g["wgt"][:100]), dict(poses=g["poses"][:, :, :11]),
                   dict(idx=g["idx"].astype(np.float32)), dict(sem=g["sem"][:5])]:
        with pytest.raises(ValueError):
            create("strip257", **change)
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    a = [np.ascontiguousarray(g[k]) for k in ("rest", "idx", "wgt", "poses")]
    t = np.ascontiguousarray(g["tris"], np.uint32)
    assert lib.lrc_deform_create_skinned(None, a[0].ctypes.data, 257, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, 3, 3,
                                         t.ctypes.data, len(t), None, None, None) == E
    assert b"out is NULL" in lib.lrc_last_error()
    h = C.c_void_p(5)
    assert lib.lrc_deform_create_skinned(None, None, 257, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, 3, 3,
                                         t.ctypes.data, len(t), None, None, C.byref(h)) == E
    assert b"NULL rest" in lib.lrc_last_error() and not h.value


# ---- the simulator keys ------------------------------------------------------------------------------------------------------------

def sim_with(config):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
    sim.config = config
    sim.scene = object()
    return sim


PATH = [[0.0, 1.8, 2.6, 0.0, 20.0], [0.2, 2.8, 1.8, 0.0, 100.0]]
RIG = {"mesh": "walker_rig", "semantic": 13, "instance": 1001, "path": PATH, "animation": {"cycle": 0.8, "phase": 0.25}}
RIGID = {"mesh": "pedestrian", "instance": 1002, "path": [[0.0, 3.0, 1.0, 0.0, 0.0]]}


def skin_files(tmp_path, skeleton=True):
    from lidarcast.ply import write_triangle_mesh
    r = synth.make_walker_rig(smooth=0.08)
    ply, npz = str(tmp_path / "body.ply"), str(tmp_path / "body_skin.npz")
    write_triangle_mesh(ply, r)
    extra = dict(parents=r.skeleton.parents, joints=r.skeleton.joints_rest) if skeleton else {}
    np.savez(npz, bone_index=r.bone_index, bone_weight=r.bone_weight, poses=r.poses12, **extra)
    return r, ply, npz


def test_simulator_skin_keys(tmp_path):
    plan = sim_with({"movers": {"period": 0.1, "nonrigid_flow": True, "objects": [RIG, RIGID]}})._mover_plan()
    r = synth.make_walker_rig(semantic=13, instance=1001)
    got, clip = plan["skins"][0], plan["clips"][0]
    assert plan["skins"][1] is None and plan["keyframes"] == [None, None] and plan["nonrigid_flow"] is True
    assert (clip.K, clip.cycle, clip.phase, clip.loop) == (8, 0.8, 0.25, True)
    assert_bit_equal(got["rest"], r.vertices.astype(F), "rest")
    assert_bit_equal(got["poses12"], r.poses12, "poses")
    assert np.array_equal(got["bone_index"], r.bone_index) and np.array_equal(got["bone_weight"], r.bone_weight)
    assert len(got["skeleton"]) == 6
    assert plan["objects"][0]["animation"] == {"cycle": 0.8, "phase": 0.25, "loop": True, "num_keyframes": 8}
    keys = skin.keyframes(r.vertices, r.bone_index, r.bone_weight, r.poses12)
    assert plan["objects"][0]["box_min"] == [float(x) for x in keys.reshape(-1, 3).min(0)]         # all key poses
    assert plan["objects"][0]["box_max"] == [float(x) for x in keys.reshape(-1, 3).max(0)]
    # a skin file serves the mesh file's own vertices and topology
    rig_s, ply, npz = skin_files(tmp_path)
    obj = {"mesh": ply, "skin": npz, "path": PATH, "animation": {"cycle": 1.0, "loop": False}}
    plan = sim_with({"movers": {"objects": [obj]}})._mover_plan()
    got = plan["skins"][0]
    assert_bit_equal(got["rest"], rig_s.vertices.astype(F), "rest from the mesh file")
    assert_bit_equal(got["bone_weight"], rig_s.bone_weight, "weights from the skin file")
    assert (plan["clips"][0].K, plan["clips"][0].loop) == (8, False) and len(got["skeleton"]) == 6
    _, ply, npz = skin_files(tmp_path, skeleton=False)
    assert sim_with({"movers": {"objects": [obj]}})._mover_plan()["skins"][0]["skeleton"] is None


def test_simulator_skin_refusals(tmp_path):
    rig_s, ply, npz = skin_files(tmp_path)
    obj = {"mesh": ply, "skin": npz, "path": PATH, "animation": {"cycle": 1.0}}
    with pytest.raises(ValueError, match="skin and keyframes exclude each other"):
        sim_with({"movers": {"objects": [dict(obj, keyframes="x.npy")]}})._mover_plan()
    with pytest.raises(ValueError, match="skin needs an animation entry"):
        sim_with({"movers": {"objects": [{k: v for k, v in obj.items() if k != "animation"}]}})._mover_plan()
    # the refusals of `animation` apply as they are
    with pytest.raises(ValueError, match="animation is not available under motion.movers"):
        sim_with({"motion": {"speed": 1.0, "movers": {"objects": [RIG]}}})._mover_plan(nested=True)
    with pytest.raises(ValueError, match="flow is not available in a set with an animated mover"):
        sim_with({"movers": {"flow": True, "objects": [RIGID, RIG]}})._mover_plan()
    with pytest.raises(ValueError, match="flow is not available in a set with an animated mover"):
        sim_with({"movers": {"flow": True, "objects": [obj]}})._mover_plan()
    # what a skin file must hold
    np.savez(npz, bone_index=rig_s.bone_index, bone_weight=rig_s.bone_weight)
    with pytest.raises(ValueError, match="lacks \\['poses'\\]"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()
    np.savez(npz, bone_index=rig_s.bone_index[:50], bone_weight=rig_s.bone_weight, poses=rig_s.poses12)
    with pytest.raises(ValueError, match=r"bone_index \(V, 4\) uint8"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()
    np.savez(npz, bone_index=rig_s.bone_index.astype(np.int32), bone_weight=rig_s.bone_weight, poses=rig_s.poses12)
    with pytest.raises(ValueError, match=r"bone_index \(V, 4\) uint8"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()
    np.savez(npz, bone_index=rig_s.bone_index, bone_weight=rig_s.bone_weight, poses=rig_s.poses12[:, :, :11])
    with pytest.raises(ValueError, match=r"poses must be \(K, B, 12\)"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()
    np.savez(npz, bone_index=rig_s.bone_index, bone_weight=rig_s.bone_weight, poses=rig_s.poses12, parents=rig_s.skeleton.parents)
    with pytest.raises(ValueError, match="parents and joints together"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()
    np.savez(npz, bone_index=rig_s.bone_index, bone_weight=rig_s.bone_weight, poses=rig_s.poses12, parents=[-1, 0], joints=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="skeleton has 2 bones, its poses 6"):
        sim_with({"movers": {"objects": [obj]}})._mover_plan()
    np.save(str(tmp_path / "pickled.npy"), np.array([{"a": 1}], dtype=object), allow_pickle=True)
    with pytest.raises(ValueError):                                   # loaded with allow_pickle=False
        sim_with({"movers": {"objects": [dict(obj, skin=str(tmp_path / "pickled.npy"))]}})._mover_plan()


def test_tracks_file_carries_the_joints(tmp_path):
    from containers import S3DISSimScene
    _, ply, npz = skin_files(tmp_path, skeleton=False)
    bare = {"mesh": ply, "skin": npz, "instance": 1003, "path": [[0.0, 2.0, 2.0, 0.0, 45.0]], "animation": {"cycle": 0.8}}
    walk = dict(RIG, animation={"cycle": 0.8, "phase": 0.0})
    plan = sim_with({"movers": {"period": 0.05, "objects": [walk, RIGID, bare]}})._mover_plan()
    P = 4
    times = np.arange(P) * plan["period"]
    scene = S3DISSimScene("fab")
    scene.mover_tracks = {"period": plan["period"], "objects": plan["objects"], "times": times,
                          "states": np.stack([t.state(times) for t in plan["tracks"]], axis=1),
                          "poses12": np.stack([t.poses12(times) for t in plan["tracks"]], axis=1),
                          "shapes": {m: plan["clips"][m].shapes3(times) for m in (0, 2)}, "keyframes": {},
                          "skins": {m: plan["skins"][m] for m in (0, 2)}}

    class Frame:
        mover_ids = np.array([0, 1, 1, 2, 3], np.uint8)
    scene.frames = [Frame() for _ in range(P)]
    out = scene.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "fab_mover_tracks.json"))
    assert disk == json.loads(json.dumps(out))
    r = plan["skins"][0]
    keys = skin.keyframes(r["rest"], r["bone_index"], r["bone_weight"], r["poses12"])
    # x = t / 0.8 * 8 = 0, 0.5, 1, 1.5: knots and half-way blends
    assert [fr["movers"][0]["shape"] for fr in disk["frames"]] == [[0, 1, 0.0], [0, 1, 0.5], [1, 2, 0.0], [1, 2, 0.5]]
    joints = np.array([fr["movers"][0]["joints"] for fr in disk["frames"]])
    assert joints.shape == (P, 6, 3)
    for f, fr in enumerate(disk["frames"]):
        k0, k1, w = fr["movers"][0]["shape"]
        v = deform.blend(keys[k0], keys[k1], w).astype(np.float64)
        assert fr["movers"][0]["box7"][3:6] == [float(x) for x in (v.max(0) - v.min(0))]
        j0, j1 = r["skeleton"].joints(r["poses12"][k0]), r["skeleton"].joints(r["poses12"][k1])
        m12 = np.asarray(scene.mover_tracks["poses12"][f][0], np.float64).reshape(3, 4)
        want = (j0 + w * (j1 - j0)) @ m12[:, :3].T + m12[:, 3]
        assert np.array_equal(joints[f], want)
        assert "joints" not in fr["movers"][1] and "joints" not in fr["movers"][2]          # rigid; skinned without a skeleton
        assert fr["movers"][2]["shape"][:2] == fr["movers"][0]["shape"][:2]
    assert np.abs(joints[1] - joints[0]).max() > 0.01                  # the walker moves along its path
