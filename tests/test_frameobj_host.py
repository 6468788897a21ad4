"""CPU: per-frame object annotations -- the numpy restatement against records worked out by hand,
FrameObjectsResult.boxes7 against the closed form, the JSON of S3DISSimulator.export_frame_annotations on a stub engine
result, and the C symbols."""
import json
import os

import numpy as np
import pytest

import frameobj_restate as R
from conftest import REPO
from helpers import pose

INF = np.inf


def _signbit_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the restatement on hand-made records ----------------------------------------------------------------------------
def _hand_mesh():
    return R.hand_made_case()[0]


def test_restatement_on_hand_made_records():
    (v, f, sem, ins), M, (t, prim, pts) = R.hand_made_case()
    tab = R.object_table(v, f, sem, ins)
    assert tab["key"].tolist() == [7 | 1 << 16, 8 | 2 << 16]
    assert tab["obj"].tolist() == [0, 0, 1, 1] and tab["tri_count"].tolist() == [2, 2]
    assert tab["q"].tolist() == [1 << 31, 1 << 32, 1 << 31, 1 << 33]
    assert tab["total_q"].tolist() == [(1 << 31) + (1 << 32), (1 << 31) + (1 << 33)]
    assert tab["wmin"].tolist() == [[0, 0, 0], [-4, -1, 0]] and tab["wmax"].tolist() == [[2, 1, 0], [1, 1, 0]]
    out = R.restate(tab, t, prim, pts, M[None], 6)
    assert out["returns"].tolist() == [[3, 0]] == R.HAND_MADE_RESULT["returns"]
    assert out["seen_tris"].tolist() == [[2, 0]] == R.HAND_MADE_RESULT["seen_tris"]
    assert out["seen_q"].tolist() == [[(1 << 31) + (1 << 32), 0]] == R.HAND_MADE_RESULT["seen_q"]
    assert _signbit_equal(out["vmin"], [[[-0.0, -0.5, -2.0], [INF, INF, INF]]])
    assert _signbit_equal(out["vmax"], [[[0.0, 1.0, 0.5], [-INF, -INF, -INF]]])
    assert _signbit_equal(out["vmin"], R.HAND_MADE_RESULT["vmin"]) and _signbit_equal(out["vmax"], R.HAND_MADE_RESULT["vmax"])
    assert np.signbit(out["vmin"][0, 0, 0]) and not np.signbit(out["vmax"][0, 0, 0])
    assert out["rejected_rays"] == 0
    # the same frame again doubles returns and nothing else; a non-finite point of a returned ray is rejected
    st = R.new_state(1, tab)
    R.accumulate(st, tab, t, prim, pts, M[None], 6)
    pts2 = pts.copy()
    pts2[4, 1] = np.inf
    R.accumulate(st, tab, t, prim, pts2, M[None], 6)
    twice = R.finish(st, tab)
    assert twice["returns"].tolist() == [[5, 0]] and twice["rejected_rays"] == 1
    for name in ("seen_tris", "seen_q", "vmin", "vmax"):
        assert _signbit_equal(twice[name].astype(np.float64), out[name].astype(np.float64)), name


def test_restatement_rotated_pose_and_label_defaults():
    v, f, sem, ins = _hand_mesh()
    assert R.object_table(v, f)["key"].tolist() == [0]                        # no labels: one object, key 0
    assert R.object_table(v, f, sem, None)["key"].tolist() == [7, 8]
    M = pose(1.0, 2.0, 3.0, 0.7)
    x = np.array([[2.0, 2.0, 3.0]], np.float32)                               # e = (1, 0, 0) -> s = R^T e = (cos, -sin, 0)
    s = R.sensor_coords(M, x)
    assert np.allclose(s, [[np.cos(0.7), -np.sin(0.7), 0.0]], rtol=0, atol=1e-16)


# ---- boxes7 ----------------------------------------------------------------------------------------------------------
def _result(K=1, F=1, **kw):
    from lidarcast import FrameObjectsResult
    d = dict(key=np.zeros(K, np.uint32), tri_count=np.ones(K, np.uint32), total_q=np.full(K, 1 << 32, np.uint64),
             wmin=np.zeros((K, 3)), wmax=np.ones((K, 3)), returns=np.zeros((F, K), np.uint32),
             seen_tris=np.zeros((F, K), np.uint32), seen_q=np.zeros((F, K), np.uint64),
             vmin=np.full((F, K, 3), INF), vmax=np.full((F, K, 3), -INF))
    d.update(kw)
    return FrameObjectsResult(**d)


def test_boxes7_closed_form_and_tilt_refusal():
    r = _result(wmin=np.array([[1.0, 2.0, 0.0]]), wmax=np.array([[3.0, 3.0, 1.0]]))
    M = pose(0.5, 0.5, 1.0, 0.7)
    b = r.boxes7(M[None])
    assert b.shape == (1, 1, 7)
    c, s = np.cos(0.7), np.sin(0.7)
    ex, ey, ez = 2.0 - 0.5, 2.5 - 0.5, 0.5 - 1.0
    assert np.abs(b[0, 0, :3] - [c * ex + s * ey, -s * ex + c * ey, ez]).max() <= 1e-12
    assert b[0, 0, 3:6].tolist() == [2.0, 1.0, 1.0]                           # exact
    assert abs(b[0, 0, 6] - (-0.7)) <= 1e-15
    tilt = np.eye(4)
    a = 0.2
    tilt[1, 1], tilt[1, 2], tilt[2, 1], tilt[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    with pytest.raises(ValueError):
        r.boxes7(tilt[None])
    with pytest.raises(ValueError):
        r.boxes7(np.stack([M, M]))                                            # one pose per frame


def test_seen_ratio_is_zero_for_zero_area():
    r = _result(K=2, total_q=np.array([0, 1 << 32], np.uint64), seen_q=np.array([[0, 1 << 31]], np.uint64))
    assert r.seen_ratio.tolist() == [[0.0, 0.5]]
    assert r.sem.dtype == np.uint16 and r.ins.dtype == np.uint16


# ---- the simulator layer on a stub engine result ----------------------------------------------------------------------
class _StubEngine:
    def __init__(self, result):
        self.result, self.calls = result, 0

    def frame_objects(self, intrinsics, poses, mesh, max_range=None, chunk_poses=None):
        self.calls += 1
        assert np.asarray(poses).shape == (2, 4, 4)
        return self.result


def _stub_sim(result):
    from containers import RoomBounds, S3DISScene
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast import synth
    from s3dis_simulator import S3DISSimulator
    sim = S3DISSimulator.__new__(S3DISSimulator)              # no engine construction: that needs a GPU
    sim.config = {}
    mesh = synth.unit_cube()
    sim.scene = S3DISScene("stubroom", mesh, RoomBounds.from_vertices(mesh.vertices))
    sim.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
    sim.raycast_engine = _StubEngine(result)
    return sim


def test_export_frame_annotations_json_shape_and_filters(tmp_path):
    from trajectory import line_trajectory, poses_from_waypoints
    # objects: table (7) ins 1; chair (8) ins 0; wall (2) ins 3; chair (8) ins 2
    key = np.array([7 | 1 << 16, 8 | 0 << 16, 2 | 3 << 16, 8 | 2 << 16], np.uint32)
    order = np.argsort(key)
    key = key[order]
    K = 4
    returns = np.array([[50, 60, 70, 9], [3, 0, 0, 10]], np.uint32)[:, order]
    vmin = np.full((2, K, 3), INF)
    vmax = np.full((2, K, 3), -INF)
    vmin[returns > 0], vmax[returns > 0] = -1.0, 1.0
    r = _result(K=K, F=2, key=key, returns=returns, vmin=vmin, vmax=vmax, wmin=np.zeros((K, 3)),
                wmax=np.tile([1.0, 2.0, 3.0], (K, 1)), total_q=np.full(K, 1 << 33, np.uint64),
                seen_q=(returns.astype(np.uint64) << np.uint64(20)), tri_count=np.full(K, 12, np.uint32))
    sim = _stub_sim(r)
    wps = line_trajectory((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), 2)
    d = sim.export_frame_annotations(wps, tmp_path, min_points=10)
    path = tmp_path / "stubroom_frame_annotations.json"
    assert json.loads(path.read_text()) == d and sim.raycast_engine.calls == 1
    assert d["scene_name"] == "stubroom" and d["num_frames"] == 2 and d["min_points"] == 10
    assert [o["key"] for o in d["objects"]] == key.tolist()
    tab = {o["key"]: o for o in d["objects"]}
    t = tab[7 | 1 << 16]
    assert (t["sem"], t["ins"], t["class"], t["tri_count"], t["area_m2"]) == (7, 1, "table", 12, 2.0)
    assert t["world_min"] == [0, 0, 0] and t["world_max"] == [1, 2, 3]
    assert tab[2 | 3 << 16]["class"] == "wall"
    poses = poses_from_waypoints(wps)
    assert np.array_equal(np.array(d["frames"][0]["pose"]), np.asarray(poses[0], np.float64))
    # frame 0: the table (50 points) is listed; chair ins 0 (ins == 0), the wall (class not mapped) and chair ins 2
    # (9 < min_points) are not.  frame 1: the table has 3 points, chair ins 2 has 10
    f0, f1 = d["frames"]
    assert [(o["class"], o["ins"], o["num_points"]) for o in f0["objects"]] == [("table", 1, 50)]
    assert [(o["class"], o["ins"], o["num_points"]) for o in f1["objects"]] == [("chair", 2, 10)]
    o = f0["objects"][0]
    assert set(o) == {"object", "class", "sem", "ins", "num_points", "seen_ratio", "box7", "visible_min", "visible_max"}
    assert len(o["box7"]) == 7 and o["box7"][3:6] == [1.0, 2.0, 3.0]
    assert o["seen_ratio"] == float(50 << 20) / float(1 << 33)
    assert o["visible_min"] == [-1.0] * 3 and o["visible_max"] == [1.0] * 3
    assert d["objects"][o["object"]]["key"] == 7 | 1 << 16
    # a custom mapping lists other classes; min_points is honoured
    d2 = sim.export_frame_annotations(wps, tmp_path, min_points=1, semantic_mapping={"wall": 2})
    assert [[(o["class"], o["num_points"]) for o in f["objects"]] for f in d2["frames"]] == [[("wall", 70)], []]


def test_export_frame_annotations_refuses_motion(tmp_path):
    from trajectory import line_trajectory
    sim = _stub_sim(_result())
    sim.config["motion"] = {"speed": 0.5}
    with pytest.raises(NotImplementedError):
        sim.export_frame_annotations(line_trajectory((0, 0, 0), (1, 0, 0), 2), tmp_path)
    assert sim.raycast_engine.calls == 0 and not list(tmp_path.iterdir())


# ---- symbols ---------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lrc_frameobj_create", "lrc_frameobj_destroy", "lrc_frameobj_get_info", "lrc_frameobj_objects",
               "lrc_frameobj_reset", "lrc_frameobj_accumulate_dev", "lrc_frameobj_export", "lrc_frameobj_export_dev")


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes as C
    import lidarcast
    from lidarcast import _capi
    hdr = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    lib = lidarcast.load()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and (name + "(") in hdr, name
        assert hasattr(lib, name), f"liblidarcast.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, name
    assert C.sizeof(_capi.LrcFrameobjInfo) == 40
    assert lidarcast.FrameObjects.__name__ == "FrameObjects" and "FrameObjectsResult" in lidarcast.__all__
