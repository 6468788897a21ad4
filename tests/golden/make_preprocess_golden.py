#!/usr/bin/env python3
"""Capture golden values of the REFERENCE's preprocessing helpers (run in the build container only).

    python tests/golden/make_preprocess_golden.py     # writes tests/golden/preprocess_golden.json

Imports /root/reference/s3dis_data_loader.py (never copied) with a stand-in ``open3d``: its PointCloud stores what it is
given, remove_statistical_outlier returns a given inlier list, estimate_normals and write_point_cloud only record their
calls.  What is recorded here is the reference's own numpy code run verbatim: load_room_data on 6- and 7-column text
and on points.npy, get_available_rooms, seeded simulate_robot_sparsity with and without occlusion, the labels
preprocess_pointcloud returns (the inlier / outlier quirk) and the summary file save_pointcloud_variants writes.
Inputs are seeded and stored in the file next to the results."""
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np  # noqa: E402

WRITTEN = []
INLIERS = []


class _PointCloud:
    def __init__(self):
        self.points, self.colors, self.normals = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))

    def has_colors(self):
        return len(self.colors) > 0

    def remove_statistical_outlier(self, nb_neighbors, std_ratio):
        ind = list(INLIERS)
        clean = _PointCloud()
        clean.points = np.asarray(self.points)[ind]
        if self.has_colors():
            clean.colors = np.asarray(self.colors)[ind]
        return clean, ind

    def estimate_normals(self, search_param=None):
        self.normals = np.tile([0.0, 0.0, 1.0], (len(self.points), 1))


o3d = types.ModuleType("open3d")
o3d.geometry = types.SimpleNamespace(PointCloud=_PointCloud, KDTreeSearchParamHybrid=lambda **kw: kw)
o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a, dtype=np.float64))
o3d.io = types.SimpleNamespace(write_point_cloud=lambda path, pcd: WRITTEN.append(os.path.basename(path)))
sys.modules["open3d"] = o3d
spec = importlib.util.spec_from_file_location("ref_s3dis_data_loader", os.path.join(REF, "s3dis_data_loader.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

rng = np.random.default_rng(77)
out = {}
with tempfile.TemporaryDirectory() as d, redirect_stdout(io.StringIO()):
    # ---- loader: 7-column text, 6-column text, points.npy, rooms of an area ----
    pts = np.round(rng.uniform(0, 5, (40, 3)), 3)
    rgb = rng.integers(0, 256, (40, 3)).astype(np.float64)
    lab = rng.integers(0, 13, (40, 1)).astype(np.float64)
    for room, data in (("office_1", np.hstack([pts, rgb, lab])), ("office_2", np.hstack([pts, rgb]))):
        os.makedirs(os.path.join(d, "Area_1", room))
        np.savetxt(os.path.join(d, "Area_1", room, f"{room}.txt"), data, fmt="%.3f %.3f %.3f %d %d %d" +
                   (" %d" if data.shape[1] == 7 else ""))
    os.makedirs(os.path.join(d, "Area_1", "hallway_3"))
    npy = np.hstack([pts[:10], rgb[:10], lab[:10]])
    np.save(os.path.join(d, "Area_1", "hallway_3", "points.npy"), npy)
    open(os.path.join(d, "Area_1", "notes.md"), "w").close()                 # a file, not a room
    loader = ref.S3DISLoader(d)
    out["room_data"] = {"pts": pts.tolist(), "rgb": rgb.tolist(), "lab": lab[:, 0].tolist()}
    out["loaded"] = {}
    for room in ("office_1", "office_2", "hallway_3"):
        p, c, l = loader.load_room_data("Area_1", room)
        out["loaded"][room] = {"points": p.tolist(), "colors": c.tolist(), "labels": None if l is None else l.tolist()}
    out["rooms"] = loader.get_available_rooms("Area_1")
    out["rooms_missing_area"] = loader.get_available_rooms("Area_9")

    # ---- seeded sparsity, with and without occlusion ----
    cfg = {"preprocessing": {"remove_outliers": True, "outlier_nb_neighbors": 20, "outlier_std_ratio": 2.0,
                             "estimate_normals": False, "normal_search_radius": 0.1, "normal_max_nn": 30}}
    pre = ref.S3DISPreprocessor(cfg)
    room_pts = rng.uniform([0, 0, 0], [6, 4, 3], (500, 3))
    room_rgb = rng.uniform(0, 1, (500, 3))
    room_lab = rng.integers(0, 13, 500)
    out["sparsity_input"] = {"points": room_pts.tolist(), "colors": room_rgb.tolist(), "labels": room_lab.tolist()}
    out["sparsity"] = {}
    for name, sc in (("sparse_50", {"name": "sparse_50", "keep_ratio": 0.5, "occlusion": False}),
                     ("occluded_70", {"name": "occluded_70", "keep_ratio": 0.7, "occlusion": True}),
                     ("occluded_full", {"name": "occluded_full", "keep_ratio": 1.0, "occlusion": True})):
        np.random.seed(1234)
        p, c, l = pre.simulate_robot_sparsity(room_pts, room_rgb, room_lab, sc)
        out["sparsity"][name] = {"config": sc, "points": p.tolist(), "colors": c.tolist(), "labels": l.tolist()}

    # ---- the labels preprocess_pointcloud returns: those of the REMOVED rows ----
    INLIERS[:] = sorted(rng.choice(500, 460, replace=False).tolist())
    p, c, l, n = pre.preprocess_pointcloud(room_pts, room_rgb, room_lab)
    out["quirk"] = {"inliers": list(INLIERS), "points": p.tolist(), "labels": l.tolist(), "normals": n}

    # ---- summary file of save_pointcloud_variants ----
    WRITTEN.clear()
    room_data = {"room_info": {"area_name": "Area_1", "room_name": "office_1", "processing_time": 0.5},
                 "original_data": {"points": room_pts, "colors": room_rgb, "labels": room_lab, "point_count": 500},
                 "processed_data": {"points": p, "colors": c, "labels": l, "normals": None, "point_count": len(p)},
                 "sparsity_variants": {k: {"points": np.asarray(v["points"]), "colors": np.asarray(v["colors"]),
                                           "labels": np.asarray(v["labels"]), "normals": None,
                                           "point_count": len(v["points"]), "config": v["config"]}
                                       for k, v in out["sparsity"].items()}}
    room_data["sparsity_variants"]["dense"] = {"points": p, "colors": c, "labels": l, "normals": None,
                                               "point_count": len(p), "config": {"name": "dense"}}
    ref.save_pointcloud_variants(room_data, os.path.join(d, "out"), {})
    out["summary_bytes"] = open(os.path.join(d, "out", "pointclouds", "Area_1_office_1_summary.txt"), "rb").read().decode("utf-8")
    out["written"] = list(WRITTEN)
with open(os.path.join(HERE, "preprocess_golden.json"), "w") as f:
    json.dump(out, f)
print("wrote", os.path.getsize(os.path.join(HERE, "preprocess_golden.json")), "bytes")
