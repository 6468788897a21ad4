#!/usr/bin/env python3
"""Capture golden values of the REFERENCE's detection-box helpers (run in the build container only).

    python tests/golden/make_bbox_golden.py        # writes tests/golden/bbox_golden.json

Imports /root/reference/lidar_net_bbox_visualizer.py (never copied) with an empty stand-in for ``open3d``: the methods
recorded here are pure numpy and run verbatim -- calculate_bbox (:227-249), evaluate_bbox_quality (:251-259),
extract_instances_by_semantic (:163-201) and the bytes generate_detection_annotations (:358-420) writes.  Inputs are
seeded and stored in the file next to the results."""
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

sys.modules.setdefault("open3d", types.ModuleType("open3d"))
spec = importlib.util.spec_from_file_location("ref_lidar_net_bbox_visualizer", os.path.join(REF, "lidar_net_bbox_visualizer.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
vis = ref.LiDARNetBBoxVisualizer()


def corners(size, lo=(0.0, 0.0, 0.0)):
    lo = np.asarray(lo, np.float64)
    hi = lo + np.asarray(size, np.float64)
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])


rng = np.random.default_rng(2024)
clouds = {
    "random": rng.normal([1.0, 2.0, 0.5], [0.3, 0.2, 0.4], (200, 3)).astype(np.float32).astype(np.float64),
    "planar_z": np.column_stack([rng.uniform(0, 1, 50), rng.uniform(0, 2, 50), np.full(50, 0.75)]),
    "single_point": np.array([[0.5, -1.25, 2.0]]),
    "line_x": np.column_stack([rng.uniform(-1, 1, 20), np.zeros(20), np.zeros(20)]),
    "volume_at_limit": corners((0.1, 0.1, 0.1)),
    "volume_below_limit": corners((0.1, 0.1, 0.0999)),
    "aspect_at_limit": corners((1.0, 1.0, 10.0), (2.0, 3.0, 0.0)),
    "aspect_above_limit": corners((1.0, 1.0, 10.0001)),
    "negative_coords": corners((0.4, 0.7, 0.9), (-3.0, -2.5, -0.1)),
}
out = {"clouds": {k: v.tolist() for k, v in clouds.items()}, "bbox": {}, "quality": {}}
for name, pts in clouds.items():
    b = vis.calculate_bbox(pts)
    out["bbox"][name] = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in b.items()}
    ok, why = vis.evaluate_bbox_quality(b, "chair")
    out["quality"][name] = [bool(ok), why]

# one room: three classes, instance 0, instances of 9 / 10 / 19 / 20 points, ids out of order, a class not in the mapping
sizes = {(19, 3): 20, (19, 1): 9, (19, 7): 10, (19, 0): 15, (18, 2): 19, (18, 5): 30, (15, 4): 12, (2, 1): 40,
         (23, 9): 5}
sem, ins = [], []
for (s, i), n in sizes.items():
    sem += [s] * n
    ins += [i] * n
perm = rng.permutation(len(sem))
room = {"points": rng.uniform(0, 4, (len(sem), 3)).astype(np.float32).astype(np.float64),
        "colors": rng.integers(0, 256, (len(sem), 3)).astype(np.float64) / 255.0,
        "semantic_labels": np.array(sem, np.uint16)[perm], "instance_labels": np.array(ins, np.uint16)[perm]}
out["room"] = {k: v.tolist() for k, v in room.items()}
out["instances"] = {}
for sid in (19, 18, 15, 23, 2, 99):
    inst = vis.extract_instances_by_semantic(room, sid)
    out["instances"][str(sid)] = [{"instance_id": int(d["instance_id"]), "semantic_id": int(d["semantic_id"]),
                                   "points": d["points"].tolist(), "colors": d["colors"].tolist()} for d in inst]

# annotation file bytes: boxes of every class name (one unknown), an infinite aspect ratio among them
bboxes = []
for name, cname in zip(clouds, ["chair", "table", "window", "sofa", "bookcase", "board", "stairs", "lamp", "chair"]):
    b = vis.calculate_bbox(clouds[name])
    b.update(object_name=cname, instance_id=np.uint16(3), semantic_id=19)
    bboxes.append(b)
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "ann.json")
    with redirect_stdout(io.StringIO()):
        vis.generate_detection_annotations(bboxes, path)
        vis.generate_detection_annotations([], os.path.join(d, "empty.json"))
    out["annotation_names"] = list(clouds)
    out["annotation_classes"] = [b["object_name"] for b in bboxes]
    out["annotation_bytes"] = open(path, "rb").read().decode("utf-8")
    out["annotation_bytes_empty"] = open(os.path.join(d, "empty.json"), "rb").read().decode("utf-8")
with open(os.path.join(HERE, "bbox_golden.json"), "w") as f:
    json.dump(out, f)
print("wrote", os.path.getsize(os.path.join(HERE, "bbox_golden.json")), "bytes")
