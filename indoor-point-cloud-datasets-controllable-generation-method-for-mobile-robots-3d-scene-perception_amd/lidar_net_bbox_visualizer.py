"""3-D detection annotations from a labelled scan cloud: the reference's LiDARNetBBoxVisualizer
(lidar_net_bbox_visualizer.py) with the same names and contracts, without Open3D.

The cloud is the file this package writes, combined_pointcloud_with_label.ply (float x, y, z; uchar r, g, b; ushort sem,
ins), read in one numpy call instead of one struct.unpack per vertex.  The statistical outlier filter (Open3D's
remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0)) and the boxes of all instances of a room run in ONE device
call (lidarcast.instance_boxes, csrc/lrc_boxes.hip); the box arithmetic, quality check and the Group-Free-3D JSON are
host float64, as in the reference.  The plotting methods and process_area are not provided."""
import json
import shutil
from pathlib import Path

import numpy as np

# the reference's default: LiDAR-Net semantic ids
LIDAR_NET_SEMANTIC_MAPPING = {"window": 15, "table": 18, "chair": 19, "sofa": 20, "bookcase": 23, "board": 21, "stairs": 10}
# the ids this simulator writes (S3DIS class list, s3dis_annotation_loader.py); S3DIS has no stairs class
S3DIS_SEMANTIC_MAPPING = {"window": 5, "table": 7, "chair": 8, "sofa": 9, "bookcase": 10, "board": 11}
# class names of the annotation file (Group-Free-3D vocabulary)
GROUPFREE_CLASSES = {"window": "window", "table": "table", "chair": "chair", "sofa": "sofa", "bookcase": "bookshelf",
                     "board": "picture", "stairs": "counter"}
OUTLIER_K = 20              # remove_outliers' defaults, which process_room_instances uses
OUTLIER_STD_RATIO = 2.0


class LiDARNetBBoxVisualizer:
    """Boxes per (class, instance) of a labelled cloud.  semantic_mapping: class name -> semantic id, in the order the
    classes are processed; None = the reference's LiDAR-Net ids, S3DIS_SEMANTIC_MAPPING for this simulator's output."""

    def __init__(self, semantic_mapping=None, ctx=None):
        self.detection_classes = set(LIDAR_NET_SEMANTIC_MAPPING)
        self.semantic_mapping = dict(LIDAR_NET_SEMANTIC_MAPPING if semantic_mapping is None else semantic_mapping)
        self.class_colors = {"window": [1.0, 0.0, 0.0], "table": [0.0, 0.0, 1.0], "chair": [1.0, 1.0, 0.0],
                             "sofa": [1.0, 0.0, 1.0], "bookcase": [0.0, 1.0, 1.0], "board": [1.0, 0.5, 0.0],
                             "stairs": [0.5, 0.0, 1.0]}
        self.bbox_params = {"min_points": 10, "min_volume": 0.001, "max_aspect_ratio": 10.0, "max_vis_points": 1000}
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            import lidarcast
            self._ctx = lidarcast.Context(0)
        return self._ctx

    # ---- input ----------------------------------------------------------------------------------------------
    def load_ply_file(self, ply_path):
        """dict of points (N,3) float64, colors (N,3) float64 in [0, 1], semantic_labels / instance_labels (N,) uint16
        and file_name; None for an empty or unreadable file."""
        from containers.s3dis_sim_scene import read_labeled_ply
        ply_path = Path(ply_path)
        try:
            rec = read_labeled_ply(ply_path)
        except Exception as e:          # the reference reports and skips a file it cannot read
            print(f"        [Error] Failed to load PLY {ply_path}: {e}")
            return None
        if rec is None or len(rec) == 0:
            return None
        points = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
        colors = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.float64) / 255.0
        return {"points": points, "colors": colors, "semantic_labels": np.array(rec["sem"]),
                "instance_labels": np.array(rec["ins"]), "file_name": ply_path.name}

    def extract_instances_by_semantic(self, room_data, target_semantic_id):
        """The instances of one class, ascending instance id; instance 0 and instances under min_points rows skipped."""
        rows = np.flatnonzero(room_data["semantic_labels"] == target_semantic_id)
        if len(rows) == 0:
            return []
        ins = room_data["instance_labels"][rows]
        colors = room_data["colors"]
        out = []
        for iid in np.unique(ins):
            if iid == 0:
                continue
            sel = rows[ins == iid]
            if len(sel) < self.bbox_params["min_points"]:
                continue
            out.append({"points": room_data["points"][sel], "colors": None if colors is None else colors[sel],
                        "instance_id": iid, "semantic_id": target_semantic_id})
        return out

    # ---- filter and boxes -----------------------------------------------------------------------------------------
    def remove_outliers(self, points, colors=None, k=OUTLIER_K, std_ratio=OUTLIER_STD_RATIO):
        """(filtered_points, filtered_colors) in row order; fewer than k points are returned unchanged.  One device call
        (the points are taken as float32: the precision of the PLY they come from)."""
        if len(points) < k:
            return points, colors
        import lidarcast
        n = len(points)
        _, _, keep = lidarcast.instance_boxes(self._context(), np.asarray(points, dtype=np.float32),
                                              np.zeros(n, np.uint16), np.ones(n, np.uint16), [0], min_points=1, k=k,
                                              std_ratio=std_ratio, return_rows=True)
        m = keep.astype(bool)
        return points[m], (None if colors is None else colors[m])

    @staticmethod
    def _bbox_from_extremes(min_coords, max_coords, point_count):
        size = max_coords - min_coords
        ordered = np.sort(size)
        return {"center": ((min_coords + max_coords) / 2).tolist(), "size": size.tolist(),
                "min_coords": min_coords.tolist(), "max_coords": max_coords.tolist(), "volume": float(np.prod(size)),
                "aspect_ratio": ordered[2] / ordered[0] if ordered[0] > 0 else float("inf"), "point_count": point_count}

    def calculate_bbox(self, points):
        if len(points) == 0:
            return None
        return self._bbox_from_extremes(points.min(axis=0), points.max(axis=0), len(points))

    def evaluate_bbox_quality(self, bbox, object_name):
        if bbox["volume"] < self.bbox_params["min_volume"]:
            return False, f"Volume too small: {bbox['volume']:.6f} < {self.bbox_params['min_volume']}"
        if bbox["aspect_ratio"] > self.bbox_params["max_aspect_ratio"]:
            return False, f"Aspect ratio too large: {bbox['aspect_ratio']:.2f} > {self.bbox_params['max_aspect_ratio']}"
        return True, "Quality check passed."

    def _class_ids(self):
        return list(dict.fromkeys(int(v) for v in self.semantic_mapping.values()))

    def _accepted(self, boxes, make_bbox):
        """The reference's loop order (classes in mapping order, instances by id) over the device's boxes: empty ones and
        those failing the quality check dropped, metadata attached."""
        out = []
        for name, sid in self.semantic_mapping.items():
            for b in boxes[boxes["sem"] == sid]:
                if b["num_kept"] == 0:
                    continue
                bbox = make_bbox(b)
                ok, _ = self.evaluate_bbox_quality(bbox, name)
                if not ok:
                    continue
                bbox.update(object_name=name, instance_id=np.uint16(b["ins"]), semantic_id=sid)
                out.append(bbox)
        return out

    def bboxes_from_boxes(self, boxes):
        """Accepted bbox dicts from lidarcast.instance_boxes / instance_boxes_dev output alone (no per-point arrays): the
        cloud never has to leave the device.  Same values as process_room_instances (the box is the float32 min / max)."""
        return self._accepted(boxes, lambda b: self._bbox_from_extremes(b["min3"].astype(np.float64),
                                                                       b["max3"].astype(np.float64), int(b["num_kept"])))

    def room_bboxes(self, room_data):
        """All accepted boxes of a room, with filtered_points / filtered_colors: one device call for every instance."""
        import lidarcast
        pts, sem, ins = room_data["points"], room_data["semantic_labels"], room_data["instance_labels"]
        colors = room_data["colors"]
        boxes, _, keep = lidarcast.instance_boxes(self._context(), np.asarray(pts, dtype=np.float32), sem, ins,
                                                  self._class_ids(), min_points=self.bbox_params["min_points"],
                                                  k=OUTLIER_K, std_ratio=OUTLIER_STD_RATIO, return_rows=True)
        kept = np.flatnonzero(keep)
        key = (sem[kept].astype(np.uint32) << 16) | ins[kept].astype(np.uint32)
        order = np.argsort(key, kind="stable")
        uniq, first = np.unique(key[order], return_index=True)
        groups = dict(zip(uniq.tolist(), np.split(kept[order], first[1:])))

        def make_bbox(b):
            rows = groups[(int(b["sem"]) << 16) | int(b["ins"])]
            bbox = self.calculate_bbox(pts[rows])
            bbox["filtered_points"] = pts[rows]
            bbox["filtered_colors"] = None if colors is None else colors[rows]
            return bbox
        return self._accepted(boxes, make_bbox)

    # ---- output -------------------------------------------------------------------------------------------------
    def process_room_instances(self, room_ply_path, output_dir=None):
        """Boxes of one room file; simulation_results/<stem>/<stem>_detection_annotations.json and a copy of the PLY,
        relative to the current directory.  None when the file is missing or unreadable or no box is accepted."""
        room_ply_path = Path(room_ply_path)
        if not room_ply_path.exists():
            print(f"  [Error] Room file does not exist: {room_ply_path}")
            return None
        room = self.load_ply_file(room_ply_path)
        if room is None:
            return None
        all_bboxes = self.room_bboxes(room)
        if not all_bboxes:
            return None
        scene_dir = Path("simulation_results") / room_ply_path.stem
        scene_dir.mkdir(parents=True, exist_ok=True)
        self.generate_detection_annotations(all_bboxes, scene_dir / f"{room_ply_path.stem}_detection_annotations.json")
        target = scene_dir / room_ply_path.name
        if not target.exists():
            try:
                shutil.copy2(room_ply_path, target)
            except Exception as e:
                print(f"  [Warning] Failed to copy PLY file: {e}")
        return all_bboxes

    def generate_detection_annotations(self, bboxes, output_path):
        """Group-Free-3D annotation file (json, indent 2), one entry per box in list order."""
        anns = []
        for i, b in enumerate(bboxes):
            name = b["object_name"]
            anns.append({
                "instance_id": i + 1, "class_name": GROUPFREE_CLASSES.get(name, name), "original_class_name": name,
                "bbox_3d": {"center": b["center"], "size": b["size"], "rotation": [0, 0, 0],
                            "min_coords": b["min_coords"], "max_coords": b["max_coords"]},
                "point_count": int(b["point_count"]), "volume": float(b["volume"]),
                "aspect_ratio": float(b["aspect_ratio"]), "confidence": 1.0, "bbox_format": "AABB",
                "coordinate_system": "world", "units": "meters", "framework": "Group-Free-3D"})
        meta = {"dataset": "LiDAR-Net", "annotation_type": "3D_object_detection", "framework": "Group-Free-3D",
                "classes": list(GROUPFREE_CLASSES.values()), "original_classes": list(GROUPFREE_CLASSES.keys()),
                "class_mapping": dict(GROUPFREE_CLASSES), "bbox_format": "AABB", "coordinate_system": "world",
                "units": "meters", "total_objects": len(anns), "compatible_with": ["Group-Free-3D", "VoteNet", "ScanNet"]}
        with open(output_path, "w", encoding="utf-8") as f:
            json.dump({"metadata": meta, "annotations": anns}, f, indent=2, ensure_ascii=False)
