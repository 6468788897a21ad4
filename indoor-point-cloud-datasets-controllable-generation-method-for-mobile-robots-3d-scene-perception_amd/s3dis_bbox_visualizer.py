#!/usr/bin/env python3
"""S3DIS ground-truth boxes from a room's Annotations/<class>_<k>.txt files (reference: s3dis_bbox_visualizer.py), with
the Open3D work on the GPU.

Each annotated object goes through Open3D's remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0) and the
axis-aligned box of the kept rows is judged and written to
simulation_results/<Area>_<room>/<Area>_<room>_detection_annotations.json.  Here the filter and the min / max of every
object of a room (visualize_room_bboxes) or of every room of an area (process_area) run in ONE device call,
lidarcast.object_boxes (csrc/lrc_objboxes.hip), through the single method filter_objects.  An object of 20 rows or more
gets exactly what lidarcast.preprocess_cloud's outlier stage computes for it alone; parity with Open3D itself (its
summation order) is not pinned: Open3D is absent on every host this project uses.

Names, tables, messages and return values follow the reference, and so do its quirks:
- files are taken in Path.glob order and rooms in iterdir order; object_name = stem.split('_')[0];
- np.loadtxt parses; a single-row file (a 1-D result), an empty or an unparsable file gives None and is skipped;
- an object whose filter keeps nothing is dropped; point_count is the kept count; instance_id is 1-based over the
  room's accepted boxes;
- the JSON goes to Path("simulation_results") under the working directory, whatever output_dir says;
- process_area draws np.random.choice(all_rooms, 5, replace=False) from the global stream when there are more than 5
  rooms and returns []; main's first-room mode writes the annotation file twice (simulation_results and output_dir).
Files of classes outside detection_classes are skipped before parsing (the output is the same).  Box arithmetic
(centre, size, np.prod volume, aspect ratio) stays on the host in the reference's numpy expressions, from the device's
float64 min / max.
Divergences: an object file with a non-finite value is skipped with a warning (Open3D's
behaviour on NaN is not pinned); the matplotlib plots and create_bbox_mesh (Open3D geometry) raise
NotImplementedError.
"""
import argparse
import json
import warnings
from pathlib import Path

import numpy as np

_PLOTS = "bounding-box plots and meshes are out of scope (DESIGN.md section 9); the annotation JSON is written"


class S3DISBBoxVisualizer:
    """S3DIS bounding box generator and visualizer."""

    def __init__(self, ctx=None):
        # Detection classes (excluding door)
        self.detection_classes = {
            'window', 'table', 'chair', 'sofa', 'bookcase', 'board', 'stairs'
        }

        # Class color mapping for visualization
        self.class_colors = {
            'window': [1.0, 0.0, 0.0],    # Red
            'table': [0.0, 0.0, 1.0],     # Blue
            'chair': [1.0, 1.0, 0.0],     # Yellow
            'sofa': [1.0, 0.0, 1.0],      # Magenta
            'bookcase': [0.0, 1.0, 1.0],  # Cyan
            'board': [1.0, 0.5, 0.0],     # Orange
            'stairs': [0.5, 0.0, 1.0]     # Purple
        }

        # Bounding box generation parameters
        self.bbox_params = {
            'min_points': 10,
            'min_volume': 0.001,
            'max_aspect_ratio': 10.0,
            'max_vis_points': 1000,  # Maximum points for visualization
        }
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            import lidarcast
            self._ctx = lidarcast.Context(0)
        return self._ctx

    # ---- the reference's host methods -------------------------------------------------------------------------------
    def load_annotation_file(self, annotation_file):
        """Load a single annotation file."""
        try:
            data = np.loadtxt(annotation_file)
            if len(data) == 0:
                return None
            points = data[:, :3]
            colors = data[:, 3:6] / 255.0 if data.shape[1] >= 6 else None
            labels = data[:, 6].astype(int) if data.shape[1] > 6 else None
            object_name = annotation_file.stem.split('_')[0]
            return {
                'points': points,
                'colors': colors,
                'labels': labels,
                'object_name': object_name,
                'file_name': annotation_file.name
            }
        except Exception:
            return None

    def remove_outliers(self, points, colors=None, k=20, std_ratio=2.0):
        """Statistical outlier removal of one object on the GPU: (filtered_points, filtered_colors)."""
        if len(points) < k:
            return points, colors
        import lidarcast
        r = lidarcast.object_boxes(self._context(), points, [0, len(points)], k=k, std_ratio=std_ratio)
        ind = r.kept_rows(0).astype(np.int64)
        filtered_points = np.asarray(points, dtype=np.float64)[ind]
        filtered_colors = np.asarray(colors, dtype=np.float64)[ind] if colors is not None else None
        return filtered_points, filtered_colors

    def calculate_bbox(self, points):
        """Calculate 3D bounding box."""
        if len(points) == 0:
            return None
        return self._bbox(points.min(axis=0), points.max(axis=0), len(points))

    @staticmethod
    def _bbox(min_coords, max_coords, point_count):
        center = (min_coords + max_coords) / 2
        size = max_coords - min_coords

        volume = float(np.prod(size))
        sorted_size = np.sort(size)
        aspect_ratio = sorted_size[2] / sorted_size[0] if sorted_size[0] > 0 else float('inf')

        return {
            'center': center,
            'size': size,
            'min_coords': min_coords,
            'max_coords': max_coords,
            'volume': volume,
            'aspect_ratio': aspect_ratio,
            'point_count': point_count
        }

    def evaluate_bbox_quality(self, bbox, object_name):
        """Evaluate bounding box quality."""
        if object_name not in self.detection_classes:
            return False, f"Class {object_name} not in detection set"
        if bbox['point_count'] < self.bbox_params['min_points']:
            return False, f"Insufficient points: {bbox['point_count']} < {self.bbox_params['min_points']}"
        if bbox['volume'] < self.bbox_params['min_volume']:
            return False, f"Volume too small: {bbox['volume']:.6f} < {self.bbox_params['min_volume']}"
        if bbox['aspect_ratio'] > self.bbox_params['max_aspect_ratio']:
            return False, f"Aspect ratio too large: {bbox['aspect_ratio']:.2f} > {self.bbox_params['max_aspect_ratio']}"
        return True, "Quality OK"

    def load_room_point_cloud(self, room_path):
        """Load point cloud data for an entire room."""
        room_files = list(room_path.glob("*.txt"))
        if not room_files:
            return None
        room_file = room_files[0]
        try:
            data = np.loadtxt(room_file)
            if len(data) == 0:
                return None
            points = data[:, :3]
            colors = data[:, 3:6] / 255.0 if data.shape[1] >= 6 else None
            labels = data[:, 6].astype(int) if data.shape[1] > 6 else None
            return {
                'points': points,
                'colors': colors,
                'labels': labels,
                'file_name': room_file.name
            }
        except Exception:
            return None

    # ---- the device call and the room flow around it ----------------------------------------------------------------
    def filter_objects(self, point_sets, k=20, std_ratio=2.0):
        """remove_outliers + min / max of every object at once: one (min3, max3, num_kept) per (m, 3) float64 array of
        point_sets, in order (min3 = +inf, max3 = -inf, num_kept = 0 when the filter kept nothing).  The only place the
        room and area flow reaches the device."""
        if not point_sets:
            return []
        import lidarcast
        sizes = np.array([len(p) for p in point_sets], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        r = lidarcast.object_boxes(self._context(), np.concatenate(point_sets, axis=0), off, k=k, std_ratio=std_ratio)
        return [(np.array(b["min3"], dtype=np.float64), np.array(b["max3"], dtype=np.float64), int(b["num_kept"]))
                for b in r.boxes]

    def _room_objects(self, room_path):
        """The room's detection-class objects in glob order (None without an Annotations folder)."""
        annotations_dir = room_path / "Annotations"
        if not annotations_dir.exists():
            return None
        objects = []
        for txt_file in list(annotations_dir.glob("*.txt")):
            if txt_file.stem.split('_')[0] not in self.detection_classes:
                continue                                  # skipped by the reference after parsing: same output
            data = self.load_annotation_file(txt_file)
            if data is None:
                continue
            if not np.isfinite(data['points']).all():
                warnings.warn(f"{txt_file}: non-finite coordinates, object skipped")
                continue
            objects.append(data)
        return objects

    def _room_bboxes(self, room_path, objects, results):
        """The reference's per-object checks and the room's JSON, from filter_objects' results."""
        bboxes = []
        for data, (lo, hi, kept) in zip(objects, results):
            if kept == 0:
                continue
            bbox_info = self._bbox(lo, hi, kept)
            is_suitable, reason = self.evaluate_bbox_quality(bbox_info, data['object_name'])
            if not is_suitable:
                continue
            bbox_info['object_name'] = data['object_name']
            bbox_info['file_name'] = data['file_name']
            bbox_info['room_name'] = room_path.name
            bboxes.append(bbox_info)

        if not bboxes:
            return None

        simulation_results_dir = Path("simulation_results")
        simulation_results_dir.mkdir(parents=True, exist_ok=True)
        area_name = room_path.parent.name
        room_name = room_path.name
        scene_name = f"{area_name}_{room_name}"
        scene_dir = simulation_results_dir / scene_name
        if not scene_dir.exists():
            scene_dir.mkdir(parents=True, exist_ok=True)
        json_path = scene_dir / f"{scene_name}_detection_annotations.json"
        self.generate_detection_annotations(bboxes, json_path)
        return bboxes

    def visualize_room_bboxes(self, room_path, output_dir=None):
        """Boxes of a single room (one device call for all its objects); writes the room's annotation JSON."""
        objects = self._room_objects(room_path)
        if objects is None:
            return None
        results = self.filter_objects([d['points'] for d in objects])
        return self._room_bboxes(room_path, objects, results)

    def process_area(self, area_path, output_dir=None):
        """Every room of the area in one device call; writes each room's JSON.  Returns [] as the reference does (its
        visualisation selection is commented out), after the same draw from the global np.random stream."""
        if not area_path.exists():
            return None

        all_rooms = [d for d in area_path.iterdir() if d.is_dir()]

        if len(all_rooms) > 5:
            selected_rooms_for_vis = np.random.choice(all_rooms, 5, replace=False).tolist()  # noqa: F841
        else:
            selected_rooms_for_vis = all_rooms  # noqa: F841

        rooms = [(room, self._room_objects(room)) for room in all_rooms]
        flat = [d['points'] for _, objects in rooms if objects for d in objects]
        results = iter(self.filter_objects(flat))
        all_room_bboxes = []
        for room, objects in rooms:
            if objects is None:
                continue
            room_bboxes = self._room_bboxes(room, objects, [next(results) for _ in objects])
            if room_bboxes:
                all_room_bboxes.extend(room_bboxes)

        selected_bboxes = []
        return selected_bboxes

    def generate_detection_annotations(self, bboxes, output_path):
        """Generate detection annotation file (compatible with Group-Free-3D)."""
        class_name_mapping = {
            'window': 'window',
            'table': 'table',
            'chair': 'chair',
            'sofa': 'sofa',
            'bookcase': 'bookshelf',
            'board': 'picture',
            'stairs': 'counter'  # Stairs -> counter (closest category)
        }

        detection_annotations = []

        for i, bbox in enumerate(bboxes):
            original_class = bbox['object_name']
            groupfree_class = class_name_mapping.get(original_class, original_class)
            ann = {
                'instance_id': i + 1,
                'class_name': groupfree_class,
                'original_class_name': original_class,
                'bbox_3d': {
                    'center': bbox['center'].tolist(),
                    'size': bbox['size'].tolist(),
                    'rotation': [0, 0, 0],
                    'min_coords': bbox['min_coords'].tolist(),
                    'max_coords': bbox['max_coords'].tolist()
                },
                'point_count': bbox['point_count'],
                'volume': bbox['volume'],
                'aspect_ratio': bbox['aspect_ratio'],
                'confidence': 1.0,
                'bbox_format': 'AABB',
                'coordinate_system': 'world',
                'units': 'meters',
                'framework': 'Group-Free-3D'
            }
            detection_annotations.append(ann)

        annotation_file = {
            'metadata': {
                'dataset': 'S3DIS',
                'annotation_type': '3D_object_detection',
                'framework': 'Group-Free-3D',
                'classes': list(class_name_mapping.values()),
                'original_classes': list(class_name_mapping.keys()),
                'class_mapping': class_name_mapping,
                'bbox_format': 'AABB',
                'coordinate_system': 'world',
                'units': 'meters',
                'total_objects': len(detection_annotations),
                'compatible_with': ['Group-Free-3D', 'VoteNet', 'ScanNet']
            },
            'annotations': detection_annotations
        }

        with open(output_path, 'w', encoding='utf-8') as f:
            json.dump(annotation_file, f, indent=2, ensure_ascii=False)

        print(f"[Annotation] Saved {len(detection_annotations)} annotations to: {output_path}")
        return detection_annotations

    # ---- out of scope -----------------------------------------------------------------------------------------------
    def create_bbox_mesh(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def create_area_summary_visualization(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def plot_area_bboxes_3d(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def draw_bbox_3d(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def draw_bbox_2d(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def plot_area_bboxes_2d(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def plot_area_statistics(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)


def main(argv=None):
    """Main function."""
    parser = argparse.ArgumentParser(description="S3DIS bounding box generation and visualization tool (headless version)")
    parser.add_argument("--data_root", type=str, required=True, help="S3DIS dataset root directory")
    parser.add_argument("--area_name", type=str, help="Specify area name (e.g., Area_1)")
    parser.add_argument("--room_name", type=str, help="Specify room name (e.g., office_1)")
    parser.add_argument("--output_dir", type=str, default=None, help="Output directory")
    parser.add_argument("--process_all_areas", action="store_true", help="Process all areas")

    args = parser.parse_args(argv)

    data_root = Path(args.data_root)
    if not data_root.exists():
        print(f"[Error] Data root directory does not exist: {data_root}")
        return

    visualizer = S3DISBBoxVisualizer()

    if args.output_dir:
        output_dir = Path(args.output_dir)
    else:
        output_dir = data_root / "bbox_visualization_results"

    output_dir.mkdir(parents=True, exist_ok=True)

    if args.process_all_areas:
        print("[Main] Processing all areas...")
        area_names = [f"Area_{i}" for i in range(1, 7)]
        total_bboxes = 0

        for area_name in area_names:
            area_path = data_root / area_name
            if area_path.exists():
                area_bboxes = visualizer.process_area(area_path, output_dir)
                if area_bboxes:
                    total_bboxes += len(area_bboxes)
            else:
                print(f"[Main] Area {area_name} does not exist")

        print(f"[Main] All areas processed. Total bounding boxes: {total_bboxes}")

    elif args.area_name and args.room_name:
        room_path = data_root / args.area_name / args.room_name
        if room_path.exists():
            bboxes = visualizer.visualize_room_bboxes(room_path, None)
            if bboxes:
                print(f"[Main] Room processed: {len(bboxes)} bounding boxes")
            else:
                print("[Main] No valid bounding boxes in room")
        else:
            print(f"[Main] Room does not exist: {room_path}")

    elif args.area_name:
        area_path = data_root / args.area_name
        if area_path.exists():
            area_bboxes = visualizer.process_area(area_path, output_dir)
            if area_bboxes:
                print(f"[Main] Area processed: {len(area_bboxes)} bounding boxes")
            else:
                print("[Main] No valid bounding boxes in area")
        else:
            print(f"[Main] Area does not exist: {area_path}")

    else:
        area_names = [f"Area_{i}" for i in range(1, 7)]

        for area_name in area_names:
            area_path = data_root / area_name
            if area_path.exists():
                rooms = [d for d in area_path.iterdir() if d.is_dir()]
                if rooms:
                    test_room = rooms[0]
                    bboxes = visualizer.visualize_room_bboxes(test_room, output_dir)
                    if bboxes:
                        ann_path = output_dir / f"{area_name}_{test_room.name}_detection_annotations.json"
                        visualizer.generate_detection_annotations(bboxes, ann_path)
                        print(f"[Main] Room processed: {len(bboxes)} bounding boxes")
                    else:
                        print("[Main] No valid bounding boxes in room")
                    break


if __name__ == "__main__":
    main()
