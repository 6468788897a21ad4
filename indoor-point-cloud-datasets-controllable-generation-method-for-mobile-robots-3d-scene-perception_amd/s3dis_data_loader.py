#!/usr/bin/env python3
"""S3DIS room loading and preprocessing (reference: s3dis_data_loader.py), with the Open3D work on the GPU.

S3DISPreprocessor.preprocess_pointcloud runs the statistical outlier filter and the PCA normals of
lidarcast.preprocess_cloud (csrc/lrc_preprocess.hip) in one device call, where the reference calls Open3D's
remove_statistical_outlier and estimate_normals(KDTreeSearchParamHybrid).  Names, arguments, return values and the
pickle layout follow the reference, because the reconstruction stage reads the pickle.  Parity with Open3D itself
(neighbour tie order, summation order, eigenvector sign) is not pinned: Open3D is absent on every host this project
uses.

Reference behaviours kept on purpose:
- Label quirk (:96-107).  Open3D returns the INLIER indices, which the reference names outlier_indices and masks out
  of the labels, so the labels it returns belong to the REMOVED rows (and need not match the kept points in length).
  That is the default here too, so a labelled room fails at its first subsampled variant and main skips it, as the
  reference does; S3DISPreprocessor(config, kept_labels=True) (main: --kept_labels) returns the labels of the kept rows.
- use_shs_net: true falls back to the PCA normals: the module the reference imports for it does not exist there either.
- simulate_robot_sparsity and _simulate_occlusion draw from the GLOBAL np.random in the reference's call order, so
  np.random.seed(s) reproduces the reference's rows.
- Console output is not reproduced (as in s3dis_annotation_loader.py), and no plot is drawn: main accepts
  --save_normal_visualizations and ignores it, and the visualize_normals* methods raise NotImplementedError.
"""
import argparse
import pickle
import time
from pathlib import Path

import numpy as np

_PLOTS = "normal plots are out of scope (DESIGN.md section 9); write the normals with save_pointcloud_variants"


class S3DISLoader:
    """Loader for the S3DIS dataset layout <data_root>/<area>/<room>/."""

    def __init__(self, data_root: str):
        self.data_root = Path(data_root)
        self.area_names = [f"Area_{i}" for i in range(1, 7)]

    def load_room_data(self, area_name: str, room_name: str):
        """(points (N,3), colors (N,3) in [0, 1], labels (N,) int or None) from the first *.txt of the room folder
        (x y z r g b [label]), else from points.npy."""
        room_path = self.data_root / area_name / room_name
        if not room_path.exists():
            raise FileNotFoundError(f"Room data not found: {room_path}")
        txt_files = list(room_path.glob("*.txt"))
        if txt_files:
            data = np.loadtxt(txt_files[0])
        else:
            npy_file = room_path / "points.npy"
            if not npy_file.exists():
                raise FileNotFoundError(f"Point cloud data missing: {room_path}")
            data = np.load(npy_file)
        points = data[:, :3]
        colors = data[:, 3:6] / 255.0 if data.shape[1] >= 6 else np.ones((len(data), 3))
        labels = data[:, 6].astype(int) if data.shape[1] > 6 else None
        return points, colors, labels

    def get_available_rooms(self, area_name: str):
        """Sorted names of the room folders of an area ([] when the area does not exist)."""
        area_path = self.data_root / area_name
        if not area_path.exists():
            return []
        return sorted(d.name for d in area_path.iterdir() if d.is_dir())


class S3DISPreprocessor:
    """Outlier filter and normals of a room cloud, configured by the 'preprocessing' section of the YAML config."""

    def __init__(self, config_dict, ctx=None, kept_labels=False):
        self.config = config_dict["preprocessing"]
        self.kept_labels = bool(kept_labels)
        self._ctx = ctx

    def _context(self):
        if self._ctx is None:
            import lidarcast
            self._ctx = lidarcast.Context(0)
        return self._ctx

    def estimate_normals(self, points):
        """PCA normals of every row with the configured hybrid search (normal_search_radius, normal_max_nn)."""
        from lidarcast import preprocess
        return preprocess.estimate_normals(self._context(), points, radius=self.config["normal_search_radius"],
                                           max_nn=self.config["normal_max_nn"])

    def preprocess_pointcloud(self, points, colors=None, labels=None):
        """(processed_points, processed_colors, labels, normals), as the reference returns them (see the label quirk in
        the module docstring)."""
        from lidarcast import preprocess
        cfg = self.config
        points = np.asarray(points, dtype=np.float64)
        remove = bool(cfg["remove_outliers"])
        normals_on = bool(cfg["estimate_normals"])        # use_shs_net: PCA normals as well (see the module docstring)
        r = preprocess.preprocess_cloud(
            self._context(), points, remove_outliers=remove, nb_neighbors=cfg.get("outlier_nb_neighbors", 20),
            std_ratio=cfg.get("outlier_std_ratio", 2.0), estimate_normals=normals_on,
            radius=cfg.get("normal_search_radius", 0.1), max_nn=cfg.get("normal_max_nn", 30))
        if remove:
            ind = r.kept.astype(np.int64)
            if labels is not None:
                if self.kept_labels:
                    labels = labels[ind]
                else:
                    inlier_mask = np.ones(len(points), dtype=bool)
                    inlier_mask[ind] = False
                    labels = labels[inlier_mask]
            processed_points = points[ind]
            processed_colors = np.asarray(colors, dtype=np.float64)[ind] if colors is not None else None
        else:
            processed_points = points
            processed_colors = np.asarray(colors, dtype=np.float64) if colors is not None else None
        normals = r.normals if normals_on else None
        return processed_points, processed_colors, labels, normals

    def simulate_robot_sparsity(self, points, colors=None, labels=None, sparsity_config=None):
        """Random subsampling to keep_ratio, then the occlusion heuristic when sparsity_config['occlusion']."""
        if sparsity_config is None:
            return points, colors, labels
        if sparsity_config["keep_ratio"] < 1.0:
            n_keep = int(len(points) * sparsity_config["keep_ratio"])
            indices = np.random.choice(len(points), n_keep, replace=False)
            points = points[indices]
            if colors is not None:
                colors = colors[indices]
            if labels is not None:
                labels = labels[indices]
        if sparsity_config.get("occlusion", False):
            points, colors, labels = self._simulate_occlusion(points, colors, labels)
        return points, colors, labels

    def _simulate_occlusion(self, points, colors=None, labels=None, occlusion_ratio=0.3):
        """Rows within +-30 degrees elevation and 8 m of a robot 0.5 m above the floor centre; rows in the outer 10 %
        of x and of y each survive with probability 0.4.  occlusion_ratio is unused, as in the reference."""
        min_coords = np.min(points, axis=0)
        max_coords = np.max(points, axis=0)
        room_size = max_coords - min_coords
        robot_pos = np.array([(min_coords[0] + max_coords[0]) / 2, (min_coords[1] + max_coords[1]) / 2,
                              min_coords[2] + 0.5])
        rel_pos = points - robot_pos
        distances = np.linalg.norm(rel_pos, axis=1)
        elevation_angles = np.arctan2(rel_pos[:, 2], np.sqrt(rel_pos[:, 0] ** 2 + rel_pos[:, 1] ** 2))
        vertical_fov_mask = np.abs(elevation_angles) < np.radians(30)
        distance_mask = distances < 8.0
        corner_mask = np.ones(len(points), dtype=bool)
        for i in [0, 1]:
            corner_regions = [points[:, i] < min_coords[i] + room_size[i] * 0.1,
                              points[:, i] > max_coords[i] - room_size[i] * 0.1]
            for corner_region in corner_regions:
                corner_mask[corner_region] &= np.random.random(np.sum(corner_region)) > 0.6
        final_mask = vertical_fov_mask & distance_mask & corner_mask
        return (points[final_mask], colors[final_mask] if colors is not None else None,
                labels[final_mask] if labels is not None else None)

    def visualize_normals(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def visualize_normals_high_quality(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)

    def visualize_normal_statistics(self, *args, **kwargs):
        raise NotImplementedError(_PLOTS)


def save_processed_data(data_dict, output_path):
    """Pickle the room dict (the reconstruction stage's input)."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, "wb") as f:
        pickle.dump(data_dict, f)


def save_pointcloud_variants(room_data, output_dir, config):
    """<output_dir>/pointclouds/: the original, processed and every variant cloud as PLY (lidarcast.ply's Open3D
    layout), plus <area>_<room>_summary.txt."""
    from lidarcast.ply import write_point_cloud
    pointcloud_dir = Path(output_dir) / "pointclouds"
    pointcloud_dir.mkdir(parents=True, exist_ok=True)
    area_name = room_data["room_info"]["area_name"]
    room_name = room_data["room_info"]["room_name"]
    original_data = room_data["original_data"]
    write_point_cloud(pointcloud_dir / f"{area_name}_{room_name}_original.ply", original_data["points"],
                      colors=original_data["colors"])
    processed_data = room_data["processed_data"]
    write_point_cloud(pointcloud_dir / f"{area_name}_{room_name}_processed.ply", processed_data["points"],
                      colors=processed_data["colors"], normals=processed_data["normals"])
    for variant_name, variant_data in room_data["sparsity_variants"].items():
        write_point_cloud(pointcloud_dir / f"{area_name}_{room_name}_{variant_name}.ply", variant_data["points"],
                          colors=variant_data["colors"], normals=variant_data["normals"])
    summary_path = pointcloud_dir / f"{area_name}_{room_name}_summary.txt"
    with open(summary_path, "w", encoding="utf-8") as f:
        f.write(f"S3DIS point cloud summary - {area_name}/{room_name}\n")
        f.write("=" * 60 + "\n\n")
        f.write(f"Original cloud: {len(original_data['points'])} points\n")
        f.write(f"Processed cloud: {len(processed_data['points'])} points\n\n")
        f.write("Sparsity variants:\n")
        f.write("-" * 40 + "\n")
        for variant_name, variant_data in room_data["sparsity_variants"].items():
            cfg = variant_data["config"]
            f.write(f"{variant_name}:\n")
            f.write(f"  Points: {len(variant_data['points'])}\n")
            f.write(f"  Keep ratio: {cfg.get('keep_ratio', 1.0)}\n")
            f.write(f"  Occlusion simulation: {cfg.get('occlusion', False)}\n")
            f.write(f"  File: {area_name}_{room_name}_{variant_name}.ply\n\n")


def load_config(config_path):
    """YAML configuration (PyYAML is imported here only, so the package does not depend on it)."""
    import yaml
    with open(config_path, "r", encoding="utf-8") as f:
        return yaml.safe_load(f)


def _process_room(loader, preprocessor, config, area_name, room, output_dir, save_pointclouds):
    start_time = time.time()
    original_points, original_colors, original_labels = loader.load_room_data(area_name, room)
    processed_points, processed_colors, processed_labels, normals = preprocessor.preprocess_pointcloud(
        original_points, original_colors, original_labels)
    room_data = {
        "room_info": {"area_name": area_name, "room_name": room, "processing_time": time.time() - start_time},
        "original_data": {"points": original_points, "colors": original_colors, "labels": original_labels,
                          "point_count": len(original_points)},
        "processed_data": {"points": processed_points, "colors": processed_colors, "labels": processed_labels,
                           "normals": normals, "point_count": len(processed_points)},
        "sparsity_variants": {},
    }
    for sparsity_config in config["sparsity_experiments"]:
        if sparsity_config["name"] == "dense":
            sparse_points, sparse_colors, sparse_labels = processed_points, processed_colors, processed_labels
        else:
            sparse_points, sparse_colors, sparse_labels = preprocessor.simulate_robot_sparsity(
                processed_points, processed_colors, processed_labels, sparsity_config)
        if normals is not None and len(sparse_points) != len(processed_points):
            sparse_normals = preprocessor.estimate_normals(sparse_points)     # use_shs_net: the same PCA fallback
        else:
            sparse_normals = normals
        room_data["sparsity_variants"][sparsity_config["name"]] = {
            "points": sparse_points, "colors": sparse_colors, "labels": sparse_labels, "normals": sparse_normals,
            "point_count": len(sparse_points), "config": sparsity_config}
    save_processed_data(room_data, output_dir / f"{area_name}_{room}_preprocessed.pkl")
    if save_pointclouds:
        save_pointcloud_variants(room_data, output_dir, config)
    return room_data


def main(argv=None):
    """The reference's CLI: --config (YAML), --area_name / --room_name overrides, --save_pointclouds; the room list is
    the area's folders when room_name is empty.  --save_normal_visualizations is accepted and ignored (no plots);
    --kept_labels (not in the reference) returns the labels of the kept rows.  With the reference's label quirk a
    labelled room (7-column text) fails at its first subsampled variant (the removed rows' labels are indexed with the
    kept rows' sample), and is skipped, as in the reference.
    Writes <output_root>/preprocessed_data/<area>_<room>_preprocessed.pkl per room.  As in the reference, a room that
    fails is skipped (its error is not raised); returns {room: room_data} of the rooms that succeeded."""
    parser = argparse.ArgumentParser(description="S3DIS preprocessing utility")
    parser.add_argument("--config", type=str, required=True, help="Path to YAML configuration file")
    parser.add_argument("--area_name", type=str, help="Override area name from config")
    parser.add_argument("--room_name", type=str, help="Override room name from config")
    parser.add_argument("--save_pointclouds", action="store_true", help="Export individual point clouds to PLY")
    parser.add_argument("--save_normal_visualizations", action="store_true", help="Accepted; no plots are drawn")
    parser.add_argument("--kept_labels", action="store_true",
                        help="Return the labels of the kept rows (the reference returns those of the removed rows)")
    args = parser.parse_args(argv)
    config = load_config(args.config)
    if args.area_name:
        config["data"]["area_name"] = args.area_name
    if args.room_name:
        config["data"]["room_name"] = args.room_name
    loader = S3DISLoader(config["data"]["data_root"])
    preprocessor = S3DISPreprocessor(config, kept_labels=args.kept_labels)
    output_dir = Path(config["data"]["output_root"]) / "preprocessed_data"
    output_dir.mkdir(parents=True, exist_ok=True)
    area_name = config["data"]["area_name"]
    room_name = config["data"]["room_name"]
    rooms = [room_name] if room_name else loader.get_available_rooms(area_name)
    done = {}
    for room in rooms:
        try:
            done[room] = _process_room(loader, preprocessor, config, area_name, room, output_dir, args.save_pointclouds)
        except Exception:                                              # noqa: BLE001  (the reference skips the room)
            continue
    return done


if __name__ == "__main__":
    main()
