"""Scene assembly: frames -> statistics -> combined cloud -> result files
(reference: containers/s3dis_sim_scene.py; class and method names, file names and file contents follow it --
tests/golden/make_containers_golden.py runs the reference's own classes for the fixtures).

Differences from the reference, all on purpose:
  * labels come from the hit triangles (written back by the trace kernel) when the frames carry
    them, instead of a 1-NN query against the raw annotated cloud at export time;
    without labels the reference's defaults apply (grey 0.5 -> 127, labels 0, :575-584); with an annotated
    cloud attached (``set_annotated_cloud``) the reference's 1-NN assignment runs, on the GPU;
  * the labelled PLY is written with one structured-array ``tofile`` instead of a per-point
    ``struct.pack`` loop; header and record layout are byte-identical (:619-641);
  * ``combined_pointcloud.ply`` is written by this package's own PLY writer (the reference hands it to Open3D);
  * the ``_load_s3dis_*`` hooks read the annotation files through this package's ``s3dis_annotation_loader`` (same
    names and results as the reference's module) and, like the reference, report "no data" on any failure.
"""
import json
import os
import pickle
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional

import numpy as np

from .s3dis_sim_frame import S3DISSimFrame


class NumpyEncoder(json.JSONEncoder):
    """numpy scalars and arrays as plain JSON numbers / lists."""

    def default(self, obj):
        if isinstance(obj, np.integer):
            return int(obj)
        if isinstance(obj, np.floating):
            return float(obj)
        if isinstance(obj, np.ndarray):
            return obj.tolist()
        return super().default(obj)


@dataclass
class SimulationStats:
    total_frames: int
    total_points: int
    average_coverage: float
    average_scan_density: float
    average_incident_angle: float
    average_range: float
    simulation_time: float
    frames_per_second: float

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)


class ResultExporter:
    """Writes frames, statistics and the summary below one output directory (reference :57-130: same file names,
    same text)."""

    _STAT_LINES = (("Total frames", "total_frames", ""), ("Total points", "total_points", ""),
                   ("Average coverage", "average_coverage", ".3f"),
                   ("Average scan density", "average_scan_density", ".3f"),
                   ("Average incident angle", "average_incident_angle", ".3f"),
                   ("Average range", "average_range", ".3f"))

    def __init__(self, output_dir: Path):
        self.output_dir = Path(output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)

    def export_frames(self, frames: List[S3DISSimFrame], format: str = "pkl"):
        if format not in ("pkl", "json"):
            raise ValueError(f"Unsupported format: {format}")
        frames_dir = self.output_dir / "frames"
        frames_dir.mkdir(exist_ok=True)
        for frame in frames:
            path = frames_dir / f"frame_{frame.frame_index:04d}.{format}"
            if format == "pkl":
                with open(path, "wb") as f:
                    pickle.dump(frame.to_dict(), f)
            else:
                with open(path, "w") as f:
                    json.dump(frame.to_dict(), f, indent=2, cls=NumpyEncoder)

    def export_statistics(self, stats: SimulationStats, format: str = "json"):
        if format == "json":
            with open(self.output_dir / "simulation_statistics.json", "w") as f:
                json.dump(stats.to_dict(), f, indent=2, cls=NumpyEncoder)
        elif format == "txt":
            lines = ["Simulation Statistics", "=" * 50]
            lines += [f"{label}: {format_spec(getattr(stats, attr), spec)}" for label, attr, spec in self._STAT_LINES]
            lines += [f"Simulation time: {stats.simulation_time:.3f}s",
                      f"Frames per second: {stats.frames_per_second:.3f} FPS"]
            with open(self.output_dir / "simulation_statistics.txt", "w") as f:
                f.write("\n".join(lines) + "\n")
        else:
            raise ValueError(f"Unsupported format: {format}")

    def export_summary(self, sim_scene: "S3DISSimScene", format: str = "json"):
        if format != "json":
            raise ValueError(f"Unsupported format: {format}")
        summary = {
            "scene_name": sim_scene.scene_name,
            "simulation_config": sim_scene.simulation_config,
            "statistics": sim_scene.statistics.to_dict(),
            "frame_summary": {
                "frame_indices": [f.frame_index for f in sim_scene.frames],
                "point_counts": [f.get_num_points() for f in sim_scene.frames],
                "coverage_ratios": [f.get_coverage_ratio() for f in sim_scene.frames],
            },
        }
        with open(self.output_dir / "simulation_summary.json", "w") as f:
            json.dump(summary, f, indent=2, cls=NumpyEncoder)


def format_spec(value, spec):
    return format(value, spec) if spec else str(value)


PLY_HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
              b"property float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
              b"property ushort sem\nproperty ushort ins\nend_header\n")
PLY_RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                       ("blue", "u1"), ("sem", "<u2"), ("ins", "<u2")])   # 19 bytes, packed


def write_labeled_ply(path, points, colors_u8, semantic_labels, instance_labels):
    """8-attribute binary PLY of the reference (float x,y,z; uchar r,g,b; ushort sem, ins)."""
    n = len(points)
    rec = np.empty(n, dtype=PLY_RECORD)
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rec["red"], rec["green"], rec["blue"] = colors_u8[:, 0], colors_u8[:, 1], colors_u8[:, 2]
    rec["sem"], rec["ins"] = semantic_labels, instance_labels
    with open(path, "wb") as f:
        f.write(PLY_HEADER % n)
        rec.tofile(f)


def read_labeled_ply(path):
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline()
            if line.startswith(b"element vertex"):
                n = int(line.split()[-1])
            if line.strip() == b"end_header":
                break
        return np.fromfile(f, dtype=PLY_RECORD, count=n)


class S3DISSimScene:
    """All frames of one simulated scene."""

    def __init__(self, scene_name: str, simulation_config: Optional[Dict[str, Any]] = None,
                 mesh: Optional[object] = None, s3dis_data_root: Optional[str] = None,
                 area: Optional[str] = None, room: Optional[str] = None):
        self.scene_name = scene_name
        self.simulation_config = simulation_config or {}
        self.frames: List[S3DISSimFrame] = []
        self.statistics: Optional[SimulationStats] = None
        self.exporter: Optional[ResultExporter] = None
        self.mesh = mesh
        self.s3dis_data_root, self.area, self.room = s3dis_data_root, area, room
        self._s3dis_cache = None      # the reference's cache slot (dict of the four annotated arrays)
        self._annotated = None        # (points f64 (M,3), colors (M,3) in 0..1, sem (M,), ins (M,))
        self._nn = None
        # the movers key of the simulator: {period, objects, times (P,), states (P, M, 4): x, y, z, yaw,
        # poses12 (P, M, 12), sensor_poses (P, 4, 4)} of the run, None without the key
        self.mover_tracks = None

    def append_frame(self, frame: S3DISSimFrame):
        self.frames.append(frame)

    def get_total_frames(self) -> int:
        return len(self.frames)

    def get_total_points(self) -> int:
        return sum(f.get_num_points() for f in self.frames)

    def _mean(self, getter) -> float:
        return np.mean([getter(f) for f in self.frames]) if self.frames else 0.0

    def get_average_coverage(self) -> float:
        return self._mean(S3DISSimFrame.get_coverage_ratio)

    def get_average_scan_density(self) -> float:
        return self._mean(S3DISSimFrame.get_scan_density)

    def get_average_incident_angle(self) -> float:
        return self._mean(S3DISSimFrame.get_mean_incident_angle)

    def get_average_range(self) -> float:
        return self._mean(S3DISSimFrame.get_mean_range)

    def get_frame_statistics(self) -> Dict[str, List[float]]:
        """Per-frame series (empty dict without frames)."""
        if not self.frames:
            return {}
        series = (("frame_indices", lambda f: f.frame_index), ("point_counts", S3DISSimFrame.get_num_points),
                  ("coverage_ratios", S3DISSimFrame.get_coverage_ratio),
                  ("scan_densities", S3DISSimFrame.get_scan_density),
                  ("incident_angles", S3DISSimFrame.get_mean_incident_angle),
                  ("ranges", S3DISSimFrame.get_mean_range))
        return {name: [get(f) for f in self.frames] for name, get in series}

    def get_quality_distribution(self) -> Dict[str, Any]:
        """mean / std / min / max of the coverage, point-count and incident-angle series."""
        if not self.frames:
            return {}
        per_frame = self.get_frame_statistics()

        def four(v):
            return {"mean": np.mean(v), "std": np.std(v), "min": np.min(v), "max": np.max(v)}
        return {"coverage_distribution": four(per_frame["coverage_ratios"]),
                "point_count_distribution": four(per_frame["point_counts"]),
                "incident_angle_distribution": four(per_frame["incident_angles"])}

    def compute_statistics(self, simulation_time: float = 0.0):
        n = self.get_total_frames()
        self.statistics = SimulationStats(
            total_frames=n, total_points=self.get_total_points(),
            average_coverage=self.get_average_coverage(),
            average_scan_density=self.get_average_scan_density(),
            average_incident_angle=self.get_average_incident_angle(),
            average_range=self.get_average_range(),
            simulation_time=simulation_time if n else 0.0,
            frames_per_second=n / simulation_time if (n and simulation_time > 0) else 0.0)

    # ---- assembly ---------------------------------------------------------------------------------
    def combined_points(self) -> np.ndarray:
        """np.vstack of the non-empty frames in frame order (reference :326, :362)."""
        parts = [f.points for f in self.frames if len(f.points) > 0]
        return np.vstack(parts) if parts else np.empty((0, 3), dtype=np.float32)

    def combined_labels(self):
        sem, ins = [], []
        for f in self.frames:
            k = len(f.points)
            if k == 0:
                continue
            sem.append(f.semantic_labels if f.semantic_labels is not None else np.zeros(k, np.uint16))
            ins.append(f.instance_labels if f.instance_labels is not None else np.zeros(k, np.uint16))
        if not sem:
            return np.empty(0, np.uint16), np.empty(0, np.uint16)
        return np.concatenate(sem).astype(np.uint16), np.concatenate(ins).astype(np.uint16)

    # ---- export-time labels from an annotated cloud (the reference's semantics) -------------------------
    def set_annotated_cloud(self, points, colors, semantic_labels, instance_labels):
        """The arrays the reference reads from the S3DIS annotations and caches
        (containers/s3dis_sim_scene.py:396-409).  Loading the annotation files is out of scope here."""
        self._annotated = (np.ascontiguousarray(points, dtype=np.float64), np.asarray(colors),
                           np.asarray(semantic_labels), np.asarray(instance_labels))
        if self._nn is not None:
            self._nn.close()
        self._nn = None

    def _get_default_colors_and_labels(self, num_points: int):
        return (np.ones((num_points, 3), dtype=np.float32) * 0.5, np.zeros(num_points, dtype=np.uint16),
                np.zeros(num_points, dtype=np.uint16))

    def _ensure_annotations(self):
        """The reference's lazy load of the room's annotation files (:392-409), tried once per scene, when
        s3dis_data_root / area / room are configured and no cloud was attached by hand."""
        if (self._annotated is None and self._s3dis_cache is None and self.s3dis_data_root and self.area
                and self.room):
            self._s3dis_cache = {}
            pts, cols, sem, ins = self._load_s3dis_annotations_with_colors()
            if pts is not None and len(pts) > 0:
                self.set_annotated_cloud(pts, cols, sem, ins)
                self._s3dis_cache = {"points": pts, "colors": cols, "labels": sem, "instances": ins}

    def _get_colors_and_labels_from_s3dis(self, points: np.ndarray):
        """Nearest annotated point per hit point -> (colors, semantic, instance); defaults without a cloud.
        Same contract as the reference method of this name (:379-427); the ball-tree query is the GPU 1-NN."""
        self._ensure_annotations()
        if self._annotated is None or len(points) == 0:
            return self._get_default_colors_and_labels(len(points))
        if self._nn is None:
            import lidarcast
            self._nn_ctx = lidarcast.Context(0)
            self._nn = lidarcast.NearestIndex(self._nn_ctx, self._annotated[0])
        idx = self._nn.query(points)
        _, colors, sem, ins = self._annotated
        return colors[idx], sem[idx], ins[idx]

    # ---- result files (reference :249-337, :339-377, :614-641) ---------------------------------------------
    def save_results(self, output_dir: Path, formats: List[str] = ["pkl", "txt"]):
        """Statistics (json and/or txt), summary (json, else the plain-text one), combined_pointcloud.ply and
        combined_pointcloud_with_label.ply below output_dir.  As in the reference the statistics are recomputed
        here with simulation_time 0, and per-frame files are not written."""
        output_dir = Path(output_dir)
        self.exporter = ResultExporter(output_dir)
        self.compute_statistics()
        for fmt in formats:
            if fmt in ("json", "txt"):
                self.exporter.export_statistics(self.statistics, fmt)
        if "json" in formats:
            self.exporter.export_summary(self, "json")
        elif "txt" in formats:
            self._save_simple_summary(output_dir)
        self._export_combined_pointcloud(output_dir)
        self._export_combined_pointcloud_with_labels(output_dir)

    def _save_simple_summary(self, output_dir: Path):
        lines = ["S3DIS Simulation Results Summary", "=" * 50, "",
                 f"Scene name: {self.scene_name}",
                 f"Total frames: {len(self.frames)}",
                 f"Total points: {self.get_total_points():,}",
                 f"Average coverage: {self.get_average_coverage():.3f}",
                 f"Average scan density: {self.get_average_scan_density():.3f}",
                 f"Average incident angle: {self.get_average_incident_angle():.1f}\u00b0",
                 f"Average range: {self.get_average_range():.2f}m"]
        if self.statistics:
            lines += ["", "Simulation Statistics:",
                      f"  Simulation time: {self.statistics.simulation_time:.2f}s",
                      f"  Frame rate: {self.statistics.frames_per_second:.1f} FPS"]
        lines += ["", "Frame Details:", "-" * 30]
        lines += [f"Frame {i + 1:2d}: {f.get_num_points():5d} points, coverage {f.get_coverage_ratio():.3f}, "
                  f"density {f.get_scan_density():.3f}" for i, f in enumerate(self.frames)]
        with open(Path(output_dir) / "simulation_summary.txt", "w", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")

    def _export_combined_pointcloud(self, output_dir: Path):
        """combined_pointcloud.ply: all frames' points, every frame in its own viridis colour i / num_frames
        (:306-337).  Written as binary PLY with double coordinates and uchar colours, the layout Open3D gives a
        PointCloud, by this package's writer."""
        parts, cols = [], []
        for i, frame in enumerate(self.frames):
            if len(frame.points) > 0:
                parts.append(frame.points)
                cols.append(np.tile(_viridis(i / len(self.frames)), (len(frame.points), 1)))
        if not parts:
            return
        from lidarcast.ply import write_point_cloud
        write_point_cloud(Path(output_dir) / "combined_pointcloud.ply", np.vstack(parts).astype(np.float64),
                          colors=np.vstack(cols))

    def _export_combined_pointcloud_with_labels(self, output_dir: Path):
        """combined_pointcloud_with_label.ply: np.vstack of the non-empty frames with colour, semantic and instance
        label per point (:339-377)."""
        cloud = self._labelled_cloud()
        if cloud is not None:
            self._save_labeled_ply(Path(output_dir) / "combined_pointcloud_with_label.ply", *cloud)

    def _labelled_cloud(self):
        """(points, colours uint8, sem, ins) of combined_pointcloud_with_label.ply; None without points."""
        pts = self.combined_points()
        if len(pts) == 0:
            return None
        has_frame_labels = any(f.semantic_labels is not None for f in self.frames if len(f.points) > 0)
        # With the annotation source configured (the reference's normal wiring, :379-427) the files decide colours and
        # labels, also when the frames carry the hit triangles' labels: load them before choosing the branch.
        self._ensure_annotations()
        if self._annotated is not None or not has_frame_labels:
            # the reference's path: per frame, colours and labels of the nearest annotated point, or its defaults
            cols, sems, inss = [], [], []
            for f in self.frames:
                if len(f.points) > 0:
                    c, s_, i_ = self._get_colors_and_labels_from_s3dis(f.points)
                    cols.append(c); sems.append(s_); inss.append(i_)
            colors = (np.vstack(cols) * 255).astype(np.uint8)
            sem, ins = np.concatenate(sems), np.concatenate(inss)
        else:                                 # labels written back by the trace kernel; the reference's default grey
            sem, ins = self.combined_labels()
            colors = np.full((len(pts), 3), int(0.5 * 255), dtype=np.uint8)
        return pts, colors, sem, ins

    def export_detection_annotations(self, output_dir: Path, semantic_mapping=None):
        """The detection annotations lidar_net_bbox_visualizer.py derives from combined_pointcloud_with_label.ply, without
        writing the cloud: output_dir/combined_pointcloud_with_label_detection_annotations.json (the name the reference
        tool gives it).  semantic_mapping: class name -> semantic id, default S3DIS_SEMANTIC_MAPPING (the ids this
        simulator writes).  Returns the accepted bbox dicts, or None (no points, or no box accepted; no file then)."""
        from lidar_net_bbox_visualizer import S3DIS_SEMANTIC_MAPPING, LiDARNetBBoxVisualizer
        cloud = self._labelled_cloud()
        if cloud is None:
            return None
        pts, colors, sem, ins = cloud
        vis = LiDARNetBBoxVisualizer(S3DIS_SEMANTIC_MAPPING if semantic_mapping is None else semantic_mapping)
        # the coordinates as the PLY holds them (float32), so that the boxes are those of the written file
        bboxes = vis.room_bboxes({"points": np.asarray(pts, np.float32).astype(np.float64), "colors": colors / 255.0,
                                  "semantic_labels": np.asarray(sem, np.uint16), "instance_labels": np.asarray(ins, np.uint16)})
        if not bboxes:
            return None
        Path(output_dir).mkdir(parents=True, exist_ok=True)
        vis.generate_detection_annotations(bboxes, Path(output_dir) / "combined_pointcloud_with_label_detection_annotations.json")
        return bboxes

    def export_mover_tracks(self, output_dir) -> Dict[str, Any]:
        """Ground truth of the moving objects of a run under the movers key, written to ``output_dir``/<scene>_mover_tracks.json:
        the period, the object table (mesh, semantic, instance, the mesh's own box) and, per frame and mover, the time, the
        pose (x, y, z, yaw_deg and the row-major 3 x 4 object-to-world matrix), the oriented box (``box7``: world centre,
        extents of the mesh's own AABB, heading = yaw) and ``num_points``, the frame's returns from that mover.  An animated
        mover (``animation`` entry) also carries ``shape``: [k0, k1, w] of the frame, and its box is that of the frame's own
        blended vertices.  A skinned mover with a skeleton also carries ``joints``: its B joint positions at the frame's shape in
        world coordinates -- the joints under key pose k0 and under k1 blended with w in float64 (j0 + w (j1 - j0)), then taken
        out by the mover's pose.  Under the
        nested key ``motion: {movers: ...}`` (movers that move while a sweep is scanned) ``pose`` is the pose at the START of the
        frame's sweep, every mover additionally carries ``end_pose`` (x, y, z, yaw_deg at the END of the sweep) and ``record24``
        (the mover sweep record the scan used), and every frame ``sweep_duration`` in seconds.  With ``per_ray_shape: true``
        there an animated mover's ``shape`` is the shape at the START of the sweep and it additionally carries ``end_shape``,
        [k0, k1, w] at its END, and a rig with a skeleton ``end_joints``, the joints at the end shape taken out by the end pose.  Under ``movers: {noise: ...}``
        and under ``motion: {movers: {sensor_noise: ...}}`` (seeded sensor noise drawn in the mover kernels) the file additionally holds the noise model -- ``noise``: seed,
        range_std, angle_std_deg, dropout and first_frame (frame f has frame id first_frame + f) -- and every frame ``returns``,
        its kept noisy returns (static_points plus every mover's num_points).  Returns the dict."""
        tr = self.mover_tracks
        if tr is None:
            raise ValueError("this scene was not simulated under the movers key")
        objs = tr["objects"]
        frames = []
        for f, frame in enumerate(self.frames):
            ids = getattr(frame, "mover_ids", None)
            if ids is None:
                raise ValueError(f"frame {f} carries no mover_ids")
            counts = np.bincount(np.asarray(ids, dtype=np.int64), minlength=len(objs) + 1)
            movers = []
            for m, obj in enumerate(objs):
                x, y, z, yaw = (float(v) for v in tr["states"][f][m])
                lo, hi = np.asarray(obj["box_min"], np.float64), np.asarray(obj["box_max"], np.float64)
                shape = joints = None
                if m in tr.get("shapes", {}):       # an animated mover: the box of the frame's own blended vertices (host blend)
                    from lidarcast.deform import blend
                    shape = [float(v) for v in tr["shapes"][m][f]]
                    rig = tr.get("skins", {}).get(m)
                    if rig is not None:         # a skinned mover: its two key poses skinned on the host (lidarcast.skin.apply)
                        from lidarcast import skin
                        k0 = skin.apply(rig["rest"], rig["bone_index"], rig["bone_weight"], rig["poses12"][int(shape[0])])
                        k1 = k0 if shape[1] == shape[0] else \
                            skin.apply(rig["rest"], rig["bone_index"], rig["bone_weight"], rig["poses12"][int(shape[1])])
                        if rig.get("skeleton") is not None:
                            j0, j1 = (rig["skeleton"].joints(rig["poses12"][int(k)]) for k in shape[:2])
                            m12 = np.asarray(tr["poses12"][f][m], np.float64).reshape(3, 4)
                            joints = (j0 + shape[2] * (j1 - j0)) @ m12[:, :3].T + m12[:, 3]
                    else:
                        k0, k1 = tr["keyframes"][m][int(shape[0])], tr["keyframes"][m][int(shape[1])]
                    verts = blend(k0, k1, shape[2]).astype(np.float64)
                    lo, hi = verts.min(0), verts.max(0)
                c, s = np.cos(yaw), np.sin(yaw)
                mid = 0.5 * (lo + hi)
                centre = np.array([c * mid[0] - s * mid[1] + x, s * mid[0] + c * mid[1] + y, mid[2] + z])
                movers.append({"mover": m + 1, "instance": obj["instance"], "semantic": obj["semantic"],
                               "pose": {"x": x, "y": y, "z": z, "yaw_deg": float(np.degrees(yaw)),
                                        "matrix12": [float(v) for v in tr["poses12"][f][m]]},
                               "box7": [float(v) for v in centre] + [float(v) for v in (hi - lo)] + [yaw],
                               "num_points": int(counts[m + 1])})
                if shape is not None:
                    movers[-1]["shape"] = [int(shape[0]), int(shape[1]), shape[2]]
                if joints is not None:
                    movers[-1]["joints"] = [[float(v) for v in j] for j in joints]
                if "end_states" in tr:
                    ex, ey, ez, eyaw = (float(v) for v in tr["end_states"][f][m])
                    movers[-1]["end_pose"] = {"x": ex, "y": ey, "z": ez, "yaw_deg": float(np.degrees(eyaw))}
                    movers[-1]["record24"] = [float(v) for v in tr["records24"][f][m]]
                if m in tr.get("end_shapes", {}):       # per-ray shape: the shape at the end of the sweep
                    end = [float(v) for v in tr["end_shapes"][m][f]]
                    movers[-1]["end_shape"] = [int(end[0]), int(end[1]), end[2]]
                    rig = tr.get("skins", {}).get(m)
                    if rig is not None and rig.get("skeleton") is not None:
                        from lidarcast.movers import pose12
                        j0, j1 = (rig["skeleton"].joints(rig["poses12"][int(k)]) for k in end[:2])
                        e12 = pose12(tr["end_states"][f][m]).astype(np.float64).reshape(3, 4)
                        ej = (j0 + end[2] * (j1 - j0)) @ e12[:, :3].T + e12[:, 3]
                        movers[-1]["end_joints"] = [[float(v) for v in j] for j in ej]
            frames.append({"frame": f, "time": float(tr["times"][f]), "static_points": int(counts[0]), "movers": movers})
            if "end_states" in tr:
                frames[-1]["sweep_duration"] = float(tr["sweep_duration"])
            if tr.get("noise") is not None:
                frames[-1]["returns"] = int(len(ids))
        summary = {"scene_name": self.scene_name, "period": float(tr["period"]), "num_frames": len(frames), "objects": objs,
                   "frames": frames}
        if tr.get("noise") is not None:
            nz = tr["noise"]
            summary["noise"] = {"seed": int(nz.seed), "range_std": float(nz.range_std),
                                "angle_std_deg": float(np.degrees(nz.angle_std)), "dropout": float(nz.dropout),
                                "first_frame": int(nz.first_frame)}
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / f"{self.scene_name}_mover_tracks.json", "w") as fh:
            json.dump(summary, fh, indent=2)
        return summary

    def export_scene_flow(self, output_dir) -> Dict[str, Any]:
        """Scene-flow ground truth of a run under ``movers: {..., flow: true}``, written to ``output_dir``/<scene>_scene_flow.npz:
        ``points`` (K, 3) float32 of all frames stacked, ``flow`` (K, 3) float32 (world displacement of the surface under the
        point up to the next frame), ``status`` (K,) uint8 (0 no next frame, 1 visible from the next pose, 2 occluded, 3 out of
        range), ``mover_ids`` (K,) uint8, ``frame_offsets`` (F + 1,) int64 (frame f = rows [offsets[f], offsets[f + 1])),
        ``sensor_poses`` (F, 4, 4) float64, ``mover_poses12`` (F, M, 12) float32 and ``times`` (F,).  A run under
        ``nonrigid_flow: true`` with animated movers adds ``animated_movers`` (D,) int64, their places among the movers, and
        ``mover_shapes`` (F, D, 3) float64, each one's [k0, k1, w] per frame.  Returns the arrays."""
        tr = self.mover_tracks
        if tr is None:
            raise ValueError("this scene was not simulated under the movers key")
        cols = {"points": [], "flow": [], "status": [], "mover_ids": []}
        for f, frame in enumerate(self.frames):
            if getattr(frame, "flow", None) is None or getattr(frame, "flow_status", None) is None:
                raise ValueError(f"frame {f} carries no flow: the movers key needs flow: true")
            pts = np.asarray(frame.points, np.float32).reshape(-1, 3)
            rows = {"points": pts, "flow": np.asarray(frame.flow, np.float32).reshape(-1, 3),
                    "status": np.asarray(frame.flow_status, np.uint8).reshape(-1),
                    "mover_ids": np.asarray(frame.mover_ids, np.uint8).reshape(-1)}
            if any(len(a) != len(pts) for a in rows.values()):
                raise ValueError(f"frame {f}: points, flow, flow_status and mover_ids differ in length")
            for k, a in rows.items():
                cols[k].append(a)
        empty = {"points": (0, 3), "flow": (0, 3), "status": (0,), "mover_ids": (0,)}
        out = {k: np.concatenate(v) if v else np.zeros(empty[k], np.float32 if len(empty[k]) == 2 else np.uint8)
               for k, v in cols.items()}
        out["frame_offsets"] = np.concatenate([[0], np.cumsum([len(a) for a in cols["points"]])]).astype(np.int64)
        out["sensor_poses"] = np.asarray(tr["sensor_poses"], np.float64).reshape(-1, 4, 4)
        out["mover_poses12"] = np.asarray(tr["poses12"], np.float32)
        out["times"] = np.asarray(tr["times"], np.float64)
        if tr.get("shapes"):        # a run under nonrigid_flow: true with animated movers
            animated = sorted(tr["shapes"])
            out["animated_movers"] = np.asarray(animated, np.int64)
            out["mover_shapes"] = np.stack([np.asarray(tr["shapes"][m], np.float64) for m in animated], axis=1)
        path = Path(output_dir)
        path.mkdir(parents=True, exist_ok=True)
        np.savez(path / f"{self.scene_name}_scene_flow.npz", **out)
        return out

    def _save_labeled_ply(self, output_path: Path, points: np.ndarray, colors: np.ndarray,
                          semantic_labels: np.ndarray, instance_labels: np.ndarray):
        write_labeled_ply(output_path, points, colors, semantic_labels, instance_labels)

    # ---- S3DIS annotation hooks (loaders themselves are out of scope, see the module docstring) ------------
    def _load_s3dis_txt_pointcloud(self, file_path: str) -> tuple:
        """``x y z r g b [label]`` text rows -> (points, colours in 0..1); (None, None) on any problem (:482-503)."""
        try:
            data = np.loadtxt(file_path)
            if data.shape[1] < 6:
                return None, None
            colors = data[:, 3:6]
            return data[:, :3], (colors / 255.0 if colors.max() > 1.0 else colors)
        except Exception:                                          # noqa: BLE001 - the reference swallows everything
            return None, None

    def _load_s3dis_original_data(self) -> tuple:
        """The room's raw coloured cloud ``{root}/{area}/{room}/{room}.txt`` (or the *_inst_nostring.txt variant)."""
        if not self.s3dis_data_root or not self.area or not self.room:
            return None, None
        base = f"{self.s3dis_data_root}/{self.area}/{self.room}"
        for path in (f"{base}/{self.room}.txt", f"{base}/Area_{self.area}_{self.room}_inst_nostring.txt"):
            if os.path.exists(path):
                points, colors = self._load_s3dis_txt_pointcloud(path)
                if points is None or len(points) == 0:
                    return None, None
                return points, colors
        return None, None

    def _annotation_arrays(self):
        from s3dis_annotation_loader import S3DISAnnotationLoader
        loader = S3DISAnnotationLoader(self.s3dis_data_root)
        rooms = loader.load_room_annotations(self.area, self.room)
        if not rooms:
            return None
        points, sem, ins = loader.create_labeled_pointcloud_with_instances(rooms)
        return (points, sem, ins) if len(points) else None

    def _load_s3dis_annotations(self) -> tuple:
        if not self.s3dis_data_root or not self.area or not self.room:
            return None, None
        try:
            got = self._annotation_arrays()
            return (got[1], got[2]) if got else (None, None)
        except Exception:                                          # noqa: BLE001
            return None, None

    def _load_s3dis_annotations_with_colors(self) -> tuple:
        if not self.s3dis_data_root or not self.area or not self.room:
            return None, None, None, None
        try:
            got = self._annotation_arrays()
            if not got:
                return None, None, None, None
            points, sem, ins = got
            raw_points, raw_colors = self._load_s3dis_original_data()
            if raw_points is None or raw_colors is None:
                colors = np.ones((len(points), 3), dtype=np.float32) * 0.5
            else:
                import lidarcast
                colors = raw_colors[lidarcast.NearestIndex(lidarcast.Context(0), raw_points).query(points)]
            return points, colors, sem, ins
        except Exception:                                          # noqa: BLE001
            return None, None, None, None

    def _decode_colors_to_labels(self, colors: np.ndarray) -> tuple:
        try:
            from s3dis_annotation_loader import S3DISColorEncoder
            return S3DISColorEncoder().decode_colors_to_labels_and_instances(colors)
        except Exception:                                          # noqa: BLE001
            return np.zeros(len(colors), dtype=np.uint16), np.zeros(len(colors), dtype=np.uint16)

    # ---- selection, dictionary round trip ----------------------------------------------------------------
    def filter_frames_by_quality(self, min_coverage: float = 0.0, max_coverage: float = 1.0) -> "S3DISSimScene":
        kept = S3DISSimScene(self.scene_name, self.simulation_config)
        kept.frames = [f for f in self.frames if min_coverage <= f.get_coverage_ratio() <= max_coverage]
        return kept

    def get_best_frames(self, num_frames: int = 10, quality_metric: str = "coverage") -> List[S3DISSimFrame]:
        keys = {"coverage": S3DISSimFrame.get_coverage_ratio, "points": S3DISSimFrame.get_num_points,
                "density": S3DISSimFrame.get_scan_density}
        if quality_metric not in keys:
            raise ValueError(f"Unsupported quality metric: {quality_metric}")
        return sorted(self.frames, key=keys[quality_metric], reverse=True)[:num_frames]

    def to_dict(self) -> Dict[str, Any]:
        return {"scene_name": self.scene_name, "simulation_config": self.simulation_config,
                "frames": [f.to_dict() for f in self.frames],
                "statistics": self.statistics.to_dict() if self.statistics else None}

    @classmethod
    def from_dict(cls, scene_dict: Dict[str, Any]) -> "S3DISSimScene":
        scene = cls(scene_name=scene_dict["scene_name"], simulation_config=scene_dict.get("simulation_config", {}))
        for fd in scene_dict["frames"]:
            scene.append_frame(S3DISSimFrame.from_dict(fd))
        if scene_dict.get("statistics"):
            scene.statistics = SimulationStats(**scene_dict["statistics"])
        return scene

    def __repr__(self) -> str:
        return (f"S3DISSimScene(name='{self.scene_name}', frames={self.get_total_frames()}, "
                f"points={self.get_total_points()}, avg_coverage={self.get_average_coverage():.3f})")


def _viridis(x: float) -> np.ndarray:
    """RGB in 0..1 of matplotlib's viridis at x (the reference colours frame i with plt.cm.viridis(i / n));
    without matplotlib a five-stop linear approximation of the same map."""
    try:
        import matplotlib.pyplot as plt
        return np.asarray(plt.cm.viridis(x)[:3], dtype=np.float64)
    except Exception:                                              # noqa: BLE001
        stops = np.array([[0.267, 0.005, 0.329], [0.229, 0.322, 0.546], [0.128, 0.567, 0.551],
                          [0.369, 0.789, 0.383], [0.993, 0.906, 0.144]])
        p = min(max(float(x), 0.0), 1.0) * 4
        i = min(int(p), 3)
        return stops[i] + (stops[i + 1] - stops[i]) * (p - i)
