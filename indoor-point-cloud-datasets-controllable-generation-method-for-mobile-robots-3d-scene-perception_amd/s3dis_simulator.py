"""Drop-in caller of the engines: the reference's S3DISSimulator scan stage
(reference: s3dis_simulator.py:36-77 construction, :220-296 run_simulation).

Scope: sensor + engine selection, trajectory (planned or straight), the scan loop and the result files, under the
reference's method names and signatures.  Scene loading takes a mesh object (anything with ``.vertices`` /
``.triangles``) or a PLY path; visualisation, furniture-aware collision checking, the batch / CLI drivers and NKSR
reconstruction are not part of this package.

``run_simulation`` keeps the reference's per-frame ScanQuality formulas, including two quirks of the
reference loop that a drop-in must reproduce to give the same statistics (``bug_compatible=True``):
the incident angles are overwritten with zeros (:266-269) and the range statistics are norms from the
WORLD origin, not from the sensor (:283-284).
"""
import itertools
import json
import time
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from containers import RoomBounds, S3DISScene, S3DISSimFrame, S3DISSimScene, ScanQuality
from lidar import (DualAxisLidarIntrinsics, Indoor8LineLidarIntrinsics, create_lidar)
from raycast_engine import RaycastEngineCPU, RaycastEngineGPU
from trajectory import (AutoTrajectoryGenerator, PathType, SmartTrajectoryGenerator, Waypoint, poses_from_waypoints,
                        sweep_end_poses)


_POOL = None             # thread pool of _quality_many, created on first use
_NO_GROUP = object()     # run_simulation(process_group=_NO_GROUP): single-process scan even inside a distributed job


class S3DISSimulator:
    def __init__(self, config: Dict[str, Any], use_dense_lidar: bool = False, use_blk2go: bool = False,
                 bug_compatible: bool = True):
        self.config = config
        self.use_dense_lidar = use_dense_lidar
        self.use_blk2go = use_blk2go
        self.bug_compatible = bug_compatible
        self.scene: Optional[S3DISScene] = None
        self.lidar_config = None
        self.raycast_engine = None
        self.trajectory_generator: Optional[SmartTrajectoryGenerator] = None
        self.auto_trajectory_generator: Optional[AutoTrajectoryGenerator] = None
        self.collision_detector = None          # furniture-aware planning is out of scope
        self._initialize_components()

    def _initialize_components(self):
        if self.use_blk2go:
            self.lidar_config = DualAxisLidarIntrinsics.create_blk2go_dual_axis()
        elif self.use_dense_lidar:
            self.lidar_config = Indoor8LineLidarIntrinsics.create_dense_32line()
        else:
            self.lidar_config = Indoor8LineLidarIntrinsics.create_standard_8line()
        # Both names are the HIP engine in this package; construction raises without a GPU.
        use_gpu = self.config.get("raycast_engine", {}).get("use_gpu", False)
        self.raycast_engine = RaycastEngineGPU() if use_gpu else RaycastEngineCPU()

    def load_scene(self, scene_path, scene_name: Optional[str] = None) -> S3DISScene:
        """scene_path: path to a triangle-mesh PLY (name defaults to the file stem, reference :78-129), or a mesh
        object."""
        if isinstance(scene_path, (str, bytes)) or hasattr(scene_path, "__fspath__"):
            from lidarcast.ply import read_triangle_mesh
            mesh = read_triangle_mesh(scene_path)
            scene_name = scene_name or Path(str(scene_path)).stem
            if len(np.asarray(mesh.vertices)) == 0:
                raise ValueError(f"Failed to load mesh file: {scene_path}")
        else:
            mesh = scene_path
            if len(np.asarray(mesh.vertices)) == 0:
                raise ValueError("Failed to load mesh: no vertices")
        self.scene = S3DISScene(scene_name or "scene", mesh, RoomBounds.from_vertices(mesh.vertices))
        self.trajectory_generator = SmartTrajectoryGenerator(
            self._bounds_dict(), robot_height=self.config.get("trajectory", {}).get("robot_height", 1.0))
        # same planner settings as the reference (s3dis_simulator.py:127): reduced radius for narrow spaces
        self.auto_trajectory_generator = AutoTrajectoryGenerator(robot_radius=0.15, context=self.raycast_engine.ctx)
        return self.scene

    def _bounds_dict(self) -> Dict[str, float]:
        b = self.scene.room_bounds
        return {"x_min": b.x_min, "x_max": b.x_max, "y_min": b.y_min, "y_max": b.y_max,
                "z_min": b.z_min, "z_max": b.z_max}

    def generate_auto_trajectory(self, num_waypoints: int = 20) -> Tuple[List[Waypoint], Dict[str, Any]]:
        """Planned trajectory for the loaded scene (reference s3dis_simulator.py:132-167)."""
        if self.auto_trajectory_generator is None or self.scene is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        return self.auto_trajectory_generator.generate_optimal_trajectory(
            mesh=self.scene.room_mesh, room_bounds=self._bounds_dict(), num_waypoints=num_waypoints)

    def generate_trajectory(self, start_point: Tuple[float, float, float], end_point: Tuple[float, float, float],
                            path_type: PathType = PathType.STRAIGHT,
                            num_waypoints: int = 20) -> Tuple[List[Waypoint], Dict[str, Any]]:
        """Trajectory between two positions -> (waypoints, quality as a dict) (reference :181-218; the furniture
        re-planning branch has nothing to act on here)."""
        if self.trajectory_generator is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        waypoints, quality = self.trajectory_generator.generate_trajectory(
            start_point=start_point, end_point=end_point, path_type=path_type, num_waypoints=num_waypoints)
        return waypoints, quality.to_dict()

    def add_furniture(self, furniture_mesh, name: str, category: str = "unknown"):
        """The reference forwards this to its CollisionDetector, which does not import; furniture
        that is part of the room mesh occludes rays without it."""
        raise NotImplementedError("furniture-aware collision checking is out of scope (DESIGN.md section 9); "
                                  "put the furniture into the room mesh")

    def save_results(self, sim_scene: S3DISSimScene, output_dir, waypoints: Optional[List[Waypoint]] = None,
                     save_visualizations: bool = True):
        """Result files of the scene (statistics, summary, both combined clouds; reference :298-371).  The
        visualisations the reference adds are out of scope; the flag is accepted and ignored."""
        sim_scene.save_results(Path(output_dir))

    def run_complete_simulation(self, scene_path, start_point: Tuple[float, float, float],
                                end_point: Tuple[float, float, float], path_type: PathType = PathType.STRAIGHT,
                                num_waypoints: int = 20, output_dir=None,
                                scene_name: Optional[str] = None) -> S3DISSimScene:
        """load_scene -> generate_trajectory -> run_simulation -> save_results (reference :373-413)."""
        self.load_scene(scene_path, scene_name)
        waypoints, _ = self.generate_trajectory(start_point, end_point, path_type, num_waypoints)
        sim_scene = self.run_simulation(waypoints)
        self.save_results(sim_scene, Path("s3dis_simulation_results") if output_dir is None else Path(output_dir),
                          waypoints)
        return sim_scene

    def run_auto_simulation(self, scene_path, num_waypoints: int = 20, output_dir=None,
                            scene_name: Optional[str] = None) -> S3DISSimScene:
        """load_scene -> generate_auto_trajectory -> run_simulation -> save_results + trajectory_analysis.json
        (reference :415-455).  The planned waypoints and the planner's report stay available as
        ``last_waypoints`` / ``last_analysis``."""
        self.load_scene(scene_path, scene_name)
        waypoints, analysis = self.generate_auto_trajectory(num_waypoints)
        self.last_waypoints, self.last_analysis = waypoints, analysis
        sim_scene = self.run_simulation(waypoints)
        out = Path("s3dis_auto_simulation_results") if output_dir is None else Path(output_dir)
        self.save_results(sim_scene, out, waypoints)
        with open(out / "trajectory_analysis.json", "w", encoding="utf-8") as f:
            json.dump(analysis, f, indent=2, ensure_ascii=False)
        return sim_scene

    # ---- the scan stage ---------------------------------------------------------------------------
    def _quality(self, points, incident_angles, total_points_per_scan, room_volume, ranges=None) -> ScanQuality:
        k = len(points)
        if ranges is None:
            ranges = np.linalg.norm(points, axis=1) if k > 0 else None     # from the world origin, as the reference
        return ScanQuality(
            coverage_ratio=k / total_points_per_scan, num_points=k,
            incident_angle_mean=np.mean(incident_angles) if len(incident_angles) > 0 else 0,
            incident_angle_std=np.std(incident_angles) if len(incident_angles) > 0 else 0,
            scan_density=k / room_volume,
            range_mean=np.mean(ranges) if k > 0 else 0, range_std=np.std(ranges) if k > 0 else 0)

    def _quality_from_stats(self, fr, total_points_per_scan, room_volume):
        """ScanQuality of every frame from the per-pose statistics the device computed with numpy's arithmetic."""
        counts = fr["counts"].tolist()
        zero = np.float64(0.0)
        P = len(counts)
        am = [zero] * P if self.bug_compatible else list(fr["incident_mean"])
        asd = [zero] * P if self.bug_compatible else list(fr["incident_std"])
        rm, rs = list(fr["range_origin_mean"]), list(fr["range_origin_std"])      # numpy scalars, as np.mean returns them
        out = []
        for i, k in enumerate(counts):
            if k == 0:
                out.append(ScanQuality(0.0, 0, 0, 0, 0.0, 0, 0))
            else:
                out.append(ScanQuality(k / total_points_per_scan, k, am[i], asd[i], k / room_volume, rm[i], rs[i]))
        return out

    def _quality_many(self, points, angles, total_points_per_scan, room_volume, ranges):
        """ScanQuality of every frame; frames are independent, so a small thread pool reduces them side by side."""
        zero_angles = self.bug_compatible      # mean and std of an all-zero block are exactly 0.0: no need to reduce it

        def one(i):
            k = len(points[i])
            r = ranges[i]
            a = angles[i]
            return ScanQuality(
                coverage_ratio=k / total_points_per_scan, num_points=k,
                incident_angle_mean=(np.float64(0.0) if zero_angles else np.mean(a)) if k > 0 else 0,
                incident_angle_std=(np.float64(0.0) if zero_angles else np.std(a)) if k > 0 else 0,
                scan_density=k / room_volume,
                range_mean=np.mean(r) if k > 0 else 0, range_std=np.std(r) if k > 0 else 0)
        n = len(points)
        if n < 8 or sum(len(p) for p in points) < (1 << 18):
            return [one(i) for i in range(n)]
        global _POOL
        if _POOL is None:
            import os
            from concurrent.futures import ThreadPoolExecutor
            _POOL = ThreadPoolExecutor(max_workers=max(2, min(8, (os.cpu_count() or 2))))
        return list(_POOL.map(one, range(n)))

    def evaluate_surface_coverage(self, waypoints: List[Waypoint]) -> Dict[str, Any]:
        """What the scan of ``waypoints`` saw of the loaded room, JSON-ready: covered and total area,
        ratio, seen triangles, returned rays, redundancy (returns per covered m^2) and per-class figures keyed by the S3DIS
        class name where the label is a known class id.  Scans again on the GPU; run_simulation is not involved."""
        if self.scene is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        if self.config.get("motion") is not None:
            raise NotImplementedError("surface coverage of moving-sensor sweeps is outside its scope")
        if self.config.get("noise") is not None:
            raise NotImplementedError("surface coverage under the noise key is outside its scope")
        if self.config.get("beam") is not None:
            raise NotImplementedError("surface coverage under the beam key is outside its scope")
        if self.config.get("materials") is not None:
            raise NotImplementedError("surface coverage under the materials key is outside its scope")
        if self.config.get("movers") is not None:
            raise NotImplementedError("surface coverage under the movers key is outside its scope")
        from lidarcast.synth import S3DIS_CLASSES
        s = self.raycast_engine.surface_coverage(self.lidar_config, poses_from_waypoints(waypoints),
                                                 self.scene.room_mesh)
        out = s.to_dict(class_names=dict(enumerate(S3DIS_CLASSES)))
        out["num_poses"] = len(waypoints)
        return out

    def export_occupancy_grid(self, waypoints: List[Waypoint], output_dir, voxel_size: float = 0.05,
                              min_returns: int = 1) -> Dict[str, Any]:
        """Semantic occupancy grid of the scan of ``waypoints`` over the loaded room, written to
        ``output_dir``: <scene>_occupancy.npz (state, sem, ins, returns, origin, voxel_size, dims),
        <scene>_occupancy.json (counts and per-class occupied voxels keyed by the S3DIS class name where the label is
        a known class id) and <scene>_occupied_voxels.ply (occupied voxel centres with their labels, the labelled-PLY
        layout).  The extent is the room mesh's bounds with a one-voxel margin.  Scans again on the GPU; run_simulation
        is not involved.  Returns the JSON summary."""
        if self.scene is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        if self.config.get("motion") is not None:
            raise NotImplementedError("occupancy grids of moving-sensor sweeps are outside their scope")
        if self.config.get("noise") is not None:
            raise NotImplementedError("occupancy grids under the noise key are outside their scope")
        if self.config.get("beam") is not None:
            raise NotImplementedError("occupancy grids under the beam key are outside their scope")
        if self.config.get("materials") is not None:
            raise NotImplementedError("occupancy grids under the materials key are outside their scope")
        if self.config.get("movers") is not None:
            raise NotImplementedError("occupancy grids under the movers key are outside their scope")
        from containers.s3dis_sim_scene import write_labeled_ply
        from lidarcast.synth import S3DIS_CLASSES
        r = self.raycast_engine.occupancy_grid(self.lidar_config, poses_from_waypoints(waypoints), self.scene.room_mesh,
                                               voxel_size=voxel_size, min_returns=min_returns)
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        name = self.scene.scene_name
        r.to_npz(out / f"{name}_occupancy.npz")
        centres, sem, ins = r.occupied_centres()
        write_labeled_ply(out / f"{name}_occupied_voxels.ply", centres.astype(np.float32),
                          np.full((len(centres), 3), 127, dtype=np.uint8), sem, ins)
        summary = r.to_dict(class_names=dict(enumerate(S3DIS_CLASSES)))
        summary["scene_name"] = name
        summary["num_poses"] = len(waypoints)
        with open(out / f"{name}_occupancy.json", "w") as f:
            json.dump(summary, f, indent=2)
        return summary

    def export_dynamic_occupancy(self, waypoints: List[Waypoint], output_dir, voxel_size: float = 0.05,
                                 min_returns: int = 1, process_group=None) -> Dict[str, Any]:
        """Per-frame occupancy of the scan of ``waypoints`` over the loaded room and its movers, written to
        ``output_dir``: <scene>_dynamic_occupancy.npz (one grid per frame: the dense state (F, nx, ny, nz) and the sparse list with
        sem, ins, returns, mover and mover_returns), <scene>_static_map.npz (one slot: every frame's free space, the movers'
        returns left out) and <scene>_dynamic_occupancy.json (per frame the counts, occupied voxels per class keyed by the S3DIS
        class name where known, and dynamic voxels per mover).  Works with the top-level ``movers`` key (rigid, ``animation``,
        ``skin`` and ``movers.noise``; frame k is at k * period) and with no feature key at all (the room alone, one grid per
        waypoint).  The extent is the room mesh's bounds with a one-voxel margin.  Scans again on the GPU; run_simulation is not
        involved.  Returns the JSON summary."""
        if self.scene is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        motion = self.config.get("motion")
        if motion is not None:
            key = "motion.movers" if isinstance(motion, dict) and motion.get("movers") is not None else "motion"
            raise NotImplementedError(f"dynamic occupancy under the {key} key is outside its scope: no sweep scan exports its "
                                      "per-ray origins yet")
        for key in ("noise", "beam", "materials"):
            if self.config.get(key) is not None:
                raise NotImplementedError(f"dynamic occupancy under the {key} key is outside its scope")
        batched = isinstance(self.lidar_config, Indoor8LineLidarIntrinsics) and self.lidar_config.vertical_degrees is not None
        if not batched:
            raise NotImplementedError("dynamic occupancy needs a multi-line sensor with a direction table (the dual-axis sensor "
                                      "is outside its scope)")
        from lidarcast.distributed import active_group
        dist, _ = (None, None) if process_group is _NO_GROUP else active_group(process_group)
        if dist is not None:
            raise NotImplementedError("dynamic occupancy on a multi-rank process group is outside its scope")
        from lidarcast.synth import S3DIS_CLASSES
        engine, mesh = self.raycast_engine, self.scene.room_mesh
        poses = poses_from_waypoints(waypoints)
        plan = self._mover_plan() if len(waypoints) > 0 else None
        deformables, mset, mover_poses, shapes, noise = {}, None, None, None, None
        try:
            if plan is not None:
                from lidarcast.movers import MoverSet
                times = np.arange(len(waypoints), dtype=np.float64) * plan["period"]
                mover_poses = np.stack([t.poses12(times) for t in plan["tracks"]], axis=1)       # (P, M, 12) float32
                noise = plan["noise"]
                animated = [m for m, c in enumerate(plan["clips"]) if c is not None]
                if animated:
                    from lidarcast import deform
                    for m in animated:
                        mm, rig = plan["meshes"][m], plan["skins"][m]
                        if rig is not None:
                            deformables[m] = deform.SkinnedDeformable(engine.ctx, rig["rest"], mm.triangles, rig["bone_index"],
                                                                      rig["bone_weight"], rig["poses12"], mm.triangle_sem,
                                                                      mm.triangle_ins)
                        else:
                            deformables[m] = deform.Deformable(engine.ctx, plan["keyframes"][m], mm.triangles, mm.triangle_sem,
                                                               mm.triangle_ins)
                    shapes = np.stack([plan["clips"][m].shapes3(times) for m in animated], axis=1)      # (P, D, 3)
                mset = MoverSet(engine.ctx, [deformables.get(m, mm) for m, mm in enumerate(plan["meshes"])])
            r, static = engine.dynamic_occupancy(self.lidar_config, poses, mesh, movers=mset, mover_poses=mover_poses,
                                                 shapes=shapes, noise=noise, voxel_size=voxel_size, min_returns=min_returns,
                                                 static_map=True)
        finally:
            if mset is not None:
                mset.close()
            for d in deformables.values():
                d.close()
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        name = self.scene.scene_name
        r.to_npz(out / f"{name}_dynamic_occupancy.npz")
        static.to_npz(out / f"{name}_static_map.npz")
        names = dict(enumerate(S3DIS_CLASSES))
        summary = r.to_dict(class_names=names)
        if len(waypoints) == 0:             # the one slot the object needs to exist is not a scanned frame
            summary["num_frames"], summary["frames"] = 0, []
        summary["scene_name"] = name
        summary["num_poses"] = len(waypoints)
        summary["movers"] = [] if plan is None else plan["objects"]
        summary["static_map"] = static.to_dict(class_names=names)["frames"][0]
        with open(out / f"{name}_dynamic_occupancy.json", "w") as f:
            json.dump(summary, f, indent=2)
        return summary

    def export_frame_annotations(self, waypoints: List[Waypoint], output_dir, min_points: int = 10,
                                 semantic_mapping: Optional[Dict[str, int]] = None) -> Dict[str, Any]:
        """Per-frame detection annotations of the scan of ``waypoints`` over the loaded room,
        written to ``output_dir``/<scene>_frame_annotations.json: the object table (key, sem, class name where known,
        ins, tri_count, area in m^2, world AABB) and, per frame, the pose and every listed object with ``num_points``,
        ``seen_ratio``, ``box7`` (the amodal box in the sensor frame: cx, cy, cz, dx, dy, dz, heading) and the visible
        box ``visible_min`` / ``visible_max``.  An object is listed when it has at least ``min_points`` returns in the
        frame, its class is in ``semantic_mapping`` (class name -> semantic id, default S3DIS_SEMANTIC_MAPPING: the
        classes of export_detection_annotations) and its instance id is not 0.  Scans again on the GPU; run_simulation
        is not involved.  Returns the dict."""
        if self.scene is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        if self.config.get("motion") is not None:
            raise NotImplementedError("frame annotations of moving-sensor sweeps are outside their scope")
        if self.config.get("noise") is not None:
            raise NotImplementedError("frame annotations under the noise key are outside their scope")
        if self.config.get("beam") is not None:
            raise NotImplementedError("frame annotations under the beam key are outside their scope")
        if self.config.get("materials") is not None:
            raise NotImplementedError("frame annotations under the materials key are outside their scope")
        if self.config.get("movers") is not None:
            raise NotImplementedError("frame annotations under the movers key are outside their scope")
        from lidar_net_bbox_visualizer import S3DIS_SEMANTIC_MAPPING
        from lidarcast.synth import S3DIS_CLASSES
        mapping = S3DIS_SEMANTIC_MAPPING if semantic_mapping is None else semantic_mapping
        name_of = {int(s): n for n, s in mapping.items()}
        poses = np.ascontiguousarray(poses_from_waypoints(waypoints), dtype=np.float64).reshape(-1, 4, 4)
        r = self.raycast_engine.frame_objects(self.lidar_config, poses, self.scene.room_mesh)
        boxes = r.boxes7(poses)
        ratio = r.seen_ratio
        sem, ins, area = r.sem, r.ins, r.total_area
        objects = []
        for k in range(r.num_objects):
            s = int(sem[k])
            cls = name_of.get(s, S3DIS_CLASSES[s] if s < len(S3DIS_CLASSES) else None)
            objects.append({"index": k, "key": int(r.key[k]), "sem": s, "class": cls, "ins": int(ins[k]),
                            "tri_count": int(r.tri_count[k]), "area_m2": float(area[k]),
                            "world_min": [float(x) for x in r.wmin[k]], "world_max": [float(x) for x in r.wmax[k]]})
        listed = [k for k in range(r.num_objects) if int(sem[k]) in name_of and int(ins[k]) != 0]
        frames = []
        for f in range(len(poses)):
            objs = []
            for k in listed:
                n = int(r.returns[f, k])
                if n < int(min_points):
                    continue
                objs.append({"object": k, "class": name_of[int(sem[k])], "sem": int(sem[k]), "ins": int(ins[k]),
                             "num_points": n, "seen_ratio": float(ratio[f, k]),
                             "box7": [float(x) for x in boxes[f, k]],
                             "visible_min": [float(x) for x in r.vmin[f, k]],
                             "visible_max": [float(x) for x in r.vmax[f, k]]})
            frames.append({"frame": f, "pose": [[float(x) for x in row] for row in poses[f]], "objects": objs})
        name = self.scene.scene_name
        summary = {"scene_name": name, "num_frames": len(poses), "min_points": int(min_points),
                   "rejected_rays": int(r.rejected_rays), "objects": objects, "frames": frames}
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / f"{name}_frame_annotations.json", "w") as fh:
            json.dump(summary, fh, indent=2)
        return summary

    def _noise_model(self, nested=False, under_movers=False, under_sweep_movers=False):
        """The NoiseModel of the config key ``noise`` (None without the key): ``seed`` is required; ``range_std`` (m),
        ``angle_std_deg`` and ``dropout`` default to the sensor record's range_noise_std, angle_noise_std (degrees) and
        dropout_probability.  first_frame = 0: frame p of a run has frame id p.  ``nested``: the same entries under
        ``motion: {noise: ...}``, the seeded noise of moving-sensor sweeps.  ``under_movers``: the same entries under
        ``movers: {noise: ...}``, the seeded noise drawn in the mover kernels.  ``under_sweep_movers``: the
        same entries under ``motion: {movers: {sensor_noise: ...}}``, that noise under movers in sweeps."""
        if under_sweep_movers:
            cfg, key = ((self.config.get("motion") or {}).get("movers") or {}).get("sensor_noise"), "motion.movers.sensor_noise"
        elif under_movers:
            cfg, key = (self.config.get("movers") or {}).get("noise"), "movers.noise"
        else:
            cfg = (self.config.get("motion") or {}).get("noise") if nested else self.config.get("noise")
            key = "motion.noise" if nested else "noise"
        if cfg is None:
            return None
        if not isinstance(cfg, dict):
            raise ValueError(f"the {key} key must be a mapping with a seed: {{seed, range_std?, angle_std_deg?, dropout?}}")
        if "seed" not in cfg:
            raise ValueError(f"the {key} key needs a seed")
        unknown = set(cfg) - {"seed", "range_std", "angle_std_deg", "dropout"}
        if unknown:
            raise ValueError(f"unknown entries under the {key} key: {sorted(unknown)}")
        from lidarcast.noise import NoiseModel
        k = self.lidar_config
        return NoiseModel(seed=int(cfg["seed"]),
                          range_std=float(cfg.get("range_std", getattr(k, "range_noise_std", 0.0))),
                          angle_std=float(np.deg2rad(float(cfg.get("angle_std_deg", getattr(k, "angle_noise_std", 0.0))))),
                          dropout=float(cfg.get("dropout", getattr(k, "dropout_probability", 0.0))))

    def _beam_model(self):
        """The BeamModel of the config key ``beam`` (None without the key): ``divergence_mrad`` (the beam's full angle) is
        required; ``pattern`` (single, cross5, hex7), ``max_echoes``, ``separation`` (m) and ``min_fraction`` default to
        BeamModel's."""
        cfg = self.config.get("beam")
        if cfg is None:
            return None
        if "divergence_mrad" not in cfg:
            raise ValueError("the beam key needs divergence_mrad")
        unknown = set(cfg) - {"divergence_mrad", "pattern", "max_echoes", "separation", "min_fraction"}
        if unknown:
            raise ValueError(f"unknown entries under the beam key: {sorted(unknown)}")
        from lidarcast.echo import BeamModel
        kw = {k: cfg[k] for k in ("pattern", "max_echoes", "separation", "min_fraction") if k in cfg}
        return BeamModel(float(cfg["divergence_mrad"]) * 1e-3, **kw)

    def _material_table(self):
        """The MaterialTable of the config key ``materials`` (None without the key): ``classes`` maps a class name (S3DIS class
        list) or a semantic id to ``{kind: diffuse | glass | mirror, albedo?, pass?, retro_deg? or retro_cos?}``;
        ``max_bounces`` and ``min_intensity`` default to MaterialTable's.  ``retro_deg`` becomes retro_cos = cos(retro_deg) here,
        on the host.  The key stands alone: motion, noise and beam are refused beside it."""
        cfg = self.config.get("materials")
        if cfg is None:
            return None
        for other in ("motion", "noise", "beam"):
            if self.config.get(other) is not None:
                raise ValueError(f"the materials key cannot be combined with the {other} key")
        unknown = set(cfg) - {"classes", "max_bounces", "min_intensity"}
        if unknown:
            raise ValueError(f"unknown entries under the materials key: {sorted(unknown)}")
        from lidarcast.material import MaterialTable
        kw = {k: cfg[k] for k in ("max_bounces", "min_intensity") if k in cfg}
        return MaterialTable.from_classes(cfg.get("classes", {}), **kw)

    def _mover_plan(self, nested=False):
        """The moving objects of the config key ``movers`` (None without the key): ``period`` (seconds between frames; frame k
        is at k * period) and ``objects``, each ``{mesh: pedestrian | <path to a mesh>, semantic: id or S3DIS class name,
        instance: id, path: [[t, x, y, z, yaw_deg], ...]}``, and optionally ``flow: true`` (scene flow: frames then carry the flow
        to the next frame and its status).  Returns {period, meshes, tracks, objects (JSON-ready), flow}.
        ``nonrigid_flow: true`` is ``flow: true`` for a set with animated movers: their rows flow with
        their triangle from the frame's shape to the next frame's, rigid movers take the rigid step; refused beside ``flow:
        true``, under ``motion.movers`` and with more than 16 animated movers.
        The key stands alone: motion, noise, beam and materials are refused beside it.
        An object may carry ``animation: {cycle: <seconds>, phase: 0.0, loop: true}`` (a deforming mover):
        with ``mesh: walker`` the keyframes come from ``synth.make_walker``, with ``keyframes: <file.npy>`` a (K, V, 3) array serves
        the mesh file's own topology; frame k takes the shape of k * period.  The plan then also holds ``clips`` and ``keyframes``
        (one entry per object, None for a rigid one).  ``flow: true`` is refused in a set with an animated mover (the rigid flow
        step is wrong for it), and so is ``animation`` under ``motion.movers`` unless that key carries ``per_ray_shape: true``.
        ``per_ray_shape: true`` (under ``motion.movers`` only) accepts animated objects there: each one's
        clip is evaluated at the start and at the end of every sweep, and every ray meets the mover at the shape it has at the
        moment the ray fires.  The plan's ``per_ray_shape`` holds the flag.
        An animated object may be SKINNED instead: ``mesh: walker_rig`` takes ``synth.make_walker_rig``, and
        ``skin: <file.npz>`` beside ``mesh: <file>`` takes the mesh file's vertices as the rest shape and, from the file,
        ``bone_index`` (V, 4) uint8, ``bone_weight`` (V, 4) float32, ``poses`` (K, B, 12) float32 and optionally ``parents`` (B,) and
        ``joints`` (B, 3), a skeleton whose joints then go to the tracks file.  The plan's ``skins`` holds one dict per such object
        (None otherwise) and its ``keyframes`` entry is None: the key poses are skinned on the device.  ``skin`` beside
        ``keyframes`` is refused, and so is ``skin`` without ``animation``.
        ``nested``: the same entries under ``motion: {movers: ...}``, movers that go on moving while a sweep is scanned (DESIGN.md
        section 5n): sweep k starts at k * period.  There ``flow: true`` is refused (no scene flow under sweeps), and so are
        ``motion.noise``, beam and materials beside it.
        ``noise: {seed, range_std?, angle_std_deg?, dropout?}`` under the (top-level) movers key draws seeded sensor noise in the
        mover kernels: the entries and defaults of the noise key, frame p has frame id p; the plan's
        ``noise`` holds the NoiseModel (None without the entry).  ``flow: true`` and ``nonrigid_flow: true`` are refused beside it;
        a top-level noise key beside movers stays refused, and so does ``motion.noise`` beside ``motion.movers``.
        ``sensor_noise: {seed, range_std?, angle_std_deg?, dropout?}`` under ``motion.movers`` (there only)
        draws that noise under movers in sweeps: the entries, defaults and unknown-entry refusal of the noise key, sweep p has
        frame id p, and the plan's ``noise`` holds the NoiseModel.  Rigid, ``animation`` and ``skin`` objects all work (animated
        ones with ``per_ray_shape: true``, as without noise).  The entry is not called ``noise``: ``noise`` under ``motion.movers``
        and ``motion.noise`` beside ``motion.movers`` have been refused since sections 5n and 5r, configurations that spell them
        rely on that refusal, and a name of its own keeps both refusals as they are.  ``flow`` and ``nonrigid_flow`` are refused
        beside it as beside ``movers.noise``."""
        cfg = (self.config.get("motion") or {}).get("movers") if nested else self.config.get("movers")
        key = "motion.movers" if nested else "movers"
        if cfg is None:
            return None
        if nested:
            if (self.config.get("motion") or {}).get("noise") is not None:
                raise ValueError("motion.movers cannot be combined with motion.noise: noise under mover sweeps is not built by "
                                 "this pair of keys; it is asked for with motion: {speed, movers: {sensor_noise: {seed, ...}, ...}}")
            for other in ("beam", "materials"):
                if self.config.get(other) is not None:
                    raise ValueError(f"motion.movers cannot be combined with the {other} key")
        else:
            for other in ("motion", "noise", "beam", "materials"):
                if self.config.get(other) is not None:
                    raise ValueError(f"the movers key cannot be combined with the {other} key")
        unknown = set(cfg) - {"period", "objects", "flow", "nonrigid_flow"} - ({"per_ray_shape", "sensor_noise"} if nested else {"noise"})
        if unknown:
            raise ValueError(f"unknown entries under the {key} key: {sorted(unknown)}")
        per_ray_shape = cfg.get("per_ray_shape", False)
        if not isinstance(per_ray_shape, bool):
            raise ValueError(f"{key}.per_ray_shape must be true or false")
        noise = self._noise_model(under_sweep_movers=True) if nested else self._noise_model(under_movers=True)
        if nested and noise is not None and (cfg.get("flow", False) is True or cfg.get("nonrigid_flow", False) is True):
            which = "nonrigid_flow" if cfg.get("nonrigid_flow", False) is True else "flow"
            raise ValueError(f"motion.movers.{which} is not available beside motion.movers.sensor_noise: a noisy point sits off its "
                             "surface by more than the status margin of 2^-12 max(L, 1), so its own surface would occlude it "
                             "(scene flow under noise is not built)")
        if not isinstance(cfg.get("flow", False), bool):
            raise ValueError(f"{key}.flow must be true or false")
        if nested and cfg.get("flow", False):
            raise ValueError("motion.movers.flow is not available: scene flow under moving-sensor sweeps is not built")
        nonrigid = cfg.get("nonrigid_flow", False)
        if not isinstance(nonrigid, bool):
            raise ValueError(f"{key}.nonrigid_flow must be true or false")
        if nested and nonrigid:
            raise ValueError("motion.movers.nonrigid_flow is not available: scene flow under moving-sensor sweeps is not built")
        if nonrigid and cfg.get("flow", False):
            raise ValueError(f"{key}.nonrigid_flow and {key}.flow exclude each other: nonrigid_flow gives the rigid movers of "
                             "the set the rigid step")
        if noise is not None and (cfg.get("flow", False) or nonrigid):
            raise ValueError(f"movers.{'nonrigid_flow' if nonrigid else 'flow'} is not available beside movers.noise: a noisy point "
                             "sits off its surface by more than the status margin of 2^-12 max(L, 1), so its own surface would "
                             "occlude it (scene flow under noise is not built)")
        period = float(cfg.get("period", 0.1))
        if not (np.isfinite(period) and period > 0.0):
            raise ValueError(f"{key}.period must be a positive number of seconds")
        objects = cfg.get("objects")
        if not objects:
            raise ValueError(f"the {key} key needs at least one object")
        if len(objects) > 255:
            raise ValueError(f"the {key} key takes at most 255 objects")
        from lidarcast import synth
        from lidarcast.movers import MoverTrack
        meshes, tracks, listed, clips, keyframes, skins = [], [], [], [], [], []
        for k, obj in enumerate(objects):
            unknown = set(obj) - {"mesh", "semantic", "instance", "path", "animation", "keyframes", "skin"}
            if unknown:
                raise ValueError(f"unknown entries of mover {k}: {sorted(unknown)}")
            if "path" not in obj:
                raise ValueError(f"mover {k} needs a path")
            sem = obj.get("semantic", 13)
            if isinstance(sem, str):
                if sem not in synth.S3DIS_CLASSES:
                    raise ValueError(f"mover {k}: unknown class {sem!r}")
                sem = synth.S3DIS_CLASSES.index(sem)
            sem, ins = int(sem), int(obj.get("instance", k + 1))
            if not (0 <= sem < 65536 and 0 <= ins < 65536):
                raise ValueError(f"mover {k}: semantic and instance ids must fit 16 bits")
            name = obj.get("mesh", "pedestrian")
            if name == "pedestrian":
                mesh = synth.make_pedestrian(semantic=sem, instance=ins)
            elif name == "walker":
                mesh = synth.make_walker(semantic=sem, instance=ins)
            elif name == "walker_rig":
                mesh = synth.make_walker_rig(semantic=sem, instance=ins)
            else:
                from lidarcast.ply import read_triangle_mesh
                src = read_triangle_mesh(str(name))
                f = np.asarray(src.triangles, np.int32)
                mesh = synth.TriangleMesh(vertices=np.asarray(src.vertices, np.float64), triangles=f,
                                          triangle_sem=np.full(len(f), sem, np.uint16), triangle_ins=np.full(len(f), ins, np.uint16))
            clip, keys, rig = self._mover_animation(k, key, obj, mesh, nested and not per_ray_shape)
            meshes.append(mesh)
            tracks.append(MoverTrack(obj["path"]))
            clips.append(clip)
            keyframes.append(keys)
            skins.append(rig)
            box = np.asarray(mesh.vertices) if keys is None else keys.reshape(-1, 3)      # an animated mover: all its keyframes
            if rig is not None:             # a skinned mover: all its key poses, skinned on the host one at a time
                from lidarcast import skin
                each = [skin.apply(rig["rest"], rig["bone_index"], rig["bone_weight"], p) for p in rig["poses12"]]
                box = np.stack([np.min([v.min(0) for v in each], 0), np.max([v.max(0) for v in each], 0)])
            listed.append({"index": k, "mesh": str(name), "semantic": sem, "instance": ins, "num_triangles": len(mesh.triangles),
                           "box_min": [float(x) for x in box.min(0)], "box_max": [float(x) for x in box.max(0)]})
            if clip is not None:
                listed[-1]["animation"] = {"cycle": clip.cycle, "phase": clip.phase, "loop": clip.loop, "num_keyframes": clip.K}
        if cfg.get("flow", False) and any(c is not None for c in clips):
            raise ValueError(f"{key}.flow is not available in a set with an animated mover: the flow of a rigid step is wrong "
                             "for a surface that changes shape (non-rigid flow is not built)")
        if nonrigid and sum(c is not None for c in clips) > 16:
            raise ValueError(f"{key}.nonrigid_flow takes at most 16 animated movers")
        return {"period": period, "meshes": meshes, "tracks": tracks, "objects": listed, "flow": bool(cfg.get("flow", False)),
                "nonrigid_flow": nonrigid, "clips": clips, "keyframes": keyframes, "skins": skins, "noise": noise,
                "per_ray_shape": per_ray_shape}

    @staticmethod
    def _mover_animation(k, key, obj, mesh, refuse):
        """(Clip, (K, V, 3) float32 keyframes or None, skin dict or None) of mover ``k``'s ``animation`` entry, three times None
        without one.  A skinned mover has no keyframes; its dict holds rest, bone_index, bone_weight, poses12 and skeleton
        (a ``lidarcast.skin.Skeleton`` or None).  ``refuse``: the key is ``motion.movers`` without ``per_ray_shape: true``,
        where an animation is refused."""
        anim = obj.get("animation")
        if anim is None:
            if obj.get("keyframes") is not None:
                raise ValueError(f"mover {k}: keyframes need an animation entry")
            if obj.get("skin") is not None:
                raise ValueError(f"mover {k}: skin needs an animation entry")
            return None, None, None
        if refuse:
            raise ValueError("animation is not available under motion.movers: deformation within a sweep is not built")
        if not isinstance(anim, dict) or set(anim) - {"cycle", "phase", "loop"} or "cycle" not in anim:
            raise ValueError(f"mover {k}: animation is {{cycle: <seconds>, phase: 0.0, loop: true}}")
        if not isinstance(anim.get("loop", True), bool):
            raise ValueError(f"mover {k}: animation.loop must be true or false")
        if obj.get("skin") is not None and obj.get("keyframes") is not None:
            raise ValueError(f"mover {k}: skin and keyframes exclude each other")
        from lidarcast.deform import Clip
        rig = None
        if obj.get("skin") is not None:
            rig = S3DISSimulator._skin_file(k, str(obj["skin"]), mesh)
        elif getattr(mesh, "poses12", None) is not None:        # mesh: walker_rig
            rig = {"rest": np.asarray(mesh.vertices, np.float32), "bone_index": mesh.bone_index, "bone_weight": mesh.bone_weight,
                   "poses12": mesh.poses12, "skeleton": mesh.skeleton}
        if rig is not None:
            return Clip(len(rig["poses12"]), anim["cycle"], phase=float(anim.get("phase", 0.0)), loop=anim.get("loop", True)), None, rig
        if obj.get("keyframes") is not None:
            keys = np.load(str(obj["keyframes"]), allow_pickle=False)
            if keys.ndim != 3 or keys.shape[1:] != (len(mesh.vertices), 3) or keys.shape[0] < 1:
                raise ValueError(f"mover {k}: keyframes must be (K, V, 3) with V = {len(mesh.vertices)} vertices of its mesh, "
                                 f"got {keys.shape}")
            keys = np.ascontiguousarray(keys, dtype=np.float32)
        elif getattr(mesh, "keyframes", None) is not None:
            keys = mesh.keyframes
        else:
            raise ValueError(f"mover {k}: an animation needs mesh: walker or a keyframes file (or mesh: walker_rig or a skin file)")
        if not np.isfinite(keys).all():
            raise ValueError(f"mover {k}: keyframes must be finite")
        return Clip(len(keys), anim["cycle"], phase=float(anim.get("phase", 0.0)), loop=anim.get("loop", True)), keys, None

    @staticmethod
    def _skin_file(k, path, mesh):
        """The skin dict of mover ``k`` from ``skin: <file.npz>``; the rest shape is the mesh file's vertices."""
        from lidarcast import skin
        V = len(mesh.vertices)
        with np.load(path, allow_pickle=False) as z:
            missing = {"bone_index", "bone_weight", "poses"} - set(z.files)
            if missing:
                raise ValueError(f"mover {k}: the skin file lacks {sorted(missing)}")
            index, weight, poses = z["bone_index"], z["bone_weight"], z["poses"]
            parents = z["parents"] if "parents" in z.files else None
            joints = z["joints"] if "joints" in z.files else None
        if index.shape != (V, 4) or index.dtype != np.uint8 or weight.shape != (V, 4):
            raise ValueError(f"mover {k}: skin needs bone_index (V, 4) uint8 and bone_weight (V, 4) with V = {V} vertices of its "
                             f"mesh, got {index.shape} {index.dtype} and {weight.shape}")
        if poses.ndim != 3 or poses.shape[0] < 1 or not 1 <= poses.shape[1] <= 255 or poses.shape[2] != 12:
            raise ValueError(f"mover {k}: skin poses must be (K, B, 12) with 1 <= B <= 255, got {poses.shape}")
        if (parents is None) != (joints is None):
            raise ValueError(f"mover {k}: a skin file holds parents and joints together or neither")
        skeleton = None
        if parents is not None:
            skeleton = skin.Skeleton(parents, joints)
            if len(skeleton) != poses.shape[1]:
                raise ValueError(f"mover {k}: the skin file's skeleton has {len(skeleton)} bones, its poses {poses.shape[1]}")
        return {"rest": np.ascontiguousarray(mesh.vertices, dtype=np.float32), "bone_index": np.ascontiguousarray(index),
                "bone_weight": np.ascontiguousarray(weight, dtype=np.float32),
                "poses12": np.ascontiguousarray(poses, dtype=np.float32), "skeleton": skeleton}

    def run_simulation(self, waypoints: List[Waypoint], process_group=None) -> S3DISSimScene:
        """The scan stage (reference :220-296).  Inside an initialised ``torch.distributed`` job with more than one
        rank (one process per GPU, backend "nccl" = RCCL), or with an explicit ``process_group``, the waypoints are
        sharded over the ranks in contiguous blocks, ONE all-gather per scan assembles the scene, and every rank
        returns the complete S3DISSimScene -- identical to the single-process result."""
        if self.scene is None:
            raise ValueError("Scene not loaded. Call load_scene() first.")
        if self.raycast_engine is None:
            raise ValueError("Raycast engine is not initialized.")
        mesh = self.scene.room_mesh
        sim_scene = S3DISSimScene(scene_name=self.scene.scene_name, simulation_config=self.config, mesh=mesh,
                                  s3dis_data_root=self.config.get("s3dis_data_root"),
                                  area=self.config.get("area"), room=self.config.get("room"))
        start = time.time()
        total = self.lidar_config.get_total_points_per_scan()
        volume = self.scene.room_bounds.get_volume()

        # The whole trajectory in ONE launch; compaction into per-pose frames happens in HBM and only the kept rows
        # cross PCIe, into page-locked buffers -- the frames below are views of those (lrc_scan_poses_compact).
        # In bug-compatible mode the incident angles are overwritten with zeros anyway (reference :266-269), so they
        # are not even transferred.  range_origin is |point| from the WORLD origin (reference :283-284), float32,
        # formed on the device exactly as np.linalg.norm(points, axis=1) forms it.
        engine = self.raycast_engine
        # the per-frame mean / std of the ScanQuality records come from the device as well, computed with numpy's own
        # summation order (csrc/lrc_stats.h), so neither the range column nor a host reduction is needed
        from lidarcast.npmodel import reductions_match
        device_stats = reductions_match()       # a numpy that sums differently reduces the columns itself
        batched = isinstance(self.lidar_config, Indoor8LineLidarIntrinsics) and \
            self.lidar_config.vertical_degrees is not None
        # the hit triangles' labels are an extra of this package's frames (the reference's frame has none,
        # containers/s3dis_sim_frame.py:90-101): by default they stay on the device side -- a second, labels-only scan of
        # the same poses fetches them the first time a frame's labels are looked at (or at export) -- so that a caller who
        # never does is not made to wait for four of every sixteen bytes to cross PCIe.  raycast_engine.eager_labels: true
        # brings them with the points as before.
        # opt-in surface materials (config key ``materials: {classes: {window: {kind: glass, ...}, ...}, max_bounces?,
        # min_intensity?}``): a ray that meets glass or a mirror goes on inside the kernel; frames then
        # carry intensities, bounces and surface_points per point, and their labels come with the points.  Without the key
        # nothing changes.
        materials = self._material_table() if len(waypoints) > 0 else None
        # opt-in moving objects (config key ``movers: {period, objects: [{mesh, semantic, instance, path}, ...]}``): rigid meshes
        # at a different pose in every frame, traced in their own frames beside the room; frames then
        # carry mover_ids per point and their labels come with the points.  Without the key nothing changes.
        movers = self._mover_plan() if len(waypoints) > 0 else None
        lazy_labels = batched and materials is None and movers is None and not bool(self.config.get("raycast_engine", {}).get("eager_labels", False))
        want = ("point3",) + (() if lazy_labels else ("sem", "ins")) + \
            ("range_origin_stats" if device_stats else "range_origin",) + \
            (() if self.bug_compatible else (("incident_deg", "incident_stats") if device_stats else ("incident_deg",)))
        device_gen = bool(self.config.get("raycast_engine", {}).get("device_ray_generation", False))
        fr = None
        from lidarcast.distributed import active_group, scan_frames_sharded, scan_lidars_sharded
        dist, group = (None, None) if process_group is _NO_GROUP else active_group(process_group)
        # opt-in moving-sensor sweeps (config key ``motion: {speed: m/s}``): every ray is cast from the pose of the sensor at
        # the moment it fires; frames then carry per-point times.  Without the key nothing changes.
        motion = self.config.get("motion")
        sweep = sweep_noise = sweep_movers = None
        if motion is not None and len(waypoints) > 0:
            if dist is not None:
                raise NotImplementedError("moving-sensor sweeps are not available on a multi-rank process group")
            if not isinstance(self.lidar_config, Indoor8LineLidarIntrinsics):
                raise NotImplementedError("moving-sensor sweeps need a multi-line sensor (not the dual-axis sensor)")
            start_poses = poses_from_waypoints(waypoints)
            end_poses = sweep_end_poses(waypoints, self.lidar_config.scan_frequency, float(motion.get("speed", 0.0)))
            sweep = engine.sweep_inputs(self.lidar_config, start_poses, end_poses)
            # ... with seeded sensor noise under them (nested key ``motion: {speed, noise: {seed, range_std?, angle_std_deg?,
            # dropout?}}``, the entries of the noise key below): the row is jittered and the range drawn in the sweep's own
            # kernel; frame p has frame id p.  Without the nested entry nothing changes.
            # ... or with moving objects under them (nested key ``motion: {speed, movers: {period, objects: [...]}}``, the entries
            # of the movers key above): every ray meets each mover at the pose the mover has at the moment the ray fires (DESIGN.md
            # section 5n); sweep k starts at k * period and lasts 1 / scan_frequency; frames carry point_times AND mover_ids.
            # ... and seeded sensor noise under those (``sensor_noise: {seed, ...}`` under motion.movers).
            sweep_movers = self._mover_plan(nested=True)
            sweep_noise = self._noise_model(nested=True)
        # opt-in seeded sensor noise (config key ``noise: {seed, range_std?, angle_std_deg?, dropout?}``): range noise, angle
        # jitter and dropout drawn in the kernel; frame p of the run has frame id p, so scanning any
        # subset again reproduces it.  Without the key nothing changes.
        noise = self._noise_model() if len(waypoints) > 0 else None
        if noise is not None:
            if motion is not None:
                raise ValueError("the noise key cannot be combined with moving-sensor sweeps (motion): noise under sweeps is "
                                 "asked for with the nested key motion: {speed, noise: {seed, ...}}")
            if dist is not None:
                raise ValueError("the noise key is not available on a multi-rank process group")
            if not batched:
                raise ValueError("the noise key needs a multi-line sensor with a direction table (not the dual-axis sensor)")
        # opt-in beam footprint (config key ``beam: {divergence_mrad, pattern?, max_echoes?, separation?, min_fraction?}``):
        # every table row is a diverging beam of sub-rays reduced to echoes in the kernel; a frame then
        # holds up to max_echoes points per beam and carries beam_index, echo_index and echo_weight per point.  Without the key
        # nothing changes.
        beam = self._beam_model() if len(waypoints) > 0 else None
        if beam is not None:
            if motion is not None:
                raise ValueError("the beam key cannot be combined with moving-sensor sweeps (motion)")
            if noise is not None:
                raise ValueError("the beam key cannot be combined with the noise key")
            if dist is not None:
                raise ValueError("the beam key is not available on a multi-rank process group")
            if not batched:
                raise ValueError("the beam key needs a multi-line sensor with a direction table (not the dual-axis sensor)")
        if movers is not None:
            if dist is not None:
                raise ValueError("the movers key is not available on a multi-rank process group")
            if not batched:
                raise ValueError("the movers key needs a multi-line sensor with a direction table (not the dual-axis sensor)")
            from lidarcast.movers import MoverSet
            times = np.arange(len(waypoints), dtype=np.float64) * movers["period"]
            states = np.stack([t.state(times) for t in movers["tracks"]], axis=1)            # (P, M, 4): x, y, z, yaw
            mover_poses = np.stack([t.poses12(times) for t in movers["tracks"]], axis=1)       # (P, M, 12) float32
            animated = [m for m, c in enumerate(movers["clips"]) if c is not None]
            deformables, mset = {}, None
            try:
                if animated:        # deforming movers: one Deformable each, set per run of frames with equal shapes
                    from lidarcast import deform
                    for m in animated:
                        mm = movers["meshes"][m]
                        rig = movers["skins"][m]
                        if rig is not None:         # bone poses skinned on the device
                            deformables[m] = deform.SkinnedDeformable(engine.ctx, rig["rest"], mm.triangles, rig["bone_index"],
                                                                      rig["bone_weight"], rig["poses12"], mm.triangle_sem,
                                                                      mm.triangle_ins)
                            continue
                        deformables[m] = deform.Deformable(engine.ctx, movers["keyframes"][m], mm.triangles, mm.triangle_sem,
                                                           mm.triangle_ins)
                    mset = MoverSet(engine.ctx, [deformables.get(m, mm) for m, mm in enumerate(movers["meshes"])])
                    shapes = np.stack([movers["clips"][m].shapes3(times) for m in animated], axis=1)      # (P, D, 3)
                    scan = deform.scan_deforming_flow_frames if movers["nonrigid_flow"] else deform.scan_deforming_frames
                    extra = {} if movers["noise"] is None else {"noise": movers["noise"]}      # (never beside nonrigid_flow)
                    fr = scan(engine, self.lidar_config, poses_from_waypoints(waypoints), mesh, mset, mover_poses, shapes,
                              want=want, **extra)
                else:
                    mset = MoverSet(engine.ctx, movers["meshes"])
                    if movers["noise"] is not None:      # seeded noise drawn in the mover kernels
                        fr = engine.scan_noisy_mover_frames(self.lidar_config, poses_from_waypoints(waypoints), mesh, mset,
                                                            mover_poses, movers["noise"], want=want)
                    else:
                        scan = engine.scan_flow_frames if movers["flow"] or movers["nonrigid_flow"] else engine.scan_mover_frames
                        fr = scan(self.lidar_config, poses_from_waypoints(waypoints), mesh, mset, mover_poses, want=want)
            finally:
                if mset is not None:
                    mset.close()
                for d in deformables.values():
                    d.close()
            sim_scene.mover_tracks = {"period": movers["period"], "objects": movers["objects"], "times": times,
                                      "states": states, "poses12": mover_poses,
                                      "sensor_poses": poses_from_waypoints(waypoints)}
            if movers["noise"] is not None:
                sim_scene.mover_tracks["noise"] = movers["noise"]
            if animated:
                sim_scene.mover_tracks["shapes"] = {m: movers["clips"][m].shapes3(times) for m in animated}
                sim_scene.mover_tracks["keyframes"] = {m: movers["keyframes"][m] for m in animated if movers["skins"][m] is None}
                sim_scene.mover_tracks["skins"] = {m: movers["skins"][m] for m in animated if movers["skins"][m] is not None}
        elif materials is not None:
            if dist is not None:
                raise ValueError("the materials key is not available on a multi-rank process group")
            if not batched:
                raise ValueError("the materials key needs a multi-line sensor with a direction table (not the dual-axis sensor)")
            fr = engine.scan_material_frames(self.lidar_config, poses_from_waypoints(waypoints), mesh, materials, want=want)
        elif beam is not None:
            fr = engine.scan_echo_frames(self.lidar_config, poses_from_waypoints(waypoints), mesh, beam, want=want)
        elif noise is not None:
            fr = engine.scan_noisy_frames(self.lidar_config, poses_from_waypoints(waypoints), mesh, noise, want=want)
        elif sweep is not None and sweep_movers is not None:
            from lidarcast.movers import MoverSet, scan_mover_sweep_frames, scan_noisy_mover_sweep_frames, sweep_records
            duration = 1.0 / float(self.lidar_config.scan_frequency)
            times = np.arange(len(waypoints), dtype=np.float64) * sweep_movers["period"]
            states = np.stack([t.state(times) for t in sweep_movers["tracks"]], axis=1)                  # (P, M, 4) at the sweep's start
            end_states = np.stack([t.state(times + duration) for t in sweep_movers["tracks"]], axis=1)   # ... and at its end
            records = sweep_records(sweep_movers["tracks"], times, times + duration)                      # (P, M, 24) float32
            if "sem" not in want:           # the labels are the winner's: they come with the points
                want = want[:1] + ("sem", "ins") + want[1:]
            animated = [m for m, c in enumerate(sweep_movers["clips"]) if c is not None]
            deformables, mset = {}, None
            try:
                if animated:        # animated movers under sweeps: a per-ray shape between the sweep's two end shapes
                    from lidarcast import deform
                    for m in animated:
                        mm, rig = sweep_movers["meshes"][m], sweep_movers["skins"][m]
                        if rig is not None:
                            deformables[m] = deform.SkinnedDeformable(engine.ctx, rig["rest"], mm.triangles, rig["bone_index"],
                                                                      rig["bone_weight"], rig["poses12"], mm.triangle_sem,
                                                                      mm.triangle_ins)
                        else:
                            deformables[m] = deform.Deformable(engine.ctx, sweep_movers["keyframes"][m], mm.triangles,
                                                               mm.triangle_sem, mm.triangle_ins)
                    mset = MoverSet(engine.ctx, [deformables.get(m, mm) for m, mm in enumerate(sweep_movers["meshes"])])
                    shapes_a = np.stack([sweep_movers["clips"][m].shapes3(times) for m in animated], axis=1)             # (P, D, 3)
                    shapes_b = np.stack([sweep_movers["clips"][m].shapes3(times + duration) for m in animated], axis=1)
                    extra = {} if sweep_movers["noise"] is None else {"noise": sweep_movers["noise"]}
                    fr = deform.scan_deforming_sweep_frames(engine, self.lidar_config, None, None, mesh, mset, records, shapes_a,
                                                            shapes_b, want=want, inputs=sweep, **extra)
                else:
                    mset = MoverSet(engine.ctx, sweep_movers["meshes"])
                    if sweep_movers["noise"] is not None:      # seeded noise drawn in the sweep's mover kernels
                        fr = scan_noisy_mover_sweep_frames(engine, self.lidar_config, None, None, mesh, mset, records,
                                                           sweep_movers["noise"], want=want, inputs=sweep)
                    else:
                        fr = scan_mover_sweep_frames(engine, self.lidar_config, None, None, mesh, mset, records, want=want,
                                                     inputs=sweep)
            finally:
                if mset is not None:
                    mset.close()
                for d in deformables.values():
                    d.close()
            sim_scene.mover_tracks = {"period": sweep_movers["period"], "objects": sweep_movers["objects"], "times": times,
                                      "states": states, "poses12": records[:, :, :12], "sensor_poses": poses_from_waypoints(waypoints),
                                      "end_states": end_states, "records24": records, "sweep_duration": duration}
            if sweep_movers["noise"] is not None:
                sim_scene.mover_tracks["noise"] = sweep_movers["noise"]
            if animated:
                sim_scene.mover_tracks["shapes"] = {m: shapes_a[:, j] for j, m in enumerate(animated)}
                sim_scene.mover_tracks["end_shapes"] = {m: shapes_b[:, j] for j, m in enumerate(animated)}
                sim_scene.mover_tracks["keyframes"] = {m: sweep_movers["keyframes"][m] for m in animated if sweep_movers["skins"][m] is None}
                sim_scene.mover_tracks["skins"] = {m: sweep_movers["skins"][m] for m in animated if sweep_movers["skins"][m] is not None}
        elif sweep is not None and sweep_noise is not None:
            from lidarcast.noise import scan_noisy_sweep_frames
            fr = scan_noisy_sweep_frames(engine, self.lidar_config, None, None, mesh, sweep_noise, want=want, inputs=sweep)
        elif sweep is not None:
            fr = engine.scan_sweep_frames(self.lidar_config, None, None, mesh, want=want, inputs=sweep)
        elif dist is not None and len(waypoints) > 0:
            if batched:
                fr = scan_frames_sharded(engine, self.lidar_config, poses_from_waypoints(waypoints), mesh, dist, group)
            else:
                lidars = [create_lidar(self.lidar_config, wp.to_pose_matrix()) for wp in waypoints]
                fr = scan_lidars_sharded(engine, lidars, mesh, dist, group)
            # attributes the gathered rows do not carry are the reference's own numpy expressions of the points; the
            # range statistics come from the device when the engine computed them on the assembled rows
            from lidarcast.npmodel import reductions_match
            if "range_origin_mean" in fr and not reductions_match():
                del fr["range_origin_mean"], fr["range_origin_std"]
            if "range_origin_mean" not in fr:
                fr["range_origin"] = np.linalg.norm(fr["point3"], axis=1) if fr["total"] else np.zeros(0, np.float32)
            if not self.bug_compatible:
                fr.pop("range_origin_mean", None), fr.pop("range_origin_std", None)     # angle statistics: host numpy
                if "range_origin" not in fr:
                    fr["range_origin"] = np.linalg.norm(fr["point3"], axis=1) if fr["total"] else np.zeros(0, np.float32)
                cen = np.repeat(np.stack([wp.to_pose_matrix()[:3, 3] for wp in waypoints]), fr["counts"], axis=0)
                v = fr["point3"] - cen
                v = v / np.linalg.norm(v, axis=1, keepdims=True)
                fr["incident_deg"] = np.degrees(np.arccos(np.abs(v[:, 2])))      # raycast_engine_cpu.py:100-107
        elif len(waypoints) > 0 and batched:
            fr = engine.scan_frames(self.lidar_config, poses_from_waypoints(waypoints), mesh, want=want)
        elif len(waypoints) > 0 and device_gen and isinstance(self.lidar_config, DualAxisLidarIntrinsics):
            # opt-in: dual-axis rays generated in the kernel from the host-drawn scan angles
            lidars = [create_lidar(self.lidar_config, wp.to_pose_matrix()) for wp in waypoints]
            fr = engine.scan_frames_dual_axis(lidars, mesh, want=want)
        elif len(waypoints) > 0 and isinstance(self.lidar_config, DualAxisLidarIntrinsics) and \
                hasattr(engine, "scan_frames_lidars"):
            # host-generated rays (dual-axis sensor, the bit-exact default): all rays of all poses at a fixed stride with
            # the dropout mask, one launch, compaction and statistics in HBM
            lidars = [create_lidar(self.lidar_config, wp.to_pose_matrix()) for wp in waypoints]
            fr = engine.scan_frames_lidars(lidars, mesh, want=want)
        elif len(waypoints) > 0:
            # any other sensor object with get_rays(): all poses in one launch, ragged segments, masked on the host
            lidars = [create_lidar(self.lidar_config, wp.to_pose_matrix()) for wp in waypoints]
            seg, off = engine.scan_lidars(lidars, mesh, want=("t", "point3", "incident_deg", "sem", "ins"))
        if fr is not None:
            if self.bug_compatible:            # one zero block, frames take views of it (reference :266-269)
                fr["incident_deg"] = np.zeros(fr["total"])
            counts_l = fr["counts"].tolist()
            ends_l = list(itertools.accumulate(counts_l))
            pts_f, ang_f = ([fr[a][e - c:e] for c, e in zip(counts_l, ends_l)] for a in ("point3", "incident_deg"))
            if "sem" in fr:
                sem_f, ins_f = ([fr[a][e - c:e] for c, e in zip(counts_l, ends_l)] for a in ("sem", "ins"))
                src_f = itertools.repeat(None)
            else:      # labels on demand: one labels-only scan of the trajectory (of the SAME sweeps), shared by its frames
                sem_f = ins_f = itertools.repeat(None)
                src_f = itertools.repeat(_LazyTrajectoryLabels(engine, self.lidar_config, poses_from_waypoints(waypoints),
                                                               mesh, counts_l, sweep, noise if sweep is None else sweep_noise,
                                                               beam))
            if "range_origin_mean" in fr:      # statistics from the device
                qual = self._quality_from_stats(fr, total, volume)
            else:
                # (sharded scans) per-frame statistics are numpy reductions over 10^4..10^5 values each; they release
                # the GIL, so the frames of a long trajectory are reduced side by side (same numpy calls, same values)
                qual = self._quality_many(pts_f, ang_f, total, volume, engine.split_frames(fr, "range_origin"))
        if fr is not None:
            first = len(sim_scene.frames)
            sim_scene.frames.extend(map(S3DISSimFrame, range(len(waypoints)), pts_f, ang_f, qual, itertools.repeat(None),
                                        sem_f, ins_f, src_f))
            if "point_times" in fr:        # seconds since the start of the frame's sweep, per point
                for f, e, c in zip(sim_scene.frames[first:], ends_l, counts_l):
                    f.point_times = fr["point_times"][e - c:e]
            if "echo_weight" in fr:        # per point: its beam (table row), its place among the beam's echoes, the sub-rays behind it
                for f, e, c in zip(sim_scene.frames[first:], ends_l, counts_l):
                    f.beam_index, f.echo_index, f.echo_weight = (fr[a][e - c:e] for a in ("beam_index", "echo_index", "echo_weight"))
            if "mover" in fr:              # per point: 0 for the room, m + 1 for mover m of the movers key
                for f, e, c in zip(sim_scene.frames[first:], ends_l, counts_l):
                    f.mover_ids = fr["mover"][e - c:e]
            if "flow_status" in fr:        # per point: where its surface goes up to the next frame, and whether it is seen there
                for f, e, c in zip(sim_scene.frames[first:], ends_l, counts_l):
                    f.flow, f.flow_status = fr["flow"][e - c:e], fr["flow_status"][e - c:e]
            if "bounces" in fr:            # per point: the return's strength, the panes and mirrors on its way, where it came from
                for f, e, c in zip(sim_scene.frames[first:], ends_l, counts_l):
                    f.intensities, f.bounces, f.surface_points = (fr[a][e - c:e] for a in ("intensity", "bounces", "surface_point3"))
        for i, wp in enumerate(waypoints if fr is None else ()):
            a, b = off[i], off[i + 1]
            keep = seg["t"][a:b] != np.inf
            points, angles = seg["point3"][a:b][keep], seg["incident_deg"][a:b][keep]
            sem, ins = seg["sem"][a:b][keep], seg["ins"][a:b][keep]
            if self.bug_compatible:
                angles = np.zeros(len(points))                # reference :266-269
            q = self._quality(points, angles, total, volume)
            sim_scene.append_frame(S3DISSimFrame(i, points, angles, q, semantic_labels=sem,
                                                 instance_labels=ins))
        sim_scene.compute_statistics(time.time() - start)
        return sim_scene


class _LazyTrajectoryLabels:
    """The hit triangles' labels of a scanned trajectory, fetched when a frame is first asked for them: one labels-only scan
    of the same poses over the same mesh (the scan is a pure function of both: same kept rays, same order), whose result
    all frames of the trajectory share."""

    def __init__(self, engine, intrinsics, poses, mesh, counts, sweep=None, noise=None, beam=None):
        # sweep: the (motion records, fire table, period) of a moving-sensor scan -- rescanned exactly, never as static poses
        # noise: the NoiseModel of a noisy scan -- rescanned with the same seed and frame ids, never as the clean scan
        # both: noisy moving-sensor sweeps -- rescanned as such from the same records and model, never as either alone
        self._args = (engine, intrinsics, np.array(poses, dtype=np.float64, copy=True), mesh)
        self._sweep = sweep
        self._noise = noise
        self._beam = beam      # the BeamModel of an echo scan -- rescanned as echoes, never as the clean labels-only scan
        self._counts = list(counts)
        self._sem = self._ins = None
        import threading
        self._lock = threading.Lock()

    def frame_labels(self, i):
        with self._lock:
            if self._sem is None:
                engine, intrinsics, poses, mesh = self._args
                if self._beam is not None:
                    fr = engine.scan_echo_frames(intrinsics, poses, mesh, self._beam, want=("sem", "ins"))
                elif self._sweep is not None and self._noise is not None:
                    from lidarcast.noise import scan_noisy_sweep_frames
                    fr = scan_noisy_sweep_frames(engine, intrinsics, None, None, mesh, self._noise, want=("sem", "ins"),
                                                 inputs=self._sweep)
                elif self._noise is not None:
                    fr = engine.scan_noisy_frames(intrinsics, poses, mesh, self._noise, want=("sem", "ins"))
                elif self._sweep is not None:
                    fr = engine.scan_sweep_frames(intrinsics, None, None, mesh, want=("sem", "ins"), inputs=self._sweep)
                else:
                    fr = engine.scan_frames(intrinsics, poses, mesh, want=("sem", "ins"))
                if fr["counts"].tolist() != self._counts:
                    raise RuntimeError("the mesh or the scan options changed between the scan and the first look at its labels")
                self._sem, self._ins, self._ends = fr["sem"], fr["ins"], list(itertools.accumulate(self._counts))
                self._args = self._sweep = self._noise = self._beam = None
        e, c = self._ends[i], self._counts[i]
        return self._sem[e - c:e], self._ins[e - c:e]


def load_config(config_path: str) -> Dict[str, Any]:
    """YAML configuration file -> dict (reference :458-465)."""
    import yaml
    with open(config_path, "r", encoding="utf-8") as f:
        return yaml.safe_load(f)


def load_default_config() -> Dict[str, Any]:
    """configs/default_config.yaml next to this module (the reference looks for the same file and does not ship
    it either: FileNotFoundError there and here)."""
    return load_config(str(Path(__file__).parent / "configs" / "default_config.yaml"))


def create_simulator_from_config(config_path: Optional[str] = None) -> S3DISSimulator:
    return S3DISSimulator(load_default_config() if config_path is None else load_config(config_path))


def run_scene_batch(scenes, trajectories, sensor=None, config: Optional[Dict[str, Any]] = None,
                    use_dense_lidar: bool = False, use_blk2go: bool = False, output_base_dir=None,
                    process_group=None, skip_existing: bool = True, on_scene=None) -> Dict[str, Any]:
    """Several scenes through one simulator, the job of the reference's batch loop (s3dis_simulator.py:594-726:
    per scene load -> trajectory -> run_simulation -> save_results, failures collected, finished scenes skipped) as
    a function instead of a hard-coded ``main``.

    scenes        list of (name, mesh object or PLY path)
    trajectories  {name: waypoints (List[Waypoint]) or (P,4,4) poses}, or an int = waypoints planned per scene
    sensor        optional intrinsics record replacing the simulator's default (e.g. a 32-line x 2048 sweep)
    output_base_dir  results of scene ``name`` go to <dir>/<name>; a scene whose labelled cloud and statistics
                  file exist is skipped (the reference's resume rule, :637-648)
    on_scene      optional callable (name, sim_scene): called when a scene is done (after its files are written); the scene
                  is then NOT kept in the report, as the reference's loop keeps none (:661-700) -- its frames' page-locked
                  buffers go back to the pool and the next scene's scan reuses them instead of locking fresh pages
    Inside a torch.distributed job the scenes are dealt round-robin to the ranks (each scene is one rank's work, its
    trajectory is not sharded again) and the per-scene summaries are gathered; ``sim_scene`` objects stay on the
    rank that produced them.  Returns {"scenes": {name: {...}}, "failed": [...], "skipped": [...], "total_rays",
    "seconds", "rays_per_s", "build_seconds", "seconds_including_build", "rays_per_s_including_build"}: ``seconds`` = the
    scan stages only, ``build_seconds`` = the scene builds (mesh -> BVH resident in HBM, which the reference pays per
    POSE, raycast_engine_cpu.py:46-47, and this engine once per mesh, on the GPU); file writing is in neither."""
    from lidarcast.distributed import active_group
    dist, group = active_group(process_group)
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if dist is not None else (0, 1)
    sim = S3DISSimulator(config or {"raycast_engine": {"use_gpu": True}}, use_dense_lidar=use_dense_lidar,
                         use_blk2go=use_blk2go)
    if sensor is not None:
        sim.lidar_config = sensor
    done, failed, skipped = {}, [], []
    rays_per_pose = sim.lidar_config.get_total_points_per_scan()
    for i, (name, source) in enumerate(scenes):
        if i % world != rank:
            continue
        out_dir = None if output_base_dir is None else Path(output_base_dir) / name
        if (skip_existing and out_dir is not None and (out_dir / "combined_pointcloud_with_label.ply").exists()
                and (out_dir / "simulation_statistics.txt").exists()):
            skipped.append(name)
            continue
        try:
            sim.load_scene(source, name)
            traj = trajectories if isinstance(trajectories, int) else trajectories[name]
            if isinstance(traj, int):
                waypoints, _ = sim.generate_auto_trajectory(traj)
            elif isinstance(traj, np.ndarray):
                waypoints = [Waypoint(m[0, 3], m[1, 3], m[2, 3], yaw=float(np.arctan2(m[1, 0], m[0, 0])),
                                      timestamp=float(k)) for k, m in enumerate(traj.reshape(-1, 4, 4))]
            else:
                waypoints = list(traj)
            tb = time.perf_counter()
            sim.raycast_engine.scene_for(sim.scene.room_mesh)        # scene build: timed on its own
            t0 = time.perf_counter()
            sim_scene = sim.run_simulation(waypoints, process_group=_NO_GROUP)
            dt = time.perf_counter() - t0
            if out_dir is not None:
                sim.save_results(sim_scene, out_dir, waypoints)
            done[name] = {"sim_scene": sim_scene, "frames": len(sim_scene.frames), "rays": len(waypoints) * rays_per_pose,
                          "points": int(sim_scene.get_total_points()), "seconds": dt, "build_seconds": t0 - tb}
            if on_scene is not None:
                on_scene(name, sim_scene)
                done[name]["sim_scene"] = None
            del sim_scene
        except Exception as e:                                       # noqa: BLE001 - the reference collects and goes on
            failed.append((name, str(e)))
    if dist is not None:
        parts = [None] * world
        summary = {k: {a: b for a, b in v.items() if a != "sim_scene"} for k, v in done.items()}
        dist.all_gather_object(parts, (summary, failed, skipped), group=group)
        for r, (sm, fl, sk) in enumerate(parts):
            if r != rank:
                done.update(sm)
                failed += fl
                skipped += sk
        seconds = max(sum(v["seconds"] for v in part[0].values()) for part in parts)    # ranks work side by side
        with_build = max(sum(v["seconds"] + v["build_seconds"] for v in part[0].values()) for part in parts)
    else:
        seconds = sum(v["seconds"] for v in done.values())
        with_build = sum(v["seconds"] + v["build_seconds"] for v in done.values())
    total_rays = sum(v["rays"] for v in done.values())
    order = [n for n, _ in scenes]
    return {"scenes": {n: done[n] for n in order if n in done}, "failed": failed, "skipped": skipped, "ranks": world,
            "total_rays": int(total_rays), "seconds": seconds, "rays_per_s": total_rays / seconds if seconds > 0 else 0.0,
            "build_seconds": with_build - seconds, "seconds_including_build": with_build,
            "rays_per_s_including_build": total_rays / with_build if with_build > 0 else 0.0}
