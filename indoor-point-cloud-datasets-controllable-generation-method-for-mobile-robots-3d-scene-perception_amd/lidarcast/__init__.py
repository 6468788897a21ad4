"""lidarcast -- Python face of liblidarcast, the MI355X-native LiDAR ray-cast scan engine."""
from ._capi import LIB_PATH, LRC_INVALID_PRIM, LidarcastError, load
from .core import (ATTRS, FRAME_ATTRS, Context, DeviceHits, DirectionTable, NearestIndex, OccupancyIndex, PinnedPool, ScanPipe, Scene,
                   bake_triangle_labels, motion_records)
from .boxes import BOX_DTYPE, instance_boxes, instance_boxes_dev
from .preprocess import (Preprocessed, estimate_normals, preprocess_cloud, preprocess_cloud_dev,
                         remove_statistical_outlier)
from .objboxes import OBJBOX_DTYPE, ObjectBoxes, object_boxes, object_boxes_dev
from .coverage import CoverageSummary, SurfaceCoverage, scan_coverage
from .voxgrid import OccupancyGrid, OccupancyResult, scan_occupancy
from .voxseq import DynamicOccupancyResult, OccupancySequence, scan_dynamic_occupancy
from .frameobj import FrameObjects, FrameObjectsResult, scan_frame_objects
from .noise import NoiseModel
from . import flow  # noqa: F401  (binds Scene.scan_flow_dev / Scene.scan_flow_compact)
from . import movers  # noqa: F401  (binds Scene.scan_noisy_movers_dev / Scene.scan_noisy_movers_compact)

__all__ = ["LIB_PATH", "LRC_INVALID_PRIM", "LidarcastError", "load", "ATTRS", "Context",
           "DeviceHits", "DirectionTable", "Scene", "motion_records", "ScanPipe", "PinnedPool", "FRAME_ATTRS", "NearestIndex", "OccupancyIndex", "bake_triangle_labels", "BOX_DTYPE", "instance_boxes", "instance_boxes_dev",
           "Preprocessed", "preprocess_cloud", "preprocess_cloud_dev", "remove_statistical_outlier", "estimate_normals",
           "OBJBOX_DTYPE", "ObjectBoxes", "object_boxes", "object_boxes_dev", "CoverageSummary", "SurfaceCoverage",
           "scan_coverage", "OccupancyGrid", "OccupancyResult", "scan_occupancy", "OccupancySequence",
           "DynamicOccupancyResult", "scan_dynamic_occupancy", "FrameObjects",
           "FrameObjectsResult", "scan_frame_objects", "NoiseModel", "version",
           "device_count"]


def version():
    return load().lrc_version().decode()


def device_count():
    return int(load().lrc_device_count())
