"""Detection boxes of the object instances of a labelled cloud (include/lidarcast.h, "detection boxes";
csrc/lrc_boxes.hip): the k-NN statistical outlier filter of Open3D's remove_statistical_outlier inside every instance
and the axis-aligned box of what is left, all instances in one device call (reference:
lidar_net_bbox_visualizer.py:163-249)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check

# one row per instance of min_points rows or more, ordered by (position of the class in class_ids, ins); the layout
# of lrc_box
BOX_DTYPE = np.dtype([("sem", "<u2"), ("ins", "<u2"), ("num_points", "<u4"), ("num_kept", "<u4"), ("filtered", "<u4"),
                      ("min3", "<f4", (3,)), ("max3", "<f4", (3,)), ("mean", "<f8"), ("threshold", "<f8")])


def _class_array(class_ids):
    ids = np.ascontiguousarray(np.asarray(class_ids, dtype=np.int64).reshape(-1))
    if ids.size and (ids.min() < 0 or ids.max() > 0xFFFF):
        raise ValueError("class ids must be uint16")
    return ids.astype(np.uint16)


def _capacity(num_rows, min_points, num_classes):
    return int(min(num_rows // max(int(min_points), 1), num_classes * 0xFFFF))


def instance_boxes(ctx, points, sem, ins, class_ids, min_points=10, k=20, std_ratio=2.0, cell_size=0.0, return_rows=False):
    """Host arrays: points (K,3) float32, sem / ins (K,) uint16.  Returns the BOX_DTYPE array, and with return_rows also
    the per-row avg distance (float64, -1 where the filter did not run) and keep flag (uint8, 1 = inside its box)."""
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be (K, 3)")
    s = np.ascontiguousarray(np.asarray(sem), dtype=np.uint16)
    i = np.ascontiguousarray(np.asarray(ins), dtype=np.uint16)
    if s.shape != (len(p),) or i.shape != (len(p),):
        raise ValueError("sem and ins must have shape (K,)")
    ids = _class_array(class_ids)
    cap = _capacity(len(p), min_points, len(ids))
    out = np.empty(cap, dtype=BOX_DTYPE)
    avg = np.empty(len(p), dtype=np.float64) if return_rows else None
    keep = np.empty(len(p), dtype=np.uint8) if return_rows else None
    nb = C.c_uint64(0)
    check(_capi.load().lrc_instance_boxes(
        ctx._h, p.ctypes.data, s.ctypes.data, i.ctypes.data, len(p), ids.ctypes.data, len(ids), int(min_points), int(k),
        float(std_ratio), float(cell_size), out.ctypes.data if cap else None, cap, C.byref(nb),
        None if avg is None else avg.ctypes.data, None if keep is None else keep.ctypes.data), "lrc_instance_boxes")
    boxes = out[:nb.value].copy()
    return (boxes, avg, keep) if return_rows else boxes


def instance_boxes_dev(ctx, xyzl_t, class_ids, min_points=10, k=20, std_ratio=2.0, cell_size=0.0, return_rows=False,
                       stream=0):
    """xyzl_t: (K,4) float32 device tensor of rows x, y, z, label bits (sem | ins<<16), e.g. the scan pipeline's rows.
    The cloud stays on the device; the boxes come back as a BOX_DTYPE array (the call returns once `stream` has run
    its work).  return_rows: also the per-row avg (float64) and keep (uint8) device tensors."""
    import torch
    if xyzl_t.dim() != 2 or xyzl_t.shape[1] != 4 or xyzl_t.dtype != torch.float32 or not xyzl_t.is_contiguous():
        raise ValueError("rows must be a contiguous (K, 4) float32 tensor")
    K = xyzl_t.shape[0]
    ids = _class_array(class_ids)
    cap = _capacity(K, min_points, len(ids))
    out = np.empty(cap, dtype=BOX_DTYPE)
    avg_t = keep_t = None
    if return_rows:
        avg_t = torch.empty(K, dtype=torch.float64, device=xyzl_t.device)
        keep_t = torch.empty(K, dtype=torch.uint8, device=xyzl_t.device)
    nb = C.c_uint64(0)
    check(_capi.load().lrc_instance_boxes_dev(
        ctx._h, C.c_void_p(xyzl_t.data_ptr()), K, ids.ctypes.data, len(ids), int(min_points), int(k), float(std_ratio),
        float(cell_size), out.ctypes.data if cap else None, cap, C.byref(nb),
        None if avg_t is None else C.c_void_p(avg_t.data_ptr()), None if keep_t is None else C.c_void_p(keep_t.data_ptr()),
        C.c_void_p(int(stream))), "lrc_instance_boxes_dev")
    boxes = out[:nb.value].copy()
    return (boxes, avg_t, keep_t) if return_rows else boxes
