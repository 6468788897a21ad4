"""Boxes of many float64 objects in one device call (include/lidarcast.h, "object boxes"; csrc/lrc_objboxes.hip): Open3D's
remove_statistical_outlier(nb_neighbors=k, std_ratio) inside each object and the axis-aligned box of the kept rows
(reference: s3dis_bbox_visualizer.py:70-116, one Annotations/<class>_<k>.txt file per object).

Objects are runs of one concatenated (n, 3) cloud: object s is rows [offsets[s], offsets[s+1]).  An object of m >= k rows
gets exactly what lrc_cloud_preprocess(nb_neighbors=k, std_ratio) computes for that object alone (avg, keep, mean and
threshold bit for bit); an object of m < k rows keeps every row (avg = -1, mean = 0, threshold = +inf), as the reference
returns such points untouched.  Parity with Open3D itself (its summation order) is not pinned: Open3D is absent here.
1 <= k <= 32; n and the object count below 2^31; a non-finite coordinate raises (LRC_ERR_INVALID_ARG)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import check

# one row per object, in object order; the layout of lrc_objbox
OBJBOX_DTYPE = np.dtype([("num_points", "<u8"), ("num_kept", "<u8"), ("filtered", "<u4"), ("reserved_", "<u4"),
                         ("min3", "<f8", (3,)), ("max3", "<f8", (3,)), ("mean", "<f8"), ("threshold", "<f8")])


@dataclass
class ObjectBoxes:
    boxes: np.ndarray                # (S,) OBJBOX_DTYPE; min3 = +inf, max3 = -inf where nothing was kept
    kept: object                     # kept row indices, ascending (object after object); uint32 array or int32 tensor
    kept_offsets: np.ndarray         # (S+1,) int64: object s's kept rows are kept[kept_offsets[s]:kept_offsets[s+1]]
    avg: object = None               # (n,) float64 mean k-NN distance per row (-1 where the filter did not run)
    keep: object = None              # (n,) uint8 1 = the row is inside its object's box

    def kept_rows(self, s):
        """Object s's kept rows as indices into the concatenated cloud (ascending)."""
        return self.kept[int(self.kept_offsets[s]):int(self.kept_offsets[s + 1])]


def _offsets(offsets):
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if len(off) < 1:
        raise ValueError("offsets need num_objects + 1 entries")
    return off.view(np.uint64)          # a negative entry wraps to a huge one, which the library rejects


def _kept_offsets(boxes):
    return np.concatenate([[0], np.cumsum(boxes["num_kept"].astype(np.int64))])


def object_boxes(ctx, points, offsets, k=20, std_ratio=2.0, cell_size=0.0, return_rows=False):
    """Host points (n, 3) (converted to float64) and offsets (S+1,).  Returns an ObjectBoxes record; return_rows adds the
    per-row avg and keep arrays."""
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be (n, 3)")
    n = len(p)
    off = _offsets(offsets)
    S = len(off) - 1
    boxes = np.zeros(S, dtype=OBJBOX_DTYPE)
    kept = np.empty(n, dtype=np.uint32)
    avg = np.empty(n, dtype=np.float64) if return_rows else None
    keep = np.empty(n, dtype=np.uint8) if return_rows else None
    check(_capi.load().lrc_object_boxes(
        ctx._h, p.ctypes.data if n else None, n, off.ctypes.data, S, int(k), float(std_ratio), float(cell_size),
        boxes.ctypes.data if S else None, kept.ctypes.data if n else None,
        None if avg is None or not n else avg.ctypes.data, None if keep is None or not n else keep.ctypes.data),
        "lrc_object_boxes")
    ko = _kept_offsets(boxes)
    return ObjectBoxes(boxes, kept[:ko[-1]].copy(), ko, avg, keep)


def object_boxes_dev(ctx, points_t, offsets, k=20, std_ratio=2.0, cell_size=0.0, return_rows=False, stream=0):
    """points_t: contiguous (n, 3) float64 device tensor; offsets: host (S+1,).  The boxes come back as an OBJBOX_DTYPE
    array, kept (int32 view of the uint32 indices) and with return_rows avg / keep as device tensors; the call returns
    once `stream` has run its work."""
    import torch
    if points_t.dim() != 2 or points_t.shape[1] != 3 or points_t.dtype != torch.float64 or not points_t.is_contiguous():
        raise ValueError("points must be a contiguous (n, 3) float64 tensor")
    n = points_t.shape[0]
    dev = points_t.device
    off = _offsets(offsets)
    S = len(off) - 1
    boxes = np.zeros(S, dtype=OBJBOX_DTYPE)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    avg = torch.empty(n, dtype=torch.float64, device=dev) if return_rows else None
    keep = torch.empty(n, dtype=torch.uint8, device=dev) if return_rows else None

    def ptr(t):
        return None if t is None or not n else C.c_void_p(t.data_ptr())
    check(_capi.load().lrc_object_boxes_dev(
        ctx._h, ptr(points_t), n, off.ctypes.data, S, int(k), float(std_ratio), float(cell_size),
        boxes.ctypes.data if S else None, ptr(kept), ptr(avg), ptr(keep), C.c_void_p(int(stream))),
        "lrc_object_boxes_dev")
    ko = _kept_offsets(boxes)
    return ObjectBoxes(boxes, kept[:int(ko[-1])], ko, avg, keep)
