"""Room preprocessing of a float64 cloud (include/lidarcast.h, "cloud preprocessing"; csrc/lrc_preprocess.hip): Open3D's
remove_statistical_outlier(nb_neighbors, std_ratio) and estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) on
the kept rows, in one device call (reference: s3dis_data_loader.py:85-158).

Neighbours of the normal search are the rows with d2 < radius^2, itself included, ordered by (d2, index), the first
max_nn; the normal is the unit eigenvector of the smallest eigenvalue of Open3D's cumulant covariance from the
closed-form 3x3 solver (Eberly) that Open3D's default fast_normal_computation path uses.  The sign is the solver's: no
orientation is applied, and parity of the sign with Open3D is not pinned (Open3D is absent here).  1 <= nb_neighbors,
max_nn <= 32 (the neighbour lists live in registers)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import LrcPreprocessOpts, check


@dataclass
class Preprocessed:
    kept: np.ndarray                 # (m,) uint32 kept row indices, ascending (Open3D's `ind`)
    normals: object = None           # (m, 3) float64, kept order; None without estimate_normals
    avg: object = None               # (n,) float64 mean k-NN distance per input row (-1 where the filter did not run)
    nn_count: object = None          # (m,) uint8 neighbours used per normal
    mean: float = 0.0                # filter statistics (0 and +inf without the filter)
    threshold: float = float("inf")


def _opts(remove_outliers, nb_neighbors, std_ratio, estimate_normals, radius, max_nn, cell_size):
    return LrcPreprocessOpts(int(bool(remove_outliers)), int(nb_neighbors), float(std_ratio), int(bool(estimate_normals)),
                             int(max_nn), float(radius), float(cell_size))


def _points(points):
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be (n, 3)")
    return p


def preprocess_cloud(ctx, points, remove_outliers=True, nb_neighbors=20, std_ratio=2.0, estimate_normals=True,
                     radius=0.1, max_nn=30, cell_size=0.0):
    """Host (n, 3) points (converted to float64).  Returns a Preprocessed record."""
    p = _points(points)
    n = len(p)
    o = _opts(remove_outliers, nb_neighbors, std_ratio, estimate_normals, radius, max_nn, cell_size)
    kept = np.empty(n, dtype=np.uint32)
    normals = np.empty((n, 3), dtype=np.float64) if estimate_normals else None
    avg = np.empty(n, dtype=np.float64)
    nn = np.empty(n, dtype=np.uint8) if estimate_normals else None
    stats = np.empty(2, dtype=np.float64)
    m = C.c_uint64(0)
    check(_capi.load().lrc_cloud_preprocess(
        ctx._h, p.ctypes.data if n else None, n, C.byref(o), kept.ctypes.data if n else None, C.byref(m),
        None if normals is None or not n else normals.ctypes.data, avg.ctypes.data if n else None,
        None if nn is None or not n else nn.ctypes.data, stats.ctypes.data), "lrc_cloud_preprocess")
    k = m.value
    return Preprocessed(kept[:k].copy(), None if normals is None else normals[:k].copy(), avg,
                        None if nn is None else nn[:k].copy(), float(stats[0]), float(stats[1]))


def preprocess_cloud_dev(ctx, points_t, remove_outliers=True, nb_neighbors=20, std_ratio=2.0, estimate_normals=True,
                         radius=0.1, max_nn=30, cell_size=0.0, stream=0):
    """points_t: contiguous (n, 3) float64 device tensor.  Returns a Preprocessed record of device tensors (kept int32
    view of the uint32 indices, normals, avg, nn_count), sliced to the kept count; the call returns once `stream` has
    run its work."""
    import torch
    if points_t.dim() != 2 or points_t.shape[1] != 3 or points_t.dtype != torch.float64 or not points_t.is_contiguous():
        raise ValueError("points must be a contiguous (n, 3) float64 tensor")
    n = points_t.shape[0]
    dev = points_t.device
    o = _opts(remove_outliers, nb_neighbors, std_ratio, estimate_normals, radius, max_nn, cell_size)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float64, device=dev) if estimate_normals else None
    avg = torch.empty(n, dtype=torch.float64, device=dev)
    nn = torch.empty(n, dtype=torch.uint8, device=dev) if estimate_normals else None
    stats = np.empty(2, dtype=np.float64)
    m = C.c_uint64(0)

    def ptr(t):
        return None if t is None or not n else C.c_void_p(t.data_ptr())
    check(_capi.load().lrc_cloud_preprocess_dev(
        ctx._h, ptr(points_t), n, C.byref(o), ptr(kept), C.byref(m), ptr(normals), ptr(avg), ptr(nn), stats.ctypes.data,
        C.c_void_p(int(stream))), "lrc_cloud_preprocess_dev")
    k = m.value
    return Preprocessed(kept[:k], None if normals is None else normals[:k], avg, None if nn is None else nn[:k],
                        float(stats[0]), float(stats[1]))


def remove_statistical_outlier(ctx, points, nb_neighbors=20, std_ratio=2.0, cell_size=0.0):
    """Open3D's ``ind``: the inlier row indices in ascending order (int64)."""
    r = preprocess_cloud(ctx, points, remove_outliers=True, nb_neighbors=nb_neighbors, std_ratio=std_ratio,
                         estimate_normals=False, cell_size=cell_size)
    return r.kept.astype(np.int64)


def estimate_normals(ctx, points, radius=0.1, max_nn=30, cell_size=0.0):
    """(n, 3) float64 normals of every row (hybrid radius / max_nn search; see the module docstring)."""
    r = preprocess_cloud(ctx, points, remove_outliers=False, estimate_normals=True, radius=radius, max_nn=max_nn,
                         cell_size=cell_size)
    return r.normals
