"""Semantic occupancy grids from scans over the C ABI (lrc_voxgrid_*, csrc/lrc_voxgrid.hip).

Three states per voxel, the ground truth of semantic scene completion: OCCUPIED (a return ended in it), FREE (a ray
passed through it), UNKNOWN (no ray reached it).  Free space needs the poses and the per-ray ranges, so it is carved
at scan time.  Not to be confused with ``OccupancyIndex`` (the planner's robot-cube test).

Grid: origin g (3 float64), voxel size s > 0, dims (nx, ny, nz), nx*ny*nz <= 2^31 - 1; the voxel of x is
floor((x - g) / s) per axis (f64 subtract, divide, floor); arrays have shape (nx, ny, nz) in C order, z fastest.  A
returned ray (finite t) walks, in float64, every voxel from the voxel of its float32 origin to the voxel of its float32
hit point (the scene cloud's row), axis by axis in order of the next boundary crossing (ties x, y, z); every in-grid
voxel of the walk but the last gets the free bit, the last, if in the grid, one return with the ray's (sem, ins).
Finalize: occupied iff returns >= min_returns, else free iff the free bit is set, else unknown; sem = majority label of
the returns (ties to the smallest), ins = majority instance among the returns with that sem (ties to the smallest).
The full statement is in include/lidarcast.h and tests/voxgrid_restate.py.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict

import numpy as np

from . import _capi
from ._capi import LrcVoxgridInfo, check

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
MAX_VOXELS = (1 << 31) - 1


def check_grid(origin, voxel_size, dims):
    """Validated (origin (3,) float64, voxel_size float, dims (3,) int) or ValueError; touches no device."""
    o = np.asarray(origin, dtype=np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("origin must be 3 finite numbers")
    try:
        s = float(voxel_size)
    except (TypeError, ValueError):
        raise ValueError("voxel_size must be a number") from None
    if not np.isfinite(s) or s <= 0.0:
        raise ValueError("voxel_size must be finite and > 0")
    d = np.asarray(dims).reshape(-1)
    if d.shape != (3,) or d.dtype.kind not in "iuf" or not np.all(np.isfinite(d)) or not np.all(d == np.floor(d)):
        raise ValueError("dims must be 3 integers")
    d = [int(x) for x in d]
    if min(d) < 1:
        raise ValueError("every dim must be >= 1")
    if d[0] * d[1] * d[2] > MAX_VOXELS:
        raise ValueError("nx*ny*nz must not exceed 2^31 - 1")
    return o, s, tuple(d)


def default_extent(vertices, voxel_size):
    """Grid around a mesh with a one-voxel margin: origin = min(vertices) - s, dims = floor((max(vertices) - origin) / s)
    + 2 per axis.  floor((x - origin) / s) is monotone in x, so every vertex lands in voxels 0 .. dims - 2."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    if len(v) == 0:
        raise ValueError("the mesh has no vertices")
    s = float(voxel_size)
    if not np.isfinite(s) or s <= 0.0:
        raise ValueError("voxel_size must be finite and > 0")
    lo = np.array([v[:, 0].min(), v[:, 1].min(), v[:, 2].min()])
    hi = np.array([v[:, 0].max(), v[:, 1].max(), v[:, 2].max()])
    origin = lo - s
    dims = tuple(int(x) + 2 for x in np.floor((hi - origin) / s))
    return origin, dims


@dataclass
class OccupancyResult:
    origin: np.ndarray             # (3,) float64
    voxel_size: float
    dims: tuple
    min_returns: int
    idx: np.ndarray                # (K,) uint32, ascending: every voxel with >= 1 return
    sem: np.ndarray                # (K,) uint16
    ins: np.ndarray                # (K,) uint16
    returns: np.ndarray            # (K,) uint32
    num_free: int
    num_occupied: int
    num_unknown: int
    rejected_rays: int = 0
    state: np.ndarray = None       # (nx, ny, nz) uint8 0 unknown / 1 free / 2 occupied; None without dense
    per_class: Dict[int, int] = field(default_factory=dict)   # sem -> occupied voxels

    def _dense(self, values, dtype):
        out = np.zeros(int(np.prod(self.dims)), dtype=dtype)
        out[self.idx.astype(np.int64)] = values
        return out.reshape(self.dims)

    @property
    def dense_sem(self):
        return self._dense(self.sem, np.uint16)

    @property
    def dense_ins(self):
        return self._dense(self.ins, np.uint16)

    @property
    def dense_returns(self):
        return self._dense(self.returns, np.uint32)

    @property
    def occupied(self):
        """(K,) bool over the sparse list: returns >= min_returns."""
        return self.returns >= self.min_returns

    def coords(self, idx=None):
        """(K, 3) int64 voxel coordinates of linear indices (default: the sparse list)."""
        i = self.idx if idx is None else np.asarray(idx)
        return np.stack(np.unravel_index(i.astype(np.int64), self.dims), axis=1)

    def occupied_centres(self):
        """(M, 3) float64 centres g + (i + 0.5) * s of the occupied voxels, with their (sem, ins)."""
        m = self.occupied
        c = self.coords(self.idx[m]).astype(np.float64)
        return self.origin + (c + 0.5) * self.voxel_size, self.sem[m], self.ins[m]

    def counts(self):
        return {"free": self.num_free, "occupied": self.num_occupied, "unknown": self.num_unknown,
                "voxels_with_returns": int(len(self.idx)), "returns": int(self.returns.sum(dtype=np.uint64)),
                "rejected_rays": self.rejected_rays}

    def to_dict(self, class_names=None):
        """JSON-ready summary: grid, counts and per-class occupied voxels (``class_names``: sem -> name, where known)."""
        def name(s):
            return class_names[s] if class_names is not None and s in class_names else str(s)
        return {"origin": [float(x) for x in self.origin], "voxel_size": self.voxel_size,
                "dims": [int(x) for x in self.dims], "min_returns": self.min_returns, "counts": self.counts(),
                "per_class_occupied_voxels": {name(s): int(n) for s, n in self.per_class.items()}}

    def to_npz(self, path):
        """state, sem, ins, returns (dense, (nx, ny, nz)), origin, voxel_size, dims."""
        if self.state is None:
            raise ValueError("finalize(dense=True) is needed for the npz (it holds the dense state)")
        np.savez_compressed(path, state=self.state, sem=self.dense_sem, ins=self.dense_ins, returns=self.dense_returns,
                            origin=self.origin, voxel_size=np.float64(self.voxel_size),
                            dims=np.array(self.dims, dtype=np.int64))


class OccupancyGrid:
    """Free bits and returns of one voxel grid, in HBM, accumulated over scans until ``reset``."""

    def __init__(self, ctx, origin, voxel_size, dims):
        o, s, d = check_grid(origin, voxel_size, dims)
        self._lib = _capi.load()
        self.ctx = ctx
        h = C.c_void_p()
        dd = (C.c_int64 * 3)(*d)
        check(self._lib.lrc_voxgrid_create(ctx._h, o.ctypes.data_as(C.c_void_p), s, dd, C.byref(h)),
              "lrc_voxgrid_create")
        self._h = h
        self.origin, self.voxel_size, self.dims = o, s, d
        self.num_voxels = d[0] * d[1] * d[2]

    def info(self):
        i = LrcVoxgridInfo()
        check(self._lib.lrc_voxgrid_get_info(self._h, C.byref(i)), "lrc_voxgrid_get_info")
        return i

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.lrc_voxgrid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=0):
        check(self._lib.lrc_voxgrid_reset(self._h, C.c_void_p(int(stream))), "lrc_voxgrid_reset")

    def accumulate_dev(self, poses_t, dirs_t, t_label_t, stream=0):
        """poses_t (P, 16) or (P, 4, 4) float64, dirs_t (N, 3) float64 and t_label_t (P*N) x 8 B device tensors of a
        pose-batched scan (Scene.scan_poses_dev with DeviceHits(want=("t_label",)))."""
        import torch
        P, N = int(poses_t.shape[0]), int(dirs_t.shape[0])
        if poses_t.dtype != torch.float64 or dirs_t.dtype != torch.float64 or poses_t.numel() != P * 16 or \
                dirs_t.numel() != N * 3:
            raise ValueError("poses_t must be (P, 16) float64 and dirs_t (N, 3) float64")
        if not (poses_t.is_contiguous() and dirs_t.is_contiguous() and t_label_t.is_contiguous()):
            raise ValueError("poses_t, dirs_t and t_label_t must be contiguous")
        if t_label_t.numel() * t_label_t.element_size() < P * N * 8:
            raise ValueError("t_label_t needs 8 bytes per ray (P * N rays)")
        check(self._lib.lrc_voxgrid_accumulate_dev(self._h, C.c_void_p(poses_t.data_ptr()), P,
                                                   C.c_void_p(dirs_t.data_ptr()), N, C.c_void_p(t_label_t.data_ptr()),
                                                   C.c_void_p(int(stream))), "lrc_voxgrid_accumulate_dev")

    def free_bits(self):
        """(ceil(V/32),) uint32 free bitset after all enqueued work."""
        w = np.zeros(int(self.info().words), dtype=np.uint32)
        check(self._lib.lrc_voxgrid_export_bits(self._h, w.ctypes.data_as(C.c_void_p)), "lrc_voxgrid_export_bits")
        return w

    def finalize(self, min_returns=1, dense=True, stream=0):
        """OccupancyResult of everything accumulated so far (the accumulation itself is kept).  Runs on the device
        (lrc_voxgrid_finalize_dev) and synchronises once, on the counts."""
        import torch
        mr = int(min_returns)
        if mr < 1 or mr > 0xFFFFFFFF:
            raise ValueError("min_returns must be >= 1")
        dev = torch.device("cuda", self.ctx.device)
        bound = max(1, int(self.info().sparse_bound))
        idx = torch.empty(bound, dtype=torch.int32, device=dev)
        ret = torch.empty(bound, dtype=torch.int32, device=dev)
        sem = torch.empty(bound, dtype=torch.int16, device=dev)
        ins = torch.empty(bound, dtype=torch.int16, device=dev)
        state = torch.empty(self.num_voxels, dtype=torch.uint8, device=dev) if dense else None
        counts = torch.zeros(6, dtype=torch.int64, device=dev)
        check(self._lib.lrc_voxgrid_finalize_dev(
            self._h, mr, C.c_void_p(idx.data_ptr()), C.c_void_p(sem.data_ptr()), C.c_void_p(ins.data_ptr()),
            C.c_void_p(ret.data_ptr()), bound, None if state is None else C.c_void_p(state.data_ptr()),
            C.c_void_p(counts.data_ptr()), C.c_void_p(int(stream))), "lrc_voxgrid_finalize_dev")
        c = counts.cpu().numpy().astype(np.uint64)          # the one synchronisation
        k = int(c[0])
        r = OccupancyResult(origin=self.origin.copy(), voxel_size=self.voxel_size, dims=self.dims, min_returns=mr,
                            idx=idx[:k].cpu().numpy().view(np.uint32), sem=sem[:k].cpu().numpy().view(np.uint16),
                            ins=ins[:k].cpu().numpy().view(np.uint16), returns=ret[:k].cpu().numpy().view(np.uint32),
                            num_free=int(c[1]), num_occupied=int(c[2]), num_unknown=int(c[3]), rejected_rays=int(c[4]),
                            state=None if state is None else state.cpu().numpy().reshape(self.dims))
        occ = r.occupied
        if occ.any():
            u, n = np.unique(r.sem[occ], return_counts=True)
            r.per_class = {int(a): int(b) for a, b in zip(u, n)}
        return r


def scan_occupancy(scene, grid, poses, dirs, max_range, chunk_poses=None, stream=0):
    """Scan ``poses`` (P, 4, 4) with the sensor-frame direction table ``dirs`` (N, 3) float64 (numpy or a device tensor)
    on ``scene`` (lidarcast.Scene, built with its triangle labels) and accumulate every returned ray into ``grid``
    (OccupancyGrid).  The scan runs in chunks of ``chunk_poses`` poses through Scene.scan_poses_dev into one reused
    t_label buffer (default: about 256 MB of pairs), so the buffers stay bounded however many poses there are.
    Returns ``grid``."""
    import torch
    from .core import DeviceHits
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
    P = poses.shape[0]
    dev = torch.device("cuda", scene.ctx.device)
    dirs_t = dirs if isinstance(dirs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64))
    dirs_t = dirs_t.to(dev, dtype=torch.float64).contiguous()
    if dirs_t.ndim != 2 or dirs_t.shape[1] != 3 or dirs_t.shape[0] == 0:
        raise ValueError("dirs must be a non-empty (N, 3) table")
    if P == 0:
        return grid
    N = int(dirs_t.shape[0])
    chunk = int(chunk_poses) if chunk_poses else max(1, (32 << 20) // N)
    chunk = max(1, min(chunk, P))
    hits = DeviceHits(chunk * N, dev, want=("t_label",))
    poses_t = torch.from_numpy(poses).to(dev)
    for p0 in range(0, P, chunk):
        p1 = min(P, p0 + chunk)
        scene.scan_poses_dev(poses_t[p0:p1], dirs_t, hits, max_range, stream=stream)
        grid.accumulate_dev(poses_t[p0:p1], dirs_t, hits["t_label"], stream=stream)
    torch.cuda.synchronize(dev)
    return grid
