"""Per-frame object annotations of scans over the C ABI (lrc_frameobj_*, csrc/lrc_frameobj.hip).

Object k is the k-th distinct label word ``key = sem | ins << 16`` among the mesh's triangles, ascending.  For every
(frame, object) the device keeps, in the SENSOR's frame of that frame's pose: ``returns`` (returned rays on the object),
``seen_tris`` / ``seen_q`` (triangles with a return, and their quantised area, each triangle once per frame) and
``vmin`` / ``vmax`` (the box of the returns; +inf / -inf without any).  The static table holds every object's triangle
count, quantised area ``total_q`` (q = rint(area * 2^32), as in lidarcast.coverage) and world AABB.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import LrcFrameobjInfo, check

Q_SCALE = 2.0 ** -32          # m^2 per unit of quantised area
MAX_OBJECTS = 4096


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _yaw_poses(poses):
    """(P, 4, 4) float64 poses whose rotation is about z, or ValueError."""
    M = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    R = M[:, :3, :3]
    if not ((R[:, 2, 2] == 1.0).all() and (R[:, 0, 2] == 0.0).all() and (R[:, 1, 2] == 0.0).all()
            and (R[:, 2, 0] == 0.0).all() and (R[:, 2, 1] == 0.0).all()):
        raise ValueError("boxes7 needs poses whose rotation is about z (R[2][2] == 1, the other off-axis entries 0)")
    return M


@dataclass
class FrameObjectsResult:
    """The static object table (K rows) and the per-(frame, object) arrays (F, K[, 3])."""
    key: np.ndarray                # (K,) uint32  sem | ins << 16, ascending
    tri_count: np.ndarray          # (K,) uint32
    total_q: np.ndarray            # (K,) uint64
    wmin: np.ndarray               # (K, 3) float64 world AABB of the object's triangles
    wmax: np.ndarray
    returns: np.ndarray            # (F, K) uint32
    seen_tris: np.ndarray          # (F, K) uint32
    seen_q: np.ndarray             # (F, K) uint64
    vmin: np.ndarray               # (F, K, 3) float64 sensor frame; +inf where returns == 0
    vmax: np.ndarray               # (F, K, 3) float64 sensor frame; -inf where returns == 0
    rejected_rays: int = 0

    @property
    def sem(self):
        return (self.key & 0xFFFF).astype(np.uint16)

    @property
    def ins(self):
        return (self.key >> 16).astype(np.uint16)

    @property
    def num_frames(self):
        return int(self.returns.shape[0])

    @property
    def num_objects(self):
        return int(self.key.shape[0])

    @property
    def total_area(self):
        """(K,) float64 m^2."""
        return self.total_q.astype(np.float64) * Q_SCALE

    @property
    def seen_ratio(self):
        """(F, K) float64 seen_q / total_q, 0 where total_q == 0."""
        tq = self.total_q.astype(np.float64)[None, :]
        out = np.zeros(self.seen_q.shape, dtype=np.float64)
        np.divide(self.seen_q.astype(np.float64), tq, out=out, where=tq != 0)
        return out

    def boxes7(self, poses):
        """(F, K, 7) float64 amodal boxes (cx, cy, cz, dx, dy, dz, heading) of every object in every frame's sensor
        frame: centre R^T ((wmin + wmax) / 2 - c) in the expression order of the kernel's s, size wmax - wmin, heading
        -atan2(R[1][0], R[0][0]).  ``poses``: (F, 4, 4) whose rotation is about z; anything else raises ValueError."""
        M = _yaw_poses(poses)
        if M.shape[0] != self.num_frames:
            raise ValueError("need one pose per frame")
        R, c = M[:, :3, :3], M[:, :3, 3]
        mid = (self.wmin + self.wmax) / 2
        e = mid[None, :, :] - c[:, None, :]                                   # (F, K, 3)
        out = np.empty((M.shape[0], self.num_objects, 7), dtype=np.float64)
        for a in range(3):
            out[:, :, a] = (R[:, None, 0, a] * e[:, :, 0] + R[:, None, 1, a] * e[:, :, 1]) + R[:, None, 2, a] * e[:, :, 2]
        out[:, :, 3:6] = (self.wmax - self.wmin)[None, :, :]
        out[:, :, 6] = (-np.arctan2(R[:, 1, 0], R[:, 0, 0]))[:, None]
        return out


class FrameObjects:
    """The static object table of one mesh and ``num_frames`` rows of per-object accumulators, in HBM."""

    def __init__(self, ctx, vertices, triangles, sem=None, ins=None, num_frames=1):
        self._lib = _capi.load()
        self.ctx = ctx
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        f = np.ascontiguousarray(triangles, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("vertices and triangles must be (V, 3) and (T, 3)")
        lab = []
        for name, a in (("sem", sem), ("ins", ins)):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.uint16)
            if a is not None and a.shape != (f.shape[0],):
                raise ValueError(f"{name} must have shape (T,)")
            lab.append(a)
        h = C.c_void_p()
        check(self._lib.lrc_frameobj_create(ctx._h, _ptr(v), v.shape[0], _ptr(f), f.shape[0], _ptr(lab[0]), _ptr(lab[1]),
                                            int(num_frames), C.byref(h)), "lrc_frameobj_create")
        self._h = h
        i = self.info()
        self.num_triangles, self.num_frames = int(i.num_triangles), int(i.num_frames)
        self.num_objects, self.words_per_frame = int(i.num_objects), int(i.words_per_frame)

    def info(self):
        i = LrcFrameobjInfo()
        check(self._lib.lrc_frameobj_get_info(self._h, C.byref(i)), "lrc_frameobj_get_info")
        return i

    @property
    def rejected_rays(self):
        return int(self.info().rejected_rays)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.lrc_frameobj_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=0):
        check(self._lib.lrc_frameobj_reset(self._h, C.c_void_p(int(stream))), "lrc_frameobj_reset")

    def accumulate_dev(self, t_t, prim_t, point3_t, poses, rays_per_pose, first_frame=0, stream=0):
        """t_t float32, prim_t int32 (or uint32 bits) and point3_t float32 (.., 3) device tensors of P x rays_per_pose
        rays, pose-major; ``poses``: (P, 4, 4) or (P, 16) float64, numpy or a device tensor.  Pose p goes to frame
        first_frame + p."""
        import torch
        if isinstance(poses, torch.Tensor):
            poses_t = poses
        else:
            poses_t = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)).to(t_t.device)
        if poses_t.dtype != torch.float64 or poses_t.numel() % 16 or not poses_t.is_contiguous():
            raise ValueError("poses must be contiguous (P, 16) float64")
        P, N = poses_t.numel() // 16, int(rays_per_pose)
        if int(first_frame) < 0:
            raise ValueError("first_frame must be >= 0")
        if t_t.numel() < P * N or prim_t.numel() < P * N or point3_t.numel() < 3 * P * N:
            raise ValueError("t_t, prim_t and point3_t need P * rays_per_pose rows")
        if t_t.element_size() != 4 or prim_t.element_size() != 4 or point3_t.dtype != torch.float32:
            raise ValueError("t_t and prim_t must hold 4-byte entries and point3_t float32")
        if not (t_t.is_contiguous() and prim_t.is_contiguous() and point3_t.is_contiguous()):
            raise ValueError("t_t, prim_t and point3_t must be contiguous")
        if P == 0 or N == 0:
            if int(first_frame) + P > self.num_frames:
                raise ValueError("first_frame + num_poses > num_frames")
            return
        check(self._lib.lrc_frameobj_accumulate_dev(self._h, C.c_void_p(poses_t.data_ptr()), P, N,
                                                    C.c_void_p(t_t.data_ptr()), C.c_void_p(prim_t.data_ptr()),
                                                    C.c_void_p(point3_t.data_ptr()), int(first_frame),
                                                    C.c_void_p(int(stream))), "lrc_frameobj_accumulate_dev")

    def objects(self):
        """(key (K,) uint32, tri_count (K,) uint32, total_q (K,) uint64, wmin (K, 3), wmax (K, 3) float64)."""
        K = self.num_objects
        key, cnt = np.zeros(K, np.uint32), np.zeros(K, np.uint32)
        tq = np.zeros(K, np.uint64)
        wmin, wmax = np.zeros((K, 3), np.float64), np.zeros((K, 3), np.float64)
        check(self._lib.lrc_frameobj_objects(self._h, _ptr(key), _ptr(cnt), _ptr(tq), _ptr(wmin), _ptr(wmax)),
              "lrc_frameobj_objects")
        return key, cnt, tq, wmin, wmax

    def export(self):
        """FrameObjectsResult of everything accumulated so far, after all enqueued work (the accumulation is kept).
        Two blocking calls: lrc_frameobj_export and, for rejected_rays, lrc_frameobj_get_info; each waits for the device."""
        F, K = self.num_frames, self.num_objects
        ret, tris = np.zeros((F, K), np.uint32), np.zeros((F, K), np.uint32)
        sq = np.zeros((F, K), np.uint64)
        vmin, vmax = np.zeros((F, K, 3), np.float64), np.zeros((F, K, 3), np.float64)
        check(self._lib.lrc_frameobj_export(self._h, _ptr(ret), _ptr(tris), _ptr(sq), _ptr(vmin), _ptr(vmax)),
              "lrc_frameobj_export")
        key, cnt, tq, wmin, wmax = self.objects()
        return FrameObjectsResult(key=key, tri_count=cnt, total_q=tq, wmin=wmin, wmax=wmax, returns=ret, seen_tris=tris,
                                  seen_q=sq, vmin=vmin, vmax=vmax, rejected_rays=self.rejected_rays)


def scan_frame_objects(scene, frames, poses, dirs, max_range, chunk_poses=None, stream=0):
    """Scan ``poses`` (P, 4, 4) with the sensor-frame direction table ``dirs`` (N, 3) float64 (numpy or a device tensor)
    on ``scene`` (lidarcast.Scene) and accumulate pose p into frame p of ``frames`` (FrameObjects).  The scan runs in
    chunks of ``chunk_poses`` poses through Scene.scan_poses_dev into one reused t / prim / point3 buffer (default:
    about 640 MB of records), so the buffers stay bounded however many poses there are.  Returns ``frames``."""
    import torch
    from .core import DeviceHits
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
    P = poses.shape[0]
    if P > frames.num_frames:
        raise ValueError("every pose is its own frame: need num_frames >= number of poses")
    dev = torch.device("cuda", scene.ctx.device)
    dirs_t = dirs if isinstance(dirs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.float64))
    dirs_t = dirs_t.to(dev, dtype=torch.float64).contiguous()
    if dirs_t.ndim != 2 or dirs_t.shape[1] != 3 or dirs_t.shape[0] == 0:
        raise ValueError("dirs must be a non-empty (N, 3) table")
    if P == 0:
        return frames
    N = int(dirs_t.shape[0])
    chunk = int(chunk_poses) if chunk_poses else max(1, (32 << 20) // N)
    chunk = max(1, min(chunk, P))
    hits = DeviceHits(chunk * N, dev, want=("t", "prim", "point3"))
    poses_t = torch.from_numpy(poses).to(dev)
    for p0 in range(0, P, chunk):
        p1 = min(P, p0 + chunk)
        scene.scan_poses_dev(poses_t[p0:p1], dirs_t, hits, max_range, stream=stream)
        frames.accumulate_dev(hits["t"], hits["prim"], hits["point3"], poses_t[p0:p1], N, first_frame=p0, stream=stream)
    torch.cuda.synchronize(dev)
    return frames
