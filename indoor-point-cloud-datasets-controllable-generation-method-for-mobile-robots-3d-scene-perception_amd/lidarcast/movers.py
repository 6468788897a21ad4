"""Moving objects: rigid movers traced per frame (include/lidarcast.h "moving objects").

``MoverSet`` holds 1 to 255 rigid meshes, each modelled around its own origin, as scenes of one context; ``MoverTrack`` turns
a timed path into the (12,) float32 object-to-world poses the scan takes.  ``Scene.scan_movers_dev`` /
``Scene.scan_movers_compact`` trace the static scene once and every mover in its own frame, and keep the nearest;
``rays`` and ``merge`` are the two host steps of that, without a GPU (lrc_mover_rays, lrc_mover_merge).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check

MAX_MOVERS = 255


class MoverSet:
    """meshes: 1 to 255 triangle meshes (``vertices``, ``triangles`` and optionally ``triangle_sem`` / ``triangle_ins``, as
    ``lidarcast.synth.TriangleMesh``), each around its own origin.  Builds and owns one ``Scene`` per mesh on ``ctx`` and the
    set's handle; ``boxes`` holds every mesh's own (lo, hi) float64 box."""

    def __init__(self, ctx, meshes):
        from .core import Scene
        meshes = list(meshes)
        if not 1 <= len(meshes) <= MAX_MOVERS:
            raise ValueError("a mover set has 1 to 255 movers")
        self._lib = _capi.load()
        self.ctx = ctx
        self.scenes = []
        self.boxes = []
        self._h = None
        try:
            for m in meshes:
                v = np.asarray(m.vertices, dtype=np.float64)
                self.scenes.append(Scene(ctx, v, m.triangles, getattr(m, "triangle_sem", None), getattr(m, "triangle_ins", None)))
                self.boxes.append((v.min(0), v.max(0)) if len(v) else (np.zeros(3), np.zeros(3)))
            arr = (C.c_void_p * len(self.scenes))(*[s._h for s in self.scenes])
            h = C.c_void_p()
            check(self._lib.lrc_movers_create(ctx._h, arr, len(self.scenes), C.byref(h)), "lrc_movers_create")
            self._h = h
        except Exception:
            self.close()
            raise

    def __len__(self):
        return len(self.scenes)

    def handle(self, ctx):
        """The set's handle for a scan on ``ctx``."""
        if not self._h:
            raise ValueError("mover set is closed")
        if ctx is not self.ctx:
            raise ValueError("mover set belongs to another context (device)")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.lrc_movers_destroy(self._h)
            self._h = None
        for s in getattr(self, "scenes", []):
            s.close()
        self.scenes = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MoverTrack:
    """path: [[t, x, y, z, yaw_deg], ...] with increasing t.  The position is piecewise linear in time and held at both ends;
    the yaw is interpolated along the shorter arc between two knots.  ``poses12(times)`` gives the (len(times), 12) float32
    row-major [R | c] object-to-world poses (a rotation about z), computed in float64 and narrowed last."""

    def __init__(self, path):
        p = np.array(path, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 5 or len(p) < 1:
            raise ValueError("a mover path is a list of [t, x, y, z, yaw_deg] rows")
        if not np.isfinite(p).all():
            raise ValueError("a mover path must be finite")
        if (np.diff(p[:, 0]) <= 0).any():
            raise ValueError("the times of a mover path must increase")
        self.path = p

    def state(self, times):
        """(x, y, z, yaw in radians) float64 at ``times``: (n, 4)."""
        t = np.atleast_1d(np.asarray(times, dtype=np.float64))
        p = self.path
        out = np.empty((len(t), 4))
        if len(p) == 1:
            out[:, :3] = p[0, 1:4]
            out[:, 3] = np.deg2rad(p[0, 4])
            return out
        tc = np.clip(t, p[0, 0], p[-1, 0])
        k = np.clip(np.searchsorted(p[:, 0], tc, side="right") - 1, 0, len(p) - 2)
        u = (tc - p[k, 0]) / (p[k + 1, 0] - p[k, 0])
        out[:, :3] = p[k, 1:4] + u[:, None] * (p[k + 1, 1:4] - p[k, 1:4])
        dyaw = (p[k + 1, 4] - p[k, 4] + 180.0) % 360.0 - 180.0          # the shorter arc, in [-180, 180)
        out[:, 3] = np.deg2rad(p[k, 4] + u * dyaw)
        return out

    def poses12(self, times):
        return pose12(self.state(times))


def pose12(state):
    """(n, 4) float64 (x, y, z, yaw) -> (n, 12) float32 row-major [Rz(yaw) | c]: float64 arithmetic, narrowed last."""
    s = np.asarray(state, dtype=np.float64).reshape(-1, 4)
    m = np.zeros((len(s), 3, 4))
    c, sn = np.cos(s[:, 3]), np.sin(s[:, 3])
    m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1], m[:, 2, 2] = c, -sn, sn, c, 1.0
    m[:, :, 3] = s[:, :3]
    return m.reshape(-1, 12).astype(np.float32)


def pose12_from_matrix(mat):
    """(..., 4, 4) or (..., 3, 4) float64 object-to-world matrices -> (..., 12) float32."""
    m = np.asarray(mat, dtype=np.float64)
    return np.ascontiguousarray(m[..., :3, :4]).reshape(m.shape[:-2] + (12,)).astype(np.float32)


def rays(rays6, pose12_):
    """lrc_mover_rays: the (n, 6) float32 world rays in the frame of ONE mover pose (12,) float32; no GPU."""
    lib = _capi.load()
    r = np.ascontiguousarray(rays6, dtype=np.float32).reshape(-1, 6)
    p = np.ascontiguousarray(pose12_, dtype=np.float32).reshape(12)
    out = np.empty_like(r)
    check(lib.lrc_mover_rays(r.ctypes.data, len(r), p.ctypes.data, out.ctypes.data), "lrc_mover_rays")
    return out


def merge(t_static, normal3_static, t_movers, normal3_movers, poses12):
    """lrc_mover_merge for ONE frame: (n,) ranges and (n, 3) normals of the static cast, (M, n) ranges and (M, n, 3) normals of
    the mover casts, (M, 12) mover poses; no GPU.  Returns the winner's (t, normal3, mover): mover 0 is the static scene,
    m + 1 mover m."""
    lib = _capi.load()
    ts = np.ascontiguousarray(t_static, dtype=np.float32).reshape(-1)
    n = len(ts)
    ns = np.ascontiguousarray(normal3_static, dtype=np.float32).reshape(n, 3)
    tm = np.ascontiguousarray(t_movers, dtype=np.float32).reshape(-1, n) if n else np.zeros((len(poses12), 0), np.float32)
    M = tm.shape[0]
    nm = np.ascontiguousarray(normal3_movers, dtype=np.float32).reshape(M, n, 3)
    p = np.ascontiguousarray(poses12, dtype=np.float32).reshape(M, 12)
    out_t = np.empty(n, np.float32)
    out_n = np.empty((n, 3), np.float32)
    out_m = np.empty(n, np.uint8)
    check(lib.lrc_mover_merge(n, M, ts.ctypes.data, ns.ctypes.data, tm.ctypes.data, nm.ctypes.data, p.ctypes.data,
                              out_t.ctypes.data, out_n.ctypes.data, out_m.ctypes.data), "lrc_mover_merge")
    return out_t, out_n, out_m
