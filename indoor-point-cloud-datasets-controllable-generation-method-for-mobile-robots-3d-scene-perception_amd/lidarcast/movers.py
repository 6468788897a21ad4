"""Moving objects: rigid movers traced per frame (include/lidarcast.h "moving objects").

``MoverSet`` holds 1 to 255 rigid meshes, each modelled around its own origin, as scenes of one context; ``MoverTrack`` turns
a timed path into the (12,) float32 object-to-world poses the scan takes.  ``Scene.scan_movers_dev`` /
``Scene.scan_movers_compact`` trace the static scene once and every mover in its own frame, and keep the nearest;
``rays`` and ``merge`` are the two host steps of that, without a GPU (lrc_mover_rays, lrc_mover_merge).

Movers under moving-sensor sweeps are this module's own, as the noisy sweeps are ``lidarcast.noise``'s:
``sweep_records`` makes the (P, M, 24) mover sweep records from tracks, ``sweep_rays`` / ``sweep_normals`` are the host steps,
``scan_mover_sweeps_dev``, ``scan_mover_sweeps_compact`` and ``scan_mover_sweep_frames`` the scans -- module functions that take
the scene or the engine as their first argument.

Seeded sensor noise under movers is at the end: ``scan_noisy_movers_dev``, ``scan_noisy_movers_compact``
and ``scan_noisy_mover_frames``, module functions as well, bound as ``Scene`` and engine methods of the same names.  The same
noise under movers in sweeps follows: ``scan_noisy_mover_sweeps_dev``, ``scan_noisy_mover_sweeps_compact``
and ``scan_noisy_mover_sweep_frames``.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check

MAX_MOVERS = 255


class MoverSet:
    """meshes: 1 to 255 triangle meshes (``vertices``, ``triangles`` and optionally ``triangle_sem`` / ``triangle_ins``, as
    ``lidarcast.synth.TriangleMesh``), each around its own origin.  Builds and owns one ``Scene`` per mesh on ``ctx`` and the
    set's handle; ``boxes`` holds every mesh's own (lo, hi) float64 box.  A ``lidarcast.deform.Deformable`` among the meshes
    brings its own scene, which the set uses without owning it (close the set before the deformable); its box is that of
    all its keyframes."""

    def __init__(self, ctx, meshes):
        from .core import Scene
        from .deform import Deformable
        meshes = list(meshes)
        if not 1 <= len(meshes) <= MAX_MOVERS:
            raise ValueError("a mover set has 1 to 255 movers")
        self._lib = _capi.load()
        self.ctx = ctx
        self.scenes = []
        self.boxes = []
        self.deformables = []       # the ``lidarcast.deform.Deformable`` members, in the set's order
        self._owned = []
        self._h = None
        try:
            for m in meshes:
                if isinstance(m, Deformable):       # its own scene, not owned here; the box of all its keyframes
                    if m.ctx is not ctx:
                        raise ValueError("a deformable of a mover set must belong to the set's context")
                    inf = m.scene.info
                    self.scenes.append(m.scene)
                    self.deformables.append(m)
                    self.boxes.append((np.array(inf["bounds_lo"], np.float64), np.array(inf["bounds_hi"], np.float64)))
                    continue
                v = np.asarray(m.vertices, dtype=np.float64)
                self.scenes.append(Scene(ctx, v, m.triangles, getattr(m, "triangle_sem", None), getattr(m, "triangle_ins", None)))
                self._owned.append(self.scenes[-1])
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
        for s in getattr(self, "_owned", []):
            s.close()
        self.scenes, self._owned, self.deformables = [], [], []

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


# ---- movers under moving-sensor sweeps (include/lidarcast.h "movers under moving-sensor sweeps") -----
# Every ray of a sweep meets each mover at the pose the mover has when the ray fires.  Module functions, as
# lidarcast.noise.sweep_rays / scan_noisy_sweeps_* are: the scene and the engine are arguments.

def sweep_records(tracks, t_start, t_end):
    """(P, M, 24) float32 mover sweep records of M ``MoverTrack``s over P sweeps that start at ``t_start`` (P,) and end at
    ``t_end`` (P,) seconds: the start pose12, dq = (cos(a/2), 0, 0, sin(a/2)) of the yaw step a from start to end along the
    shorter arc, dc = c_end - c_start; float64 arithmetic, narrowed last.  Each track is evaluated at the two times and nothing
    else: the record moves straight between the two poses, so a path knot inside a sweep is cut straight.  A mover that does not
    move during a sweep gets the still record (dq = (1, 0, 0, 0), dc = 0) exactly.  Raises ValueError for a yaw step above
    pi/2 within one sweep."""
    t0 = np.atleast_1d(np.asarray(t_start, dtype=np.float64))
    t1 = np.atleast_1d(np.asarray(t_end, dtype=np.float64))
    if t0.shape != t1.shape or t0.ndim != 1:
        raise ValueError("t_start and t_end must be (P,)")
    tracks = list(tracks)
    out = np.zeros((len(t0), len(tracks), 24), np.float32)
    for m, tr in enumerate(tracks):
        a, b = tr.state(t0), tr.state(t1)
        dyaw = (b[:, 3] - a[:, 3] + np.pi) % (2.0 * np.pi) - np.pi          # the shorter arc, in [-pi, pi)
        if (np.abs(dyaw) > np.pi / 2).any():
            k = int(np.argmax(np.abs(dyaw)))
            raise ValueError(f"mover {m} turns by {abs(dyaw[k]):.3f} rad in sweep {k}: at most pi/2 per sweep")
        out[:, m, :12] = pose12(a)
        out[:, m, 12] = np.cos(0.5 * dyaw)
        out[:, m, 15] = np.sin(0.5 * dyaw)
        out[:, m, 16:19] = b[:, :3] - a[:, :3]
    return out


def _per_ray(rays, width, fire_of_ray, record24):
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, width)
    f = np.ascontiguousarray(fire_of_ray, dtype=np.float64).reshape(-1)
    if len(f) != len(r):
        raise ValueError("fire_of_ray must hold one firing fraction per row")
    return r, f, np.ascontiguousarray(record24, dtype=np.float32).reshape(24)


def sweep_rays(rays6, fire_of_ray, record24):
    """lrc_mover_sweep_rays: the (n, 6) float32 world rays, ray i in the frame the mover of ONE sweep record (24,) float32 has at
    ``fire_of_ray[i]`` (float64, narrowed to float32 as the kernel narrows it); no GPU."""
    lib = _capi.load()
    r, f, rec = _per_ray(rays6, 6, fire_of_ray, record24)
    out = np.empty_like(r)
    check(lib.lrc_mover_sweep_rays(r.ctypes.data, f.ctypes.data, len(r), rec.ctypes.data, out.ctypes.data), "lrc_mover_sweep_rays")
    return out


def sweep_normals(normal3, fire_of_ray, record24):
    """lrc_mover_sweep_normals: the (n, 3) float32 normals of ONE mover's cast turned into the world, normal i by the pose the
    mover of the record has at ``fire_of_ray[i]``; no GPU.  ``merge`` then serves unchanged: it picks the winner, and the
    winner's normal is the row of this array."""
    lib = _capi.load()
    q, f, rec = _per_ray(normal3, 3, fire_of_ray, record24)
    out = np.empty_like(q)
    check(lib.lrc_mover_sweep_normals(q.ctypes.data, f.ctypes.data, len(q), rec.ctypes.data, out.ctypes.data),
          "lrc_mover_sweep_normals")
    return out


def _scan_name(sweep, noisy, tail):
    return "lrc_scan_" + ("noisy_" if noisy else "") + ("mover_sweeps_" if sweep else "movers_") + tail


def _scan_movers_dev(scene, sweep, noisy, sensor_t, dirs_t, fire_t, hits, max_range, movers, side_t, noise, mover_t, stream):
    """The four ``*_dev`` scans of the mover family.  ``sweep``: sensor_t holds (P, 24) motion records, fire_t the firing
    fractions and side_t the (P, M, 24) mover sweep records, else (P, 16) poses and (P, M, 12) mover poses.  ``noisy``: the call
    brings ``noise``."""
    import torch
    from .core import _check_side_tensor, _dptr, _stream
    name, width = ("mover_records_t", 24) if sweep else ("mover_poses_t", 12)
    P, N = sensor_t.shape[0], dirs_t.shape[0]
    if sweep and (sensor_t.numel() != P * 24 or fire_t.numel() != N):
        raise ValueError("motion_t must be (P, 24) and fire_t (N,)")
    if hits.n != P * N:
        raise ValueError("hits must hold P * N records")
    handle, entries = None, None
    if movers is not None:
        handle, entries = movers.handle(scene.ctx), P * len(movers) * width
        if side_t is None:
            raise ValueError(f"{name} must be (P, M, {width})")
    _check_side_tensor(name, side_t, torch.float32, entries, f"be (P, M, {width})", sensor_t)
    _check_side_tensor("mover_t", mover_t, torch.uint8, P * N, "hold P * N entries", sensor_t)
    nz = [noise.struct()] if noisy else []
    fn = _scan_name(sweep, noisy, "dev")
    check(getattr(scene._lib, fn)(scene._h, handle, _dptr(sensor_t), P, _dptr(dirs_t), *([_dptr(fire_t)] if sweep else []), N,
                                  _dptr(side_t), float(max_range), *[C.byref(z) for z in nz], C.byref(hits.struct), _dptr(mover_t),
                                  _stream(stream)), fn)


def _scan_movers_compact(scene, sweep, noisy, sensor, dirs, fire, max_range, movers, side, noise, want, capacity):
    """The four ``*_compact`` scans of the mover family, by the same two switches; ``side`` is mover_records under ``sweep``,
    else mover_poses.  Under ``sweep`` the table brings the firing fractions, or takes ``fire``."""
    from .core import DirectionTable, _ptr, _table_for
    name, width = ("mover_records", 24) if sweep else ("mover_poses", 12)
    sensor = np.ascontiguousarray(sensor, dtype=np.float64).reshape(-1, 24 if sweep else 16)
    h, P, reach = scene._h, sensor.shape[0], float(max_range)
    if sweep and fire is None and not isinstance(dirs, DirectionTable):
        raise ValueError("fire is required with a plain direction table")
    with _table_for(scene.ctx, dirs, fire) as tab:
        if sweep:
            if tab is dirs and fire is not None and \
                    (tab.fire is None or not np.array_equal(tab.fire, np.asarray(fire, np.float64).reshape(-1))):
                tab.set_fire(fire)
            if tab.fire is None:
                raise ValueError("the direction table has no firing fractions")
        handle, rec = None, None
        if movers is not None:
            handle = movers.handle(scene.ctx)
            rec = np.ascontiguousarray(side, dtype=np.float32)
            if rec.shape != (P, len(movers), width):
                raise ValueError(f"{name} must be (P, M, {width}) = ({P}, {len(movers)}, {width}), got {rec.shape}")
        nz = [noise.struct()] if noisy else []
        fn = _scan_name(sweep, noisy, "compact")
        return scene._scan_frames(fn, P, tab.n, want, capacity, lambda fr, cap, total, rows:
                                  getattr(scene._lib, fn)(h, handle, _ptr(sensor), P, tab._h, _ptr(rec), reach,
                                                          *[C.byref(z) for z in nz], fr, rows, cap, total),
                                  side=[("mover", np.uint8, ())])


def _sweep_frames(engine, noisy, intrinsics, start_poses, end_poses, mesh, movers, mover_records, noise, want, inputs, need):
    """The two ``*_sweep_frames`` scans: the sweep's inputs, the compact scan with the index column, and ``point_times``."""
    motion, fire, T = inputs if inputs is not None else engine.sweep_inputs(intrinsics, start_poses, end_poses)
    engine._need_table(intrinsics, need, NotImplementedError)
    ask = tuple(want) + (() if "index" in want else ("index",))
    fr = _scan_movers_compact(engine.scene_for(mesh), True, noisy, motion, engine._resident_table(intrinsics), fire,
                              intrinsics.max_range, movers, mover_records, noise, ask, None)
    fr["point_times"] = fire[fr["index"]] * T
    if "index" not in want:
        del fr["index"]
    return fr


def scan_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, max_range, movers, mover_records_t, mover_t=None, stream=0):
    """Moving-sensor sweeps with moving objects on device tensors (lrc_scan_mover_sweeps_dev): motion_t (P, 24) float64, dirs_t
    (N, 3) float64, fire_t (N,) float64 as ``Scene.scan_sweeps_dev`` takes them; ``movers`` a MoverSet or None,
    ``mover_records_t`` (P, M, 24) float32 (``sweep_records``; the caller vouches for them), ``mover_t`` an optional (P * N)
    uint8 tensor: 0 for the static scene, m + 1 for mover m.  Records as ``Scene.scan_poses_dev``."""
    _scan_movers_dev(scene, True, False, motion_t, dirs_t, fire_t, hits, max_range, movers, mover_records_t, None, mover_t, stream)


def scan_mover_sweeps_compact(scene, motion, dirs, fire, max_range, movers, mover_records, want=("point3", "sem", "ins"),
                              capacity=None):
    """Moving-sensor sweeps with moving objects straight to frames (lrc_scan_mover_sweeps_compact): ``motion``, ``dirs`` and
    ``fire`` as ``Scene.scan_sweeps_compact`` takes them, ``movers`` a MoverSet or None, ``mover_records`` (P, M, 24) float32.
    The return value of ``Scene.scan_movers_compact``: the frames plus ``mover``, one uint8 per kept row."""
    return _scan_movers_compact(scene, True, False, motion, dirs, fire, max_range, movers, mover_records, None, want, capacity)


def scan_mover_sweep_frames(engine, intrinsics, start_poses, end_poses, mesh, movers, mover_records, want=("point3", "sem", "ins"),
                            inputs=None):
    """``RaycastEngineHIP.scan_sweep_frames`` with moving objects that move while the sweep is scanned: sweep k moves from
    start_poses[k] to end_poses[k], and every ray meets mover m at the pose ``mover_records[k, m]`` gives for the moment the ray
    fires.  The dict of ``scan_sweep_frames`` (``point_times`` included) plus ``mover``, one uint8 per kept row: 0 for the static
    mesh, m + 1 for mover m.  ``inputs``: a ``sweep_inputs`` triple to scan exactly those sensor records again."""
    return _sweep_frames(engine, False, intrinsics, start_poses, end_poses, mesh, movers, mover_records, None, want, inputs,
                         "movers under moving-sensor sweeps need a sensor with a pose-independent direction table")


# ---- seeded sensor noise under movers (include/lidarcast.h "seeded sensor noise under movers") --------------
# Module functions with the scene and the engine as arguments, as the scans above are; they are also bound below as
# ``Scene.scan_noisy_movers_dev`` and ``Scene.scan_noisy_movers_compact``, and by ``raycast_engine`` as
# ``RaycastEngineHIP.scan_noisy_mover_frames``.

def scan_noisy_movers_dev(scene, poses_t, dirs_t, hits, max_range, movers, mover_poses_t, noise, mover_t=None, stream=0):
    """``Scene.scan_movers_dev`` with seeded sensor noise drawn in the mover kernels (lrc_scan_noisy_movers_dev): ``noise`` a
    ``lidarcast.noise.NoiseModel`` (pose p of the call is frame ``noise.first_frame + p``); everything else as there.  The
    all-zero model gives ``scan_movers_dev``'s bytes, ``movers=None`` those of ``Scene.scan_noisy_dev`` and a zero column."""
    _scan_movers_dev(scene, False, True, poses_t, dirs_t, None, hits, max_range, movers, mover_poses_t, noise, mover_t, stream)


def scan_noisy_movers_compact(scene, poses, dirs, max_range, movers, mover_poses, noise, want=("point3", "sem", "ins"),
                              capacity=None):
    """``Scene.scan_movers_compact`` with seeded sensor noise drawn in the mover kernels (lrc_scan_noisy_movers_compact):
    ``noise`` a ``lidarcast.noise.NoiseModel`` (pose p of the call is frame ``noise.first_frame + p``).  The return value of
    ``scan_movers_compact``: the frames plus ``mover``, one uint8 per kept row."""
    return _scan_movers_compact(scene, False, True, poses, dirs, None, max_range, movers, mover_poses, noise, want, capacity)


def scan_noisy_mover_frames(engine, intrinsics, poses, mesh, movers, mover_poses, noise, want=("point3", "sem", "ins")):
    """``RaycastEngineHIP.scan_mover_frames`` with seeded sensor noise drawn in the mover kernels: ``noise`` a
    ``lidarcast.noise.NoiseModel``; pose p is frame ``noise.first_frame + p``, so any subset of a run can be scanned again with
    its exact noise (``noise.at_frame``).  The dict of ``scan_mover_frames``."""
    engine._need_table(intrinsics, "seeded sensor noise under movers needs a sensor with a pose-independent direction table")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    return scan_noisy_movers_compact(engine.scene_for(mesh), poses, engine._resident_table(intrinsics), intrinsics.max_range, movers,
                                     mover_poses, noise, want=want)


# ---- seeded sensor noise under movers in sweeps (include/lidarcast.h "seeded sensor noise under movers in sweeps", DESIGN.md
# section 5t) --------------------------------------------------------------------------------------------------------------------
# Module functions with the scene and the engine as arguments, as the scans of the movers under moving-sensor sweeps are.

def scan_noisy_mover_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, max_range, movers, mover_records_t, noise, mover_t=None,
                                stream=0):
    """``scan_mover_sweeps_dev`` with seeded sensor noise drawn in the mover kernels (lrc_scan_noisy_mover_sweeps_dev): ``noise`` a
    ``lidarcast.noise.NoiseModel`` (sweep p of the call is frame ``noise.first_frame + p``); everything else as there.  The
    all-zero model gives ``scan_mover_sweeps_dev``'s bytes, ``movers=None`` those of ``lidarcast.noise.scan_noisy_sweeps_dev`` and a
    zero column."""
    _scan_movers_dev(scene, True, True, motion_t, dirs_t, fire_t, hits, max_range, movers, mover_records_t, noise, mover_t, stream)


def scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, max_range, movers, mover_records, noise,
                                    want=("point3", "sem", "ins"), capacity=None):
    """``scan_mover_sweeps_compact`` with seeded sensor noise drawn in the mover kernels (lrc_scan_noisy_mover_sweeps_compact):
    ``noise`` a ``lidarcast.noise.NoiseModel``; all sweeps are traced in one call, so sweep p is frame ``noise.first_frame + p``.
    The return value of ``scan_mover_sweeps_compact``."""
    return _scan_movers_compact(scene, True, True, motion, dirs, fire, max_range, movers, mover_records, noise, want, capacity)


def scan_noisy_mover_sweep_frames(engine, intrinsics, start_poses, end_poses, mesh, movers, mover_records, noise,
                                  want=("point3", "sem", "ins"), inputs=None):
    """``scan_mover_sweep_frames`` with seeded sensor noise drawn in the mover kernels: ``noise`` a
    ``lidarcast.noise.NoiseModel``; sweep k is frame ``noise.first_frame + k``, so any run of sweeps can be scanned again with its
    exact noise (``noise.at_frame``).  The dict of ``scan_mover_sweep_frames``: ``point_times`` and ``mover`` included."""
    return _sweep_frames(engine, True, intrinsics, start_poses, end_poses, mesh, movers, mover_records, noise, want, inputs,
                         "seeded sensor noise under movers in sweeps needs a sensor with a pose-independent direction table")


def _bind():
    from .core import Scene
    Scene.scan_noisy_movers_dev = scan_noisy_movers_dev
    Scene.scan_noisy_movers_compact = scan_noisy_movers_compact


_bind()
