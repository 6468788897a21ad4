"""Scene flow under movers: per-point flow and visibility at the next frame (include/lidarcast.h "scene flow", DESIGN.md
section 5m).

For every return of a frame scanned with movers (``Scene.scan_movers_dev``): ``flow`` is the displacement of the surface the point
lies on up to a next frame, ``status`` whether that place has a line of sight from the next sensor pose and lies in range.
``Scene.scan_flow_dev`` / ``Scene.scan_flow_compact`` compute both on the GPU; ``rays`` and ``status`` are the host steps of
that, without a GPU (lrc_flow_rays, lrc_flow_status); ``sensor_flow`` turns the world flow into the moving sensor's coordinates.
``Scene.scan_nonrigid_flow_dev`` and ``nonrigid_rays`` are the same for a set with deforming movers: rows on
a deforming triangle flow with the triangle from one shape to the next; ``lidarcast.deform`` pairs the frames of an animation.
"""
import numpy as np

from . import _capi
from ._capi import check

NONE, VISIBLE, OCCLUDED, OUT_OF_RANGE = 0, 1, 2, 3
STATUS_NAMES = ("none", "visible", "occluded", "out_of_range")


def pair_next(poses, mover_poses=None):
    """Frame k paired with k + 1, the last frame with nothing: (next_poses (P, 4, 4), next_mover_poses (P, M, 12) or None,
    has_next (P,) uint8).  The last frame's "next" entries repeat its own, so that every table is a checked pose."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    nxt = np.concatenate([poses[1:], poses[-1:]]) if P else poses.copy()
    has = np.ones(P, np.uint8)
    if P:
        has[-1] = 0
    nmp = None
    if mover_poses is not None:
        mp = np.ascontiguousarray(mover_poses, dtype=np.float32)
        nmp = np.concatenate([mp[1:], mp[-1:]]) if P else mp.copy()
    return nxt, nmp, has


def rays(t, point3, mover, mover_poses, next_mover_poses, next_poses, has_next, max_range, min_range=0.0):
    """lrc_flow_rays: steps 1 to 3 for P frames of N rows; no GPU.  ``t`` (P * N,) float32 (+inf: no return), ``point3``
    (P * N, 3) float32, ``mover`` (P * N,) uint8 or None, ``mover_poses`` / ``next_mover_poses`` (P, M, 12) float32 or None (no
    movers), ``next_poses`` (P, 4, 4) float64, ``has_next`` (P,) uint8 or None.  Returns a dict: flow3, rays6 (o, h), keep, thr and
    the status so far (0, 3, or 1 for a row to be cast)."""
    lib = _capi.load()
    nxt = np.ascontiguousarray(next_poses, dtype=np.float64).reshape(-1, 16)
    P = len(nxt)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    n = len(t)
    if P == 0 or n % P:
        raise ValueError("t must hold P * N entries")
    N = n // P
    x = np.ascontiguousarray(point3, dtype=np.float32).reshape(n, 3)
    M, w, A, B = 0, None, None, None
    if mover_poses is not None:
        A = np.ascontiguousarray(mover_poses, dtype=np.float32)
        B = np.ascontiguousarray(next_mover_poses, dtype=np.float32)
        if A.ndim != 3 or A.shape[0] != P or A.shape[2] != 12 or B.shape != A.shape:
            raise ValueError("mover_poses and next_mover_poses must be (P, M, 12)")
        M = A.shape[1]
        w = np.ascontiguousarray(mover, dtype=np.uint8).reshape(n)
    hn = None if has_next is None else np.ascontiguousarray(has_next, dtype=np.uint8).reshape(P)
    out = {"flow3": np.empty((n, 3), np.float32), "rays6": np.empty((n, 6), np.float32), "keep": np.empty(n, np.uint8),
           "thr": np.empty(n, np.float32), "status": np.empty(n, np.uint8)}
    ptr = lambda a: None if a is None else a.ctypes.data
    check(lib.lrc_flow_rays(ptr(t), ptr(x), ptr(w), P, N, M, ptr(A), ptr(B), ptr(nxt), ptr(hn), float(max_range), float(min_range),
                            ptr(out["flow3"]), ptr(out["rays6"]), ptr(out["keep"]), ptr(out["thr"]), ptr(out["status"])),
          "lrc_flow_rays")
    return out


def nonrigid_rays(t, point3, mover, prim, mover_poses, next_mover_poses, next_poses, has_next, max_range, pairs, min_range=0.0):
    """lrc_nonrigid_flow_rays: ``rays`` for a set with deforming movers (non-rigid scene flow); no GPU.
    ``prim`` (P * N,) uint32 is the records' prim column; ``pairs`` a list of (mover m, verts_a (V, 3) float32, verts_b (V, 3)
    float32, triangles (T, 3)): rows of mover m + 1 whose prim is below T flow with their triangle from shape a to shape b,
    every other row takes the rigid step.  The dict of ``rays``."""
    import ctypes as C
    lib = _capi.load()
    nxt = np.ascontiguousarray(next_poses, dtype=np.float64).reshape(-1, 16)
    P = len(nxt)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    n = len(t)
    if P == 0 or n % P:
        raise ValueError("t must hold P * N entries")
    N = n // P
    x = np.ascontiguousarray(point3, dtype=np.float32).reshape(n, 3)
    j = np.ascontiguousarray(prim, dtype=np.uint32).reshape(n)
    M, w, A, B = 0, None, None, None
    if mover_poses is not None:
        A = np.ascontiguousarray(mover_poses, dtype=np.float32)
        B = np.ascontiguousarray(next_mover_poses, dtype=np.float32)
        if A.ndim != 3 or A.shape[0] != P or A.shape[2] != 12 or B.shape != A.shape:
            raise ValueError("mover_poses and next_mover_poses must be (P, M, 12)")
        M = A.shape[1]
        w = np.ascontiguousarray(mover, dtype=np.uint8).reshape(n)
    hn = None if has_next is None else np.ascontiguousarray(has_next, dtype=np.uint8).reshape(P)
    pairs = list(pairs)
    held = []               # the arrays behind the pointers, alive across the call
    table = (_capi.LrcSurfacePairHost * max(len(pairs), 1))()
    for k, (m, va, vb, tris) in enumerate(pairs):
        va = np.ascontiguousarray(va, dtype=np.float32).reshape(-1, 3)
        vb = np.ascontiguousarray(vb, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 3)
        if va.shape != vb.shape:
            raise ValueError(f"pair {k}: verts_a and verts_b must have the same shape")
        held.append((va, vb, f))
        table[k] = _capi.LrcSurfacePairHost(int(m), va.ctypes.data, vb.ctypes.data, f.ctypes.data, len(f), len(va))
    out = {"flow3": np.empty((n, 3), np.float32), "rays6": np.empty((n, 6), np.float32), "keep": np.empty(n, np.uint8),
           "thr": np.empty(n, np.float32), "status": np.empty(n, np.uint8)}
    ptr = lambda a: None if a is None else a.ctypes.data
    check(lib.lrc_nonrigid_flow_rays(ptr(t), ptr(x), ptr(w), ptr(j), P, N, M, ptr(A), ptr(B), ptr(nxt), ptr(hn), float(max_range),
                                     float(min_range), C.cast(table, C.c_void_p), len(pairs), ptr(out["flow3"]), ptr(out["rays6"]),
                                     ptr(out["keep"]), ptr(out["thr"]), ptr(out["status"])), "lrc_nonrigid_flow_rays")
    return out


def status(t_static, t_movers, thr, status_in):
    """lrc_flow_status: step 5 for n rows; no GPU.  ``t_static`` (n,) float32 ranges of the room's cast, ``t_movers`` (M, n) of the
    movers' casts or None, ``thr`` (n,) and ``status_in`` (n,) uint8 of ``rays``.  Returns the final (n,) uint8 status."""
    lib = _capi.load()
    ts = np.ascontiguousarray(t_static, dtype=np.float32).reshape(-1)
    n = len(ts)
    tm = None if t_movers is None else np.ascontiguousarray(t_movers, dtype=np.float32).reshape(-1, n)
    M = 0 if tm is None else tm.shape[0]
    th = np.ascontiguousarray(thr, dtype=np.float32).reshape(n)
    st = np.ascontiguousarray(status_in, dtype=np.uint8).reshape(n)
    out = np.empty(n, np.uint8)
    check(lib.lrc_flow_status(n, M, ts.ctypes.data, None if not M else tm.ctypes.data, th.ctypes.data, st.ctypes.data,
                              out.ctypes.data), "lrc_flow_status")
    return out


def sensor_flow(points, flow, pose, next_pose):
    """The flow as the moving sensor sees it, float64 on the host: a world point x with world flow f lies at T_k^-1 x in the
    sensor's frame now and at T_(k+1)^-1 (x + f) next; the difference of the two, (K, 3) float64."""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    f = np.asarray(flow, np.float64).reshape(-1, 3)
    T0, T1 = np.asarray(pose, np.float64).reshape(4, 4), np.asarray(next_pose, np.float64).reshape(4, 4)
    now = (x - T0[:3, 3]) @ T0[:3, :3]
    nxt = ((x + f) - T1[:3, 3]) @ T1[:3, :3]
    return nxt - now


# ---- the scans (lrc_scan_flow_dev, lrc_scan_flow_compact) -------------------------------------------------------------------------
# Module functions with the scene and the engine as arguments, as lidarcast.noise's sweep scans are; they are also bound below as
# ``Scene.scan_flow_dev``, ``Scene.scan_flow_compact`` and ``RaycastEngineHIP.scan_flow_frames``.

def scan_flow_dev(scene, hits, mover_t, P, N, max_range, movers, mover_poses_t, next_mover_poses_t, next_poses_t, flow_t,
                  status_t=None, has_next_t=None, stream=0):
    """Scene flow of the records of ``Scene.scan_movers_dev`` on device tensors (lrc_scan_flow_dev): ``hits`` holds P * N records
    with t and point3, ``mover_t`` their (P * N) uint8 mover column (None without a set), ``mover_poses_t`` /
    ``next_mover_poses_t`` (P, M, 12) float32, ``next_poses_t`` (P, 16) float64, ``has_next_t`` an optional (P) uint8 tensor.
    ``flow_t`` (P * N, 3) float32 receives the flow, ``status_t`` (P * N) uint8 the status (None: the flow alone, nothing is
    cast).  Everything is enqueued on ``stream``."""
    import ctypes as C

    import torch

    from .core import _check_side_tensor, _dptr, _stream
    if hits.n != P * N:
        raise ValueError("hits must hold P * N records")
    if flow_t is None:
        raise ValueError("flow_t must be (P * N, 3)")
    handle, entries = None, None
    if movers is not None:
        handle, entries = movers.handle(scene.ctx), P * len(movers) * 12
        if mover_poses_t is None or next_mover_poses_t is None:
            raise ValueError("mover_poses_t and next_mover_poses_t must be (P, M, 12)")
    _check_side_tensor("mover_poses_t", mover_poses_t, torch.float32, entries, "be (P, M, 12)", flow_t)
    _check_side_tensor("next_mover_poses_t", next_mover_poses_t, torch.float32, entries, "be (P, M, 12)", flow_t)
    _check_side_tensor("mover_t", mover_t, torch.uint8, P * N, "hold P * N entries", flow_t)
    _check_side_tensor("next_poses_t", next_poses_t, torch.float64, P * 16, "be (P, 16)", flow_t)
    _check_side_tensor("has_next_t", has_next_t, torch.uint8, P, "hold P entries", flow_t)
    _check_side_tensor("flow_t", flow_t, torch.float32, 3 * P * N, "be (P * N, 3)", flow_t)
    _check_side_tensor("status_t", status_t, torch.uint8, P * N, "hold P * N entries", flow_t)
    check(scene._lib.lrc_scan_flow_dev(scene._h, handle, C.byref(hits.struct), _dptr(mover_t), P, N, _dptr(mover_poses_t),
                                       _dptr(next_mover_poses_t), _dptr(next_poses_t), _dptr(has_next_t), float(max_range),
                                       _dptr(flow_t), _dptr(status_t), _stream(stream)), "lrc_scan_flow_dev")


def scan_nonrigid_flow_dev(scene, hits, mover_t, P, N, max_range, movers, mover_poses_t, next_mover_poses_t, next_poses_t, flow_t,
                           pairs=(), status_t=None, has_next_t=None, stream=0):
    """``scan_flow_dev`` for a set with deforming movers (lrc_scan_nonrigid_flow_dev): ``hits`` holds t,
    point3 AND prim; ``pairs`` is a list of at most 16 (mover m, verts_a_t, verts_b_t) with (V, 3) float32 device tensors of
    mover m's deformable -- the shape the records were scanned with (``Deformable.snapshot``) and the next shape, None for the
    deformable's current vertices.  All P frames share the pairs.  The status is cast against the movers' scenes as they stand
    on ``stream``: set the next shape before the call.  Without pairs this is ``scan_flow_dev``."""
    import ctypes as C

    import torch

    from .core import _check_side_tensor, _dptr, _stream
    if hits.n != P * N:
        raise ValueError("hits must hold P * N records")
    if flow_t is None:
        raise ValueError("flow_t must be (P * N, 3)")
    handle, entries = None, None
    if movers is not None:
        handle, entries = movers.handle(scene.ctx), P * len(movers) * 12
        if mover_poses_t is None or next_mover_poses_t is None:
            raise ValueError("mover_poses_t and next_mover_poses_t must be (P, M, 12)")
    _check_side_tensor("mover_poses_t", mover_poses_t, torch.float32, entries, "be (P, M, 12)", flow_t)
    _check_side_tensor("next_mover_poses_t", next_mover_poses_t, torch.float32, entries, "be (P, M, 12)", flow_t)
    _check_side_tensor("mover_t", mover_t, torch.uint8, P * N, "hold P * N entries", flow_t)
    _check_side_tensor("next_poses_t", next_poses_t, torch.float64, P * 16, "be (P, 16)", flow_t)
    _check_side_tensor("has_next_t", has_next_t, torch.uint8, P, "hold P entries", flow_t)
    _check_side_tensor("flow_t", flow_t, torch.float32, 3 * P * N, "be (P * N, 3)", flow_t)
    _check_side_tensor("status_t", status_t, torch.uint8, P * N, "hold P * N entries", flow_t)
    pairs = list(pairs)
    table = (_capi.LrcSurfacePair * max(len(pairs), 1))()
    for k, (m, va_t, vb_t) in enumerate(pairs):
        V = None                # the size is checked where the mover is known to be a deformable's scene; the library refuses the rest
        if movers is not None and 0 <= int(m) < len(movers) and any(d.scene is movers.scenes[int(m)] for d in movers.deformables):
            V = 3 * movers.scenes[int(m)].num_vertices
        _check_side_tensor(f"pairs[{k}] verts_a_t", va_t, torch.float32, V, "be (V, 3)", flow_t)
        _check_side_tensor(f"pairs[{k}] verts_b_t", vb_t, torch.float32, V, "be (V, 3)", flow_t)
        table[k] = _capi.LrcSurfacePair(int(m), _dptr(va_t), _dptr(vb_t))
    check(scene._lib.lrc_scan_nonrigid_flow_dev(scene._h, handle, C.byref(hits.struct), _dptr(mover_t), P, N, _dptr(mover_poses_t),
                                                _dptr(next_mover_poses_t), _dptr(next_poses_t), _dptr(has_next_t),
                                                float(max_range), C.cast(table, C.c_void_p) if pairs else None, len(pairs),
                                                _dptr(flow_t), _dptr(status_t), _stream(stream)), "lrc_scan_nonrigid_flow_dev")


def scan_flow_compact(scene, poses, dirs, max_range, movers, mover_poses, next_poses, next_mover_poses, has_next=None,
                      want=("point3", "sem", "ins"), capacity=None, with_status=True):
    """``Scene.scan_movers_compact`` with scene flow (lrc_scan_flow_compact): per pose the sensor pose ``next_poses`` (P, 4, 4)
    and the mover poses ``next_mover_poses`` (P, M, 12) of the frame to flow to, ``has_next`` (P,) uint8 or None (all ones).  The
    return value of ``scan_movers_compact`` plus, one entry per kept row, ``flow`` (float32 x 3: the displacement of the surface
    under the point) and ``flow_status`` (uint8: 1 visible from the next pose, 2 occluded, 3 out of range, 0 no next frame; left
    out with ``with_status=False``, which casts nothing)."""
    from .core import _ptr, _table_for
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
    lib, h, P, reach = scene._lib, scene._h, poses.shape[0], float(max_range)
    nxt = np.ascontiguousarray(next_poses, dtype=np.float64).reshape(-1, 16)
    if nxt.shape[0] != P:
        raise ValueError(f"next_poses must be (P, 4, 4) with P = {P}")
    hn = None if has_next is None else np.ascontiguousarray(has_next, dtype=np.uint8).reshape(-1)
    if hn is not None and hn.shape[0] != P:
        raise ValueError(f"has_next must hold P = {P} entries")
    with _table_for(scene.ctx, dirs) as table:
        handle, mp, nmp = None, None, None
        if movers is not None:
            handle = movers.handle(scene.ctx)
            mp = np.ascontiguousarray(mover_poses, dtype=np.float32)
            nmp = np.ascontiguousarray(next_mover_poses, dtype=np.float32)
            for name, a in (("mover_poses", mp), ("next_mover_poses", nmp)):
                if a.shape != (P, len(movers), 12):
                    raise ValueError(f"{name} must be (P, M, 12) = ({P}, {len(movers)}, 12), got {a.shape}")
        side = [("mover", np.uint8, ()), ("flow", np.float32, (3,))] + ([("flow_status", np.uint8, ())] if with_status else [])
        return scene._scan_frames("lrc_scan_flow_compact", P, table.n, want, capacity, lambda fr, cap, total, rows, flow, st=None:
                                  lib.lrc_scan_flow_compact(h, handle, _ptr(poses), P, table._h, _ptr(mp), _ptr(nxt), _ptr(nmp),
                                                            _ptr(hn), reach, fr, rows, flow, st, cap, total),
                                  side=side)


def scan_flow_frames(engine, intrinsics, poses, mesh, movers, mover_poses, want=("point3", "sem", "ins")):
    """``RaycastEngineHIP.scan_mover_frames`` with scene flow: frame k is paired with frame k + 1 -- its flow leads to the movers'
    poses ``mover_poses[k + 1]`` and its status says whether the place can be seen from ``poses[k + 1]`` -- and the last frame
    has no next.  The dict of ``scan_mover_frames`` plus ``flow`` (float32 x 3) and ``flow_status`` (uint8: 0 no next frame,
    1 visible, 2 occluded, 3 out of range), one entry per kept row."""
    engine._need_table(intrinsics, "scene flow needs a sensor with a pose-independent direction table")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    nxt, nmp, has = pair_next(poses, None if movers is None else mover_poses)
    return scan_flow_compact(engine.scene_for(mesh), poses, engine._resident_table(intrinsics), intrinsics.max_range, movers,
                             mover_poses, nxt, nmp, has, want=want)


def _bind():
    from .core import Scene
    Scene.scan_flow_dev = scan_flow_dev
    Scene.scan_nonrigid_flow_dev = scan_nonrigid_flow_dev
    Scene.scan_flow_compact = scan_flow_compact


_bind()
