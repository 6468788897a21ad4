"""Deforming movers: keyframed meshes blended and refitted on the device (include/lidarcast.h "deforming movers", DESIGN.md
section 5o).

``Deformable`` holds one topology with K keyframes of its vertices and owns an ordinary ``Scene`` built from keyframe 0;
``set(k0, k1, w)`` enqueues the blend of two keyframes and the refit of the scene's triangle records, slot boxes and node
boxes -- the tree is not rebuilt, and the refitted tree gives the hits of a fresh build bit for bit.  ``blend`` and ``refit``
are the two host steps of that, without a GPU (lrc_deform_blend, lrc_deform_refit).  ``Clip`` turns times into the
(k0, k1, w) of a cyclic or one-shot animation.  ``SkinnedDeformable`` is a ``Deformable`` whose shapes are bone poses skinned on
the device instead of whole vertex arrays.  A ``lidarcast.movers.MoverSet`` takes a ``Deformable`` among its meshes;
``scan_deforming_frames`` / ``scan_deforming_dev`` scan frames whose movers change shape from frame to frame;
``scan_deforming_flow_frames`` / ``scan_deforming_flow_dev`` add the non-rigid scene flow from each frame to the next (DESIGN.md
section 5p), for which ``Deformable.snapshot`` keeps the shape a frame was scanned with while the next one is set.

Animated movers under sweeps: ``Deformable.span(shape_a, shape_b)`` puts the deformable between two shapes,
and the mover-sweep scans then meet it, ray by ray, at the shape it has at the ray's own firing fraction; ``span_vertices`` and
``span_refit`` are the host steps (lrc_span_vertices, lrc_deform_span_refit), ``scan_deforming_sweeps_dev`` /
``scan_deforming_sweep_frames`` the scans of sweeps whose movers change shape while the sweep is scanned.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import LrcHits, check
from .core import Scene


class _OwnedScene(Scene):
    """The ``Scene`` of a deformable: every method of ``lidarcast.Scene`` on a handle the deformable owns."""

    def __init__(self, ctx, handle, num_vertices, num_triangles):
        self._lib = _capi.load()
        self.ctx = ctx
        self._h = C.c_void_p(handle)
        self.num_vertices, self.num_triangles = num_vertices, num_triangles

    def close(self):            # lrc_deform_destroy frees the scene
        self._h = None


class Deformable:
    """keyframes: (K, V, 3), narrowed to float32 once; triangles (T, 3); optional per-triangle labels.  ``scene`` is the
    deformable's scene (float32 nodes, built from keyframe 0), valid until ``close``; ``keyframes`` the float32 array."""

    def __init__(self, ctx, keyframes, triangles, triangle_sem=None, triangle_ins=None):
        self._lib = _capi.load()
        self.ctx = ctx
        self._h = None
        self.scene = None
        k = np.ascontiguousarray(np.asarray(keyframes), dtype=np.float32)
        if k.ndim != 3 or k.shape[2] != 3:
            raise ValueError("keyframes must be (K, V, 3)")
        f, sem, ins = self._topology(triangles, triangle_sem, triangle_ins)
        self.keyframes, self.triangles = k, f
        self._V = k.shape[1]
        h = C.c_void_p()
        check(self._lib.lrc_deform_create(ctx._h, k.ctypes.data, k.shape[0], k.shape[1], f.ctypes.data, f.shape[0],
                                          None if sem is None else sem.ctypes.data, None if ins is None else ins.ctypes.data,
                                          C.byref(h)), "lrc_deform_create")
        self._h = h
        self.scene = _OwnedScene(ctx, self._lib.lrc_deform_scene(h), k.shape[1], f.shape[0])

    @staticmethod
    def _topology(triangles, triangle_sem, triangle_ins):
        """(triangles (T, 3) uint32, labels (T,) uint16 or None) as the library takes them."""
        f = np.asarray(triangles)
        if f.size == 0:
            f = np.zeros((0, 3), dtype=np.uint32)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("triangles must be (T, 3)")
        if f.size and f.dtype.kind != "u" and f.min() < 0:
            raise ValueError("negative triangle index")
        f = np.ascontiguousarray(f, dtype=np.uint32)
        sem = None if triangle_sem is None else np.ascontiguousarray(triangle_sem, dtype=np.uint16)
        ins = None if triangle_ins is None else np.ascontiguousarray(triangle_ins, dtype=np.uint16)
        for lab in (sem, ins):
            if lab is not None and lab.shape != (f.shape[0],):
                raise ValueError("per-triangle labels must have shape (T,)")
        return f, sem, ins

    def __len__(self):
        return len(self.triangles)

    @property
    def num_keyframes(self):
        return self.keyframes.shape[0]

    def set(self, k0, k1, w, stream=0):
        """Enqueue on ``stream`` the shape ``blend(keyframes[k0], keyframes[k1], w)`` and the refit of the scene to it
        (lrc_deform_set_dev); no host synchronisation.  A scan enqueued on the same stream afterwards sees the new shape."""
        if not self._h:
            raise ValueError("deformable is closed")
        if int(k0) < 0 or int(k1) < 0:
            raise ValueError("keyframe index out of range")
        check(self._lib.lrc_deform_set_dev(self._h, int(k0), int(k1), float(np.float32(w)), C.c_void_p(int(stream))),
              "lrc_deform_set_dev")

    def span(self, shape_a, shape_b, stream=0):
        """Enqueue on ``stream`` the span between two shapes, each a (k0, k1, w) triple as ``set`` takes it
        (lrc_deform_span_dev); no host synchronisation.  A mover-sweep scan enqueued on the same stream afterwards meets the
        deformable per ray at ``span_vertices(VA, VB, float32(fire))``; every other scan or cast sees shape A.  ``set`` ends it."""
        if not self._h:
            raise ValueError("deformable is closed")
        a, b = tuple(shape_a), tuple(shape_b)
        if len(a) != 3 or len(b) != 3:
            raise ValueError("a shape is (k0, k1, w)")
        if min(int(a[0]), int(a[1]), int(b[0]), int(b[1])) < 0:
            raise ValueError("keyframe index out of range")
        check(self._lib.lrc_deform_span_dev(self._h, int(a[0]), int(a[1]), float(np.float32(a[2])), int(b[0]), int(b[1]),
                                            float(np.float32(b[2])), C.c_void_p(int(stream))), "lrc_deform_span_dev")

    def span_launches(self):
        """(kernel launches of one ``span`` whose two shapes are blended, of one whose two shapes are keyframe copies)."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        check(self._lib.lrc_deform_span_launches(self._h, C.byref(a), C.byref(b)), "lrc_deform_span_launches")
        return int(a.value), int(b.value)

    def vertices(self):
        """The current (V, 3) float32 vertices, read back synchronously."""
        out = np.empty((self._V, 3), np.float32)
        check(self._lib.lrc_deform_vertices(self._h, out.ctypes.data), "lrc_deform_vertices")
        return out

    def snapshot(self, out_t=None, stream=0):
        """Enqueue on ``stream`` a copy of the current vertices into ``out_t``, a (V, 3) float32 device tensor (None: a new one),
        and return it (lrc_deform_snapshot_dev); no host synchronisation.  What the non-rigid flow keeps of a shape before the
        next one is set."""
        import torch
        if not self._h:
            raise ValueError("deformable is closed")
        V = self._V
        if out_t is None:
            out_t = torch.empty((V, 3), dtype=torch.float32, device=f"cuda:{self.ctx.device}")
        if out_t.dtype != torch.float32 or not out_t.is_cuda or not out_t.is_contiguous() or out_t.numel() != 3 * V:
            raise ValueError("out_t must be a contiguous (V, 3) float32 device tensor")
        check(self._lib.lrc_deform_snapshot_dev(self._h, C.c_void_p(out_t.data_ptr()), C.c_void_p(int(stream))),
              "lrc_deform_snapshot_dev")
        return out_t

    def launches(self):
        """(kernel launches of one ``set`` that blends, of one that copies a keyframe)."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        check(self._lib.lrc_deform_launches(self._h, C.byref(a), C.byref(b)), "lrc_deform_launches")
        return int(a.value), int(b.value)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.lrc_deform_destroy(self._h)
            self._h = None
        if getattr(self, "scene", None) is not None:
            self.scene._h = None
            self.scene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SkinnedDeformable(Deformable):
    """A ``Deformable`` that keeps no keyframes: a rest shape ``rest`` (V, 3), up to four bone influences per vertex
    (``bone_index`` (V, 4) uint8, ``bone_weight`` (V, 4) float32) and K key poses ``poses12`` (K, B, 12) float32, skinned on the
    device at every ``set`` (lrc_deform_create_skinned).  Key pose k is keyframe k: ``set(k0, k1, w)``
    gives the bytes a ``Deformable`` made from ``lidarcast.skin.keyframes(...)`` holds after the same call, so ``scene``,
    ``set``, ``vertices``, ``snapshot``, ``launches`` and ``close`` are the base class's, and a ``MoverSet``, the
    ``scan_deforming_*`` functions and the non-rigid flow take it as they take a ``Deformable``.  It has no ``keyframes``
    array; ``keyframe(k)`` skins one on the host on demand."""

    def __init__(self, ctx, rest, triangles, bone_index, bone_weight, poses12, triangle_sem=None, triangle_ins=None):
        from . import skin
        self._lib = _capi.load()
        self.ctx = ctx
        self._h = None
        self.scene = None
        r, i, w = skin.influences(rest, bone_index, bone_weight)
        p = skin.clip_poses(poses12)
        f, sem, ins = self._topology(triangles, triangle_sem, triangle_ins)
        self.rest, self.bone_index, self.bone_weight, self.poses12, self.triangles = r, i, w, p, f
        self._V = len(r)
        h = C.c_void_p()
        check(self._lib.lrc_deform_create_skinned(ctx._h, r.ctypes.data, len(r), i.ctypes.data, w.ctypes.data, p.ctypes.data,
                                                  p.shape[0], p.shape[1], f.ctypes.data, f.shape[0],
                                                  None if sem is None else sem.ctypes.data, None if ins is None else ins.ctypes.data,
                                                  C.byref(h)), "lrc_deform_create_skinned")
        self._h = h
        self.scene = _OwnedScene(ctx, self._lib.lrc_deform_scene(h), len(r), f.shape[0])

    @property
    def num_keyframes(self):
        return self.poses12.shape[0]

    def keyframe(self, k):
        """The (V, 3) float32 vertices of key pose ``k``, skinned on the host (``lidarcast.skin.apply``)."""
        from . import skin
        return skin.apply(self.rest, self.bone_index, self.bone_weight, self.poses12[int(k)])


def blend(a, b, w):
    """lrc_deform_blend: the (V, 3) float32 blend of vertex arrays ``a`` and ``b``; no GPU.  Per coordinate
    v = a + w * (b - a), clamped into [min(a, b), max(a, b)]; w == 0 copies ``a`` and w == 1 copies ``b`` bit for bit."""
    lib = _capi.load()
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape")
    out = np.empty_like(a)
    check(lib.lrc_deform_blend(a.ctypes.data, b.ctypes.data, len(a), float(np.float32(w)), out.ctypes.data), "lrc_deform_blend")
    return out


def refit(nodes16, slot_prim, triangles, vertices):
    """lrc_deform_refit: the tree ``nodes16`` (num_nodes, 16) float32 over the leaf slots ``slot_prim`` refitted to
    ``vertices``; no GPU.  Returns (nodes with every child box recomputed and the references untouched, (num_slots, 12)
    triangle records, (num_slots, 6) slot boxes)."""
    lib = _capi.load()
    nodes = np.array(nodes16, dtype=np.float32, order="C").reshape(-1, 16)       # a copy: the input keeps its boxes
    sp = np.ascontiguousarray(slot_prim, dtype=np.uint32).reshape(-1)
    f = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    rec = np.zeros((len(sp), 12), np.float32)
    box = np.zeros((len(sp), 6), np.float32)
    check(lib.lrc_deform_refit(nodes.ctypes.data, len(nodes), sp.ctypes.data, len(sp), f.ctypes.data, len(f), v.ctypes.data,
                               len(v), rec.ctypes.data, box.ctypes.data), "lrc_deform_refit")
    return nodes, rec, box


def span_vertices(a, b, s):
    """lrc_span_vertices: the (V, 3) float32 shape a span between vertex arrays ``a`` and ``b`` has at the firing fraction ``s``
    (narrowed to float32 as the kernel narrows it); no GPU.  Per coordinate ``a`` where s == 0 or the two have the same bits,
    ``b`` where s == 1, else ``blend``'s value."""
    lib = _capi.load()
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError("a and b must have the same shape")
    out = np.empty_like(a)
    check(lib.lrc_span_vertices(a.ctypes.data, b.ctypes.data, len(a), float(np.float32(s)), out.ctypes.data), "lrc_span_vertices")
    return out


def span_refit(nodes16, slot_prim, triangles, vertices_a, vertices_b):
    """lrc_deform_span_refit: the tree ``nodes16`` (num_nodes, 16) float32 over the leaf slots ``slot_prim`` refitted to hold
    both ``vertices_a`` and ``vertices_b``; no GPU.  Returns (nodes with every child box recomputed and the references untouched,
    (num_slots, 6) span boxes, (num_slots, 18) slot vertices: A's three, then B's)."""
    lib = _capi.load()
    nodes = np.ascontiguousarray(nodes16, dtype=np.float32).reshape(-1, 16)
    sp = np.ascontiguousarray(slot_prim, dtype=np.uint32).reshape(-1)
    f = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    va = np.ascontiguousarray(vertices_a, dtype=np.float32).reshape(-1, 3)
    vb = np.ascontiguousarray(vertices_b, dtype=np.float32).reshape(-1, 3)
    if va.shape != vb.shape:
        raise ValueError("vertices_a and vertices_b must have the same shape")
    out = np.zeros_like(nodes)
    box = np.zeros((len(sp), 6), np.float32)
    rec = np.zeros((len(sp), 18), np.float32)
    check(lib.lrc_deform_span_refit(nodes.ctypes.data, len(nodes), sp.ctypes.data, len(sp), f.ctypes.data, len(f), va.ctypes.data,
                                    vb.ctypes.data, len(va), out.ctypes.data, box.ctypes.data, rec.ctypes.data),
          "lrc_deform_span_refit")
    return out, box, rec


class Clip:
    """An animation of K keyframes that takes ``cycle`` seconds: at time t the shape lies at x = (t / cycle + phase) * K
    keyframes.  ``loop``: k0 = floor(x) mod K, k1 = (k0 + 1) mod K (the last keyframe blends back into the first); without
    ``loop`` x is clamped to [0, K - 1] and the clip holds its first and last keyframe.  w = x - floor(x), float64 arithmetic,
    narrowed to float32 last."""

    def __init__(self, K, cycle, phase=0.0, loop=True):
        self.K, self.cycle, self.phase, self.loop = int(K), float(cycle), float(phase), bool(loop)
        if self.K < 1:
            raise ValueError("a clip has at least one keyframe")
        if not (np.isfinite(self.cycle) and self.cycle > 0.0) or not np.isfinite(self.phase):
            raise ValueError("a clip needs a positive finite cycle and a finite phase")

    def shape(self, times):
        """(k0, k1, w) at ``times``: two (n,) uint32 arrays and one (n,) float32 array."""
        t = np.atleast_1d(np.asarray(times, dtype=np.float64))
        if not np.isfinite(t).all():
            raise ValueError("times must be finite")
        x = (t / self.cycle + self.phase) * self.K
        if not self.loop:
            x = np.clip(x, 0.0, float(self.K - 1))
        fl = np.floor(x)
        w = (x - fl).astype(np.float32)
        if self.loop:
            k0 = np.mod(fl, self.K).astype(np.int64)
            k1 = (k0 + 1) % self.K
        else:
            k0 = fl.astype(np.int64)
            k1 = np.minimum(k0 + 1, self.K - 1)
        return k0.astype(np.uint32), k1.astype(np.uint32), w

    def shapes3(self, times):
        """The same as an (n, 3) float64 array [k0, k1, w]: one mover's column of the ``shapes`` of ``scan_deforming_*``."""
        k0, k1, w = self.shape(times)
        return np.stack([k0.astype(np.float64), k1.astype(np.float64), w.astype(np.float64)], 1)


def _shapes(shapes, P, movers):
    ds = [m for m in movers.deformables]
    s = np.asarray(shapes, dtype=np.float64)
    if s.shape != (P, len(ds), 3):
        raise ValueError(f"shapes must be (P, D, 3) = ({P}, {len(ds)}, 3), got {s.shape}")
    return ds, s


def _runs(s):
    """[(first, past-the-end)] of the runs of consecutive frames with equal shapes."""
    P = len(s)
    cut = [0] + [p for p in range(1, P) if not np.array_equal(s[p], s[p - 1])] + [P]
    return [(a, b) for a, b in zip(cut[:-1], cut[1:]) if b > a]


def scan_deforming_frames(engine, intrinsics, poses, mesh, movers, mover_poses, shapes, want=("point3", "sem", "ins"), noise=None):
    """``RaycastEngineHIP.scan_mover_frames`` with movers that change shape from frame to frame: ``shapes`` (P, D, 3) float64
    holds [k0, k1, w] per frame and per deformable of the set, in the set's order (``Clip.shapes3``).  Per run of consecutive
    frames with equal shapes every deformable is set once and the run is scanned by lrc_scan_movers_compact; a scan does not
    depend on how its poses are split into calls, so the runs stack to the dict ``scan_mover_frames``
    returns for all frames.  ``noise``: an optional ``lidarcast.noise.NoiseModel``: frame f is scanned
    with the noise of frame ``noise.first_frame + f`` (a run that starts at frame a scans with ``noise.at_frame(noise.first_frame
    + a)``), by ``scan_noisy_mover_frames``."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    ds, s = _shapes(shapes, P, movers)

    def scan(a, b):
        if noise is None:
            return engine.scan_mover_frames(intrinsics, poses[a:b], mesh, movers, mp[a:b], want=want)
        return engine.scan_noisy_mover_frames(intrinsics, poses[a:b], mesh, movers, mp[a:b],
                                              noise.at_frame(noise.first_frame + a), want=want)

    mp = np.ascontiguousarray(mover_poses, dtype=np.float32)
    if mp.shape != (P, len(movers), 12):
        raise ValueError(f"mover_poses must be (P, M, 12) = ({P}, {len(movers)}, 12), got {mp.shape}")
    parts = []
    for a, b in _runs(s):
        for j, d in enumerate(ds):
            d.set(int(s[a, j, 0]), int(s[a, j, 1]), s[a, j, 2])
        engine.ctx.synchronize()          # the frame path scans on the library's own streams
        parts.append(scan(a, b))
    if not parts:
        return scan(0, P)
    out = {}
    for key in parts[0]:
        if key == "total":
            out[key] = int(sum(p[key] for p in parts))
        else:
            out[key] = np.concatenate([p[key] for p in parts], 0)
    return out


def scan_deforming_dev(scene, poses_t, dirs_t, hits, max_range, movers, mover_poses_t, shapes, mover_t=None, stream=0, noise=None):
    """``Scene.scan_movers_dev`` with movers that change shape from frame to frame, everything enqueued on ``stream`` with no
    host synchronisation: per run of consecutive frames with equal ``shapes`` (P, D, 3) one ``set`` per deformable, then
    lrc_scan_movers_dev on the run's slice of the poses, the records and ``mover_t``.  ``noise``: an optional
    ``lidarcast.noise.NoiseModel``: a run that starts at frame a is scanned by lrc_scan_noisy_movers_dev
    with ``noise.at_frame(noise.first_frame + a)``, so frame f has the noise of frame ``noise.first_frame + f``."""
    P, N = poses_t.shape[0], dirs_t.shape[0]
    if hits.n != P * N:
        raise ValueError("hits must hold P * N records")
    if "tile_count" in hits.want:
        raise ValueError("tile_count is not written by this scan")
    ds, s = _shapes(shapes, P, movers)
    M = len(movers)
    mp = mover_poses_t.reshape(P, M, 12)
    for a, b in _runs(s):
        for j, d in enumerate(ds):
            d.set(int(s[a, j, 0]), int(s[a, j, 1]), s[a, j, 2], stream=stream)
        part = _HitsSlice(hits, a * N, b * N)
        rows = None if mover_t is None else mover_t[a * N:b * N]
        if noise is None:
            scene.scan_movers_dev(poses_t[a:b], dirs_t, part, max_range, movers, mp[a:b], rows, stream=stream)
        else:
            scene.scan_noisy_movers_dev(poses_t[a:b], dirs_t, part, max_range, movers, mp[a:b],
                                        noise.at_frame(noise.first_frame + a), rows, stream=stream)


def _span_shapes(shapes_a, shapes_b, P, movers):
    ds, a = _shapes(shapes_a, P, movers)
    _, b = _shapes(shapes_b, P, movers)
    return ds, a, b, _runs(np.concatenate([a, b], axis=2))


def scan_deforming_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, max_range, movers, records_t, shapes_a, shapes_b,
                              mover_t=None, stream=0, noise=None):
    """``lidarcast.movers.scan_mover_sweeps_dev`` with movers that change shape while a sweep is scanned,
    everything enqueued on ``stream`` with no host synchronisation: ``shapes_a`` / ``shapes_b`` (P, D, 3) float64 hold [k0, k1,
    w] at the start and at the end of every sweep per deformable of the set, in the set's order (``Clip.shapes3`` of the two
    times).  Per run of consecutive sweeps with equal (A, B) one ``span`` per deformable, then lrc_scan_mover_sweeps_dev on the
    run's slice of the sensor records, the mover records, the hit records and ``mover_t``.  ``noise``: an optional
    ``lidarcast.noise.NoiseModel``: a run that starts at sweep a is scanned by
    lrc_scan_noisy_mover_sweeps_dev with ``noise.at_frame(noise.first_frame + a)``, so sweep p has the noise of frame
    ``noise.first_frame + p``; a dropped ray meets no shape, and the jitter does not touch the fraction the shape is taken at."""
    from .movers import scan_mover_sweeps_dev, scan_noisy_mover_sweeps_dev
    P, N = motion_t.shape[0], dirs_t.shape[0]
    if hits.n != P * N:
        raise ValueError("hits must hold P * N records")
    if "tile_count" in hits.want:
        raise ValueError("tile_count is not written by this scan")
    ds, sa, sb, runs = _span_shapes(shapes_a, shapes_b, P, movers)
    mt = motion_t.reshape(P, 24)
    rt = records_t.reshape(P, len(movers), 24)
    for a, b in runs:
        for j, d in enumerate(ds):
            d.span(sa[a, j], sb[a, j], stream=stream)
        rows = None if mover_t is None else mover_t[a * N:b * N]
        if noise is None:
            scan_mover_sweeps_dev(scene, mt[a:b], dirs_t, fire_t, _HitsSlice(hits, a * N, b * N), max_range, movers, rt[a:b], rows,
                                  stream=stream)
        else:
            scan_noisy_mover_sweeps_dev(scene, mt[a:b], dirs_t, fire_t, _HitsSlice(hits, a * N, b * N), max_range, movers, rt[a:b],
                                        noise.at_frame(noise.first_frame + a), rows, stream=stream)


def scan_deforming_sweep_frames(engine, intrinsics, start_poses, end_poses, mesh, movers, mover_records, shapes_a, shapes_b,
                                want=("point3", "sem", "ins"), inputs=None, noise=None):
    """``lidarcast.movers.scan_mover_sweep_frames`` with movers that change shape while a sweep is scanned: the host-pointer twin
    of ``scan_deforming_sweeps_dev``.  Per run of consecutive sweeps with equal (A, B) every deformable is spanned once, the
    context is synchronised (the frame path scans on the library's own streams) and the run is scanned by
    lrc_scan_mover_sweeps_compact; the runs stack to the dict ``scan_mover_sweep_frames`` returns for all sweeps
    (``point_times`` and ``mover`` included).  ``noise``: an optional ``lidarcast.noise.NoiseModel``: a
    run that starts at sweep a is scanned by lrc_scan_noisy_mover_sweeps_compact with ``noise.at_frame(noise.first_frame + a)``."""
    from .movers import scan_mover_sweep_frames, scan_noisy_mover_sweep_frames

    def scan(a, b):
        if noise is None:
            return scan_mover_sweep_frames(engine, intrinsics, None, None, mesh, movers, rec[a:b], want=want,
                                           inputs=(motion[a:b], fire, T))
        return scan_noisy_mover_sweep_frames(engine, intrinsics, None, None, mesh, movers, rec[a:b],
                                             noise.at_frame(noise.first_frame + a), want=want, inputs=(motion[a:b], fire, T))
    motion, fire, T = inputs if inputs is not None else engine.sweep_inputs(intrinsics, start_poses, end_poses)
    motion = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 24)
    P = len(motion)
    rec = np.ascontiguousarray(mover_records, dtype=np.float32)
    if rec.shape != (P, len(movers), 24):
        raise ValueError(f"mover_records must be (P, M, 24) = ({P}, {len(movers)}, 24), got {rec.shape}")
    ds, sa, sb, runs = _span_shapes(shapes_a, shapes_b, P, movers)
    parts = []
    for a, b in runs:
        for j, d in enumerate(ds):
            d.span(sa[a, j], sb[a, j])
        engine.ctx.synchronize()
        parts.append(scan(a, b))
    if not parts:
        return scan(0, P)
    out = {}
    for key in parts[0]:
        if key == "total":
            out[key] = int(sum(p[key] for p in parts))
        else:
            out[key] = np.concatenate([p[key] for p in parts], 0)
    return out


def _mover_index(movers, d):
    """The place of deformable ``d`` among the movers of the set."""
    return next(m for m, sc in enumerate(movers.scenes) if sc is d.scene)


def scan_deforming_flow_dev(scene, poses_t, dirs_t, hits, max_range, movers, mover_poses_t, shapes, flow_t, status_t=None,
                            mover_t=None, stream=0):
    """``scan_deforming_dev`` with non-rigid scene flow: frame k is paired with frame k + 1 -- the next
    sensor pose ``poses_t[k + 1]``, the movers' poses ``mover_poses_t[k + 1]`` and the shapes ``shapes[k + 1]`` -- and everything
    is enqueued on ``stream`` with no host wait.  Per frame: shape k is set unless it already stands, the frame is scanned, the
    deformables whose shape changes are snapshot, shape k + 1 is set, and lrc_scan_nonrigid_flow_dev is called with one surface
    pair per changed deformable (snapshot -> current vertices); so every shape is blended and refitted once.  ``hits`` must hold
    t, point3 and prim; ``flow_t`` (P * N, 3) float32 and ``status_t`` (P * N) uint8 or None receive the two columns, the last
    frame's +0 and 0 (it has no next).  ``mover_t`` (P * N) uint8 receives the mover column (None: a tensor of this call's)."""
    import torch
    P, N = poses_t.shape[0], dirs_t.shape[0]
    if hits.n != P * N:
        raise ValueError("hits must hold P * N records")
    if "tile_count" in hits.want:
        raise ValueError("tile_count is not written by this scan")
    if not all(a in hits.want for a in ("t", "point3", "prim")):
        raise ValueError("hits must hold t, point3 and prim")
    if flow_t is None or flow_t.numel() != 3 * P * N:
        raise ValueError("flow_t must be (P * N, 3)")
    ds, s = _shapes(shapes, P, movers)
    if len(ds) > 16:
        raise ValueError("at most 16 deforming movers take part in a non-rigid flow")
    M = len(movers)
    mp = mover_poses_t.reshape(P, M, 12)
    pt = poses_t.reshape(P, 16)
    flow = flow_t.reshape(P * N, 3)
    where = [_mover_index(movers, d) for d in ds]
    # torch's own work (the mover column, the snapshots, the last frame's zeros) goes to the caller's stream as well
    own = torch.cuda.ExternalStream(int(stream), device=poses_t.device) if int(stream) else torch.cuda.default_stream(poses_t.device)
    with torch.cuda.stream(own):
        if mover_t is None:
            mover_t = torch.empty(P * N, dtype=torch.uint8, device=poses_t.device)
        snaps = [None] * len(ds)
        standing = [None] * len(ds)                # the shape each deformable's scene holds
        for k in range(P):
            for j, d in enumerate(ds):
                if standing[j] is None or not np.array_equal(standing[j], s[k, j]):
                    d.set(int(s[k, j, 0]), int(s[k, j, 1]), s[k, j, 2], stream=stream)
                    standing[j] = s[k, j]
            rows = slice(k * N, (k + 1) * N)
            part = _HitsSlice(hits, k * N, (k + 1) * N)
            scene.scan_movers_dev(pt[k:k + 1], dirs_t, part, max_range, movers, mp[k:k + 1], mover_t[rows], stream=stream)
            if k + 1 == P:
                flow[rows].zero_()
                if status_t is not None:
                    status_t[rows].zero_()
                break
            pairs = []
            for j, d in enumerate(ds):
                if not np.array_equal(s[k + 1, j], s[k, j]):
                    snaps[j] = d.snapshot(snaps[j], stream=stream)
                    d.set(int(s[k + 1, j, 0]), int(s[k + 1, j, 1]), s[k + 1, j, 2], stream=stream)
                    standing[j] = s[k + 1, j]
                    pairs.append((where[j], snaps[j], None))
            scene.scan_nonrigid_flow_dev(part, mover_t[rows], 1, N, max_range, movers, mp[k:k + 1], mp[k + 1:k + 2], pt[k + 1:k + 2],
                                         flow[rows], pairs=pairs, status_t=None if status_t is None else status_t[rows],
                                         stream=stream)
    return mover_t


def scan_deforming_flow_frames(engine, intrinsics, poses, mesh, movers, mover_poses, shapes, want=("point3", "sem", "ins")):
    """``scan_deforming_frames`` with non-rigid scene flow: the dict it returns plus ``flow`` (float32 x 3) and ``flow_status``
    (uint8: 0 no next frame, 1 visible, 2 occluded, 3 out of range), one entry per kept row; frame k is paired with k + 1.  The
    shared columns are ``scan_deforming_frames``' own; the two flow columns come from ``scan_deforming_flow_dev`` on the
    engine's context, gathered for the kept rows by the frames' index column."""
    import torch
    engine._need_table(intrinsics, "scene flow needs a sensor with a pose-independent direction table")
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    P = len(poses)
    ask = tuple(want) + (() if "index" in want else ("index",))
    out = scan_deforming_frames(engine, intrinsics, poses, mesh, movers, mover_poses, shapes, want=ask)
    from .core import DeviceHits
    dirs = np.ascontiguousarray(engine._direction_table(intrinsics), dtype=np.float64)
    N = len(dirs)
    dev = f"cuda:{engine.ctx.device}"
    hits = DeviceHits(P * N, dev, want=("t", "point3", "prim"))
    flow_t = torch.empty((P * N, 3), dtype=torch.float32, device=dev)
    status_t = torch.empty(P * N, dtype=torch.uint8, device=dev)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    scan_deforming_flow_dev(engine.scene_for(mesh), to(poses.reshape(P, 16)), to(dirs), hits, intrinsics.max_range, movers,
                            to(np.ascontiguousarray(mover_poses, dtype=np.float32)), shapes, flow_t, status_t)
    row = np.repeat(np.arange(P, dtype=np.int64) * N, out["counts"].astype(np.int64)) + out["index"].astype(np.int64)
    row_t = torch.from_numpy(row).to(dev)
    out["flow"] = flow_t[row_t].cpu().numpy()
    out["flow_status"] = status_t[row_t].cpu().numpy()
    if "index" not in want:
        del out["index"]
    return out


class _HitsSlice:
    """Records [first, last) of a ``DeviceHits`` as the records of a call of their own."""

    def __init__(self, hits, first, last):
        self.n = last - first
        self.want = hits.want
        self.tensors = {a: hits.tensors[a][first:last] for a in hits.want}
        self.struct = LrcHits()
        for a, t in self.tensors.items():
            setattr(self.struct, a, t.data_ptr())
