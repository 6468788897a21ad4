"""Seeded sensor noise drawn on the GPU (include/lidarcast.h "seeded sensor noise").

``NoiseModel`` names the three sensor parameters the multi-line sensor records declare -- range noise, angle jitter,
dropout -- plus a seed and the frame id of the first pose of a call.  The noise of ray i of pose p is a pure function of
(seed, first_frame + p, i): ``Scene.scan_noisy_dev`` / ``Scene.scan_noisy_compact`` draw it in the trace kernel, and
``draws`` evaluates the same integers and float32 operations on the host, without a GPU.

The same noise under moving-sensor sweeps is this module's own: ``sweep_rays`` (the host twin),
``scan_noisy_sweeps_dev``, ``scan_noisy_sweeps_compact`` and ``scan_noisy_sweep_frames``, module functions that take the
scene or the engine as their first argument.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _capi
from ._capi import LrcNoise, check


@dataclasses.dataclass(frozen=True)
class NoiseModel:
    """seed: 64-bit; range_std in metres; angle_std in RADIANS (azimuth and elevation alike); dropout a probability in
    [0, 1); first_frame: frame id of pose 0 of a call.  Zero parameters switch their step off."""
    seed: int
    range_std: float = 0.0
    angle_std: float = 0.0
    dropout: float = 0.0
    first_frame: int = 0

    @classmethod
    def from_intrinsics(cls, k, seed, first_frame=0):
        """The sensor record's own parameters.  ``angle_noise_std`` of the multi-line record is in DEGREES (its
        ``add_noise`` applies ``np.deg2rad``): converted here."""
        return cls(seed=int(seed), range_std=float(getattr(k, "range_noise_std", 0.0)),
                   angle_std=float(np.deg2rad(getattr(k, "angle_noise_std", 0.0))),
                   dropout=float(getattr(k, "dropout_probability", 0.0)), first_frame=int(first_frame))

    def at_frame(self, first_frame):
        """The same model for a call whose pose 0 is frame ``first_frame``."""
        return dataclasses.replace(self, first_frame=int(first_frame))

    def struct(self):
        nz = LrcNoise()
        nz.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        nz.first_frame = int(self.first_frame) & 0xFFFFFFFFFFFFFFFF
        nz.range_std, nz.angle_std, nz.dropout = float(self.range_std), float(self.angle_std), float(self.dropout)
        return nz


def draws(model, P, N):
    """What the kernel draws for P poses x N rays, on the host (lrc_noise_draws): dict of ``z_range``, ``z_az``, ``z_el``
    (P, N) float32 standard normal variates and ``keep`` (P, N) bool (False: the ray is dropped)."""
    lib = _capi.load()
    P, N = int(P), int(N)
    z = [np.zeros((P, N), np.float32) for _ in range(3)]
    keep = np.zeros((P, N), np.uint8)
    nz = model.struct()
    check(lib.lrc_noise_draws(C.byref(nz), P, N, *(a.ctypes.data for a in z), keep.ctypes.data), "lrc_noise_draws")
    return {"z_range": z[0], "z_az": z[1], "z_el": z[2], "keep": keep.astype(bool)}


def table():
    """(base, slope): the (24, 64) float32 quantile table in use (lrc_noise_table)."""
    lib = _capi.load()
    base, slope = np.zeros((24, 64), np.float32), np.zeros((24, 64), np.float32)
    check(lib.lrc_noise_table(base.ctypes.data, slope.ctypes.data), "lrc_noise_table")
    return base, slope


def words_dev(ctx, ctr=None, key=None, words=None, stream=0):
    """The generator and the variate on the DEVICE, on chosen inputs (test hook lrc_internal_noise_words_dev; ``ctx`` a
    ``lidarcast.Context``).  With ``ctr`` (n, 4) and ``key`` (n, 2) of 32-bit words: the n Philox4x32-10 blocks.  With
    ``words`` (n, 4) instead: those words as they are.  Returns (words (n, 4) uint32, z (n, 4) float32: the standard normal
    variate of every word from the context's resident table)."""
    import torch
    if (ctr is None) == (words is None) or (ctr is not None and key is None):
        raise ValueError("either ctr and key, or words")
    dev = torch.device("cuda", ctx.device)

    def up(a, width):
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, width)
        return torch.from_numpy(a.view(np.int32)).to(dev)
    if ctr is not None:
        c_t, k_t = up(ctr, 4), up(key, 2)
        if c_t.shape[0] != k_t.shape[0]:
            raise ValueError("ctr must be (n, 4) and key (n, 2)")
        w_t = torch.zeros_like(c_t)
    else:
        c_t = k_t = None
        w_t = up(words, 4)
    n = w_t.shape[0]
    z_t = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
    ptr = lambda x: None if x is None else x.data_ptr()
    check(ctx._lib.lrc_internal_noise_words_dev(ctx._h, ptr(c_t), ptr(k_t), n, ptr(w_t), ptr(z_t), C.c_void_p(int(stream))),
          "lrc_internal_noise_words_dev")
    torch.cuda.synchronize(dev)
    return w_t.cpu().numpy().view(np.uint32), z_t.cpu().numpy()


# ---- noisy moving-sensor sweeps (include/lidarcast.h "noisy moving-sensor sweeps") ----------------
# The seeded noise under moving-sensor sweeps: the table row is jittered in front of the rotation into the world, the world
# direction swept behind it, dropout and the range draw as in the static noisy scan.  Module functions, as
# lidarcast.movers.rays / merge are: the scene and the engine are arguments.

def sweep_rays(model, motion, dirs, fire):
    """What the noisy-sweep kernel casts and uses, on the host (lrc_noisy_sweep_rays, compiled from the kernel's own
    generator): ``motion`` (P, 24) records (``lidarcast.motion_records``), ``dirs`` (N, 3) float64, ``fire`` (N,) firing
    fractions in [0, 1).  Dict of ``rays`` (P*N, 6) float32 origin | direction (NaN direction: the ray is dropped),
    ``centres`` (P*N, 3) float64 range-filter centres c(s), ``range_term`` (P*N,) float32 = float32(range_std) * z (zeros
    when range_std == 0) and ``keep`` (P*N,) bool."""
    lib = _capi.load()
    motion = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 24)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    fire = np.ascontiguousarray(fire, dtype=np.float64).reshape(-1)
    if dirs.ndim != 2 or dirs.shape[1] != 3 or fire.size != dirs.shape[0]:
        raise ValueError("dirs must be (N, 3) and fire (N,)")
    P, N = motion.shape[0], dirs.shape[0]
    rays = np.zeros((P * N, 6), np.float32)
    centres = np.zeros((P * N, 3), np.float64)
    term = np.zeros(P * N, np.float32)
    keep = np.zeros(P * N, np.uint8)
    nz = model.struct()
    check(lib.lrc_noisy_sweep_rays(C.byref(nz), motion.ctypes.data, P, dirs.ctypes.data, fire.ctypes.data, N, rays.ctypes.data,
                                   centres.ctypes.data, term.ctypes.data, keep.ctypes.data), "lrc_noisy_sweep_rays")
    return {"rays": rays, "centres": centres, "range_term": term, "keep": keep.astype(bool)}


def scan_noisy_sweeps_dev(scene, motion_t, dirs_t, fire_t, hits, max_range, noise, stream=0):
    """Noisy moving-sensor sweeps on device tensors (lrc_scan_noisy_sweeps_dev): motion_t (P, 24) float64, dirs_t (N, 3)
    float64, fire_t (N,) float64, ``noise`` a NoiseModel (sweep k is frame ``noise.first_frame + k``); records as
    ``Scene.scan_poses_dev``.  The caller vouches for the records and the fire table (see ``lidarcast.motion_records``)."""
    from .core import _dptr, _stream
    P, N = motion_t.shape[0], dirs_t.shape[0]
    if motion_t.numel() != P * 24 or fire_t.numel() != N:
        raise ValueError("motion_t must be (P, 24) and fire_t (N,)")
    nz = noise.struct()
    check(scene._lib.lrc_scan_noisy_sweeps_dev(scene._h, _dptr(motion_t), P, _dptr(dirs_t), N, _dptr(fire_t), float(max_range),
                                               C.byref(nz), C.byref(hits.struct), _stream(stream)), "lrc_scan_noisy_sweeps_dev")


def scan_noisy_sweeps_compact(scene, motion, dirs, fire, max_range, noise, want=("point3", "sem", "ins"), capacity=None):
    """Noisy moving-sensor sweeps straight to frames (lrc_scan_noisy_sweeps_compact): ``motion``, ``dirs`` and ``fire`` as
    ``Scene.scan_sweeps_compact`` takes them (a DirectionTable or an (N, 3) table; ``fire`` None takes the DirectionTable's
    resident fractions, a different table than the resident one is uploaded into it), ``noise`` a NoiseModel.  Same return
    value as ``Scene.scan_poses_compact``."""
    from .core import DirectionTable, _ptr, _table_for
    motion = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 24)
    lib, h, P, reach = scene._lib, scene._h, motion.shape[0], float(max_range)
    if fire is None and not isinstance(dirs, DirectionTable):
        raise ValueError("fire is required with a plain direction table")
    with _table_for(scene.ctx, dirs, fire) as tab:
        if tab is dirs and fire is not None and \
                (tab.fire is None or not np.array_equal(tab.fire, np.asarray(fire, np.float64).reshape(-1))):
            tab.set_fire(fire)
        if tab.fire is None:
            raise ValueError("the direction table has no firing fractions")
        nz = noise.struct()
        return scene._scan_frames("lrc_scan_noisy_sweeps_compact", P, tab.n, want, capacity, lambda fr, cap, total:
                                  lib.lrc_scan_noisy_sweeps_compact(h, _ptr(motion), P, tab._h, reach, C.byref(nz), fr, cap, total))


def scan_noisy_sweep_frames(engine, intrinsics, start_poses, end_poses, mesh, noise, want=("point3", "sem", "ins"), inputs=None):
    """``RaycastEngineHIP.scan_sweep_frames`` with the seeded noise drawn in the kernel: sweep k moves from start_poses[k]
    to end_poses[k] and is frame ``noise.first_frame + k``.  The dict of ``scan_sweep_frames``, ``point_times`` included.
    ``inputs``: a ``sweep_inputs`` triple to scan exactly those records again (with ``noise.at_frame`` for a subset)."""
    motion, fire, T = inputs if inputs is not None else engine.sweep_inputs(intrinsics, start_poses, end_poses)
    engine._need_table(intrinsics, "noisy moving-sensor sweeps need a sensor with a pose-independent direction table",
                       NotImplementedError)
    ask = tuple(want) + (() if "index" in want else ("index",))
    fr = scan_noisy_sweeps_compact(engine.scene_for(mesh), motion, engine._resident_table(intrinsics), fire,
                                   intrinsics.max_range, noise, want=ask)
    fr["point_times"] = fire[fr["index"]] * T
    if "index" not in want:
        del fr["index"]
    return fr
