"""Beam footprint and multi-echo returns (include/lidarcast.h "beam footprint and multi-echo returns").

``BeamModel`` describes a diverging beam as K sub-rays around the axis and the reduction of their closest hits to at most
``max_echoes`` echoes: ``Scene.scan_echoes_dev`` / ``Scene.scan_echoes_compact`` cast the sub-rays in neighbouring lanes of
the trace kernel and reduce them there; ``BeamModel.reduce`` runs the same reduction on the host, without a GPU
(lrc_echo_reduce).
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import LrcBeam, check

PATTERNS = ("single", "cross5", "hex7")


def pattern_offsets(pattern, divergence):
    """(K, 2) float64 offsets (du, dv) in radians of a named pattern, the axis first: ``single`` the axis alone, ``cross5`` /
    ``hex7`` the axis plus a ring of 4 / 6 sub-rays at 90 / 60 degree steps, at radius ``divergence / (2 sqrt 2)`` (the RMS radius
    of a uniformly lit disc whose full angle is ``divergence``)."""
    if pattern == "single":
        return np.zeros((1, 2))
    if pattern not in ("cross5", "hex7"):
        raise ValueError(f"unknown beam pattern {pattern!r} (one of {PATTERNS}, or a (K, 2) array)")
    n = 4 if pattern == "cross5" else 6
    r = float(divergence) / (2.0 * math.sqrt(2.0))
    ang = np.arange(n) * (2.0 * math.pi / n)
    return np.concatenate([np.zeros((1, 2)), np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)])


class BeamModel:
    """divergence: the beam's full angle in RADIANS; pattern: ``single``, ``cross5``, ``hex7`` or an explicit (K, 2) array of
    (du, dv) offsets in radians (1 <= K <= 16; ``divergence`` is then informative only); max_echoes in [1, 4]; separation in
    metres: hits further apart along the beam than this start a new echo; min_fraction: echoes carried by fewer than
    ``max(1, ceil(min_fraction * K))`` sub-rays are discarded."""

    def __init__(self, divergence, pattern="hex7", max_echoes=2, separation=0.05, min_fraction=0.0):
        self.divergence = float(divergence)
        if isinstance(pattern, str):
            self.pattern = pattern
            off = pattern_offsets(pattern, self.divergence)
        else:
            self.pattern = "explicit"
            off = np.array(pattern, dtype=np.float64)
            if off.ndim != 2 or off.shape[1] != 2:
                raise ValueError("an explicit beam pattern must be a (K, 2) array")
        if not np.isfinite(self.divergence) or self.divergence < 0.0:
            raise ValueError("divergence must be finite and not negative")
        if not 1 <= len(off) <= 16:
            raise ValueError("a beam has 1 to 16 sub-rays")
        if not np.isfinite(off).all():
            raise ValueError("non-finite beam offset")
        if not 1 <= int(max_echoes) <= 4:
            raise ValueError("max_echoes must lie in [1, 4]")
        if not (np.isfinite(separation) and separation > 0.0):
            raise ValueError("separation must be finite and positive")
        if not 0.0 <= float(min_fraction) <= 1.0:
            raise ValueError("min_fraction must lie in [0, 1]")
        self.offsets = np.ascontiguousarray(off)
        self.offsets.setflags(write=False)
        self.max_echoes = int(max_echoes)
        self.separation = float(separation)
        self.min_fraction = float(min_fraction)

    @property
    def subrays(self):
        return len(self.offsets)

    @property
    def min_count(self):
        return max(1, int(math.ceil(self.min_fraction * self.subrays)))

    def struct(self):
        b = LrcBeam()
        b.subrays, b.max_echoes, b.min_count, b.separation = self.subrays, self.max_echoes, self.min_count, self.separation
        return b

    def reduce(self, t):
        """The reduction alone, on the host (lrc_echo_reduce): ``t`` (B, K) float32 closest-hit distances of B beams, +inf for a
        sub-ray without a hit -> (rep (B, E) int32: the representative sub-ray of each echo, -1 for an empty slot;
        weight (B, E) uint8: its member count)."""
        return reduce(t, self.struct())

    def __repr__(self):
        return (f"BeamModel(divergence={self.divergence!r}, pattern={self.pattern!r}, K={self.subrays}, "
                f"max_echoes={self.max_echoes}, separation={self.separation!r}, min_count={self.min_count})")


def reduce(t, beam):
    """lrc_echo_reduce on (B, K) float32 distances with an ``LrcBeam``: (rep (B, E) int32, weight (B, E) uint8)."""
    lib = _capi.load()
    t = np.ascontiguousarray(t, dtype=np.float32)
    K, E = int(beam.subrays), int(beam.max_echoes)
    if t.ndim != 2 or (1 <= K <= 16 and t.shape[1] != K):
        raise ValueError("t must be (B, K)")
    B = t.shape[0]
    rep = np.full((B, max(E, 1)), -1, np.int32)
    weight = np.zeros((B, max(E, 1)), np.uint8)
    check(lib.lrc_echo_reduce(t.ctypes.data, B, C.byref(beam), rep.ctypes.data, weight.ctypes.data), "lrc_echo_reduce")
    return rep, weight


def reduce_lanes_dev(ctx, t, beam, stream=0):
    """The DEVICE reduction alone (test hook lrc_internal_echo_lanes_dev): the lanes of the trace kernel's tail on (B, K) float32
    distances with an ``LrcBeam``, sub-ray k of beam b entering with slot k and label b * K + k.  Dict of (B, E) arrays:
    ``rep`` int32 (-1: empty slot), ``range`` float32 (+inf), ``label`` uint32 (b * K + rep; not specified for an empty slot),
    ``weight`` uint8.  ``ctx`` a ``lidarcast.Context``."""
    import torch
    t = np.ascontiguousarray(t, dtype=np.float32)
    K, E = int(beam.subrays), int(beam.max_echoes)
    if t.ndim != 2 or (1 <= K <= 16 and t.shape[1] != K):
        raise ValueError("t must be (B, K)")
    B = t.shape[0]
    dev = torch.device("cuda", ctx.device)
    t_t = torch.from_numpy(t).to(dev)
    rep, label = (torch.full((B, max(E, 1)), fill, dtype=torch.int32, device=dev) for fill in (-2, -2))
    rng = torch.full((B, max(E, 1)), float("nan"), dtype=torch.float32, device=dev)
    weight = torch.full((B, max(E, 1)), 255, dtype=torch.uint8, device=dev)
    check(ctx._lib.lrc_internal_echo_lanes_dev(ctx._h, t_t.data_ptr(), B, C.byref(beam), rep.data_ptr(), rng.data_ptr(),
                                               label.data_ptr(), weight.data_ptr(), C.c_void_p(int(stream))),
          "lrc_internal_echo_lanes_dev")
    torch.cuda.synchronize(dev)
    return {"rep": rep.cpu().numpy(), "range": rng.cpu().numpy(), "label": label.cpu().numpy().view(np.uint32),
            "weight": weight.cpu().numpy()}
