"""Seeded sensor noise drawn on the GPU (include/lidarcast.h "seeded sensor noise").

``NoiseModel`` names the three sensor parameters the multi-line sensor records declare -- range noise, angle jitter,
dropout -- plus a seed and the frame id of the first pose of a call.  The noise of ray i of pose p is a pure function of
(seed, first_frame + p, i): ``Scene.scan_noisy_dev`` / ``Scene.scan_noisy_compact`` draw it in the trace kernel, and
``draws`` evaluates the same integers and float32 operations on the host, without a GPU.
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
