"""numpy restatement of the noisy moving-sensor sweep rays (include/lidarcast.h "noisy moving-sensor sweeps", csrc/lrc_device.h
gen_ray_noisy_sweep): the composition of tests/noise_restate.py and tests/sweep_restate.py, nothing of its own.  Per sweep k the
table rows are jittered with the draws of frame first_frame + k (noise_restate.jitter_rows), the jittered rows go through
sweep_restate.sweep_rays with record k alone, dropped rays get a NaN direction, and the range term is float32(range_std) * z."""
import numpy as np

import noise_restate as nr
from sweep_restate import sweep_rays


def noisy_sweep_rays(motion, dirs, fire, model, base, slope):
    """(rays (P*N, 6) float32 with a NaN direction for a dropped ray, centres (P*N, 3) float64, range term (P*N,) float32, keep
    (P*N,) bool, rows (P, N, 3) float64 as rotated) of ``model`` (a lidarcast.noise.NoiseModel) over the sweeps ``motion``."""
    motion = np.asarray(motion, dtype=np.float64).reshape(-1, 24)
    dirs = np.asarray(dirs, dtype=np.float64)
    P, N = len(motion), len(dirs)
    d = nr.draws(model.seed, model.first_frame, P, N, model.dropout, base, slope)
    sa = np.float64(model.angle_std)
    rays = np.empty((P, N, 6), np.float32)
    cen = np.empty((P, N, 3))
    rows = np.empty((P, N, 3))
    for k in range(P):
        rows[k] = dirs if model.angle_std == 0 else nr.jitter_rows(dirs, sa * d["z_az"][k].astype(np.float64),
                                                                  sa * d["z_el"][k].astype(np.float64))
        rays[k], cen[k] = sweep_rays(motion[k:k + 1], rows[k], fire)
    keep = d["keep"] if model.dropout != 0 else np.ones((P, N), bool)
    rays[~keep, 3:] = np.nan
    term = np.float32(model.range_std) * d["z_range"] if model.range_std != 0 else np.zeros((P, N), np.float32)
    return rays.reshape(P * N, 6), cen.reshape(P * N, 3), term.reshape(-1).astype(np.float32), keep.reshape(-1), rows
