"""numpy restatement of the seeded sensor noise under movers of lrc_scan_noisy_movers_* (include/lidarcast.h "seeded sensor
noise under movers").  Written from the header's text out of the two restatements it composes: tests/noise_restate.py gives the
jittered rays, the filter centres, the range term and the keep mask; tests/mover_restate.py takes the kept rays into every
mover's frame and merges the casts on the CLEAN ranges.  Then t' = t + term as one float32 add, t' <= 0 is a miss, and
mover_restate.record assembles the record at t'.  It takes any "cast these rays" function, as mover_restate does."""
import numpy as np

import mover_restate as mv
import noise_restate as nr

F32 = np.float32


def table():
    """The (24, 64) quantile table in use, base and slope."""
    from lidarcast.noise import table as t
    return t()


def _miss(n):
    return {"t": np.full(n, np.inf, F32), "prim": np.full(n, mv.INVALID, np.uint32), "sem": np.zeros(n, np.uint16),
            "ins": np.zeros(n, np.uint16), "normal3": np.zeros((n, 3), F32)}


def cast_kept(cast, rays, keep):
    """``cast`` on the rays of ``keep`` only; every other ray is a miss (never cast)."""
    out = _miss(len(rays))
    if keep.any():
        got = cast(np.ascontiguousarray(rays[keep], F32))
        for a in out:
            out[a][keep] = np.asarray(got[a]).astype(out[a].dtype)
    return out


def scan(cast_static, cast_movers, poses, dirs, mover_poses12, model, max_range, min_range=0.0, incident_mode=0, tab=None):
    """P poses (P, 4, 4) of the table ``dirs`` (N, 3) under ``model`` (a lidarcast.noise.NoiseModel; pose p is frame
    model.first_frame + p), M movers given by their cast functions and ``mover_poses12`` (P, M, 12).  Returns (record dict over
    all P * N rays, winners dict on the clean ranges before any filter, info dict: rays, centres, term, keep)."""
    base, slope = table() if tab is None else tab
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    P, N, M = len(poses), len(dirs), len(cast_movers)
    rays, cen, term, keep, _ = nr.noisy_rays(poses, dirs, model.seed, model.first_frame, model.range_std, model.angle_std,
                                             model.dropout, base, slope)
    mp = np.asarray(mover_poses12, F32).reshape(P, M, 12) if M else np.zeros((P, 0, 12), F32)
    wins = []
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        r, k = rays[sl], keep[sl]
        static = cast_kept(cast_static, r, k)                           # 1: a dropped ray is cast against nothing
        movers = [cast_kept(c, mv.to_object(np.where(k[:, None], r, F32(0)), mp[p, m]), k) for m, c in enumerate(cast_movers)]
        wins.append(mv.merge(static, movers, mp[p]))                    # 3: the winner on the clean ranges
    win = {a: np.concatenate([w[a] for w in wins]) for a in wins[0]}
    noisy = dict(win)
    with np.errstate(invalid="ignore"):
        t = (win["t"] + term).astype(F32) if model.range_std != 0 else win["t"].copy()       # 4: one float32 add (inf stays inf)
    t[~(t > 0)] = np.inf                                                 # t' <= 0 is no return
    noisy["t"] = t
    safe = np.where(keep[:, None], rays, F32(1))                         # a dropped ray's NaN direction never reaches a record
    rec = mv.record(noisy, safe, np.repeat(cen, N, axis=0), max_range, min_range, incident_mode)
    return rec, win, {"rays": rays, "centres": np.repeat(cen, N, axis=0), "term": term, "keep": keep}
