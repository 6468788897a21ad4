"""numpy restatement of the scene flow under movers of lrc_scan_flow_* (include/lidarcast.h "scene flow").  Written from the
header's text, not from csrc/lrc_flow.h: the tests compare the two.  Like tests/mover_restate.py it takes any "cast these rays"
function -- the CPU oracle on the host, the explicit-ray cast on the GPU -- that maps (n, 6) float32 rays to a dict with the
per-ray t (+inf: a miss), nothing filtered and nothing culled."""
import numpy as np

import mover_restate as mv

F32, F64 = np.float32, np.float64
NONE, VISIBLE, OCCLUDED, OUT_OF_RANGE = 0, 1, 2, 3
MARGIN = F32(2.0 ** -12)


def target(x, A, B):
    """step 1 for rows that moved: x (n, 3) float32, A and B (n, 12) float32, the row's own pose pair.  float64, one rounding per
    operation: e = x - c_A, q = R_A^T e, y = R_B q + c_B in the header's order of additions."""
    x, A, B = x.astype(F64), A.astype(F64).reshape(-1, 3, 4), B.astype(F64).reshape(-1, 3, 4)
    e = x - A[:, :, 3]
    q = np.empty_like(e)
    y = np.empty_like(e)
    for j in range(3):
        q[:, j] = (A[:, 0, j] * e[:, 0] + A[:, 1, j] * e[:, 1]) + A[:, 2, j] * e[:, 2]
    for j in range(3):
        y[:, j] = ((B[:, j, 0] * q[:, 0] + B[:, j, 1] * q[:, 1]) + B[:, j, 2] * q[:, 2]) + B[:, j, 3]
    return y


def rays(t, point3, mover, A, B, next_poses, has_next, N, max_range, min_range=0.0):
    """steps 1 to 3 and 6 for P frames of N rows: t (P * N,), point3 (P * N, 3), mover (P * N,) uint8 or None, A / B (P, M, 12) or
    None, next_poses (P, 4, 4) float64, has_next (P,) or None.  Returns flow3, rays6 (o, h), keep, thr, L and the status so far
    (0, 3, or 1 for a row to be cast); ray, thr and L of a row that is not cast are zero."""
    t = np.asarray(t, F32).reshape(-1)
    n = len(t)
    P = n // N
    x = np.asarray(point3, F32).reshape(n, 3)
    nxt = np.asarray(next_poses, F64).reshape(P, 4, 4)
    frame = np.repeat(np.arange(P), N)
    live = t < np.inf
    if has_next is not None:
        live &= np.asarray(has_next).reshape(P)[frame] != 0
    M = 0 if A is None else np.asarray(A).shape[1]
    w = np.zeros(n, np.int64) if (mover is None or M == 0) else np.asarray(mover).astype(np.int64).reshape(n)
    y = x.astype(F64)
    own = live & (w > 0) & (w <= M)
    if own.any():
        Ar = np.asarray(A, F32).reshape(P, M, 12)[frame[own], w[own] - 1]
        Br = np.asarray(B, F32).reshape(P, M, 12)[frame[own], w[own] - 1]
        differ = (Ar.view(np.uint32) != Br.view(np.uint32)).any(axis=1)
        idx = np.flatnonzero(own)[differ]
        y[idx] = target(x[idx], Ar[differ], Br[differ])
    flow = np.where(live[:, None], (y - x.astype(F64)).astype(F32), F32(0))
    flow[~live] = F32(0)                                                       # +0, whatever the sign of a difference would be
    y32 = y.astype(F32)
    c = nxt[frame, :3, 3]
    o = c.astype(F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = y32 - o
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        h = d / L[:, None]
        thr = L - MARGIN * np.maximum(L, F32(1))
        e = y32.astype(F64) - c
        dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    inside = dist < max_range
    if min_range > 0.0:
        inside &= dist >= min_range
    status = np.where(live, np.where(inside, VISIBLE, OUT_OF_RANGE), NONE).astype(np.uint8)
    keep = status == VISIBLE
    rays6 = np.where(keep[:, None], np.concatenate([o, h], axis=1), F32(0)).astype(F32)
    return {"flow3": flow.astype(F32), "rays6": rays6, "keep": keep.astype(np.uint8), "thr": np.where(keep, thr, F32(0)).astype(F32),
            "L": np.where(keep, L, F32(0)).astype(F32), "status": status}


def judge(t_static, t_movers, thr, status_in):
    """step 5: rows of status 1 are occluded iff the float32 minimum of the ranges is below thr; other rows keep their status."""
    t = np.asarray(t_static, F32).copy()
    for tm in ([] if t_movers is None else t_movers):
        tm = np.asarray(tm, F32)
        t = np.where(tm < t, tm, t)
    out = np.asarray(status_in, np.uint8).copy()
    cast = out == VISIBLE
    out[cast] = np.where(t[cast] < np.asarray(thr, F32)[cast], OCCLUDED, VISIBLE)
    return out, t


def cast_finite(cast, r, keep):
    """the ranges of ``cast`` for the kept rays that are finite (the finite-ray contract); +inf everywhere else"""
    t = np.full(len(r), np.inf, F32)
    ok = keep.astype(bool) & np.isfinite(r).all(axis=1)
    if ok.any():
        t[ok] = np.asarray(cast(np.ascontiguousarray(r[ok]))["t"], F32)
    return t


def scan(cast_static, cast_movers, t, point3, mover, A, B, next_poses, has_next, N, max_range, min_range=0.0):
    """The whole of lrc_scan_flow_dev for P frames: returns (flow3, status, details) with details the dict of ``rays`` plus
    t_static, t_movers (M, n) and t_min."""
    r = rays(t, point3, mover, A, B, next_poses, has_next, N, max_range, min_range)
    n = len(r["keep"])
    P = n // N
    M = len(cast_movers)
    ts = np.full(n, np.inf, F32)
    tm = np.full((M, n), np.inf, F32)
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        ts[sl] = cast_finite(cast_static, r["rays6"][sl], r["keep"][sl])
        for m, cast in enumerate(cast_movers):
            tm[m, sl] = cast_finite(cast, mv.to_object(r["rays6"][sl], np.asarray(B, F32).reshape(P, M, 12)[p, m]), r["keep"][sl])
    status, t_min = judge(ts, tm, r["thr"], r["status"])
    r.update(t_static=ts, t_movers=tm, t_min=t_min)
    return r["flow3"], status, r


def pair_next(poses, mover_poses):
    """frame k with k + 1; the last frame has none (its next entries repeat its own)"""
    poses = np.asarray(poses, F64).reshape(-1, 4, 4)
    mp = np.asarray(mover_poses, F32)
    has = np.ones(len(poses), np.uint8)
    has[-1] = 0
    return np.concatenate([poses[1:], poses[-1:]]), np.concatenate([mp[1:], mp[-1:]]), has


def three_mover_poses(P=3):
    """The layout the flow tests use for three movers: the pedestrian on its walk, the 12-triangle cube beside it at chest
    height and turning, a second pedestrian on the other side (no mover swallows the sensor in any frame)."""
    out = np.empty((P, 3, 12), F32)
    for f in range(P):
        x, y, z, yaw = mv.walker_state(f)
        out[f, 0] = mv.pose12(x, y, z, yaw)
        out[f, 1] = mv.pose12(x + 0.6, y + 0.5, 1.0, 0.3 + f)
        out[f, 2] = mv.pose12(x - 0.5, y - 0.6, 0.0, -yaw)
    return out
