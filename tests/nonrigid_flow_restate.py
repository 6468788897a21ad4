"""numpy restatement of the non-rigid scene flow of lrc_scan_nonrigid_flow_dev (include/lidarcast.h "non-rigid scene flow").
Written from the header's text, not from csrc/lrc_flow.h: the tests compare the two.  It stands on tests/flow_restate.py (the
rigid target, the verdict, the casts of finite rays) and tests/mover_restate.py (rays into a mover's frame), and like them takes
any "cast these rays" function.  A surface pair here is (m, VA (V, 3) float32, VB (V, 3) float32, tris3 (T, 3))."""
import numpy as np

import flow_restate as fl
import mover_restate as mv

F32, F64 = np.float32, np.float64


def dot(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]


def rest(x, A):
    """step 1: q = R_A^T (x - c_A), float64, the expressions of the rigid target"""
    x, A = x.astype(F64), A.astype(F64).reshape(-1, 3, 4)
    e = x - A[:, :, 3]
    q = np.empty_like(e)
    for j in range(3):
        q[:, j] = (A[:, 0, j] * e[:, 0] + A[:, 1, j] * e[:, 1]) + A[:, 2, j] * e[:, 2]
    return q


def world(z, B):
    """step 9: y = R_B z + c_B"""
    B = B.astype(F64).reshape(-1, 3, 4)
    y = np.empty_like(z)
    for j in range(3):
        y[:, j] = ((B[:, j, 0] * z[:, 0] + B[:, j, 1] * z[:, 1]) + B[:, j, 2] * z[:, 2]) + B[:, j, 3]
    return y


def barycentric(q, a):
    """steps 3 to 7: (s, u, v) of q (n, 3) float64 in the triangles a (n, 3 vertices, 3) float64; u = v = 0 unless den > 0"""
    e1, e2, r = a[:, 1] - a[:, 0], a[:, 2] - a[:, 0], q - a[:, 0]
    d11, d12, d22, r1, r2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(r, e1), dot(r, e2)
    den = d11 * d22 - d12 * d12
    ok = den > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(ok, (d22 * r1 - d12 * r2) / den, 0.0)
        v = np.where(ok, (d11 * r2 - d12 * r1) / den, 0.0)
    return (1.0 - u) - v, u, v


def displaced(q, va, vb):
    """steps 2 to 8: va, vb (n, 3 vertices, 3) float32.  Returns (z, bent): z = q, the same bits, where no D differs from 0."""
    a = va.astype(F64)
    s, u, v = barycentric(q, a)
    D = vb.astype(F64) - a
    bent = (D != 0.0).any(axis=(1, 2))
    z = q + ((s[:, None] * D[:, 0] + u[:, None] * D[:, 1]) + v[:, None] * D[:, 2])
    return np.where(bent[:, None], z, q), bent


def rays(t, point3, mover, prim, A, B, next_poses, has_next, N, max_range, pairs, min_range=0.0):
    """steps 1 to 10 and the steps of the scene flow from y on, for P frames of N rows; the dict of flow_restate.rays plus
    ``paired`` (the rows that had a pair) and ``y`` (float64)."""
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
    j = np.asarray(prim).reshape(n).view(np.uint32).astype(np.int64) if prim is not None else np.zeros(n, np.int64)
    y = x.astype(F64)
    own = live & (w > 0) & (w <= M)
    paired = np.zeros(n, bool)
    if own.any():
        Aall, Ball = np.asarray(A, F32).reshape(P, M, 12), np.asarray(B, F32).reshape(P, M, 12)
        for m, va, vb, tris in pairs:
            tris = np.asarray(tris).astype(np.int64).reshape(-1, 3)
            rows = np.flatnonzero(own & (w == m + 1) & (j < len(tris)))
            if not len(rows):
                continue
            paired[rows] = True
            Ar, Br = Aall[frame[rows], m], Ball[frame[rows], m]
            q = rest(x[rows], Ar)
            idx = tris[j[rows]]
            z, bent = displaced(q, np.asarray(va, F32)[idx], np.asarray(vb, F32)[idx])
            differ = (Ar.view(np.uint32) != Br.view(np.uint32)).any(axis=1)
            go = bent | differ                                                  # step 10
            y[rows[go]] = world(z[go], Br[go])
        rigid = np.flatnonzero(own & ~paired)
        if len(rigid):
            Ar, Br = Aall[frame[rigid], w[rigid] - 1], Ball[frame[rigid], w[rigid] - 1]
            differ = (Ar.view(np.uint32) != Br.view(np.uint32)).any(axis=1)
            y[rigid[differ]] = fl.target(x[rigid[differ]], Ar[differ], Br[differ])
    flow = np.where(live[:, None], (y - x.astype(F64)).astype(F32), F32(0))
    flow[~live] = F32(0)
    y32 = y.astype(F32)
    c = nxt[frame, :3, 3]
    o = c.astype(F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = y32 - o
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        h = d / L[:, None]
        thr = L - fl.MARGIN * np.maximum(L, F32(1))
        e = y32.astype(F64) - c
        dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    inside = dist < max_range
    if min_range > 0.0:
        inside &= dist >= min_range
    status = np.where(live, np.where(inside, fl.VISIBLE, fl.OUT_OF_RANGE), fl.NONE).astype(np.uint8)
    keep = status == fl.VISIBLE
    rays6 = np.where(keep[:, None], np.concatenate([o, h], axis=1), F32(0)).astype(F32)
    return {"flow3": flow.astype(F32), "rays6": rays6, "keep": keep.astype(np.uint8), "thr": np.where(keep, thr, F32(0)).astype(F32),
            "L": np.where(keep, L, F32(0)).astype(F32), "status": status, "paired": paired, "y": y}


def scan(cast_static, cast_movers, t, point3, mover, prim, A, B, next_poses, has_next, N, max_range, pairs, min_range=0.0):
    """The whole of lrc_scan_nonrigid_flow_dev for P frames: (flow3, status, details) as flow_restate.scan returns them.
    ``cast_movers`` cast on the movers' scenes AS THEY STAND at the next frame (the next shape for a deformable)."""
    r = rays(t, point3, mover, prim, A, B, next_poses, has_next, N, max_range, pairs, min_range)
    n = len(r["keep"])
    P = n // N
    M = len(cast_movers)
    ts = np.full(n, np.inf, F32)
    tm = np.full((M, n), np.inf, F32)
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        ts[sl] = fl.cast_finite(cast_static, r["rays6"][sl], r["keep"][sl])
        for m, cast in enumerate(cast_movers):
            tm[m, sl] = fl.cast_finite(cast, mv.to_object(r["rays6"][sl], np.asarray(B, F32).reshape(P, M, 12)[p, m]), r["keep"][sl])
    status, t_min = fl.judge(ts, tm, r["thr"], r["status"])
    r.update(t_static=ts, t_movers=tm, t_min=t_min)
    return r["flow3"], status, r
