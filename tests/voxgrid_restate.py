"""numpy restatement of the semantic occupancy grid (csrc/lrc_voxgrid.hip, include/lidarcast.h).

Grid.  origin g (3 float64, finite), voxel size s (float64, finite, > 0), dims (nx, ny, nz), each >= 1, nx*ny*nz <=
2^31 - 1.  The voxel of a float64 point x is i_a = floor((x_a - g_a) / s) per axis: an f64 subtract, then an f64
divide, then floor.  It is inside iff 0 <= i < n on every axis; its linear index is (i*ny + j)*nz + k, so arrays have
shape (nx, ny, nz) in C order, z fastest.

Rays.  Pose-batched static scans.  Ray (p, i) has origin o, float32 exactly as the scan forms it, and end point e, the
float32 hit point o + (d/|d|)*t: the row the scene cloud holds.  A ray contributes only if its t is finite (it
returns).  Rays without a return carve nothing.

Walk (float64, no contraction; o and e widened exactly).  a = voxel of o, b = voxel of e, D = e - o.  For each axis with
b_a != a_a: n_a = |b_a - a_a| steps, step_a = sign(b_a - a_a), tMax_a = ((g_a + (a_a + 1)*s) - o_a) / D_a stepping up,
((g_a + a_a*s) - o_a) / D_a stepping down, tDelta_a = s / |D_a|.  Axes with n_a = 0 take no part.  Visit a; then, while
any n_a > 0, take the axis with the smallest tMax among those with n_a > 0 (ties x, then y, then z), step it, tMax_a +=
tDelta_a, n_a -= 1, visit the new voxel.  The walk ends in b: 6-connected, Manhattan + 1 voxels.  Every visited voxel
except b that lies in the grid gets its free bit; b, if in the grid, gets one return with the ray's (sem, ins).  a == b
carves nothing.  Voxels outside the grid are ignored, but the walk is defined over the whole segment.  A returned ray
whose o or e is not finite, whose voxel coordinates leave [-2^31, 2^31) or whose walk has 2^24 or more steps is
rejected: it carves nothing, records no return, and is counted.

Accumulation is additive until reset: free bits are an OR, returns are integer counts.

Finalize (min_returns >= 1).  returns[v] = number of returns in v.  v is occupied iff returns[v] >= min_returns, else
free iff its free bit is set, else unknown.  sem[v] = most frequent semantic label among v's returns, ties to the
smallest; ins[v] = most frequent instance among the returns whose sem equals sem[v], ties to the smallest; both 0
without returns.  Outputs: the sparse list ascending by linear index of every voxel with >= 1 return (idx u32, sem u16,
ins u16, returns u32), the dense state u8 (0 unknown, 1 free, 2 occupied) and the counts.

Everything below is numpy float64 with one rounding per operation (numpy never fuses), vectorised over rays in lockstep
steps.
"""
import numpy as np

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
MAX_STEPS = 1 << 24
COORD_LIMIT = 2.0 ** 31


def voxel_of(x, origin, s):
    """(R, 3) float64 voxel coordinates floor((x - g) / s), still float64."""
    return np.floor((np.asarray(x, np.float64) - np.asarray(origin, np.float64)) / np.float64(s))


def linear(c, dims):
    c = np.asarray(c, np.int64)
    return (c[..., 0] * dims[1] + c[..., 1]) * dims[2] + c[..., 2]


def inside(c, dims):
    c = np.asarray(c, np.int64)
    return np.all((c >= 0) & (c < np.asarray(dims, np.int64)), axis=-1)


def walk(o, e, origin, s, dims):
    """Walk the segments o[r] -> e[r] ((R, 3) float32 each).  Returns (free (V,) bool, end (R, 3) int64 = b,
    ok (R,) bool: not rejected, visited (R,) int64 voxel counts)."""
    o32 = np.asarray(o, np.float32).reshape(-1, 3)
    e32 = np.asarray(e, np.float32).reshape(-1, 3)
    dims = tuple(int(x) for x in dims)
    V = dims[0] * dims[1] * dims[2]
    free = np.zeros(V, bool)
    R = o32.shape[0]
    ov, ev = o32.astype(np.float64), e32.astype(np.float64)
    ok = np.isfinite(ov).all(1) & np.isfinite(ev).all(1)
    with np.errstate(all="ignore"):
        fa, fb = voxel_of(ov, origin, s), voxel_of(ev, origin, s)
    ok &= np.all((fa >= -COORD_LIMIT) & (fa < COORD_LIMIT) & (fb >= -COORD_LIMIT) & (fb < COORD_LIMIT), axis=1)
    a = np.where(ok[:, None], fa, 0).astype(np.int64)
    b = np.where(ok[:, None], fb, 0).astype(np.int64)
    n = np.abs(b - a)
    ok &= n.sum(1) < MAX_STEPS
    n[~ok] = 0
    step = np.sign(b - a)
    g = np.asarray(origin, np.float64)
    sd = np.float64(s)
    with np.errstate(all="ignore"):
        D = ev - ov
        plane = g + (a.astype(np.float64) + np.where(step > 0, 1.0, 0.0)) * sd
        tmax = np.where(n > 0, (plane - ov) / D, np.inf)
        tdel = np.where(n > 0, sd / np.abs(D), np.inf)
    cur = a.copy()
    visited = np.where(ok, n.sum(1) + 1, 0)
    act = n.sum(1) > 0
    while act.any():
        idx = np.flatnonzero(act)
        c = cur[idx]
        inn = inside(c, dims)
        free[linear(c[inn], dims)] = True
        nn, tm = n[idx], tmax[idx]
        ax = (nn[:, 0] > 0) & ((nn[:, 1] == 0) | (tm[:, 0] <= tm[:, 1])) & ((nn[:, 2] == 0) | (tm[:, 0] <= tm[:, 2]))
        ay = ~ax & (nn[:, 1] > 0) & ((nn[:, 2] == 0) | (tm[:, 1] <= tm[:, 2]))
        axis = np.where(ax, 0, np.where(ay, 1, 2))
        cur[idx, axis] += step[idx, axis]
        tmax[idx, axis] = tmax[idx, axis] + tdel[idx, axis]
        n[idx, axis] -= 1
        act[idx] = n[idx].sum(1) > 0
    assert np.array_equal(cur[ok], b[ok])
    return free, b, ok, visited


def keys_of(end, ok, labels, dims):
    """Return keys (idx, sem, ins) of the rays whose end voxel is inside the grid."""
    lab = np.asarray(labels, np.uint32).reshape(-1)
    m = ok & inside(end, dims)
    return linear(end[m], dims), (lab[m] & 0xFFFF).astype(np.int64), (lab[m] >> 16).astype(np.int64)


def vote(idx, sem, ins):
    """Sparse list (idx, sem, ins, returns) from per-return keys: majority sem (ties smallest), then majority ins among
    the returns with that sem (ties smallest)."""
    if len(idx) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    order = np.lexsort((ins, sem, idx))
    idx, sem, ins = idx[order], sem[order], ins[order]
    trip = np.stack([idx, sem, ins], 1)
    ut, cnt = np.unique(trip, axis=0, return_counts=True)
    out_idx, out_sem, out_ins, out_ret = [], [], [], []
    starts = np.flatnonzero(np.r_[True, ut[1:, 0] != ut[:-1, 0]])
    ends = np.r_[starts[1:], len(ut)]
    for s0, s1 in zip(starts, ends):
        rows, c = ut[s0:s1], cnt[s0:s1]
        sems = np.unique(rows[:, 1])
        per = np.array([c[rows[:, 1] == x].sum() for x in sems])
        best = sems[np.argmax(per)]                       # argmax: first maximum = smallest label
        sel = rows[:, 1] == best
        out_idx.append(rows[0, 0])
        out_sem.append(best)
        out_ins.append(rows[sel, 2][np.argmax(c[sel])])
        out_ret.append(c.sum())
    return np.array(out_idx), np.array(out_sem), np.array(out_ins), np.array(out_ret)


def finalize(free, idx, sem, ins, dims, min_returns=1):
    """(sparse dict, state (V,) uint8, counts dict) from the free bits and the per-return keys."""
    if min_returns < 1:
        raise ValueError("min_returns must be >= 1")
    vi, vs, vn, vr = vote(np.asarray(idx, np.int64), np.asarray(sem, np.int64), np.asarray(ins, np.int64))
    V = int(np.prod(dims))
    state = np.where(free, FREE, UNKNOWN).astype(np.uint8)
    occ = vi[vr >= min_returns]
    state[occ] = OCCUPIED
    sparse = {"idx": vi.astype(np.uint32), "sem": vs.astype(np.uint16), "ins": vn.astype(np.uint16),
              "returns": vr.astype(np.uint32)}
    counts = {"free": int((state == FREE).sum()), "occupied": int((state == OCCUPIED).sum()),
              "unknown": int((state == UNKNOWN).sum()), "num_sparse": len(vi), "returns": int(vr.sum())}
    assert counts["free"] + counts["occupied"] + counts["unknown"] == V
    return sparse, state, counts


def grid_from_rays(o, e, labels, origin, s, dims, min_returns=1):
    """The whole definition over returned rays (o, e float32 (R, 3), labels uint32 sem | ins << 16)."""
    free, end, ok, _ = walk(o, e, origin, s, dims)
    i, se, ins = keys_of(end, ok, labels, dims)
    sparse, state, counts = finalize(free, i, se, ins, dims, min_returns)
    counts["rejected_rays"] = int((~ok).sum())
    return sparse, state, counts
