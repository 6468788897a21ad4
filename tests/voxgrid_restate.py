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


def limits(o, e, origin, s, dims):
    """The limits of the walk for the segments o[r] -> e[r] ((R, 3) float32 each).  Returns (ok (R,) bool: not rejected,
    a, b (R, 3) int64 voxels of o and e, zeros where refused, n (R, 3) int64 steps per axis, zeros where rejected)."""
    ov = np.asarray(o, np.float32).reshape(-1, 3).astype(np.float64)
    ev = np.asarray(e, np.float32).reshape(-1, 3).astype(np.float64)
    ok = np.isfinite(ov).all(1) & np.isfinite(ev).all(1)
    with np.errstate(all="ignore"):
        fa, fb = voxel_of(ov, origin, s), voxel_of(ev, origin, s)
    ok &= np.all((fa >= -COORD_LIMIT) & (fa < COORD_LIMIT) & (fb >= -COORD_LIMIT) & (fb < COORD_LIMIT), axis=1)
    a = np.where(ok[:, None], fa, 0).astype(np.int64)
    b = np.where(ok[:, None], fb, 0).astype(np.int64)
    n = np.abs(b - a)
    ok &= n.sum(1) < MAX_STEPS
    n[~ok] = 0
    return ok, a, b, n


def walk(o, e, origin, s, dims):
    """Walk the segments o[r] -> e[r] ((R, 3) float32 each).  Returns (free (V,) bool, end (R, 3) int64 = b,
    ok (R,) bool: not rejected, visited (R,) int64 voxel counts)."""
    o32 = np.asarray(o, np.float32).reshape(-1, 3)
    e32 = np.asarray(e, np.float32).reshape(-1, 3)
    dims = tuple(int(x) for x in dims)
    V = dims[0] * dims[1] * dims[2]
    free = np.zeros(V, bool)
    ov, ev = o32.astype(np.float64), e32.astype(np.float64)
    ok, a, b, n = limits(o32, e32, origin, s, dims)
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


# ---- the hostile ray set of the static grid's edge tests ------------------------------------------------------------
# walk_kernel takes (poses, dirs, t), not segments: the set is built as pose rows of RAYS_PER_POSE rays over small
# direction tables, one block per table, and the segments the device must form from them are restated here.

RAYS_PER_POSE = 7                                    # gid / N with an N that is no power of two
# Dyadic origin and voxel size; every diagonal voxel centre and every end point reached from one lies, on all three
# axes, in the float32 binade [16, 32): o + h*t rounds on the same grid of 2^-19 on x, y and z, so equal |h*t| give
# equal |e - o|.  The negative x origin keeps o.x + 2^24 voxels below 2^22, where float32 still resolves one voxel.
HOSTILE_ORIGIN, HOSTILE_S = (-24.0, 20.25, 19.5), 0.25
HOSTILE_DIMS = ((5, 7, 33), (1, 1, 1), (1, 1, 31), (4, 8, 32), (3, 11, 31))
AXIS_TABLE = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0]], np.float64)
TIE_TABLE_A = np.array([[1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1], [-1, -1, 1], [1, -1, -1], [-1, 1, -1]], np.float64)
TIE_TABLE_B = np.array([[-1, -1, -1], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [1, 1, 1], [-1, 1, 0]], np.float64)
TIE_KINDS_B = ("tie3", "tie2", "tie2", "tie2", "tie2", "tie3", "tie2")
REJECTED_KINDS = ("rej_e", "rej_o", "rej_coord", "rej_len")
# (voxel: "first" / "mid" / "last", the (sem, ins) of its returns, two per pose).  Counted on the label block alone:
#   first  sem 5, 3 and 0xFFFF with two returns each: a three-way tie -> 3; its ins 0xFFFF and 0 tie -> 0
#   mid    sem 0 and 0xFFFF with three returns each: a two-way tie -> 0; ins 0xFFFF (2) beats 0 (1)
#   last   sem 2 four times (ins 1, 2, 3, 4), sem 7 twice (ins 9, 9): sem 2, ins 1 -- the most frequent ins overall is the
#          loser's 9
LABEL_SCENES = (("first", ((5, 1), (5, 2), (3, 0xFFFF), (3, 0), (0xFFFF, 7), (0xFFFF, 7))),
                ("mid", ((0, 0xFFFF), (0, 0xFFFF), (0xFFFF, 0), (0xFFFF, 0), (0xFFFF, 0xFFFF), (0, 0))),
                ("last", ((2, 1), (2, 2), (2, 3), (7, 9), (7, 9), (2, 4))))


def segments_of(poses, dirs, t):
    """(o, e) float32 (P*N, 3) of a pose-batched scan with IDENTITY rotations: gen_ray's fma chain then gives d =
    float32(dirs[i]) exactly, o = float32(translation), and hit_point is float32 with one rounding per operation:
    h = d / sqrt((dx*dx + dy*dy) + dz*dz), e = o + h*t."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    assert (poses[:, :3, :3] == np.eye(3)).all()
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    P, N = len(poses), len(dirs)
    with np.errstate(all="ignore"):
        o = np.repeat(poses[:, :3, 3].astype(np.float32), N, axis=0)
        d = np.tile(dirs.astype(np.float32), (P, 1))
        nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        h = d / nrm[:, None]
        e = o + h * np.asarray(t, np.float32).reshape(-1, 1)
    assert o.dtype == np.float32 and e.dtype == np.float32
    return o, e


def t_reaching(ox, ex):
    """The float32 t with float32(ox + t) == ex for a ray along +x (h.x = 1)."""
    assert float(np.float32(ox)) == ox and float(np.float32(ex)) == ex
    ox, ex = np.float32(ox), np.float32(ex)
    t = np.float32(ex - ox)
    for _ in range(8):
        got = np.float32(ox + t)
        if got == ex:
            return float(t)
        t = np.nextafter(t, np.float32(np.inf if got < ex else -np.inf))
    raise AssertionError((ox, ex))


def _block(dirs):
    return {"dirs": np.asarray(dirs, np.float64), "c": [], "t": [], "sem": [], "ins": [], "kind": []}


def _row(b, c, t, sem, ins, kind):
    """One pose: translation c and RAYS_PER_POSE entries of t, sem, ins, kind (scalars are repeated).  A ray without a
    return is of kind "miss" whatever its row was meant for."""
    n = RAYS_PER_POSE
    t = np.broadcast_to(np.asarray(t, np.float64), (n,)).astype(np.float32)
    kind = np.broadcast_to(np.asarray(kind, dtype="U12"), (n,)).copy()
    kind[np.isinf(t)] = "miss"
    b["c"].append(np.asarray(c, np.float64))
    b["t"].append(t)
    b["sem"].append(np.broadcast_to(np.asarray(sem, np.uint32), (n,)))
    b["ins"].append(np.broadcast_to(np.asarray(ins, np.uint32), (n,)))
    b["kind"].append(kind)


def _finish(b):
    P = len(b["c"])
    poses = np.tile(np.eye(4), (P, 1, 1))
    poses[:, :3, 3] = np.stack(b["c"])
    t = np.concatenate(b["t"])
    tl = np.zeros((len(t), 2), np.uint32)
    tl[:, 0] = t.view(np.uint32)
    tl[:, 1] = np.concatenate(b["sem"]) | (np.concatenate(b["ins"]) << 16)
    o, e = segments_of(poses, b["dirs"], t)
    return {"poses": poses, "dirs": b["dirs"], "t_label": tl, "t": t, "kind": np.concatenate(b["kind"]), "o": o, "e": e}


def label_voxels(dims):
    d = np.asarray(dims, np.int64)
    return {"first": np.zeros(3, np.int64), "mid": d // 2, "last": d - 1}


def hostile_rays(origin, s, dims, seed=11):
    """The hostile ray set of the static grid on one grid: a list of blocks, one per direction table, each a dict of
    poses (P, 4, 4), dirs (7, 3), t_label (P*7, 2) uint32, t (P*7,) float32, kind (P*7,) and the restated segments o, e
    (P*7, 3) float32.  Block order: two random blocks, far outside starts, the axis block (misses, the four kinds of
    rejected ray, no walk at all, the 2^24 boundary pair, axis-parallel rays), two tie blocks, the label block.  In the
    axis block rays 0..63 are all misses, rays 64..127 all rejected, and the waves behind them are mixed."""
    rng = np.random.default_rng(seed)
    n = RAYS_PER_POSE
    g = np.asarray(origin, np.float64)
    d = np.asarray(dims, np.int64)
    ext = d * s
    centre = g + 0.5 * ext
    diag = float(np.linalg.norm(ext))
    inf = np.inf

    def labels():
        return rng.integers(0, 3, n), rng.integers(0, 3, n)

    blocks = []
    # random rays in and around the grid
    for _ in range(2):
        b = _block(rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1)))
        for _ in range(8):
            t = rng.uniform(0.0, 1.5 * diag, n)
            t[rng.random(n) < 0.15] = inf
            _row(b, g + rng.uniform(-0.2, 1.2, 3) * ext, t, *labels(), "random")
        blocks.append(_finish(b))
    # far outside starts, 2 to 3 extents from the grid: row p % 7 is aimed at the grid (it enters or crosses), the
    # other rows miss it
    b = _block(TIE_TABLE_A * ext * rng.uniform(0.93, 1.07, (n, 3)))
    for p in range(21):
        k = rng.uniform(2.5, 3.5)
        _row(b, centre - k * ext * TIE_TABLE_A[p % n], k * diag * rng.uniform(0.8, 1.5, n), *labels(), "far")
    blocks.append(_finish(b))
    # the axis block
    b = _block(AXIS_TABLE)
    inner = g + (np.minimum(d - 1, (1, 2, 3)) + 0.5) * s          # a voxel centre in the grid
    big = 3.0e9 * s                                                # a voxel coordinate past 2^31
    for _ in range(9):
        _row(b, inner, inf, 0, 0, "miss")                          # rays 0..62
    _row(b, inner, [inf] + [big] * 6, *labels(), "rej_coord")      # ray 63 a miss, 64..69 rejected
    c = inner.copy()
    c[0] = 3.0e38                                                  # e.x overflows along +x; elsewhere o.x itself is too far
    for _ in range(2):
        _row(b, c, 3.0e38, *labels(), ["rej_e"] + ["rej_coord"] * 5 + ["rej_e"])
    c = inner.copy()
    c[1] = 1.0e39                                                  # narrows to float32 infinity
    for _ in range(2):
        _row(b, c, 1.0, *labels(), "rej_o")
    edge = g + (np.array([d[0] - 1, min(d[1] - 1, 2), min(d[2] - 1, 3)]) + (0.0, 0.5, 0.5)) * s   # lower x face of the last x voxel
    t_rej = t_reaching(edge[0], edge[0] + 2.0 ** 24 * s)           # Manhattan length exactly 2^24: rejected
    t_ok = t_reaching(edge[0], edge[0] + (2.0 ** 24 - 1.0) * s)    # 2^24 - 1: accepted, leaves the grid at once
    for _ in range(2):
        _row(b, edge, [t_rej] + [big] * 5 + [t_rej], *labels(), ["rej_len"] + ["rej_coord"] * 5 + ["rej_len"])
    for _ in range(3):
        _row(b, inner, big, *labels(), "rej_coord")                # rays 112..132: wave 1 (64..127) holds rejected rays only
    start = edge.copy()
    start[0] = g[0] + max(d[0] - 3, 0) * s                         # a row of up to three voxels to the +x face
    for c in (edge, start):
        t = rng.uniform(0.0, 1.3, n) * ext[[0, 0, 1, 1, 2, 2, 0]]
        t[0], t[6] = t_reaching(c[0], c[0] + (2.0 ** 24 - 1.0) * s), t_rej if c is edge else t[6]
        _row(b, c, t, *labels(), ["len_ok"] + ["axis"] * 5 + ["rej_len" if c is edge else "axis"])
    _row(b, inner, 0.0, *labels(), "nowalk_zero")                  # t = +0.0 is finite: a return, e == o
    _row(b, inner, 2.0 ** -20, *labels(), "nowalk_tiny")
    _row(b, inner, 0.25 * s, *labels(), "nowalk_voxel")            # ends in the start voxel
    for _ in range(8):
        t = rng.uniform(0.0, 1.3, n) * ext[[0, 0, 1, 1, 2, 2, 0]]
        t[rng.random(n) < 0.15] = inf
        _row(b, g + rng.uniform(-0.3, 1.3, 3) * ext, t, *labels(), "axis")
    blocks.append(_finish(b))
    # exact ties: poses at voxel centres of the main diagonal (the same index on all three axes, also just outside the
    # grid), dirs (+-1, +-1, +-1) and (+-1, +-1, 0); each component moves k voxels
    m = int(d.min())
    for table, kinds in ((TIE_TABLE_A, ("tie3",) * n), (TIE_TABLE_B, TIE_KINDS_B)):
        b = _block(table)
        length = np.sqrt((table * table).sum(1))
        for i in sorted({-1, 0, m // 2, m - 1, m}):
            for _ in range(2):
                k = rng.choice([0.7, 1.0, 1.5, 2.0, 2.5, 3.0], n)
                _row(b, g + (i + 0.5) * s, k * s * length, *labels(), kinds)
        blocks.append(_finish(b))
    # hostile labels: two +x rays per pose from the centre of the -x neighbour into the centre of the voxel
    b = _block(AXIS_TABLE)
    vox = label_voxels(dims)
    for name, pairs in LABEL_SCENES:
        c = g + (vox[name] + (-0.5, 0.5, 0.5)) * s
        for j in range(0, len(pairs), 2):
            (s0, i0), (s1, i1) = pairs[j], pairs[j + 1]
            _row(b, c, [s] + [inf] * 5 + [s], [s0] + [0] * 5 + [s1], [i0] + [0] * 5 + [i1], "label")
    blocks.append(_finish(b))
    return blocks


def returned_segments(blocks):
    """(o, e, labels) of the returned rays (finite t) of some blocks, in ray order."""
    keep = [np.isfinite(b["t"]) for b in blocks]
    return (np.concatenate([b["o"][k] for b, k in zip(blocks, keep)]),
            np.concatenate([b["e"][k] for b, k in zip(blocks, keep)]),
            np.concatenate([b["t_label"][k, 1] for b, k in zip(blocks, keep)]))


def launch_edge_rays(origin, s, dims, total=257, seed=3):
    """One pose at the centre of voxel (0, 0, 0) with a table of ``total`` rows: the axis and tie directions, then
    random ones; misses, rejected rays and t = 0 in between.  Prefixes [:n] of (dirs, t_label) are the launch edges.
    Returns (poses (1, 4, 4), dirs (total, 3), t_label (total, 2))."""
    rng = np.random.default_rng(seed)
    g = np.asarray(origin, np.float64)
    ext = np.asarray(dims, np.int64) * s
    special = np.concatenate([AXIS_TABLE[:6], TIE_TABLE_A, TIE_TABLE_B[:5]])
    dirs = rng.normal(size=(total, 3)) * rng.uniform(0.5, 2.0, (total, 1))
    dirs[:len(special)] = special[:total]
    t = rng.uniform(0.0, 1.2 * float(np.linalg.norm(ext)), total).astype(np.float32)
    u = rng.random(total)
    t[u < 0.1] = np.inf
    t[(u >= 0.1) & (u < 0.15)] = np.float32(3.0e9 * s)
    t[(u >= 0.15) & (u < 0.18)] = 0.0
    t[0] = np.float32(1.5 * s)                                   # a launch of one ray carves and returns
    tl = np.zeros((total, 2), np.uint32)
    tl[:, 0] = t.view(np.uint32)
    tl[:, 1] = rng.integers(0, 3, total).astype(np.uint32) | (rng.integers(0, 3, total).astype(np.uint32) << 16)
    pose = np.eye(4)
    pose[:3, 3] = g + 0.5 * s
    return pose[None], dirs, tl


def walk_long(o, e, origin, s, dims, long_steps=1 << 16):
    """walk() for a set that holds a few accepted rays too long to walk step by step (up to 2^24 - 1 steps).  Such a
    ray must be axis-parallel; its walk is then the row of voxels from a to b whatever the arithmetic, written here
    directly: every voxel of the row but b that lies in the grid is free, and b is the end."""
    o32 = np.asarray(o, np.float32).reshape(-1, 3)
    e32 = np.asarray(e, np.float32).reshape(-1, 3)
    dims = tuple(int(x) for x in dims)
    ok, a, b, n = limits(o32, e32, origin, s, dims)
    long = ok & (n.sum(1) >= long_steps)
    free, _, ok_short, _ = walk(o32[~long], e32[~long], origin, s, dims)
    assert np.array_equal(ok_short, ok[~long])
    for r in np.flatnonzero(long):
        ax = np.flatnonzero(n[r])
        assert len(ax) == 1, "a long ray must be axis-parallel"
        ax = int(ax[0])
        if all(0 <= a[r, x] < dims[x] for x in range(3) if x != ax):
            step = 1 if b[r, ax] > a[r, ax] else -1
            lo, hi = (a[r, ax], min(b[r, ax], dims[ax])) if step > 0 else (max(b[r, ax] + 1, 0), a[r, ax] + 1)
            for i in range(max(lo, 0), min(hi, dims[ax])):
                c = a[r].copy()
                c[ax] = i
                free[linear(c, dims)] = True
    return free, b, ok, np.where(ok, n.sum(1) + 1, 0)


def grid_from_rays_long(o, e, labels, origin, s, dims, min_returns=1):
    """grid_from_rays over walk_long."""
    free, end, ok, _ = walk_long(o, e, origin, s, dims)
    i, se, ins = keys_of(end, ok, labels, dims)
    sparse, state, counts = finalize(free, i, se, ins, dims, min_returns)
    counts["rejected_rays"] = int((~ok).sum())
    return sparse, state, counts


def growth_rays(origin, s, dims, poses=90, seed=5):
    """One block of ``poses`` poses over one random table for the key buffer's growth paths: random rays in and around the
    grid, misses and a few rejected rays.  Chunks of it are slices of whole poses (chunk())."""
    rng = np.random.default_rng(seed)
    n = RAYS_PER_POSE
    g = np.asarray(origin, np.float64)
    ext = np.asarray(dims, np.int64) * s
    b = _block(rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1)))
    for _ in range(poses):
        t = rng.uniform(0.0, 1.0, n) ** 3 * 0.8 * float(np.linalg.norm(ext))      # mostly short: returns pile up
        u = rng.random(n)
        t[u < 0.15] = np.inf
        t[(u >= 0.15) & (u < 0.2)] = 3.0e9 * s
        _row(b, g + rng.uniform(-0.1, 1.1, 3) * ext, t, rng.integers(0, 3, n), rng.integers(0, 3, n), "random")
    return _finish(b)


def chunk(block, p0, p1):
    """Poses [p0, p1) of a block, as a block."""
    n = RAYS_PER_POSE
    out = {k: block[k][p0 * n:p1 * n] for k in ("t_label", "t", "kind", "o", "e")}
    out["poses"], out["dirs"] = block["poses"][p0:p1], block["dirs"]
    return out
