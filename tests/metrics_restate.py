"""numpy restatements, plain references, tolerances and case builders for the metrics kernels (csrc/lrc_metrics.hip:
min_dist_kernel, rbf_sum_kernel) and the planner's occupancy kernel (csrc/lrc_occupancy.hip).  numpy only; shared by
tests/test_metrics_restate_host.py (no GPU: the restatements against numpy and against each other, and the wrong kernel
models the cases must reject) and tests/test_metrics_edges_gpu.py / tests/test_occupancy_edges_gpu.py (the kernels).

Launch geometry the cases are built around: min_dist / rbf_sum run one thread per row of A in blocks of 256 and stream
B through LDS in tiles of 1024 rows; occupancy runs 256 threads x 8 vertices per block in x and 64 positions per block
in y."""
import functools

import numpy as np

TILE = 1024          # rows of B per LDS tile
BLOCK = 256          # rows of A per block
OCC_VPB = 256 * 8    # vertices per occupancy block
OCC_Q = 64           # positions per occupancy block

NS = (1, 63, 64, 255, 256, 257, 513)
MS = (1, 255, 1023, 1024, 1025, 2048, 2049, 3079)
THIN = ((70001, 5), (3, 70001))
SHAPES = tuple((n, m) for n in NS for m in MS) + THIN
SCALES = (0.01, 1.0, 50.0)
SQUARE = tuple(sorted(set(NS) | set(MS)))            # A = B cases of the large gamma

OCC_VS = (1, 7, 8, 9, 2047, 2048, 2049, 4097)
OCC_QS = (1, 63, 64, 65, 129)
OCC_HALF = 0.125                                     # with positions on a 1/64 grid, p +- half is exact


# ---- restatements and references ----------------------------------------------------------------------------------

def _rows(n, m, per=1 << 22):
    """Row ranges of A that keep an (rows, m) temporary at about ``per`` elements."""
    step = max(1, per // max(m, 1))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def min_dist32(a, b):
    """The kernel's text in float32: sqrt(((dx*dx + dy*dy) + dz*dz).min(1)).  NaN propagates as np.min does."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    out = np.empty(len(a), np.float32)
    bx, by, bz = b[:, 0][None], b[:, 1][None], b[:, 2][None]
    with np.errstate(all="ignore"):
        for lo, hi in _rows(len(a), len(b)):
            dx, dy, dz = a[lo:hi, 0:1] - bx, a[lo:hi, 1:2] - by, a[lo:hi, 2:3] - bz
            out[lo:hi] = np.sqrt(((dx * dx + dy * dy) + dz * dz).min(1))
    return out


def min_dist64(a, b):
    """The plain reference: the same float32 inputs widened to float64, sqrt(sum((a - b)**2)), min."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    out = np.empty(len(a), np.float64)
    with np.errstate(all="ignore"):
        for lo, hi in _rows(len(a), len(b)):
            d2 = sum((a[lo:hi, c:c + 1] - b[:, c][None]) ** 2 for c in range(3))
            out[lo:hi] = np.sqrt(d2).min(1)
    return out


def rbf64(a, b, gamma):
    """The plain reference: sum_ij exp(-gamma * sum((a_i - b_j)**2)), differences, squares and every sum in
    np.longdouble from the widened float32 inputs.  The direct form, not |a|^2 + |b|^2 - 2 a.b.  A tuple of gammas
    gives a tuple of sums over the same squared distances."""
    a, b = np.asarray(a, np.float32).astype(np.longdouble), np.asarray(b, np.float32).astype(np.longdouble)
    gammas = gamma if isinstance(gamma, tuple) else (gamma,)
    s = [np.longdouble(0) for _ in gammas]
    with np.errstate(all="ignore"):
        for lo, hi in _rows(len(a), len(b), 1 << 20):
            d2 = sum((a[lo:hi, c:c + 1] - b[:, c][None]) ** 2 for c in range(3))
            for j, g in enumerate(gammas):
                s[j] += np.exp(-np.longdouble(g) * d2).sum()
    return tuple(s) if isinstance(gamma, tuple) else s[0]


def rbf64_isnan(a, b, gamma):
    """Is rbf64 NaN?  Pairs of finite rows give finite terms, so only the strips of pairs that touch a non-finite row are
    evaluated."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad_a, bad_b = ~np.isfinite(a).all(1), ~np.isfinite(b).all(1)
    return bool((bad_a.any() and np.isnan(rbf64(a[bad_a], b, gamma))) or
                (bad_b.any() and np.isnan(rbf64(a, b[bad_b], gamma))))


def rbf_expanded64(a, b, gamma, clamp_nan=False):
    """The kernel's float64 form: exp(-gamma * max(|a|^2 + |b|^2 - 2 a.b, 0)) summed, np.maximum carrying NaN as the
    reference's rbf_kernel does.  ``clamp_nan`` is the wrong model in which the clamp turns a NaN into 0."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    an = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    bn = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    s = 0.0
    with np.errstate(all="ignore"):
        for lo, hi in _rows(len(a), len(b)):
            dot = (a[lo:hi, 0:1] * b[:, 0][None] + a[lo:hi, 1:2] * b[:, 1][None]) + a[lo:hi, 2:3] * b[:, 2][None]
            d2 = an[lo:hi, None] + bn[None] - 2.0 * dot
            d2 = np.where(d2 > 0.0, d2, 0.0) if clamp_nan else np.maximum(d2, 0.0)
            s += float(np.exp(-gamma * d2).sum())
    return s


def rbf_bound(a, b, gamma):
    """Relative tolerance of the expanded float64 form against rbf64.  Derived, not measured:
      gamma * 8 * 2**-53 * (max|a|^2 + max|b|^2)   the cancellation of the expansion in front of the exponent
      (m + 8 + 3 + nblk) * 2**-53                  the sequential per-thread sum over m, the 8-level block tree, the host
                                                   sum over nblk = ceil(n / 256) blocks, and exp's own rounding."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    n, m = len(a), len(b)
    nblk = -(-n // BLOCK)
    return (gamma * 8 * 2.0 ** -53 * ((a * a).sum(1).max() + (b * b).sum(1).max())
            + (m + 8 + 3 + nblk) * 2.0 ** -53)


def occupied(v, p, half):
    """The reference's expression, any(all((v >= p - half) & (v <= p + half), axis=1)) per position, in float64; a block
    of positions at a time."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    out = np.zeros(len(p), dtype=bool)
    with np.errstate(all="ignore"):
        lo, hi = p - half, p + half
        for a, b in _rows(len(p), 3 * len(v)):
            out[a:b] = np.all((v[None] >= lo[a:b, None]) & (v[None] <= hi[a:b, None]), axis=2).any(1)
    return out


# ---- metrics case builders ----------------------------------------------------------------------------------------

def _seed(*k):
    return np.random.default_rng([int(x) for x in k])


def far_clouds(n, m):
    """A in the unit cube (spread 1), B in the unit cube shifted by 20 on every axis: at least 10 spreads away."""
    rng = _seed(11, n, m)
    a = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    b = (rng.uniform(0.0, 1.0, (m, 3)) + 20.0).astype(np.float32)
    return a, b


PLANT_OFFSET = np.array([3.0e-4, -2.0e-4, 5.0e-4], np.float32)      # |offset| = 6.2e-4 < 1e-3


def planted_pairs(n, m):
    """(row of A, row of B) pairs to bring together, one pair at a time: A at the block edges, B at the tile edges."""
    rows = sorted({i for i in (0, BLOCK - 1, BLOCK, n - 1) if 0 <= i < n})
    cols = sorted({k for k in (0, TILE - 1, TILE, TILE + 1, m - 1) if 0 <= k < m})
    return [(i, k) for i in rows for k in cols]


def plant(a, b, i, k):
    """A copy of ``a`` whose row i sits PLANT_OFFSET from row k of ``b``, and the planted distance in the kernel's own
    float32 arithmetic.  The pair is brought together from A's side: every other row of A keeps all of B, row k
    included, at its own far distance."""
    a = a.copy()
    a[i] = b[k] + PLANT_OFFSET
    d = a[i] - b[k]
    return a, np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


@functools.lru_cache(maxsize=None)
def general_clouds(n, m, scale):
    """Seeded uniform clouds in [-scale, scale]^3.  Up to 100 rows of B coincide with rows of A, with +0.0 on A's side
    and -0.0 on B's side of one coordinate; up to 100 further rows of B are one float32 ulp from a row of A."""
    rng = _seed(23, n, m, int(scale * 100))
    a = rng.uniform(-scale, scale, (n, 3)).astype(np.float32)
    b = rng.uniform(-scale, scale, (m, 3)).astype(np.float32)
    idx = rng.permutation(m)
    same = idx[:min(100, (m + 1) // 2)]
    near = idx[len(same):len(same) + min(100, m - len(same))]
    src = rng.integers(0, n, len(same))
    a[src[::3], 1] = 0.0
    b[same] = a[src]
    b[same[::3], 1] = -0.0
    if len(near):
        src = rng.integers(0, n, len(near))
        b[near] = a[src]
        ax = 2 * rng.integers(0, 2, len(near))           # x or z: y may be an exact zero, whose neighbour is denormal
        up = np.where(rng.integers(0, 2, len(near)) == 1, np.float32(np.inf), np.float32(-np.inf))
        b[near, ax] = np.nextafter(b[near, ax], up)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def lattice_cloud(n, scale):
    """n distinct rows at least 0.125 * scale apart: shuffled points of a 16^3 lattice."""
    assert n <= 4096
    rng = _seed(31, n, int(scale * 100))
    ids = rng.permutation(4096)[:n]
    ijk = np.stack([ids % 16, (ids // 16) % 16, ids // 256], 1).astype(np.float64) - 8.0
    return (ijk * (0.125 * scale)).astype(np.float32)


def big_gamma(scale):
    return 1e6 / (scale * scale)


NONFINITE_SHAPE = (300, 2500)                        # B: two full tiles and a partial one; A: one full block and a tail
NONFINITE_ROWS_A = (0, 255, 299)
NONFINITE_ROWS_B = (5, 1500, 2499)                   # first tile, middle tile, partial last tile
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)


def nonfinite_cases():
    """(name, a, b): one bad coordinate in one row of A or of B, plus +inf on both sides of one coordinate (inf - inf)."""
    a0, b0 = general_clouds(*NONFINITE_SHAPE, 1.0)
    out = []
    for val in NONFINITE_VALUES:
        for i in NONFINITE_ROWS_A:
            a = a0.copy()
            a[i, i % 3] = val
            out.append((f"A[{i}]={val}", a, b0))
        for k in NONFINITE_ROWS_B:
            b = b0.copy()
            b[k, k % 3] = val
            out.append((f"B[{k}]={val}", a0, b))
    for k in NONFINITE_ROWS_B:
        a, b = a0.copy(), b0.copy()
        a[7, 2] = np.inf
        b[k, 2] = np.inf
        out.append((f"A[7]=inf,B[{k}]=inf", a, b))
    return out


# ---- occupancy case builders --------------------------------------------------------------------------------------

def occ_far(V, Q):
    """Vertices around (100, 100, 100); positions on a 1/64 grid, one per cell of a lattice of pitch 1/2, so that the
    cubes of half OCC_HALF stay apart and a vertex inside one is inside no other.  Nothing is occupied."""
    rng = _seed(41, V, Q)
    v = rng.uniform(100.0, 101.0, (V, 3))
    ids = rng.permutation(512)[:Q]
    cell = np.stack([ids % 8, (ids // 8) % 8, ids // 64], 1).astype(np.float64) * 0.5
    p = cell + rng.integers(0, 8, (Q, 3)).astype(np.float64) / 64.0
    return v, p


def occ_planted_pairs(V, Q):
    vs = sorted({i for i in (0, 7, 8, OCC_VPB - 1, OCC_VPB, V - 1) if 0 <= i < V})
    qs = sorted({k for k in (0, OCC_Q - 1, OCC_Q, Q - 1) if 0 <= k < Q})
    return [(i, k) for i in vs for k in qs]


OCC_INSIDE = np.array([0.05, -0.03, 0.1])


def occ_face_cases():
    """(name, offset of the vertex from the position, axis to step outward on, direction): the six faces and a corner of
    the cube of half OCC_HALF, the other coordinates strictly inside."""
    out = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            off = OCC_INSIDE.copy()
            off[ax] = sgn * OCC_HALF
            out.append((f"face {'-+'[sgn > 0]}{'xyz'[ax]}", off, ax, sgn))
    for ax in range(3):
        out.append((f"corner, out on {'xyz'[ax]}", np.array([OCC_HALF, -OCC_HALF, OCC_HALF]), ax, (1.0, -1.0, 1.0)[ax]))
    return out


def occ_nonfinite_cases():
    """(name, vertices, positions, half) with NaN and +-inf among the vertices, the positions or as the half size."""
    out = []
    for V, Q in ((9, 65), (2049, 64)):
        v0, p0 = occ_far(V, Q)
        v0[V - 1] = p0[Q - 1] + OCC_INSIDE                # one honest hit beside the bad values
        for val in NONFINITE_VALUES:
            v = v0.copy()
            v[0] = p0[0] + OCC_INSIDE
            v[0, 1] = val                                 # a bad coordinate in a vertex that would otherwise hit
            out.append((f"V{V} Q{Q} vertex {val}", v, p0, OCC_HALF))
            p = p0.copy()
            p[Q // 2, 2] = val
            out.append((f"V{V} Q{Q} position {val}", v0, p, OCC_HALF))
            v, p = v0.copy(), p0.copy()
            v[V // 2, 0] = val
            p[0] = v[V // 2]                              # the same bad value on both sides: inf is inside [inf, inf]
            p[0, 0] = val
            out.append((f"V{V} Q{Q} both {val}", v, p, OCC_HALF))
        out.append((f"V{V} Q{Q} half inf", v0, p0, np.inf))
        out.append((f"V{V} Q{Q} half nan", v0, p0, np.nan))
    return out
