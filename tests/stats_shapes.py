"""Segment layouts and values for the frame-statistics tests (csrc/lrc_stats.h), shared by the CPU and the GPU side.

The device statistics copy numpy's summation step by step (buffer chunks of 8192 values added left to right, pairwise
sums inside a chunk, kStatPar workgroups striding over a segment's chunks, chunk sums indexed from `first_row`).  The
layouts below put segment lengths on every edge of that scheme; the values are spread over seven decades so that a
wrong bracket changes bits.  tests/test_stats_shapes_gpu.py runs the kernels on exactly this data and
tests/test_stats_shapes_discrimination.py checks, on the same data, that a wrong summation order would have been seen.

Everything here is a pure function of its arguments and fixed seeds."""
import numpy as np

CHUNK = 8192                    # numpy's buffer size: the chunk of the device scheme
STAT_PAR = 8                    # kStatPar: workgroups per segment
# ragged-tail lengths from which the slot tree of block_reduce_numpy is one level deeper (the first length of each depth)
DEPTH_TAILS = (129, 249, 489, 969, 1929, 3849, 7689)
TAIL_RESIDUES = (0, 1, 7, 8, 9, 127, 128, 129, 4095, 4096, 7689, 8191)
LONGEST = 17 * CHUNK + 8191     # three strides of kStatPar chunks
_BLOCK = 1 << 20                # rows generated (and measured) per block: bounded host memory at any layout size


def slot_depth(n):
    """Depth D of the deepest leaf of numpy's pairwise tree over n <= 8192 values (0 for a single leaf)."""
    d = 0
    while n > 128:
        h = n // 2
        h -= h % 8
        n -= h
        d += 1
    return d


def catalogue():
    """The segment-length catalogue, in a fixed shuffled order so that segments start at scattered offsets."""
    lengths = list(range(0, 301)) + list(range(1016, 1041)) + list(range(8180, 8201))
    for t in DEPTH_TAILS:
        lengths += [t - 1, t, t + 1]
    lengths += list(range(7689, 8192))
    lengths += [CHUNK * k + r for k in range(1, 11) for r in TAIL_RESIDUES]
    lengths += [LONGEST]
    order = np.random.default_rng(101).permutation(len(lengths))
    return np.asarray(lengths, dtype=np.int64)[order]


def every_tail():
    """Every ragged length 1..8191, in order."""
    return np.arange(1, CHUNK, dtype=np.int64)


def one_chunk_plus_tail():
    """8192 + r for r sampled over 0..8191: all residues that change the tail tree's depth and a stride of 13."""
    r = set(range(0, CHUNK, 13)) | set(DEPTH_TAILS) | {t - 1 for t in DEPTH_TAILS} | set(TAIL_RESIDUES)
    r |= set(range(7689, 7712)) | {8190, 8191}
    return CHUNK + np.asarray(sorted(r), dtype=np.int64)


def with_empty_segments():
    """Zero-length segments between non-empty ones, runs of them, and at both ends."""
    base = [5, 129, 8191, 8192, 8193, 3 * CHUNK + 7689, 300, 17 * CHUNK + 1, 1, 7690, 9 * CHUNK]
    out = [0, 0]
    for i, n in enumerate(base):
        out += [n] + [0] * (1 + i % 3)
    return np.asarray(out, dtype=np.int64)


def small_layout():
    return np.asarray([3, 0, 200, 8200, 17], dtype=np.int64)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])


def rows_for(counts, seed, extra=0, poison=1e18):
    """(sum(counts) + extra, 4) float32 (x, y, z, label) rows: random directions (every sign, some axis-aligned with +-0
    coordinates) times ranges exp(uniform(-7, 9)) (1e-3 .. 8e3).  The `extra` rows after the last segment hold
    `poison` in every coordinate."""
    total = int(np.sum(counts))
    rows = np.empty((total + extra, 4), dtype=np.float32)
    axes = np.array([[0.0, 0.0, 1.0], [-0.0, 1.0, -0.0], [1.0, -0.0, 0.0], [0.0, 0.0, -1.0], [-0.0, -1.0, 0.0],
                     [-1.0, 0.0, -0.0]])
    for b0 in range(0, total, _BLOCK):
        n = min(_BLOCK, total - b0)
        rng = np.random.default_rng([seed, b0 // _BLOCK])
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pick = rng.random(n) < 0.05
        d[pick] = axes[rng.integers(0, len(axes), int(pick.sum()))]
        r = np.exp(rng.uniform(-7.0, 9.0, n))
        rows[b0:b0 + n, :3] = d * r[:, None]
        rows[b0:b0 + n, 3] = rng.integers(0, 1 << 16, n).astype(np.float32)
    rows[total:] = np.float32(poison)
    return rows


def row_ranges(rows):
    """np.linalg.norm(rows[:, :3], axis=1), block by block (each row is independent: the same bits)."""
    out = np.empty(len(rows), dtype=np.float32)
    for b0 in range(0, len(rows), _BLOCK):
        out[b0:b0 + _BLOCK] = np.linalg.norm(rows[b0:b0 + _BLOCK, :3], axis=1)
    return out


def incident_values(total, seed):
    """float64 values that look like incident angles in degrees, 0..90."""
    return np.random.default_rng([seed, 7]).uniform(0.0, 90.0, int(total))


# The direct entry point's layouts (lrc_cloud_range_stats_dev): name -> (lengths, seed).
DIRECT_LAYOUTS = {
    "catalogue": (catalogue, 1),
    "every_tail": (every_tail, 2),
    "one_chunk_plus_tail": (one_chunk_plus_tail, 3),
    "with_empty": (with_empty_segments, 4),
    "small": (small_layout, 5),
}


def direct_layout(name):
    fn, seed = DIRECT_LAYOUTS[name]
    counts = fn()
    return counts, seed


# ---- the frames path (lrc_scan_rays_compact -> frames_finish) ---------------------------------------------------------
# A closed cube with the world origin just inside one corner, every ray starting inside it and aimed at a point of one
# of the three faces through that corner: every ray hits, the ranges from the world origin spread over six decades
# (1e-2 .. 1.3e4, so that a wrong bracket changes bits as it does on the direct layouts), and the keep mask keeps the
# first L_p hits of pose p, so the frame lengths are exactly the designed ones.  frames_finish has three ways of calling
# launch_segment_stats; each case picks one:
#   one_stream : chunks == 1 and P*N*row_bytes <= 4 MB (12 bytes per row: range_origin + incident_deg)
#   graded     : P >= 8, N % 64 == 0, P*N >= 2^20 -> chunks of poses [0, 2), [2, 8), [8, 16); first_row = p0 * N
#   per_pose   : P < 4, P*N >= 2^20 -> one pose per chunk
CUBE_LO, CUBE_HI = -0.01, 1.0e4
FRAME_CASES = {
    "one_stream": (20480, [0, 1, 100, 9, 60, 7689, 8191, 8192, 8193, 9000, 12000, 14000, 2 * CHUNK, 2 * CHUNK + 1,
                        20479, 20480]),
    "graded": (9 * CHUNK, [9 * CHUNK, 0, 8 * CHUNK + 1, 1, 8 * CHUNK + 7689, 8 * CHUNK + 4096, 129, 9 * CHUNK - 1,
                           8 * CHUNK, 0, 8 * CHUNK + 7697, 12000, 60, 8 * CHUNK + 7696, 7689, 8 * CHUNK + 8190]),
    "per_pose": (1 << 19, [(1 << 19) - 503, 17 * CHUNK + 8191, (1 << 19) - 1]),
}


def frame_rays(P, N, seed):
    """(P, N, 6) float32 rays: each aimed from inside the cube at a point of a face through the origin's corner whose
    two free coordinates are log-uniform in 1e-3 .. 9e3."""
    rng = np.random.default_rng([seed, P, N])
    target = np.exp(rng.uniform(np.log(1e-3), np.log(9e3), size=(P, N, 3)))
    face = rng.integers(0, 3, size=(P, N))
    np.put_along_axis(target, face[..., None], CUBE_LO, axis=2)
    inner = rng.uniform(CUBE_LO + 1.0, CUBE_HI - 1.0, size=(P, N, 3))
    o = target + rng.uniform(1e-3, 0.5, size=(P, N, 1)) * (inner - target)
    d = target - o
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return np.concatenate([o, d], axis=2).astype(np.float32)


def frame_columns_approx(rays, lengths):
    """What the frames of `rays` with the first L_p rays of pose p kept hold, to float64 accuracy: the float32 range
    from the world origin and the float64 incident angle of the exit point.  For the CPU-side discrimination check:
    the same distribution as the device's columns, not their bits."""
    rng_cols, inc_cols = [], []
    for p, L in enumerate(lengths):
        o = rays[p, :L, :3].astype(np.float64)
        d = rays[p, :L, 3:].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_axis = np.where(d > 0, (CUBE_HI - o) / d, np.where(d < 0, (CUBE_LO - o) / d, np.inf))
        axis = np.argmin(t_axis, axis=1)
        t = t_axis[np.arange(L), axis]
        pt = (o + t[:, None] * d).astype(np.float32)
        rng_cols.append(np.linalg.norm(pt, axis=1))
        cosang = np.abs(d[np.arange(L), axis]) / np.linalg.norm(d, axis=1)
        inc_cols.append(np.degrees(np.arccos(np.clip(cosang, 0.0, 1.0))))
    return rng_cols, inc_cols
