"""Inputs and restatements for the edge tests of the two box families (csrc/lrc_objboxes.hip: lidarcast.object_boxes;
csrc/lrc_boxes.hip: lidarcast.instance_boxes).  numpy only (objbox_restate's cKDTree path serves objects of more than 4096
rows); importable without a GPU.  tests/test_box_edges_host.py counts the edges every builder promises and shows that a
wrong restatement changes the expected bytes on these very inputs.

Restatement.  avg of an object of at most 4096 rows comes from the full float64 distance matrix (neighbour_restate.Brute:
the expression (dx*dx + dy*dy) + dz*dz against every row, the k smallest ascending, np.cumsum of their square roots) -- no
tree and no candidate list, tied lattices are the point.  Annotation boxes reduce mean and std as objbox_restate restates
(256 chunks); detection boxes as instance_stats does below (lane t of 256 sums rows t, t + 256, ... of the instance in
ascending row order, a halving tree over the 256 lanes).  n == 1 with k == 1 is filtered: mean 0 and 0 / 0 under the root,
a NaN threshold (sign and payload are the divider's: same() asks for a NaN, nothing more), the row removed.

The zero rule, stated once (zero_rule): an extreme that equals zero has the sign of the last kept row whose coordinate on
that axis is +0 or -0; any other extreme is the plain min / max.  That is what numpy's p[keep].min(0) / .max(0) return (a
running np.minimum / np.maximum keeps the later of two equal values), and the expected value in the tests is literally
that numpy expression.

Coordinates are multiples of 2^-10 (2^-20 in the millimetre cluster) unless a builder says otherwise, so every object is
the same set of numbers in float64 and in float32 and both families run the same inputs."""
import numpy as np

import neighbour_restate as NR
import objbox_restate as OR

LANES = 256
BRUTE_MAX = 4096
LIST_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 21, 24, 25, 32)
STD_RATIO = 2.0

OBJBOX = np.dtype([("num_points", "<u8"), ("num_kept", "<u8"), ("filtered", "<u4"), ("reserved_", "<u4"),
                   ("min3", "<f8", (3,)), ("max3", "<f8", (3,)), ("mean", "<f8"), ("threshold", "<f8")])
BOX = np.dtype([("sem", "<u2"), ("ins", "<u2"), ("num_points", "<u4"), ("num_kept", "<u4"), ("filtered", "<u4"),
                ("min3", "<f4", (3,)), ("max3", "<f4", (3,)), ("mean", "<f8"), ("threshold", "<f8")])


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def same(got, want):
    """None if the two box arrays hold the same bytes, else the first difference.  A NaN threshold in `want` asks for a
    NaN in `got` (its sign and payload are not pinned); every other field of every box is compared by its bits."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"dtype / shape: {got.dtype} {got.shape} != {want.dtype} {want.shape}"
    for f in want.dtype.names:
        g, w = bits(got[f]), bits(want[f])
        ok = g == w
        if f == "threshold":
            ok = ok | (np.isnan(want[f]) & np.isnan(got[f]))
        if not np.all(ok):
            s = int(np.flatnonzero(~(ok.reshape(len(want), -1).all(1)))[0])
            return f"box {s} field {f}: got {got[f][s]!r} ({g[s]}), want {want[f][s]!r} ({w[s]})"
    return None


# ---- restatement ----------------------------------------------------------------------------------------------------
def avg_of(p, k, cache=None):
    """avg of every row of p (m >= k rows, float64)."""
    if len(p) > BRUTE_MAX:
        return OR.restate_avg(p, k)
    key = p.tobytes()
    b = None if cache is None else cache.get(key)
    if b is None:
        b = NR.Brute(p)
        if cache is not None:
            cache[key] = b
    return b.avg(k)


def object_stats(avg, std_ratio=STD_RATIO):
    """mean, threshold of an annotation object (lrc_cloud_preprocess's order for m rows)."""
    if len(avg) == 1:                              # 0 / 0 under the root
        return (float(avg[0]) if avg[0] > 0 else 0.0), float("nan")
    return OR.restate_stats(avg, std_ratio)


def lane_tree_sum(v):
    """box_stats_kernel's sum of v (excluded rows given as +0): lanes strided by 256, then the halving tree."""
    n = len(v)
    iters = max(1, -(-n // LANES))
    pad = np.zeros(iters * LANES)
    pad[:n] = v
    acc = np.zeros(LANES)
    for i in range(iters):
        acc = acc + pad[i * LANES:(i + 1) * LANES]
    w = LANES // 2
    while w:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w //= 2
    return np.float64(acc[0])


def instance_stats(avg, std_ratio=STD_RATIO):
    """mean, threshold of a detection instance in the kernel's order."""
    n = len(avg)
    pos = avg > 0
    mean = lane_tree_sum(np.where(pos, avg, 0.0)) / np.float64(n)
    d = avg - mean
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(lane_tree_sum(np.where(pos, d * d, 0.0)) / np.float64(n - 1))
    return float(mean), float(mean + std_ratio * sd)


def keep_of(avg, thr):
    return (avg > 0) & (avg < thr)


def numpy_extremes(p, keep):
    """The expected box: literally numpy's min / max over the kept rows."""
    kp = p[keep]
    if len(kp) == 0:
        return np.full(3, np.inf, p.dtype), np.full(3, -np.inf, p.dtype)
    return kp.min(0), kp.max(0)


def zero_rule(p, keep):
    """The zero rule written out (see the header); the host test shows numpy_extremes follows it on every input."""
    kp = p[keep]
    if len(kp) == 0:
        return np.full(3, np.inf, p.dtype), np.full(3, -np.inf, p.dtype)
    lo, hi = np.empty(3, p.dtype), np.empty(3, p.dtype)
    for c in range(3):
        x = kp[:, c]
        zeros = np.flatnonzero(x == 0)
        lo[c] = x[zeros[-1]] if x[np.argmin(x)] == 0 else x[np.argmin(x)]
        hi[c] = x[zeros[-1]] if x[np.argmax(x)] == 0 else x[np.argmax(x)]
    return lo, hi


class Parts:
    """The pieces an expected output is made of; the host test swaps one at a time for a wrong one."""
    avg = staticmethod(avg_of)
    object_stats = staticmethod(object_stats)
    instance_stats = staticmethod(instance_stats)
    keep = staticmethod(keep_of)
    extremes = staticmethod(numpy_extremes)

    @staticmethod
    def rows_of(off, s):
        return int(off[s]), int(off[s + 1])


def offsets_of(objs):
    return np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int64)


def concat(objs):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float64).reshape(-1, 3) for o in objs])), offsets_of(objs)


def expected_objects(pts, off, k, std_ratio=STD_RATIO, cache=None, parts=Parts):
    """(OBJBOX array, avg (n,), keep (n,) uint8, kept row indices) of lidarcast.object_boxes(pts, off, k, std_ratio)."""
    S, n = len(off) - 1, len(pts)
    boxes = np.zeros(S, OBJBOX)
    avg, keep = np.full(n, -1.0), np.ones(n, np.uint8)
    boxes["min3"], boxes["max3"], boxes["threshold"] = np.inf, -np.inf, np.inf
    m_all = np.diff(off)
    one = np.flatnonzero((m_all == 1) & (k > 1)) if parts.rows_of is Parts.rows_of else np.zeros(0, np.int64)
    if len(one):                                   # one-row objects below k: the row is the box
        boxes["num_points"][one] = boxes["num_kept"][one] = 1
        boxes["min3"][one] = boxes["max3"][one] = pts[off[one]]
    done = set(one.tolist())
    for s in range(S):
        if s in done:
            continue
        a, e = parts.rows_of(off, s)
        p = pts[a:e]
        m = len(p)
        b = boxes[s]
        b["num_points"] = m
        kp = np.ones(m, bool)
        if m >= k:
            av = parts.avg(p, k, cache)
            mean, thr = parts.object_stats(av, std_ratio)
            kp = parts.keep(av, thr)
            avg[a:e], keep[a:e] = av, kp
            b["filtered"], b["mean"], b["threshold"] = 1, mean, thr
        b["num_kept"] = int(kp.sum())
        b["min3"], b["max3"] = parts.extremes(p, kp)
    return boxes, avg, keep, np.flatnonzero(keep).astype(np.uint32)


def expected_instances(p32, sem, ins, class_ids, min_points, k, std_ratio=STD_RATIO, cache=None, parts=Parts):
    """(BOX array, avg (K,), keep (K,) uint8) of lidarcast.instance_boxes, boxes ordered by (class position, ins)."""
    K = len(p32)
    pos = np.full(1 << 16, -1, np.int64)
    pos[np.asarray(class_ids, np.int64)] = np.arange(len(class_ids))
    cls = pos[sem]
    key = np.where((ins != 0) & (cls >= 0), (cls << 16) | ins, 1 << 40)
    order = np.argsort(key, kind="stable")                   # ascending row order inside an instance
    sk = key[order]
    cut = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1], [True]])) if K else np.zeros(1, np.int64)
    avg, keep = np.full(K, -1.0), np.zeros(K, np.uint8)
    out = []
    for a, e in zip(cut[:-1], cut[1:]):
        if sk[a] == 1 << 40 or e - a < min_points:
            continue
        rows = order[a:e]
        n = len(rows)
        b = np.zeros((), BOX)
        b["sem"], b["ins"], b["num_points"] = class_ids[int(sk[a]) >> 16], int(sk[a]) & 0xFFFF, n
        p = p32[rows]
        if n == 1 and k > 1:
            keep[rows] = 1
            b["num_kept"], b["min3"], b["max3"], b["threshold"] = 1, p[0], p[0], np.inf
            out.append(b)
            continue
        kp = np.ones(n, bool)
        b["threshold"] = np.inf
        if n >= k:
            av = parts.avg(p.astype(np.float64), k, cache)
            mean, thr = parts.instance_stats(av, std_ratio)
            kp = parts.keep(av, thr)
            avg[rows] = av
            b["filtered"], b["mean"], b["threshold"] = 1, mean, thr
        keep[rows] = kp
        b["num_kept"] = int(kp.sum())
        b["min3"], b["max3"] = parts.extremes(p, kp)
        out.append(b)
    return (np.stack(out) if out else np.zeros(0, BOX)), avg, keep


# ---- building blocks ------------------------------------------------------------------------------------------------
Q = 1024.0                                          # coordinates are k / Q
FAR = 1000.0                                        # an outlier this far off is removed, and makes the threshold so
#                                                     large that the filter keeps every row of the unit cube


def _cube(rng, m, lo=(0, 0, 0), size=1.0):
    """m rows of a cube, multiples of 1 / Q."""
    return (rng.integers(0, int(size * Q), (m, 3)) + np.round(np.asarray(lo, np.float64) * Q)) / Q


def _tiny(dtype):
    return float(np.finfo(dtype).smallest_subnormal)


def signed_objects(dtype=np.float64, seed=11):
    """Objects wholly in each of the seven octants with a negative axis, objects straddling the origin on one, two and
    three axes, and one wholly negative object whose maxima are the smallest negative denormals of `dtype`; each with 60
    rows (filtered at k = 20) and with 7 (not filtered)."""
    rng = np.random.default_rng(seed)
    objs, kinds = [], []
    for m in (60, 7):
        for o in range(1, 8):
            sign = np.array([-1.0 if o >> c & 1 else 1.0 for c in range(3)])
            objs.append(_cube(rng, m, (0.125, 0.125, 0.125)) * sign)
            kinds.append(("octant", o, m))
        for axes in ((0,), (1, 2), (0, 1, 2)):
            lo = [(-0.5 if c in axes else 0.125) for c in range(3)]
            p = _cube(rng, m, lo)
            for c in axes:                                       # both signs for certain, no zero
                p[p[:, c] == 0, c] = 1 / Q
                p[0, c], p[1, c] = -abs(p[0, c]), abs(p[1, c])
            objs.append(p)
            kinds.append(("straddle", len(axes), m))
        p = -_cube(rng, m, (0.125, 0.125, 0.125))
        for c in range(3):
            p[c + 1, c] = -_tiny(dtype)
            p[c + 2, c] = -2 * _tiny(dtype)
        p[0] = -FAR                                              # see _zero_object: every other row is kept
        objs.append(p)
        kinds.append(("denormal", 0, m))
    edges = {"octants": len({k[1] for k in kinds if k[0] == "octant"}),
             "straddle_axes": sorted({k[1] for k in kinds if k[0] == "straddle"}),
             "denormal": sum(k[0] == "denormal" for k in kinds),
             "filtered": sum(k[2] >= 20 for k in kinds), "unfiltered": sum(k[2] < 20 for k in kinds)}
    return objs, edges, kinds


def _zero_object(rng, m, axis, side, last, zero_rows, removed_last):
    """m rows of the unit cube on the positive side of `axis` (side = min) or mirrored (side = max); the rows
    zero_rows get +-0 on `axis` with alternating signs, the last of them the sign `last`.  removed_last appends a far
    outlier (the filter removes it) whose coordinate on `axis` is a zero of the other sign.  Row 50 of a filtered
    object is a far outlier too, so that the filter keeps every row of the cube, the zero rows among them."""
    p = _cube(rng, m)
    p[p[:, axis] == 0, axis] = 1 / Q
    if m >= 50:
        p[50] = FAR
    if side == "max":
        p[:, axis] = -p[:, axis]
    signs = [(-1.0 if (i % 2) else 1.0) for i in range(len(zero_rows))]
    signs[-1] = last
    if len(signs) > 1 and signs[0] == last:
        signs[0] = -last                                         # the first and the last zero row differ
    for r, s in zip(zero_rows, signs):
        p[r, axis] = np.copysign(0.0, s)
    if removed_last:
        far = np.full(3, -2 * FAR)
        far[axis] = np.copysign(0.0, -last)
        p = np.vstack([p, far])
    return p


def zero_objects(seed=12):
    """Per axis, side (min, max) and sign of the last kept zero row: an object of 300 rows (zero rows 5, 100, 280), the
    same followed by a removed far outlier holding a zero of the other sign, an object of 700 rows whose zero rows 3,
    260, 520, 690 fall into different 256-lane strides (detection) and different chunks (annotation: ceil(700 / 256) = 3
    rows each), and an unfiltered one of 10 rows.  Then per axis an object with zero rows whose extremes are not zero
    (it straddles the origin)."""
    rng = np.random.default_rng(seed)
    objs, kinds = [], []
    for axis in range(3):
        for side in ("min", "max"):
            for last in (1.0, -1.0):
                for m, rows, removed in ((300, (5, 100, 280), False), (299, (5, 100, 280), True),
                                         (700, (3, 260, 520, 690), False), (10, (2, 6, 8), False)):
                    objs.append(_zero_object(rng, m, axis, side, last, rows, removed))
                    kinds.append((axis, side, last, len(objs[-1]), removed))
    for axis in range(3):
        p = _cube(rng, 300, (-0.5, -0.5, -0.5))
        p[p[:, axis] == 0, axis] = 1 / Q
        p[[7, 150, 290], axis] = [0.0, -0.0, 0.0]
        p[50] = FAR
        objs.append(p)
        kinds.append((axis, "inner", 1.0, 300, False))
    return objs, {"objects": len(objs)}, kinds


def equal_avg_object():
    """256 rows: 128 pairs 0.25 apart, the pairs 16 apart on a line.  At k = 2 every avg is 0.125, the sums of 256 equal
    values are exact in either reduction order, so mean == threshold == avg: nothing is kept, and avg <= threshold
    would keep everything."""
    p = np.zeros((256, 3))
    p[:, 0] = np.repeat(np.arange(128) * 16.0, 2)
    p[1::2, 1] = 0.25
    return p


def list_length_objects(k, seed=13):
    """One cloud for the list length k: objects of k - 1, k, k + 1 and 300 rows, one row, and equal_avg_object()."""
    rng = np.random.default_rng(seed + k)
    objs = [_cube(rng, m, (-0.25, 3.0, -1.0), 0.5) for m in (k - 1, k, k + 1, 300, 1)] + [equal_avg_object()]
    return objs, {"sizes": [len(o) for o in objs]}


def table_objects(seed=14):
    """Offset tables: S = 1; runs of one and of three empty objects at the start, in the middle and at the end."""
    rng = np.random.default_rng(seed)
    A, B, C, D = (_cube(rng, m, (-0.5, 0, 0), 0.5) for m in (40, 5, 300, 25))
    E = np.zeros((0, 3))
    tables = {"single": [C], "empty_runs_1": [E, A, B, E, C, D, E],
              "empty_runs_3": [E, E, E, A, B, E, E, E, C, D, E, E, E]}
    return tables, {name: [s for s, o in enumerate(objs) if len(o) == 0] for name, objs in tables.items()}


def many_objects(S, seed=15):
    """S objects (more than one grid row of 65535 needs the stride loops): one row each, but filtered objects of 40 rows at
    0, 65534, 65535, 65536 and S - 1 and an empty object beside each of them."""
    rng = np.random.default_rng(seed)
    big = sorted({i for i in (0, 65534, 65535, 65536, S - 1) if 0 <= i < S})
    empty = set()
    for i in big:
        j = i + 1 if i + 1 < S and i + 1 not in big else i - 1
        while j in big:
            j -= 1
        empty.add(j)
    m = np.ones(S, np.int64)
    m[big] = 40
    m[sorted(empty)] = 0
    off = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    pts = _cube(rng, int(off[-1]), (-4, -4, -1), 8.0)
    for i in big:                                               # compact, so that the filter has something to keep
        pts[off[i]:off[i + 1]] = _cube(rng, 40, (i % 7 - 3.0, -0.5, 0), 0.25)
    return pts, off, {"filtered": big, "empty": sorted(empty), "rows": int(off[-1])}


def sheet(m, seed):
    """m rows of a 4 x 3 sheet 2 / Q thick.  Rows 0, 256, 257 and m - 1 hold -0, +0, -0, +0 in z (z >= 0 elsewhere): with
    m > 65536 rows 0 and 256 are one lane's first and second row of chunk 0."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.integers(0, 4 * 1024, m), rng.integers(0, 3 * 1024, m), rng.integers(1, 3, m)], 1) / Q
    rows = [r for r in (0, 256, 257) if r < m - 1] + [m - 1]
    p[rows, 2] = [-0.0, 0.0, -0.0, 0.0][-len(rows):]
    return p


def chunk_objects():
    """Reduction chunks: chunk = ceil(m / 256); a lane takes a second row of its chunk from chunk = 257 on."""
    small = [sheet(m, 16 + m) for m in (255, 256, 257, 511, 512, 513)]
    large = [sheet(m, 17 + m) for m in (65535, 65536, 65537)]
    return (small, large), {"rows": [len(o) for o in small + large], "chunk": [-(-len(o) // 256) for o in small + large]}


def degenerate_objects(seed=18):
    """name -> (object, lattice spacing or None), and the rows each holds."""
    rng = np.random.default_rng(seed)
    out = {}
    out["identical"] = (np.tile([[-1.5, 2.25, 0.75]], (40, 1)), None)
    p = _cube(rng, 300, (-0.5, -0.5, 0), 1.0)
    p[40:60] = p[40]
    out["coincident_in_300"] = (p, None)
    line = np.zeros((200, 3))
    line[:, 1] = rng.permutation(200) / 64.0 - 1.0
    line[:, 0], line[:, 2] = -0.5, 2.0
    out["axis_line"] = (line, 1 / 64.0)
    plane = _cube(rng, 400, (-1, 0, -1), 2.0)
    plane[:, 1] = -3.0
    out["axis_plane"] = (plane, None)
    mm = rng.integers(0, 1024, (1000, 3)) / 2.0 ** 20            # inside 1 mm
    out["mm_and_km"] = (np.vstack([mm[:500], [[FAR, 0.0, 0.0]], mm[500:]]), None)
    out["lattice"] = (NR.lattice(), 0.25)
    out["decimal_lattice"] = (NR.decimal_lattice(), 0.1)
    return out, {name: len(p) for name, (p, _) in out.items()}


def mixed_wave_objects(seed=19):
    """600 objects of 1..40 rows, centres 1 / 16 apart on x and cubes of side 0.5: neighbours overlap in space, so after
    the cell sort a wavefront holds rows of filtered (>= 20 rows) and unfiltered objects."""
    rng = np.random.default_rng(seed)
    objs = [_cube(rng, 1 + s % 40, (s / 16.0 - 18.0, -0.25, -0.25), 0.5) for s in range(600)]
    return objs, {"filtered": sum(len(o) >= 20 for o in objs), "unfiltered": sum(len(o) < 20 for o in objs)}


# ---- annotation-box cases: name -> (objects, k, the two further cell sizes) ----------------------------------------------
def object_cases():
    cases = {"signed": (signed_objects()[0], 20, (0.125, 3.0)), "zero_extremes": (zero_objects()[0], 20, (0.125, 3.0))}
    for k in LIST_LENGTHS:
        cases[f"k{k:02d}"] = (list_length_objects(k)[0], k, (0.05, 20.0))
    for name, objs in table_objects()[0].items():
        cases[name] = (objs, 20, (0.05, 2.0))
    small, large = chunk_objects()[0]
    cases["chunks_small"] = (small, 20, (0.05, 2.0))
    cases["chunks_large"] = (large, 20, (0.02, 1.0))
    for name, (p, spacing) in degenerate_objects()[0].items():
        cases["deg_" + name] = ([p], 20, (spacing or 0.05, 7.0))
    cases["mixed_waves"] = (mixed_wave_objects()[0], 20, (0.05, 2.0))
    return cases


# ---- detection-box inputs -----------------------------------------------------------------------------------------------
def cloud_of(instances, ignored_every=5, seed=20):
    """One labelled cloud from (sem, ins, rows) triples: the instances one after the other in row order, and after
    every `ignored_every` rows one row with ins = 0 (ignored), so kept and ignored rows interleave."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for _, _, p in instances])
    sem = np.concatenate([np.full(len(p), s, np.uint16) for s, _, p in instances])
    ins = np.concatenate([np.full(len(p), i, np.uint16) for _, i, p in instances])
    if ignored_every:
        at = np.arange(ignored_every, len(pts), ignored_every)
        pts = np.insert(pts, at, rng.integers(-4096, 4096, (len(at), 3)) / Q, axis=0)
        sem = np.insert(sem, at, sem[at - 1])
        ins = np.insert(ins, at, 0)
    return np.ascontiguousarray(pts.astype(np.float32)), sem, ins


CLASSES6 = [5, 0, 0xFFFF, 9, 10, 11]               # class ids 0 and 0xFFFF; 9 gets no row


def labelled(objs, classes=(5, 0, 0xFFFF, 10, 11)):
    """Objects as instances: classes in turn, instance ids 1, 2, ... and 65535 for the last; empty objects are left out."""
    objs = [o for o in objs if len(o)]
    out = [(classes[j % len(classes)], 1 + j // len(classes), o) for j, o in enumerate(objs)]
    out[-1] = (out[-1][0], 65535, out[-1][2])
    return out


def size_instances(min_points, k, seed=21):
    """Instances of min_points - 1, min_points, k - 1, k, k + 1, 255, 256, 257 and 513 rows (those of no row left out)."""
    rng = np.random.default_rng(seed)
    sizes = [m for m in (min_points - 1, min_points, k - 1, k, k + 1, 255, 256, 257, 513) if m > 0]
    return labelled([_cube(rng, m, (-0.5, -0.5, -0.5), 1.0) for m in sizes]), sizes


def many_segments(seed=22):
    """64 classes x 1100 instances of one row, min_points = 1: 70400 workgroups of box_grid_kernel and box_stats_kernel;
    three instances of 40 rows are first, in the middle and last in box order."""
    rng = np.random.default_rng(seed)
    classes = [int(c) for c in rng.permutation(np.arange(100, 164))]
    sem = np.repeat(np.array(classes, np.uint16), 1100)
    ins = np.tile(np.arange(1, 1101, dtype=np.uint16), 64)
    pts = _cube(rng, len(sem), (-4, -4, -1), 8.0)
    big = [(classes[0], 1), (classes[32], 550), (classes[63], 1100)]
    extra = [(s, i, _cube(rng, 39, (j - 1.0, -0.5, 0), 0.25)) for j, (s, i) in enumerate(big)]
    pts = np.vstack([pts] + [p for _, _, p in extra])
    sem = np.concatenate([sem] + [np.full(39, s, np.uint16) for s, _, _ in extra])
    ins = np.concatenate([ins] + [np.full(39, i, np.uint16) for _, i, _ in extra])
    for j, (s, i) in enumerate(big):                             # the 40th row joins its 39
        pts[np.flatnonzero((sem == s) & (ins == i))[0]] = [j - 1.0, -0.5, 0.0]
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm].astype(np.float32)), sem[perm], ins[perm], classes, big


def instance_cases():
    """name -> (points32, sem, ins, class ids, min_points, k, the two further cell sizes)."""
    c = {}
    signed32 = signed_objects(np.float32)[0]
    c["signed"] = cloud_of(labelled(signed32)) + (CLASSES6, 1, 20, (0.125, 3.0))
    c["zero_extremes"] = cloud_of(labelled(zero_objects()[0])) + (CLASSES6, 1, 20, (0.125, 3.0))
    for k in LIST_LENGTHS:
        c[f"k{k:02d}"] = cloud_of(labelled(list_length_objects(k)[0])) + (CLASSES6, 1, k, (0.05, 20.0))
    for mp, k in ((5, 20), (20, 20), (30, 20), (1, 20), (1, 1)):
        c[f"sizes_mp{mp}_k{k}"] = cloud_of(size_instances(mp, k)[0]) + (CLASSES6, mp, k, (0.05, 2.0))
    one = cloud_of(labelled(table_objects()[0]["empty_runs_1"]))
    c["one_class"] = one + ([0xFFFF], 1, 20, (0.05, 2.0))
    c["every_row_ignored"] = (one[0], one[1], np.zeros_like(one[2]), CLASSES6, 1, 20, (0.05, 2.0))
    rng = np.random.default_rng(23)
    ids64 = [0, 0xFFFF] + [int(x) for x in rng.permutation(np.arange(1, 400))[:62]]
    c["64_classes"] = cloud_of(labelled([_cube(rng, 1 + (7 * j) % 45, (-1, -1, -1), 0.75) for j in range(128)],
                                        ids64)) + (ids64, 1, 20, (0.05, 2.0))
    for name, (p, spacing) in degenerate_objects()[0].items():
        c["deg_" + name] = cloud_of([(10, 65535, p)]) + (CLASSES6, 1, 20, (spacing or 0.05, 7.0))
    return c
