"""A bit-equal pass of the device frame statistics only means something if a wrong summation order would have changed
the bits.  On exactly the data of tests/test_stats_shapes_gpu.py (tests/stats_shapes.py), np.mean / np.std must differ
from each of these wrong schemes in a clear share of the segments of every length class the scheme is distinct on:
  left_to_right     one running sum over the whole segment
  unchunked         numpy's pairwise recursion without the 8192-value buffer chunks            (n > 8192)
  chunks_pairwise   numpy's chunk sums combined by a balanced tree instead of left to right     (>= 3 chunks)
  float64_once      float32 values accumulated in float64, rounded to float32 once at the end   (float32 only)
while lidarcast.npmodel, the scheme csrc/lrc_stats.h implements, agrees with numpy on a sample of the same segments.
Shares are counted per family (the direct layouts together, the three frames cases together), dtype, scheme and length
class.  The frames' values here are the analytic hit ranges and angles of the same rays, not the device's bits."""
import functools

import numpy as np
import pytest

import stats_shapes as ss
from helpers import bits

CHUNK = ss.CHUNK
CLASSES = (("leaf 9..128", 9, 128), ("tree 129..8192", 129, CHUNK), ("two chunks 8193..16384", CHUNK + 1, 2 * CHUNK),
           ("3+ chunks", 2 * CHUNK + 1, 1 << 62))
SHARE = 0.30


def _left_to_right(a):
    return np.cumsum(a)[-1]                      # add.accumulate: one dependent chain in the array's type


def _unchunked(a):
    n = len(a)
    if n <= CHUNK:
        return np.add.reduce(a)                  # one buffer chunk: numpy's pairwise sum itself
    n2 = n // 2
    n2 -= n2 % 8
    return a.dtype.type(_unchunked(a[:n2]) + _unchunked(a[n2:]))


def _tree(c, T):
    if len(c) == 1:
        return c[0]
    h = len(c) // 2
    return T(_tree(c[:h], T) + _tree(c[h:], T))


def _chunks_pairwise(a):
    return _tree([np.add.reduce(a[i:i + CHUNK]) for i in range(0, len(a), CHUNK)], a.dtype.type)


def _float64_once(a):
    return a.dtype.type(np.add.reduce(a, dtype=np.float64))


SCHEMES = {                                     # name -> (sum, dtypes, first class index it is distinct on)
    "left_to_right": (_left_to_right, (np.float32, np.float64), 0),
    "unchunked": (_unchunked, (np.float32, np.float64), 2),
    "chunks_pairwise": (_chunks_pairwise, (np.float32, np.float64), 3),
    "float64_once": (_float64_once, (np.float32,), 0),
}


def _mean_std(a, total):
    T = a.dtype.type
    n = T(len(a))
    m = T(total(a) / n)
    x = (a - m).astype(a.dtype)
    x = (x * x).astype(a.dtype)
    return m, T(np.sqrt(T(total(x) / n)))


def _class_of(n):
    for k, (_, lo, hi) in enumerate(CLASSES):
        if lo <= n <= hi:
            return k
    return None


@functools.lru_cache(maxsize=1)
def _datasets():
    """(source, segments) pairs: the float32 range columns of every direct layout, float64 incident-like values over
    the catalogue, and both columns of the three frames cases (their analytic values)."""
    return list(_generate())


def _generate():
    for name in ss.DIRECT_LAYOUTS:
        counts, seed = ss.direct_layout(name)
        rng = ss.row_ranges(ss.rows_for(counts, seed))
        off = ss.offsets(counts)
        yield f"direct/{name}/float32", [rng[off[i]:off[i + 1]] for i in range(len(counts))]
    counts, seed = ss.direct_layout("catalogue")
    inc = ss.incident_values(int(counts.sum()), seed)
    off = ss.offsets(counts)
    yield "direct/catalogue/float64", [inc[off[i]:off[i + 1]] for i in range(len(counts))]
    for case, (N, lengths) in ss.FRAME_CASES.items():
        rays = ss.frame_rays(len(lengths), N, seed=len(case))
        r, a = ss.frame_columns_approx(rays, lengths)
        yield f"frames/{case}/float32", r
        yield f"frames/{case}/float64", a


def test_depth_tails_are_where_the_slot_tree_deepens():
    """DEPTH_TAILS are exactly the lengths <= 8191 at which the ragged tail's tree first reaches a new depth."""
    first = {}
    for n in range(1, CHUNK):
        first.setdefault(ss.slot_depth(n), n)
    assert tuple(v for k, v in sorted(first.items()) if k > 0) == ss.DEPTH_TAILS


def test_layouts_cover_the_kernel_edges():
    cat = ss.catalogue()
    assert len(cat) > 256                                        # more than one segment_combine_kernel workgroup
    assert cat.max() == ss.LONGEST > 2 * ss.STAT_PAR * CHUNK    # the c += kStatPar loop runs three times
    assert set(range(7689, 8192)) <= set(cat.tolist()) and 0 in cat
    assert set(ss.every_tail().tolist()) == set(range(1, CHUNK))
    assert (ss.with_empty_segments() == 0).sum() > 10
    for case, (N, lengths) in ss.FRAME_CASES.items():
        assert max(lengths) <= N and N % 64 == 0
        P = len(lengths)
        if case == "one_stream":
            assert P * N < (1 << 20) and P * N * 12 <= (4 << 20)
        elif case == "graded":
            assert P >= 8 and P * N >= (1 << 20)
            # poses of the later chunks ([2, 8) and [8, 16)) above 8 chunks with ragged tails
            assert any(n > ss.STAT_PAR * CHUNK and n % CHUNK for n in lengths[2:8])
            assert any(n > ss.STAT_PAR * CHUNK and n % CHUNK for n in lengths[8:])
        else:
            assert P < 4 and P * N >= (1 << 20)


@pytest.mark.parametrize("source", ["direct/catalogue/float32", "direct/catalogue/float64", "frames/graded/float32"])
def test_npmodel_is_numpy_on_this_data(source):
    """The scheme the kernel implements (lidarcast.npmodel) gives numpy's bits on a sample of the segments."""
    from lidarcast import npmodel
    segs = dict(_datasets())[source]
    rng = np.random.default_rng(3)
    pick = [i for i in range(len(segs)) if len(segs[i]) > 0]
    pick = sorted(rng.choice(pick, min(60, len(pick)), replace=False).tolist()) + \
        [i for i in range(len(segs)) if len(segs[i]) > 2 * CHUNK][:4]
    for i in pick:
        a = segs[i]
        m, s = npmodel.model_mean_std(a)
        assert bits(np.asarray([m, s])).tolist() == bits(np.asarray([np.mean(a), np.std(a)])).tolist(), (source, len(a))


def test_wrong_summation_orders_change_the_bits():
    tally = {}               # (family, dtype, scheme, class) -> (segments, segments on which numpy differs)
    for source, segs in _datasets():
        family, _, dtname = source.split("/")
        dt = segs[0].dtype.type
        for a in segs:
            k = _class_of(len(a))
            if k is None:
                continue
            m, s = np.mean(a), np.std(a)
            assert type(m) is dt
            for scheme, (total, dtypes, first_class) in SCHEMES.items():
                if dt not in dtypes or k < first_class:
                    continue
                wm, ws = _mean_std(a, total)
                diff = bits(np.asarray([m, s])).tolist() != bits(np.asarray([wm, ws], dtype=dt)).tolist()
                n, d = tally.get((family, dtname, scheme, k), (0, 0))
                tally[(family, dtname, scheme, k)] = (n + 1, d + int(diff))
    rows, failures, seen = [], [], set()
    for (family, dtname, scheme, k), (n, d) in sorted(tally.items()):
        seen.add((scheme, k))
        rows.append(f"{family:7s} {dtname:8s} {scheme:16s} {CLASSES[k][0]:24s} {d:5d}/{n:<5d} {d / n:6.1%}")
        if d < SHARE * n:
            failures.append(rows[-1])
    assert not failures, "wrong schemes numpy agrees with too often:\n" + "\n".join(failures) + "\n\nall:\n" + \
        "\n".join(rows)
    # every scheme was put to the test on every class it is distinct on
    for scheme, (_, _, first_class) in SCHEMES.items():
        for k in range(first_class, len(CLASSES)):
            assert (scheme, k) in seen, (scheme, CLASSES[k][0])
