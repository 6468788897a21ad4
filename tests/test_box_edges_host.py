"""A pass of tests/test_objboxes_edges_gpu.py and tests/test_boxes_edges_gpu.py only means something if the inputs of
tests/box_edges.py hold the edges they promise and if a wrong kernel would change the expected bytes on those very inputs.
On the CPU:
  - the edges are counted: octants, straddled axes, denormal extremes, kept zero rows of both signs and which is last,
    removed zero rows after the last kept one, zero rows in different lane strides and chunks, object sizes around every
    list length, empty objects, objects and segments beyond 65535, chunk boundaries, each branch of the cell rule,
    wavefronts mixing filtered and unfiltered objects, the class list's limits;
  - mutated restatements (small variants written here, not switches of the shipped one) change the expected bytes: zero
    extremes by IEEE total order, the first zero row wins, removed rows count for the sign, avg >= 0 kept, avg <= threshold
    kept, n for n - 1 under the root, k - 1 and k + 1 neighbours, np.sum for the running sum of roots, the statistics summed
    in plain row order, an empty object taking its neighbour's rows;
  - numpy's own zero rule (the expected boxes are numpy's min / max) is asserted for float32 and float64, so another numpy
    build fails here and not on the GPU."""
import numpy as np
import pytest

import box_edges as BE
import neighbour_restate as NR
import objbox_restate as OR

K = 20
_BRUTE = {}


def neg(x):
    return np.signbit(x)


def _keep(p, k=K):
    if len(p) < k:
        return np.ones(len(p), bool)
    avg = BE.avg_of(np.asarray(p, np.float64), k, _BRUTE)
    return BE.keep_of(avg, BE.object_stats(avg)[1])


# ---- edge counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_signed_objects_hold_every_octant_straddle_and_denormal(dtype):
    objs, edges, kinds = BE.signed_objects(dtype)
    assert edges == {"octants": 7, "straddle_axes": [1, 2, 3], "denormal": 2, "filtered": 11, "unfiltered": 11}
    seen, straddled = set(), set()
    for p, (kind, what, m) in zip(objs, kinds):
        assert len(p) == m and np.array_equal(p.astype(dtype).astype(np.float64), p)      # the same numbers in float32
        allneg, allpos = (p < 0).all(0), (p > 0).all(0)
        if kind == "octant":
            assert (allneg | allpos).all() and allneg.any()
            seen.add((tuple(allneg), m >= K))
        elif kind == "straddle":
            mixed = ~allneg & ~allpos
            assert mixed.sum() == what and not (p == 0).any()
            straddled.add((what, m >= K))
        else:
            assert allneg.all()
            tiny = np.finfo(dtype).smallest_subnormal
            kp = p[_keep(p)]
            assert (kp.max(0) == -tiny).all() and (kp.max(0) > -np.finfo(dtype).tiny).all()
            assert (np.sort(kp, 0)[-2] == -2 * tiny).all()
    assert len(seen) == 14 and straddled == {(a, f) for a in (1, 2, 3) for f in (True, False)}


def test_zero_objects_hold_the_promised_zero_rows():
    objs, _, kinds = BE.zero_objects()
    count = {}
    for p, (axis, side, last, m, removed) in zip(objs, kinds):
        assert len(p) == m
        keep = _keep(p)
        x = p[:, axis]
        zeros = np.flatnonzero(x == 0)
        kz = zeros[keep[zeros]]
        assert neg(x[kz]).any() and not neg(x[kz]).all(), "kept zero rows of both signs"
        lo, hi = BE.numpy_extremes(p, keep)
        if side == "inner":                                # zero rows, but the extremes are not zero
            assert len(kz) == 3 and lo[axis] < 0 < hi[axis]
            continue
        assert neg(x[kz[-1]]) == (last < 0) and neg(x[kz[0]]) != (last < 0)
        ext = lo[axis] if side == "min" else hi[axis]
        assert ext == 0 and neg(ext) == (last < 0), "the extreme is the last kept zero row's zero"
        other = hi[axis] if side == "min" else lo[axis]
        assert other != 0 and (other > 0) == (side == "min")
        if removed:
            assert zeros[-1] == m - 1 and not keep[-1] and neg(x[-1]) != (last < 0) and len(kz) == len(zeros) - 1
        else:
            assert len(kz) == len(zeros)
        if m == 700:                                       # detection: lane j % 256, turn j // 256; annotation: chunks of 3
            assert len(set(kz // BE.LANES)) == 3 and len(set(kz // 3)) == 4 and -(-m // 256) == 3
            assert kz[0] % BE.LANES != kz[-1] % BE.LANES and kz[0] // BE.LANES != kz[-1] // BE.LANES
        key = (axis, side, last, "removed" if removed else ("unfiltered" if m < K else m))
        count[key] = count.get(key, 0) + 1
    assert len(count) == 3 * 2 * 2 * 4 and set(count.values()) == {1}


def test_list_length_objects_and_equal_avg():
    for k in BE.LIST_LENGTHS:
        objs, edges = BE.list_length_objects(k)
        assert edges["sizes"] == [k - 1, k, k + 1, 300, 1, 256]
    assert BE.LIST_LENGTHS == (1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 21, 24, 25, 32)
    pts, off = BE.concat(BE.list_length_objects(1)[0])
    b, avg, keep, _ = BE.expected_objects(pts, off, 1)
    assert (avg == 0).all() and not keep.any() and (b["filtered"][1:] == 1).all() and b["num_points"][0] == 0
    one = np.flatnonzero(b["num_points"] == 1)
    assert len(one) == 2 and np.isnan(b["threshold"][one]).all() and (b["mean"][one] == 0).all()
    p = BE.equal_avg_object()
    avg = BE.avg_of(p, 2)
    assert (avg == 0.125).all()
    assert BE.object_stats(avg) == (0.125, 0.125) and BE.instance_stats(avg) == (0.125, 0.125)
    assert not BE.keep_of(avg, 0.125).any()


def test_tables_many_objects_and_chunks():
    t, edges = BE.table_objects()
    assert edges == {"single": [], "empty_runs_1": [0, 3, 6], "empty_runs_3": [0, 1, 2, 5, 6, 7, 10, 11, 12]}
    assert [len(o) for o in t["single"]] == [300]
    assert [len(o) for o in t["empty_runs_1"]] == [0, 40, 5, 0, 300, 25, 0]
    assert [len(o) for o in t["empty_runs_3"]] == [0, 0, 0, 40, 5, 0, 0, 0, 300, 25, 0, 0, 0]
    for S in (65535, 65536, 65540):
        pts, off, e = BE.many_objects(S)
        m = np.diff(off)
        assert len(m) == S > 65534 and len(pts) == off[-1] == e["rows"] < 70_000
        assert e["filtered"] == sorted({0, 65534, 65535, 65536, S - 1} & set(range(S))) and (m[e["filtered"]] == 40).all()
        # 65534, 65535 and 65536 are neighbours: the empty objects flank every run of filtered ones
        assert (m[e["empty"]] == 0).all() and all(any(j in e["empty"] for j in (i - 1, i + 1)) or
                                                  all(j in e["filtered"] or j == S for j in (i - 1, i + 1))
                                                  for i in e["filtered"])
        assert ((m == 1).sum() + len(e["filtered"]) + len(e["empty"])) == S
        b = BE.expected_objects(pts, off, K)[0]
        assert (b["num_kept"][e["filtered"]] > 30).all()
    (small, large), edges = BE.chunk_objects()
    assert edges["rows"] == [255, 256, 257, 511, 512, 513, 65535, 65536, 65537]
    assert edges["chunk"] == [1, 1, 2, 2, 2, 3, 256, 256, 257]
    assert [len(o) for o in small] == [255, 256, 257, 511, 512, 513]
    assert [len(o) for o in large] == [65535, 65536, 65537] and sum(len(o) for o in large) < 200_000
    assert [-(-len(o) // 256) for o in large] == [256, 256, 257]
    p = large[2]
    assert neg(p[0, 2]) and p[0, 2] == 0 and not neg(p[256, 2]) and p[256, 2] == 0       # lane 0's two rows of chunk 0
    for o in small + large:
        z = np.flatnonzero(o[:, 2] == 0)
        assert len(z) >= 2 and (o[:, 2] >= 0).all() and neg(o[z, 2]).any() and not neg(o[z[-1], 2])


def _cell_rule(p, k=K):
    """The branch of the cell rule an object takes at cell_size 0."""
    ext = p.max(0) - p.min(0)
    area = max(ext[0] * ext[1], ext[1] * ext[2], ext[0] * ext[2])
    h = np.sqrt(area * k / len(p)) if area > 0 else (ext.max() * k / len(p) if ext.max() > 0 else 1.0)
    return ("sheet" if area > 0 else "line" if ext.max() > 0 else "point"), bool(ext.max() / 1024.0 > h)


def test_degenerate_objects_take_every_branch_of_the_cell_rule():
    d, edges = BE.degenerate_objects()
    assert edges == {"identical": 40, "coincident_in_300": 300, "axis_line": 200, "axis_plane": 400, "mm_and_km": 1001,
                     "lattice": 1728, "decimal_lattice": 1728}
    assert set(d) == {"identical", "coincident_in_300", "axis_line", "axis_plane", "mm_and_km", "lattice", "decimal_lattice"}
    assert _cell_rule(d["identical"][0]) == ("point", False) and not _keep(d["identical"][0]).any()
    p = d["coincident_in_300"][0]
    avg = BE.avg_of(p, K, _BRUTE)
    assert len(p) == 300 and (avg == 0).sum() == 20 and _keep(p).sum() > 250
    assert _cell_rule(d["axis_line"][0]) == ("line", False) and _cell_rule(d["axis_plane"][0]) == ("sheet", False)
    assert ((d["axis_plane"][0].max(0) - d["axis_plane"][0].min(0)) == 0).sum() == 1
    p = d["mm_and_km"][0]
    assert _cell_rule(p) == ("sheet", True) and len(p) == 1001 and (np.delete(p, 500, 0).max(0) < 1e-3).all()
    assert p[500, 0] == 1000.0 and not _keep(p)[500] and _keep(p).sum() == 1000
    assert np.array_equal(d["lattice"][0], NR.lattice()) and np.array_equal(d["decimal_lattice"][0], NR.decimal_lattice())
    assert d["lattice"][1] == 0.25 and d["decimal_lattice"][1] == 0.1


def test_mixed_waves_overlap():
    objs, edges = BE.mixed_wave_objects()
    assert edges == {"filtered": 315, "unfiltered": 285}
    assert [len(o) for o in objs] == [1 + s % 40 for s in range(600)]
    lo, hi = np.array([o.min(0) for o in objs]), np.array([o.max(0) for o in objs])
    both = np.flatnonzero([len(a) >= 10 and len(b) >= 10 for a, b in zip(objs[:-1], objs[1:])])
    assert len(both) > 400 and (lo[both + 1] < hi[both]).all() and (lo[both] < hi[both + 1]).all(), \
        "neighbouring objects overlap in space"
    mixed = [s for s in range(599) if (len(objs[s]) >= K) != (len(objs[s + 1]) >= K)]
    assert len(mixed) == 29 and all((lo[s + 1] < hi[s]).all() or len(objs[s + 1]) == 1 for s in mixed)
    assert sum(len(o) >= K for o in objs) == 315 and sum(len(o) < K for o in objs) == 285


def test_instance_cases_hold_the_class_list_and_size_edges():
    c = BE.instance_cases()
    p, sem, ins, classes, mp, k, _ = c["signed"]
    assert classes == [5, 0, 0xFFFF, 9, 10, 11] and {0, 0xFFFF} <= set(sem.tolist()) and 9 not in sem
    assert {1, 65535} <= set(ins.tolist()) and (ins == 0).sum() > 100
    zero = np.flatnonzero(ins == 0)
    assert (ins[zero - 1] != 0).all() and (np.diff(zero) == 6).all(), "ignored rows interleave with kept ones"
    assert len(c["one_class"][3]) == 1 and len(c["64_classes"][3]) == 64 == len(set(c["64_classes"][3]))
    assert not c["every_row_ignored"][2].any() and len(c["every_row_ignored"][0]) > 400
    for (mp, k), want in {(5, 20): [4, 5, 19, 20, 21], (20, 20): [19, 20, 19, 20, 21], (30, 20): [29, 30, 19, 20, 21],
                          (1, 20): [1, 19, 20, 21], (1, 1): [1, 1, 2]}.items():
        assert BE.size_instances(mp, k)[1] == want + [255, 256, 257, 513]
        assert c[f"sizes_mp{mp}_k{k}"][4:6] == (mp, k)
    for k in BE.LIST_LENGTHS:
        assert c[f"k{k:02d}"][5] == k
    for name in BE.degenerate_objects()[0]:
        assert "deg_" + name in c
    # the zero-extreme instances keep their row order: positions in the instance are the object's rows
    p, sem, ins = c["zero_extremes"][:3]
    objs = BE.zero_objects()[0]
    labels = BE.labelled(objs)
    for (s, i, o) in labels[:5]:
        assert np.array_equal(p[(sem == s) & (ins == i)].astype(np.float64), o)
    p, sem, ins, classes, big = BE.many_segments()
    b = BE.expected_instances(p, sem, ins, classes, 1, K)[0]
    assert len(b) == 70400 and len(p) < 71_000 and (b["num_points"] == 40).sum() == 3
    assert [(int(b["sem"][j]), int(b["ins"][j])) for j in (0, -1)] == [big[0], big[2]] and b["num_points"][0] == 40
    mid = int(np.flatnonzero((b["sem"] == big[1][0]) & (b["ins"] == big[1][1]))[0])
    assert 30_000 < mid < 40_000 and b["num_points"][mid] == 40 and b["num_points"][-1] == 40


# ---- numpy's rule, and the rule against numpy on every input ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_min_and_max_take_the_last_zero_row(dtype):
    rng = np.random.default_rng(0)
    for n in (2, 3, 4, 7, 8, 9, 16, 17, 255, 256, 257, 1000, 70_000):
        for last in (0.0, -0.0):
            a = rng.uniform(0.5, 1.5, (n, 3)).astype(dtype)
            rows = np.unique(rng.integers(0, n, 6))
            a[rows, :] = np.array(-last, dtype)
            a[rows[-1], :] = np.array(last, dtype)
            assert (neg(a.min(0)) == neg(last)).all() and (a.min(0) == 0).all(), (n, last)
            assert (neg((-a).max(0)) != neg(last)).all() and ((-a).max(0) == 0).all(), (n, last)
            keep = np.ones(n, bool)
            keep[rng.integers(0, n, n // 3)] = False
            keep[rows] = True
            assert (neg(a[keep].min(0)) == neg(last)).all(), (n, last)


def _object_blobs(parts=BE.Parts, names=None):
    out = {}
    for name, (objs, k, _) in BE.object_cases().items():
        if names is None or name in names:
            pts, off = BE.concat(objs)
            out[name] = b"".join(a.tobytes() for a in BE.expected_objects(pts, off, k, cache=_BRUTE, parts=parts))
    return out


def _instance_blobs(parts=BE.Parts, names=None):
    out = {}
    for name, (p, sem, ins, classes, mp, k, _) in BE.instance_cases().items():
        if names is None or name in names:
            out[name] = b"".join(a.tobytes() for a in BE.expected_instances(p, sem, ins, classes, mp, k, cache=_BRUTE,
                                                                             parts=parts))
    return out


SMALL = ("signed", "zero_extremes", "k02", "k20", "empty_runs_1", "deg_coincident_in_300", "chunks_small")


def test_the_zero_rule_is_numpys_on_every_input():
    class Rule(BE.Parts):
        extremes = staticmethod(BE.zero_rule)
    names = [n for n in BE.object_cases() if n != "chunks_large"]
    assert _object_blobs(Rule, names) == _object_blobs(BE.Parts, names)
    assert _instance_blobs(Rule) == _instance_blobs()
    for o in BE.chunk_objects()[0][1]:
        keep = np.ones(len(o), bool)
        assert all(np.array_equal(BE.bits(a), BE.bits(b)) for a, b in zip(BE.zero_rule(o, keep), BE.numpy_extremes(o, keep)))


# ---- mutants ----------------------------------------------------------------------------------------------------------
def _zero_variant(pick):
    """extremes with the zero chosen by pick(zeros of the axis among the kept rows, zeros among all rows, keep, side)."""
    def extremes(p, keep):
        lo, hi = BE.numpy_extremes(p, keep)
        lo, hi = lo.copy(), hi.copy()
        for c in range(3):
            x = p[:, c]
            allz = np.flatnonzero(x == 0)
            kz = allz[keep[allz]]
            if len(kz) and lo[c] == 0:
                lo[c] = pick(x, kz, allz, "min")
            if len(kz) and hi[c] == 0:
                hi[c] = pick(x, kz, allz, "max")
        return lo, hi
    return staticmethod(extremes)


class TotalOrder(BE.Parts):
    extremes = _zero_variant(lambda x, kz, allz, side: (x[kz].dtype.type(-0.0) if neg(x[kz]).any() else x[kz[0]])
                             if side == "min" else (x[kz].dtype.type(0.0) if not neg(x[kz]).all() else x[kz[0]]))


class FirstZero(BE.Parts):
    extremes = _zero_variant(lambda x, kz, allz, side: x[kz[0]])


class RemovedCount(BE.Parts):
    extremes = _zero_variant(lambda x, kz, allz, side: x[allz[-1]])


class KeepZeroAvg(BE.Parts):
    keep = staticmethod(lambda avg, thr: (avg >= 0) & (avg < thr))


class KeepAtThreshold(BE.Parts):
    keep = staticmethod(lambda avg, thr: (avg > 0) & (avg <= thr))


def _stats(total, denom):
    def stats(avg, std_ratio=BE.STD_RATIO):
        n = len(avg)
        pos = avg > 0
        mean = total(np.where(pos, avg, 0.0)) / np.float64(n)
        d = avg - mean
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(mean), float(mean + std_ratio * np.sqrt(total(np.where(pos, d * d, 0.0)) / np.float64(denom(n))))
    return staticmethod(stats)


class NUnderTheRoot(BE.Parts):
    object_stats = _stats(OR.fixed_sum, lambda n: n)
    instance_stats = _stats(BE.lane_tree_sum, lambda n: n)


class RowOrderSums(BE.Parts):
    object_stats = _stats(lambda v: np.cumsum(v)[-1], lambda n: n - 1)
    instance_stats = object_stats


class OneNeighbourLess(BE.Parts):
    avg = staticmethod(lambda p, k, cache=None: BE.avg_of(p, k - 1, cache) if k > 1 else BE.avg_of(p, k, cache) + 1.0)


class OneNeighbourMore(BE.Parts):
    avg = staticmethod(lambda p, k, cache=None: BE.avg_of(p, k + 1, cache) if k < 32 else BE.avg_of(p, k, cache) + 1.0)


class PairwiseSum(BE.Parts):
    @staticmethod
    def avg(p, k, cache=None):
        assert len(p) <= BE.BRUTE_MAX
        return np.sqrt(NR.Brute(p).d2[:, :k]).sum(1) / k


class EmptyTakesNeighbour(BE.Parts):
    @staticmethod
    def rows_of(off, s):
        while off[s] == off[s + 1] and s + 2 < len(off):
            s += 1
        return int(off[s]), int(off[s + 1])


def test_the_unmutated_parts_restate_the_same_bytes():
    """The mutants' scaffolding (_stats with the right sums, _zero_variant with the right row) gives the shipped bytes."""
    class Same(BE.Parts):
        object_stats = _stats(OR.fixed_sum, lambda n: n - 1)
        instance_stats = _stats(BE.lane_tree_sum, lambda n: n - 1)
        extremes = _zero_variant(lambda x, kz, allz, side: x[kz[-1]])
    assert _object_blobs(Same, SMALL) == _object_blobs(BE.Parts, SMALL)
    assert _instance_blobs(Same, SMALL) == _instance_blobs(BE.Parts, SMALL)


MUTANTS = {"total_order": (TotalOrder, "zero_extremes"), "first_zero_row": (FirstZero, "zero_extremes"),
           "removed_rows_count": (RemovedCount, "zero_extremes"), "avg_ge_0_kept": (KeepZeroAvg, "deg_coincident_in_300"),
           "avg_le_thr_kept": (KeepAtThreshold, "k02"), "n_under_the_root": (NUnderTheRoot, "k20"),
           "row_order_sums": (RowOrderSums, "k20"), "k_minus_1": (OneNeighbourLess, "k20"),
           "k_plus_1": (OneNeighbourMore, "k20"), "np_sum": (PairwiseSum, "k20")}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_changes_the_expected_bytes_of_both_families(name):
    parts, case = MUTANTS[name]
    assert _object_blobs(parts, (case,)) != _object_blobs(BE.Parts, (case,)), "annotation boxes do not notice"
    assert _instance_blobs(parts, (case,)) != _instance_blobs(BE.Parts, (case,)), "detection boxes do not notice"


def test_zero_mutants_differ_on_min_and_on_max_of_every_axis():
    """Each zero mutant changes an extreme for min and for max on each axis, not just somewhere."""
    objs, _, kinds = BE.zero_objects()
    for parts in (TotalOrder, FirstZero, RemovedCount):
        hit = set()
        for p, (axis, side, last, m, removed) in zip(objs, kinds):
            if side == "inner":
                continue
            keep = _keep(p)
            want, got = BE.numpy_extremes(p, keep), parts.extremes(p, keep)
            j = 0 if side == "min" else 1
            if BE.bits(want[j])[axis] != BE.bits(got[j])[axis]:
                hit.add((axis, side))
        assert len(hit) == 6, (parts.__name__, hit)


def test_empty_object_mutant_changes_the_expected_bytes():
    for case in ("empty_runs_1", "empty_runs_3", "k01"):
        assert _object_blobs(EmptyTakesNeighbour, (case,)) != _object_blobs(BE.Parts, (case,))
