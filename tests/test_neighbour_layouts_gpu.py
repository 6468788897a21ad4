"""GPU: the three cell-grid neighbour walks against the brute force of tests/neighbour_restate.py on clouds where
distances tie, neighbourhoods are symmetric, an axis of the grid has one cell and shells are empty:
  outlier filter  lidarcast.preprocess_cloud(estimate_normals=False)   csrc/lrc_knn64.h knn_avg
  normals         lidarcast.preprocess_cloud(remove_outliers=False)    csrc/lrc_preprocess.hip pp_nbr_kernel / pp_pca_kernel
  1-NN            lidarcast.NearestIndex                               csrc/lrc_nn.hip nn_query_kernel
  detection boxes lidarcast.instance_boxes(return_rows=True)           csrc/lrc_boxes.hip box_knn_kernel
Every case runs at several cell sizes, one of them the spacing of the cloud itself where it has one (rows sit on cell
edges): no result byte may depend on the grid.  tests/test_neighbour_layouts_host.py shows that the criteria used here
reject a wrong tie rule, a wrong radius test and the wrong eigenvector of a diagonal covariance."""
import functools

import numpy as np
import pytest

import neighbour_restate as nr
from helpers import bits

pytestmark = pytest.mark.gpu

UP = float(np.nextafter(0.5, 1))
# layout -> (builder, cell sizes after 0.0: fine ones first (the cloud's own spacing where it has one), a coarse one last,
#            radii of the normal search)
LAYOUTS = {
    "lattice": (nr.lattice, (0.25, 0.1, 3.0), (0.6, 0.5, UP)),
    "decimal_lattice": (nr.decimal_lattice, (0.1, 0.03, 2.0), (0.25,)),
    "two_clusters": (nr.two_clusters, (0.25, 8.0), (0.05,)),
    "axis_line": (nr.axis_line, (0.0005, 0.5), (0.05,)),
    "diagonal_line": (nr.diagonal_line, (0.05, 2.0), (0.1,)),
    "mm_plane": (nr.mm_plane, (0.01, 0.7), (0.05, 0.1)),
    "identical": (nr.identical, (0.001, 10.0), (0.1,)),
    "identical_far": (functools.partial(nr.identical, far=True), (0.01, 10.0), (0.1,)),
    "pole": (nr.pole, (0.25, 0.1, 1.0), (0.6,)),
    "mm_cube": (nr.mm_cube, (0.01, 0.4), (0.05, 0.1)),
}
NB_NEIGHBORS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 21, 24, 25, 32)       # every list length and the first value past it
MAX_NN = (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 30, 32)
PERMUTED = [("lattice", 1), ("lattice", 2), ("decimal_lattice", 1), ("decimal_lattice", 2)]
CASES = [(name, 0) for name in LAYOUTS] + PERMUTED


@functools.lru_cache(maxsize=None)
def brute(name, seed=0):
    """The layout and its brute force, computed once for all tests of the module."""
    build = LAYOUTS[name][0]
    p = build(seed=seed) if seed else build()
    assert p.dtype == np.float64 and p.shape[1] == 3 and len(p) <= 4096
    return p, nr.Brute(p)


def cells(name):
    return (0.0,) + LAYOUTS[name][1]


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


# ---- outlier filter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_outlier_filter_equals_the_brute_force(ctx, name):
    from lidarcast import preprocess_cloud
    p, b = brute(name)
    n = len(p)
    for k in NB_NEIGHBORS:
        want = b.avg(k)
        mean, thr = nr.restate_filter(want, 2.0)
        pos = want[want > 0]
        # input condition: no avg sits within 1e-9 of the threshold.  It cannot hold where all positive avg agree to
        # 1e-9 (a lattice at k <= 4, a line at k = 2: std is rounding noise, threshold == mean == avg); there `kept`
        # below is still exact, because it is judged with the device's own threshold.
        if len(pos) and pos.max() - pos.min() > 1e-9 * thr:
            assert (np.abs(pos - thr) > 1e-9 * thr).all(), (name, k)
        for cs in cells(name):
            r = preprocess_cloud(ctx, p, nb_neighbors=k, std_ratio=2.0, estimate_normals=False, cell_size=cs)
            assert np.array_equal(bits(r.avg), bits(want)), (name, k, cs)
            assert abs(r.mean - mean) <= 1e-12 * abs(mean) and abs(r.threshold - thr) <= 1e-12 * abs(thr), (name, k, cs)
            assert np.array_equal(r.kept.astype(np.int64), np.flatnonzero((want > 0) & (want < r.threshold))), (name, k, cs)
        if name == "identical":
            assert (want == 0.0).all() and len(r.kept) == 0
        if name == "identical_far":
            assert (want[:40] == 0.0).all() and len(r.kept) == 0
            assert want[40] > 0.0 if k > 1 else want[40] == 0.0
    assert n == len(want)


# ---- normals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, seed", CASES)
def test_normals_meet_the_criterion_on_every_row(ctx, name, seed):
    from lidarcast import preprocess_cloud
    p, b = brute(name, seed)
    worst = 0.0
    for radius in LAYOUTS[name][2]:
        for max_nn in MAX_NN:
            restated = b.neighbours(radius, max_nn)
            first = None
            for cs in cells(name):
                r = preprocess_cloud(ctx, p, remove_outliers=False, radius=radius, max_nn=max_nn, cell_size=cs)
                if first is None:
                    first = r
                    worst = max(worst, nr.check_normals_all(r.normals, r.nn_count, p, radius, max_nn, restated))
                else:
                    assert r.normals.tobytes() == first.normals.tobytes(), (name, radius, max_nn, cs)
                    assert r.nn_count.tobytes() == first.nn_count.tobytes(), (name, radius, max_nn, cs)
    print(f"\n[neighbours] {name} (row order {seed}): largest Rayleigh excess over {len(p)} rows, "
          f"{len(LAYOUTS[name][2])} radii, {len(MAX_NN)} list lengths: {worst:.3g}")


def test_pole_axis_rows_get_an_eigenvector_of_the_smallest_eigenvalue(ctx):
    """covariance diag(s, s, L), s < L: the diagonal branch of smallest_eigvec answers (1, 0, 0)."""
    from lidarcast import estimate_normals
    p, b = brute("pole")
    rows = nr.pole_interior(p)
    n = estimate_normals(ctx, p, 0.6, 32)
    assert np.array_equal(n[rows], np.tile([[1.0, 0.0, 0.0]], (len(rows), 1)))
    assert nr.check_normals_all(n, b.neighbours(0.6, 32)[0], p, 0.6, 32) <= nr.RAYLEIGH_BOUND


def test_lattice_radius_is_strict(ctx):
    from lidarcast import preprocess_cloud
    p, _ = brute("lattice")
    k = np.rint(p / 0.25)
    interior = ((k >= 2) & (k <= 9)).all(1)
    for cs in cells("lattice"):
        at = preprocess_cloud(ctx, p, remove_outliers=False, radius=0.5, max_nn=32, cell_size=cs).nn_count
        above = preprocess_cloud(ctx, p, remove_outliers=False, radius=UP, max_nn=32, cell_size=cs).nn_count
        assert (at[interior] == 27).all() and (above[interior] == 32).all(), cs


@pytest.mark.parametrize("name", ["two_clusters", "lattice"])
def test_both_stages_on_tied_data(ctx, name):
    from lidarcast import estimate_normals, preprocess_cloud
    p, b = brute(name)
    radius = LAYOUTS[name][2][0]
    first = None
    for cs in cells(name):
        r = preprocess_cloud(ctx, p, nb_neighbors=20, std_ratio=2.0, radius=radius, max_nn=30, cell_size=cs)
        want = b.avg(20)
        assert np.array_equal(bits(r.avg), bits(want))
        assert np.array_equal(r.kept.astype(np.int64), np.flatnonzero((want > 0) & (want < r.threshold)))
        assert 0 < len(r.kept) < len(p)
        pk = p[r.kept]
        assert r.normals.tobytes() == estimate_normals(ctx, pk, radius, 30, cell_size=cs).tobytes()
        if first is None:
            first = r
            nr.check_normals_all(r.normals, r.nn_count, pk, radius, 30)
        else:
            assert r.normals.tobytes() == first.normals.tobytes() and r.nn_count.tobytes() == first.nn_count.tobytes()


# ---- 1-NN -----------------------------------------------------------------------------------------------------------
def outside_queries(p):
    """Beyond each of the 6 faces and 8 corners of the cloud's box, 0.1, 10 and 1e4 away."""
    lo, hi = p.min(0), p.max(0)
    mid = 0.5 * (lo + hi)
    out = []
    for dist in (0.1, 10.0, 1.0e4):
        for a in range(3):
            for side in (0, 1):
                q = mid.copy()
                q[a] = hi[a] + dist if side else lo[a] - dist
                out.append(q)
        for corner in range(8):
            out.append([hi[a] + dist if (corner >> a) & 1 else lo[a] - dist for a in range(3)])
    return np.array(out)


def lattice_midpoints(spacing=0.25, side=12):
    """Cell centres (8 rows tie), face midpoints (4) and edge midpoints (2) of lattice(): exact in float32."""
    k = np.arange(side) * spacing
    h = k[:-1] + 0.5 * spacing
    out = []
    for axes in ((h, h, h), (k, h, h), (h, k, h), (h, h, k), (h, k, k), (k, h, k), (k, k, h)):
        out.append(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3))
    return np.vstack(out)


@functools.lru_cache(maxsize=None)
def nn_queries(name):
    p, _ = brute(name)
    lo, hi = p.min(0), p.max(0)
    span = np.maximum(hi - lo, 0.01)
    rng = np.random.default_rng(7)
    parts = [p, outside_queries(p), rng.uniform(lo - 0.2 * span, hi + 0.2 * span, (1000, 3))]
    if name == "lattice":
        parts.append(lattice_midpoints())
    q = np.ascontiguousarray(np.vstack(parts), dtype=np.float32)
    return q, nr.nearest(p, q)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_nearest_equals_the_brute_force(ctx, name):
    import lidarcast
    p, _ = brute(name)
    q, (widx, wdist) = nn_queries(name)
    if name in ("lattice", "pole"):                              # exact in float32: the row itself
        assert np.array_equal(widx[:len(p)], np.arange(len(p))) and (wdist[:len(p)] == 0.0).all()
    if name == "identical":                                      # the lowest duplicate
        assert (widx[:len(p)] == 0).all()
    if name == "lattice":
        d = nr.d2(q[-1331 - 4356 - 4752:].astype(np.float64), p)
        ties = (d == d.min(1, keepdims=True)).sum(1)
        assert (ties[:1331] == 8).all() and (ties[1331:1331 + 4356] == 4).all() and (ties[1331 + 4356:] == 2).all()
    for cs in cells(name):
        index = lidarcast.NearestIndex(ctx, p, cell_size=cs)
        idx, dist = index.query(q, return_distance=True)
        index.close()
        assert np.array_equal(idx.astype(np.int64), widx), (name, cs)
        assert np.array_equal(bits(dist), bits(wdist)), (name, cs)


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_nearest_query_counts_off_the_block_size(ctx, count):
    import lidarcast
    p, _ = brute("lattice")
    q, (widx, wdist) = nn_queries("lattice")
    q, widx, wdist = q[-count:], widx[-count:], wdist[-count:]      # edge midpoints: every answer a tie
    index = lidarcast.NearestIndex(ctx, p, cell_size=0.25)
    idx, dist = index.query(np.ascontiguousarray(q), return_distance=True)
    index.close()
    assert np.array_equal(idx.astype(np.int64), widx) and np.array_equal(bits(dist), bits(wdist))


def test_nearest_on_a_grid_cut_down_by_the_cell_cap(ctx):
    import lidarcast
    p, _ = brute("mm_cube")
    n, h, rounds = nr.nn_grid(p, 1.0e-4)
    assert rounds >= 1 and 32.0e6 < float(n.prod()) <= 64.0e6 and h > 0.5 / 1024.0     # the h *= 1.26 loop ran
    # queries inside the box only, and few: on this grid a query outside the box visits every one of the ~64 M cells
    # before it may stop, a performance cliff that this test is not about
    q = np.random.default_rng(9).uniform(0.01, 0.49, (256, 3)).astype(np.float32)
    assert (q > p.min(0)).all() and (q < p.max(0)).all()
    widx, wdist = nr.nearest(p, q)
    index = lidarcast.NearestIndex(ctx, p, cell_size=1.0e-4)
    idx, dist = index.query(q, return_distance=True)
    index.close()
    assert np.array_equal(idx.astype(np.int64), widx) and np.array_equal(bits(dist), bits(wdist))


# ---- detection boxes ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_case(name, k, split, min_points=10):
    """The float32 cloud, its instance ids (split: instances of k - 1, k and the remaining rows; else one instance) and,
    by the rule of include/lidarcast.h "detection boxes", the restated avg per row, the rows kept unfiltered and per
    filtered instance (rows, mean, threshold); avg is the brute force over the float32 values widened to float64."""
    p32 = np.ascontiguousarray(brute(name)[0], dtype=np.float32)
    ins = np.ones(len(p32), np.uint16)
    if split:
        ins[:] = 3
        ins[:k - 1] = 1
        ins[k - 1:2 * k - 1] = 2
    avg = np.full(len(p32), -1.0)
    whole = np.zeros(len(p32), np.uint8)
    filtered = {}
    for iid in np.unique(ins):
        rows = np.flatnonzero(ins == iid)
        if len(rows) < min_points:
            continue
        if len(rows) < k:
            whole[rows] = 1
            continue
        avg[rows] = nr.Brute(p32[rows].astype(np.float64)).avg(k)
        filtered[int(iid)] = (rows,) + nr.restate_filter(avg[rows], 2.0)
    return p32, ins, avg, whole, filtered


@pytest.mark.parametrize("k", [1, 20, 32])
@pytest.mark.parametrize("name", ["lattice", "two_clusters", "axis_line"])
def test_detection_boxes_equal_the_brute_force(ctx, name, k):
    import lidarcast
    for split in (False, True):
        p32, ins, wavg, whole, filtered = box_case(name, k, split)
        sem = np.full(len(p32), 7, np.uint16)
        first = None
        for cs in cells(name):
            boxes, avg, keep = lidarcast.instance_boxes(ctx, p32, sem, ins, [7], k=k, std_ratio=2.0, cell_size=cs,
                                                        return_rows=True)
            assert np.array_equal(bits(avg), bits(wavg)), (name, k, cs)
            got = {int(b["ins"]): b for b in boxes}
            wkeep = whole.copy()
            for iid, (rows, mean, thr) in filtered.items():
                b = got[iid]
                assert b["filtered"] == 1
                assert abs(b["mean"] - mean) <= 1e-12 * abs(mean) and abs(b["threshold"] - thr) <= 1e-12 * abs(thr)
                wkeep[rows] = (wavg[rows] > 0) & (wavg[rows] < b["threshold"])
            assert np.array_equal(keep, wkeep), (name, k, cs)
            if split:
                assert (avg[:k - 1] == -1.0).all()
                assert (avg[k - 1:2 * k - 1] == -1.0).all() == (k < 10)         # an instance of exactly k rows is filtered
            blob = boxes.tobytes() + avg.tobytes() + keep.tobytes()
            first = first or blob
            assert blob == first, (name, k, cs)
