"""GPU: min_dist_kernel and rbf_sum_kernel (csrc/lrc_metrics.hip) against tests/metrics_restate.py at every launch edge:
the last row of a partial 1024-row tile of B, a tile boundary, a block of A whose tail threads have no row, long thin
clouds either way, coincident rows and one-ulp neighbours, non-finite coordinates, and input arrays that are not
C-contiguous float32.

  min_distances   bit for bit the float32 restatement min_dist32 (which tests/test_metrics_restate_host.py shows to be
                  numpy's own computation), and within 4 * 2**-24 relative of the float64 reference min_dist64.
  rbf_kernel_sum  within rbf_bound (derived in metrics_restate.rbf_bound) of the long-double direct form rbf64 for gamma
                  0.7 and 10; exactly n * m for gamma 0; exactly n for gamma 1e6 / scale**2 on a lattice cloud against
                  itself.  The long-double reference is the slow part, so each shape meets one of the three scales for
                  gamma 0.7 / 10 (every n and every m meets all three); everything else runs at all three.
The wrong kernels these cases reject are modelled in tests/test_metrics_restate_host.py."""
import numpy as np
import pytest

import metrics_restate as mr
from helpers import bits

pytestmark = pytest.mark.gpu

REL32 = 4 * 2.0 ** -24
WORST = {"min_dist32 vs min_dist64 / (4 * 2**-24)": 0.0, "rbf_kernel_sum vs rbf64 / rbf_bound": 0.0}
IDS = [f"{n}x{m}" for n, m in mr.SHAPES]


@pytest.fixture(scope="module")
def metrics():
    from lidarcast import metrics
    yield metrics
    for k, v in WORST.items():
        print(f"\nworst {k} = {v:.4f}", end="")


def _same(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    ne = bits(got) != bits(want)
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} rows differ, first at {np.flatnonzero(ne)[:5]}"


@pytest.mark.parametrize("n,m", mr.SHAPES, ids=IDS)
def test_planted_nearest_row_is_found(metrics, n, m):
    """B lies 20 spreads from A.  One row of A at a block edge is brought within 1e-3 of one row of B at a tile edge:
    that row answers the planted distance, every other row its own far distance."""
    a, b = mr.far_clouds(n, m)
    far = mr.min_dist32(a, b)
    assert far.min() > 10.0
    _same(metrics.min_distances(a, b), far, "far clouds")
    for i, k in mr.planted_pairs(n, m):
        a2, d = mr.plant(a, b, i, k)
        want = far.copy()
        want[i] = d
        assert d < 1e-3 and bits(mr.min_dist32(a2[i:i + 1], b))[0] == bits(d)
        _same(metrics.min_distances(a2, b), want, f"A[{i}] planted at B[{k}]")


@pytest.mark.parametrize("n,m", mr.SHAPES, ids=IDS)
def test_min_distances_equal_the_restatement_bit_for_bit(metrics, n, m):
    worst = 0.0
    for scale in mr.SCALES:
        a, b = mr.general_clouds(n, m, scale)
        for x, y, tag in ((a, b, "A->B"), (b, a, "B->A")):
            got = metrics.min_distances(x, y)
            _same(got, mr.min_dist32(x, y), f"scale {scale} {tag}")
            ref = mr.min_dist64(x, y)
            zero = ref == 0.0
            assert not bits(got[zero]).any(), "a coincident row is not at +0.0"
            if (~zero).any():
                worst = max(worst, float((np.abs(got[~zero].astype(np.float64) - ref[~zero]) / ref[~zero]).max()))
    k = "min_dist32 vs min_dist64 / (4 * 2**-24)"
    WORST[k] = max(WORST[k], worst / REL32)
    print(f"worst relative error / (4 * 2**-24) = {worst / REL32:.4f}")
    assert worst <= REL32


@pytest.mark.parametrize("n,m", mr.SHAPES, ids=IDS)
def test_rbf_kernel_sum_within_the_derived_bound(metrics, n, m):
    idx = mr.SHAPES.index((n, m))
    scale = mr.SCALES[(idx // len(mr.MS) + idx % len(mr.MS)) % 3]
    a, b = mr.general_clouds(n, m, scale)
    worst = 0.0
    for gamma, ref in zip((0.7, 10.0), mr.rbf64(a, b, (0.7, 10.0))):
        got = metrics.rbf_kernel_sum(a, b, gamma)
        assert bits(np.float64(got)) == bits(np.float64(metrics.rbf_kernel_sum(a, b, gamma))), "not repeatable"
        ratio = float(abs(np.longdouble(got) - ref) / ref) / mr.rbf_bound(a, b, gamma)
        print(f"scale {scale} gamma {gamma}: sum {got!r}, error / rbf_bound = {ratio:.4f}")
        worst = max(worst, ratio)
    k = "rbf_kernel_sum vs rbf64 / rbf_bound"
    WORST[k] = max(WORST[k], worst)
    assert worst <= 1.0
    for s in mr.SCALES:
        a, b = mr.general_clouds(n, m, s)
        assert metrics.rbf_kernel_sum(a, b, 0.0) == float(n * m)          # a stale or a skipped row changes the count
        assert metrics.rbf_kernel_sum(b, a, 0.0) == float(n * m)


@pytest.mark.parametrize("n", mr.SQUARE)
def test_rbf_large_gamma_leaves_the_diagonal(metrics, n):
    """A = B with distinct rows at least 0.1 * scale apart: the expanded form is exactly 0 on identical rows and every other
    term underflows far below one ulp of n."""
    for scale in mr.SCALES:
        x = mr.lattice_cloud(n, scale)
        assert metrics.rbf_kernel_sum(x, x, mr.big_gamma(scale)) == float(n), (n, scale)
    x = mr.lattice_cloud(n, 1.0)
    assert metrics.compute_mmd_sampled(x, x) == 0.0
    assert metrics.compute_mmd_sampled(x, x, gamma=mr.big_gamma(1.0)) == 0.0


def test_non_finite_coordinates_propagate_as_in_numpy(metrics):
    nan_rows = nan_sums = 0
    for name, a, b in mr.nonfinite_cases():
        want = mr.min_dist32(a, b)
        got = metrics.min_distances(a, b)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN rows {np.flatnonzero(np.isnan(got))[:5]} " \
                                                              f"expected {np.flatnonzero(np.isnan(want))[:5]}"
        ok = ~np.isnan(want)
        _same(got[ok], want[ok], name)
        nan_rows += int((~ok).sum())
        back = metrics.min_distances(b, a)
        assert np.array_equal(back, mr.min_dist32(b, a), equal_nan=True), name + " (B->A)"
        for gamma in (0.0, 0.7):
            got = metrics.rbf_kernel_sum(a, b, gamma)
            want = mr.rbf_expanded64(a, b, gamma)
            assert np.isnan(got) == np.isnan(want), (name, gamma, got, want)
            assert np.isnan(got) or not mr.rbf64_isnan(a, b, gamma), (name, gamma)      # NaN wherever rbf64 is NaN
            # the same float64 form on both sides: only the orders of summation and exp's rounding differ
            tol = (len(b) + 8 + 3 + 2 + 32) * 2.0 ** -53
            assert np.isnan(got) or abs(got - want) <= tol * want, (name, gamma, got, want)
            nan_sums += bool(np.isnan(want))
    assert nan_rows >= 3 * len(a) and nan_sums > 20          # the cases do hold NaN answers
    a, b = mr.general_clouds(257, 1025, 1.0)                  # a gamma that is not finite: -inf * 0 on coincident rows
    x = mr.lattice_cloud(300, 1.0)
    for gamma in (np.inf, np.nan, -np.inf):
        for p, q in ((a, b), (x, x), (x, x + np.float32(0.0625))):
            got, want = metrics.rbf_kernel_sum(p, q, gamma), mr.rbf_expanded64(p, q, gamma)
            assert np.isnan(got) == np.isnan(want) and (np.isnan(want) or got == want), (gamma, got, want)


def test_input_layouts_give_the_bytes_of_the_plain_call(metrics):
    rng = np.random.default_rng(5)
    a64 = rng.uniform(-3, 3, (600, 3))
    b64 = rng.uniform(-3, 3, (2500, 3))
    a, b = a64.astype(np.float32), b64.astype(np.float32)
    want, want_s = metrics.min_distances(a, b), metrics.rbf_kernel_sum(a, b, 0.7)
    _same(want, mr.min_dist32(a, b), "plain call")
    ro_a, ro_b = a.copy(), b.copy()
    ro_a.setflags(write=False)
    ro_b.setflags(write=False)
    wide_a, wide_b = np.repeat(a, 2, 0), np.repeat(b, 2, 0)
    for tag, x, y in (("float64", a64, b64), ("Fortran order", np.asfortranarray(a), np.asfortranarray(b)),
                      ("every second row", wide_a[::2], wide_b[::2]), ("read-only", ro_a, ro_b),
                      ("list of lists", a.tolist(), b.tolist()),
                      ("column slice", np.hstack([a, a])[:, :3], np.hstack([b, b])[:, 3:])):
        _same(metrics.min_distances(x, y), want, tag)
        assert metrics.rbf_kernel_sum(x, y, 0.7) == want_s, tag
    empty = np.zeros((0, 3), np.float32)
    out = metrics.min_distances(empty, b)
    assert out.shape == (0,) and out.dtype == np.float32
    with pytest.raises(ValueError):
        metrics.min_distances(a, empty)
    assert metrics.rbf_kernel_sum(empty, b, 0.7) == 0.0 and metrics.rbf_kernel_sum(a, empty, 0.7) == 0.0
    assert metrics.rbf_kernel_sum(empty, empty, 0.7) == 0.0
    with pytest.raises(ValueError):
        metrics.min_distances(a[:, :2], b)


def _sample(points, k):
    return points if len(points) <= k else points[np.random.choice(len(points), k, replace=False)]


@pytest.mark.parametrize("fn,k,lx,ly", [("compute_chamfer_distance", 5000, 5000, 5001),
                                        ("compute_chamfer_distance", 5000, 5001, 5000),
                                        ("compute_hausdorff_distance", 3000, 3000, 3001),
                                        ("compute_hausdorff_distance", 3000, 3001, 3000)])
def test_sampling_thresholds_draw_as_the_definition(metrics, fn, k, lx, ly):
    """A cloud of exactly k points is taken whole, one of k + 1 is subsampled with np.random.choice on the global stream,
    X first and then Y; the value is the definition on those draws and the stream ends where the definition leaves it."""
    rng = np.random.default_rng(lx)
    X = rng.uniform(-2, 2, (lx, 3)).astype(np.float32)
    Y = (rng.uniform(-2, 2, (ly, 3)) + 0.01).astype(np.float32)
    state = np.random.get_state()
    try:
        np.random.seed(77)
        got = getattr(metrics, fn)(X, Y)
        after = np.random.random()
        np.random.seed(77)
        Xs, Ys = _sample(X, k), _sample(Y, k)
        assert len(Xs) == len(Ys) == k
        ab, ba = mr.min_dist32(Xs, Ys), mr.min_dist32(Ys, Xs)
        want = float(np.mean(ab) + np.mean(ba)) if "chamfer" in fn else float(max(np.max(ab), np.max(ba)))
        assert got == want and isinstance(got, float)
        assert np.random.random() == after
    finally:
        np.random.set_state(state)
