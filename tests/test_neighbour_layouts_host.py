"""A pass of tests/test_neighbour_layouts_gpu.py only means something if its brute force is the contract and its normals
criterion rejects what it is meant to reject.  On the CPU, on the layouts of tests/neighbour_restate.py:
  - the brute force equals the cKDTree restatement of tests/test_preprocess_gpu.py bit for bit on the control cloud;
  - neighbours chosen with ties broken by the highest index instead of the lowest are rejected by check_normals_all;
  - (0, 0, 1) on a covariance diag(s, s, L), s < L, is rejected and both eigenvectors of s are accepted;
  - the radius test is strict: a shell at exactly d2 == radius^2 is out, and in one float64 step above."""
import numpy as np
import pytest

import neighbour_restate as nr
from test_preprocess_gpu import restate_avg, restate_neighbours


def test_brute_force_equals_the_ckdtree_restatement():
    p = nr.mm_cube()
    b = nr.Brute(p)
    for k in (1, 2, 5, 20, 32):
        assert np.array_equal(b.avg(k).view(np.uint64), restate_avg(p, k).view(np.uint64)), k
    assert np.array_equal(nr.avg(p, 20), b.avg(20))
    rows = np.arange(len(p))
    for radius, max_nn in ((0.05, 30), (0.1, 30), (0.1, 3), (0.03, 32)):
        cnt, idx, cov = b.neighbours(radius, max_nn)
        # spare: with about 100 rows inside 0.1 the 30th must be strictly closer than the last candidate fetched
        wcnt, widx, wcov = restate_neighbours(p, radius, max_nn, rows, spare=120)
        assert np.array_equal(cnt, wcnt) and np.array_equal(idx, widx), (radius, max_nn)
        assert np.array_equal(cov.view(np.uint64), wcov.view(np.uint64)), (radius, max_nn)
    assert (b.neighbours(0.1, 30)[0] == 30).mean() > 0.5 and (b.neighbours(0.05, 30)[0] < 30).all()


@pytest.mark.parametrize("layout, radius, max_nn", [("lattice", 0.6, 10), ("lattice", 0.6, 16),
                                                    ("decimal_lattice", 0.25, 10)])
def test_wrong_tie_rule_is_rejected(layout, radius, max_nn):
    p = getattr(nr, layout)()
    n = len(p)
    right = nr.neighbours(p, radius, max_nn)
    cnt, idx, cov = nr.neighbours(p, radius, max_nn, tie_key=-np.arange(n))          # highest index first among equals
    assert np.array_equal(cnt, right[0])
    differs = (np.sort(idx, 1) != np.sort(right[1], 1)).any(1)
    _, v = np.linalg.eigh(cov)
    wrong = v[:, :, 0]                                   # the normal a walk with the wrong tie rule would hand back
    excess, w = nr.rayleigh_excess(wrong, right[2])
    rejected = differs & (w[:, 2] > 0) & (excess > nr.RAYLEIGH_BOUND)
    print(f"\n[neighbours] {layout} r={radius} max_nn={max_nn}: sets differ on {differs.mean():.1%} of the rows, "
          f"{rejected.sum() / differs.sum():.1%} of those rejected")
    assert differs.mean() >= 0.5
    assert rejected.sum() >= 0.8 * differs.sum()
    with pytest.raises(AssertionError, match="Rayleigh"):
        nr.check_normals_all(wrong, cnt, p, radius, max_nn)
    _, v = np.linalg.eigh(right[2])
    assert nr.check_normals_all(v[:, :, 0], cnt, p, radius, max_nn) <= 1e-12     # and the right rule passes


def test_diagonal_case_is_rejected():
    p = nr.pole()
    rows = nr.pole_interior(p)
    cnt, _, cov = nr.neighbours(p, 0.6, 32)
    _, v = np.linalg.eigh(cov)
    good = v[:, :, 0].copy()
    for axis in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
        n = good.copy()
        n[rows] = axis
        assert nr.check_normals_all(n, cnt, p, 0.6, 32) <= 1e-12
    n = good.copy()
    n[rows] = (0.0, 0.0, 1.0)
    excess, _ = nr.rayleigh_excess(n[rows], cov[rows])
    assert (excess > 0.5).all()                              # (L - s) / L = 0.8 on these rows
    with pytest.raises(AssertionError, match="Rayleigh"):
        nr.check_normals_all(n, cnt, p, 0.6, 32)
    one = good.copy()
    one[rows[0]] = (0.0, 0.0, 1.0)                           # a single wrong row is enough
    with pytest.raises(AssertionError, match="Rayleigh"):
        nr.check_normals_all(one, cnt, p, 0.6, 32)


def test_other_clauses_of_the_criterion_reject():
    p = nr.mm_plane()
    cnt, _, cov = nr.neighbours(p, 0.05, 30)
    _, v = np.linalg.eigh(cov)
    good = np.where((cnt < 3)[:, None], [0.0, 0.0, 1.0], v[:, :, 0])
    assert (cnt < 3).any() and (cnt >= 3).any()
    nr.check_normals_all(good, cnt, p, 0.05, 30)
    bad = cnt.copy()
    bad[7] += 1
    with pytest.raises(AssertionError, match="counts"):
        nr.check_normals_all(good, bad, p, 0.05, 30)
    n = good.copy()
    n[np.flatnonzero(cnt < 3)[0]] = (0.0, 0.0, -1.0)
    with pytest.raises(AssertionError, match="fewer than 3"):
        nr.check_normals_all(n, cnt, p, 0.05, 30)
    n = good.copy()
    n[np.flatnonzero(cnt >= 3)[0]] *= 1.0 + 1e-11
    with pytest.raises(AssertionError):
        nr.check_normals_all(n, cnt, p, 0.05, 30)


def test_radius_is_strict_on_the_lattice():
    p = nr.lattice()
    k = np.rint(p / 0.25)
    interior = ((k >= 2) & (k <= 9)).all(1)
    assert interior.sum() == 8 ** 3
    cnt = nr.neighbours(p, 0.5, 32)[0]
    assert (cnt[interior] == 27).all()                      # the 6 rows at d2 == 0.25 == radius^2 are out
    up = np.nextafter(0.5, 1)
    assert up * up > 0.25
    cnt, idx, _ = nr.neighbours(p, up, 32)
    assert (cnt[interior] == 32).all()                      # 33 inside: max_nn cuts the tied shell at the lowest indices
    d2 = nr.d2(p[interior], p)
    tied = [np.flatnonzero(row == 0.25) for row in d2]
    assert all(len(t) == 6 for t in tied)
    assert all(np.array_equal(np.sort(i[27:]), t[:5]) for i, t in zip(idx[interior], tied))


def test_nearest_takes_the_lowest_index_among_equals():
    p = nr.lattice()
    centre = (p[:1] + 0.125).astype(np.float32)             # a cell centre: 8 rows at the same distance
    if (centre > 2.75).any():
        centre = (p[:1] - 0.125).astype(np.float32)
    idx, dist = nr.nearest(p, centre)
    same = np.flatnonzero(nr.d2(centre.astype(np.float64), p)[0] == 3 * 0.125 ** 2)
    assert len(same) == 8 and idx[0] == same.min() and dist[0] == np.sqrt(3 * 0.125 ** 2)
    dup = nr.identical(far=True)
    assert nr.nearest(dup, dup.astype(np.float32))[0].tolist() == [0] * 40 + [40]
