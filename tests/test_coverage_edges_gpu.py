"""-m gpu: surface coverage and greedy view selection (csrc/lrc_coverage.hip) against the numpy restatement on the edge
inputs of tests/coverage_restate.py, bit for bit: meshes of 1, 31, 32, 33, 1025 and 32769 triangles, pose lengths around
every launch edge of accumulate, runs across the lane and stride boundaries and across a non-returned ray, a dropped
pose, 4096 classes, exact gain ties inside one thread's loop and across threads, S around 1024, a second gain workgroup,
the stop rules, stray bits in an initial cover, and a target hit exactly.
tests/test_voxgrid_coverage_edges_host.py shows on the CPU that the inputs hold these edges and discriminate."""
import numpy as np
import pytest

import coverage_restate as R
from helpers import random_soup
from test_coverage_gpu import _dev

pytestmark = pytest.mark.gpu

Q = 2.0 ** -32


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


def _cov(ctx, v, f, sem=None, S=1):
    from lidarcast import SurfaceCoverage
    return SurfaceCoverage(ctx, v, f, sem, num_sets=S)


_MESHES = {}


def _soup(T):
    """(vertices, triangles, restated q) of the soup of T triangles, restated once."""
    if T not in _MESHES:
        v, f = random_soup(T, seed=T)
        _MESHES[T] = (v, f, R.area_q(v, f))
    return _MESHES[T]


def _equal():
    if "eq" not in _MESHES:
        v, f = R.equal_q_mesh(200)
        _MESHES["eq"] = (v, f, R.area_q(v, f))
    return _MESHES["eq"]


def _write(cov, seen):
    """Write the (S, T) pattern by accumulating one ray per seen triangle (pose k -> set k)."""
    import torch
    t, prim, N = R.seen_records(seen)
    cov.reset()
    cov.accumulate_dev(_dev(t, torch.float32), _dev(prim, torch.int32), seen.shape[0], N)
    bits, _, _ = cov.export()
    assert np.array_equal(bits, R.pack(seen))


def _assert_select(got, rp, rg, total_q, initial_q=0):
    picks, gains_m2, cum = got
    assert list(picks) == rp, (list(picks), rp)
    assert np.array_equal(gains_m2, np.array(rg, np.float64) * Q)
    assert list(cum) == [float(c) / float(total_q) for c in R.cumulative_q(rg, initial_q)]


# ---- accumulate -------------------------------------------------------------------------------------------------------
ACC = [(n, 33) for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)] + \
      [(1025, t) for t in (1, 31, 32, 1025, 32769)]


@pytest.mark.parametrize("N, T", ACC)
def test_accumulate_edges(ctx, N, T):
    import torch
    v, f, q = _soup(T)
    cov = _cov(ctx, v, f, S=2)
    assert cov.words_per_set == (T + 31) // 32 and np.array_equal(cov.area_q(), q)
    assert cov.total_q == sum(int(x) for x in q)
    t, prim = R.edge_records(N, T)
    sop = np.array(R.EDGE_SET_OF_POSE, np.int32)
    cov.accumulate_dev(_dev(t, torch.float32), _dev(prim, torch.int32), 3, N, _dev(sop, torch.int32))
    bits, hits, ret = cov.export()
    seen, h, r = R.accumulate(t, prim, 3, N, 2, T, set_of_pose=sop)
    assert np.array_equal(bits, R.pack(seen)) and np.array_equal(hits, h) and np.array_equal(ret, r)
    # pose 1 names set 2 of two: its rays are dropped -- the result is that of poses 0 and 2 alone
    only = R.accumulate(np.concatenate([t[:N], t[2 * N:]]), np.concatenate([prim[:N], prim[2 * N:]]), 2, N, 2, T,
                        set_of_pose=(1, 0))
    assert np.array_equal(bits, R.pack(only[0])) and np.array_equal(hits, only[1]) and np.array_equal(ret, only[2])
    assert int(ret[0]) == N and int(hits[T // 2]) >= N                       # the pose that is one prim throughout
    for k in (0, 1, None):
        s = cov.summary(k)
        mask = seen.any(0) if k is None else seen[k]
        assert np.array_equal(s.seen, mask) and s.seen_triangles == int(mask.sum())
        assert s.covered_q == R.covered_q(mask, q) and s.total_q == cov.total_q
        assert s.returns == (int(r.sum()) if k is None else int(r[k])) and s.per_class_q == {}
    cov.close()


# ---- summaries with classes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one class", "no classes", "4096 classes"])
def test_summaries_per_class(ctx, case):
    import torch
    T = 4096 if case == "4096 classes" else 33
    v, f, q = _soup(T)
    rng = np.random.default_rng(T)
    sem = {"one class": np.full(T, 7, np.uint16), "no classes": None,
           "4096 classes": rng.permutation(np.concatenate([[0, 0xFFFF], np.arange(100, 100 + T - 2)])).astype(np.uint16)}[case]
    assert sem is None or len(set(sem.tolist())) == (4096 if T == 4096 else 1)
    S, N = 3, 500
    cov = _cov(ctx, v, f, sem, S=S)
    assert len(cov.class_ids) == {"one class": 1, "no classes": 0, "4096 classes": 4096}[case]
    prim = rng.integers(0, T, S * N).astype(np.uint32)
    t = rng.uniform(0.1, 5.0, S * N).astype(np.float32)
    t[rng.random(S * N) < 0.3] = np.inf
    cov.accumulate_dev(_dev(t, torch.float32), _dev(prim, torch.int32), S, N)
    seen, h, r = R.accumulate(t, prim, S, N, S, T)
    totals = {} if sem is None else R.per_class(np.ones(T, bool), q, sem)
    assert [int(x) for x in cov.class_ids] == sorted(totals)
    assert [int(x) for x in cov.class_total_q] == [totals[c][1] for c in sorted(totals)]
    for k in (0, 1, 2, None):
        s = cov.summary(k)
        mask = seen.any(0) if k is None else seen[k]
        assert np.array_equal(s.seen, mask) and s.seen_triangles == int(mask.sum())
        assert s.covered_q == R.covered_q(mask, q) and s.total_q == cov.total_q
        assert s.returns == (int(r.sum()) if k is None else int(r[k]))
        want = {} if sem is None else {c: (int(q[mask & (sem == c)].sum(dtype=np.uint64)), totals[c][1]) for c in totals}
        assert s.per_class_q == want
        assert sum(c for c, _ in s.per_class_q.values()) == (s.covered_q if sem is not None else 0)
    assert np.array_equal(s.hits, h)
    cov.close()


def test_4097_labels_are_refused(ctx):
    v, f = random_soup(4097, seed=1)
    with pytest.raises(ValueError):
        _cov(ctx, v, f, np.arange(4097, dtype=np.uint16))
    _cov(ctx, v[:3 * 4096], f[:4096], np.arange(4096, dtype=np.uint16)).close()


# ---- selection: sizes and ties -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 2500])
def test_select_sizes_and_exact_ties(ctx, S):
    v, f, q = _equal()
    assert (q == q[0]).all()
    cov = _cov(ctx, v, f, S=S)
    seen = R.tie_sets(S)
    _write(cov, seen)
    rp, rg = R.greedy(seen, q, 12)
    first = cov.select(12)
    _assert_select(first, rp, rg, cov.total_q)
    again = cov.select(12)                                      # the selection state is reset by every call
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    if S == 2500:                                               # the smaller index in every tie, round after round
        assert rp[:7] == [300, 1324, 2348, 900, 1030, 1000, 2050]
    if S == 1025:
        assert rp[:2] == [0, 1024]
    for group in R.tie_groups_below(S):                         # within a tie group the picks ascend
        mine = [k for k in rp if k in group]
        assert mine == sorted(mine)
    # the same sizes on a soup (distinct q, random patterns: no ties)
    sv, sf, sq = _soup(200)
    soup = _cov(ctx, sv, sf, S=S)
    pattern = np.random.default_rng(S).random((S, 200)) < 0.02
    _write(soup, pattern)
    sp, sg = R.greedy(pattern, sq, 8)
    _assert_select(soup.select(8), sp, sg, soup.total_q)
    cov.close()
    soup.close()


def test_select_second_gain_workgroup(ctx):
    """W = 1025 words: gain_kernel runs two workgroups per set and the second holds one word with one valid bit."""
    T = 32769
    v, f, q = _soup(T)
    cov = _cov(ctx, v, f, S=3)
    assert cov.words_per_set == 1025
    seen = np.zeros((3, T), bool)
    seen[0, 32768] = True                                       # a gain from the second workgroup only
    seen[1, [7, 20000, 32768]] = True                           # from both
    seen[2, 9] = True
    _write(cov, seen)
    rp, rg = R.greedy(seen, q, 3)
    assert rp[0] == 1 and 0 not in rp                           # set 1 covers set 0's only triangle
    _assert_select(cov.select(3), rp, rg, cov.total_q)
    only = seen.copy()
    only[1] = False
    _write(cov, only)
    rp, rg = R.greedy(only, q, 3)
    assert 0 in rp and rg[rp.index(0)] == int(q[32768])
    _assert_select(cov.select(3), rp, rg, cov.total_q)
    cov.close()


# ---- selection: stop rules, initial cover, target -------------------------------------------------------------------
def test_select_stop_rules(ctx):
    v, f, q = _equal()
    S = 1023
    cov = _cov(ctx, v, f, S=S)
    seen = R.tie_sets(S, sparse=True)
    _write(cov, seen)
    picks, gains, cum = cov.select(0)                           # budget 0
    assert len(picks) == 0 and len(gains) == 0 and len(cum) == 0
    rp, rg = R.greedy(seen, q, S)                               # a full run: stops at the first zero gain
    assert 10 <= len(rp) < 40
    _assert_select(cov.select(S), rp, rg, cov.total_q)
    _assert_select(cov.select(5000), rp, rg, cov.total_q)       # budget > S
    _assert_select(cov.select(S, target_ratio=1.5), rp, rg, cov.total_q)   # a target never reached
    for none in (0.0, -1.0, -0.0):                              # target <= 0 is ignored
        _assert_select(cov.select(S, target_ratio=none), rp, rg, cov.total_q)
    _assert_select(cov.select(4), rp[:4], rg[:4], cov.total_q)
    cov.reset()                                                 # nothing seen at all
    assert len(cov.select(5)[0]) == 0
    cov.close()


def test_select_initial_cover_with_stray_bits(ctx):
    T = 200
    v, f, q = _equal()
    cov = _cov(ctx, v, f, S=1025)
    seen = R.tie_sets(1025)
    _write(cov, seen)
    init = np.zeros(T, bool)
    init[[0, 1, 2, 60, 199]] = True                             # triangles of the first tie group among them
    words = R.pack(init).copy()
    assert words.shape == (7,) and words.dtype == np.uint32
    words[-1] |= np.uint32(0xFFFFFF00)                          # bits 200..223: past T
    rp, rg = R.greedy(seen, q, 6, initial=init)
    iq = R.covered_q(init, q)
    masked = cov.select(6, initial=init)
    _assert_select(masked, rp, rg, cov.total_q, iq)
    stray = cov.select(6, initial=words)
    assert all(np.array_equal(a, b) for a, b in zip(masked, stray))
    # an initial cover that already reaches the target picks nothing
    big = np.zeros(T, bool)
    big[:150] = True
    assert R.greedy(seen, q, 6, initial=big, target_ratio=0.75)[0] == []
    assert len(cov.select(6, initial=big, target_ratio=0.75)[0]) == 0
    w = R.pack(big).copy()
    w[-1] |= np.uint32(0xFFFFFF00)
    assert len(cov.select(6, initial=w, target_ratio=0.75)[0]) == 0
    one_more = float(np.nextafter(0.75, 2.0))
    rp, rg = R.greedy(seen, q, 6, initial=big, target_ratio=one_more)
    assert len(rp) == 1
    _assert_select(cov.select(6, initial=w, target_ratio=one_more), rp, rg, cov.total_q, R.covered_q(big, q))
    cov.close()


@pytest.mark.parametrize("mesh", ["equal q", "soup"])
def test_select_target_hit_exactly(ctx, mesh):
    v, f, q = _equal() if mesh == "equal q" else _soup(200)
    S = 1025
    cov = _cov(ctx, v, f, S=S)
    seen = R.tie_sets(S) if mesh == "equal q" else np.random.default_rng(2).random((S, 200)) < 0.02
    _write(cov, seen)
    rp, rg = R.greedy(seen, q, 12)
    assert len(rp) == 12
    cum = R.cumulative_q(rg)
    for k in (0, 1, 5, 10):
        target = float(cum[k]) / float(cov.total_q)
        assert R.greedy(seen, q, 12, target_ratio=target)[0] == rp[:k + 1]
        _assert_select(cov.select(12, target_ratio=target), rp[:k + 1], rg[:k + 1], cov.total_q)   # stops after pick k
        above = float(np.nextafter(target, 2.0))
        _assert_select(cov.select(12, target_ratio=above), rp[:k + 2], rg[:k + 2], cov.total_q)    # one more pick
    cov.close()
