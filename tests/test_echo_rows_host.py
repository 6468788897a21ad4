"""CPU: the row sets of tests/echo_rows.py have teeth.  The clustering restated there in a form that can be bent is
echo_restate.reduce_rows when it is not bent; every bend -- a rule of the header broken one way -- changes the result on the
exhaustive set; the sets hold rows of every kind the device tests are for; and the host reduction (lrc_echo_reduce) passes
all of them.

No mutant breaks ties by the LARGER k: tied sub-rays are 0 apart, so they always share a cluster, and nothing the reduction
returns (smallest k of a cluster, member count, the clusters' order) depends on the order inside a cluster -- the (t, k) order
of the header is not observable."""
import ctypes as C

import numpy as np
import pytest

import echo_restate as er
import echo_rows as rows


@pytest.fixture(scope="module")
def sets():
    return {K: rows.row_set(K) for K in range(1, 17)}


def test_alphabet_and_set_sizes(sets):
    assert rows.ALPHABET.dtype == np.float32 and len(rows.ALPHABET) == 6
    for K in range(1, 6):
        assert sets[K].shape == (6 ** K, K) and len(np.unique(sets[K], axis=0)) == 6 ** K
    for K in range(6, 17):
        t = sets[K]
        assert t.shape == (rows.RANDOM_ROWS + 4, K) and t.dtype == np.float32
        assert np.isin(t, rows.EXTENDED).all()
        assert np.isinf(t[-4]).all() and (t[-3] == t[-3, 0]).all() and np.isfinite(t[-3]).all()
        assert (np.diff(t[-2]) == rows.SEP).all() and (np.diff(t[-1]) == -rows.SEP).all()
        assert np.array_equal(rows.row_set(K), t)                                   # seeded: the same rows every time
    # the chain 1 + 0.25 j and each value's next float up are all there
    assert np.isin(rows.CHAIN, rows.EXTENDED).all() and np.isin(np.nextafter(rows.CHAIN, rows.INF), rows.EXTENDED).all()
    assert np.isin(rows.ALPHABET, rows.EXTENDED).all()
    f = rows.fillers(5, 3)
    assert np.isinf(f[0::2]).all() and (f[1::2] == 2.0).all()


@pytest.mark.parametrize("K", range(1, 17))
def test_unbent_clustering_is_the_restatement_and_the_host_reduction(sets, K):
    from lidarcast import echo
    from lidarcast._capi import LrcBeam
    t = sets[K]
    for mc in sorted({1, min(2, K), K}):
        want = er.reduce_rows(t, 4, mc, rows.SEP)
        mine = rows.reduce_rows(t, 4, mc, rows.SEP)
        assert np.array_equal(mine[0], want[0]) and np.array_equal(mine[1], want[1]), (K, mc)
        for E in (1, 2, 3, 4):
            b = LrcBeam()
            b.subrays, b.max_echoes, b.min_count, b.separation = K, E, mc, rows.SEP
            rep, w = echo.reduce(t, b)
            assert np.array_equal(rep, want[0][:, :E]) and np.array_equal(w, want[1][:, :E]), (K, E, mc)


def test_crafted_rows_give_their_recorded_results():
    for c in rows.CRAFTED:
        rep, w = er.reduce_rows(c.t, c.E, c.min_count, c.separation)
        assert rep.tolist() == c.rep and w.tolist() == c.weight, c


@pytest.mark.parametrize("K", [3, 4, 5])
def test_every_mutant_changes_the_exhaustive_set(sets, K):
    """Each bent rule changes the result under some (E, min_count) the device tests run: one changed row would tell the mutant
    from the reduction; asked for are ten (of 216) at K = 3 and a hundred from K = 4, so that no single row carries a rule."""
    t = sets[K]
    changed = dict.fromkeys(rows.MUTANTS, 0)
    for mc in sorted({1, min(2, K), K}):
        want = er.reduce_rows(t, 4, mc, rows.SEP)
        for m in rows.MUTANTS:
            got = rows.reduce_rows(t, 4, mc, rows.SEP, mutant=m)
            for E in (1, 2, 3, 4):
                n = int(((got[0][:, :E] != want[0][:, :E]) | (got[1][:, :E] != want[1][:, :E])).any(axis=1).sum())
                changed[m] = max(changed[m], n)
    print(f"\n[echo rows] K={K}: rows changed by each mutant (largest over E, min_count): {changed}")
    for m, n in changed.items():
        assert n >= (10 if K == 3 else 100), (K, m, n)


def test_ties_broken_by_larger_k_change_nothing(sets):
    """The (t, k) order is not observable: sorting ties the other way round gives the same result on every exhaustive row."""
    for K in (3, 4, 5):
        t = sets[K]
        for mc in sorted({1, 2, K}):
            rep = np.full((len(t), 4), -1, np.int32)
            w = np.zeros((len(t), 4), np.uint8)
            for b, row in enumerate(t):
                ks = sorted((k for k in range(K) if row[k] < np.inf), key=lambda k: (row[k], -k))
                cl = []
                for m, k in enumerate(ks):
                    if m == 0 or np.float32(row[k] - row[ks[m - 1]]) > rows.SEP:
                        cl.append([k])
                    else:
                        cl[-1].append(k)
                for e, c in enumerate([c for c in cl if len(c) >= mc][:4]):
                    rep[b, e], w[b, e] = min(c), len(c)
            want = er.reduce_rows(t, 4, mc, rows.SEP)
            assert np.array_equal(rep, want[0]) and np.array_equal(w, want[1]), (K, mc)


@pytest.mark.parametrize("K", range(1, 17))
def test_sets_hold_every_kind(sets, K):
    """The kinds the device tests name, wherever (K, E, min_count) admits them at all: two clusters of min_count members need
    2 min_count <= K, more clusters than echoes (E + 1) min_count <= K, a dropped nearest cluster 1 + min_count <= K with
    min_count >= 2, a representative behind its cluster's nearest member a cluster of two."""
    prof = rows.profile(sets[K], rows.SEP)
    for E in (1, 2, 3, 4):
        for mc in sorted({1, min(2, K), K}):
            n = rows.kinds(prof, E, mc)
            print(f"[echo rows] K={K} E={E} min_count={mc}: {n}")
            for kind, possible in rows.possible_kinds(K, E, mc).items():
                assert (n[kind] > 0) == possible, (K, E, mc, kind, n)
            assert n["all_miss"] >= 1
