"""Crafted rows for the multi-echo reduction (numpy only): the rows tests/test_echo_host.py gives the host reduction, an
exhaustive set over a six-letter alphabet for K = 1..5 and a seeded random set for K = 6..16.  The host tests and the device
tests (tests/test_echo_lanes_gpu.py: lrcecho::reduce_lanes through lrc_internal_echo_lanes_dev) run the same rows against
tests/echo_restate.py.

The alphabet is built around one separation, 0.25 (exact in float32): 1.0 and 1.25 are exactly the separation apart (no split),
1.0 and the float above 1.25 one ulp more (split), that float and 1.5 one ulp less (no split), 3.0 is far from everything and
+inf is a miss.  ``clusters`` restates the clustering once more, in a form that can be bent: tests/test_echo_rows_host.py
shows that it is echo_restate.reduce_rows when it is not bent, and that every bend changes the result on these rows."""
import itertools

import numpy as np

INF = np.float32(np.inf)
SEP = np.float32(0.25)
A = np.float32(1.0)
B = np.float32(A + SEP)
B1 = np.nextafter(B, INF)
ALPHABET = np.array([A, B, B1, 1.5, 3.0, INF], dtype=np.float32)

assert B == np.float32(1.25) and np.float32(B - A) == SEP                  # a gap of exactly the separation
assert np.float32(B1 - A) > SEP                                             # ... and one ulp (of 1.25) above it
assert np.float32(ALPHABET[3] - B) == SEP and np.float32(ALPHABET[3] - B1) < SEP
assert np.float32(ALPHABET[4] - ALPHABET[3]) > SEP and np.float32(B1 - B) < SEP

CHAIN = (np.float32(1.0) + np.float32(0.25) * np.arange(16, dtype=np.float32)).astype(np.float32)      # every gap == SEP
assert (np.diff(CHAIN) == SEP).all()
_FINITE = np.unique(np.concatenate([ALPHABET[:-1], CHAIN]))
EXTENDED = np.concatenate([_FINITE, np.nextafter(_FINITE, INF), [INF]]).astype(np.float32)
EXTENDED = np.unique(EXTENDED)                                              # sorted, +inf last
RANDOM_ROWS = 4096


# ---- the rows of tests/test_echo_host.py, with the result each must give ---------------------------------------------------------

class Case:
    def __init__(self, group, t, E, rep, weight, min_count=1, separation=0.05):
        self.group, self.E, self.min_count, self.separation = group, E, min_count, np.float32(separation)
        self.t = np.array(t, dtype=np.float32).reshape(1, -1)
        self.rep, self.weight = [list(rep)], [list(weight)]

    def __repr__(self):
        return f"Case({self.group}, t={self.t[0].tolist()}, E={self.E}, min_count={self.min_count}, separation={self.separation})"


_SLOPE = np.float32(1.0) + np.arange(7, dtype=np.float32) * np.float32(0.04)       # 0.24 m end to end, separation 0.05
_FOUR = [4.0, 1.0, 3.0, 2.0, 1.01, INF, 3.0]
_SMALL = [1.0, 2.0, 2.01, 3.0, 3.0, 3.0, 5.0]
CRAFTED = [
    Case("ties", [2.0, 1.0, 1.0, 2.0, 1.0], 2, [1, 0], [3, 2]),
    Case("ties", [1.0, 1.0, 1.0], 3, [0, -1, -1], [3, 0, 0]),
    Case("separation", [A, B, INF], 2, [0, -1], [2, 0], separation=SEP),           # a gap equal to the separation does not split
    Case("separation", [A, B1, INF], 2, [0, 1], [1, 1], separation=SEP),
    Case("separation", [B1, A, INF], 2, [1, 0], [1, 1], separation=SEP),           # the same two the other way round
    Case("chain", _SLOPE[::-1].copy(), 2, [0, -1], [7, 0]),
    Case("chain", _SLOPE[[3, 0, 6, 1, 5, 2, 4]], 2, [0, -1], [7, 0]),
    Case("misses", [INF] * 5, 2, [-1, -1], [0, 0]),
    Case("misses", [INF, 3.0, INF, 1.0, 3.01], 2, [3, 1], [1, 2]),
    Case("more_clusters", _FOUR, 2, [1, 3], [2, 1]),
    Case("more_clusters", _FOUR, 4, [1, 3, 2, 0], [2, 1, 2, 1]),
    Case("more_clusters", _FOUR, 1, [1], [2]),
    Case("min_count", _SMALL, 2, [1, 3], [2, 3], min_count=2),
    Case("min_count", _SMALL, 2, [3, -1], [3, 0], min_count=3),
]


def crafted(group):
    cases = [c for c in CRAFTED if c.group == group]
    assert cases, group
    return cases


# ---- the row sets ---------------------------------------------------------------------------------------------------------------------

def exhaustive(K):
    """(6^K, K) float32: every row over the alphabet."""
    idx = np.array(list(itertools.product(range(len(ALPHABET)), repeat=K)), dtype=np.int64).reshape(-1, K)
    return ALPHABET[idx]


def random_rows(K):
    """(RANDOM_ROWS + 4, K) float32: seeded rows over the extended alphabet, then the all-miss row, the all-equal row and the
    K-long chain of gaps equal to the separation, rising and falling."""
    rng = np.random.default_rng(7000 + K)
    rows = EXTENDED[rng.integers(0, len(EXTENDED), size=(RANDOM_ROWS, K))]
    extra = np.stack([np.full(K, INF, np.float32), np.full(K, 1.5, np.float32), CHAIN[:K], CHAIN[:K][::-1]])
    return np.concatenate([rows, extra]).astype(np.float32)


def row_set(K):
    """The rows of K sub-rays the device tests run, for the separation SEP."""
    return exhaustive(K) if K <= 5 else random_rows(K)


def fillers(n, K):
    """(n, K) float32: all-miss and all-tie beams in turn."""
    out = np.full((n, K), INF, np.float32)
    out[1::2] = np.float32(2.0)
    return out


# ---- the clustering once more, in a form that can be bent ---------------------------------------------------------------------------

MUTANTS = ("split_at_ge", "rep_is_nearest", "small_takes_slot", "count_gt", "no_chaining")


def clusters(row, separation, mutant=None):
    """The clusters of one row in ascending order, each a list of sub-ray numbers in the order by (t, k)."""
    sep = np.float32(separation)
    ks = sorted((k for k in range(len(row)) if row[k] < np.inf), key=lambda k: (row[k], k))
    out = []
    for m, k in enumerate(ks):
        if m:
            gap = np.float32(row[k] - row[out[-1][0] if mutant == "no_chaining" else ks[m - 1]])
            split = gap >= sep if mutant == "split_at_ge" else gap > sep
        if m == 0 or split:
            out.append([k])
        else:
            out[-1].append(k)
    return out


def reduce_rows(t, max_echoes, min_count, separation, mutant=None):
    """echo_restate.reduce_rows over ``clusters``; ``mutant`` one of MUTANTS bends one rule."""
    t = np.asarray(t, dtype=np.float32)
    rep = np.full((len(t), max_echoes), -1, np.int32)
    weight = np.zeros((len(t), max_echoes), np.uint8)
    for b, row in enumerate(t):
        e = 0
        for c in clusters(row, separation, mutant):
            if e == max_echoes:
                break
            if len(c) > min_count if mutant == "count_gt" else len(c) >= min_count:
                rep[b, e] = c[0] if mutant == "rep_is_nearest" else min(c)
                weight[b, e] = len(c)
                e += 1
            elif mutant == "small_takes_slot":
                e += 1
    return rep, weight


def profile(t, separation):
    """What the kinds below are counted from, per row and cluster (padded to K clusters): ``size`` (B, K) members, 0 behind the
    last cluster, and ``far`` (B, K) bool: the representative (smallest k) is not the cluster's nearest member."""
    t = np.asarray(t, dtype=np.float32)
    size = np.zeros(t.shape, np.int64)
    far = np.zeros(t.shape, bool)
    for b, row in enumerate(t):
        for j, c in enumerate(clusters(row, separation)):
            size[b, j] = len(c)
            far[b, j] = row[min(c)] > row[c[0]]
    return size, far


def possible_kinds(K, E, min_count):
    """Which kinds K sub-rays admit at all under (E, min_count): n clusters of min_count members need n * min_count sub-rays, a
    dropped nearest cluster one sub-ray in front of a cluster that is kept, a far representative a cluster of two.  The six
    letters of the exhaustive sets (K <= 5) lie in at most three clusters: 1.0 | above 1.25 .. 1.5 | 3.0."""
    return {"two_echoes": E >= 2 and 2 * min_count <= K,
            "more_clusters_than_E": (E + 1) * min_count <= K and (K > 5 or E + 1 <= 3),
            "nearest_dropped": min_count >= 2 and 1 + min_count <= K,
            "rep_not_nearest": K >= 2}


def kinds(prof, E, min_count):
    """Rows of each kind under (E, min_count), from ``profile``: dict of counts."""
    size, far = prof
    kept = size >= min_count
    nkept = kept.sum(axis=1)
    first_e = kept & (np.cumsum(kept, axis=1) <= E)                           # the clusters that become echoes
    return {"two_echoes": int((np.minimum(nkept, E) >= 2).sum()),
            "more_clusters_than_E": int((nkept > E).sum()),
            "nearest_dropped": int(((size[:, 0] > 0) & ~kept[:, 0] & (nkept > 0)).sum()),
            "rep_not_nearest": int((first_e & far).any(axis=1).sum()),
            "all_miss": int((size[:, 0] == 0).sum())}
