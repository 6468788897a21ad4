"""numpy restatement of the beam model of lrc_scan_echoes_* (include/lidarcast.h "beam footprint and multi-echo returns"):
the sub-ray rows of a beam and the reduction of a beam's closest-hit distances to echoes.  Written from the header's text, not
from csrc/lrc_echo.h: the tests compare the two."""
import numpy as np

import noise_restate as nr


def subray_rows(dirs, offsets):
    """(K, N, 3) float64: table rows (N, 3) moved by the offsets (K, 2) = (du, dv) radians.  dp = du / h with h = sqrt(a*a + b*b),
    dt = dv, then the jitter step of the seeded noise; a zero offset and a row with h == 0 pass through bit for bit."""
    dirs = np.asarray(dirs, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.float64).reshape(-1, 2)
    a, b = dirs[:, 0], dirs[:, 1]
    h = np.sqrt(a * a + b * b)
    hs = np.where(h == 0.0, 1.0, h)
    out = np.empty((len(offsets), len(dirs), 3))
    for k, (du, dv) in enumerate(offsets):
        if du == 0.0 and dv == 0.0:
            out[k] = dirs
        else:
            out[k] = nr.jitter_rows(dirs, np.full(len(dirs), du) / hs, np.full(len(dirs), dv))      # h == 0 rows: left as they are
    return out


def reduce_rows(t, max_echoes, min_count, separation):
    """t (B, K) float32, +inf = no hit -> rep (B, E) int32 (-1: empty slot), weight (B, E) uint8."""
    t = np.asarray(t, dtype=np.float32)
    B, K = t.shape
    sep = np.float32(separation)
    rep = np.full((B, max_echoes), -1, np.int32)
    weight = np.zeros((B, max_echoes), np.uint8)
    for b in range(B):
        ks = [k for k in range(K) if t[b, k] < np.inf]
        ks.sort(key=lambda k: (t[b, k], k))
        clusters = []
        for m, k in enumerate(ks):
            if m == 0 or np.float32(t[b, k] - t[b, ks[m - 1]]) > sep:
                clusters.append([k])
            else:
                clusters[-1].append(k)
        kept = [c for c in clusters if len(c) >= min_count][:max_echoes]
        for e, c in enumerate(kept):
            rep[b, e] = min(c)
            weight[b, e] = len(c)
    return rep, weight


def count_clusters(t, min_count, separation):
    """(B,) number of clusters of at least min_count members, without the cap of max_echoes."""
    rep, _ = reduce_rows(t, np.asarray(t).shape[1], min_count, separation)
    return (rep >= 0).sum(axis=1)
