"""numpy restatement of surface coverage (csrc/lrc_coverage.hip): the quantised area table, the
accumulation of returned rays into per-set bitsets / hits / returned-ray counts, summaries and the greedy selection."""
import numpy as np

Q_ONE = 2.0 ** 32
LIMIT = 1 << 63
INVALID = 0xFFFFFFFF


def area_q(vertices, triangles):
    """(T,) uint64 q = rint(area * 2^32); area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (v1 - v0) x (v2 - v0) as
    a*b - c*d per component, float64, no fused multiply-add.  Raises ValueError where the device refuses the mesh."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(triangles, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    s = area * Q_ONE
    if not (s < float(LIMIT)).all():
        raise ValueError("a triangle's quantised area reaches 2^63")
    q = np.rint(s).astype(np.uint64)
    if sum(int(x) for x in q) > LIMIT:
        raise ValueError("total quantised area exceeds 2^63")
    return q


def words(T):
    return (T + 31) // 32


def returned(t, prim, T):
    t = np.asarray(t, dtype=np.float32)
    prim = np.asarray(prim).astype(np.uint32)
    return np.isfinite(t) & (prim.astype(np.int64) < T)


def accumulate(t, prim, num_poses, rays_per_pose, num_sets, T, set_of_pose=None, state=None):
    """-> (seen (S, T) bool, hits (T,) uint32, returns (S,) uint64), added onto ``state`` if given."""
    P, N, S = int(num_poses), int(rays_per_pose), int(num_sets)
    seen, hits, ret = state if state is not None else (np.zeros((S, T), bool), np.zeros(T, np.uint32),
                                                        np.zeros(S, np.uint64))
    t = np.asarray(t, dtype=np.float32)[:P * N].reshape(P, N)
    prim = np.asarray(prim).astype(np.uint32)[:P * N].reshape(P, N)
    sop = np.arange(P) if set_of_pose is None else np.asarray(set_of_pose, dtype=np.int64)
    for p in range(P):
        s = int(sop[p])
        if s >= S:
            continue
        ok = returned(t[p], prim[p], T)
        pr = prim[p][ok].astype(np.int64)
        seen[s, pr] = True
        hits += np.bincount(pr, minlength=T).astype(np.uint32)
        ret[s] += np.uint64(ok.sum())
    return seen, hits, ret


def pack(seen):
    """(..., T) bool -> (..., W) uint32, bit j of word j // 32, least significant first."""
    seen = np.asarray(seen, dtype=bool)
    T = seen.shape[-1]
    pad = np.zeros(seen.shape[:-1] + (words(T) * 32,), bool)
    pad[..., :T] = seen
    return np.packbits(pad, axis=-1, bitorder="little").view("<u4").astype(np.uint32)


def covered_q(mask, q):
    return sum(int(x) for x in q[np.asarray(mask, bool)])


def per_class(mask, q, sem):
    """{sem: (covered_q, total_q)}"""
    sem = np.asarray(sem)
    return {int(s): (covered_q(mask & (sem == s), q), covered_q(sem == s, q)) for s in np.unique(sem)}


def greedy(seen, q, budget, initial=None, target_ratio=None):
    """seen (S, T) bool -> (picks, gains) with the device's rule: largest gain = sum of q over seen_k & ~covered, ties to
    the smallest k; stop after budget picks, at gain 0, or once float64(covered_q) / float64(total_q) >= target_ratio:
    both integers are converted to float64 first (round to nearest even), then divided once in float64, as
    include/lidarcast.h states it.  (Python's int / int rounds the exact quotient once instead, and differs from it
    once covered_q passes 2^53.)"""
    seen = np.asarray(seen, bool)
    S, T = seen.shape
    qi = [int(x) for x in q]
    total = sum(qi)
    covered = np.zeros(T, bool) if initial is None else np.asarray(initial, bool).copy()
    cq = covered_q(covered, q)
    picks, gains = [], []
    qo = np.array(qi, dtype=object)
    for _ in range(min(int(budget), S)):
        if target_ratio is not None and target_ratio > 0 and total and float(cq) / float(total) >= target_ratio:
            break
        g = [int(qo[seen[k] & ~covered].sum()) if (seen[k] & ~covered).any() else 0 for k in range(S)]
        k = int(np.argmax(g))                 # first maximum
        if g[k] == 0:
            break
        picks.append(k)
        gains.append(g[k])
        covered |= seen[k]
        cq += g[k]
    return picks, gains


# ---- builders of the coverage edge tests ------------------------------------------------------------------------------

def equal_q_mesh(T, seed=4):
    """T triangles with identical coordinates, each on vertex rows of its own: identical area_q, so gains tie exactly."""
    tri = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, 3))
    return np.tile(tri, (T, 1)), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


# positions in a pose of N rays (entries at or past N fall away): the runs and single rays the accumulate test promises
RUN_LANES = (60, 71)           # one prim over rays 60..70: across the lane 63 | 64 boundary of two waves
RUN_STRIDE = (250, 263)        # one prim over rays 250..262: across the per-thread stride of 256 (two passes, other lanes)
RUN_SPLIT = (20, 31)           # one prim over rays 20..30 with ray 25 not returned (t = inf, the same prim)
SPLIT_AT = 25
SINGLES = {"last_prim": 5, "prim_T": 6, "invalid_prim": 7, "nan_t": 8, "neg_zero_t": 9, "neg_t": 10}
EDGE_SET_OF_POSE = (1, 2, 0)   # with two sets: pose 1 is dropped


def edge_records(N, T, seed=0):
    """(t (3*N,) float32, prim (3*N,) uint32) of three poses of N rays.  Pose 0: random prims in short runs with misses, and
    on top the runs and single rays above.  Pose 1: the same rays again (its set index is out of range: all dropped).
    Pose 2: every ray returns from one prim (T // 2)."""
    rng = np.random.default_rng(seed + 7 * N)
    prim = rng.integers(0, T, N).astype(np.uint32)
    for i in range(1, N):
        if rng.random() < 0.5:
            prim[i] = prim[i - 1]
    t = rng.uniform(0.1, 5.0, N).astype(np.float32)
    t[rng.random(N) < 0.15] = np.inf
    miss = rng.random(N) < 0.1
    t[miss], prim[miss] = np.inf, INVALID
    a = [(T // 3, RUN_LANES), ((2 * T) // 3, RUN_STRIDE), (T // 4, RUN_SPLIT)]
    for p, (lo, hi) in a:
        prim[lo:hi] = p
        t[lo:hi] = 1.0
    if SPLIT_AT < N:
        t[SPLIT_AT] = np.inf
    for name, (pv, tv) in {"last_prim": (T - 1, 1.0), "prim_T": (T, 1.0), "invalid_prim": (INVALID, 1.0),
                           "nan_t": (0, np.nan), "neg_zero_t": (0, -0.0), "neg_t": (0, -2.5)}.items():
        i = SINGLES[name]
        if i < N:
            prim[i], t[i] = pv, tv
    whole_t = np.full(N, 2.0, np.float32)
    whole_p = np.full(N, T // 2, np.uint32)
    return np.concatenate([t, t, whole_t]), np.concatenate([prim, prim, whole_p])


def seen_records(seen):
    """One ray per seen triangle: (t, prim, N) of S poses (pose k -> set k) that write the (S, T) pattern ``seen``."""
    seen = np.asarray(seen, bool)
    S = seen.shape[0]
    N = max(1, int(seen.sum(1).max()))
    t = np.full((S, N), np.inf, np.float32)
    prim = np.full((S, N), INVALID, np.uint32)
    for k in np.flatnonzero(seen.any(1)):
        j = np.flatnonzero(seen[k])
        prim[k, :len(j)] = j
        t[k, :len(j)] = 1.0
    return t.reshape(-1), prim.reshape(-1), N


# groups of sets with equal gains; the sets of one group see disjoint triangles, as many each as the second entry says, so
# the tie comes back in the following rounds until the group is used up
TIE_GROUPS = (((300, 1324, 2348), 10),      # k, k + 1024, k + 2048: one thread's stride-1024 loop
              ((1030, 900), 8),             # thread 6 holds 1030, thread 900 holds the smaller index
              ((2050, 1000), 6),            # thread 2 holds 2050, thread 1000 the smaller index
              ((0, 1024), 5),               # thread 0's loop, the first and the last set of S = 1025
              ((1022, 17), 4))


def tie_sets(S, T=200, seed=1, sparse=False):
    """(S, T) bool seen pattern for the equal-q mesh: the TIE_GROUPS whose indices fit below S, and every other set with 0 to
    3 of the remaining triangles (``sparse``: only every 50th of them sees anything)."""
    rng = np.random.default_rng(seed)
    seen = np.zeros((S, T), bool)
    nxt = 0
    used = set()
    for group, width in TIE_GROUPS:
        if max(group) >= S:
            continue
        for k in group:
            seen[k, nxt:nxt + width] = True
            nxt += width
            used.add(k)
    assert nxt < T - 20
    for k in range(S):
        if k in used or (sparse and k % 50):
            continue
        seen[k, rng.integers(nxt, T, rng.integers(0, 4))] = True
    return seen


def tie_groups_below(S):
    return [g for g, _ in TIE_GROUPS if max(g) < S]


def cumulative_q(gains, initial_q=0):
    out, c = [], int(initial_q)
    for g in gains:
        c += int(g)
        out.append(c)
    return out
