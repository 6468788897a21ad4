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
    the smallest k; stop after budget picks, at gain 0, or once covered / total >= target_ratio."""
    seen = np.asarray(seen, bool)
    S, T = seen.shape
    qi = [int(x) for x in q]
    total = sum(qi)
    covered = np.zeros(T, bool) if initial is None else np.asarray(initial, bool).copy()
    cq = covered_q(covered, q)
    picks, gains = [], []
    qo = np.array(qi, dtype=object)
    for _ in range(min(int(budget), S)):
        if target_ratio is not None and target_ratio > 0 and total and cq / total >= target_ratio:
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
