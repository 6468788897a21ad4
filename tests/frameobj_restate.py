"""numpy restatement of the per-frame object annotations (csrc/lrc_frameobj.hip): the object table,
the sensor-frame coordinate of a returned ray and the per-(frame, object) accumulators.

Object k is the k-th distinct label word key = sem | ins << 16, ascending.  A ray returns iff its t is finite and its
prim < T; a returned ray with a non-finite point coordinate is rejected (counted, otherwise ignored); rows of rays that do
not return are never read.  s_a = (R[0][a]*e_0 + R[1][a]*e_1) + R[2][a]*e_2 with e = float64(x) - c, no fused
multiply-add (numpy's element-wise ufuncs round after every operation).  Minima and maxima follow the IEEE total order
on finite values (-0.0 below +0.0): they are taken on an order-preserving uint64 image of the doubles."""
import numpy as np

from coverage_restate import area_q

INVALID = 0xFFFFFFFF
MAX_OBJECTS = 4096
_TOP = np.uint64(1 << 63)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
IMG_POS_INF = np.uint64(0xFFF0000000000000)
IMG_NEG_INF = np.uint64(0x000FFFFFFFFFFFFF)


def image(x):
    """float64 -> uint64 whose unsigned order is the IEEE total order."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, b ^ _ALL, b ^ _TOP)


def unimage(i):
    i = np.ascontiguousarray(i, dtype=np.uint64)
    return np.where(i >> np.uint64(63) != 0, i ^ _TOP, i ^ _ALL).view(np.float64)


def object_table(vertices, triangles, sem=None, ins=None):
    """-> dict(key (K,) uint32, obj (T,) object index of every triangle, tri_count (K,) uint32, q (T,) uint64,
    total_q (K,) uint64, wmin / wmax (K, 3) float64)."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(triangles, dtype=np.int64)
    T = len(f)
    s = np.zeros(T, np.uint32) if sem is None else np.asarray(sem).astype(np.uint16).astype(np.uint32)
    i = np.zeros(T, np.uint32) if ins is None else np.asarray(ins).astype(np.uint16).astype(np.uint32)
    word = s | (i << np.uint32(16))
    key, obj = np.unique(word, return_inverse=True)
    if len(key) > MAX_OBJECTS:
        raise ValueError("more than 4096 distinct objects")
    q = area_q(v, f)
    K = len(key)
    tri_count = np.bincount(obj, minlength=K).astype(np.uint32)
    total_q = np.zeros(K, np.uint64)
    wmin, wmax = np.zeros((K, 3)), np.zeros((K, 3))
    for k in range(K):
        sel = obj == k
        total_q[k] = np.uint64(sum(int(x) for x in q[sel]))
        im = image(v[f[sel].reshape(-1)])                     # (3n, 3)
        wmin[k], wmax[k] = unimage(im.min(0)), unimage(im.max(0))
    return {"key": key.astype(np.uint32), "obj": obj.astype(np.int64), "tri_count": tri_count, "q": q,
            "total_q": total_q, "wmin": wmin, "wmax": wmax}


def sensor_coords(pose, x32):
    """(n, 3) float32 world points -> (n, 3) float64 in the frame of ``pose`` (4, 4)."""
    M = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    R, c = M[:3, :3], M[:3, 3]
    e = np.asarray(x32, dtype=np.float32).astype(np.float64) - c
    s = np.empty_like(e)
    for a in range(3):
        s[:, a] = (R[0, a] * e[:, 0] + R[1, a] * e[:, 1]) + R[2, a] * e[:, 2]
    return s


def new_state(num_frames, table):
    F, K, T = int(num_frames), len(table["key"]), len(table["obj"])
    return {"returns": np.zeros((F, K), np.uint32), "seen": np.zeros((F, T), bool),
            "lo": np.full((F, K, 3), IMG_POS_INF, np.uint64), "hi": np.full((F, K, 3), IMG_NEG_INF, np.uint64),
            "rejected": 0}


def accumulate(state, table, t, prim, point3, poses, rays_per_pose, first_frame=0):
    """Add the records of len(poses) x rays_per_pose rays, pose-major, to ``state``; pose p -> frame first_frame + p."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    P, N, T = len(poses), int(rays_per_pose), len(table["obj"])
    F = state["returns"].shape[0]
    if first_frame + P > F:
        raise ValueError("first_frame + num_poses > num_frames")
    t = np.asarray(t, dtype=np.float32).reshape(-1)[:P * N].reshape(P, N)
    prim = np.asarray(prim).reshape(-1).astype(np.uint32)[:P * N].reshape(P, N)
    point3 = np.asarray(point3, dtype=np.float32).reshape(-1, 3)[:P * N].reshape(P, N, 3)
    for p in range(P):
        f = first_frame + p
        ok = np.isfinite(t[p]) & (prim[p].astype(np.int64) < T)
        idx = np.flatnonzero(ok)                              # only these rows are read
        x = point3[p][idx]
        fin = np.isfinite(x).all(1)
        state["rejected"] += int((~fin).sum())
        idx, x = idx[fin], x[fin]
        pr = prim[p][idx].astype(np.int64)
        k = table["obj"][pr]
        state["returns"][f] += np.bincount(k, minlength=state["returns"].shape[1]).astype(np.uint32)
        state["seen"][f, pr] = True
        im = image(sensor_coords(poses[p], x))
        for a in range(3):
            np.minimum.at(state["lo"][f, :, a], k, im[:, a])
            np.maximum.at(state["hi"][f, :, a], k, im[:, a])
    return state


def finish(state, table):
    """-> dict(returns, seen_tris (F, K) uint32, seen_q (F, K) uint64, vmin, vmax (F, K, 3) float64, rejected_rays)."""
    F, K = state["returns"].shape
    seen_tris, seen_q = np.zeros((F, K), np.uint32), np.zeros((F, K), np.uint64)
    for f in range(F):
        j = np.flatnonzero(state["seen"][f])
        seen_tris[f] = np.bincount(table["obj"][j], minlength=K)
        for k in np.unique(table["obj"][j]):
            seen_q[f, k] = np.uint64(sum(int(x) for x in table["q"][j[table["obj"][j] == k]]))
    return {"returns": state["returns"].copy(), "seen_tris": seen_tris, "seen_q": seen_q,
            "vmin": unimage(state["lo"]), "vmax": unimage(state["hi"]), "rejected_rays": state["rejected"]}


def restate(table, t, prim, point3, poses, rays_per_pose, num_frames=None):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    st = new_state(len(poses) if num_frames is None else num_frames, table)
    return finish(accumulate(st, table, t, prim, point3, poses, rays_per_pose), table)


def hand_made_case():
    """Two objects, four triangles, six rays, one frame -- every value worked out by hand (tests/test_frameobj_host.py
    asserts them on the restatement, tests/test_frameobj_gpu.py on the device).
    -> (vertices, triangles, sem, ins), pose (4, 4), (t, prim, point3)."""
    # four right triangles in the plane z = 0; areas 0.5, 1.0, 0.5, 2.0 -> q = 2^31, 2^32, 2^31, 2^33
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, -1, 0], [-4, 0, 0], [0, 0, 0.25]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 2], [0, 1, 4], [0, 5, 2]], np.int32)
    sem = np.array([7, 7, 8, 8], np.uint16)
    ins = np.array([1, 1, 2, 2], np.uint16)
    M = np.eye(4)
    M[:3, 3] = (0.0, 2.0, 3.0)
    nan3 = [np.nan] * 3
    #        t       prim     point3                what
    rays = [(1.0,    0,       [0.0, 2.5, 3.5]),     # A, triangle 0: e = (+0, .5, .5)         -> s = (+0.0, .5, .5)
            (2.0,    0,       [-0.0, 1.5, 2.5]),    # A, triangle 0 again: e = (-0, -.5, -.5) -> s = (-0.0, -.5, -.5)
            (1.0,    INVALID, nan3),                # finite t, invalid prim: ignored
            (np.inf, 2,       nan3),                # valid prim (object B), t = inf: ignored -> B has no return
            (1.5,    1,       [0.0, 3.0, 1.0]),     # A, triangle 1: e = (+0, 1, -2)          -> s = (+0.0, 1, -2)
            (1.0,    7,       nan3)]                # prim >= T: ignored
    t = np.array([r[0] for r in rays], np.float32)
    prim = np.array([r[1] for r in rays], np.uint32)
    pts = np.array([r[2] for r in rays], np.float32)
    return (v, f, sem, ins), M, (t, prim, pts)


HAND_MADE_RESULT = {                                 # one frame, objects A and B
    "returns": [[3, 0]],
    "seen_tris": [[2, 0]],                           # triangle 0 once, triangle 1
    "seen_q": [[(1 << 31) + (1 << 32), 0]],          # two rays on triangle 0 count its q once
    "vmin": [[[-0.0, -0.5, -2.0], [np.inf] * 3]],    # a min that ties on zero is -0.0
    "vmax": [[[0.0, 1.0, 0.5], [-np.inf] * 3]],      # a max that ties on zero is +0.0
}
