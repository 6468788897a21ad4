"""float64 numpy / scipy restatement of the per-object outlier filter of include/lidarcast.h "object boxes" (the outlier
stage of lrc_cloud_preprocess on one object), shared by tests/golden/make_s3dis_bbox_golden.py and the object-box tests.

avg: candidates from cKDTree, the fixed expression (dx*dx + dy*dy) + dz*dz, the k smallest ascending, np.cumsum of their
square roots, / k.  mean and std: the library's reduction order restated (256 contiguous chunks of ceil(m / 256) rows,
lanes strided by 256 and summed one after the other, a halving tree over the 256 lanes, the same tree over the 256
chunks), so mean and threshold are bit-exact and keep needs no tolerance.  Not Open3D: parity with Open3D itself is
not pinned."""
import numpy as np

RED = 256


def d2(q, p):
    d = q[:, None, :] - p
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def restate_avg(p, k, chunk=1 << 16):
    """avg of every row of an object of m >= k rows."""
    from scipy.spatial import cKDTree
    m = len(p)
    kk = min(m, k + 8)
    tree = cKDTree(p)
    out = np.empty(m)
    for a in range(0, m, chunk):
        q = p[a:a + chunk]
        _, cand = tree.query(q, kk, workers=16)
        dd = np.sort(d2(q, p[cand.reshape(len(q), kk)]), axis=1)[:, :k]
        out[a:a + chunk] = np.cumsum(np.sqrt(dd), axis=1)[:, -1] / k
    return out


def _tree(x):
    x = x.copy()
    w = RED // 2
    while w:
        x[:, :w] = x[:, :w] + x[:, w:2 * w]
        w //= 2
    return x[:, 0]


def fixed_sum(v):
    """The library's sum of v (m,) (excluded rows given as +0)."""
    m = len(v)
    chunk = -(-m // RED)
    if chunk == 0:
        return 0.0
    iters = -(-chunk // RED)
    lanes = np.zeros((RED, iters * RED))
    pad = np.zeros(RED * chunk)
    pad[:m] = v
    lanes[:, :chunk] = pad.reshape(RED, chunk)
    lanes = lanes.reshape(RED, iters, RED)
    acc = np.zeros((RED, RED))
    for i in range(iters):
        acc = acc + lanes[:, i, :]
    return float(_tree(_tree(acc)[None, :])[0])


def restate_stats(avg, std_ratio):
    m = len(avg)
    pos = avg > 0
    mean = fixed_sum(np.where(pos, avg, 0.0)) / m
    dev = avg - mean
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = mean + std_ratio * np.sqrt(fixed_sum(np.where(pos, dev * dev, 0.0)) / (m - 1))
    return mean, thr


def restate_object(p, k=20, std_ratio=2.0):
    """(avg, keep, mean, threshold, filtered) of one object."""
    p = np.asarray(p, np.float64)
    m = len(p)
    if m < k:
        return np.full(m, -1.0), np.ones(m, bool), 0.0, float("inf"), False
    avg = restate_avg(p, k)
    mean, thr = restate_stats(avg, std_ratio)
    return avg, (avg > 0) & (avg < thr), mean, thr, True


def restate_filter_objects(point_sets, k=20, std_ratio=2.0):
    """S3DISBBoxVisualizer.filter_objects restated: (min3, max3, num_kept) per object."""
    out = []
    for p in point_sets:
        p = np.asarray(p, np.float64)
        keep = restate_object(p, k, std_ratio)[1]
        kp = p[keep]
        if len(kp):
            out.append((kp.min(axis=0), kp.max(axis=0), len(kp)))
        else:
            out.append((np.full(3, np.inf), np.full(3, -np.inf), 0))
    return out


def restate_remove_outliers(points, colors=None, k=20, std_ratio=2.0):
    """The reference's remove_outliers with the restated filter: (points, colors) of the kept rows."""
    if len(points) < k:
        return points, colors
    keep = restate_object(points, k, std_ratio)[1]
    return np.asarray(points)[keep], (np.asarray(colors)[keep] if colors is not None else None)
