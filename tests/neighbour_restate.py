"""Brute-force restatements of the three neighbour searches (1-NN: csrc/lrc_nn.hip; k-NN average and radius / max_nn
neighbours: csrc/lrc_knn64.h, csrc/lrc_preprocess.hip, csrc/lrc_boxes.hip), the clouds on which the cell-grid walks can
go wrong without random room samples noticing (exact ties, symmetric neighbourhoods, grids of one cell on an axis, empty
shells) and the criterion a normal has to meet on every row.  numpy only; importable without a GPU.

Every distance is the kernels' expression (dx*dx + dy*dy) + dz*dz in float64 against every row of the cloud: no tree, no
grid, nothing to share a mistake with.  Query rows are chunked so that no (rows, n, 3) array exceeds about 100 MB."""
import numpy as np

CHUNK_BYTES = 100e6
LIST_MAX = 32                                      # the longest list the kernels keep (nb_neighbors, max_nn <= 32)


# ---- restatements ---------------------------------------------------------------------------------------------------
def d2(q, p):
    """(len(q), len(p)) float64 squared distances, the expression all three kernels use."""
    d = q[:, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _chunks(nq, n):
    step = max(1, int(CHUNK_BYTES // (24 * max(n, 1))))
    return [(a, min(a + step, nq)) for a in range(0, nq, step)]


def ordered(q, p, keep, tie_key=None):
    """The first `keep` rows of p per query in (d2, tie_key) order (tie_key: the row index unless given): their indices
    and their d2."""
    n = len(p)
    key = np.arange(n) if tie_key is None else np.asarray(tie_key)
    idx = np.empty((len(q), keep), np.int64)
    val = np.empty((len(q), keep))
    for a, e in _chunks(len(q), n):
        dd = d2(q[a:e], p)
        order = np.lexsort((np.broadcast_to(key, dd.shape), dd), axis=1)[:, :keep]
        idx[a:e] = order
        val[a:e] = np.take_along_axis(dd, order, 1)
    return idx, val


def cumulant_cov(p, idx):
    """Open3D's nine cumulants summed in the order of idx (-1: no neighbour) and the covariance E[xx^T] - E[x]E[x]^T;
    the loop of tests/test_preprocess_gpu.py::restate_neighbours."""
    cnt = (idx >= 0).sum(1)
    s = np.zeros((len(idx), 9))
    for j in range(idx.shape[1]):
        m = idx[:, j] >= 0
        x, y, z = (p[idx[m, j], c] for c in range(3))
        s[m] += np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], 1)
    s /= np.maximum(cnt, 1)[:, None]
    cov = np.empty((len(idx), 3, 3))
    cov[:, 0, 0] = s[:, 3] - s[:, 0] * s[:, 0]
    cov[:, 0, 1] = cov[:, 1, 0] = s[:, 4] - s[:, 0] * s[:, 1]
    cov[:, 0, 2] = cov[:, 2, 0] = s[:, 5] - s[:, 0] * s[:, 2]
    cov[:, 1, 1] = s[:, 6] - s[:, 1] * s[:, 1]
    cov[:, 1, 2] = cov[:, 2, 1] = s[:, 7] - s[:, 1] * s[:, 2]
    cov[:, 2, 2] = s[:, 8] - s[:, 2] * s[:, 2]
    return cov


class Brute:
    """The LIST_MAX first rows of every row of p in (d2, tie_key) order, computed once; avg() and neighbours() of any
    list length and radius read from it."""

    def __init__(self, p, tie_key=None):
        self.p = np.ascontiguousarray(p, dtype=np.float64)
        self.n = len(self.p)
        self.idx, self.d2 = ordered(self.p, self.p, min(LIST_MAX, self.n), tie_key)

    def avg(self, k):
        found = min(k, self.n)
        return np.cumsum(np.sqrt(self.d2[:, :found]), axis=1)[:, -1] / found

    def neighbours(self, radius, max_nn):
        """(count, (n, max_nn) indices padded with -1, (n, 3, 3) covariance)."""
        take = min(max_nn, self.n)
        inside = self.d2[:, :take] < radius * radius
        idx = np.full((self.n, max_nn), -1, np.int64)
        idx[:, :take] = np.where(inside, self.idx[:, :take], -1)
        return inside.sum(1), idx, cumulant_cov(self.p, idx)


def avg(p, k):
    """Mean distance to the min(k, n) nearest rows, the row itself included: the smallest d2 ascending, np.sqrt, summed
    one after the other, / min(k, n)."""
    assert 1 <= k <= LIST_MAX
    return Brute(p).avg(k)


def neighbours(p, radius, max_nn, tie_key=None):
    """Rows with d2 < radius^2 in np.lexsort((index, d2)) order, the first max_nn: count, padded indices, covariance."""
    assert 1 <= max_nn <= LIST_MAX
    return Brute(p, tie_key).neighbours(radius, max_nn)


def nearest(p, q32):
    """Index (the smallest among equals: np.argmin takes the first minimum) and distance of the row of p nearest to each
    float32 query, widened to float64."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = np.asarray(q32, dtype=np.float32).astype(np.float64)
    idx = np.empty(len(q), np.int64)
    dist = np.empty(len(q))
    for a, e in _chunks(len(q), len(p)):
        dd = d2(q[a:e], p)
        idx[a:e] = np.argmin(dd, axis=1)
        dist[a:e] = np.sqrt(dd[np.arange(e - a), idx[a:e]])
    return idx, dist


def restate_filter(avg_, std_ratio):
    """mean and threshold of the outlier filter (include/lidarcast.h, "cloud preprocessing")."""
    n = len(avg_)
    pos = avg_[avg_ > 0]
    mean = pos.sum() / n
    return mean, mean + std_ratio * np.sqrt(((pos - mean) ** 2).sum() / (n - 1))


def nn_grid(p, cell_size):
    """lrc_nn_create's grid arithmetic restated: (cells per axis, the cell size used, rounds of the h *= 1.26 loop that
    keeps the grid at 64e6 cells or fewer)."""
    p = np.asarray(p, dtype=np.float64)
    ext = p.max(0) - p.min(0)
    h = float(cell_size)
    if not h > 0.0:
        h = np.sqrt(max(ext[0] * ext[1], ext[1] * ext[2], ext[0] * ext[2], 1e-12) / len(p)) * 2.0
    h = max(h, max(ext.max(), 1e-9) / 1024.0)
    rounds = 0
    while True:
        n = np.maximum(1, np.floor(ext / h).astype(np.int64) + 1)
        if float(n[0]) * float(n[1]) * float(n[2]) <= 64.0e6:
            return n, h, rounds
        h *= 1.26
        rounds += 1


# ---- layouts: float64 (n, 3), n <= 4096, fixed seeds ------------------------------------------------------------------
def _shuffled(p, seed):
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))])


def _grid_indices(side):
    k = np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)


def lattice(spacing=0.25, side=12, seed=0):
    """side^3 rows k * spacing: exact in binary and in float32, every shell of neighbours an exact tie."""
    return _shuffled(_grid_indices(side) * spacing, seed)


def decimal_lattice(side=12, seed=0):
    """k * 0.1 + (0.3, -1.7, 2.9): no coordinate is representable, so the grid's floor((p - lo) * inv_h) and the 1e-6 h
    shrink of the stop test decide where a row on a cell edge lands."""
    return _shuffled(_grid_indices(side) * 0.1 + np.array([0.3, -1.7, 2.9]), seed)


def two_clusters(seed=0):
    """Two clusters of 1500 rows (sigma 0.01) 50 m apart and 24 lone rows on the segment between them, in millimetres:
    the automatic cell size puts a cluster into one cell and the lone rows walk many empty shells."""
    rng = np.random.default_rng(100 + seed)
    far = np.array([40.0, 30.0, 2.0])
    a = rng.normal(0.0, 0.01, (1500, 3))
    b = rng.normal(0.0, 0.01, (1500, 3)) + far
    t = (np.arange(24) + 1.0) / 25.0
    return _shuffled(np.round(np.vstack([a, b, t[:, None] * far]), 3), seed)


def axis_line(seed=0):
    """2000 rows (k * 0.001, 0, 0): the grid is n x 1 x 1."""
    p = np.zeros((2000, 3))
    p[:, 0] = np.arange(2000) * 0.001
    return _shuffled(p, seed)


def diagonal_line(seed=0):
    """800 rows 1 cm apart along (1, 2, 3), in millimetres."""
    u = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    return _shuffled(np.round(np.arange(800)[:, None] * 0.01 * u, 3), seed)


def mm_plane(seed=0):
    """1500 uniform rows of the unit square on z = 0.3, in millimetres."""
    rng = np.random.default_rng(200 + seed)
    p = np.column_stack([rng.uniform(0, 1, 1500), rng.uniform(0, 1, 1500), np.full(1500, 0.3)])
    return _shuffled(np.round(p, 3), seed)


def identical(far=False):
    """40 copies of one row; with far, one more row 5 m away."""
    p = np.tile([[1.1, 2.3, 0.7]], (40, 1))
    return np.vstack([p, [[6.1, 2.3, 0.7]]]) if far else p


def pole(seed=0):
    """16 layers z = k * 0.25 of five rows: the axis and four arms 0.25 long.  The neighbourhood of an interior axis row
    is symmetric about the axis with more vertical than horizontal spread: covariance diag(s, s, L), s < L, exactly."""
    z = np.arange(16) * 0.25
    arms = np.array([[0.0, 0.0], [0.25, 0.0], [-0.25, 0.0], [0.0, 0.25], [0.0, -0.25]])
    p = _shuffled(np.array([[x, y, zz] for zz in z for x, y in arms]), seed)
    rows = pole_interior(p)
    cnt, _, cov = neighbours(p, 0.6, 32)
    c = cov[rows]
    off = c[:, [0, 0, 1], [1, 2, 2]]
    assert len(rows) == 12 and (cnt[rows] == 25).all() and (off == 0.0).all()
    assert (c[:, 0, 0] == c[:, 1, 1]).all() and (c[:, 0, 0] < c[:, 2, 2]).all() and (c[:, 0, 0] > 0).all()
    return p


def pole_interior(p):
    """The axis rows of pole() two layers or more from either end."""
    return np.flatnonzero((p[:, 0] == 0) & (p[:, 1] == 0) & (p[:, 2] >= 0.5) & (p[:, 2] <= 3.25))


def mm_cube(seed=0):
    """3000 uniform rows of a cube of side 0.5, in millimetres: the control."""
    return np.round(np.random.default_rng(300 + seed).uniform(0, 0.5, (3000, 3)), 3)


# ---- the normals criterion ------------------------------------------------------------------------------------------
RAYLEIGH_BOUND = 1e-9
GAP = 1e-3


def rayleigh_excess(normals, cov):
    """(n^T C n - lambda_min) / lambda_max per row, nan where lambda_max <= 0; and the eigenvalues."""
    w = np.linalg.eigvalsh(cov)
    r = np.einsum("ni,nij,nj->n", normals, cov, normals)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w[:, 2] > 0, (r - w[:, 0]) / w[:, 2], np.nan), w


def check_normals_all(got, nn, p, radius, max_nn, restated=None):
    """Every row of the normals of p is judged, ill-separated ones included:
      - nn equals the restated counts;
      - fewer than 3 neighbours give exactly (0, 0, 1);
      - every other normal is finite and of unit length within 1e-12;
      - where lambda_max > 0, (n^T C n - lambda_min) / lambda_max <= 1e-9 with the eigenvalues of the restated
        covariance: when the two smallest eigenvalues coincide any vector of their plane passes, one of another plane
        does not;
      - where the two smallest are at least 1e-3 lambda_max apart, 1 - |cos| <= 1e-9 against numpy's eigenvector.
    Returns the largest Rayleigh excess (0.0 when no row has one)."""
    cnt, _, cov = restated if restated is not None else neighbours(p, radius, max_nn)
    assert np.array_equal(np.asarray(nn).astype(np.int64), cnt), "neighbour counts differ from the brute force"
    got = np.asarray(got)
    few = cnt < 3
    assert (got[few] == [0.0, 0.0, 1.0]).all(), "fewer than 3 neighbours must give (0, 0, 1)"
    if few.all():
        return 0.0
    g, c = got[~few], cov[~few]
    assert np.isfinite(g).all()
    assert (np.abs(np.linalg.norm(g, axis=1) - 1.0) <= 1e-12).all()
    excess, w = rayleigh_excess(g, c)
    live = w[:, 2] > 0
    worst = float(excess[live].max()) if live.any() else 0.0
    assert worst <= RAYLEIGH_BOUND, f"Rayleigh excess {worst:.3g} on {int((excess[live] > RAYLEIGH_BOUND).sum())} rows"
    sep = live & ((w[:, 1] - w[:, 0]) >= GAP * w[:, 2])
    if sep.any():
        _, v = np.linalg.eigh(c[sep])
        dev = 1.0 - np.abs(np.einsum("ij,ij->i", g[sep], v[:, :, 0]))
        assert dev.max() <= 1e-9, dev.max()
    return worst
