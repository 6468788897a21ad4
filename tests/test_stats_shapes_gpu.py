"""The device frame statistics (csrc/lrc_stats.h) and the validation metrics (csrc/lrc_metrics.hip) at the shapes where
such kernels go wrong, against plain numpy.

Statistics: every segment's mean / std must carry np.mean / np.std's bits (float32 ranges, float64 incident angles) at
every summation shape of tests/stats_shapes.py -- segments above 8 x 8192 values (the second pass of the kStatPar
stride), hundreds to thousands of segments in one call (several combine workgroups), every ragged tail 1..8191, empty
segments between others, rows beyond the counts, a scratch that grows between calls, and all three ways frames_finish
calls launch_segment_stats.  tests/test_stats_shapes_discrimination.py shows on the same data that a wrong summation
order would change the bits.

Metrics: min_distances bit for bit against numpy's float32 brute force and rbf_kernel_sum against a float64 brute force,
at B sizes around the 1024-point LDS tile and A sizes around the 256-thread workgroup."""
import numpy as np
import pytest

import stats_shapes as ss
from helpers import assert_bit_equal, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    c = lidarcast.Context(0)
    yield c
    c.close()


def _segment_stats_ref(values, counts):
    off = ss.offsets(counts)
    mean = np.zeros(len(counts), dtype=values.dtype)
    std = np.zeros(len(counts), dtype=values.dtype)
    for i in range(len(counts)):
        if counts[i]:
            seg = values[off[i]:off[i + 1]]
            mean[i], std[i] = np.mean(seg), np.std(seg)
    return mean, std


def _assert_segments_equal(got, ref, counts, what):
    ne = np.flatnonzero(bits(got) != bits(ref))
    assert len(ne) == 0, f"{what}: {len(ne)} of {len(counts)} segments differ; lengths " \
                         f"{[int(counts[i]) for i in ne[:12]]}, first got {got[ne[0]]!r} want {ref[ne[0]]!r}"


def _direct(ctx, rows, counts):
    """lrc_cloud_range_stats_dev over (x, y, z, label) rows in HBM; outputs start as a poison that must be overwritten."""
    import torch
    dev = torch.device("cuda", 0)
    d_rows = torch.from_numpy(rows).to(dev)
    d_counts = torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dev)
    rng = torch.full((len(rows),), -1.0, dtype=torch.float32, device=dev)
    mean = torch.full((len(counts),), -1.0, dtype=torch.float32, device=dev)
    std = torch.full((len(counts),), -1.0, dtype=torch.float32, device=dev)
    ctx.cloud_range_stats_dev(d_rows, d_counts, rng, mean, std, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rng.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy()


def _check_direct(ctx, counts, seed, what, extra=0):
    rows = ss.rows_for(counts, seed, extra=extra)
    rng, mean, std = _direct(ctx, rows, counts)
    ref_rng = ss.row_ranges(rows)
    assert_bit_equal(rng, ref_rng, f"{what}: d_range against np.linalg.norm(rows[:, :3], axis=1)")
    ref_mean, ref_std = _segment_stats_ref(ref_rng[:int(np.sum(counts))], counts)
    _assert_segments_equal(mean, ref_mean, counts, f"{what}: mean")
    _assert_segments_equal(std, ref_std, counts, f"{what}: std")
    assert bits(mean[counts == 0]).tolist() == [0] * int((counts == 0).sum()), what     # +0 for an empty segment
    assert bits(std[counts == 0]).tolist() == [0] * int((counts == 0).sum()), what


def _scratch_values(counts, max_rows):
    """segment_stats_scratch_values: the chunk-sum scratch a call needs."""
    return max_rows // ss.CHUNK + len(counts) + 2


# ---- the direct entry point: lrc_cloud_range_stats_dev -------------------------------------------------------------------

def test_catalogue_then_small_then_every_tail_on_one_context():
    """On a fresh context: the whole catalogue in one call (~1000 segments: four combine workgroups; segments up to
    17 x 8192 + 8191 rows: the kStatPar stride loop three times), then a small call, then every length 1..8191 in one
    call (33.5 M rows, 8191 segments), whose scratch is larger than the first call left -- the scratch is reallocated."""
    import lidarcast
    c = lidarcast.Context(0)
    try:
        cat, seed = ss.direct_layout("catalogue")
        _check_direct(c, cat, seed, "catalogue")
        small, seed = ss.direct_layout("small")
        _check_direct(c, small, seed, "small after the catalogue")
        tails, seed = ss.direct_layout("every_tail")
        need1 = _scratch_values(cat, int(cat.sum()))
        assert _scratch_values(tails, int(tails.sum())) > need1 + need1 // 4         # beyond the capacity call 1 left
        _check_direct(c, tails, seed, "every tail 1..8191")
    finally:
        c.close()


def test_one_chunk_plus_every_sampled_tail(ctx):
    counts, seed = ss.direct_layout("one_chunk_plus_tail")
    _check_direct(ctx, counts, seed, "8192 + r")


def test_empty_segments_between_others(ctx):
    counts, seed = ss.direct_layout("with_empty")
    _check_direct(ctx, counts, seed, "empty segments interleaved")


def test_rows_beyond_the_counts_are_not_read(ctx):
    """max_rows larger than the sum of the counts: the rows after the last segment hold 1e18 in every coordinate; their
    ranges are computed, and no segment's statistics may change."""
    counts, seed = ss.direct_layout("with_empty")
    _check_direct(ctx, counts, seed, "poisoned tail rows", extra=3 * ss.CHUNK + 77)
    counts, seed = ss.direct_layout("small")
    _check_direct(ctx, counts, seed, "poisoned tail rows, small", extra=1)


# ---- the frames path: lrc_scan_rays_compact -> frames_finish --------------------------------------------------------------

@pytest.mark.parametrize("case", list(ss.FRAME_CASES))
def test_frames_statistics_on_every_frames_finish_path(ctx, case):
    """Host rays into a closed cube with a keep mask chosen from a first cast so that pose p keeps exactly L_p rays:
    counts equal the design, and the per-pose statistics equal np.mean / np.std of the returned columns bit for bit,
    float32 ranges and float64 incident angles."""
    import lidarcast
    from lidarcast import synth
    N, lengths = ss.FRAME_CASES[case]
    P = len(lengths)
    cube = synth.unit_cube(ss.CUBE_LO, ss.CUBE_HI)
    scene = lidarcast.Scene(ctx, cube.vertices, cube.triangles)
    try:
        rays = ss.frame_rays(P, N, seed=len(case))
        hit = np.isfinite(scene.cast(rays.reshape(-1, 6), want=("t",))["t"]).reshape(P, N)
        keep = np.zeros((P, N), dtype=bool)
        for p, L in enumerate(lengths):
            idx = np.flatnonzero(hit[p])[:L]
            assert len(idx) == L, (case, p, L, len(idx))
            keep[p, idx] = True
        want = ("range_origin", "incident_deg", "range_origin_stats", "incident_stats")
        fr = scene.scan_rays_compact(rays, keep, np.zeros((P, 3)), 1e6, want=want)
    finally:
        scene.close()
    counts = np.asarray(lengths, dtype=np.int64)
    assert np.array_equal(fr["counts"], counts), (case, fr["counts"])
    assert fr["total"] == counts.sum()
    for col, dt in (("range_origin", np.float32), ("incident", np.float64)):
        values = fr["range_origin"] if col == "range_origin" else fr["incident_deg"]
        assert values.dtype == dt and fr[f"{col}_mean"].dtype == dt
        ref_mean, ref_std = _segment_stats_ref(values, counts)
        _assert_segments_equal(fr[f"{col}_mean"], ref_mean, counts, f"{case}: {col} mean")
        _assert_segments_equal(fr[f"{col}_std"], ref_std, counts, f"{case}: {col} std")


# ---- the validation metrics at tile and workgroup edges -----------------------------------------------------------------

N_SIZES = (1, 255, 256, 257, 1000)
M_SIZES = (1, 1023, 1024, 1025, 2049, 3073)
_TILE = 1024


def _metric_clouds(n, m, seed):
    """B uniform in [-1, 1]^3; A's first rows sit 1e-4 from the B points on either side of every tile edge (B[m - 1]
    first), so a kernel that drops a tile's first or last point, or a whole partial tile, changes their minimum."""
    rng = np.random.default_rng([seed, n, m])
    b = rng.uniform(-1.0, 1.0, size=(m, 3)).astype(np.float32)
    a = rng.uniform(-1.2, 1.2, size=(n, 3))
    edges = [m - 1] + sorted({j for t in range(0, m + _TILE, _TILE) for j in (t - 1, t) if 0 <= j < m} - {m - 1})
    k = min(n, len(edges))
    a[:k] = b[edges[:k]] + rng.uniform(-1e-4, 1e-4, size=(k, 3))
    return a.astype(np.float32), b


@pytest.mark.parametrize("m", M_SIZES)
@pytest.mark.parametrize("n", N_SIZES)
def test_min_distances_bit_equal_to_numpy(n, m):
    """numpy's float32 brute force: per pair ((dx*dx + dy*dy) + dz*dz) then one sqrt -- the kernel's expression, and
    sqrt is monotonic, so the minimum must carry the same bits."""
    from lidarcast import metrics
    a, b = _metric_clouds(n, m, 1)
    ref = np.linalg.norm(a[:, None] - b, axis=2).min(1)
    assert ref.dtype == np.float32
    assert_bit_equal(metrics.min_distances(a, b), ref, f"min_distances n={n} m={m}")


def _rbf_ref(a, b, gamma):
    d = a.astype(np.float64)[:, None] - b.astype(np.float64)
    return float(np.exp(-gamma * np.einsum("ijk,ijk->ij", d, d)).sum())


def _rbf_bound(a, b, gamma):
    """Relative error bound of rbf_kernel_sum against the float64 brute force (u = 2^-53, R = max |a| + max |b|).
    The kernel's d2 = |a|^2 + |b|^2 - 2 a.b from float32 inputs (exact products, 2 roundings per 3-term sum, 2 more
    to combine) is off by at most 4u R^2; the brute force's sum of squares of exact differences by at most 3u R^2, so
    a term exp(-gamma d2) is off by at most 7u gamma R^2 relative, plus an ulp of exp on each side.  All terms are
    positive: summing them (m per thread, 8 tree levels per workgroup, one per workgroup on the host; numpy's
    pairwise sum on the other side, log2(n m) + 16 levels at most) adds at most one u of relative error per level.
    A factor of 2 covers the second-order terms."""
    u = 2.0 ** -53
    R = float(np.linalg.norm(a.astype(np.float64), axis=1).max() + np.linalg.norm(b.astype(np.float64), axis=1).max())
    n, m = len(a), len(b)
    levels = m + 8 + (n + 255) // 256 + np.log2(n * m) + 16
    return 2.0 * u * (7.0 * gamma * R * R + 4.0 + levels)


@pytest.mark.parametrize("m", M_SIZES)
@pytest.mark.parametrize("n", N_SIZES)
def test_rbf_kernel_sum_against_float64(n, m):
    from lidarcast import metrics
    a, b = _metric_clouds(n, m, 2)
    for gamma in (0.7, 6.0):
        got, ref = metrics.rbf_kernel_sum(a, b, gamma), _rbf_ref(a, b, gamma)
        bound = _rbf_bound(a, b, gamma)
        assert bound < 1e-10
        assert abs(got - ref) <= bound * ref, (n, m, gamma, got, ref, abs(got - ref) / ref, bound)
    # gamma = 0: every term is exp(-0) = 1 exactly, and n * m < 2^53 ones add exactly
    assert metrics.rbf_kernel_sum(a, b, 0.0) == float(n * m)


@pytest.mark.parametrize("n", sorted(set(N_SIZES + M_SIZES)))
def test_rbf_kernel_sum_of_a_cloud_with_itself_at_huge_gamma(n):
    """Distinct points at least 2e-3 apart and gamma = 1e12: every off-diagonal term is exp(<= -4e6) = 0, while a point
    against itself gives d2 = (|a|^2 + |a|^2) - 2 (a.a) = 0 exactly in the kernel's expression: the sum is n exactly."""
    from lidarcast import metrics
    rng = np.random.default_rng(n)
    cells = rng.choice(30 ** 3, n, replace=False)
    x = np.stack(np.unravel_index(cells, (30, 30, 30)), axis=1) * 2e-3 + (0.3, -0.7, 1.1)
    x = (x + rng.uniform(-1e-5, 1e-5, size=x.shape)).astype(np.float32)
    assert metrics.rbf_kernel_sum(x, x, 1e12) == float(n)


def test_metrics_empty_clouds():
    from lidarcast import metrics
    a = np.ones((5, 3), np.float32)
    with pytest.raises(ValueError):
        metrics.min_distances(a, np.zeros((0, 3), np.float32))
    out = metrics.min_distances(np.zeros((0, 3), np.float32), a)
    assert out.shape == (0,) and out.dtype == np.float32
    assert metrics.rbf_kernel_sum(np.zeros((0, 3), np.float32), a, 1.0) == 0.0
