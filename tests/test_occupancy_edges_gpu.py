"""GPU: occupancy_kernel (csrc/lrc_occupancy.hip) through lidarcast.OccupancyIndex against the reference's expression
(metrics_restate.occupied) at every launch edge: a vertex in the last slot of the last thread, the first vertex of a second
block (one block covers 256 x 8 vertices), a query block of exactly 64 positions and its neighbours, all six faces and a
corner of the cube, non-finite coordinates, inputs that are not C-contiguous float64, and more query blocks than one
launch holds.  The wrong kernels these cases reject are modelled in tests/test_metrics_restate_host.py."""
import numpy as np
import pytest

import metrics_restate as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


def _index(ctx, v):
    import lidarcast
    return lidarcast.OccupancyIndex(ctx, v)


@pytest.mark.parametrize("V", mr.OCC_VS)
def test_planted_vertex_sets_exactly_its_flag(ctx, V):
    for Q in mr.OCC_QS:
        v0, p = mr.occ_far(V, Q)
        far = _index(ctx, v0)
        assert not far.occupied(p, mr.OCC_HALF).any()
        for i, k in mr.occ_planted_pairs(V, Q):
            v = v0.copy()
            v[i] = p[k] + mr.OCC_INSIDE
            want = np.zeros(Q, bool)
            want[k] = True
            occ = _index(ctx, v)
            got = occ.occupied(p, mr.OCC_HALF)
            assert got.dtype == bool and np.array_equal(got, want), (V, Q, i, k, np.flatnonzero(got))
            assert not occ.occupied(p + 50.0, mr.OCC_HALF).any(), "flags of the query before"
            assert np.array_equal(occ.occupied(p, mr.OCC_HALF), want)
            occ.close()
        far.close()


def test_faces_and_corners_are_inclusive(ctx):
    V, Q = 2049, 65
    v0, p = mr.occ_far(V, Q)
    assert np.array_equal(p * 64, np.round(p * 64))            # p +- 0.125 is exact
    for vi, qi in ((V - 1, Q - 1), (0, 0), (2048, 63)):
        for name, off, ax, sgn in mr.occ_face_cases():
            v = v0.copy()
            v[vi] = p[qi] + off
            want = np.zeros(Q, bool)
            want[qi] = True
            assert np.array_equal(_index(ctx, v).occupied(p, mr.OCC_HALF), want), (name, vi, qi)
            v[vi, ax] = np.nextafter(v[vi, ax], sgn * np.inf)
            assert not _index(ctx, v).occupied(p, mr.OCC_HALF).any(), (name, vi, qi, "one ulp outside")
    v = v0.copy()
    v[V - 1] = p[Q - 1]
    v[7] = np.nextafter(p[3], np.inf)
    occ = _index(ctx, v)
    want = np.zeros(Q, bool)
    want[Q - 1] = True
    assert np.array_equal(occ.occupied(p, 0.0), want)          # half = 0: only the coincident vertex
    assert not occ.occupied(p, -0.125).any() and not occ.occupied(p, -1.0 / 64).any()      # negative half: nothing
    for half in (0.0, -1e-300, 1.0 / 64, 5e-324):
        assert np.array_equal(occ.occupied(p, half), mr.occupied(v, p, half)), half


def test_non_finite_coordinates_answer_as_numpy(ctx):
    hits = 0
    for name, v, p, half in mr.occ_nonfinite_cases():
        want = mr.occupied(v, p, half)
        assert np.array_equal(_index(ctx, v).occupied(p, half), want), name
        hits += int(want.sum())
    assert hits > 20


def test_input_layouts_equal_the_plain_call(ctx):
    rng = np.random.default_rng(3)
    v = rng.integers(0, 320, (4097, 3)).astype(np.float64) / 64.0      # float32 holds these exactly
    p = rng.integers(-32, 352, (129, 3)).astype(np.float64) / 64.0
    want = _index(ctx, v).occupied(p, mr.OCC_HALF)
    assert np.array_equal(want, mr.occupied(v, p, mr.OCC_HALF)) and 5 < want.sum() < 124
    v2, p2 = np.repeat(v, 2, 0), np.repeat(p, 2, 0)
    for tag, x, y in (("float32", v.astype(np.float32), p.astype(np.float32)),
                      ("every second row", v2[::2], p2[::2]),
                      ("Fortran order", np.asfortranarray(v), np.asfortranarray(p)),
                      ("column slice", np.hstack([v, v])[:, 3:], np.hstack([p, p])[:, :3]),
                      ("list of lists", v.tolist(), p.tolist())):
        assert np.array_equal(_index(ctx, x).occupied(y, mr.OCC_HALF), want), tag


def test_more_query_blocks_than_one_launch_holds(ctx):
    """65 535 blocks of 64 positions fill gridDim.y; 65 more positions need a second launch."""
    Q = 65535 * 64 + 65
    p = np.empty((Q, 3))
    p[:] = (1.0, 2.0, 3.0)
    v, _ = mr.occ_far(9, 1)
    hit = (Q - 1, 65535 * 64 - 1)
    p[hit[0]] = (-7.0, 0.5, 0.25)
    p[hit[1]] = (9.0, -4.0, 0.75)
    v[8] = p[hit[0]] + mr.OCC_INSIDE
    v[0] = p[hit[1]] - mr.OCC_INSIDE
    got = _index(ctx, v).occupied(p, mr.OCC_HALF)
    assert got.shape == (Q,) and sorted(np.flatnonzero(got)) == sorted(hit)
