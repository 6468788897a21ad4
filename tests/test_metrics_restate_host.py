"""No GPU.  tests/metrics_restate.py is what the metrics and occupancy kernels are compared with on the device
(tests/test_metrics_edges_gpu.py, tests/test_occupancy_edges_gpu.py), so here
  * min_dist32 is numpy's own float32 computation, bit for bit, and within 4 * 2**-24 of the float64 reference
    (three correctly rounded differences, three squares, two sums and one square root: <= 3.5 * 2**-24);
  * numpy's expanded float64 RBF sum stays inside rbf_bound of the long-double direct form;
  * discrimination, in the manner of tests/test_stats_shapes_discrimination.py: a bit-equal pass on the device only
    means something if a subtly wrong kernel would have failed.  Each wrong model below is run through the same cases and
    the same comparisons as the device tests and must be rejected by at least one of them; the rejecting cases are printed.
"""
import numpy as np
import pytest

import metrics_restate as mr
from helpers import bits

REL32 = 4 * 2.0 ** -24


def _numpy_min(a, b):
    return np.linalg.norm(a[:, None] - b, axis=2).min(1)


@pytest.mark.parametrize("scale", [0.01, 1.0, 50.0, 1000.0])
def test_min_dist32_is_numpys_computation_and_near_float64(scale):
    worst = 0.0
    for n, m in ((257, 1025), (64, 255), (1, 1), (513, 2049)):
        a, b = mr.general_clouds(n, m, scale)
        for x, y in ((a, b), (b, a)):
            got = mr.min_dist32(x, y)
            want = _numpy_min(x, y)
            assert got.dtype == want.dtype == np.float32
            assert np.array_equal(bits(got), bits(want)), (scale, n, m)
            ref = mr.min_dist64(x, y)
            zero = ref == 0.0
            assert zero.sum() >= min(len(x), len(y), 100) // 2          # the coincident rows are there
            assert np.array_equal(bits(got[zero]), np.zeros(int(zero.sum()), np.uint32))      # exactly +0.0
            rel = np.abs(got[~zero].astype(np.float64) - ref[~zero]) / ref[~zero]
            if rel.size:
                worst = max(worst, float(rel.max()))
            ulp = np.spacing(np.abs(x).max())
            assert ((ref > 0) & (ref <= 2 * ulp)).any() or min(n, m) == 1    # the one-ulp neighbours are there
    print(f"scale {scale}: worst min_dist32 error / (4 * 2**-24) = {worst / REL32:.3f}")
    assert worst <= REL32


@pytest.mark.parametrize("scale", mr.SCALES)
def test_numpy_expanded_rbf_stays_inside_rbf_bound(scale):
    worst = 0.0
    for n, m in ((257, 1025), (63, 255), (1, 1)):
        a, b = mr.general_clouds(n, m, scale)
        for gamma in (0.0, 0.7, 10.0, 1.0 / (scale * scale)):
            ref = mr.rbf64(a, b, gamma)
            got = mr.rbf_expanded64(a, b, gamma)
            ratio = float(abs(np.longdouble(got) - ref) / ref) / mr.rbf_bound(a, b, gamma)
            worst = max(worst, ratio)
    print(f"scale {scale}: worst expanded-form error / rbf_bound = {worst:.4f}")
    assert worst <= 1.0


def test_exact_rbf_cases_are_exact_in_numpy():
    """gamma = 0 counts the pairs; on a lattice cloud against itself the large gamma leaves the diagonal alone."""
    for scale in mr.SCALES:
        for n in (1, 257, 3079):
            x = mr.lattice_cloud(n, scale)
            for i in range(0, n, 97):                     # every 97th row against all the others
                assert n == 1 or mr.min_dist64(x[i:i + 1], np.delete(x, i, 0))[0] >= 0.1 * scale
            assert len(np.unique(x, axis=0)) == n
            assert mr.rbf_expanded64(x, x, mr.big_gamma(scale)) == float(n)
            assert mr.rbf_expanded64(x, x[:5], 0.0) == float(n * len(x[:5]))


# ---- wrong models of min_dist_kernel / rbf_sum_kernel --------------------------------------------------------------
# A model is (rows of B the kernel would really visit, rows of A it would really write).

def _b_exact(b):
    return b


def _b_drop_last_partial(b):
    return b[:-1] if len(b) % mr.TILE else b


def _b_stale_tail(b):
    """The partial last tile read to the full 1024 rows: the slots past its end still hold the tile before (for a single
    partial tile LDS holds nothing of this launch: modelled as the last row again)."""
    r = len(b) % mr.TILE
    if r == 0:
        return b
    base = len(b) - r
    stale = b[base - mr.TILE + r:base] if base else np.repeat(b[-1:], mr.TILE - r, 0)
    return np.concatenate([b, stale])


def _b_skip_first_of_tile(b):
    keep = np.arange(len(b)) % mr.TILE != 0
    return b[keep]


def _written_all(n):
    return n


def _written_full_blocks(n):
    return n // mr.BLOCK * mr.BLOCK


MODELS = {
    "last row of a partial B tile dropped": (_b_drop_last_partial, _written_all),
    "partial last tile read to 1024 rows": (_b_stale_tail, _written_all),
    "rows of A past the last full block unwritten": (_b_exact, _written_full_blocks),
    "first row of each tile skipped": (_b_skip_first_of_tile, _written_all),
}


def _model_min(a, b, model, rows=slice(None)):
    """The model's output for ``rows`` of A."""
    fb, fw = MODELS[model]
    bb = fb(b)
    out = mr.min_dist32(a[rows], bb) if len(bb) else np.full(len(a[rows]), np.inf, np.float32)
    out[np.arange(len(a))[rows] >= fw(len(a))] = 0.0      # the output buffer as the allocator may hand it out
    return out


def _model_rbf(a, b, gamma, model):
    fb, fw = MODELS[model]
    bb = fb(b)
    return mr.rbf_expanded64(a[:fw(len(a))], bb, gamma) if len(bb) and fw(len(a)) else 0.0


def _same(x, y):
    return np.array_equal(bits(x), bits(y))


def test_min_dist_checks_reject_every_wrong_model():
    """The planted-row check and the bit-for-bit check on general clouds, as the device test makes them."""
    rejected = {k: [] for k in MODELS}
    for n, m in mr.SHAPES:
        a, b = mr.far_clouds(n, m)
        want0 = mr.min_dist32(a, b)
        got0 = {k: _model_min(a, b, k) for k in MODELS}
        for i, k in mr.planted_pairs(n, m):
            a2, d = mr.plant(a, b, i, k)
            want = want0.copy()
            want[i:i + 1] = mr.min_dist32(a2[i:i + 1], b)
            assert bits(want[i]) == bits(d), "the planted row is not the nearest"
            for name in MODELS:
                got = got0[name].copy()
                got[i:i + 1] = _model_min(a2, b, name, slice(i, i + 1))
                if not _same(got, want):
                    rejected[name].append(f"planted {n}x{m} A{i} B{k}")
        a, b = mr.general_clouds(n, m, 1.0)
        want = mr.min_dist32(a, b)
        for name in MODELS:
            if not _same(_model_min(a, b, name), want):
                rejected[name].append(f"general {n}x{m}")
    for name, cases in rejected.items():
        print(f"min_distances, {name}: rejected by {len(cases)} cases, e.g. {cases[:4]}")
    # the stale tail re-reads rows that were already counted: a minimum cannot show it, the RBF sum does (below)
    assert rejected.pop("partial last tile read to 1024 rows") == []
    assert all(rejected.values()), {k: len(v) for k, v in rejected.items()}


def test_rbf_checks_reject_every_wrong_model():
    """gamma = 0 must give exactly n * m at every shape; gamma = 0.7 must stay inside rbf_bound of rbf64."""
    rejected = {k: [] for k in MODELS}
    for n, m in mr.SHAPES:
        for name, (fb, fw) in MODELS.items():
            idx = np.arange(m)
            if float(fw(n)) * float(len(fb(idx))) != float(n) * float(m):      # exp(-0 * d2) = 1 for every pair visited
                rejected[name].append(f"gamma 0 {n}x{m}")
    for n, m in ((257, 1025), (513, 3079), (63, 255), (257, 1)):
        a, b = mr.general_clouds(n, m, 1.0)
        ref = mr.rbf64(a, b, 0.7)
        tol = mr.rbf_bound(a, b, 0.7)
        assert abs(np.longdouble(mr.rbf_expanded64(a, b, 0.7)) - ref) <= tol * ref
        for name in MODELS:
            if not abs(np.longdouble(_model_rbf(a, b, 0.7, name)) - ref) <= tol * ref:
                rejected[name].append(f"gamma 0.7 {n}x{m}")
    for name, cases in rejected.items():
        print(f"rbf_kernel_sum, {name}: rejected by {len(cases)} cases, e.g. {cases[:4]}")
    assert all(rejected.values()), {k: len(v) for k, v in rejected.items()}


def test_nonfinite_cases_reject_the_clamp_that_drops_nan():
    """min_dist_kernel with `best = d2 < best ? d2 : best` (a NaN never wins) and rbf_sum_kernel with
    `d2 > 0 ? d2 : 0` (a NaN becomes 0 and adds exp(0) = 1)."""
    def min_nan_dropped(a, b):
        with np.errstate(all="ignore"):
            d = a[:, None, :] - b[None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            return np.sqrt(np.fmin.reduce(d2, axis=1, initial=np.float32(np.inf)))

    rej_min, rej_rbf, nan_rows, nan_sums = [], [], 0, 0
    for name, a, b in mr.nonfinite_cases():
        want = mr.min_dist32(a, b)
        nan_rows += int(np.isnan(want).sum())
        if not np.array_equal(min_nan_dropped(a, b), want, equal_nan=True):
            rej_min.append(name)
        for gamma in (0.0, 0.7):
            want = mr.rbf_expanded64(a, b, gamma)
            nan_sums += bool(np.isnan(want))
            assert not mr.rbf64_isnan(a, b, gamma) or np.isnan(want)           # NaN wherever the direct form is NaN
            if np.isnan(mr.rbf_expanded64(a, b, gamma, clamp_nan=True)) != np.isnan(want):
                rej_rbf.append(f"{name} gamma {gamma}")
    print(f"NaN dropped in min: rejected by {len(rej_min)} cases, e.g. {rej_min[:4]}")
    print(f"NaN clamped in rbf: rejected by {len(rej_rbf)} cases, e.g. {rej_rbf[:4]}")
    assert rej_min and rej_rbf and nan_rows and nan_sums
    # all of them are caught except where numpy itself has no NaN (an infinite coordinate against finite ones)
    for name, a, b in mr.nonfinite_cases():
        if np.isnan(mr.min_dist32(a, b)).any():
            assert name in rej_min, name


# ---- wrong models of occupancy_kernel ------------------------------------------------------------------------------

def _occ_exclusive(face):
    def f(v, p, half, state):
        with np.errstate(all="ignore"):
            lo = v[None] >= (p - half)[:, None]
            hi = v[None] <= (p + half)[:, None]
            ax, upper = divmod(face, 2)
            if upper:
                hi[..., ax] = v[None, :, ax] < (p[:, ax] + half)[:, None]
            else:
                lo[..., ax] = v[None, :, ax] > (p[:, ax] - half)[:, None]
            return (lo & hi).all(2).any(1)
    return f


def _occ_vertex_tail(v, p, half, state):
    return mr.occupied(v[:-1], p, half) if len(v) > 1 else np.zeros(len(p), bool)


def _occ_last_of_block(v, p, half, state):
    out = mr.occupied(v, p, half)
    q = np.arange(len(p))
    last = (q % mr.OCC_Q == mr.OCC_Q - 1) | (q == len(p) - 1)
    out[last] = False
    return out


def _occ_not_cleared(v, p, half, state):
    out = mr.occupied(v, p, half)
    if state.get("flags") is not None and len(state["flags"]) == len(out):
        out = out | state["flags"]
    state["flags"] = out
    return out


OCC_MODELS = {f"exclusive comparison on face {'xyz'[f // 2]}{'-+'[f % 2]}": _occ_exclusive(f) for f in range(6)}
OCC_MODELS.update({"vertex tail v0 + j < V - 1": _occ_vertex_tail,
                   "only the first nq - 1 positions of a block answered": _occ_last_of_block,
                   "flags not cleared between queries": _occ_not_cleared})


def test_occupancy_checks_reject_every_wrong_model():
    """The planted-vertex check with its second query, then the faces and the corner.  To stay quick here the planted
    pairs are modelled at every Q for V <= 9 and at Q = 65 for the larger V (the device test runs them all), and the
    exclusive faces are modelled on the face cases only."""
    rejected = {k: [] for k in OCC_MODELS}
    structural = {k: f for k, f in OCC_MODELS.items() if not k.startswith("exclusive")}
    for V in mr.OCC_VS:
        for Q in (mr.OCC_QS if V <= 9 else (65,)):
            v0, p = mr.occ_far(V, Q)
            assert not mr.occupied(v0, p, mr.OCC_HALF).any()
            for i, k in mr.occ_planted_pairs(V, Q):
                v = v0.copy()
                v[i] = p[k] + mr.OCC_INSIDE
                want = np.zeros(Q, bool)
                want[k] = True
                assert np.array_equal(mr.occupied(v, p, mr.OCC_HALF), want)
                far = p + 50.0                               # the second query of the same index: nothing set
                for name, f in structural.items():
                    state = {}
                    if not (np.array_equal(f(v, p, mr.OCC_HALF, state), want)
                            and not f(v, far, mr.OCC_HALF, state).any()):
                        rejected[name].append(f"planted V{V} Q{Q} v{i} q{k}")
    V, Q = 2049, 65
    v0, p = mr.occ_far(V, Q)
    for cname, off, ax, sgn in mr.occ_face_cases():
        v = v0.copy()
        v[V - 1] = p[Q - 1] + off
        assert mr.occupied(v, p, mr.OCC_HALF)[Q - 1] and mr.occupied(v, p, mr.OCC_HALF).sum() == 1
        for name, f in OCC_MODELS.items():
            if not f(v, p, mr.OCC_HALF, {})[Q - 1]:
                rejected[name].append(cname)
        v[V - 1, ax] = np.nextafter(v[V - 1, ax], sgn * np.inf)
        assert not mr.occupied(v, p, mr.OCC_HALF).any()
    for name, cases in rejected.items():
        print(f"occupancy, {name}: rejected by {len(cases)} cases, e.g. {cases[:4]}")
    assert all(rejected.values()), {k: len(v) for k, v in rejected.items()}


def test_occupied_is_the_per_position_expression():
    for name, v, p, half in mr.occ_nonfinite_cases():
        with np.errstate(all="ignore"):
            want = np.array([np.any(np.all((v >= q - half) & (v <= q + half), axis=1)) for q in p])
        assert np.array_equal(mr.occupied(v, p, half), want), name
