"""CPU: the numpy restatement of the semantic occupancy grid (tests/voxgrid_restate.py) against hand answers, the grid
checks of the Python layer, the default extent, and the compiled voxgrid kernels' resources and walk arithmetic."""
import os
import re
import subprocess

import numpy as np
import pytest

import voxgrid_restate as R
from conftest import PKG


def _run(o, e, labels=None, origin=(0.0, 0.0, 0.0), s=1.0, dims=(10, 3, 3), min_returns=1):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    e = np.asarray(e, np.float32).reshape(-1, 3)
    lab = np.zeros(len(o), np.uint32) if labels is None else np.asarray(labels, np.uint32)
    return R.grid_from_rays(o, e, lab, origin, s, dims, min_returns)


def _cells(state, dims, value):
    return {tuple(int(x) for x in c) for c in np.argwhere(state.reshape(dims) == value)}


def test_axis_aligned_ray_through_five_voxels():
    sp, st, c = _run([0.5, 1.5, 1.5], [4.5, 1.5, 1.5], labels=[3 | (7 << 16)])
    dims = (10, 3, 3)
    assert _cells(st, dims, R.FREE) == {(x, 1, 1) for x in range(4)}
    assert _cells(st, dims, R.OCCUPIED) == {(4, 1, 1)}
    assert list(sp["idx"]) == [(4 * 3 + 1) * 3 + 1] and list(sp["sem"]) == [3] and list(sp["ins"]) == [7]
    assert list(sp["returns"]) == [1]
    assert c == {"free": 4, "occupied": 1, "unknown": 90 - 5, "num_sparse": 1, "returns": 1, "rejected_rays": 0}
    free, end, ok, visited = R.walk(np.float32([[0.5, 1.5, 1.5]]), np.float32([[4.5, 1.5, 1.5]]), (0, 0, 0), 1.0, dims)
    assert list(visited) == [5] and ok.all() and list(end[0]) == [4, 1, 1]


def test_negative_direction():
    sp, st, _ = _run([4.5, 1.5, 1.5], [0.5, 1.5, 1.5])
    assert _cells(st, (10, 3, 3), R.FREE) == {(x, 1, 1) for x in range(1, 5)}
    assert _cells(st, (10, 3, 3), R.OCCUPIED) == {(0, 1, 1)}


def test_exact_voxel_corner_breaks_ties_x_then_y_then_z():
    dims = (3, 3, 3)
    sp, st, c = _run([0.5, 0.5, 0.5], [2.5, 2.5, 2.5], dims=dims)
    # tMax = 0.25 on every axis: x, then y, then z, then again x, y, z
    assert _cells(st, dims, R.FREE) == {(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)}
    assert _cells(st, dims, R.OCCUPIED) == {(2, 2, 2)}
    # the same segment backwards: ties still go x, y, z
    sp, st, c = _run([2.5, 2.5, 2.5], [0.5, 0.5, 0.5], dims=dims)
    assert _cells(st, dims, R.FREE) == {(2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1), (0, 1, 1), (0, 0, 1)}
    # a tie on two axes only
    sp, st, c = _run([0.5, 0.5, 0.5], [1.5, 1.5, 0.5], dims=dims)
    assert _cells(st, dims, R.FREE) == {(0, 0, 0), (1, 0, 0)} and _cells(st, dims, R.OCCUPIED) == {(1, 1, 0)}


def test_start_voxel_equals_end_voxel_carves_nothing():
    sp, st, c = _run([0.2, 0.2, 0.2], [0.7, 0.6, 0.9], labels=[4])
    assert c["free"] == 0 and c["occupied"] == 1 and list(sp["idx"]) == [0] and list(sp["sem"]) == [4]


def test_sensor_outside_the_grid_enters_it():
    dims = (3, 3, 3)
    sp, st, c = _run([-2.5, 1.5, 1.5], [1.5, 1.5, 1.5], dims=dims)
    assert _cells(st, dims, R.FREE) == {(0, 1, 1)} and _cells(st, dims, R.OCCUPIED) == {(1, 1, 1)}
    # diagonal entry through the grid's corner region
    sp, st, c = _run([-1.5, -1.5, 0.5], [1.5, 1.5, 0.5], dims=dims)
    assert _cells(st, dims, R.FREE) == {(0, 0, 0), (1, 0, 0)}
    assert _cells(st, dims, R.OCCUPIED) == {(1, 1, 0)}


def test_end_voxel_outside_the_grid_records_no_return():
    dims = (3, 3, 3)
    sp, st, c = _run([0.5, 1.5, 1.5], [5.5, 1.5, 1.5], dims=dims)
    assert _cells(st, dims, R.FREE) == {(0, 1, 1), (1, 1, 1), (2, 1, 1)}
    assert c["occupied"] == 0 and c["num_sparse"] == 0 and len(sp["idx"]) == 0


def test_voting_ties_for_sem_and_for_ins():
    dims = (3, 3, 3)
    o = [[0.5, 0.5, 0.5]] * 9
    e = [[2.5, 0.5, 0.5]] * 4 + [[0.5, 2.5, 0.5]] * 5
    lab = [2 | (7 << 16), 2 | (4 << 16), 3 | (1 << 16), 3 | (9 << 16),          # sem 2 vs 3: 2 each -> 2; ins 7 vs 4 -> 4
           5 | (1 << 16), 5 | (1 << 16), 6 | (2 << 16), 6 | (2 << 16), 6 | (3 << 16)]   # sem 6 (3 votes), ins 2
    sp, st, c = _run(o, e, lab, dims=dims)
    got = {int(i): (int(s), int(n), int(r)) for i, s, n, r in zip(sp["idx"], sp["sem"], sp["ins"], sp["returns"])}
    assert got == {18: (2, 4, 4), 6: (6, 2, 5)}
    assert list(sp["idx"]) == [6, 18]                                           # ascending by linear index


def test_min_returns_leaves_a_voxel_free_or_unknown():
    dims = (10, 3, 3)
    # voxel (2,1,1): one return, and a second ray passes through it (free bit); voxel (0,0,0): one return, no free bit
    o = [[0.5, 1.5, 1.5], [0.5, 1.5, 1.5], [0.2, 0.2, 0.2]]
    e = [[2.5, 1.5, 1.5], [4.5, 1.5, 1.5], [0.7, 0.7, 0.7]]
    sp, st, c = _run(o, e, dims=dims, min_returns=2)
    s3 = st.reshape(dims)
    assert s3[2, 1, 1] == R.FREE and s3[0, 0, 0] == R.UNKNOWN and s3[4, 1, 1] == R.UNKNOWN
    assert c["occupied"] == 0 and c["num_sparse"] == 3 and c["free"] == 4
    sp1, st1, c1 = _run(o, e, dims=dims, min_returns=1)
    assert st1.reshape(dims)[2, 1, 1] == R.OCCUPIED and c1["occupied"] == 3
    with pytest.raises(ValueError):
        R.finalize(np.zeros(90, bool), [], [], [], dims, min_returns=0)


def test_rejected_rays_carve_nothing():
    dims = (3, 3, 3)
    sp, st, c = _run([[0.5, 0.5, 0.5], [np.inf, 0.5, 0.5], [0.5, 0.5, 0.5]],
                     [[3e9, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], dims=dims)
    assert c["rejected_rays"] == 2 and _cells(st, dims, R.FREE) == {(0, 0, 0), (1, 0, 0)}
    assert list(sp["idx"]) == [18]
    # a walk of 2^24 steps is refused
    free, end, ok, visited = R.walk(np.float32([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]),
                                    np.float32([[2.0 ** 24 + 0.5, 0.5, 0.5], [3.5, 0.5, 0.5]]), (0, 0, 0), 1.0, (4, 1, 1))
    assert list(ok) == [False, True] and list(visited) == [0, 4] and free[:3].all() and not free[3]


def test_restated_walk_is_six_connected_and_order_free():
    rng = np.random.default_rng(3)
    dims = (23, 17, 11)
    o = rng.uniform(-0.3, 1.3, (400, 3)).astype(np.float32)
    e = rng.uniform(-0.3, 1.3, (400, 3)).astype(np.float32)
    lab = rng.integers(0, 4, 400).astype(np.uint32) | (rng.integers(0, 3, 400).astype(np.uint32) << 16)
    g, s = (-0.1, -0.05, 0.0), 0.05
    free, end, ok, visited = R.walk(o, e, g, s, dims)
    a, b = R.voxel_of(o.astype(np.float64), g, s), R.voxel_of(e.astype(np.float64), g, s)
    assert ok.all() and np.array_equal(visited, np.abs(b - a).sum(1) + 1)
    sp, st, c = R.grid_from_rays(o, e, lab, g, s, dims)
    p = rng.permutation(400)
    sp2, st2, c2 = R.grid_from_rays(o[p], e[p], lab[p], g, s, dims)
    assert np.array_equal(st, st2) and c == c2 and all(np.array_equal(sp[k], sp2[k]) for k in sp)


# ---- the Python layer's checks (before any device is touched) -------------------------------------------------------
@pytest.mark.parametrize("origin, s, dims", [
    ((0, 0, 0), 0.0, (2, 2, 2)), ((0, 0, 0), -0.1, (2, 2, 2)), ((0, 0, 0), np.inf, (2, 2, 2)),
    ((0, 0, 0), np.nan, (2, 2, 2)), ((0, 0, 0), "a", (2, 2, 2)),
    ((0, 0, 0), 0.1, (0, 2, 2)), ((0, 0, 0), 0.1, (2, -1, 2)), ((0, 0, 0), 0.1, (2, 2)),
    ((0, 0, 0), 0.1, (2, 2, 2.5)), ((0, 0, 0), 0.1, (2048, 1024, 1024)),
    ((0, np.nan, 0), 0.1, (2, 2, 2)), ((0, 0), 0.1, (2, 2, 2))])
def test_bad_grids_are_refused_before_any_device(origin, s, dims):
    from lidarcast import OccupancyGrid
    from lidarcast.voxgrid import check_grid
    with pytest.raises(ValueError):
        check_grid(origin, s, dims)
    with pytest.raises(ValueError):
        OccupancyGrid(None, origin, s, dims)                   # no context at all: refused before it is needed


def test_largest_grid_is_accepted():
    from lidarcast.voxgrid import check_grid
    assert check_grid((0, 0, 0), 0.1, (2 ** 31 - 1, 1, 1))[2] == (2 ** 31 - 1, 1, 1)
    assert check_grid([1, 2, 3], 1, np.array([4, 5, 6], np.int64)) == (pytest.approx([1, 2, 3]), 1.0, (4, 5, 6))


@pytest.mark.parametrize("name, s", [("synth_A6_office2", 0.05), ("synth_hall", 0.02), ("synth_A6_office2", 0.3)])
def test_default_extent_holds_every_vertex(name, s):
    from lidarcast import synth
    from lidarcast.voxgrid import default_extent
    m = synth.make_scene(name)
    origin, dims = default_extent(m.vertices, s)
    c = R.voxel_of(m.vertices, origin, s)
    assert (c >= 0).all() and (c <= np.array(dims) - 2).all()
    lo, hi = m.vertices.min(0), m.vertices.max(0)
    assert np.array_equal(origin, lo - s) and dims == tuple(int(x) + 2 for x in np.floor((hi - (lo - s)) / s))


# ---- compiled resources and walk arithmetic ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    d = tmp_path_factory.mktemp("vox_res")
    src = os.path.join(PKG, "csrc", "lrc_voxgrid.hip")
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(d / "v.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split()[0]] = int(m.group(2))
    a = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", str(d / "v.s")], capture_output=True,
                       text=True)
    assert a.returncode == 0, a.stderr[-4000:]
    return res, (d / "v.s").read_text()


KERNELS = ("walk_kernel", "head_kernel", "dense_kernel", "vote_kernel", "popcount_kernel", "counts_kernel")


def test_voxgrid_kernels_have_no_scratch_and_eight_waves(compiled):
    res, _ = compiled
    for k in KERNELS:
        names = [n for n in res if k in n and "rocprim" not in n]
        assert len(names) == 1, (k, list(res))
        u = res[names[0]]
        print(f"{k}: VGPRs {u['VGPRs']}, waves/SIMD {u['Occupancy']}, scratch {u['ScratchSize']} B/lane")
        assert u["ScratchSize"] == 0, (k, u)
        assert u["Occupancy"] == 8, (k, u)          # the walk is latency-bound: it keeps every wave slot
        assert u["VGPRs"] <= 64, (k, u)
    # the rocprim sort / encode / scan instantiated for gfx950 spill nothing either
    for n, u in res.items():
        if "rocprim" in n and u.get("VGPRs", 0) > 0:
            assert u["ScratchSize"] == 0, (n, u)


def _walk_body(asm):
    m = re.search(r"^(_ZN\S*walk_kernel\S*):", asm, re.M)
    body = asm[m.end():]
    return [ln.split()[0] for ln in body[:body.index("s_endpgm")].splitlines() if ln.strip().startswith("v_")]


def test_walk_kernel_has_no_fused_walk_arithmetic(compiled):
    """The walk's float64 arithmetic (voxel coordinates, tMax, tDelta, the boundary planes and tMax += tDelta) is
    unfused.  The only f64 FMAs left are gen_ray's explicit dgemm_row (3 x 3: the scan's own direction arithmetic) and
    the residual steps of the correctly rounded divisions (5 per v_div_fixup_f64: 6 voxel coordinates, 3 tMax, 3
    tDelta)."""
    _, asm = compiled
    ins = _walk_body(asm)
    fma = sum(x.startswith(("v_fma_f64", "v_fmac_f64")) for x in ins)
    div = sum(x.startswith("v_div_fixup_f64") for x in ins)
    mul = sum(x.startswith("v_mul_f64") for x in ins)
    assert div == 12, div
    assert fma == 9 + 5 * div, (fma, div)
    assert mul == div + 3, mul                     # one quotient product per division + the 3 plane products (a + 1) * s
    assert sum(x.startswith("v_floor_f64") for x in ins) == 6
    assert not any(x.startswith(("v_fma_mix", "v_fmac_f64_dpp", "v_pk_fma_f64")) for x in ins)


def test_library_exports_the_voxgrid_symbols():
    import lidarcast
    lib = lidarcast.load()
    names = ("lrc_voxgrid_create", "lrc_voxgrid_destroy", "lrc_voxgrid_get_info", "lrc_voxgrid_reset",
             "lrc_voxgrid_accumulate_dev", "lrc_voxgrid_finalize", "lrc_voxgrid_finalize_dev", "lrc_voxgrid_export_bits")
    for n in names:
        assert hasattr(lib, n), n
        assert n in lidarcast._capi.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", lidarcast.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (lrc_voxgrid_\w+)", out))
    assert exported == set(names)
