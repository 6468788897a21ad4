"""CPU: the numpy restatement of surface coverage (tests/coverage_restate.py) against hand-computed answers, the
planner's ``selection`` argument, and the coverage kernels' compiled resources."""
import os
import re
import subprocess

import numpy as np
import pytest

import coverage_restate as R
from conftest import PKG


def _cube():
    from lidarcast import synth
    return synth.unit_cube()


def test_unit_cube_areas_are_exact():
    m = _cube()
    q = R.area_q(m.vertices, m.triangles)
    assert q.dtype == np.uint64 and (q == np.uint64(2 << 32)).all()          # every triangle: half of a 2 x 2 face
    assert sum(int(x) for x in q) * 2.0 ** -32 == 24.0


def test_two_triangles_sharing_an_edge_and_a_zero_area_triangle():
    v = np.array([[0, 0, 0], [3, 0, 0], [3, 2, 0], [0, 2, 0], [6, 0, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]], np.int32)                 # the last one is degenerate (collinear)
    q = R.area_q(v, f)
    assert list(q) == [3 << 32, 3 << 32, 0]
    q2 = R.area_q(np.array([[0, 0, 0], [1e-5, 0, 0], [0, 1e-5, 0]]), np.array([[0, 1, 2]]))
    assert int(q2[0]) == int(np.rint(0.5e-10 * 2.0 ** 32)) == 0                # below the quantum: rounds to 0


def test_oversized_meshes_are_refused_by_the_restatement():
    with pytest.raises(ValueError):
        R.area_q(np.array([[0, 0, 0], [2e5, 0, 0], [0, 2e5, 0]]), np.array([[0, 1, 2]]))     # one triangle past 2^63
    v = np.array([[0, 0, 0], [4e4, 0, 0], [0, 4e4, 0]], np.float64)                          # 8e8 m^2 each, 3 of them
    with pytest.raises(ValueError):
        R.area_q(v, np.array([[0, 1, 2]] * 3))
    assert len(R.area_q(v, np.array([[0, 1, 2]] * 2))) == 2


def test_accumulate_by_hand():
    T = 40
    inf = np.inf
    # two poses x 6 rays: misses, a range-filtered hit (finite prim, t = inf), an invalid prim, a run of equal prims
    t = np.array([1, 1, 1, inf, inf, 2, 1, inf, 1, 1, 1, 1], np.float32)
    prim = np.array([3, 3, 3, 5, R.INVALID, 39, 7, 7, 33, 33, 3, 50], np.uint32)   # 50 >= T: ignored
    seen, hits, ret = R.accumulate(t, prim, 2, 6, 2, T)
    assert set(np.flatnonzero(seen[0])) == {3, 39} and set(np.flatnonzero(seen[1])) == {3, 7, 33}
    assert hits[3] == 4 and hits[39] == 1 and hits[7] == 1 and hits[33] == 2 and hits[5] == 0 and hits.sum() == 8
    assert list(ret) == [4, 4]
    bits = R.pack(seen)
    assert bits.shape == (2, 2) and bits[0, 0] == (1 << 3) and bits[0, 1] == (1 << 7)
    # set_of_pose maps both poses to set 1; an entry >= num_sets drops the pose
    seen2, _, ret2 = R.accumulate(t, prim, 2, 6, 2, T, set_of_pose=[1, 1])
    assert not seen2[0].any() and set(np.flatnonzero(seen2[1])) == {3, 7, 33, 39} and list(ret2) == [0, 8]
    _, hits3, ret3 = R.accumulate(t, prim, 2, 6, 2, T, set_of_pose=[0, 2])
    assert list(ret3) == [4, 0] and hits3.sum() == 4


def test_summary_by_hand():
    q = np.array([1, 2, 4, 8, 16], np.uint64)
    sem = np.array([0, 0, 2, 2, 7])
    mask = np.array([1, 0, 1, 0, 1], bool)
    assert R.covered_q(mask, q) == 21
    assert R.per_class(mask, q, sem) == {0: (1, 3), 2: (4, 12), 7: (16, 16)}


def test_greedy_ties_and_stops():
    q = np.array([5, 5, 3, 3, 1, 0], np.uint64)
    seen = np.array([[0, 0, 1, 1, 0, 0],      # 6
                     [1, 0, 0, 0, 1, 0],      # 6: tie with set 0 -> set 0 first
                     [1, 1, 0, 0, 0, 0],      # 10
                     [0, 0, 0, 0, 0, 1]], bool)  # gain 0 always
    picks, gains = R.greedy(seen, q, 10)
    assert picks == [2, 0, 1] and gains == [10, 6, 1]
    assert R.greedy(seen, q, 2) == ([2, 0], [10, 6])
    total = 17
    assert R.greedy(seen, q, 10, target_ratio=10 / total) == ([2], [10])           # reached exactly by the first pick
    assert R.greedy(seen, q, 10, target_ratio=11 / total) == ([2, 0], [10, 6])
    init = np.array([1, 1, 1, 1, 0, 0], bool)
    assert R.greedy(seen, q, 10, initial=init) == ([1], [1])
    assert R.greedy(seen, q, 10, initial=init, target_ratio=0.9) == ([], [])       # 16 / 17 already


def test_pack_round_trip():
    from lidarcast.coverage import pack_bits, unpack_bits
    rng = np.random.default_rng(1)
    for T in (1, 31, 32, 33, 100):
        s = rng.random(T) < 0.5
        w = pack_bits(s, T)
        assert w.dtype == np.uint32 and np.array_equal(w, R.pack(s)) and np.array_equal(unpack_bits(w, T), s)


# ---- planner selection argument (CPU: the robot-cube test is restated in numpy) ------------------------------------
def _blocked_numpy(self, pts, mesh):
    v = np.asarray(mesh.vertices)
    if len(pts) == 0 or len(v) == 0:
        return np.zeros(len(pts), dtype=bool)
    r = self.robot_radius
    return np.array([bool(np.any(np.all((v >= p - r) & (v <= p + r), axis=1))) for p in pts])


@pytest.fixture
def planner_cpu(monkeypatch):
    from trajectory import AutoTrajectoryGenerator
    monkeypatch.setattr(AutoTrajectoryGenerator, "_blocked", _blocked_numpy)
    from lidarcast import synth
    m = synth.make_room(size=(4.0, 3.0, 2.5), num_boxes=2, seed=3, cell=0.5)
    lo, hi = m.vertices.min(0), m.vertices.max(0)
    bounds = {"x_min": lo[0], "x_max": hi[0], "y_min": lo[1], "y_max": hi[1], "z_min": lo[2], "z_max": hi[2]}
    return AutoTrajectoryGenerator, m, bounds


def test_planner_rejects_unknown_selection(planner_cpu):
    cls, m, bounds = planner_cpu
    np.random.seed(4)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        cls(robot_radius=0.15).generate_optimal_trajectory(m, bounds, num_waypoints=10, selection="coverage")
    assert np.array_equal(np.random.get_state()[1], state)                # refused before any draw


def test_planner_reference_selection_is_the_default(planner_cpu):
    cls, m, bounds = planner_cpu
    outs = []
    for kw in ({}, {"selection": "reference"}):
        np.random.seed(11)
        wps, info = cls(robot_radius=0.15).generate_optimal_trajectory(m, bounds, num_waypoints=10, **kw)
        outs.append((np.array([[w.x, w.y, w.z, w.yaw] for w in wps]), repr(info), np.random.get_state()))
    (a, ia, sa), (b, ib, sb) = outs
    assert a.shape[0] > 0 and a.tobytes() == b.tobytes() and ia == ib and "surface_coverage" not in ia
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


# ---- compiled resources of the coverage kernels ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    d = tmp_path_factory.mktemp("cov_res")
    src = os.path.join(PKG, "csrc", "lrc_coverage.hip")
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", str(d / "c.o")], capture_output=True, text=True)
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
    a = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", str(d / "c.s")], capture_output=True,
                       text=True)
    assert a.returncode == 0, a.stderr[-4000:]
    return res, (d / "c.s").read_text()


KERNELS = ("area_kernel", "accumulate_kernel", "summary_kernel", "gain_kernel", "pick_kernel", "or_kernel")


def test_coverage_kernels_have_no_scratch_and_eight_waves(compiled):
    res, _ = compiled
    for k in KERNELS:
        names = [n for n in res if k in n]
        assert len(names) == 1, (k, list(res))
        u = res[names[0]]
        assert u["ScratchSize"] == 0, (k, u)
        assert u["Occupancy"] == 8, (k, u)          # measured sufficient: every kernel is memory- or atomic-bound
        assert u["VGPRs"] <= 32, (k, u)


def test_area_kernel_has_no_fused_area_arithmetic(compiled):
    """The cross product, the sum of squares and the products around the square root are separate v_mul_f64 /
    v_add_f64; the only f64 FMAs are the correctly rounded square-root expansion's residual steps (after v_rsq_f64)."""
    _, asm = compiled
    body = asm[asm.index("area_kernel"):]
    body = body[:body.index("s_endpgm")]
    ins = [ln.split()[0] for ln in body.splitlines() if ln.strip().startswith("v_")]
    assert "v_rsq_f64_e32" in ins or "v_rsq_f64" in ins
    first_rsq = next(i for i, x in enumerate(ins) if x.startswith("v_rsq_f64"))
    assert not any(x.startswith(("v_fma_f64", "v_fmac_f64")) for x in ins[:first_rsq])
    assert not any(x.startswith("v_sqrt_f64") for x in ins)         # the bare instruction is not correctly rounded
    assert any(x.startswith("v_rndne_f64") for x in ins)             # rint: round half to even
