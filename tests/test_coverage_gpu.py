"""-m gpu: surface coverage (csrc/lrc_coverage.hip) against the numpy restatement (tests/coverage_restate.py): the area
table bit for bit, accumulation of synthetic and real scans, analytic scenes, the greedy selection, and the opt-in
planner / simulator layers."""
import numpy as np
import pytest

import coverage_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import lidarcast
    return lidarcast.Context(0)


@pytest.fixture(scope="module")
def office():
    from lidarcast import synth
    return synth.make_scene("synth_A6_office2")


def _cov(ctx, mesh, S=1, sem=True):
    from lidarcast import SurfaceCoverage
    return SurfaceCoverage(ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem if sem else None, num_sets=S)


def _dirs_sphere(n=20000):
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    r = np.sqrt(1 - z * z)
    phi = i * np.pi * (3 - np.sqrt(5))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def _pose(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


# ---- area table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["synth_A6_office2", "synth_rough_A6"])
def test_area_table_bit_equal(ctx, name):
    from lidarcast import synth
    m = synth.make_scene(name)
    cov = _cov(ctx, m)
    q = R.area_q(m.vertices, m.triangles)
    got = cov.area_q()
    assert got.dtype == np.uint64 and np.array_equal(got, q), int((got != q).sum())
    assert cov.total_q == sum(int(x) for x in q)
    pc = R.per_class(np.ones(len(q), bool), q, m.triangle_sem)
    assert [int(s) for s in cov.class_ids] == sorted(pc)
    assert [int(x) for x in cov.class_total_q] == [pc[int(s)][1] for s in cov.class_ids]


def test_oversized_mesh_is_refused(ctx):
    from lidarcast import SurfaceCoverage
    with pytest.raises(ValueError):
        SurfaceCoverage(ctx, np.array([[0, 0, 0], [2e5, 0, 0], [0, 2e5, 0]], float), np.array([[0, 1, 2]], np.int32))
    v = np.array([[0, 0, 0], [4e4, 0, 0], [0, 4e4, 0]], np.float64)
    with pytest.raises(ValueError):
        SurfaceCoverage(ctx, v, np.array([[0, 1, 2]] * 3, np.int32))
    ok = SurfaceCoverage(ctx, v, np.array([[0, 1, 2]] * 2, np.int32))
    assert ok.total_q == 2 * int(R.area_q(v, [[0, 1, 2]])[0])
    with pytest.raises(ValueError):
        SurfaceCoverage(ctx, np.array([[0, 0, np.nan], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32))


# ---- accumulate on synthetic records -------------------------------------------------------------------------------
def _synthetic(seed, P, N, T):
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, T, P * N).astype(np.uint32)
    runs = rng.random(P * N) < 0.7                                   # long runs of equal prims
    for i in range(1, P * N):
        if runs[i]:
            prim[i] = prim[i - 1]
    t = rng.uniform(0.1, 5, P * N).astype(np.float32)
    t[rng.random(P * N) < 0.1] = np.inf                             # range-filtered: valid prim, t = inf
    miss = rng.random(P * N) < 0.1
    t[miss] = np.inf
    prim[miss] = R.INVALID
    prim[rng.random(P * N) < 0.01] = R.INVALID                       # invalid prim with a finite t: ignored
    return t, prim


def _dev(a, torch_dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").view(torch_dtype)


def test_accumulate_synthetic_equals_restatement(ctx):
    import torch
    from lidarcast import synth
    m = synth.make_room(size=(3, 3, 2.5), num_boxes=2, seed=5, cell=0.1)
    T = len(m.triangles)
    P, N, S = 9, 3000, 4
    t, prim = _synthetic(0, P, N, T)
    sop = np.array([3, 0, 0, 2, 3, 1, 0, 2, 3], np.int32)
    cov = _cov(ctx, m, S)
    cov.accumulate_dev(_dev(t, torch.float32), _dev(prim, torch.int32), P, N, _dev(sop, torch.int32))
    bits, hits, ret = cov.export()
    seen, h, r = R.accumulate(t, prim, P, N, S, T, set_of_pose=sop)
    assert np.array_equal(bits, R.pack(seen)) and np.array_equal(hits, h) and np.array_equal(ret, r)
    # the same rays over three calls, again: repeated calls add up
    cov2 = _cov(ctx, m, S)
    for a, b in ((0, 2), (2, 7), (7, 9)):
        cov2.accumulate_dev(_dev(t[a * N:b * N], torch.float32), _dev(prim[a * N:b * N], torch.int32), b - a, N,
                            _dev(sop[a:b], torch.int32))
    b2, h2, r2 = cov2.export()
    assert np.array_equal(b2, bits) and np.array_equal(h2, hits) and np.array_equal(r2, ret)
    cov2.accumulate_dev(_dev(t, torch.float32), _dev(prim, torch.int32), P, N, _dev(sop, torch.int32))
    b3, h3, r3 = cov2.export()
    assert np.array_equal(b3, bits) and np.array_equal(h3, 2 * hits) and np.array_equal(r3, 2 * ret)
    cov2.reset()
    b4, h4, r4 = cov2.export()
    assert not b4.any() and not h4.any() and not r4.any()
    # default map (pose p -> set p) and summaries of every set and of the union
    cov3 = _cov(ctx, m, P)
    cov3.accumulate_dev(_dev(t, torch.float32), _dev(prim, torch.int32), P, N)
    seen3, h3, r3 = R.accumulate(t, prim, P, N, P, T)
    q = R.area_q(m.vertices, m.triangles)
    for k in list(range(P)) + [None]:
        s = cov3.summary(k)
        mask = seen3.any(0) if k is None else seen3[k]
        assert np.array_equal(s.seen, mask) and s.seen_triangles == int(mask.sum())
        assert s.covered_q == R.covered_q(mask, q) and s.total_q == cov3.total_q
        assert s.returns == (int(r3.sum()) if k is None else int(r3[k]))
        assert {c: v for c, v in s.per_class_q.items()} == R.per_class(mask, q, m.triangle_sem)
        assert s.ratio == float(s.covered_q) / float(s.total_q) and s.redundancy == s.returns / (s.covered_q * 2.0 ** -32)
    assert np.array_equal(s.hits, h3)


# ---- analytic scenes ------------------------------------------------------------------------------------------------
def _scan_cover(ctx, mesh, poses, dirs, max_range, S=1):
    from lidarcast import Scene, scan_coverage
    scene = Scene(ctx, mesh.vertices, mesh.triangles)
    cov = _cov(ctx, mesh, S, sem=False)
    scan_coverage(scene, cov, poses, dirs, max_range, set_of_pose=np.zeros(len(poses), np.int64) if S == 1 else None)
    return scene, cov


def test_unit_cube_from_its_centre_is_fully_seen(ctx):
    from lidarcast import synth
    m = synth.unit_cube()
    _, cov = _scan_cover(ctx, m, _pose(0, 0, 0)[None], _dirs_sphere(), 10.0)
    s = cov.summary(0)
    assert s.seen.all() and s.covered_q == s.total_q and s.ratio == 1.0 and s.covered_area == 24.0
    assert s.returns == 20000 and s.hits.sum() == 20000


def test_box_occluder_hides_exactly_the_face_behind_it(ctx):
    from lidarcast import synth
    c = synth.unit_cube(-2.0, 2.0)
    v = np.concatenate([c.vertices, [[1, -2.5, -2.5], [1, 2.5, -2.5], [1, 2.5, 2.5], [1, -2.5, 2.5]]])
    f = np.concatenate([c.triangles, np.array([[8, 9, 10], [8, 10, 11]], np.int32)])
    m = synth.TriangleMesh(vertices=v, triangles=f.astype(np.int32))
    _, cov = _scan_cover(ctx, m, _pose(0, 0, 0)[None], _dirs_sphere(), 10.0)
    s = cov.summary(0)
    face = np.all(np.isclose(v[f][:, :, 0], 2.0), axis=1)            # the cube's +x face: behind the occluder
    assert face.sum() == 2
    assert np.array_equal(~s.seen, face)
    q = R.area_q(v, f)
    assert s.covered_q == R.covered_q(~face, q)


def test_wall_beyond_max_range_is_unseen_although_hit(ctx):
    from lidarcast import synth
    m = synth.unit_cube(-2.0, 2.0)
    pose = _pose(-1.5, 0, 0)[None]
    dirs = _dirs_sphere()
    scene, cov = _scan_cover(ctx, m, pose, dirs, 3.4)
    s = cov.summary(0)
    face = np.all(np.isclose(m.vertices[m.triangles][:, :, 0], 2.0), axis=1)
    assert np.array_equal(~s.seen, face)
    rec = scene.scan_poses(pose, dirs, 3.4, want=("t", "prim"))
    far = scene.scan_poses(pose, dirs, 10.0, want=("t", "prim"))
    hit_face = np.isin(far["prim"], np.flatnonzero(face))
    assert hit_face.any() and np.isinf(rec["t"][hit_face]).all()      # the rays hit the wall; the range filter drops them
    assert s.returns == int(np.isfinite(rec["t"]).sum())


# ---- a real trajectory ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim_run(office):
    from s3dis_simulator import S3DISSimulator
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    sim.load_scene(office, "synth_A6_office2")
    np.random.seed(3)
    wps, _ = sim.generate_auto_trajectory(num_waypoints=20)
    return sim, wps


def test_trajectory_coverage_equals_host_scan_restatement(sim_run, office):
    from trajectory import poses_from_waypoints
    sim, wps = sim_run
    eng = sim.raycast_engine
    poses = poses_from_waypoints(wps)
    s = eng.surface_coverage(sim.lidar_config, poses, office)
    rec, N = eng.scan_poses(sim.lidar_config, poses, office, want=("t", "prim"))
    T = len(office.triangles)
    seen, hits, ret = R.accumulate(rec["t"].reshape(-1), rec["prim"].reshape(-1), len(poses), N, 1, T,
                                   set_of_pose=np.zeros(len(poses)))
    assert np.array_equal(s.seen, seen[0])
    ok = np.isfinite(rec["t"].reshape(-1))
    assert np.array_equal(s.hits, np.bincount(rec["prim"].reshape(-1)[ok], minlength=T).astype(np.uint32))
    q = R.area_q(office.vertices, office.triangles)
    assert s.covered_q == R.covered_q(seen[0], q) and s.returns == int(ok.sum()) == int(ret[0])
    assert s.per_class_q == R.per_class(seen[0], q, office.triangle_sem)
    assert 0.0 < s.ratio < 1.0


def test_evaluate_surface_coverage_agrees_with_summary(sim_run, office):
    from lidarcast.synth import S3DIS_CLASSES
    from trajectory import poses_from_waypoints
    sim, wps = sim_run
    d = sim.evaluate_surface_coverage(wps)
    s = sim.raycast_engine.surface_coverage(sim.lidar_config, poses_from_waypoints(wps), office)
    assert d["covered_area_m2"] == s.covered_area and d["ratio"] == s.ratio and d["returns"] == s.returns
    assert d["redundancy_returns_per_m2"] == s.redundancy and d["num_poses"] == len(wps)
    assert set(d["per_class"]) == {S3DIS_CLASSES[c] for c in s.per_class}
    for c, (cm, tm, r) in s.per_class.items():
        assert d["per_class"][S3DIS_CLASSES[c]] == {"covered_m2": cm, "total_m2": tm, "ratio": r}
    import json
    json.dumps(d)


def test_sweeps_and_dual_axis_are_out_of_scope(sim_run, office):
    from lidar import DualAxisLidarIntrinsics
    sim, wps = sim_run
    with pytest.raises(NotImplementedError):
        sim.raycast_engine.surface_coverage(DualAxisLidarIntrinsics.create_blk2go_dual_axis(), np.eye(4)[None], office)
    sim.config["motion"] = {"speed": 0.5}
    try:
        with pytest.raises(NotImplementedError):
            sim.evaluate_surface_coverage(wps)
    finally:
        del sim.config["motion"]


# ---- greedy selection -------------------------------------------------------------------------------------------------
def test_greedy_selection_equals_restatement(sim_run, office):
    from lidarcast import Scene, SurfaceCoverage, scan_coverage
    sim, _ = sim_run
    eng = sim.raycast_engine
    Lx, Ly, _ = 5.0, 4.0, 3.0
    gx, gy = np.meshgrid(np.linspace(0.4, Lx - 0.4, 16), np.linspace(0.4, Ly - 0.4, 14))
    poses = np.stack([_pose(x, y, 1.0 + 0.3 * ((i % 3) - 1)) for i, (x, y) in enumerate(zip(gx.ravel(), gy.ravel()))])
    P = len(poses)
    assert P >= 200
    cov = eng.coverage_sets(sim.lidar_config, poses, office, chunk_poses=37)
    bits, _, _ = cov.export()
    q = R.area_q(office.vertices, office.triangles)
    T = len(q)
    seen = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :T].astype(bool)
    picks, gains_m2, cum = cov.select(P)
    rp, rg = R.greedy(seen, q, P)
    assert list(picks) == rp and np.array_equal(gains_m2, np.array(rg, float) * 2.0 ** -32)
    union = cov.summary(None)
    assert sum(rg) == union.covered_q and cum[-1] == union.ratio
    # target ratio: stops at the first pick that reaches it
    target = 0.9 * union.ratio
    p2, g2, c2 = cov.select(P, target_ratio=target)
    k = int(np.argmax([float(c) / float(cov.total_q) >= target for c in np.cumsum(np.array(rg, dtype=object))]))
    assert list(p2) == rp[:k + 1] and c2[-1] >= target and (len(c2) < 2 or c2[-2] < target)
    # budget, and an initial cover
    p3, _, _ = cov.select(5)
    assert list(p3) == rp[:5]
    p4, g4, _ = cov.select(P, initial=seen[rp[0]])
    r4p, r4g = R.greedy(seen, q, P, initial=seen[rp[0]])
    assert list(p4) == r4p and np.array_equal(g4, np.array(r4g, float) * 2.0 ** -32)
    # the engine's one-call form
    sp, sg, sc = eng.select_views(sim.lidar_config, poses, office, 8)
    assert list(sp) == rp[:8] and np.array_equal(sg, gains_m2[:8])


# ---- planner ------------------------------------------------------------------------------------------------------
def test_planner_surface_coverage_picks_the_restatement_winner(office):
    from lidar import Indoor8LineLidarIntrinsics
    from s3dis_simulator import S3DISSimulator
    from trajectory import poses_from_waypoints
    sim = S3DISSimulator({"raycast_engine": {"use_gpu": True}})
    sim.load_scene(office, "synth_A6_office2")
    gen = sim.auto_trajectory_generator
    b = sim._bounds_dict()
    np.random.seed(7)
    ref_wps, ref_info = gen.generate_optimal_trajectory(office, b, num_waypoints=20)
    ref_state = np.random.get_state()
    np.random.seed(7)
    wps, info = gen.generate_optimal_trajectory(office, b, num_waypoints=20, selection="surface_coverage")
    st = np.random.get_state()
    assert np.array_equal(ref_state[1], st[1]) and ref_state[2] == st[2]           # coverage adds no draws
    assert "surface_coverage" not in ref_info
    block = info["surface_coverage"]
    # restate: scan every candidate, rank by covered_q, ties to the reference score, then order
    np.random.seed(7)
    gen.room_analysis = gen._analyze_room_layout(office, b)
    cands = gen._generate_trajectory_candidates(max(int(20 * gen.interpolation_density), gen.min_waypoints))
    k = Indoor8LineLidarIntrinsics.create_standard_8line()
    q = R.area_q(office.vertices, office.triangles)
    cq = []
    for c in cands:
        rec, N = sim.raycast_engine.scan_poses(k, poses_from_waypoints(c.waypoints), office, want=("t", "prim"))
        seen, _, _ = R.accumulate(rec["t"].reshape(-1), rec["prim"].reshape(-1), len(c.waypoints), N, 1,
                                  len(q), set_of_pose=np.zeros(len(c.waypoints)))
        cq.append(R.covered_q(seen[0], q))
    scores = [gen._reference_score(c) for c in cands]
    win = min(range(len(cands)), key=lambda i: (-cq[i], -scores[i], i))
    assert block["winner_index"] == win
    assert block["candidate_ratios"] == [float(x) / float(sum(int(v) for v in q)) for x in cq]
    assert [(w.x, w.y, w.z, w.yaw) for w in wps] == [(w.x, w.y, w.z, w.yaw) for w in cands[win].waypoints]
    # the default planner output did not change: same bytes as a fresh default call
    np.random.seed(7)
    again, again_info = gen.generate_optimal_trajectory(office, b, num_waypoints=20)
    assert [(w.x, w.y, w.z, w.yaw) for w in again] == [(w.x, w.y, w.z, w.yaw) for w in ref_wps]
    assert repr(again_info) == repr(ref_info)
