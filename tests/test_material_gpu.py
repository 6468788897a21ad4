"""-m gpu: surface materials in the trace kernel (lrc_scan_materials_dev / lrc_scan_materials_compact, GEN = 7), on both node
routes: the quantised images where the scene has them, and the float32 nodes of a scene created under LRC_QNODES=0.

The comparator is the numpy restatement of the header's chain (tests/material_restate.py) over the EXISTING explicit-ray cast
(Scene.cast, no centre, no filter), segment by segment; the record is assembled on the host from (o_0, d_0, T, final surface)
with the range filter in float64.  Every column must agree bit for bit -- t, prim, normal3, point3, sem, ins, intensity, bounces,
surface_point3 -- except incident_deg, where the device's acos meets libm's on identical inputs: rtol 1e-13, as in
tests/test_echo_gpu.py.  The restatements are computed once per scene and shared; each case asserts on the restatement that it
exercises what it is for."""
import ctypes as C

import numpy as np
import pytest

import helpers
import material_restate as mr
from helpers import table_rays

pytestmark = pytest.mark.gpu

HITS = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg", "intensity")
EXTRA = ("bounces", "surface_point3")
CAST = ("t", "prim", "sem", "ins", "normal3", "point3", "intensity")
FRAMES = ("point3", "sem", "ins", "incident_deg", "index", "range_origin")
ROUTES = ("quantised", "float32")


def assert_bit_equal(a, b, what=""):
    """helpers.assert_bit_equal, and plain equality for the one-byte column (bounces)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.itemsize != 1:
        return helpers.assert_bit_equal(a, b, what)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ne = a != b
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.size} entries differ; first at {np.argwhere(ne)[0]}"


def _views(out):
    for k, dt in (("prim", np.uint32), ("sem", np.uint16), ("ins", np.uint16)):
        if k in out:
            out[k] = out[k].view(dt)
    return out


class Case:
    """One mesh on both node routes, with the restated chains of the three poses at width 100."""


@pytest.fixture(scope="module")
def engine():
    from raycast_engine import RaycastEngineGPU
    e = RaycastEngineGPU()
    yield e
    e.clear_cache()


def _case(engine, mesh, rec, max_bounces):
    import lidarcast
    c = Case()
    c.mesh, c.rec, c.max_bounces = mesh, rec, max_bounces
    mk = lambda: lidarcast.Scene(engine.ctx, mesh.vertices, mesh.triangles, mesh.triangle_sem, mesh.triangle_ins)
    c.scenes = {"quantised": mk()}
    with pytest.MonkeyPatch.context() as mp:          # the variable is read at every scene creation
        mp.setenv("LRC_QNODES", "0")
        c.scenes["float32"] = mk()
    assert c.scenes["float32"].info["quantised_nodes"] == 0
    c.k, c.dirs, c.poses = mr.scan_inputs(100)
    c.rays, cen = table_rays(c.dirs, c.poses)
    c.cen = np.repeat(cen, len(c.dirs), axis=0)
    c.cast = lambda rays: c.scenes["quantised"].cast(rays, center=None, max_range=np.inf, want=CAST)
    c.chain = mr.chain(c.cast, c.rays, rec, max_bounces)
    c.want = mr.assemble(c.chain, c.rays, c.cen, c.k.max_range)
    return c


@pytest.fixture(scope="module")
def pane(engine):
    c = _case(engine, mr.pane_scene()[0], mr.pane_records(), 4)
    yield c
    for s in c.scenes.values():
        s.close()


@pytest.fixture(scope="module")
def room(engine):
    c = _case(engine, mr.room_mesh(), mr.room_records(), 3)
    assert c.scenes["quantised"].info["quantised_nodes"] == 1          # a real tree on the quantised route
    yield c
    for s in c.scenes.values():
        s.close()


def table_of(rec, max_bounces, min_intensity=0.0):
    from lidarcast.material import MaterialTable
    return MaterialTable(rec, max_bounces=max_bounces, min_intensity=min_intensity)


def material_dev(scene, poses, dirs, table, max_range, want=HITS, surface=True):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    b = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    s = torch.full((P * N, 3), -1.0, dtype=torch.float32, device="cuda") if surface else None
    scene.scan_materials_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                             torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range, table, bounces_t=b, surface_t=s)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["bounces"] = b.cpu().numpy()
    if surface:
        out["surface_point3"] = s.cpu().numpy()
    return out


def clean_dev(scene, poses, dirs, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    scene.scan_poses_dev(torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda(),
                         torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), hits, max_range)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


def assert_records(got, want, what, clean=None):
    """Every column bit for bit; incident_deg bit for bit where the clean scan's own value applies (``clean``: rows whose record
    is the clean scan's), to rtol 1e-13 elsewhere."""
    for a in HITS + EXTRA:
        if a == "incident_deg":
            g, w = got[a], want[a]
            err = np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)
            print(f"\n[material] {what}: incident_deg of {len(g)} records, max relative difference {err.max() if len(g) else 0:.3g}")
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=0, err_msg=f"{what}: incident_deg")
        else:
            assert_bit_equal(got[a], want[a], f"{what}: {a}")


# ---- 1: every column against the restatement, both scenes, both routes --------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_pane_scene_equals_the_restatement(pane, route):
    """12.5 tiles per pose: tiles straddle poses and the last one is partial; one tile holds four different bounce counts."""
    hist = mr.bounce_histogram(pane.want, 4)
    print(f"\n[material] pane scene: returns after 0..4 bounces {hist.tolist()}, capped {int(pane.chain['capped'].sum())}")
    assert (hist > 0).all() and pane.chain["capped"].sum() > 0
    assert (pane.chain["ret"] & (pane.chain["sem"] == 5)).sum() > 0          # glass answers near normal incidence
    assert mr.tile_variety(pane.want, pane.chain) >= 3
    got = material_dev(pane.scenes[route], pane.poses, pane.dirs, table_of(pane.rec, 4), pane.k.max_range)
    assert_records(got, pane.want, f"pane scene, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_room_equals_the_restatement(room, route):
    hist = mr.bounce_histogram(room.want, 3)
    print(f"\n[material] room: returns after 0..3 bounces {hist.tolist()}, without a return {int((~room.want['keep']).sum())}")
    assert (hist > 0).all() and room.chain["capped"].sum() > 0
    assert (room.chain["ret"] & (room.chain["sem"] == 10)).sum() > 0
    assert mr.tile_variety(room.want, room.chain) >= 3
    got = material_dev(room.scenes[route], room.poses, room.dirs, table_of(room.rec, 3), room.k.max_range)
    assert_records(got, room.want, f"room, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_without_intensity_and_surface_points_the_other_columns_are_the_same(pane, room, route):
    """No output reads I or pp: a lane on a diffuse surface takes the short way (T += t alone), lanes on glass and mirrors the
    whole step.  Every other column is the restatement's, bit for bit."""
    cols = ("t", "prim", "normal3", "point3", "sem", "ins", "incident_deg")
    for c, name in ((pane, "pane scene"), (room, "room")):
        got = material_dev(c.scenes[route], c.poses, c.dirs, table_of(c.rec, c.max_bounces), c.k.max_range, want=cols, surface=False)
        for a in cols:
            if a == "incident_deg":
                np.testing.assert_allclose(got[a], c.want[a], rtol=1e-13, atol=0, err_msg=f"{name}, {route} nodes: incident_deg")
            else:
                assert_bit_equal(got[a], c.want[a], f"{name} without intensity, {route} nodes: {a}")
        assert_bit_equal(got["bounces"], c.want["bounces"], f"{name} without intensity, {route} nodes: bounces")
        only_t = material_dev(c.scenes[route], c.poses, c.dirs, table_of(c.rec, c.max_bounces), c.k.max_range, want=("t",), surface=False)
        assert_bit_equal(only_t["t"], c.want["t"], f"{name}, t alone, {route} nodes")


def test_range_filter_applies_to_the_point_on_the_original_beam(pane):
    """max_range 2.5 m: returns whose total path is longer are dropped although their surface may lie nearer."""
    want = mr.assemble(pane.chain, pane.rays, pane.cen, 2.5)
    dropped = pane.chain["ret"] & ~want["keep"]
    assert dropped.sum() > 100 and (pane.chain["b"][dropped] > 0).sum() > 20 and want["keep"].sum() > 100
    got = material_dev(pane.scenes["quantised"], pane.poses, pane.dirs, table_of(pane.rec, 4), 2.5)
    assert_records(got, want, "pane scene, max_range 2.5")
    assert (got["bounces"][dropped] == 0).all() and not got["surface_point3"][dropped].any()


# ---- 2, 3: the clean scan inside ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_all_diffuse_table_gives_the_clean_scan(room, route):
    from lidarcast.material import MaterialTable
    scene = room.scenes[route]
    clean = clean_dev(scene, room.poses, room.dirs, room.k.max_range)
    got = material_dev(scene, room.poses, room.dirs, MaterialTable.diffuse(12), room.k.max_range)
    assert (clean["t"] != np.inf).sum() > 2000
    for a in HITS:
        assert_bit_equal(got[a], clean[a], f"all-diffuse table, {route} nodes: {a}")
    assert not got["bounces"].any()
    assert_bit_equal(got["surface_point3"], clean["point3"], "all-diffuse table: the surface point is the record's point")
    one = material_dev(scene, room.poses, room.dirs, MaterialTable.diffuse(1), room.k.max_range)       # every id beyond the table
    for a in HITS:
        assert_bit_equal(one[a], clean[a], f"one-class table, {route} nodes: {a}")


@pytest.mark.parametrize("route", ROUTES)
def test_rays_that_end_on_their_first_diffuse_surface_carry_the_clean_record(pane, room, route):
    for c, name in ((pane, "pane scene"), (room, "room")):
        scene = c.scenes[route]
        clean = clean_dev(scene, c.poses, c.dirs, c.k.max_range)
        got = material_dev(scene, c.poses, c.dirs, table_of(c.rec, c.max_bounces), c.k.max_range)
        kind = mr.record_of(c.rec, got["sem"])[0]
        sel = (got["t"] != np.inf) & (got["bounces"] == 0) & (kind == mr.DIFFUSE)
        assert 1000 < sel.sum() < len(sel)
        for a in HITS:
            assert_bit_equal(got[a][sel], clean[a][sel], f"{name}, {route} nodes: {a} of rays without a bounce")
        assert_bit_equal(got["surface_point3"][sel], clean["point3"][sel], f"{name}: surface point of rays without a bounce")


# ---- 4: the split into calls ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_result_does_not_depend_on_the_split_into_calls(pane, route):
    scene, tab = pane.scenes[route], table_of(pane.rec, 4)
    whole = material_dev(scene, pane.poses, pane.dirs, tab, pane.k.max_range)
    a = material_dev(scene, pane.poses[:1], pane.dirs, tab, pane.k.max_range)
    b = material_dev(scene, pane.poses[1:], pane.dirs, tab, pane.k.max_range)
    for col in HITS + EXTRA:
        assert_bit_equal(np.concatenate([a[col], b[col]]), whole[col], f"1 + 2 poses against 3, {route} nodes: {col}")


# ---- 5, 6: the cap and the floor ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_max_bounces_zero_drops_every_ray_whose_first_surface_continues(pane, route):
    ch = mr.chain(pane.cast, pane.rays, pane.rec, 0)
    want = mr.assemble(ch, pane.rays, pane.cen, pane.k.max_range)
    first = pane.chain["first_continues"]
    assert first.sum() > 900 and (first == ch["capped"]).all() and not want["keep"][first].any()
    got = material_dev(pane.scenes[route], pane.poses, pane.dirs, table_of(pane.rec, 0), pane.k.max_range)
    assert (got["t"][first] == np.inf).all() and not got["bounces"].any()
    assert_records(got, want, f"max_bounces 0, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_min_intensity_drops_what_the_restatement_drops(pane, route):
    thr = float(np.float32(np.median(pane.chain["I"][pane.chain["ret"]])))
    ch = mr.chain(pane.cast, pane.rays, pane.rec, 4, min_intensity=thr)
    want = mr.assemble(ch, pane.rays, pane.cen, pane.k.max_range)
    dropped = pane.want["keep"] & ~want["keep"]
    assert 800 < dropped.sum() < 1600
    got = material_dev(pane.scenes[route], pane.poses, pane.dirs, table_of(pane.rec, 4, thr), pane.k.max_range)
    assert_records(got, want, f"min_intensity {thr:.4f}, {route} nodes")
    assert (got["t"][dropped] == np.inf).all()


# ---- 7: full tiles ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_width_96_full_tiles(pane, route):
    """8 x 96 = 768 rays per pose: 12 whole tiles, a pose ends on a tile boundary (width 100 above: it does not)."""
    k, dirs, poses = mr.scan_inputs(96)
    rays, cen = table_rays(dirs, poses)
    ch = mr.chain(pane.cast, rays, pane.rec, 4)
    want = mr.assemble(ch, rays, np.repeat(cen, len(dirs), axis=0), k.max_range)
    assert len(rays) % 64 == 0 and (mr.bounce_histogram(want, 4)[:4] > 0).all()
    got = material_dev(pane.scenes[route], poses, dirs, table_of(pane.rec, 4), k.max_range)
    assert_records(got, want, f"width 96, {route} nodes")


# ---- 8: frames, the engine, refusals, the simulator key ---------------------------------------------------------------------------

def host_frames(rec, P, N):
    """Host compaction of fixed-stride material records: what lrc_scan_materials_compact must return."""
    keep = (rec["t"] != np.inf).reshape(P, N)
    sel = keep.reshape(-1)
    pts = rec["point3"][sel]
    return {"counts": keep.sum(1), "point3": pts, "sem": rec["sem"][sel], "ins": rec["ins"][sel],
            "incident_deg": rec["incident_deg"][sel], "index": np.nonzero(keep)[1].astype(np.uint32),
            "range_origin": np.linalg.norm(pts, axis=1) if len(pts) else np.zeros(0, np.float32),
            "intensity": rec["intensity"][sel], "bounces": rec["bounces"][sel], "surface_point3": rec["surface_point3"][sel]}


def assert_frames_equal(fr, want, what):
    assert fr["counts"].tolist() == want["counts"].tolist(), what
    for k in ("point3", "sem", "ins", "incident_deg", "index", "range_origin", "intensity", "bounces", "surface_point3"):
        assert_bit_equal(fr[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("route", ROUTES)
def test_compact_frames(pane, room, route):
    for c, name in ((pane, "pane scene"), (room, "room")):
        scene, tab = c.scenes[route], table_of(c.rec, c.max_bounces)
        rec = material_dev(scene, c.poses, c.dirs, tab, c.k.max_range)
        want = host_frames(rec, len(c.poses), len(c.dirs))
        assert want["counts"].sum() > 1500 and (want["bounces"] > 0).sum() > 300
        fr = scene.scan_materials_compact(c.poses, c.dirs, c.k.max_range, tab, want=FRAMES)
        assert_frames_equal(fr, want, f"compact, {name}, {route} nodes")
        small = scene.scan_materials_compact(c.poses, c.dirs, c.k.max_range, tab, want=("point3",))      # no index column asked for
        assert "index" not in small
        for k in ("point3", "intensity", "bounces", "surface_point3"):
            assert_bit_equal(small[k], want[k], f"compact without index, {name}: {k}")
        with pytest.raises(ValueError, match="capacity"):
            scene.scan_materials_compact(c.poses, c.dirs, c.k.max_range, tab, want=FRAMES, capacity=10)


def test_engine_scan_material_frames(engine, room):
    tab = table_of(room.rec, 3)
    fr = engine.scan_material_frames(room.k, room.poses, room.mesh, tab, want=FRAMES)
    rec = material_dev(engine.scene_for(room.mesh), room.poses, room.dirs, tab, room.k.max_range)
    assert_frames_equal(fr, host_frames(rec, len(room.poses), len(room.dirs)), "engine")
    # the device records of the engine's own scene are the restatement's too
    assert_records(rec, room.want, "engine scene")


def test_refusals_on_a_scene(engine, pane):
    import torch
    import lidarcast
    from lidarcast import DeviceHits
    scene, tab = pane.scenes["quantised"], table_of(pane.rec, 4)
    P, N = len(pane.poses), len(pane.dirs)
    pt = torch.from_numpy(pane.poses.reshape(P, 16).copy()).cuda()
    dt = torch.from_numpy(pane.dirs).cuda()
    noise = torch.zeros(P * N, dtype=torch.float32, device="cuda")
    try:
        scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_materials_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, tab)
        with pytest.raises(ValueError, match="range_noise"):
            scene.scan_materials_compact(pane.poses, pane.dirs, 20.0, tab)
    finally:
        scene.reset_options()
    try:      # the angle between the original beam and the final surface's normal means nothing behind a mirror
        scene.set_options(incident_mode=1)
        with pytest.raises(ValueError, match="incident_mode 1"):
            scene.scan_materials_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, tab)
        with pytest.raises(ValueError, match="incident_mode 1"):
            scene.scan_materials_compact(pane.poses, pane.dirs, 20.0, tab)
    finally:
        scene.reset_options()
    # a table made resident on another context than the scene's (the library's own check, under the Python class)
    other = lidarcast.Context(0)
    try:
        from lidarcast import _capi
        lib, hits = _capi.load(), DeviceHits(P * N, "cuda", want=("t",))
        foreign = tab.resident(other)
        assert lib.lrc_scan_materials_dev(scene._h, pt.data_ptr(), P, dt.data_ptr(), N, foreign, 20.0, C.byref(hits.struct), None,
                                          None, None) == _capi.LRC_ERR_INVALID_ARG
        assert b"different contexts" in lib.lrc_last_error()
        table = lidarcast.DirectionTable(engine.ctx, pane.dirs)
        fr, total = _capi.LrcFrames(), C.c_uint64(0)
        counts = np.zeros(P, np.uint64)
        fr.counts = counts.ctypes.data
        assert lib.lrc_scan_materials_compact(scene._h, pane.poses.ctypes.data, P, table._h, foreign, 20.0, C.byref(fr), None, None,
                                              None, 0, C.byref(total)) == _capi.LRC_ERR_INVALID_ARG
        assert b"materials and scene belong to different contexts" in lib.lrc_last_error()
        table.close()
    finally:
        tab.close()
        other.close()
    # tensors of the wrong type, size or place would be written past their end
    good_hits = DeviceHits(P * N, "cuda", want=("t",))
    for kw, what in ((dict(surface_t=torch.zeros((P * N, 3), dtype=torch.float16, device="cuda")), "surface_t must be torch.float32"),
                     (dict(bounces_t=torch.zeros(P * N, dtype=torch.int32, device="cuda")), "bounces_t must be torch.uint8"),
                     (dict(bounces_t=torch.zeros(P * N, dtype=torch.uint8)), "bounces_t must lie on the device"),
                     (dict(surface_t=torch.zeros((3, P * N), dtype=torch.float32, device="cuda").t()), "surface_t must be contiguous")):
        with pytest.raises(ValueError, match=what):
            scene.scan_materials_dev(pt, dt, good_hits, 20.0, tab, **kw)
    with pytest.raises(ValueError, match="P \\* N records"):
        scene.scan_materials_dev(pt, dt, DeviceHits(P * N + 1, "cuda", want=("t",)), 20.0, tab)
    with pytest.raises(ValueError, match="bounces_t"):
        scene.scan_materials_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t",)), 20.0, tab,
                                 bounces_t=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    closed = lidarcast.DirectionTable(engine.ctx, pane.dirs)
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        scene.scan_materials_compact(pane.poses, closed, 20.0, tab)
    with pytest.raises(ValueError, match="direction table"):
        engine.scan_material_frames(object(), pane.poses, pane.mesh, tab)


def _sim(config, mesh, **kw):
    import s3dis_simulator
    sim = s3dis_simulator.S3DISSimulator(config, **kw)
    sim.load_scene(mesh, "room")
    return sim


def test_simulator_materials_key(engine, room, monkeypatch):
    from trajectory import line_trajectory, poses_from_waypoints
    wps = line_trajectory((1.0, 1.2, 1.0), (3.0, 1.8, 1.0), 4, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"max_bounces": 3, "min_intensity": 0.0,
           "classes": {"bookcase": {"kind": "glass", "pass": 0.9, "albedo": 0.1, "retro_deg": 5},
                       "table": {"kind": "mirror", "pass": 0.95, "albedo": 0.05, "retro_deg": 5}}}
    clean = _sim(dict(base), room.mesh).run_simulation(wps)
    sim = _sim(dict(base, materials=dict(key)), room.mesh)
    one = sim.run_simulation(wps)
    assert one.get_total_frames() == 4
    tab = sim._material_table()
    assert tab.records[10]["kind"] == 1 and tab.records[7]["kind"] == 2 and tab.max_bounces == 3
    fr = engine.scan_material_frames(sim.lidar_config, poses_from_waypoints(wps), room.mesh, tab,
                                     want=("point3", "sem", "ins", "incident_deg"))
    ends = np.cumsum(fr["counts"])
    bounced = 0
    for i, (a, c) in enumerate(zip(one.frames, clean.frames)):
        lo, hi = ends[i] - fr["counts"][i], ends[i]
        assert_bit_equal(a.points, fr["point3"][lo:hi], "frame points")
        assert_bit_equal(a.semantic_labels, fr["sem"][lo:hi], "labels come with the points")
        assert_bit_equal(a.instance_labels, fr["ins"][lo:hi])
        assert_bit_equal(a.intensities, fr["intensity"][lo:hi])
        assert_bit_equal(a.bounces, fr["bounces"][lo:hi])
        assert_bit_equal(a.surface_points, fr["surface_point3"][lo:hi])
        assert len(a.points) == len(a.intensities) == len(a.bounces) == len(a.surface_points) > 0
        assert (a.intensities >= 0).all() and (a.intensities <= 1).all() and a.bounces.max() <= 3
        # a ray without a bounce lies where it physically is; one with a bounce lies farther along the beam than its surface
        direct = a.bounces == 0
        assert_bit_equal(a.points[direct], a.surface_points[direct])
        bounced += int((~direct).sum())
        assert not hasattr(c, "bounces") and not hasattr(c, "intensities")                        # without the key nothing changes
    assert bounced >= 100
    # what the key does not cover raises instead of quietly scanning something else
    for other, cfg in (("motion", {"speed": 0.5}), ("noise", {"seed": 1}), ("beam", {"divergence_mrad": 3.0})):
        with pytest.raises(ValueError, match=f"materials key cannot be combined with the {other} key"):
            _sim(dict(base, materials=dict(key), **{other: cfg}), room.mesh).run_simulation(wps)
    with pytest.raises(ValueError, match="dual-axis"):
        _sim(dict(base, materials=dict(key)), room.mesh, use_blk2go=True).run_simulation(wps[:2])
    with pytest.raises(ValueError, match="unknown entries under the materials key"):
        _sim(dict(base, materials=dict(key, bounces=2)), room.mesh).run_simulation(wps)
    for export in (lambda: sim.evaluate_surface_coverage(wps), lambda: sim.export_occupancy_grid(wps, "unused"),
                   lambda: sim.export_frame_annotations(wps, "unused")):
        with pytest.raises(NotImplementedError, match="materials key"):
            export()
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(ValueError, match="multi-rank"):
        _sim(dict(base, materials=dict(key)), room.mesh).run_simulation(wps)
