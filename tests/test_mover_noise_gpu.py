"""-m gpu: seeded sensor noise under movers (lrc_scan_noisy_movers_dev / lrc_scan_noisy_movers_compact: the noisy ray kernel, the
explicit-ray launches under the live and keep bytes, the noisy merge kernel), on both node routes for the room and for the movers.

The comparator is tests/mover_noise_restate.py over the EXISTING explicit-ray cast (Scene.cast, no centre, no filter), as
tests/test_movers_gpu.py and tests/test_noise_gpu.py form theirs: the jittered rays, the keep mask and the range term of
tests/noise_restate.py, the kept rays cast on the room and -- taken into each mover's frame -- on the movers, the merge on the
clean ranges, t' = t + term, the record.  Every column must agree bit for bit -- t, prim, normal3, point3, sem, ins, intensity
and the mover column -- except incident_deg, where the device's acos meets libm's on identical inputs: rtol 1e-13.  Each case
asserts on the restatement that it exercises what it is for.  The inputs are those of tests/test_movers_gpu.py."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import mover_noise_restate as mnr
import mover_restate as mv
from test_movers_gpu import (FRAMES, HITS, ROUTES, _sim, _views, assert_bit_equal, assert_frames_equal,  # noqa: F401
                             assert_records, engine, host_frames, inputs, labelled, trio_poses, walker_poses, world)

pytestmark = pytest.mark.gpu

ALL = HITS + ("mover",)


def model_of(seed=7, first_frame=5, **kw):
    """The sensor record's model (the dense 32-line record: 0.01 m, 0.005 degrees, 5 % dropout)."""
    from lidar import Indoor8LineLidarIntrinsics
    from lidarcast.noise import NoiseModel
    m = NoiseModel.from_intrinsics(Indoor8LineLidarIntrinsics.create_dense_32line(), seed, first_frame)
    assert (m.range_std, m.dropout) == (0.01, 0.05) and np.isclose(np.rad2deg(m.angle_std), 0.005)
    return dataclasses.replace(m, **kw)


def zero_model(first_frame=5):
    from lidarcast.noise import NoiseModel
    return NoiseModel(seed=7, first_frame=first_frame)


@pytest.fixture(scope="module")
def tab():
    return mnr.table()


def _tensors(poses, dirs, mover_poses):
    import torch
    P = len(poses)
    mp = None if mover_poses is None else torch.from_numpy(np.ascontiguousarray(mover_poses, np.float32)).cuda()
    pt = torch.from_numpy(np.ascontiguousarray(poses).reshape(P, 16).copy()).cuda()
    return pt, torch.from_numpy(np.ascontiguousarray(dirs)).cuda(), mp


def noisy_movers_dev(scene, mset, poses, dirs, mover_poses, model, max_range, want=HITS, stream=None):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    pt, dt, mp = _tensors(poses, dirs, mover_poses)
    if stream is None:
        scene.scan_noisy_movers_dev(pt, dt, hits, max_range, mset, mp, model, mover_t=who)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            scene.scan_noisy_movers_dev(pt, dt, hits, max_range, mset, mp, model, mover_t=who, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["mover"] = who.cpu().numpy()
    return out


def movers_dev(scene, mset, poses, dirs, mover_poses, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    pt, dt, mp = _tensors(poses, dirs, mover_poses)
    scene.scan_movers_dev(pt, dt, hits, max_range, mset, mp, mover_t=who)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["mover"] = who.cpu().numpy()
    return out


def noisy_dev(scene, poses, dirs, model, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    P, N = len(poses), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    pt, dt, _ = _tensors(poses, dirs, None)
    scene.scan_noisy_dev(pt, dt, hits, max_range, model)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


_restated = {}


def restated(world, tab, width, which, model, max_range, **opts):
    """The restatement over Scene.cast, computed once per case and shared by the routes."""
    key = (width, which, model, max_range, tuple(sorted(opts.items())))
    if key not in _restated:
        k, dirs, poses, rays, cen = inputs(width)
        casts, mp = (world.casts[:1], walker_poses()) if which == "one" else (world.casts, trio_poses())
        _restated[key] = mnr.scan(world.static, casts, poses, dirs, mp, model, max_range, tab=tab, **opts)
    return _restated[key]


def sets_of(world, which, route):
    return (world.one[route], walker_poses()) if which == "one" else (world.sets[route], trio_poses())


# ---- 1: one pedestrian and the trio under the sensor record's model ---------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("which", ["one", "trio"])
@pytest.mark.parametrize("route", ROUTES)
def test_movers_under_the_sensor_records_model(world, tab, route, which, width):
    """Width 100: 600 rays per pose, waves straddle poses and the last is partial; width 128: 768 rays, whole waves, the
    scalar-cache pose path.  first_frame = 5.  A second model with an angle_std of 0.5 degrees moves rays from one surface to
    another."""
    k, dirs, poses, rays, cen = inputs(width)
    assert (len(dirs) % 64 == 0) == (width == 128)
    mset, mp = sets_of(world, which, route)
    _, cwin, _ = restated(world, tab, width, which, zero_model(), k.max_range)
    for name, model in (("sensor record", model_of()), ("jitter 0.5 degrees", model_of(angle_std=float(np.deg2rad(0.5))))):
        want, win, info = restated(world, tab, width, which, model, k.max_range)
        n_mover = int((want["mover"] != 0).sum())
        n_dropped_mover = int(((cwin["mover"] != 0) & ~info["keep"]).sum())
        n_moved = int((info["keep"] & (win["mover"] != cwin["mover"])).sum())
        print(f"\n[mover noise] {which}, width {width}, {name}: movers win {n_mover} rays, {int((~info['keep']).sum())} dropped "
              f"({n_dropped_mover} of them a mover's in the clean scan), {n_moved} kept rays change their winner")
        assert n_mover >= 10 and n_dropped_mover >= 1
        assert np.isinf(want["t"][~info["keep"]]).all() and not want["mover"][~info["keep"]].any()
        if name != "sensor record":
            assert n_moved >= 1
        got = noisy_movers_dev(world.scenes[route], mset, poses, dirs, mp, model, k.max_range)
        assert_records(got, want, f"{which}, width {width}, {name}, {route} nodes")


# ---- 2: a range draw as large as the room -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_large_range_noise_drops_returns_at_both_ends(world, tab, route):
    """range_std = 3 m, max_range = 4 m: returns with t' <= 0 and returns beyond max_range occur, on the room and on movers, and
    both have mover byte 0."""
    k, dirs, poses, rays, cen = inputs(100)
    model = model_of(range_std=3.0)
    want, win, info = restated(world, tab, 100, "trio", model, 4.0)
    with np.errstate(invalid="ignore"):
        tn = win["t"] + info["term"]
    hit = win["t"] < np.inf
    negative, far = hit & (tn <= 0), hit & (tn > 4.5)                  # (4.5: beyond the filter wherever the pose stands)
    print(f"\n[mover noise] range_std 3 m: {int(negative.sum())} returns at t' <= 0 ({int((negative & (win['mover'] != 0)).sum())} "
          f"of movers), {int(far.sum())} beyond max_range ({int((far & (win['mover'] != 0)).sum())} of movers)")
    assert negative.sum() >= 10 and far.sum() >= 10
    assert (negative & (win["mover"] != 0)).any() and (far & (win["mover"] != 0)).any()
    assert not want["mover"][negative | far].any() and np.isinf(want["t"][negative | far]).all()
    assert (want["mover"] != 0).sum() >= 10
    got = noisy_movers_dev(world.scenes[route], world.sets[route], poses, dirs, trio_poses(), model, 4.0)
    assert_records(got, want, f"range_std 3 m, {route} nodes")


# ---- 3: identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_all_zero_model_is_the_clean_mover_scan(world, route, width):
    k, dirs, poses, rays, cen = inputs(width)
    scene, mset, mp = world.scenes[route], world.sets[route], trio_poses()
    for max_range in (k.max_range, 1.6):
        clean = movers_dev(scene, mset, poses, dirs, mp, max_range)
        got = noisy_movers_dev(scene, mset, poses, dirs, mp, zero_model(), max_range)
        assert (clean["mover"] != 0).sum() >= 10
        for a in ALL:
            assert_bit_equal(got[a], clean[a], f"all-zero model, width {width}, {route} nodes, max_range {max_range}: {a}")


@pytest.mark.parametrize("width", [100, 128])
@pytest.mark.parametrize("route", ROUTES)
def test_null_set_is_the_noisy_scan(world, route, width):
    k, dirs, poses, rays, cen = inputs(width)
    scene, model = world.scenes[route], model_of(range_std=0.05)
    ref = noisy_dev(scene, poses, dirs, model, 3.0)
    got = noisy_movers_dev(scene, None, poses, dirs, None, model, 3.0)
    assert not got["mover"].any() and 100 < (ref["t"] < np.inf).sum() < 3 * len(dirs)
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"NULL set, width {width}, {route} nodes: {a}")


@pytest.mark.parametrize("route", ROUTES)
def test_a_copy_of_the_room_never_wins(world, tab, route):
    """Every kept ray meets the room and its copy at the same float32 range: the static scene keeps every tie, and the record --
    the range draw included -- is lrc_scan_noisy_dev's."""
    from lidarcast.movers import MoverSet
    import noise_restate as nr
    k, dirs, poses, rays, cen = inputs(100)
    model = model_of(angle_std=float(np.deg2rad(0.5)))
    ident = np.tile(mv.pose12(0.0, 0.0, 0.0, 0.0), (3, 1, 1))
    jittered, _, _, keep, _ = nr.noisy_rays(poses, dirs, model.seed, model.first_frame, model.range_std, model.angle_std,
                                            model.dropout, *tab)
    assert np.array_equal(mv.to_object(jittered[keep], ident[0, 0]), jittered[keep])      # the identity: the same rays
    with pytest.MonkeyPatch.context() as mp:
        if route == "float32":
            mp.setenv("LRC_QNODES", "0")
        copy = MoverSet(world.ctx, [labelled(world.room, 99, 9999)])
    try:
        ref = noisy_dev(world.scenes[route], poses, dirs, model, k.max_range)
        assert (ref["t"] < np.inf).sum() > 1500
        got = noisy_movers_dev(world.scenes[route], copy, poses, dirs, ident, model, k.max_range)
        assert not got["mover"].any() and 99 not in got["sem"]
        for a in HITS:
            assert_bit_equal(got[a], ref[a], f"copy of the room, {route} nodes: {a}")
    finally:
        copy.close()


# ---- 4: single-parameter models ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_single_parameter_models_change_only_their_part(world, tab, route):
    from lidarcast.noise import NoiseModel
    k, dirs, poses, rays, cen = inputs(100)
    scene, mset, mp = world.scenes[route], world.sets[route], trio_poses()
    clean = movers_dev(scene, mset, poses, dirs, mp, k.max_range)
    # dropout alone: the dropped rays' records become misses, every other record keeps its bytes
    model = NoiseModel(seed=7, dropout=0.05, first_frame=5)
    _, _, info = restated(world, tab, 100, "trio", model, k.max_range)
    keep = info["keep"]
    got = noisy_movers_dev(scene, mset, poses, dirs, mp, model, k.max_range)
    assert 30 < (~keep).sum() < 200 and ((clean["mover"] != 0) & ~keep).any()
    for a in ALL:
        assert_bit_equal(got[a][keep], clean[a][keep], f"dropout alone, kept rays: {a}")
    assert np.isinf(got["t"][~keep]).all() and (got["prim"][~keep] == mv.INVALID).all() and not got["mover"][~keep].any()
    assert not got["point3"][~keep].any() and not got["normal3"][~keep].any()
    # range alone: no prim, sem, ins, normal3 or mover of a kept row changes; the ranges do
    model = NoiseModel(seed=7, range_std=0.01, first_frame=5)
    got = noisy_movers_dev(scene, mset, poses, dirs, mp, model, k.max_range)
    kept = got["t"] < np.inf
    assert np.array_equal(kept, clean["t"] < np.inf)                   # 20 m of reach in a 5 m room, 1 cm of noise: nothing filtered
    for a in ("prim", "sem", "ins", "normal3", "mover"):
        assert_bit_equal(got[a][kept], clean[a][kept], f"range alone: {a}")
    assert (got["t"][kept] != clean["t"][kept]).mean() > 0.9 and (got["mover"] != 0).sum() >= 10
    assert np.abs(got["t"][kept] - clean["t"][kept]).max() < 0.01 * 5.5        # the table's clamp: |z| <= 5.42


# ---- 5: min_range with noise --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_min_range_does_not_uncover_a_mover(world, tab, route):
    """The case of tests/test_movers_gpu.py under the sensor record's model with dropout = 0: the pedestrian stands outside the
    room behind the wall x = 0; min_range 1.6 m removes the wall's near returns, and the pedestrian behind them stays hidden."""
    k, dirs, poses, rays, cen = inputs(100)
    model = model_of(dropout=0.0)
    outside = np.tile(mv.pose12(-0.6, 1.0, 0.0, 0.2), (3, 1, 1))
    want, win, info = mnr.scan(world.static, world.casts[:1], poses, dirs, outside, model, k.max_range, min_range=1.6, tab=tab)
    N = len(dirs)
    tm = world.casts[0](mv.to_object(info["rays"][:N], outside[0, 0]))["t"]
    ts = win["t"][:N]
    hidden = (ts < tm) & (tm < np.inf) & ~want["keep"][:N] & (tm > 1.6)          # the condition of the clean case, on the jittered rays
    print(f"\n[mover noise] min_range: {int(hidden.sum())} rays have a removed wall return in front of the pedestrian")
    assert hidden.sum() >= 5 and not want["mover"].any() and info["keep"].all()
    assert np.isinf(want["t"][:N][hidden]).all()
    scene = world.scenes[route]
    try:
        scene.set_options(min_range=1.6)
        got = noisy_movers_dev(scene, world.one[route], poses, dirs, outside, model, k.max_range)
    finally:
        scene.reset_options()
    assert_records(got, want, f"min_range, {route} nodes")


# ---- 6: chunking --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [100, 128])
def test_six_poses_equal_two_then_four(world, width):
    k, dirs, poses, rays, cen = inputs(width)
    poses6 = np.concatenate([poses, poses[::-1]])
    mp6 = np.concatenate([trio_poses(), trio_poses()[[1, 2, 0]]])
    scene, mset, model = world.scenes["quantised"], world.sets["quantised"], model_of()
    whole = noisy_movers_dev(scene, mset, poses6, dirs, mp6, model, k.max_range)
    a = noisy_movers_dev(scene, mset, poses6[:2], dirs, mp6[:2], model, k.max_range)
    b = noisy_movers_dev(scene, mset, poses6[2:], dirs, mp6[2:], model.at_frame(model.first_frame + 2), k.max_range)
    assert (np.bincount(whole["mover"], minlength=4) > 0).all()
    for col in ALL:
        assert_bit_equal(whole[col], np.concatenate([a[col], b[col]]), f"2 + 4 poses, width {width}: {col}")
    same = noisy_movers_dev(scene, mset, poses6[2:], dirs, mp6[2:], model, k.max_range)          # the wrong frame ids: other noise
    assert same["t"].tobytes() != b["t"].tobytes()


# ---- 7: the other entry points --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_compact_frames(world, route):
    k, dirs, poses, rays, cen = inputs(100)
    scene, mset, mp, model = world.scenes[route], world.sets[route], trio_poses(), model_of()
    rec = noisy_movers_dev(scene, mset, poses, dirs, mp, model, 3.0)
    want = host_frames(rec, 3, len(dirs))
    assert (np.bincount(want["mover"], minlength=4) > 0).all() and 0 < want["counts"].sum() < 3 * len(dirs)
    fr = scene.scan_noisy_movers_compact(poses, dirs, 3.0, mset, mp, model, want=FRAMES)
    assert_frames_equal(fr, want, f"compact, {route} nodes")
    small = scene.scan_noisy_movers_compact(poses, dirs, 3.0, mset, mp, model, want=("point3",))      # no index column asked for
    assert "index" not in small
    assert_bit_equal(small["point3"], want["point3"])
    assert_bit_equal(small["mover"], want["mover"])
    with pytest.raises(ValueError, match="capacity"):
        scene.scan_noisy_movers_compact(poses, dirs, 3.0, mset, mp, model, want=FRAMES, capacity=10)
    none = scene.scan_noisy_movers_compact(poses, dirs, 3.0, None, None, model, want=FRAMES)
    noisy = scene.scan_noisy_compact(poses, dirs, 3.0, model, want=FRAMES)
    assert none["counts"].tolist() == noisy["counts"].tolist() and not none["mover"].any() and len(none["mover"]) == noisy["total"]
    for a in FRAMES:
        assert_bit_equal(none[a], noisy[a], f"NULL set, compact: {a}")


def test_engine_scan_noisy_mover_frames(engine, world):
    from lidarcast.movers import MoverSet
    k, dirs, poses, rays, cen = inputs(100)
    mp, model = trio_poses(), model_of()
    mset = MoverSet(engine.ctx, world.meshes)
    try:
        fr = engine.scan_noisy_mover_frames(k, poses, world.room, mset, mp, model, want=FRAMES)
        rec = noisy_movers_dev(engine.scene_for(world.room), mset, poses, dirs, mp, model, k.max_range)
        assert_frames_equal(fr, host_frames(rec, 3, len(dirs)), "engine")
        assert (np.bincount(fr["mover"], minlength=4) > 0).all()
        again = engine.scan_noisy_mover_frames(k, poses[1:], world.room, mset, mp[1:], model.at_frame(model.first_frame + 1), want=FRAMES)
        off = int(fr["counts"][0])
        for a in FRAMES + ("mover",):
            assert_bit_equal(again[a], fr[a][off:], f"engine, frames 1 and 2 alone: {a}")
    finally:
        mset.close()
    with pytest.raises(ValueError, match="direction table"):
        engine.scan_noisy_mover_frames(object(), poses, world.room, None, None, model)


def test_non_default_stream(world):
    import torch
    k, dirs, poses, rays, cen = inputs(128)
    mp, model = trio_poses(), model_of()
    scene, mset = world.scenes["quantised"], world.sets["quantised"]
    ref = noisy_movers_dev(scene, mset, poses, dirs, mp, model, k.max_range)
    got = noisy_movers_dev(scene, mset, poses, dirs, mp, model, k.max_range, stream=torch.cuda.Stream())
    for col in ALL:
        assert_bit_equal(got[col], ref[col], f"own stream: {col}")


@pytest.mark.parametrize("route", ROUTES)
def test_incident_mode_1_uses_the_written_normal(world, tab, route):
    k, dirs, poses, rays, cen = inputs(100)
    model = model_of()
    want, _, _ = restated(world, tab, 100, "one", model, k.max_range, incident_mode=1)
    scene = world.scenes[route]
    try:
        scene.set_options(incident_mode=1)
        got = noisy_movers_dev(scene, world.one[route], poses, dirs, walker_poses(), model, k.max_range)
    finally:
        scene.reset_options()
    assert (want["mover"] == 1).sum() > 200
    assert_records(got, want, f"incident_mode 1, {route} nodes")


# ---- 8: deforming movers --------------------------------------------------------------------------------------------------------------

def test_deforming_movers_under_noise(engine):
    """The walker (keyframed) and the walker rig (skinned), three frames of three different shapes: scan_deforming_dev(...,
    noise=...) equals, per frame, scan_noisy_movers_dev on a fresh rigid MoverSet of that frame's vertices with first_frame + f;
    the skinned rig and the keyframe route of its host-skinned key poses equal each other."""
    import torch
    from lidar import IndoorLidar
    from lidarcast import DeviceHits, deform, skin, synth
    from lidarcast.movers import MoverSet
    from lidarcast.synth import TriangleMesh
    from skin_restate import rig
    from test_deform_gpu import scan_world
    room, walker, ped, k, poses, mp, shapes = scan_world()
    dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
    N, model = len(dirs), model_of()
    scene = engine.scene_for(room)
    g = rig("walker")
    rig_keys = skin.keyframes(g["rest"], g["idx"], g["wgt"], g["poses"])
    pt, dt, mt = _tensors(poses, dirs, mp)

    def deforming(d):
        mset = MoverSet(engine.ctx, [d, ped])
        try:
            hits = DeviceHits(3 * N, "cuda", want=HITS)
            who = torch.full((3 * N,), 255, dtype=torch.uint8, device="cuda")
            deform.scan_deforming_dev(scene, pt, dt, hits, k.max_range, mset, mt, shapes, mover_t=who, noise=model)
            torch.cuda.synchronize()
            out = _views({a: hits[a].cpu().numpy() for a in HITS})
            out["mover"] = who.cpu().numpy()
            frames = deform.scan_deforming_frames(engine, k, poses, room, mset, mp, shapes, want=FRAMES, noise=model)
            return out, frames
        finally:
            mset.close()

    def rigid_frames(keys, tris, sem, ins):
        parts = []
        for f in range(3):
            verts = deform.blend(keys[int(shapes[f, 0, 0])], keys[int(shapes[f, 0, 1])], shapes[f, 0, 2])
            body = TriangleMesh(vertices=verts.astype(np.float64), triangles=tris, triangle_sem=sem, triangle_ins=ins)
            ref_set = MoverSet(engine.ctx, [body, ped])
            try:
                parts.append(noisy_movers_dev(scene, ref_set, poses[f:f + 1], dirs, mp[f:f + 1], model.at_frame(model.first_frame + f),
                                              k.max_range))
            finally:
                ref_set.close()
        return {a: np.concatenate([p[a] for p in parts]) for a in ALL}

    results = {}
    made = [("keyframed walker", lambda: deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem,
                                                           walker.triangle_ins), walker.keyframes, walker),
            ("skinned rig", lambda: deform.SkinnedDeformable(engine.ctx, g["rest"], g["tris"], g["idx"], g["wgt"], g["poses"], g["sem"],
                                                             g["ins"]), rig_keys, None),
            ("keyframes of the rig", lambda: deform.Deformable(engine.ctx, rig_keys, g["tris"], g["sem"], g["ins"]), rig_keys, None)]
    for name, make, keys, mesh in made:
        d = make()
        try:
            got, frames = deforming(d)
        finally:
            d.close()
        results[name] = got
        tris, sem, ins = (mesh.triangles, mesh.triangle_sem, mesh.triangle_ins) if mesh is not None else (g["tris"], g["sem"], g["ins"])
        ref = rigid_frames(keys, tris, sem, ins)
        for a in ALL:
            assert_bit_equal(got[a], ref[a], f"{name}: {a}")
        assert_frames_equal(frames, host_frames(got, 3, N), f"{name}: scan_deforming_frames")
        per_frame = [got["point3"][f * N:(f + 1) * N][got["mover"][f * N:(f + 1) * N] == 1].tobytes() for f in range(3)]
        assert all((got["mover"][f * N:(f + 1) * N] == 1).sum() > 10 for f in range(3)) and len(set(per_frame)) == 3, name
        assert (got["mover"] == 2).any() and (got["mover"] == 0).any() and np.isinf(got["t"]).any()
    for a in ALL:
        assert_bit_equal(results["skinned rig"][a], results["keyframes of the rig"][a], f"skinned against keyframed: {a}")


# ---- 9: refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals(engine, world):
    import torch
    import lidarcast
    from lidarcast import DeviceHits, _capi
    from lidarcast.movers import MoverSet
    from lidarcast.noise import NoiseModel
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    k, dirs, poses, rays, cen = inputs(100)
    P, N = 3, len(dirs)
    scene, mset, mp, model = world.scenes["quantised"], world.one["quantised"], walker_poses(), model_of()
    pt, dt, mt = _tensors(poses, dirs, mp)
    before = scene.counters(), mset.scenes[0].counters()

    def hits_t():
        return DeviceHits(P * N, "cuda", want=("t",))

    # the model: what lrc_scan_noisy_dev refuses
    for bad, what in ((dict(range_std=-0.01), "range_std must be finite and not negative"), (dict(range_std=np.inf), "range_std"),
                      (dict(range_std=np.nan), "range_std"), (dict(angle_std=-1e-9), "angle_std must be finite and not negative"),
                      (dict(angle_std=np.nan), "angle_std"), (dict(dropout=1.0), r"dropout must lie in \[0, 1\)"),
                      (dict(dropout=-0.1), "dropout"), (dict(dropout=np.nan), "dropout")):
        m = dataclasses.replace(model, **bad)
        with pytest.raises(ValueError, match="lrc_scan_noisy_movers_dev: " + what):
            scene.scan_noisy_movers_dev(pt, dt, hits_t(), 20.0, mset, mt, m)
        with pytest.raises(ValueError, match="lrc_scan_noisy_movers_compact: " + what):
            scene.scan_noisy_movers_compact(poses, dirs, 20.0, mset, mp, m)
        with pytest.raises(ValueError, match="lrc_scan_noisy_movers_dev: " + what):            # without movers too
            scene.scan_noisy_movers_dev(pt, dt, hits_t(), 20.0, None, None, m)
    nz, hits = model.struct(), hits_t()
    assert lib.lrc_scan_noisy_movers_dev(scene._h, mset._h, pt.data_ptr(), P, dt.data_ptr(), N, mt.data_ptr(), 20.0, None,
                                         C.byref(hits.struct), None, None) == E
    assert b"noise is NULL" in lib.lrc_last_error()
    assert lib.lrc_scan_noisy_movers_dev(scene._h, mset._h, pt.data_ptr(), 1, dt.data_ptr(), 2 ** 32, mt.data_ptr(), 20.0, C.byref(nz),
                                         C.byref(hits.struct), None, None) == E
    assert b"2^32 - 1 rays per pose" in lib.lrc_last_error()
    noise = torch.zeros(P * N, dtype=torch.float32, device="cuda")
    try:
        scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match="lrc_scan_noisy_movers_dev: a range_noise option is set"):
            scene.scan_noisy_movers_dev(pt, dt, hits_t(), 20.0, mset, mt, model)
        with pytest.raises(ValueError, match="lrc_scan_noisy_movers_dev: a range_noise option is set"):
            scene.scan_noisy_movers_dev(pt, dt, hits_t(), 20.0, None, None, model)
        with pytest.raises(ValueError, match="lrc_scan_noisy_movers_compact: a range_noise option is set"):
            scene.scan_noisy_movers_compact(poses, dirs, 20.0, mset, mp, model)
    finally:
        scene.reset_options()
    # the movers: what lrc_scan_movers_dev refuses
    h = C.c_void_p()
    arr = (C.c_void_p * 1)(scene._h)
    assert lib.lrc_movers_create(engine.ctx._h, arr, 1, C.byref(h)) == 0
    try:
        assert lib.lrc_scan_noisy_movers_dev(scene._h, h, pt.data_ptr(), P, dt.data_ptr(), N, mt.data_ptr(), 20.0, C.byref(nz),
                                             C.byref(hits.struct), None, None) == E
        assert b"lrc_scan_noisy_movers_dev: the static scene is one of its own movers" in lib.lrc_last_error()
    finally:
        lib.lrc_movers_destroy(h)
    other = lidarcast.Context(0)
    try:
        foreign = MoverSet(other, world.meshes[:1])
        with pytest.raises(ValueError, match="another context"):
            scene.scan_noisy_movers_dev(pt, dt, hits_t(), 20.0, foreign, mt, model)
        assert lib.lrc_scan_noisy_movers_dev(scene._h, foreign._h, pt.data_ptr(), P, dt.data_ptr(), N, mt.data_ptr(), 20.0, C.byref(nz),
                                             C.byref(hits.struct), None, None) == E
        assert b"lrc_scan_noisy_movers_dev: movers and scene belong to different contexts" in lib.lrc_last_error()
        foreign.close()
    finally:
        other.close()
    with pytest.raises(ValueError, match="lrc_scan_noisy_movers_dev: tile_count"):
        scene.scan_noisy_movers_dev(pt, dt, DeviceHits(P * N, "cuda", want=("t", "tile_count")), 20.0, mset, mt, model)
    bad = mp.copy()
    bad[1, 0, 3] = np.nan
    with pytest.raises(ValueError, match="lrc_scan_noisy_movers_compact: mover pose 1 has an entry that is not finite"):
        scene.scan_noisy_movers_compact(poses, dirs, 20.0, mset, bad, model)
    bad = mp.copy()
    bad[2, 0, 0] += np.float32(2.0 ** -14)
    with pytest.raises(ValueError, match="lrc_scan_noisy_movers_compact: mover pose 2 is no rotation"):
        scene.scan_noisy_movers_compact(poses, dirs, 20.0, mset, bad, model)
    with pytest.raises(ValueError, match=r"\(P, M, 12\)"):
        scene.scan_noisy_movers_compact(poses, dirs, 20.0, mset, mp[:2], model)
    with pytest.raises(ValueError, match="P \\* N records"):
        scene.scan_noisy_movers_dev(pt, dt, DeviceHits(P * N + 1, "cuda", want=("t",)), 20.0, mset, mt, model)
    with pytest.raises(ValueError, match="mover_t must be torch.uint8"):
        scene.scan_noisy_movers_dev(pt, dt, hits_t(), 20.0, mset, mt, model, mover_t=torch.zeros(P * N, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert (scene.counters(), mset.scenes[0].counters()) == before                      # every refusal came before any launch
    assert scene.scan_noisy_movers_compact(poses, dirs, 20.0, mset, mp, NoiseModel(seed=1, dropout=0.999999))["total"] < 10


# ---- 10: the simulator end to end ---------------------------------------------------------------------------------------------------

def test_simulator_movers_noise_key(engine, world, tmp_path, monkeypatch):
    from lidarcast import deform, synth
    from lidarcast.movers import MoverSet
    from lidarcast.noise import NoiseModel
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 3, yaw=0.6)
    base = {"raycast_engine": {"use_gpu": True}}
    key = {"period": 0.1, "noise": {"seed": 7}, "objects": [
        {"mesh": "pedestrian", "semantic": 13, "instance": 1001, "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.2, 3.0, 1.6, 0.0, 120.0]]},
        {"mesh": "walker", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.3, 2.9, 0.0, 0.0]], "animation": {"cycle": 0.4}}]}
    sim = _sim(dict(base, movers=key), world.room)
    one = sim.run_simulation(wps)
    two = _sim(dict(base, movers=key), world.room).run_simulation(wps)
    clean = _sim(dict(base, movers={a: b for a, b in key.items() if a != "noise"}), world.room).run_simulation(wps)
    assert one.get_total_frames() == 3
    seen = np.zeros(3, np.int64)
    for a, b, c in zip(one.frames, two.frames, clean.frames):
        ids = a.mover_ids
        assert ids.dtype == np.uint8 and len(ids) == len(a.points) == len(a.semantic_labels) > 0
        seen += np.bincount(ids, minlength=3)
        assert (a.semantic_labels[ids == 1] == 13).all() and (a.instance_labels[ids == 1] == 1001).all()
        assert (a.semantic_labels[ids == 2] == 12).all() and (a.instance_labels[ids == 2] == 1002).all()
        assert a.points.tobytes() == b.points.tobytes() and ids.tobytes() == b.mover_ids.tobytes()        # two runs, the same bytes
        assert a.semantic_labels.tobytes() == b.semantic_labels.tobytes()
        assert 0.90 * len(c.points) < len(a.points) < 0.99 * len(c.points)                                 # 5 % dropout
    assert (seen > 0).all(), seen
    tracks = one.export_mover_tracks(tmp_path)
    disk = json.load(open(tmp_path / "room_mover_tracks.json"))
    assert disk == json.loads(json.dumps(tracks))
    k = sim.lidar_config
    assert disk["noise"] == {"seed": 7, "range_std": float(k.range_noise_std), "angle_std_deg": disk["noise"]["angle_std_deg"],
                             "dropout": float(k.dropout_probability), "first_frame": 0}
    assert np.isclose(disk["noise"]["angle_std_deg"], k.angle_noise_std)
    assert [f["returns"] for f in disk["frames"]] == [len(f.points) for f in one.frames]
    # frame 2 alone, rescanned through the engine with first_frame = 2
    plan = sim._mover_plan()
    model = NoiseModel.from_intrinsics(k, 7, first_frame=2)
    assert plan["noise"] == model.at_frame(0)
    from s3dis_simulator import poses_from_waypoints
    poses = poses_from_waypoints(wps)
    times = np.arange(3) * 0.1
    mover_poses = np.stack([t.poses12(times) for t in plan["tracks"]], axis=1)
    shapes = np.stack([plan["clips"][1].shapes3(times)], axis=1)
    walker = plan["meshes"][1]
    d = deform.Deformable(engine.ctx, plan["keyframes"][1], walker.triangles, walker.triangle_sem, walker.triangle_ins)
    mset = MoverSet(engine.ctx, [plan["meshes"][0], d])
    try:
        fr = deform.scan_deforming_frames(engine, k, poses[2:], world.room, mset, mover_poses[2:], shapes[2:],
                                          want=("point3", "sem", "ins"), noise=model)
    finally:
        mset.close()
        d.close()
    last = one.frames[2]
    assert_bit_equal(np.asarray(fr["point3"]), np.asarray(last.points, np.float32), "frame 2 alone: points")
    assert np.array_equal(fr["mover"], last.mover_ids) and np.array_equal(fr["sem"], last.semantic_labels)
    # what the key refuses
    for extra, what in ((dict(flow=True), "movers.flow is not available beside movers.noise"),
                        (dict(nonrigid_flow=True), "movers.nonrigid_flow is not available beside movers.noise")):
        with pytest.raises(ValueError, match=what):
            _sim(dict(base, movers=dict(key, **extra)), world.room).run_simulation(wps)
    with pytest.raises(ValueError, match="movers.noise key must be a mapping with a seed"):
        _sim(dict(base, movers=dict(key, noise=7)), world.room).run_simulation(wps)
    with pytest.raises(ValueError, match="movers key cannot be combined with the noise key"):
        _sim(dict(base, movers=key, noise={"seed": 1}), world.room).run_simulation(wps)
    with pytest.raises(ValueError, match="dual-axis"):
        _sim(dict(base, movers=key), world.room, use_blk2go=True).run_simulation(wps[:2])
    import lidarcast.distributed as ld
    monkeypatch.setattr(ld, "active_group", lambda group=None: (object(), group))
    with pytest.raises(ValueError, match="multi-rank"):
        sim.run_simulation(wps)
