"""-m gpu: seeded sensor noise under movers in sweeps (lrc_scan_noisy_mover_sweeps_dev / lrc_scan_noisy_mover_sweeps_compact: the
noisy sweep ray kernel, the explicit-ray launches under the live and keep bytes -- span_cast for a spanned deformable --, the noisy
sweep merge kernel), on both node routes for the room and for the movers.

The comparator is tests/mover_sweep_noise_restate.py over the EXISTING explicit-ray cast (Scene.cast, no centre, no filter): the
jittered swept rays, the keep mask and the range term of tests/noisy_sweep_restate.py, the kept rays cast on the room and -- taken
into each mover's frame at their own s -- on the movers, the merge on the clean ranges, t' = t + term, the record about c(s).
Every column must agree bit for bit -- t, prim, normal3, point3, sem, ins, intensity and the mover column -- except incident_deg,
where the device's acos meets libm's on identical inputs: rtol 1e-13, as in tests/test_mover_sweeps_gpu.py.  Each case asserts on
the restatement that it exercises what it is for; tests/test_mover_sweep_noise_host.py asserts the same over the CPU oracle.

Shapes are those of tests/test_mover_sweeps_gpu.py: N in {40, 64, 200} rays per sweep (64: a wave lies in one sweep and the
records come through the scalar cache), P in {1, 3} sweeps, M in {1, 3} movers; no P * N is a multiple of the block of 256.

The physical check of tests/test_mover_sweep_noise_host.py runs again on the GPU's output, with the bound measured there."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import mover_restate as mv
import mover_sweep_noise_restate as msn
import mover_sweep_restate as ms
import span_restate as sp
from test_mover_sweep_noise_host import BOUND_ON_BOX, SHAPES
from test_mover_sweeps_gpu import inputs, mover_records, sweeps_dev
from test_movers_gpu import (FRAMES, HITS, ROUTES, _views, assert_bit_equal, assert_frames_equal, assert_records, cast_of, engine,  # noqa: F401
                             host_frames, labelled, scene_of)

pytestmark = pytest.mark.gpu

ALL = HITS + ("mover",)


class World:
    """The room on both node routes, the three mover meshes, and per route a set of all three and one of the box."""


@pytest.fixture(scope="module")
def world(engine):
    from lidarcast.movers import MoverSet
    w = World()
    w.ctx = engine.ctx
    w.room = mv.room_mesh()
    w.meshes = msn.mover_meshes()
    w.scenes = {"quantised": scene_of(w.ctx, w.room)}
    w.sets = {"quantised": {3: MoverSet(w.ctx, w.meshes), 1: MoverSet(w.ctx, w.meshes[:1])}}
    with pytest.MonkeyPatch.context() as mp:              # the variable is read at every scene creation
        mp.setenv("LRC_QNODES", "0")
        w.scenes["float32"] = scene_of(w.ctx, w.room)
        w.sets["float32"] = {3: MoverSet(w.ctx, w.meshes), 1: MoverSet(w.ctx, w.meshes[:1])}
    assert w.scenes["quantised"].info["quantised_nodes"] == 1 and w.scenes["float32"].info["quantised_nodes"] == 0
    w.casts = [cast_of(s) for s in w.sets["quantised"][3].scenes]
    w.static = cast_of(w.scenes["quantised"])
    w.tab = msn.table()
    yield w
    for r in ROUTES:
        for s in w.sets[r].values():
            s.close()
        w.scenes[r].close()


def tensors(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def noisy_sweeps_dev(scene, mset, motion, dirs, fire, records, model, max_range, want=HITS, stream=None):
    import torch
    from lidarcast import DeviceHits
    from lidarcast.movers import scan_noisy_mover_sweeps_dev
    P, N = len(motion), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    mt, dt, ft, rt = tensors(motion, dirs, fire, None if records is None else np.asarray(records, np.float32))
    if stream is None:
        scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits, max_range, mset, rt, model, mover_t=who)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits, max_range, mset, rt, model, mover_t=who, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in want})
    out["mover"] = who.cpu().numpy()
    return out


def plain_noisy_sweeps_dev(scene, motion, dirs, fire, model, max_range, want=HITS):
    import torch
    from lidarcast import DeviceHits
    from lidarcast.noise import scan_noisy_sweeps_dev
    P, N = len(motion), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=want)
    mt, dt, ft = tensors(motion, dirs, fire)
    scan_noisy_sweeps_dev(scene, mt, dt, ft, hits, max_range, model)
    torch.cuda.synchronize()
    return _views({k: hits[k].cpu().numpy() for k in want})


_restated = {}


def restated(world, N, P, M, model, max_range, moving=True, **opts):
    """The restatement over Scene.cast, computed once per case and shared by the routes."""
    key = (N, P, M, model, max_range, moving, tuple(sorted(opts.items())))
    if key not in _restated:
        dirs, fire, _, motion, _, _ = inputs(N, P, moving)
        _restated[key] = msn.scan(world.static, world.casts[:M], motion, dirs, fire, mover_records(P, M, moving), model, max_range,
                                  tab=world.tab, **opts)
    return _restated[key]


# ---- 1: parity with the comparator ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("N,P,M", SHAPES)
def test_parity_under_the_sensor_records_model_and_under_jitter(world, N, P, M, route):
    """first_frame = 5.  The sensor record's model, and a second one with an angle_std of 0.5 degrees, which moves rays from one
    surface to another."""
    dirs, fire, _, motion, _, _ = inputs(N, P)
    rec = mover_records(P, M)
    assert (P * N) % 256 != 0 and (N % 64 == 0) == (N == 64)
    _, cwin, _ = restated(world, N, P, M, msn.zero_model(), 2.2)
    for name, model in (("sensor record", msn.model_of()), ("jitter 0.5 degrees", msn.model_of(angle_std=msn.JITTER))):
        want, win, info = restated(world, N, P, M, model, 2.2)
        per_sweep, dropped, moved = msn.conditions(want, win, info, cwin, N)
        filtered = int(((win["t"] < np.inf) & info["keep"] & ~want["keep"]).sum())
        print(f"\n[mover sweep noise] N {N}, P {P}, M {M}, {name}: movers win at least {per_sweep} rays per sweep, "
              f"{int((~info['keep']).sum())} dropped ({dropped} of them a mover's in the clean sweep), {moved} kept rays change their "
              f"winner, the filter removes {filtered}")
        assert per_sweep >= 1 and dropped >= 1 and filtered > 0
        assert np.isinf(want["t"][~info["keep"]]).all() and not want["mover"][~info["keep"]].any()
        if name != "sensor record" and N >= 64:
            assert moved >= 1
        got = noisy_sweeps_dev(world.scenes[route], world.sets[route][M], motion, dirs, fire, rec, model, 2.2)
        assert_records(got, want, f"N {N}, P {P}, M {M}, {name}, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_the_frame_id_carries_into_the_high_word(world, route):
    """first_frame = 2^32 - 1: sweep 0 has the last frame id of the low word, sweeps 1 and 2 carry into the high one."""
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    model = msn.model_of(first_frame=2 ** 32 - 1)
    want, _, info = restated(world, 200, 3, 3, model, 2.2)
    _, _, wrapped = restated(world, 200, 3, 3, model.at_frame(0), 2.2)
    assert not np.array_equal(info["keep"][200:], wrapped["keep"][:400])          # frames 2^32, 2^32 + 1 are not frames 0, 1
    assert (np.bincount(want["mover"], minlength=4) > 0).all()
    got = noisy_sweeps_dev(world.scenes[route], world.sets[route][3], motion, dirs, fire, mover_records(3, 3), model, 2.2)
    assert_records(got, want, f"first_frame 2^32 - 1, {route} nodes")


# ---- 2: a range draw as large as the room -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_large_range_noise_drops_returns_at_both_ends(world, route):
    """range_std = 3 m, max_range = 4 m: returns with t' <= 0 and returns beyond max_range occur on movers, and both have mover
    byte 0."""
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    model = msn.model_of(range_std=3.0)
    want, win, info = restated(world, 200, 3, 3, model, 4.0)
    with np.errstate(invalid="ignore"):
        tn = win["t"] + info["term"]
    hit = win["t"] < np.inf
    negative, far = hit & (tn <= 0), hit & (tn > 4.0)
    print(f"\n[mover sweep noise] range_std 3 m: {int(negative.sum())} returns at t' <= 0 ({int((negative & (win['mover'] != 0)).sum())} "
          f"of movers), {int(far.sum())} beyond max_range ({int((far & (win['mover'] != 0)).sum())} of movers)")
    assert (negative & (win["mover"] != 0)).sum() >= 10 and (far & (win["mover"] != 0)).sum() >= 10
    assert not want["mover"][negative | far].any() and np.isinf(want["t"][negative | far]).all()
    assert (want["mover"] != 0).sum() >= 10
    got = noisy_sweeps_dev(world.scenes[route], world.sets[route][3], motion, dirs, fire, mover_records(3, 3), model, 4.0)
    assert_records(got, want, f"range_std 3 m, {route} nodes")


# ---- 3: identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("route", ROUTES)
def test_all_zero_model_is_the_clean_mover_sweep_scan(world, route, N):
    dirs, fire, _, motion, _, _ = inputs(N, 3)
    rec = mover_records(3, 3)
    scene, mset = world.scenes[route], world.sets[route][3]
    for max_range in (2.2, 20.0):
        clean = sweeps_dev(scene, mset, motion, dirs, fire, rec, max_range)
        got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, msn.zero_model(), max_range)
        assert (clean["mover"] != 0).sum() >= 10
        for a in ALL:
            assert_bit_equal(got[a], clean[a], f"all-zero model, N {N}, {route} nodes, max_range {max_range}: {a}")


@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("route", ROUTES)
def test_a_null_set_is_the_noisy_sweep_scan(world, route, N):
    dirs, fire, _, motion, _, _ = inputs(N, 3)
    scene, model = world.scenes[route], msn.model_of(range_std=0.05)
    ref = plain_noisy_sweeps_dev(scene, motion, dirs, fire, model, 2.2)
    got = noisy_sweeps_dev(scene, None, motion, dirs, fire, None, model, 2.2)
    assert not got["mover"].any() and 40 < (ref["t"] < np.inf).sum() < 3 * N
    for a in HITS:
        assert_bit_equal(got[a], ref[a], f"NULL set, N {N}, {route} nodes: {a}")


@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("route", ROUTES)
def test_all_standing_still_is_the_noisy_mover_scan(world, route, N):
    """a sensor that does not move and movers with still records: the bytes of lrc_scan_noisy_movers_dev, for every firing fraction"""
    import torch
    from lidarcast import DeviceHits
    dirs, fire, start, motion, _, _ = inputs(N, 3, moving=False)
    rec = mover_records(3, 3, moving=False)
    assert all(ms.still(r) for r in rec.reshape(-1, 24))
    scene, mset, model = world.scenes[route], world.sets[route][3], msn.model_of(angle_std=msn.JITTER)
    hits = DeviceHits(3 * N, "cuda", want=HITS)
    who = torch.full((3 * N,), 255, dtype=torch.uint8, device="cuda")
    pt, dt, mp = tensors(start.reshape(3, 16).copy(), dirs, np.ascontiguousarray(rec[:, :, :12]))
    scene.scan_noisy_movers_dev(pt, dt, hits, 2.2, mset, mp, model, mover_t=who)
    torch.cuda.synchronize()
    frozen = _views({k: hits[k].cpu().numpy() for k in HITS})
    frozen["mover"] = who.cpu().numpy()
    got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 2.2)
    assert (np.bincount(frozen["mover"], minlength=4) > 0).all() and np.isinf(frozen["t"]).any()
    for a in ALL:
        assert_bit_equal(got[a], frozen[a], f"all still, N {N}, {route} nodes: {a}")


@pytest.mark.parametrize("route", ROUTES)
def test_a_copy_of_the_room_never_wins(world, route):
    """the room's copy at the identity with a still record meets every kept ray at the room's own float32 range: the room keeps the
    tie, and the record -- the range draw included -- is lrc_scan_noisy_sweeps_dev's"""
    from lidarcast.movers import MoverSet
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    model = msn.model_of(angle_std=msn.JITTER)
    rec = np.tile(ms.still_record(mv.pose12(0.0, 0.0, 0.0, 0.0)), (3, 1, 1))
    with pytest.MonkeyPatch.context() as mp:
        if route == "float32":
            mp.setenv("LRC_QNODES", "0")
        copy = MoverSet(world.ctx, [labelled(world.room, 99, 9999)])
    try:
        ref = plain_noisy_sweeps_dev(world.scenes[route], motion, dirs, fire, model, 20.0)
        got = noisy_sweeps_dev(world.scenes[route], copy, motion, dirs, fire, rec, model, 20.0)
        assert not got["mover"].any() and 99 not in got["sem"] and (ref["t"] < np.inf).sum() > 500
        for a in HITS:
            assert_bit_equal(got[a], ref[a], f"copy of the room, {route} nodes: {a}")
    finally:
        copy.close()


@pytest.mark.parametrize("N", [64, 200])
def test_six_sweeps_equal_two_then_four(world, N):
    dirs, fire, _, motion, _, _ = inputs(N, 3)
    motion6 = np.concatenate([motion, motion[::-1]])
    rec6 = np.concatenate([mover_records(3, 3), mover_records(3, 3)[[1, 2, 0]]])
    scene, mset, model = world.scenes["quantised"], world.sets["quantised"][3], msn.model_of()
    whole = noisy_sweeps_dev(scene, mset, motion6, dirs, fire, rec6, model, 2.2)
    a = noisy_sweeps_dev(scene, mset, motion6[:2], dirs, fire, rec6[:2], model, 2.2)
    b = noisy_sweeps_dev(scene, mset, motion6[2:], dirs, fire, rec6[2:], model.at_frame(model.first_frame + 2), 2.2)
    assert (np.bincount(whole["mover"], minlength=4) > 0).all()
    for col in ALL:
        assert_bit_equal(whole[col], np.concatenate([a[col], b[col]]), f"2 + 4 sweeps, N {N}: {col}")
    same = noisy_sweeps_dev(scene, mset, motion6[2:], dirs, fire, rec6[2:], model, 2.2)          # the wrong frame ids: other noise
    assert same["t"].tobytes() != b["t"].tobytes()


# ---- 4: single-parameter models, min_range, incident_mode, a stream -----------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_single_parameter_models_change_only_their_part(world, route):
    from lidarcast.noise import NoiseModel
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    rec = mover_records(3, 3)
    scene, mset = world.scenes[route], world.sets[route][3]
    clean = sweeps_dev(scene, mset, motion, dirs, fire, rec, 20.0)
    # dropout alone: the dropped rays' records become misses, every other record keeps its bytes
    model = NoiseModel(seed=msn.SEED, dropout=0.05, first_frame=5)
    _, _, info = restated(world, 200, 3, 3, model, 20.0)
    keep = info["keep"]
    got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 20.0)
    assert 10 < (~keep).sum() < 80 and ((clean["mover"] != 0) & ~keep).any()
    for a in ALL:
        assert_bit_equal(got[a][keep], clean[a][keep], f"dropout alone, kept rays: {a}")
    assert np.isinf(got["t"][~keep]).all() and (got["prim"][~keep] == mv.INVALID).all() and not got["mover"][~keep].any()
    assert not got["point3"][~keep].any() and not got["normal3"][~keep].any()
    # range alone: no prim, sem, ins, normal3 or mover of a kept row changes; the ranges do
    model = NoiseModel(seed=msn.SEED, range_std=0.01, first_frame=5)
    got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 20.0)
    kept = got["t"] < np.inf
    assert np.array_equal(kept, clean["t"] < np.inf)                   # 20 m of reach in a 5 m room, 1 cm of noise: nothing filtered
    for a in ("prim", "sem", "ins", "normal3", "mover"):
        assert_bit_equal(got[a][kept], clean[a][kept], f"range alone: {a}")
    assert (got["t"][kept] != clean["t"][kept]).mean() > 0.9 and (got["mover"] != 0).sum() >= 10
    assert np.abs(got["t"][kept] - clean["t"][kept]).max() < 0.01 * 5.5        # the table's clamp: |z| <= 5.42
    # jitter alone: the kept mask is full, and the rays are not the clean sweep's
    model = NoiseModel(seed=msn.SEED, angle_std=msn.JITTER, first_frame=5)
    want, _, info = restated(world, 200, 3, 3, model, 20.0)
    got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 20.0)
    assert info["keep"].all() and not info["term"].any() and got["point3"].tobytes() != clean["point3"].tobytes()
    assert_records(got, want, f"jitter alone, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_min_range_acts_on_the_noisy_range(world, route):
    """The case of tests/test_mover_sweeps_gpu.py under the sensor record's model with a range_std of 0.1 m: min_range 1.4 m
    removes the near returns of the box that crosses in front of the sensor, the room behind them stays hidden, and returns
    change sides of min_range with their range draw."""
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    model = msn.model_of(range_std=0.1)
    want, win, info = restated(world, 200, 3, 1, model, 20.0, min_range=1.4)
    plain, _, _ = restated(world, 200, 3, 1, model, 20.0)
    removed = (win["mover"] == 1) & info["keep"] & ~want["keep"]
    clean, _, _ = restated(world, 200, 3, 1, dataclasses.replace(model, range_std=0.0), 20.0, min_range=1.4)
    flipped = info["keep"] & (plain["t"] < np.inf) & (clean["keep"] != want["keep"])
    print(f"\n[mover sweep noise] min_range: {int(removed.sum())} near returns of the box are removed; the range draw takes "
          f"{int(flipped.sum())} returns across min_range")
    assert removed.sum() >= 20 and np.isinf(want["t"][removed]).all() and not want["mover"][removed].any()
    assert flipped.sum() >= 1
    assert (want["keep"] & (want["mover"] == 0)).sum() > 100
    scene = world.scenes[route]
    try:
        scene.set_options(min_range=1.4)
        got = noisy_sweeps_dev(scene, world.sets[route][1], motion, dirs, fire, mover_records(3, 1), model, 20.0)
    finally:
        scene.reset_options()
    assert_records(got, want, f"min_range, {route} nodes")


@pytest.mark.parametrize("route", ROUTES)
def test_incident_mode_1_uses_the_turned_normal(world, route):
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    model = msn.model_of()
    want, _, _ = restated(world, 200, 3, 3, model, 20.0, incident_mode=1)
    scene = world.scenes[route]
    try:
        scene.set_options(incident_mode=1)
        got = noisy_sweeps_dev(scene, world.sets[route][3], motion, dirs, fire, mover_records(3, 3), model, 20.0)
    finally:
        scene.reset_options()
    assert (want["mover"] > 0).sum() > 100
    assert_records(got, want, f"incident_mode 1, {route} nodes")


def test_non_default_stream(world):
    import torch
    dirs, fire, _, motion, _, _ = inputs(64, 3)
    rec, model = mover_records(3, 3), msn.model_of()
    scene, mset = world.scenes["quantised"], world.sets["quantised"][3]
    ref = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 2.2)
    got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 2.2, stream=torch.cuda.Stream())
    for col in ALL:
        assert_bit_equal(got[col], ref[col], f"own stream: {col}")


def test_one_set_serves_the_four_variants_in_turn(world):
    """The four dev scans share one scratch per set, laid out per variant (74 bytes per ray, + 24 with stored world rays, + 1 with
    live bytes).  On ONE set and stream, in the order clean (74), noisy sweep (99: the block grows), sweep (98) and noisy (99: both
    in a block an eighth larger than the noisy sweep needed), every record column and the mover column is byte-equal to the same scan on a set
    created for it alone.  (N, P, M) = (200, 2, 3), then (64, 5, 1): a set has its M for life, so each shape has its own used set."""
    from lidarcast.movers import MoverSet
    from test_mover_noise_gpu import movers_dev, noisy_movers_dev
    scene, model = world.scenes["quantised"], msn.model_of(dropout=0.25)
    assert model.range_std > 0 and model.dropout == 0.25
    for N, P, M in ((200, 2, 3), (64, 5, 1)):
        dirs, fire, start, motion, _, _ = inputs(N, min(P, 3))
        start, motion = np.concatenate([start, start[::-1]])[:P], np.concatenate([motion, motion[::-1]])[:P]
        rec = mover_records(P, M)
        mp = np.ascontiguousarray(rec[:, :, :12])
        scans = [("clean", lambda s: movers_dev(scene, s, start, dirs, mp, 2.2)),
                 ("noisy sweep", lambda s: noisy_sweeps_dev(scene, s, motion, dirs, fire, rec, model, 2.2)),
                 ("sweep", lambda s: sweeps_dev(scene, s, motion, dirs, fire, rec, 2.2)),
                 ("noisy", lambda s: noisy_movers_dev(scene, s, start, dirs, mp, model, 2.2))]
        used = MoverSet(world.ctx, world.meshes[:M])
        try:
            got = [scan(used) for _, scan in scans]
        finally:
            used.close()
        for (name, scan), g in zip(scans, got):
            fresh = MoverSet(world.ctx, world.meshes[:M])
            try:
                want = scan(fresh)
            finally:
                fresh.close()
            assert (want["mover"] != 0).any() and np.isinf(want["t"]).any()
            for col in ALL:
                assert_bit_equal(g[col], want[col], f"{name} on a used set, (N, P, M) = ({N}, {P}, {M}): {col}")


# ---- 5: the compact call and the frames ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_compact_call_is_the_dev_call(world, route):
    from lidarcast.movers import scan_noisy_mover_sweeps_compact
    from lidarcast.noise import scan_noisy_sweeps_compact
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    rec, model = mover_records(3, 3), msn.model_of()
    scene, mset = world.scenes[route], world.sets[route][3]
    dev = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, 2.2)
    want = host_frames(dev, 3, 200)
    assert (np.bincount(want["mover"], minlength=4) > 0).all() and 0 < want["counts"].sum() < 600
    fr = scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 2.2, mset, rec, model, want=FRAMES)
    assert_frames_equal(fr, want, f"compact, {route} nodes")
    small = scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 2.2, mset, rec, model, want=("point3",))      # no index column asked for
    assert "index" not in small
    assert_bit_equal(small["point3"], want["point3"])
    assert_bit_equal(small["mover"], want["mover"])
    with pytest.raises(ValueError, match="capacity"):
        scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 2.2, mset, rec, model, want=FRAMES, capacity=10)
    none = scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 2.2, None, None, model, want=FRAMES)
    noisy = scan_noisy_sweeps_compact(scene, motion, dirs, fire, 2.2, model, want=FRAMES)
    assert none["counts"].tolist() == noisy["counts"].tolist() and not none["mover"].any() and len(none["mover"]) == noisy["total"]
    for a in FRAMES:
        assert_bit_equal(none[a], noisy[a], f"NULL set, compact: {a}")


def test_engine_frames_are_the_dev_call(engine, world):
    """the engine's sensor: point_times, mover and the labels have one entry per kept row and belong together; a run of sweeps
    scanned again with its own first frame gives its bytes"""
    from helpers import aimed_pose, sensor_small
    from lidar import IndoorLidar
    from lidarcast.movers import MoverSet, scan_noisy_mover_sweep_frames
    from test_mover_sweeps_gpu import TARGET
    k = sensor_small(lines=4, width=64, max_range=6.0)
    start = np.stack([aimed_pose(TARGET, 1.5, yaw=y) for y in (0.3, -1.0)])
    end = start.copy()
    end[:, :3, 3] += (0.08, -0.09, 0.02)
    rec, model = mover_records(2, 3), msn.model_of()
    mset = MoverSet(engine.ctx, world.meshes)
    try:
        fr = scan_noisy_mover_sweep_frames(engine, k, start, end, world.room, mset, rec, model, want=("point3", "sem", "ins", "index"))
        motion, fire, T = engine.sweep_inputs(k, start, end)
        dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
        dev = noisy_sweeps_dev(engine.scene_for(world.room), mset, motion, dirs, fire, rec, model, k.max_range)
        again = scan_noisy_mover_sweep_frames(engine, k, start[1:], end[1:], world.room, mset, rec[1:], model.at_frame(model.first_frame + 1),
                                              want=("point3", "sem", "ins", "index"))
    finally:
        mset.close()
    keep = dev["t"] != np.inf
    K = int(keep.sum())
    assert fr["total"] == K == len(fr["point_times"]) == len(fr["mover"]) == len(fr["sem"]) == len(fr["ins"]) == len(fr["point3"])
    assert 0 < K < 0.97 * len(keep)                                        # 5 % dropout
    assert_bit_equal(fr["point3"], dev["point3"][keep], "frames: point3")
    assert_bit_equal(fr["mover"], dev["mover"][keep], "frames: mover")
    assert_bit_equal(fr["ins"], dev["ins"][keep], "frames: ins")
    assert np.array_equal(fr["point_times"], fire[fr["index"]] * T) and T == 1.0 / k.scan_frequency
    assert (fr["ins"][fr["mover"] == 1] == 77).all() and (fr["ins"][fr["mover"] == 2] == 1001).all()
    assert (fr["ins"][fr["mover"] == 3] == 1002).all() and (np.bincount(fr["mover"], minlength=4) > 0).all()
    off = int(fr["counts"][0])
    for a in ("point3", "sem", "ins", "index", "mover", "point_times"):
        assert_bit_equal(again[a], fr[a][off:], f"sweep 1 alone: {a}")
    with pytest.raises(NotImplementedError, match="direction table"):
        scan_noisy_mover_sweep_frames(engine, object(), start, end, world.room, None, None, model)


# ---- 6: spanned deformables -----------------------------------------------------------------------------------------------------------

def span_sweeps_dev(scene, mset, motion, dirs, fire, rec, sa, sb, max_range, noise):
    import torch
    from lidarcast import DeviceHits, deform
    P, N = len(motion), len(dirs)
    hits = DeviceHits(P * N, "cuda", want=HITS)
    who = torch.full((P * N,), 255, dtype=torch.uint8, device="cuda")
    mt, dt, ft, rt = tensors(motion, dirs, fire, np.asarray(rec, np.float32))
    deform.scan_deforming_sweeps_dev(scene, mt, dt, ft, hits, max_range, mset, rt, sa, sb, mover_t=who, noise=noise)
    torch.cuda.synchronize()
    out = _views({k: hits[k].cpu().numpy() for k in HITS})
    out["mover"] = who.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def spanned(engine):
    """the walker (keyframes), the walker rig (skinned) and the one-triangle deformable of tests/test_span_gpu.py, each alone in a set"""
    from lidarcast import deform, skin, synth
    from lidarcast.movers import MoverSet
    from test_span_host import RIG_PHASE, triangle_keyframes
    walker = synth.make_walker(semantic=13, instance=1001)
    rig = synth.make_walker_rig(semantic=13, instance=1003, smooth=0.1)
    rig_keys = skin.keyframes(rig.vertices, rig.bone_index, rig.bone_weight, rig.poses12)
    tri_keys, tri_f = triangle_keyframes()
    tri = synth.TriangleMesh(vertices=tri_keys[0].astype(np.float64), triangles=tri_f, triangle_sem=np.array([7], np.uint16),
                             triangle_ins=np.array([31], np.uint16))
    ds = {"walker": deform.Deformable(engine.ctx, walker.keyframes, walker.triangles, walker.triangle_sem, walker.triangle_ins),
          "rig": deform.SkinnedDeformable(engine.ctx, rig.vertices, rig.triangles, rig.bone_index, rig.bone_weight, rig.poses12,
                                          rig.triangle_sem, rig.triangle_ins),
          "triangle": deform.Deformable(engine.ctx, tri_keys, tri_f, tri.triangle_sem, tri.triangle_ins)}
    out = {"walker": (walker, walker.keyframes, 0.0), "rig": (rig, rig_keys, RIG_PHASE), "triangle": (tri, tri_keys, 0.0)}
    sets = {name: MoverSet(engine.ctx, [d]) for name, d in ds.items()}
    yield {name: out[name] + (sets[name], ds[name]) for name in out}
    for s in sets.values():
        s.close()
    for d in ds.values():
        d.close()


@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("name", ["walker", "rig", "triangle"])
def test_spanned_deformables_under_noise(world, spanned, name, N):
    """scan_deforming_sweeps_dev(..., noise=...): sweep p has the noise of frame first_frame + p; the comparator casts the kept
    rays of an animated mover per firing fraction on a FRESH scene of span_vertices(VA, VB, s) (span_restate.fraction_cast).  The
    three sweeps have three different (A, B): three runs, each with its own first frame.  noise=None gives the bytes of a span and
    lrc_scan_mover_sweeps_dev per sweep."""
    import torch
    from test_span_gpu import fresh_cast
    from test_span_host import clip_shapes, shape_vertices, sweep_inputs, walker_records
    mesh, keys, phase, mset, d = spanned[name]
    P = 3
    dirs, fire, motion, _, _ = sweep_inputs(N, P)
    rec = walker_records(P)
    sa, sb = clip_shapes(len(keys), P, phase)
    sa, sb = sa[:, None, :], sb[:, None, :]
    assert len({sa[p].tobytes() + sb[p].tobytes() for p in range(P)}) == P
    model = msn.model_of()
    scene = world.scenes["quantised"]
    clean = span_sweeps_dev(scene, mset, motion, dirs, fire, rec, sa, sb, 2.2, None)
    parts = []
    for p in range(P):
        d.span(sa[p, 0], sb[p, 0])
        torch.cuda.synchronize()
        parts.append(sweeps_dev(scene, mset, motion[p:p + 1], dirs, fire, rec[p:p + 1], 2.2))
    for a in ALL:
        assert_bit_equal(clean[a], np.concatenate([q[a] for q in parts]), f"{name}, noise=None: {a}")
    wants, keeps = [], []
    for p in range(P):
        va, vb = shape_vertices(keys, sa[p, 0]), shape_vertices(keys, sb[p, 0])
        cast = lambda rays, fk, va=va, vb=vb: sp.fraction_cast(fresh_cast(world.ctx, mesh), va, vb, fk)(rays)
        want, _, info = msn.scan(world.static, [cast], motion[p:p + 1], dirs, fire, rec[p:p + 1], model.at_frame(model.first_frame + p),
                                 2.2, tab=world.tab, per_ray=(0,))
        wants.append(want)
        keeps.append(info["keep"])
    want = {a: np.concatenate([w[a] for w in wants]) for a in wants[0]}
    keep = np.concatenate(keeps)
    per_sweep = [int((want["mover"][p * N:(p + 1) * N] == 1).sum()) for p in range(P)]
    dropped = int(((clean["mover"] == 1) & ~keep).sum())
    print(f"\n[mover sweep noise] {name}, N {N}: the animated mover wins {per_sweep} rays per sweep, {dropped} of its clean rays are dropped")
    assert min(per_sweep) >= 5 and dropped >= 1
    assert np.isinf(want["t"][~keep]).all() and not want["mover"][~keep].any()
    got = span_sweeps_dev(scene, mset, motion, dirs, fire, rec, sa, sb, 2.2, model)
    assert_records(got, want, f"{name}, N {N}")


def test_deforming_sweep_frames_under_noise(engine, world, spanned):
    """scan_deforming_sweep_frames(..., noise=...) stacks the runs of scan_deforming_sweeps_dev; noise=None stays as it was"""
    from helpers import aimed_pose, sensor_small
    from lidar import IndoorLidar
    from lidarcast import deform
    from test_mover_sweeps_gpu import TARGET
    from test_span_host import clip_shapes, walker_records
    mesh, keys, phase, mset, d = spanned["walker"]
    k = sensor_small(lines=4, width=64, max_range=6.0)
    start = np.stack([aimed_pose(TARGET, 1.5, yaw=y) for y in (0.3, -1.0, 2.2)])
    end = start.copy()
    end[:, :3, 3] += (0.08, -0.09, 0.02)
    rec, model = walker_records(3), msn.model_of()
    sa, sb = clip_shapes(len(keys), 3, phase)
    sa, sb = sa[:, None, :], sb[:, None, :]
    motion, fire, T = engine.sweep_inputs(k, start, end)
    dirs = np.ascontiguousarray(IndoorLidar(k, np.eye(4)).sensor_directions(), dtype=np.float64)
    scene = engine.scene_for(world.room)
    for noise in (model, None):
        fr = deform.scan_deforming_sweep_frames(engine, k, start, end, world.room, mset, rec, sa, sb,
                                                want=("point3", "sem", "ins", "index"), noise=noise)
        dev = span_sweeps_dev(scene, mset, motion, dirs, fire, rec, sa, sb, k.max_range, noise)
        keep = dev["t"] != np.inf
        assert fr["total"] == int(keep.sum()) == len(fr["point_times"]) and (fr["mover"] == 1).sum() > 10
        for a in ("point3", "sem", "ins", "mover"):
            assert_bit_equal(fr[a], dev[a][keep], f"deforming frames, noise {noise is not None}: {a}")
        assert np.array_equal(fr["point_times"], fire[fr["index"]] * T)


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals(engine, world):
    import torch
    import lidarcast
    from lidarcast import DeviceHits, _capi
    from lidarcast.movers import MoverSet, scan_noisy_mover_sweeps_compact, scan_noisy_mover_sweeps_dev
    from lidarcast.noise import NoiseModel
    lib = _capi.load()
    E = _capi.LRC_ERR_INVALID_ARG
    dirs, fire, _, motion, _, _ = inputs(200, 3)
    P, N = 3, 200
    scene, mset, rec, model = world.scenes["quantised"], world.sets["quantised"][1], mover_records(3, 1), msn.model_of()
    mt, dt, ft, rt = tensors(motion, dirs, fire, rec)
    torch.cuda.synchronize()
    before = scene.counters(), mset.scenes[0].counters()
    dev, compact = "lrc_scan_noisy_mover_sweeps_dev: ", "lrc_scan_noisy_mover_sweeps_compact: "

    def hits_t():
        return DeviceHits(P * N, "cuda", want=("t",))

    table, bare = lidarcast.DirectionTable(engine.ctx, dirs, fire), lidarcast.DirectionTable(engine.ctx, dirs)

    # the model: what lrc_scan_noisy_sweeps_dev refuses, with and without a set, in an empty call too
    for bad, what in ((dict(range_std=-0.01), "range_std must be finite and not negative"), (dict(range_std=np.inf), "range_std"),
                      (dict(range_std=np.nan), "range_std"), (dict(angle_std=-1e-9), "angle_std must be finite and not negative"),
                      (dict(angle_std=np.nan), "angle_std"), (dict(dropout=1.0), r"dropout must lie in \[0, 1\)"),
                      (dict(dropout=-0.1), "dropout"), (dict(dropout=np.nan), "dropout")):
        m = dataclasses.replace(model, **bad)
        with pytest.raises(ValueError, match=dev + what):
            scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits_t(), 20.0, mset, rt, m)
        with pytest.raises(ValueError, match=compact + what):
            scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, mset, rec, m)
        with pytest.raises(ValueError, match=dev + what):
            scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits_t(), 20.0, None, None, m)
        with pytest.raises(ValueError, match=compact + what):
            scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, None, None, m)
        bad_nz, fr0, total = m.struct(), _capi.LrcFrames(), C.c_uint64(0)          # an empty call: the model is checked all the same
        assert lib.lrc_scan_noisy_mover_sweeps_compact(scene._h, None, None, 0, table._h, None, 20.0, C.byref(bad_nz), C.byref(fr0),
                                                       None, 0, C.byref(total)) == E
        assert compact.encode() in lib.lrc_last_error()
    nz, hits = model.struct(), hits_t()
    args = (mt.data_ptr(), P, dt.data_ptr(), ft.data_ptr(), N, rt.data_ptr(), 20.0)
    assert lib.lrc_scan_noisy_mover_sweeps_dev(scene._h, mset._h, *args, None, C.byref(hits.struct), None, None) == E
    assert dev.encode() + b"noise is NULL" in lib.lrc_last_error()
    assert lib.lrc_scan_noisy_mover_sweeps_dev(scene._h, mset._h, mt.data_ptr(), 1, dt.data_ptr(), ft.data_ptr(), 2 ** 32, rt.data_ptr(),
                                               20.0, C.byref(nz), C.byref(hits.struct), None, None) == E
    assert b"2^32 - 1 rays per pose" in lib.lrc_last_error() and dev.encode() in lib.lrc_last_error()
    for missing in (0, 2, 3):                                             # motion24, dirs3, fire
        a = list(args)
        a[missing] = None
        assert lib.lrc_scan_noisy_mover_sweeps_dev(scene._h, mset._h, *a, C.byref(nz), C.byref(hits.struct), None, None) == E
        assert dev.encode() + b"motion24, dirs3 or fire is NULL" in lib.lrc_last_error()
    a = list(args)
    a[5] = None
    assert lib.lrc_scan_noisy_mover_sweeps_dev(scene._h, mset._h, *a, C.byref(nz), C.byref(hits.struct), None, None) == E
    assert dev.encode() + b"mover_motion24 is NULL" in lib.lrc_last_error()
    noise = torch.zeros(P * N, dtype=torch.float32, device="cuda")
    try:
        scene.set_options(range_noise=(noise.data_ptr(), noise.numel()))
        with pytest.raises(ValueError, match=dev + "a range_noise option is set"):
            scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits_t(), 20.0, mset, rt, model)
        with pytest.raises(ValueError, match=dev + "a range_noise option is set"):
            scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits_t(), 20.0, None, None, model)
        with pytest.raises(ValueError, match=compact + "a range_noise option is set"):
            scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, mset, rec, model)
    finally:
        scene.reset_options()
    # the movers: what lrc_scan_mover_sweeps_* refuse
    h = C.c_void_p()
    arr = (C.c_void_p * 1)(scene._h)
    assert lib.lrc_movers_create(engine.ctx._h, arr, 1, C.byref(h)) == 0
    try:
        assert lib.lrc_scan_noisy_mover_sweeps_dev(scene._h, h, *args, C.byref(nz), C.byref(hits.struct), None, None) == E
        assert dev.encode() + b"the static scene is one of its own movers" in lib.lrc_last_error()
    finally:
        lib.lrc_movers_destroy(h)
    other = lidarcast.Context(0)
    try:
        foreign = MoverSet(other, world.meshes[:1])
        with pytest.raises(ValueError, match="another context"):
            scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits_t(), 20.0, foreign, rt, model)
        assert lib.lrc_scan_noisy_mover_sweeps_dev(scene._h, foreign._h, *args, C.byref(nz), C.byref(hits.struct), None, None) == E
        assert dev.encode() + b"movers and scene belong to different contexts" in lib.lrc_last_error()
        foreign.close()
    finally:
        other.close()
    with pytest.raises(ValueError, match=dev + "tile_count"):
        scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, DeviceHits(P * N, "cuda", want=("t", "tile_count")), 20.0, mset, rt, model)
    # the compact call's host checks: the sensor's records, the mover records, the fire table
    bad = motion.copy()
    bad[1, 5] = np.nan
    with pytest.raises(ValueError, match=compact + "record 1 is not finite"):
        scan_noisy_mover_sweeps_compact(scene, bad, dirs, fire, 20.0, mset, rec, model)
    bad = rec.copy()
    bad[1, 0, 17] = np.inf
    with pytest.raises(ValueError, match=compact + "mover sweep record 1 has an entry that is not finite"):
        scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, mset, bad, model)
    bad = rec.copy()
    bad[2, 0, 0] += np.float32(2.0 ** -12)
    with pytest.raises(ValueError, match=compact + "mover sweep record 2 is no rotation"):
        scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, mset, bad, model)
    bad = rec.copy()
    bad[0, 0, 12:16] = [np.cos(0.8), 0.0, 0.0, np.sin(0.8)]
    with pytest.raises(ValueError, match=compact + "mover sweep record 0 rotates by more than pi/2 per sweep"):
        scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, mset, bad, model)
    fr, total = _capi.LrcFrames(), C.c_uint64(0)                          # a resident table without firing fractions
    assert lib.lrc_scan_noisy_mover_sweeps_compact(scene._h, mset._h, motion.ctypes.data, P, bare._h, rec.ctypes.data, 20.0,
                                                   C.byref(nz), C.byref(fr), None, 0, C.byref(total)) == E
    assert compact.encode() + b"the table has no fire table" in lib.lrc_last_error()
    with pytest.raises(ValueError, match=r"\(P, M, 24\)"):
        scan_noisy_mover_sweeps_compact(scene, motion, dirs, fire, 20.0, mset, rec[:2], model)
    with pytest.raises(ValueError, match="P \\* N records"):
        scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, DeviceHits(P * N + 1, "cuda", want=("t",)), 20.0, mset, rt, model)
    with pytest.raises(ValueError, match="mover_t must be torch.uint8"):
        scan_noisy_mover_sweeps_dev(scene, mt, dt, ft, hits_t(), 20.0, mset, rt, model,
                                    mover_t=torch.zeros(P * N, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert (scene.counters(), mset.scenes[0].counters()) == before                      # every refusal came before any launch
    few = scan_noisy_mover_sweeps_compact(scene, motion, table, None, 20.0, mset, rec, NoiseModel(seed=1, dropout=0.999999))
    assert few["total"] < 10 and scene.counters() != before[0]
    table.close()
    bare.close()


# ---- 8: the simulator end to end ------------------------------------------------------------------------------------------------------

def test_simulator_sensor_noise_entry(engine, world, tmp_path):
    import s3dis_simulator
    from lidarcast.noise import NoiseModel
    from trajectory import line_trajectory
    wps = line_trajectory((1.2, 1.0, 1.0), (3.9, 3.1, 1.0), 3, yaw=0.6)
    key = {"period": 0.1, "per_ray_shape": True, "sensor_noise": {"seed": 7}, "objects": [
        {"mesh": "walker", "semantic": 13, "instance": 1001, "animation": {"cycle": 0.8, "phase": 0.03},
         "path": [[0.0, 1.8, 2.6, 0.0, 20.0], [0.4, 3.3, 1.4, 0.0, 140.0]]},
        {"mesh": "pedestrian", "semantic": "clutter", "instance": 1002, "path": [[0.0, 3.5, 3.0, 0.0, 0.0]]},
        {"mesh": "walker_rig", "semantic": 13, "instance": 1003, "animation": {"cycle": 1.0}, "path": [[0.0, 2.6, 1.2, 0.0, 90.0]]}]}

    def run(movers_key):
        sim = s3dis_simulator.S3DISSimulator({"raycast_engine": {"use_gpu": True}, "motion": {"speed": 0.5, "movers": movers_key}})
        sim.load_scene(world.room, "room")
        return sim, sim.run_simulation(wps)
    sim, one = run(key)
    _, two = run(key)
    _, clean = run({a: b for a, b in key.items() if a != "sensor_noise"})
    assert one.get_total_frames() == 3
    T = 1.0 / sim.lidar_config.scan_frequency
    seen = np.zeros(4, np.int64)
    for a, b, c in zip(one.frames, two.frames, clean.frames):
        ids = a.mover_ids
        assert ids.dtype == np.uint8 and len(ids) == len(a.points) == len(a.point_times) == len(a.semantic_labels) > 0
        assert a.point_times.min() >= 0.0 and a.point_times.max() < T
        seen += np.bincount(ids, minlength=4)
        assert (a.instance_labels[ids == 1] == 1001).all() and (a.instance_labels[ids == 3] == 1003).all()
        assert (a.semantic_labels[ids == 2] == 12).all() and (a.instance_labels[ids == 2] == 1002).all()
        assert a.points.tobytes() == b.points.tobytes() and ids.tobytes() == b.mover_ids.tobytes()        # two runs, the same bytes
        assert a.point_times.tobytes() == b.point_times.tobytes() and a.semantic_labels.tobytes() == b.semantic_labels.tobytes()
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
    assert all("end_shape" in f["movers"][0] and f["sweep_duration"] == T for f in disk["frames"])
    assert sim._mover_plan(nested=True)["noise"] == NoiseModel.from_intrinsics(k, 7, first_frame=0)
    # rigid movers alone take the rigid route
    rigid = dict(key, objects=key["objects"][1:2])
    del rigid["per_ray_shape"]
    _, r1 = run(rigid)
    _, r2 = run(rigid)
    assert all(a.points.tobytes() == b.points.tobytes() and (a.mover_ids == 1).any() for a, b in zip(r1.frames, r2.frames))


# ---- 9: the physical check on the GPU's output ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ROUTES)
def test_points_on_a_moving_box_lie_on_the_box_at_their_own_time(world, route):
    from lidarcast.movers import MoverTrack, sweep_records
    k, dirs, fire, motion, path = ms.crossing_inputs()
    rec = sweep_records([MoverTrack(path)], [0.0], [ms.SWEEP_T])
    model = msn.model_of(range_std=0.0)
    scene, mset = world.scenes[route], world.sets[route][1]
    clean = sweeps_dev(scene, mset, motion, dirs, fire, rec, k.max_range)
    got = noisy_sweeps_dev(scene, mset, motion, dirs, fire, rec, model, k.max_range)
    on = got["mover"] == 1
    dropped = int(((clean["mover"] == 1) & np.isinf(got["t"])).sum())
    s = fire[np.flatnonzero(on) % len(dirs)]
    own = ms.box_distance(got["point3"][on], s, rec[0, 0])
    frozen = ms.box_distance(got["point3"][on], np.zeros(int(on.sum())), rec[0, 0])
    print(f"\n[mover sweep noise] GPU, {route} nodes: {int(on.sum())} of {len(on)} rays end on the box ({dropped} of the clean sweep's "
          f"{int((clean['mover'] == 1).sum())} are gone); by the pose at their own time they lie within {own.max():.3e} m of its "
          f"surface (bound {BOUND_ON_BOX:.3e} m), by the sweep-start pose within {frozen.max():.3f} m")
    assert on.sum() >= 50 and dropped >= 1
    assert own.max() <= BOUND_ON_BOX
    assert frozen.max() > 0.1
