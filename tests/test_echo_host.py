"""CPU: the host side of the beam footprint and multi-echo returns (lrc_echo_reduce, the argument checks of lrc_scan_echoes_*,
lidarcast.echo.BeamModel).  The reduction is compared with the numpy restatement of the header's text (tests/echo_restate.py)
on crafted rows -- ties, gaps of exactly the separation and one ulp above it, chains, misses, more clusters than echoes, small
clusters dropped: the rows of tests/echo_rows.py, which the device reduction gets too (tests/test_echo_lanes_gpu.py) -- and on
random rows."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import echo_restate as er
import echo_rows as rows
from conftest import REPO

INF = np.float32(np.inf)


def _beam(K, E=2, min_count=1, separation=0.05):
    from lidarcast._capi import LrcBeam
    b = LrcBeam()
    b.subrays, b.max_echoes, b.min_count, b.separation = K, E, min_count, separation
    return b


def _both(t, E=2, min_count=1, separation=0.05):
    from lidarcast import echo
    t = np.asarray(t, dtype=np.float32)
    got = echo.reduce(t, _beam(t.shape[1], E, min_count, separation))
    want = er.reduce_rows(t, E, min_count, np.float32(separation))
    assert got[0].tolist() == want[0].tolist(), (t, got, want)
    assert got[1].tolist() == want[1].tolist(), (t, got, want)
    return got


def _crafted(group):
    """Every row of the group through both reductions, each against the result tests/echo_rows.py records for it."""
    cases = rows.crafted(group)
    for c in cases:
        rep, w = _both(c.t, E=c.E, min_count=c.min_count, separation=c.separation)
        assert rep.tolist() == c.rep and w.tolist() == c.weight, c
    return cases


def test_exact_ties_are_broken_by_k():
    a, b = _crafted("ties")
    assert (a.rep, a.weight) == ([[1, 0]], [[3, 2]])
    assert (b.rep, b.weight) == ([[0, -1, -1]], [[3, 0, 0]])


def test_gap_of_exactly_the_separation_and_one_ulp_above():
    sep, a, b, b1 = rows.SEP, rows.A, rows.B, rows.B1
    assert sep == np.float32(0.25) and a == np.float32(1.0) and b == a + sep          # exact in float32
    assert np.float32(b - a) == sep
    assert b1 == np.nextafter(b, INF) and np.float32(b1 - a) > sep
    eq, above, back = _crafted("separation")
    assert eq.t.tolist() == [[a, b, INF]] and above.t.tolist() == [[a, b1, INF]] and back.t.tolist() == [[b1, a, INF]]
    assert eq.separation == above.separation == back.separation == sep
    assert (eq.rep, eq.weight) == ([[0, -1]], [[2, 0]])              # a gap equal to the separation does not split
    assert (above.rep, above.weight) == ([[0, 1]], [[1, 1]])
    assert (back.rep, back.weight) == ([[1, 0]], [[1, 1]])           # the same two the other way round


def test_a_chain_of_small_gaps_is_one_cluster():
    t = np.float32(1.0) + np.arange(7, dtype=np.float32) * np.float32(0.04)     # 0.24 m end to end, separation 0.05
    down, mixed = _crafted("chain")
    assert down.t.tolist() == [t[::-1].tolist()] and mixed.t.tolist() == [t[[3, 0, 6, 1, 5, 2, 4]].tolist()]
    for c in (down, mixed):
        assert (c.rep, c.weight, c.E, float(c.separation)) == ([[0, -1]], [[7, 0]], 2, float(np.float32(0.05)))


def test_all_misses_and_axis_miss_with_off_axis_hits():
    miss, axis = _crafted("misses")
    assert miss.t.tolist() == [[INF] * 5] and (miss.rep, miss.weight) == ([[-1, -1]], [[0, 0]])
    assert axis.t.tolist() == np.array([[INF, 3.0, INF, 1.0, 3.01]], np.float32).tolist()
    assert (axis.rep, axis.weight) == ([[3, 1]], [[1, 2]])


def test_more_clusters_than_echoes_keeps_the_nearest():
    two, four, one = _crafted("more_clusters")
    t = np.array([[4.0, 1.0, 3.0, 2.0, 1.01, INF, 3.0]], np.float32).tolist()
    assert two.t.tolist() == four.t.tolist() == one.t.tolist() == t and (two.E, four.E, one.E) == (2, 4, 1)
    assert (two.rep, two.weight) == ([[1, 3]], [[2, 1]])
    assert (four.rep, four.weight) == ([[1, 3, 2, 0]], [[2, 1, 2, 1]])
    assert (one.rep, one.weight) == ([[1]], [[2]])


def test_min_count_drops_the_nearest_cluster():
    mc2, mc3 = _crafted("min_count")
    t = np.array([[1.0, 2.0, 2.01, 3.0, 3.0, 3.0, 5.0]], np.float32).tolist()
    assert mc2.t.tolist() == mc3.t.tolist() == t and (mc2.min_count, mc3.min_count, mc2.E, mc3.E) == (2, 3, 2, 2)
    assert (mc2.rep, mc2.weight) == ([[1, 3]], [[2, 3]])
    assert (mc3.rep, mc3.weight) == ([[3, -1]], [[3, 0]])


@pytest.mark.parametrize("K", [1, 3, 5, 7, 16])
def test_random_rows_against_the_restatement(K):
    rng = np.random.default_rng(100 + K)
    B = 400
    # a few surfaces per beam, sub-rays spread around them at the scale of the separation; a quarter miss
    base = rng.uniform(0.5, 3.0, (B, 3)).astype(np.float32)
    t = (base[np.arange(B)[:, None], rng.integers(0, 3, (B, K))] + rng.normal(0, 0.03, (B, K))).astype(np.float32)
    t[rng.random((B, K)) < 0.25] = INF
    t[rng.random((B, K)) < 0.1] = np.float32(1.5)                  # exact ties
    t[:5] = INF
    for E in (1, 2, 3, 4):
        for mc in sorted({1, min(2, K), K}):
            rep, w = _both(t, E=E, min_count=mc)
            assert ((rep >= 0) == (w > 0)).all()
            assert (w <= K).all() and (w[rep >= 0] >= mc).all()


def test_refusals_of_the_beam():
    from lidarcast import _capi, echo
    lib = _capi.load()
    t = np.zeros((1, 16), np.float32)
    rep, w = np.zeros((1, 8), np.int32), np.zeros((1, 8), np.uint8)
    bad = [dict(K=0), dict(K=17), dict(E=0), dict(E=5), dict(min_count=0), dict(K=3, min_count=4),
           dict(separation=0.0), dict(separation=-1.0), dict(separation=float("inf")), dict(separation=float("nan"))]
    for kw in bad:
        b = _beam(**{"K": 3, **kw})
        assert lib.lrc_echo_reduce(t.ctypes.data, 1, C.byref(b), rep.ctypes.data, w.ctypes.data) == _capi.LRC_ERR_INVALID_ARG, kw
        with pytest.raises(ValueError, match="lrc_echo_reduce"):
            echo.reduce(t[:, :max(1, min(b.subrays, 16))], b)
        # the scans check the beam before they look at the scene
        hits = _capi.LrcHits()
        assert lib.lrc_scan_echoes_dev(None, None, 0, None, 0, None, C.byref(b), 1.0, C.byref(hits), None, None) == _capi.LRC_ERR_INVALID_ARG
        assert b"lrc_scan_echoes_dev" in lib.lrc_last_error() and b"scene" not in lib.lrc_last_error(), kw
        fr = _capi.LrcFrames()
        off = np.zeros((16, 2))
        assert lib.lrc_scan_echoes_compact(None, None, 0, None, off.ctypes.data, C.byref(b), 1.0, C.byref(fr), None, 0, None) == _capi.LRC_ERR_INVALID_ARG
        assert b"lrc_scan_echoes_compact" in lib.lrc_last_error() and b"scene" not in lib.lrc_last_error(), kw
    assert lib.lrc_echo_reduce(t.ctypes.data, 1, None, rep.ctypes.data, w.ctypes.data) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_echo_reduce(None, 1, C.byref(_beam(3)), rep.ctypes.data, w.ctypes.data) == _capi.LRC_ERR_INVALID_ARG
    assert lib.lrc_echo_reduce(None, 0, C.byref(_beam(3)), None, None) == 0


def test_symbols_load():
    from lidarcast import _capi
    lib = _capi.load()
    for name in ("lrc_scan_echoes_dev", "lrc_scan_echoes_compact", "lrc_echo_reduce"):
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
    assert "lrc_internal_echo_lanes_dev" in _capi.INTERNAL_SYMBOLS and hasattr(lib, "lrc_internal_echo_lanes_dev")
    b = _beam(0)                                   # the device hook checks the beam first, as lrc_echo_reduce does: no GPU needed
    assert lib.lrc_internal_echo_lanes_dev(None, None, 0, C.byref(b), None, None, None, None, None) == _capi.LRC_ERR_INVALID_ARG
    assert b"lrc_internal_echo_lanes_dev: subrays" in lib.lrc_last_error()
    assert lib.lrc_internal_echo_lanes_dev(None, None, 0, C.byref(_beam(3)), None, None, None, None, None) == _capi.LRC_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.lrc_last_error()


def test_refusals_that_need_no_scene():
    from lidarcast import _capi
    lib = _capi.load()
    b = _beam(3)
    fr = _capi.LrcFrames()
    for bad in (np.nan, np.inf, -np.inf):
        off = np.zeros((3, 2))
        off[2, 1] = bad
        assert lib.lrc_scan_echoes_compact(None, None, 0, None, off.ctypes.data, C.byref(b), 1.0, C.byref(fr), None, 0, None) == _capi.LRC_ERR_INVALID_ARG
        assert b"non-finite offset" in lib.lrc_last_error()
    hits = _capi.LrcHits()
    word = (C.c_uint32 * 1)()
    hits.tile_count = C.addressof(word)
    assert lib.lrc_scan_echoes_dev(None, None, 0, None, 0, None, C.byref(b), 1.0, C.byref(hits), None, None) == _capi.LRC_ERR_INVALID_ARG
    assert b"tile_count" in lib.lrc_last_error()


def test_beam_model_patterns():
    from lidarcast.echo import BeamModel
    div = 3e-3
    r = div / (2.0 * math.sqrt(2.0))
    for name, K, step in (("single", 1, None), ("cross5", 5, 90.0), ("hex7", 7, 60.0)):
        m = BeamModel(div, pattern=name)
        assert m.subrays == K and m.offsets.shape == (K, 2) and m.offsets.dtype == np.float64
        assert m.offsets[0].tolist() == [0.0, 0.0]                                    # the axis comes first
        if K > 1:
            ring = m.offsets[1:]
            assert np.allclose(np.hypot(ring[:, 0], ring[:, 1]), r, rtol=1e-15, atol=0)
            ang = np.degrees(np.arctan2(ring[:, 1], ring[:, 0])) % 360.0
            assert np.allclose(ang, np.arange(K - 1) * step, atol=1e-9)
    assert BeamModel(div).pattern == "hex7" and BeamModel(div).max_echoes == 2 and BeamModel(div).separation == 0.05
    m = BeamModel(div, pattern=[[0, 0], [1e-3, 0], [0, -1e-3]], max_echoes=3, min_fraction=0.5)
    assert m.subrays == 3 and m.min_count == 2 and m.struct().max_echoes == 3
    assert BeamModel(div, min_fraction=0.0).min_count == 1 and BeamModel(div, min_fraction=1.0).min_count == 7
    assert BeamModel(div, "cross5", min_fraction=0.41).min_count == 3
    for kw in (dict(pattern="ring9"), dict(pattern=np.zeros((17, 2))), dict(pattern=np.zeros((0, 2))), dict(pattern=np.zeros((3, 3))),
               dict(pattern=[[0, 0], [np.nan, 0]]), dict(max_echoes=0), dict(max_echoes=5), dict(separation=0.0),
               dict(separation=np.inf), dict(min_fraction=1.5), dict(min_fraction=-0.1)):
        with pytest.raises(ValueError):
            BeamModel(div, **kw)
    with pytest.raises(ValueError):
        BeamModel(np.nan)
    rep, w = BeamModel(div, "cross5").reduce(np.array([[1.0, 1.01, np.inf, 2.0, 2.0]], np.float32))
    assert rep.tolist() == [[0, 3]] and w.tolist() == [[2, 2]]


def test_struct_layout_matches_header():
    from lidarcast._capi import LrcBeam
    src = open(os.path.join(REPO, "include", "lidarcast.h")).read()
    body = re.search(r"typedef struct lrc_beam \{(.*?)\} lrc_beam;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)\s*$", d).group(1) for d in decls]
    assert [n for n, _ in LrcBeam._fields_] == names == ["subrays", "max_echoes", "min_count", "separation"]
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [t for _, t in LrcBeam._fields_] == [ctype[d.split()[0]] for d in decls]
    assert C.sizeof(LrcBeam) == 16


def test_simulator_beam_key_refusals():
    """What needs no engine: the key's own entries, and the exporters that would scan without the beam.  (The combinations
    run_simulation refuses need an engine: tests/test_echo_gpu.py.)"""
    import s3dis_simulator
    from lidarcast.echo import BeamModel

    def sim_with(config):
        sim = s3dis_simulator.S3DISSimulator.__new__(s3dis_simulator.S3DISSimulator)      # no engine is built
        sim.config = config
        sim.scene = object()
        return sim
    assert sim_with({})._beam_model() is None
    m = sim_with({"beam": {"divergence_mrad": 3.0}})._beam_model()
    assert isinstance(m, BeamModel) and m.divergence == 3.0e-3 and m.pattern == "hex7" and m.max_echoes == 2
    m = sim_with({"beam": {"divergence_mrad": 2.0, "pattern": "cross5", "max_echoes": 3, "separation": 0.1, "min_fraction": 0.4}})._beam_model()
    assert (m.subrays, m.max_echoes, m.separation, m.min_count) == (5, 3, 0.1, 2)
    with pytest.raises(ValueError, match="unknown entries under the beam key"):
        sim_with({"beam": {"divergence_mrad": 3.0, "divergence": 0.003}})._beam_model()
    with pytest.raises(ValueError, match="divergence_mrad"):
        sim_with({"beam": {"pattern": "hex7"}})._beam_model()
    with pytest.raises(ValueError):
        sim_with({"beam": {"divergence_mrad": 3.0, "pattern": "ring9"}})._beam_model()
    with pytest.raises(ValueError):
        sim_with({"beam": {"divergence_mrad": 3.0, "max_echoes": 5}})._beam_model()
    sim = sim_with({"beam": {"divergence_mrad": 3.0}})
    for export in (lambda: sim.evaluate_surface_coverage([]), lambda: sim.export_occupancy_grid([], "unused"),
                   lambda: sim.export_frame_annotations([], "unused")):
        with pytest.raises(NotImplementedError, match="beam key"):
            export()
